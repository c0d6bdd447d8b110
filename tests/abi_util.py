"""Shared by the modules that call the C ABI (include/msg_hip.h) directly -- tests/test_hip_modulate.py, tests/test_hip_linear.py:
guarded outputs, operands off their natural alignment, the pointer and stream arguments."""
import math

import torch

DEV = "cuda:0"
SENTINEL = 1536.0                       # exact in bfloat16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _shifted(t):
    """The same values 4 bytes off a 16-byte boundary -> (tensor that owns the memory, pointer)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    return buf, buf.data_ptr() + t.element_size()


class Guarded:
    """An output of `shape`, NaN everywhere (0x7FC0 in bf16), with one more row of `row` sentinel values behind it."""

    def __init__(self, shape, row, dtype=torch.float32):
        self.shape, self.n = tuple(shape), math.prod(shape)
        self.buf = torch.full((self.n + row,), float("nan"), dtype=dtype, device=DEV)
        self.buf[self.n:] = SENTINEL
        self.ptr = self.buf.data_ptr()

    def _host(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[self.n:] == SENTINEL).all()), "the guard row behind the output was written"
        return host[:self.n]

    def read(self):
        """The output in float64 on the host: every element written, the guard untouched."""
        out = self._host()
        left = int(torch.isnan(out).sum())
        assert left == 0, f"{left} of {self.n} output elements were not written"
        return out.double().reshape(self.shape)

    def assert_untouched(self):
        assert bool(torch.isnan(self._host()).all()), "a refused call wrote to its output"
