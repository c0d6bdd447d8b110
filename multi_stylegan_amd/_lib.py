"""ctypes binding of libmsg_hip.so (C ABI: include/msg_hip.h).

Nothing about that ABI is written down here: every entry point's signature, the status / storage / kernel-plan codes and
the ABI version are parsed from the header at import (``_parse_header``), and the generated call wrappers
(csrc_host/gen_fastcall.py) are built from the same parse.  A new entry point is declared in the header and nowhere else.

There is no CPU fallback: if the shared library is missing or a call reports
an error this raises.  Tensors are passed as raw device pointers together with
the HIP stream torch is currently recording on, so launches interleave
correctly with torch's own kernels.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSG_LIB_VARIANT=<tag> loads libmsg_hip_<tag>.so instead: an experimental or diagnostic build kept beside the library for
# same-box A/B timing (tools/microbench.py, tools/row3_stamps.py); never set in tests or in the benchmark
LIB_PATH = os.path.join(_HERE, "libmsg_hip" + ("_" + os.environ["MSG_LIB_VARIANT"] if os.environ.get("MSG_LIB_VARIANT") else "")
                        + ".so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "msg_hip.h")

_P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
_BY_VALUE = {"int": _I, "long long": _L, "float": _F}


class MsgHipError(RuntimeError):
    pass


def _parse_header(text):
    """The C ABI as include/msg_hip.h declares it -> ({entry point: (restype, [argtypes])}, {constant: int}): every
    prototype ``RET msg_name(ARGS);``, every enumerator of the anonymous enums and ``#define MSG_ABI_VERSION n``.  The type
    map is closed -- any pointer argument is a void*, a ``const char*`` result a char*, ``int`` / ``long long`` / ``float``
    themselves -- and anything else raises, naming the entry: a type this binding cannot pass is never skipped or guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(MSG_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^{}]*)\}", text):
        for item in filter(str.strip, body.split(",")):
            m = re.fullmatch(r"\s*(MSG_\w+)\s*=\s*(-?\d+)\s*", item)
            if not m:
                raise MsgHipError(f"{HEADER_PATH}: enumerator {item.strip()!r} is not `MSG_NAME = integer`")
            consts[m[1]] = int(m[2])

    def words(decl):
        return " ".join(decl.replace("*", " * ").split())

    sigs = {}
    for ret, name, args in re.findall(r"\b([A-Za-z_][\w\s*]*?)\b(msg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        res = ctypes.c_char_p if words(ret) == "const char *" else _BY_VALUE.get(words(ret))
        argtypes = []
        for arg in ([] if words(args) == "void" else args.split(",")):
            by_value = re.fullmatch(r"(int|long long|float) \w+", words(arg))
            argtypes.append(_P if "*" in arg else by_value and _BY_VALUE[by_value[1]])
        if res is None or None in argtypes or name in sigs:
            raise MsgHipError(f"{HEADER_PATH}: `{words(ret)} {name}({words(args)})` has a type the binding cannot pass "
                              "(arguments: pointers, int, long long, float, each with a name; results: int, long long, "
                              "const char*) or is declared twice")
        sigs[name] = (res, argtypes)
    loose = re.findall(r"\b(msg_[a-z0-9_]+)\s*\(", text)
    if len(loose) != len(sigs):
        raise MsgHipError(f"{HEADER_PATH}: not a prototype this binding can read (`RET msg_name(ARGS);`, no nested "
                          f"parentheses): {sorted(set(loose) - set(sigs)) or 'an entry declared twice'}")
    return sigs, consts


with open(HEADER_PATH) as _f:
    _SIGNATURES, _CONSTANTS = _parse_header(_f.read())
# the header's constants by their own names: MSG_OK / MSG_EINVAL / MSG_EUNSUPPORTED / MSG_ELAUNCH, the storage codes MSG_F32 /
# MSG_BF16 / MSG_F16 / MSG_F64 / MSG_F32_SPLIT, the kernel plans MSG_PLAN_*, MSG_ABI_VERSION
globals().update(_CONSTANTS)
ABI_VERSION = _CONSTANTS["MSG_ABI_VERSION"]       # compared with the loaded library's msg_abi_version() in lib()


def declared_symbols():
    """Every function the public header declares (used by the CPU-side export test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(msg_[a-z0-9_]+)\s*\(", text)))


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MsgHipError(f"{LIB_PATH} is missing: build it with `python -m multi_stylegan_amd.build` "
                              "(hipcc, --offload-arch=gfx950). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        handle.msg_abi_version.restype = _I
        found = handle.msg_abi_version()
        if found != ABI_VERSION:
            # (a stale .so used to surface as an AttributeError on the first missing symbol -- or not at all, when only a
            #  workspace size had changed)
            raise MsgHipError(f"{LIB_PATH} was built for C-ABI version {found}, this package binds version {ABI_VERSION}: "
                              "rebuild the library with `python -m multi_stylegan_amd.build --force`")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = _with_fastcall(handle)
    return _lib


class _Entries:
    """What ``lib()`` hands out: every entry point of the C ABI as an attribute -- the generated argument-vector wrapper
    (multi_stylegan_amd._msg_fastcall, csrc_host/gen_fastcall.py) where there is one, the ctypes function otherwise."""

    def __init__(self, handle, fast):
        self._ctypes, self.fastcall = handle, fast is not None
        for name in _SIGNATURES:
            setattr(self, name, getattr(fast, name, None) or getattr(handle, name))

    def __getattr__(self, name):                    # (anything else the library exports: resolved by ctypes on first use)
        return getattr(self._ctypes, name)


def _with_fastcall(handle):
    """ctypes boxes and converts every argument of a call (2.3-2.5 us per 24-argument launch); the generated wrappers read the
    Python ints / floats straight off the argument vector and call the SAME symbols of the SAME dlopen handle.  Optional:
    MSG_NO_FASTCALL=1 or a missing module (an interpreter the build did not see) leaves the ctypes binding in place."""
    if os.environ.get("MSG_NO_FASTCALL"):
        return _Entries(handle, None)
    try:
        from . import _msg_fastcall as fast
    except ImportError:
        return _Entries(handle, None)
    bound = fast.bind(handle._handle)
    want = sum(1 for res, args in _SIGNATURES.values() if res in (_I, _L))
    if bound != want:
        raise MsgHipError(f"_msg_fastcall resolved {bound} of {want} entry points of {LIB_PATH}: rebuild with "
                          "`python -m multi_stylegan_amd.build --force`")
    return _Entries(handle, fast)


def check(code, what):
    if code != 0:
        raise MsgHipError(f"{what}: {lib().msg_strerror(code).decode()} (code {code})")


def dtype_code(t: torch.Tensor, allow_half: bool = False, allow_double: bool = False) -> int:
    """MSG_* storage code of a tensor.  float16 only where `allow_half`, float64 only where `allow_double` (the FIR /
    activation entries that replace the reference's CUDA modules, which dispatch float / double / half:
    upfirdn2d_kernel.cu:225)."""
    if t.dtype == torch.float32:
        return MSG_F32
    if t.dtype == torch.bfloat16:
        return MSG_BF16
    if allow_half and t.dtype == torch.float16:
        return MSG_F16
    if allow_double and t.dtype == torch.float64:
        return MSG_F64
    raise MsgHipError(f"dtype {t.dtype} is not supported by the gfx950 kernels (float32 / bfloat16"
                      f"{' / float16' if allow_half else ''} only)")


def require_gpu(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise MsgHipError("multi_stylegan_amd ops need tensors on an MI355X (ROCm 'cuda' device); "
                              "got a CPU tensor and there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise MsgHipError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def ptr(t):
    return None if t is None else t.data_ptr()


def stream_of(device) -> int:
    """Raw hipStream_t of torch's current stream on `device` (the fast accessor: no Stream object is built)."""
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on_device(device):
    """Context that makes `device` current for the launch.  One process drives one GPU, so the device is already
    current in practice and the guard costs one integer comparison instead of two hipSetDevice round trips."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


_SCRATCH: dict = {}


def scratch_ptr(nfloats: int, device) -> int:
    """Device pointer of at least `nfloats` fp32 words of launch-scoped workspace (per-tile partial sums, K-slice slabs): ONE
    buffer per (device, stream), grown on demand and reused by every launch.  Sound because a workspace lives from a
    kernel to its reduce launch, both enqueued by the same call on the same stream, and the next user is ordered behind them on
    that stream; a fresh torch.empty per launch was ~1.5 us of host time x ~300 launches per iteration.  (A buffer that was
    outgrown stays alive until the process ends: launches already enqueued may still be reading it.)"""
    if nfloats <= 0:
        return 0
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream_of(device))
    bufs = _SCRATCH.get(key)
    if bufs is None or bufs[-1].numel() < nfloats:
        grown = torch.empty(max(int(nfloats), 1 << 20, 2 * (bufs[-1].numel() if bufs else 0)), dtype=torch.float32, device=device)
        bufs = (bufs or []) + [grown]
        _SCRATCH[key] = bufs
    return bufs[-1].data_ptr()


class KernelClock:
    """Optional per-launch timing with HIP events on the stream the kernels are launched on (bench.py's roofline
    leg).  Off by default: when off, ``span`` is a no-op and costs one attribute test."""

    def __init__(self):
        self.enabled = False
        self.only = None
        self.spans = {}

    def reset(self, enabled: bool, only=None):
        """only: tuple of key prefixes to time (None = every launch; two events per timed launch cost host time)."""
        self.enabled, self.spans, self.only = enabled, {}, (tuple(only) if only else None)

    def span(self, key, work: float):
        """``key``: the timing label, or a tuple of its '/'-separated parts -- joined only when the clock is on, so that a
        disabled clock costs the launch sites one attribute test and no string formatting."""
        if not self.enabled:
            return _NULL_SPAN
        if not isinstance(key, str):
            key = "/".join("".join(map(str, part)) if isinstance(part, tuple) else str(part) for part in key)
        if self.only is not None and not key.startswith(self.only):
            return _NULL_SPAN
        return _Span(self, key, work)

    def summary(self):
        """-> {key: dict(launches, total_ms, avg_us, work)}; call after torch.cuda.synchronize()."""
        out = {}
        for key, items in self.spans.items():
            total_ms = sum(a.elapsed_time(b) for a, b, _ in items)
            work = sum(w for _, _, w in items)
            out[key] = {"launches": len(items), "total_ms": total_ms, "avg_us": 1e3 * total_ms / len(items),
                        "work": work}
        return out


class _Span:
    __slots__ = ("clock", "key", "work", "start")

    def __init__(self, clock, key, work):
        self.clock, self.key, self.work = clock, key, work

    def __enter__(self):
        self.start = torch.cuda.Event(enable_timing=True)
        self.start.record()

    def __exit__(self, *exc):
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        self.clock.spans.setdefault(self.key, []).append((self.start, end, self.work))
        return False


class _NullSpan:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NULL_SPAN = _NullSpan()
kernel_clock = KernelClock()
