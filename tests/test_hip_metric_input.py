"""msg_metric_input / validation_metrics.metric_inputs on the GPU (csrc/metric_input.hip) against the float64 statement of
tests/metric_input_util.py: every tile, tap-count and alignment edge of the kernel, the two normalisation orders, the dtypes,
the refusals, and the three metric classes with ``input_size``.

Tolerances (metric_input_util.none_bound / normalised_bound) follow from the arithmetic, not from what the kernel gives: two convex
combinations with weights a few ulp off, then the normalisation's 2 / (hi - lo).  bf16 outputs are held to one bf16 ulp of the
rounded reference (plus the fp32 bound, which decides the rounding of a value next to a tie and is all there is next to zero)."""
import math

import pytest
import torch

import metric_input_util as mu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_H, TILE_W = 16, 64                  # MI_TY, MI_TX of csrc/metric_input.hip: the output tile of one workgroup
PAD = 64                                 # guard bytes on each side (a multiple of 16: the payload keeps its alignment)
NONE, SOURCE, RESIZED = 0, 1, 2
NORM_NAMES = {NONE: None, SOURCE: "source", RESIZED: "resized"}
B, C, T = 2, 3, 3
SIZES = [((16, 16), (16, 16)), ((7, 9), (13, 20)), ((13, 20), (7, 9)), ((20, 12), (5, 9)), ((33, 17), (8, 31)),
         ((64, 16), (8, 16)), ((24, 40), (TILE_H - 1, TILE_W - 1)), ((24, 40), (TILE_H + 1, TILE_W + 1)),
         ((256, 256), (299, 299))]


def _lib():
    from multi_stylegan_amd import _lib
    return _lib


def _code(dtype):
    return {torch.float32: 0, torch.bfloat16: 1}[dtype]


class Region:
    """``nbytes`` of device memory filled with ``fill`` between two runs of 0xA5 guard bytes; ``shift`` moves it off its 16-byte
    alignment.  Every read checks the guards."""

    def __init__(self, nbytes, shift=0, fill=0xFF):
        self.lo, self.n = PAD + shift, nbytes
        self.buf = torch.full((self.lo + nbytes + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.buf[self.lo:self.lo + nbytes] = fill
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    @classmethod
    def of(cls, tensor, shift=0):
        raw = tensor.contiguous().reshape(-1).view(torch.uint8)
        region = cls(raw.numel(), shift)
        region.buf[region.lo:region.lo + region.n] = raw.to(DEV)
        return region

    def bytes(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[:self.lo] == 0xA5).all()) and bool((host[self.lo + self.n:] == 0xA5).all()), "guard bytes were written"
        return host[self.lo:self.lo + self.n].clone()

    def values(self, dtype, shape):
        return self.bytes().view(dtype).reshape(shape)


def call(images, channel, t, size, norm, planes=3, out_dtype=torch.float32, shift_in=False, shift_out=False, ws_fill=0xFF,
         in_dtype_code=None, out_dtype_code=None, null=()):
    """The raw entry on guarded memory -> (status, output on the host or None when refused).  A refused call must leave the
    output's fill bytes alone; an accepted one must leave no element unwritten (the fill is a NaN in both dtypes)."""
    lib = _lib().lib()
    b, c, tn, h, w = images.shape
    frames = tn if t < 0 else 1
    esize = torch.empty((), dtype=out_dtype).element_size()
    src = Region.of(images, images.element_size() if shift_in else 0)
    shape = (b, planes, frames, size[0], size[1])
    out = Region(max(math.prod(shape), 1) * esize if min(shape) > 0 else 64, esize if shift_out else 0)
    nbytes = lib.msg_metric_input_workspace(b, tn, h, w, t, size[0], size[1], norm)
    ws = Region(max(nbytes, 0) + 4, 0, ws_fill)
    status = lib.msg_metric_input(None if "images" in null else src.ptr, _code(images.dtype) if in_dtype_code is None else in_dtype_code,
                                  b, c, tn, h, w, channel, t, None if "out" in null else out.ptr,
                                  _code(out_dtype) if out_dtype_code is None else out_dtype_code, planes, size[0], size[1], norm,
                                  None if "ws" in null or nbytes <= 0 else ws.ptr, torch.cuda.current_stream().cuda_stream)
    src.bytes()
    ws.bytes()
    if status != 0:
        assert bool((out.bytes() == 0xFF).all()), "a refused call wrote to its output"
        return status, None
    return status, out.values(out_dtype, shape)


_INPUTS = {}


def inputs(src, dtype=torch.float32):
    if (src, dtype) not in _INPUTS:
        _INPUTS[src, dtype] = mu.frames(B, C, T, *src, seed=sum(src)).to(dtype)
    return _INPUTS[src, dtype]


_REFERENCES = {}


def reference(src, dtype, channel, t, size, norm):
    key = (src, dtype, channel, t, size, norm)
    if key not in _REFERENCES:
        _REFERENCES[key] = mu.reference(inputs(src, dtype), channel, t, size, NORM_NAMES[norm], planes=1)
    return _REFERENCES[key]


def bounds(src, dtype, channel, t, size, norm):
    """The derived bound per sample (fp32 output)."""
    x = inputs(src, dtype)[:, channel].double()
    x = x if t < 0 else x[:, t:t + 1]
    _, spread = reference(src, dtype, channel, t, size, norm)
    out = []
    for b in range(B):
        peak = float(x[b].abs().max())
        if norm == NONE:
            out.append(mu.none_bound(src, size, peak))
        else:
            assert float(spread[b]) >= 0.1, "the bound's factor 2 / (hi - lo) is held below 20"
            out.append(mu.normalised_bound(src, size, peak, float(spread[b])))
    return out


def check(got, src, dtype, channel, t, size, norm, what=""):
    """``got`` [B, planes, T', oh, ow] (fp32 or bf16, on the host) against the statement: every plane, every sample."""
    want, _ = reference(src, dtype, channel, t, size, norm)
    assert got.shape[0] == B and got.shape[2:] == want.shape[2:]
    assert not bool(got.isnan().any()), "an output element was not written (or is NaN)"
    limit = bounds(src, dtype, channel, t, size, norm)
    worst = 0.0
    for b in range(B):
        for p in range(got.shape[1]):
            g, w = got[b, p].double(), want[b, 0]
            if got.dtype == torch.bfloat16:
                w = w.float().to(torch.bfloat16).double()
                ulp = torch.exp2(torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126))) - 7)
                excess = float(((g - w).abs() - ulp).max())
            else:
                excess = float((g - w).abs().max())
            worst = max(worst, excess / limit[b])
            assert excess <= limit[b], (what, src, size, channel, t, norm, b, p, excess, limit[b])
    print(f"{what} {src}->{size} c={channel} t={t} norm={norm} {got.dtype}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("src,size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_at_every_tile_and_tap_edge(src, size):
    """No normalisation: every channel, t = 0, T - 1 and the whole clip; every (c, t) plane of the input carries its own offset.
    Then the two normalised modes on one selection each."""
    x = inputs(src)
    for channel, t in ((0, 0), (1, T - 1), (2, -1), (1, -1)):
        status, got = call(x, channel, t, size, NONE)
        assert status == 0
        check(got, src, torch.float32, channel, t, size, NONE, "none")
        if src == size:                                                      # equal size: weights (1, 0), a copy bit for bit
            sel = x[:, channel] if t < 0 else x[:, channel, t:t + 1]
            assert torch.equal(got, sel[:, None].expand(-1, 3, -1, -1, -1))
    for norm, channel, t in ((SOURCE, 2, -1), (SOURCE, 0, T - 1), (RESIZED, 1, 0), (RESIZED, 0, -1)):
        status, got = call(x, channel, t, size, norm)
        assert status == 0
        check(got, src, torch.float32, channel, t, size, norm, NORM_NAMES[norm])
        assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0        # a convex filter keeps the range


def test_scale_above_the_cap_is_unsupported():
    L = _lib()
    assert L.MSG_METRIC_MAX_SCALE == 8
    x = inputs((72, 16))
    for norm in (NONE, SOURCE, RESIZED):
        assert call(x, 0, 0, (8, 16), norm) == (L.MSG_EUNSUPPORTED, None)
        assert L.lib().msg_metric_input_workspace(B, T, 72, 16, 0, 8, 16, norm) == -1
    assert call(inputs((16, 72)), 0, -1, (16, 8), NONE) == (L.MSG_EUNSUPPORTED, None)
    assert call(inputs((64, 16)), 0, 0, (8, 16), SOURCE)[0] == 0            # at the cap


@pytest.mark.parametrize("src,size", [((20, 12), (5, 9)), ((24, 40), (16, 48))], ids=["scalar", "vector"])
@pytest.mark.parametrize("norm", [NONE, SOURCE, RESIZED])
def test_modes_planes_and_dtypes(src, size, norm):
    """in / out dtype {f32, bf16}^2, planes 1 and 3.  (24, 40) -> (16, 48): every 16-byte path; (20, 12) -> (5, 9): none of them."""
    for in_dtype in (torch.float32, torch.bfloat16):
        x = inputs(src, in_dtype)                                            # bf16 input: the reference widens the stored values
        for out_dtype in (torch.float32, torch.bfloat16):
            for planes in (1, 3):
                for channel, t in ((1, -1), (2, 1)):
                    status, got = call(x, channel, t, size, norm, planes=planes, out_dtype=out_dtype)
                    assert status == 0 and got.shape[1] == planes
                    check(got, src, in_dtype, channel, t, size, norm, f"{in_dtype}->{out_dtype}")
                    assert all(torch.equal(got[:, 0].view(torch.uint8), got[:, p].view(torch.uint8)) for p in range(planes))


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_normalisation_is_per_sample_and_propagates_nan(in_dtype):
    src, size = (24, 40), (16, 48)
    base = inputs(src, in_dtype)
    for norm, constant, size_k in ((SOURCE, 0.5, size), (RESIZED, 0.0, size), (RESIZED, 0.5, src)):
        # a constant sample: 0 / 0 in all of its outputs.  (Behind a resize only the constant 0 stays constant -- a filter's
        #  weights sum to 1 up to rounding, in the float64 statement too -- and any constant does at equal size, where the
        #  resize is a copy.)
        x = base.clone()
        x[0] = constant
        status, got = call(x, 1, -1, size_k, norm)
        assert status == 0 and bool(got[0].isnan().all())
        want, _ = mu.reference(x[1:], 1, -1, size_k, NORM_NAMES[norm], planes=3)
        limit = mu.normalised_bound(src, size_k, float(x[1, 1].double().abs().max()), _spread(x[1:], 1, size_k, norm))
        assert float((got[1].double() - want[0]).abs().max()) <= limit      # the other sample is untouched
    for norm in (SOURCE, RESIZED):
        x = base.clone()
        x[1, 2, 1, 5, 7] = float("nan")
        status, got = call(x, 2, -1, size, norm)
        assert status == 0 and bool(got[1].isnan().all())                    # one NaN: the whole sample
        want, _ = mu.reference(x[:1], 2, -1, size, NORM_NAMES[norm], planes=3)
        limit = mu.normalised_bound(src, size, float(x[0, 2].double().abs().max()), _spread(x[:1], 2, size, norm))
        assert float((got[0].double() - want[0]).abs().max()) <= limit      # ... and no other
        status, got = call(x, 2, 0, size, norm)                              # the NaN is in time step 1: not selected
        assert status == 0 and not bool(got.isnan().any())


def _spread(x, channel, size, norm):
    spread = float(mu.reference(x, channel, -1, size, NORM_NAMES[norm], planes=1)[1][0])
    assert spread >= 0.1
    return spread


@pytest.mark.parametrize("norm", [NONE, SOURCE, RESIZED])
@pytest.mark.parametrize("in_dtype,out_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                                (torch.float32, torch.bfloat16)], ids=["f32", "bf16", "f32-bf16"])
def test_bits_do_not_depend_on_alignment_workspace_or_run(norm, in_dtype, out_dtype):
    src, size = (24, 40), (16, 48)
    x = inputs(src, in_dtype)
    status, first = call(x, 1, -1, size, norm, out_dtype=out_dtype)
    assert status == 0
    bits = first.view(torch.uint8)
    for kwargs in (dict(), dict(shift_in=True), dict(shift_out=True), dict(shift_in=True, shift_out=True), dict(ws_fill=0x00),
                   dict(ws_fill=0x7F)):
        status, again = call(x, 1, -1, size, norm, out_dtype=out_dtype, **kwargs)
        assert status == 0 and torch.equal(again.view(torch.uint8), bits), kwargs
    # a sample's result does not depend on the rest of the batch
    status, alone = call(x[1:], 1, -1, size, norm, out_dtype=out_dtype)
    assert status == 0 and torch.equal(alone.view(torch.uint8), first[1:].view(torch.uint8))


def test_refusals_launch_nothing():
    L = _lib()
    x = inputs((20, 12))
    size = (5, 9)
    bad = [dict(null=("images",)), dict(null=("out",)), dict(norm=SOURCE, null=("ws",)), dict(norm=RESIZED, null=("ws",)),
           dict(channel=C), dict(channel=-1), dict(t=T), dict(t=-2), dict(planes=0), dict(planes=2), dict(planes=4),
           dict(norm=3), dict(norm=-1), dict(in_dtype_code=2), dict(out_dtype_code=3), dict(in_dtype_code=-1),
           dict(size=(0, 9)), dict(size=(5, 0)), dict(size=(-1, 9))]
    for case in bad:
        kwargs = dict(channel=0, t=0, size=size, norm=NONE)
        kwargs.update(case)
        assert call(x, **kwargs) == (L.MSG_EINVAL, None), case
    lib = L.lib()
    ptr = Region(64).ptr
    for dims in ((0, C, T, 20, 12), (B, 0, T, 20, 12), (B, C, 0, 20, 12), (B, C, T, 0, 12), (B, C, T, 20, 0)):
        assert lib.msg_metric_input(ptr, 0, *dims, 0, -1, ptr, 0, 3, 5, 9, NONE, None, None) == L.MSG_EINVAL, dims
    # counts the block index cannot address: 2^22 x 2^22 output pixels in 2^18 x 2^16 tiles, times two samples
    assert lib.msg_metric_input(ptr, 0, B, C, T, 1 << 22, 1 << 22, 0, 0, ptr, 0, 1, 1 << 22, 1 << 22, NONE, None, None) == L.MSG_EINVAL
    # the workspace query: -1 where the entry refuses, 0 without a normalisation, the pairs' bytes with one
    q = lib.msg_metric_input_workspace
    assert q(B, T, 20, 12, 0, 5, 9, NONE) == 0 and q(B, T, 20, 12, 0, 5, 9, SOURCE) == 8 * B
    assert q(B, T, 256, 256, -1, 299, 299, RESIZED) == 8 * B * T * math.ceil(299 / TILE_H) * math.ceil(299 / TILE_W)
    for args in ((0, T, 20, 12, 0, 5, 9, NONE), (B, 0, 20, 12, 0, 5, 9, NONE), (B, T, 0, 12, 0, 5, 9, NONE), (B, T, 20, 0, 0, 5, 9, NONE),
                 (B, T, 20, 12, T, 5, 9, NONE), (B, T, 20, 12, -2, 5, 9, NONE), (B, T, 20, 12, 0, 0, 9, NONE),
                 (B, T, 20, 12, 0, 5, 0, NONE), (B, T, 20, 12, 0, 5, 9, 3), (B, T, 72, 16, 0, 8, 16, SOURCE),
                 (B, T, 1 << 22, 1 << 22, 0, 1 << 22, 1 << 22, NONE)):
        assert q(*args) == -1, args


def test_python_entry_runs_the_kernel():
    """``metric_inputs`` on device tensors: the raw entry's bits, on torch's current stream; other dtypes take the torch
    statement; a scale above the cap raises."""
    from multi_stylegan_amd import validation_metrics as vm
    L = _lib()
    src, size = (24, 40), (16, 48)
    for in_dtype in (torch.float32, torch.bfloat16):
        x = inputs(src, in_dtype)
        for norm in (NONE, SOURCE, RESIZED):
            for t, planes, dtype in ((None, 3, None), (1, 1, torch.bfloat16)):
                got = vm.metric_inputs(x.to(DEV), 2, t=t, size=size, normalize=NORM_NAMES[norm], planes=planes, dtype=dtype)
                status, want = call(x, 2, -1 if t is None else t, size, norm, planes=planes, out_dtype=dtype or torch.float32)
                assert got.is_cuda and got.dtype == want.dtype and got.is_contiguous()
                assert torch.equal(got.cpu().view(torch.uint8), want.view(torch.uint8))
    x = inputs(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = vm.metric_inputs(x.to(DEV), 0, normalize="resized", size=size)
    side.synchronize()
    check(got.cpu(), src, torch.float32, 0, -1, size, RESIZED, "side stream")
    got = vm.metric_inputs(x.to(DEV).transpose(3, 4), 1, t=0, size=None, normalize=None)   # not contiguous, source size
    assert torch.equal(got.cpu()[:, 0, 0], x[:, 1, 0].transpose(1, 2))
    got = vm.metric_inputs(x.to(DEV).double(), 1, t=0, size=size, dtype=torch.float64)    # float64: the torch statement
    assert got.is_cuda and got.dtype == torch.float64
    want, spread = reference(src, torch.float32, 1, 0, size, SOURCE)
    assert float((got.cpu()[:, 0] - want[:, 0]).abs().max()) <= max(bounds(src, torch.float32, 1, 0, size, SOURCE))
    with pytest.raises(L.MsgHipError, match="msg_metric_input"):
        vm.metric_inputs(inputs((72, 16)).to(DEV), 0, size=(8, 16))


class _Net(torch.nn.Module):
    def __init__(self, dims):
        super().__init__()
        conv = torch.nn.Conv2d if dims == 2 else torch.nn.Conv3d
        self.net = conv(3, 6, 3, stride=2, padding=1)
        self.seen = []

    def forward(self, x):
        self.seen.append(x.detach().cpu())
        return self.net(x).flatten(2).mean(2)


@pytest.mark.parametrize("kind", ["FID", "FVD", "IS"])
def test_metric_classes_resize_their_inputs(golden, kind):
    """``FID(net, input_size=(48, 48))`` / ``FVD(net, input_size=(40, 40))`` / ``IS(net, input_size=(48, 48))`` on the tiny
    generator (32 x 32 frames): the network sees the resized shape within [-1, 1], and with the seed fixed its first input is the
    statement of the frames it was made from."""
    from multi_stylegan_amd import validation_metrics as vm
    from test_hip_models import _models
    _, g, _ = _models(golden)
    size = (40, 40) if kind == "FVD" else (48, 48)
    net = _Net(3 if kind == "FVD" else 2).to(DEV)
    dataset = [mu.frames(4, 2, 3, 32, 32, seed=20 + k, ranges=((0.0, 1.0), (0.2, 0.7))) for k in range(3)]
    made = []
    g.register_forward_hook(lambda _m, _i, out: made.append(out.detach().float().cpu()))
    metric = getattr(vm, kind)(net, device=DEV, batch_size=4, data_samples=8, no_rfp=True, input_size=size)
    torch.manual_seed(7)
    scores = metric(g) if kind == "IS" else metric(g, dataset)
    assert len(scores) == 2 and all(math.isfinite(s) for s in scores)
    shape = (4, 3, 3, *size) if kind == "FVD" else (4, 3, *size)
    assert all(tuple(s.shape) == shape for s in net.seen)
    assert all(float(s.min()) >= -1.0 - 1e-6 and float(s.max()) <= 1.0 + 1e-6 for s in net.seen)
    # the first input: channel 0 of the first batch (the dataset's for FID / FVD, the generator's for IS), and for the frame
    # metrics the time step of the first draw after the seed
    torch.manual_seed(7)
    t = -1 if kind == "FVD" else int(torch.randint(0, 3, (1,)))
    frames = made[0] if kind == "IS" else dataset[0]
    normalize = "resized" if kind == "IS" else "source"
    want, spread = mu.reference(frames, 0, t, size, normalize, planes=3)
    got = net.seen[0].double() if kind == "FVD" else net.seen[0].double()[:, :, None]
    sel = frames[:, 0] if t < 0 else frames[:, 0, t:t + 1]
    for b in range(4):
        limit = mu.normalised_bound((32, 32), size, float(sel[b].abs().max()), float(spread[b]))
        assert float((got[b] - want[b]).abs().max()) <= limit, (kind, b)
