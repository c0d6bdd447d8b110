"""The device-side elastic deformation (csrc/elastic.hip: msg_elastic_deform), its Python entry (elastic.elastic_deform_batch) and
the feed hook (data.TLFMDeviceFeed(elastic=...)), against the reference's recorded outputs (tests/golden/elastic.npz) and the
tests' float64 restatement of dataset/tlfm_dataset.py:230-275 (tests/elastic_util.py).

Tolerances (none taken from what the kernels give):
  field  1e-6 alpha pixels.  A separable fp32 evaluation differs from float64 by <= 4.2e-8 alpha (measured on the host when the
         fixture was made); the margin covers FMA contraction and another summation order.  A wrong tap or halo is >= 1e-2 alpha.
  out    1e-4 (fp32) against the reference's recorded fp32 output, and against the restatement for shapes the fixture does not
         hold: the restatement is within 1.1e-5 of the reference, the fp32 position arithmetic at these sizes (<= 300 columns:
         a few roundings of half an ulp of 256, 1.5e-5 each) moves a full-contrast frame by < 5e-5.  A missed half-pixel shift,
         swapped divisors or swapped planes move these frames by ~0.28.
  bf16   2^-8: one bf16 ulp below 1, against the bf16 rounding of the float64 result (the inputs are exact in bf16).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from elastic_util import CASES, case, deform64_batch, same_bits, taps64
from tlfm_util import write_tiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELD_TOL, OUT_TOL, BF16_TOL = 1e-6, 1e-4, 2.0 ** -8


def _garbage(nbytes):
    return torch.full(((nbytes + 3) // 4,), 0x7FC55A5A, dtype=torch.int32, device=DEV)      # (NaNs, read as floats)


def _entry(frames, noise, sigma, alpha, dtype=torch.float32, offset=0):
    """msg_elastic_deform itself on [B, F, H, W] frames, with `out` and `field` pre-filled with -7 and a workspace of the test's
    own holding garbage.  ``offset``: frames and out start that many elements into their allocations (a misaligned base)."""
    from multi_stylegan_amd import _lib
    lib = _lib.lib()
    B, F, H, W = frames.shape
    src = torch.zeros(frames.numel() + offset, dtype=dtype, device=DEV)
    src[offset:] = frames.to(DEV).to(dtype).reshape(-1)
    out = torch.full((frames.numel() + offset,), -7.0, dtype=dtype, device=DEV)
    field = torch.full((B, 2, H, W), -7.0, device=DEV)
    nz = noise.to(DEV).float().contiguous()
    nbytes = lib.msg_elastic_workspace(B, H, W)
    assert nbytes == 8 * B * H * W                                         # one more [B, 2, H, W] fp32 array, nothing larger
    ws = _garbage(nbytes)
    rc = lib.msg_elastic_deform(src[offset:].data_ptr(), nz.data_ptr(), field.data_ptr(), out[offset:].data_ptr(),
                                _lib.dtype_code(src), B, F, H, W, int(sigma), float(alpha), ws.data_ptr(), _lib.stream_of(src.device))
    assert rc == _lib.MSG_OK
    torch.cuda.synchronize()
    assert offset == 0 or bool((out[:offset] == -7.0).all())
    return out[offset:].reshape(frames.shape).cpu(), field.cpu()


def _check(frames, noise, sigma, alpha, label, want_out=None):
    """fp32 and bf16 through the entry against the restatement (and `want_out`, the reference's own output, where recorded)."""
    ref_out, ref_field = deform64_batch(frames, noise, sigma, alpha)
    out, field = _entry(frames, noise, sigma, alpha)
    e_field = (field.double() - ref_field).abs().max().item() / abs(alpha)
    e_out = (out.double() - (ref_out if want_out is None else want_out.double())).abs().max().item()
    half, field16 = _entry(frames, noise, sigma, alpha, torch.bfloat16)
    e_half = (half.double() - ref_out.to(torch.bfloat16).double()).abs().max().item()
    print(f"{label}: field {e_field:.2e} alpha, out {e_out:.2e}, bf16 {e_half:.2e}")
    assert e_field <= FIELD_TOL and e_out <= OUT_TOL and e_half <= BF16_TOL
    assert not bool((out == -7.0).any()) and not bool((field == -7.0).any()) and not bool(out.isnan().any())
    assert same_bits(field16, field)                                       # the field does not depend on the frames' dtype
    return out, field


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(name):
    from multi_stylegan_amd import elastic_deform_batch
    c = case(name)
    out, field = _check(c["frames"][None], c["noise"][None], c["sigma"], c["alpha"], name, want_out=c["out"][None])
    # the Python entry: the same call on the library's launch-scoped workspace, same bits; 5-D frames are [B, C * T, H, W]
    got, got_field = elastic_deform_batch(c["frames"][None].to(DEV), c["noise"][None].to(DEV), alpha=c["alpha"], sigma=c["sigma"],
                                          return_field=True)
    assert same_bits(got, out) and same_bits(got_field, field)
    if c["frames"].shape[0] % 2 == 0:
        five = c["frames"].reshape(1, 2, -1, *c["frames"].shape[-2:]).to(DEV)
        assert same_bits(elastic_deform_batch(five, c["noise"][None].to(DEV), alpha=c["alpha"], sigma=c["sigma"]).flatten(1, 2), out)


# the issue's four (72 x 136 straddles every tile and takes the 16-byte path) and three of the tests' own: 20 x 44 (16-byte rows in
# fp32, not in bf16), 12 x 300 (a second 256-column block of the row pass, its halo across the seam), 40 x 56 at the largest sigma
@pytest.mark.parametrize("H,W,sigma", [(8, 8, 4), (40, 56, 3), (33, 33, 2), (72, 136, 5), (20, 44, 3), (12, 300, 2), (40, 56, 32)])
def test_batches(H, W, sigma):
    g = torch.Generator().manual_seed(H * 1000 + W)
    B, F, alpha = 3, 6, 25.0
    frames = torch.randint(0, 65, (B, F, H, W), generator=g).float() / 64.0
    noise = torch.rand((B, 2, H, W), generator=g) * 2 - 1
    out, field = _check(frames, noise, sigma, alpha, f"{H}x{W} sigma {sigma}")
    for dtype in (torch.float32, torch.bfloat16):
        whole, whole_field = _entry(frames, noise, sigma, alpha, dtype)
        again, again_field = _entry(frames, noise, sigma, alpha, dtype)
        assert same_bits(again, whole) and same_bits(again_field, whole_field)             # run to run
        for b in range(B):                                                                 # a sample alone
            one, one_field = _entry(frames[b:b + 1], noise[b:b + 1], sigma, alpha, dtype)
            assert same_bits(one[0], whole[b]) and same_bits(one_field[0], whole_field[b]), (dtype, b)
        shifted, shifted_field = _entry(frames, noise, sigma, alpha, dtype, offset=1)      # misaligned bases: the scalar path
        assert same_bits(shifted, whole) and same_bits(shifted_field, whole_field)


@pytest.mark.parametrize("H,W,sigma", [(8, 8, 4), (40, 56, 3)])
def test_zero_padding_in_closed_form(H, W, sigma):
    """noise == 1: d[y, x] = alpha (sum of the taps whose row is in the frame) (sum of the taps whose column is)."""
    alpha = 30.0
    g = taps64(sigma)

    def inside(size):
        at = torch.arange(size)[:, None] + torch.arange(4 * sigma + 1)[None, :] - 2 * sigma
        return (g[None, :] * ((at >= 0) & (at < size))).sum(dim=1)
    want = alpha * inside(H)[:, None] * inside(W)[None, :]
    _, field = _entry(torch.zeros(1, 1, H, W), torch.ones(1, 2, H, W), sigma, alpha)
    err = (field.double() - want).abs().max().item() / alpha
    print(f"{H}x{W}: closed form {err:.2e} alpha")
    assert err <= FIELD_TOL


def test_full_size_partition_of_unity_and_random_frames():
    B, F, H, W, sigma, alpha = 2, 6, 256, 256, 16, 80.0
    g = torch.Generator().manual_seed(77)
    noise = torch.rand((B, 2, H, W), generator=g) * 2 - 1
    flat, _ = _entry(torch.full((B, F, H, W), 0.37), noise, sigma, alpha)
    err = (flat - 0.37).abs().max().item()
    print(f"constant frame: {err:.2e}")
    assert err <= 1e-6
    _check(torch.randint(0, 65, (B, F, H, W), generator=g).float() / 64.0, noise, sigma, alpha, "256x256 defaults")


def test_status_codes_launch_nothing():
    from multi_stylegan_amd import _lib
    fn = _lib.lib()._ctypes.msg_elastic_deform                             # raw ctypes
    assert _lib.MSG_ELASTIC_MAX_SIGMA >= 32
    n = 2 * 3 * 8 * 8
    src, out = torch.zeros(n, device=DEV), torch.full((n,), -7.0, device=DEV)
    noise, field = torch.zeros(2 * 2 * 8 * 8, device=DEV), torch.full((2 * 2 * 8 * 8,), -7.0, device=DEV)
    ws = _garbage(_lib.lib().msg_elastic_workspace(2, 8, 8))
    stream = ctypes.c_void_p(_lib.stream_of(src.device))

    def call(dtype=_lib.MSG_F32, B=2, F=3, H=8, W=8, sigma=2, in_p=src.data_ptr(), noise_p=noise.data_ptr(),
             field_p=field.data_ptr(), out_p=out.data_ptr(), ws_p=ws.data_ptr()):
        return fn(in_p, noise_p, field_p, out_p, dtype, B, F, H, W, sigma, ctypes.c_float(10.0), ws_p, stream)
    for kw in (dict(in_p=None), dict(noise_p=None), dict(field_p=None), dict(out_p=None), dict(ws_p=None), dict(B=0), dict(F=0),
               dict(H=0), dict(W=-1), dict(sigma=0), dict(sigma=-3)):
        assert call(**kw) == _lib.MSG_EINVAL, kw
    for kw in (dict(dtype=_lib.MSG_F16), dict(dtype=_lib.MSG_F64), dict(dtype=17), dict(sigma=_lib.MSG_ELASTIC_MAX_SIGMA + 1)):
        assert call(**kw) == _lib.MSG_EUNSUPPORTED, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((field == -7.0).all())      # nothing was launched
    assert call(sigma=_lib.MSG_ELASTIC_MAX_SIGMA) == _lib.MSG_OK
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any()) and not bool((field == -7.0).any())
    assert _lib.lib().msg_elastic_workspace(0, 8, 8) == 0


def test_python_entry_draws_and_refusals():
    from multi_stylegan_amd import ElasticDeformation, elastic_deform_batch, elastic_deformation
    frames = (torch.randint(0, 65, (2, 2, 3, 16, 24), generator=torch.Generator().manual_seed(1)).float() / 64.0).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    noise = torch.rand((2, 2, 16, 24), device=DEV, generator=g) * 2 - 1
    want = elastic_deform_batch(frames, noise, alpha=10, sigma=2)
    got = elastic_deform_batch(frames, alpha=10, sigma=2, generator=torch.Generator(device=DEV).manual_seed(9))
    assert got.shape == frames.shape and got.data_ptr() != frames.data_ptr() and same_bits(got, want)
    assert same_bits(ElasticDeformation(alpha=10, sigma=2, generator=torch.Generator(device=DEV).manual_seed(9)).deform_batch(frames),
                     want)
    # the reference's function on a device tensor: its two [H, W] draws from the device's global generator, first one horizontal
    torch.manual_seed(4)
    planes = torch.stack([torch.rand((16, 24), device=DEV) * 2 - 1 for _ in range(2)])
    torch.manual_seed(4)
    one = elastic_deformation(frames[0].flatten(0, 1), alpha=10, sigma=2)
    assert one.shape == (6, 16, 24)
    assert same_bits(one, elastic_deform_batch(frames[:1], planes[None], alpha=10, sigma=2)[0].flatten(0, 1))
    with pytest.raises(ValueError, match="nearest"):
        elastic_deformation(frames[0, 0], sample_mode="nearest")
    with pytest.raises(ValueError, match="autograd"):
        elastic_deform_batch(frames.clone().requires_grad_(True), alpha=10, sigma=2)


def _write_dataset(root, frames, H, W, seed):
    rng = np.random.default_rng(seed)
    for kind, top in (("BF0", 65536), ("GFP", 3000)):
        for time in range(frames):
            write_tiff(os.path.join(root, "pos1", f"pos1_t{time:03d}_x_trap0001-{kind}_000_0001.tif"),
                       rng.integers(0, top, size=(H, W)).astype(np.uint16))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_feed_deforms_every_batch(tmp_path, out_dtype):
    from torch.utils.data import DataLoader
    from multi_stylegan_amd import ElasticDeformation, TFLMDatasetGAN, TLFMDeviceFeed, elastic_deform_batch, prepare_tlfm_batch
    root = str(tmp_path / "dataset")
    _write_dataset(root, 7, 16, 24, seed=8)                                   # 5 samples: batches of 2, 2, 1
    torch.manual_seed(21)
    batches = list(DataLoader(TFLMDatasetGAN(root, no_rfp=True, raw=True), batch_size=2))
    assert [len(b[0]) for b in batches] == [2, 2, 1]
    plain = [prepare_tlfm_batch(f.to(DEV), h.to(DEV), out_dtype=out_dtype) for f, h in batches]
    g = torch.Generator(device=DEV).manual_seed(33)
    want = [elastic_deform_batch(p, alpha=12, sigma=3, generator=g) for p in plain]
    module = ElasticDeformation(alpha=12, sigma=3, generator=torch.Generator(device=DEV).manual_seed(33))
    got = list(TLFMDeviceFeed(batches, DEV, elastic=module, out_dtype=out_dtype))
    assert len(got) == 3 and all(a.dtype == out_dtype and same_bits(a, b) for a, b in zip(got, want))
    assert not any(same_bits(a, p) for a, p in zip(got, plain))
    none = list(TLFMDeviceFeed(batches, DEV, elastic=None, out_dtype=out_dtype))
    assert all(same_bits(a, p) for a, p in zip(none, plain))                 # elastic=None: the feed as it was
