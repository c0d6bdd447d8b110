"""msg_tlfm_export (csrc/tlfm_export.hip) and the device side of multi_stylegan_amd/simulate.py: the kernel against the host's
torch statement count for count, the round trip through the existing reader (prepare_tlfm_batch, ResidentTLFMStore), and
simulate_dataset on the golden tiny generator."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from simulate_util import GFP, RFP, assert_round_trip, clean_frames, edge_frames, ranges_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                  # 16-bit words kept in front of and behind every raw-entry output
SHAPES = [(2, 2, 3, 8, 16),                 # vector path
          (1, 3, 2, 5, 12),                 # scalar path
          (3, 1, 1, 1, 8),                  # H = 1
          (1, 2, 1, 3, 24),                 # H < S is not reachable below 4096 pixels: S = 1 here, three short rows
          (1, 2, 1, 64, 64),                # exactly 4096 pixels: S = 1
          (1, 2, 1, 64, 72),                # S = 2
          (1, 2, 2, 33, 128),               # S = 2 over 33 rows: 17 + 16
          (1, 1, 1, 264, 512),              # S at its cap of 32: 9 rows each, the last three splits 9, 3 and 0 rows
          (2, 3, 3, 7, 250)]                # scalar path, odd W / 8


def _entry(x_dev, ranges_dev, vflip, normalise, fill, out_offset=0, gfp=GFP, rfp=RFP):
    """msg_tlfm_export itself on device tensors, into an output pre-filled with ``fill`` between two guard zones; -> the counts
    (numpy uint16) after checking that the guards still hold ``fill``."""
    from multi_stylegan_amd import _lib
    B, C, T, H, W = x_dev.shape
    n = x_dev.numel()
    backing = torch.full((GUARD + out_offset + n + GUARD,), fill, dtype=torch.int16, device=DEV)
    out = backing[GUARD + out_offset:GUARD + out_offset + n]
    lib = _lib.lib()
    ws = _lib.scratch_ptr(lib.msg_tlfm_export_workspace(B, T), x_dev.device)
    rc = lib.msg_tlfm_export(x_dev.data_ptr(), _lib.dtype_code(x_dev), ranges_dev.data_ptr(), out.data_ptr(), B, C, T, H, W,
                             int(vflip), int(normalise), gfp[0], gfp[1], rfp[0], rfp[1], ws, _lib.stream_of(x_dev.device))
    assert rc == _lib.MSG_OK
    host = backing.cpu().numpy()
    assert (host[:GUARD + out_offset] == fill).all() and (host[GUARD + out_offset + n:] == fill).all(), "a guard word was written"
    return host[GUARD + out_offset:GUARD + out_offset + n].view(np.uint16).reshape(B, C, T, H, W)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_host_statement(shape, dtype):
    from multi_stylegan_amd import export_tlfm_batch
    x = edge_frames(shape, dtype)
    assert bool(x.float().isnan().any())
    if shape == SHAPES[0]:
        assert bool(x[:, 0].float().isinf().any()) and bool((x[0, 0, 2].float().reshape(-1)[1:] == x[0, 0, 2, 0, 1].float()).all())
    B, C, T, H, W = shape
    ranges = ranges_for(B, T, shift=H)
    x_dev, ranges_dev = x.to(DEV), ranges.to(DEV)
    assert x_dev.data_ptr() % 16 == 0
    for vflip in (True, False):
        for normalise in (True, False):
            want = export_tlfm_batch(x, ranges, vertical_flip=vflip, bf_normalise=normalise).numpy()      # the host's statement
            for fill in (0x5555, -0x5556):                                    # every count is written, whatever was there
                assert np.array_equal(_entry(x_dev, ranges_dev, vflip, normalise, fill), want), (vflip, normalise, fill)
            got = export_tlfm_batch(x_dev, ranges_dev, vertical_flip=vflip, bf_normalise=normalise)       # the public op
            assert got.is_cuda and got.dtype == torch.uint16 and np.array_equal(got.cpu().numpy(), want)
    if H > 1:                                                                 # the flip is a whole-row remap and nothing else
        a = export_tlfm_batch(x_dev, ranges_dev, vertical_flip=True).cpu().numpy()
        b = export_tlfm_batch(x_dev, ranges_dev, vertical_flip=False).cpu().numpy()
        assert np.array_equal(a, b[:, :, :, ::-1])
    pair = export_tlfm_batch(x_dev, (20001, 60000), gfp=(100.0, 3000.0), rfp=(7.0, 60000.0))  # one range for all, other settings
    assert np.array_equal(pair.cpu().numpy(), export_tlfm_batch(x, (20001, 60000), gfp=(100.0, 3000.0), rfp=(7.0, 60000.0)).numpy())


def test_the_product_and_the_sum_are_rounded_separately():
    """A fused multiply-add rounds n * scale + offset once and lands on another count next to a tie.  With lo = 0 the sum is exact
    and both agree, and so do they while the sum stays in the product's binade: the offsets here are large: the inputs tell the two apart (shown on the host), and the
    kernel gives the separately rounded counts on both paths."""
    from multi_stylegan_amd import export_tlfm_batch
    for shape in ((2, 3, 2, 32, 64), (2, 3, 2, 31, 66)):                      # vector and scalar path
        x = clean_frames(shape, seed=9)
        settings = dict(gfp=(30000.0, 35000.0), rfp=(20000.0, 45000.0))
        want = export_tlfm_batch(x, (20001, 60000), **settings).numpy()
        n = torch.cat([((x[:, :1] - x[:, :1].flatten(3).amin(3)[..., None, None])
                        / (x[:, :1].flatten(3).amax(3) - x[:, :1].flatten(3).amin(3))[..., None, None]), x[:, 1:].clamp(0, 1)], dim=1)
        scale = torch.tensor([39999.0, 35000.0, 45000.0]).view(1, 3, 1, 1, 1)
        offset = torch.tensor([20001.0, 30000.0, 20000.0]).view(1, 3, 1, 1, 1)
        fused = torch.round((n.double() * scale.double() + offset.double()).float()).flip(-2).numpy()     # one rounding
        assert all(0 < (fused[:, c] != want[:, c]).sum() < 0.05 * want[:, c].size for c in range(3))      # the inputs can tell
        assert np.array_equal(export_tlfm_batch(x.to(DEV), (20001, 60000), **settings).cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_misaligned_bases_take_the_scalar_path(dtype):
    """W % 8 == 0, but the input or the output starts one element off a 16-byte boundary."""
    from multi_stylegan_amd import export_tlfm_batch
    shape = (2, 2, 3, 8, 16)
    x = edge_frames(shape, dtype, seed=1)
    ranges = ranges_for(2, 3, shift=3)
    want = export_tlfm_batch(x, ranges).numpy()
    backing = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
    backing[1:] = x.reshape(-1).to(DEV)
    shifted = backing[1:].view(shape)
    assert shifted.data_ptr() % 16 == x.element_size() and shifted.is_contiguous()
    ranges_dev = ranges.to(DEV)
    assert np.array_equal(_entry(shifted, ranges_dev, True, True, 0x5555), want)
    assert np.array_equal(export_tlfm_batch(shifted, ranges_dev).cpu().numpy(), want)
    assert np.array_equal(_entry(x.to(DEV), ranges_dev, True, True, -0x5556, out_offset=1), want)
    assert np.array_equal(_entry(shifted, ranges_dev, False, False, 0x5555, out_offset=1),
                          export_tlfm_batch(x, ranges, vertical_flip=False, bf_normalise=False).numpy())


def test_argument_errors_return_einval():
    from multi_stylegan_amd import _lib
    lib = _lib.lib()
    fn = lib._ctypes.msg_tlfm_export                                          # raw ctypes
    n = 2 * 4 * 3 * 8 * 16
    x = torch.zeros(n, device=DEV)
    out = torch.full((n,), 0x5555, dtype=torch.int16, device=DEV)
    ranges = torch.tensor([[0, 65535]] * 6, dtype=torch.int32, device=DEV)
    ws = torch.zeros(lib.msg_tlfm_export_workspace(2, 3), device=DEV)
    stream = ctypes.c_void_p(_lib.stream_of(x.device))
    assert lib.msg_tlfm_export_workspace(2, 3) == 2 * 32 * 6 and lib.msg_tlfm_export_workspace(0, 3) == 0

    def call(dtype=_lib.MSG_F32, B=2, C=2, T=3, H=8, W=16, x_p=x.data_ptr(), r_p=ranges.data_ptr(), out_p=out.data_ptr(),
             ws_p=ws.data_ptr(), normalise=1):
        return fn(x_p, dtype, r_p, out_p, B, C, T, H, W, 1, normalise, 150.0, 2200.0, 20.0, 2000.0, ws_p, stream)
    assert call(x_p=None) == _lib.MSG_EINVAL and call(r_p=None) == _lib.MSG_EINVAL and call(out_p=None) == _lib.MSG_EINVAL
    assert call(ws_p=None) == _lib.MSG_EINVAL
    assert call(B=0) == _lib.MSG_EINVAL and call(C=4) == _lib.MSG_EINVAL and call(C=0) == _lib.MSG_EINVAL
    assert call(T=-1) == _lib.MSG_EINVAL and call(H=0) == _lib.MSG_EINVAL and call(W=0) == _lib.MSG_EINVAL
    assert call(dtype=_lib.MSG_F16) == _lib.MSG_EINVAL and call(dtype=_lib.MSG_F64) == _lib.MSG_EINVAL and call(dtype=17) == _lib.MSG_EINVAL
    assert call(B=1 << 20, C=3, T=1 << 10) == _lib.MSG_EINVAL                 # more blocks than a launch can address
    torch.cuda.synchronize()
    assert bool((out == 0x5555).all())                                        # nothing was launched
    assert call(ws_p=None, normalise=0) == _lib.MSG_OK                        # no reduction, no workspace
    torch.cuda.synchronize()
    written = 2 * 2 * 3 * 8 * 16
    assert bool((out[written:] == 0x5555).all())                              # C = 2 of the 4 channels there is room for
    assert sorted(set(out[:written].cpu().tolist())) == [0, 150]              # zeros: the bright field's lo and gfp's minimum
    with pytest.raises(_lib.MsgHipError):
        _lib.check(call(C=4), "msg_tlfm_export")


def test_public_op_refusals_and_other_inputs():
    from multi_stylegan_amd import export_tlfm_batch
    x = clean_frames((2, 2, 3, 8, 16)).to(DEV)
    for bad in ((5, 5), (-1, 10), (0, 65536), (10, 5), (0.5, 9)):
        with pytest.raises(ValueError):
            export_tlfm_batch(x, bad)
    with pytest.raises(ValueError):
        export_tlfm_batch(x[0], (0, 100))
    with pytest.raises(ValueError):
        export_tlfm_batch(x.half(), (0, 100))
    with pytest.raises(ValueError):
        export_tlfm_batch(torch.zeros(1, 4, 1, 8, 8, device=DEV), (0, 100))
    with pytest.raises(ValueError):
        export_tlfm_batch(x, torch.zeros(2, 2, 2, dtype=torch.int32, device=DEV))
    strided = x.transpose(3, 4).contiguous().transpose(3, 4)
    assert not strided.is_contiguous()
    assert np.array_equal(export_tlfm_batch(strided, (0, 999)).cpu().numpy(), export_tlfm_batch(x.cpu(), (0, 999)).numpy())
    assert tuple(export_tlfm_batch(torch.zeros(0, 2, 3, 8, 16, device=DEV), (0, 9)).shape) == (0, 2, 3, 8, 16)


def test_unnormalised_zeros_write_the_offsets():
    """bf_normalise = 0 on zeros writes each channel's offset: lo for the bright field, gfp_min / rfp_min for the others."""
    from multi_stylegan_amd import export_tlfm_batch
    got = export_tlfm_batch(torch.zeros(1, 3, 1, 4, 8, device=DEV), (7, 9), bf_normalise=False).cpu().numpy()
    assert (got[:, 0] == 7).all() and (got[:, 1] == 150).all() and (got[:, 2] == 20).all()


@pytest.mark.parametrize("shape", [(2, 3, 3, 16, 24), (2, 2, 2, 33, 130)])
def test_device_round_trip(shape):
    """prepare_tlfm_batch(export_tlfm_batch(x)) on the device: within the round-trip bound of the definition, and the CPU round
    trip bit for bit."""
    from multi_stylegan_amd import export_tlfm_batch, prepare_tlfm_batch
    from tlfm_util import same_bits
    x = clean_frames(shape, seed=5)
    B, C, T, H, W = shape
    ranges = ranges_for(B, T, shift=1)
    counts = export_tlfm_batch(x.to(DEV), ranges.to(DEV))
    back = prepare_tlfm_batch(counts)
    host_counts = export_tlfm_batch(x, ranges)
    host_back = prepare_tlfm_batch(host_counts)
    assert np.array_equal(counts.cpu().numpy(), host_counts.numpy()) and same_bits(back, host_back)
    worst = assert_round_trip(x, ranges, counts, back)
    print("device round trip, worst case in counts (bright field, GFP / RFP):", worst)
    counts_bf16 = export_tlfm_batch(x.bfloat16().to(DEV), ranges.to(DEV))      # bf16 frames: the bound holds for what they hold
    assert_round_trip(x.bfloat16().float(), ranges, counts_bf16, prepare_tlfm_batch(counts_bf16))


def test_resident_store_of_exported_counts():
    from multi_stylegan_amd import ResidentTLFMStore, export_tlfm_batch, prepare_tlfm_batch
    from tlfm_util import same_bits
    shape = (3, 2, 3, 16, 24)
    x = clean_frames(shape, seed=6).to(DEV)
    counts = export_tlfm_batch(x, ranges_for(3, 3).to(DEV))
    table = torch.arange(3 * 2 * 3, dtype=torch.int32).reshape(3, 2, 3)
    store = ResidentTLFMStore.from_frames(counts.reshape(-1, 16, 24), table)
    assert store.device.type == "cuda" and len(store) == 3
    assert same_bits(store.gather([0, 1, 2]), prepare_tlfm_batch(counts))
    assert same_bits(store.gather([2, 0]), prepare_tlfm_batch(counts)[[2, 0]])


def test_two_calls_give_identical_bytes():
    from multi_stylegan_amd import export_tlfm_batch
    x = edge_frames((2, 2, 3, 136, 256), torch.float32, seed=8).to(DEV)        # S = 9: the split reduction
    ranges = ranges_for(2, 3).to(DEV)
    first = export_tlfm_batch(x, ranges).cpu().numpy().tobytes()
    for _ in range(3):
        assert export_tlfm_batch(x, ranges).cpu().numpy().tobytes() == first


# ------------------------------------------------------------------------------------------------ the tiny generator, 32^2
SEED, SAMPLES, BATCH, BF_RANGE = 11, 5, 2, (200, 50000)


@pytest.fixture(scope="module")
def tiny(golden):
    """The golden tiny generator and what an eager forward gives for the simulation's latents, in the simulation's batches."""
    from test_hip_models import _models
    from multi_stylegan_amd import simulation_latents
    _, g, _ = _models(golden)
    g.eval().requires_grad_(False)
    latents = simulation_latents(SEED, SAMPLES, g.latent_dimensions).to(DEV)
    images = []
    with torch.no_grad():
        for first in range(0, SAMPLES, BATCH):
            z = latents[first:first + BATCH]
            count = z.shape[0]
            z = torch.cat([z, z[-1:].expand(BATCH - count, -1)], dim=0) if count < BATCH else z
            images.append(g(z.contiguous(), randomize_noise=False)[:count].float().cpu())
    return g, torch.cat(images)


@pytest.mark.parametrize("use_graph", [False, True])
def test_simulate_dataset_reads_back_as_the_generator_s_frames(tiny, use_graph, tmp_path):
    from multi_stylegan_amd import TFLMDatasetGAN, prepare_tlfm_batch, simulate_dataset
    g, want = tiny
    assert tuple(want.shape) == (SAMPLES, 2, 3, 32, 32)
    out = str(tmp_path / "simulated")
    assert simulate_dataset(g, SAMPLES, out, batch_size=BATCH, bf_range=BF_RANGE, seed=SEED, use_graph=use_graph,
                            randomize_noise=False) == SAMPLES
    with open(os.path.join(out, "simulation.json")) as f:
        record = json.load(f)
    assert record["samples"] == SAMPLES and record["seed"] == SEED and record["bf_range"] == list(BF_RANGE)
    assert record["gfp"] == list(GFP) and record["rfp"] == list(RFP) and record["checkpoint"] is None
    assert sorted(n for n in os.listdir(out) if n != "simulation.json") == ["sim0000"]
    assert len(os.listdir(os.path.join(out, "sim0000"))) == SAMPLES * 2 * 3   # exactly 5 sequences: the padding is not written
    for overlap in (True, False):
        dataset = TFLMDatasetGAN(out, sequence_length=3, overlap=overlap, no_rfp=True, raw=True)
        assert len(dataset) == SAMPLES
    counts = torch.from_numpy(np.stack([dataset[k][0].numpy() for k in range(SAMPLES)]))
    back = prepare_tlfm_batch(counts)                                          # the reader's arithmetic, on the host
    ranges = torch.tensor(BF_RANGE, dtype=torch.int32).expand(SAMPLES, 3, 2)
    worst = assert_round_trip(want, ranges, counts, back)
    print("simulate_dataset round trip, worst case in counts:", worst)
    assert len({counts[k].numpy().tobytes() for k in range(SAMPLES)}) == SAMPLES   # one latent per sequence
