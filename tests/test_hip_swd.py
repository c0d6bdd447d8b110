"""The sliced Wasserstein kernels (csrc/swd.hip) on the GPU: every raw entry on guarded memory against the float64 statement of
tests/swd_util.py, at every tile edge and on both load paths, their refusals and run-to-run bit identity; then
``sliced_wasserstein`` on device tensors and the SWD / SWVD classes against their CPU run.

Every bound is derived in swd_util's docstring from the order of operations include/msg_hip.h states, not from what a kernel
returned."""
import math

import numpy as np
import pytest
import torch

import swd_util as su
from test_hip_metric_input import DEV, Region
from test_swd import StubGenerator, corner_positions, stub_dataset, texture_rows

pytestmark = pytest.mark.gpu
ROW_TILE = 128                           # PJ_T of csrc/swd.hip: descriptor rows (and directions) per workgroup
SUM_ROWS = 256                           # PS_ROWS: descriptor rows per workgroup of the plane sums
L1_CHUNK = 4096                          # elements of one direction per workgroup of the sorted L1
NAN_FILL = 0xFF


def _L():
    from multi_stylegan_amd import _lib
    return _lib


def _vm():
    from multi_stylegan_amd import validation_metrics as vm
    return vm


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _untouched(region):
    return bool((region.bytes() == NAN_FILL).all())


def _rng(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------ msg_laplacian_level
def run_level(fine, with_lap=True, shift=0, null=(), dims=None):
    """-> (status, coarse, lap) on the host.  A refused call leaves its outputs' fill bytes alone; an accepted one leaves no
    element unwritten (the fill is a NaN)."""
    lib = _L().lib()
    m, h, w = fine.shape
    M, hh, ww = dims or (m, h, w)
    src = Region.of(fine, shift)
    coarse = Region(max(m * (h // 2) * (w // 2), 1) * 4, shift)
    lap = Region(m * h * w * 4, shift)
    status = lib.msg_laplacian_level(None if "fine" in null else src.ptr, M, hh, ww, None if "coarse" in null else coarse.ptr,
                                     lap.ptr if with_lap else None, _stream())
    src.bytes()
    if status != 0:
        assert _untouched(coarse) and _untouched(lap), "a refused call wrote to an output"
        return status, None, None
    c = coarse.values(torch.float32, (m, h // 2, w // 2))
    if not with_lap:
        assert _untouched(lap)
        return status, c, None
    return status, c, lap.values(torch.float32, (m, h, w))


def check_level(fine, coarse, lap):
    want_c, want_l = su.level(fine.numpy())
    bound_c, bound_l = su.level_bounds(fine.numpy())
    assert not bool(coarse.isnan().any()) and (lap is None or not bool(lap.isnan().any())), "an element was not written"
    err_c = np.abs(coarse.double().numpy() - want_c)
    assert (err_c <= bound_c).all(), float((err_c - bound_c).max())
    worst = float((err_c / np.maximum(bound_c, 1e-300)).max())
    if lap is not None:
        err_l = np.abs(lap.double().numpy() - want_l)
        assert (err_l <= bound_l).all(), float((err_l - bound_l).max())
        worst = max(worst, float((err_l / np.maximum(bound_l, 1e-300)).max()))
    return worst


LEVEL_SIZES = [(8, 8), (16, 24), (32, 32), (130, 66)]


@pytest.mark.parametrize("size", LEVEL_SIZES)
@pytest.mark.parametrize("M", [1, 7])
def test_laplacian_level_on_noise(M, size):
    fine = torch.randn((M,) + size, generator=_rng(M + size[0])) * 50.0 + 100.0
    status, coarse, lap = run_level(fine)
    assert status == 0
    print(f"{M} x {size}: worst error / bound {check_level(fine, coarse, lap):.3f}")
    # lap = NULL: the Gaussian pyramid only, the same coarse bits
    status, only, none = run_level(fine, with_lap=False)
    assert status == 0 and none is None and torch.equal(only.view(torch.int32), coarse.view(torch.int32))
    # off the 16-byte alignment: element by element, the same bits
    status, c2, l2 = run_level(fine, shift=4)
    assert status == 0 and torch.equal(c2.view(torch.int32), coarse.view(torch.int32))
    assert torch.equal(l2.view(torch.int32), lap.view(torch.int32))


@pytest.mark.parametrize("size", LEVEL_SIZES)
def test_laplacian_level_on_impulses_pins_the_mirror_rule(size):
    """One impulse per plane: the four corners and the four edge midpoints (and their inner neighbours, which the mirror rule
    reads twice).  Away from an impulse's support the bound is 0: those outputs are exact zeros."""
    h, w = size
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1),
             (1, 1), (h - 2, w - 2), (1, w // 2 + 1), (h // 2 + 1, w - 2)]
    fine = torch.zeros((len(spots), h, w))
    for m, (y, x) in enumerate(spots):
        fine[m, y, x] = 3.7 if m % 2 else 1.0
    for shift in (0, 4):
        status, coarse, lap = run_level(fine, shift=shift)
        assert status == 0
        check_level(fine, coarse, lap)
    want_c, _ = su.level(fine.numpy())
    assert float(np.abs(want_c).max()) > 0.1                                  # (the statement sees the impulses)


def test_laplacian_level_refusals():
    einval = _L().MSG_EINVAL
    ok = torch.ones(1, 8, 8)
    for shape in ((1, 9, 8), (1, 8, 9), (1, 6, 8), (1, 8, 6), (1, 7, 7)):
        assert run_level(torch.ones(shape))[0] == einval, shape
    assert run_level(ok, dims=(0, 8, 8))[0] == einval
    assert run_level(ok, dims=(1, -8, 8))[0] == einval
    assert run_level(ok, null=("fine",))[0] == einval
    assert run_level(ok, null=("coarse",))[0] == einval
    assert run_level(ok, shift=2)[0] == einval
    assert run_level(ok)[0] == 0


# ----------------------------------------------------------------------------------------------------------- msg_swd_gather
def run_gather(level, pos, shift=0, null=(), dims=None):
    lib = _L().lib()
    B, P, h, w = level.shape
    K = pos.shape[1]
    src, idx = Region.of(level), Region.of(pos.to(torch.int32))
    rows = Region(B * K * P * 49 * 4, shift)
    b, p, hh, ww, k = dims or (B, P, h, w, K)
    status = lib.msg_swd_gather(None if "level" in null else src.ptr, b, p, hh, ww, None if "pos" in null else idx.ptr, k,
                                None if "rows" in null else rows.ptr, _stream())
    src.bytes()
    idx.bytes()
    if status != 0:
        assert _untouched(rows), "a refused call wrote to its output"
        return status, None
    return status, rows.values(torch.float32, (B * K, P * 49))


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("size", [(16, 16), (16, 24), (40, 24)])
@pytest.mark.parametrize("K", [1, 5, 128])
def test_gather_copies_the_bits(K, size, planes):
    B, (h, w) = 3, size
    level = torch.randn((B, planes, h, w), generator=_rng(K + h + planes))
    level[0, 0, 0, 0] = -0.0
    pos = corner_positions(B, h, w, max(K, 4), seed=K)[:, :K].contiguous()
    pos[B - 1, K - 1] = torch.tensor([1, w - 2], dtype=torch.int32)            # out of the legal range: taps above and to the right
    if K >= 5:
        pos[1, 0] = torch.tensor([h + 1, -2], dtype=torch.int32)               # a centre outside the plane
    want = torch.from_numpy(su.descriptors(level.numpy(), pos.numpy()))
    assert int((want == 0).sum()) >= 7 * planes
    for shift in (0, 4):
        status, rows = run_gather(level, pos, shift)
        assert status == 0 and torch.equal(rows.view(torch.int32), want.view(torch.int32)), shift


def test_gather_refusals():
    einval = _L().MSG_EINVAL
    level, pos = torch.ones(2, 1, 16, 16), torch.full((2, 3, 2), 8, dtype=torch.int32)
    for dims in ((0, 1, 16, 16, 3), (2, 0, 16, 16, 3), (2, 1, 0, 16, 3), (2, 1, 16, -1, 3), (2, 1, 16, 16, 0)):
        assert run_gather(level, pos, dims=dims)[0] == einval, dims
    for name in ("level", "pos", "rows"):
        assert run_gather(level, pos, null=(name,))[0] == einval
    assert run_gather(level, pos, shift=2)[0] == einval
    assert run_gather(level, pos)[0] == 0


# ------------------------------------------------------------------------------------------------------- msg_swd_plane_sums
def run_plane_sums(rows, planes, shift=0, null=(), dims=None, sums_shift=0):
    lib = _L().lib()
    n = rows.shape[0]
    nn, pp = dims or (n, planes)
    src = Region.of(rows, shift)
    sums = Region(planes * 2 * 8, sums_shift)
    nbytes = lib.msg_swd_plane_sums_workspace(nn, pp)
    ws = Region(max(nbytes, 0) + 8, 0)
    status = lib.msg_swd_plane_sums(None if "rows" in null else src.ptr, nn, pp, None if "sums" in null else sums.ptr,
                                    None if "ws" in null else ws.ptr, _stream())
    src.bytes()
    ws.bytes()
    if status != 0:
        assert _untouched(sums), "a refused call wrote to its output"
        return status, None
    return status, sums.values(torch.float64, (planes, 2))


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("n", [1, SUM_ROWS - 1, SUM_ROWS, SUM_ROWS + 1, 3 * SUM_ROWS + 7])
def test_plane_sums(n, planes):
    rows = torch.randn((n, planes * 49), generator=_rng(n + planes)) * 30.0 + 100.0
    x = rows.double().view(n, planes, 49)
    for shift in (0, 4):
        status, sums = run_plane_sums(rows, planes, shift)
        assert status == 0
        for p in range(planes):
            assert abs(float(sums[p, 0]) - float(x[:, p].sum())) <= 1e-12 * float(x[:, p].abs().sum())
            assert abs(float(sums[p, 1]) - float(x[:, p].square().sum())) <= 1e-12 * float(x[:, p].square().sum())


def test_plane_sums_refusals():
    einval, rows = _L().MSG_EINVAL, torch.ones(5, 49)
    assert _L().lib().msg_swd_plane_sums_workspace(0, 1) == -1 and _L().lib().msg_swd_plane_sums_workspace(5, 0) == -1
    for dims in ((0, 1), (5, 0), (-5, 1)):
        assert run_plane_sums(rows, 1, dims=dims)[0] == einval
    for name in ("rows", "sums", "ws"):
        assert run_plane_sums(rows, 1, null=(name,))[0] == einval
    assert run_plane_sums(rows, 1, shift=2)[0] == einval and run_plane_sums(rows, 1, sums_shift=4)[0] == einval
    assert run_plane_sums(rows, 1)[0] == 0


# ---------------------------------------------------------------------------------------------------------- msg_swd_project
def run_project(rows, planes, mean, istd, dirs, shift=0, null=(), dims=None):
    lib = _L().lib()
    n, R = rows.shape[0], dirs.shape[1]
    nn, pp, rr = dims or (n, planes, R)
    src, m, s, dr = Region.of(rows, shift), Region.of(mean), Region.of(istd), Region.of(dirs)
    out = Region(R * n * 4, shift)
    ptr = lambda name, region: None if name in null else region.ptr
    status = lib.msg_swd_project(ptr("rows", src), nn, pp, ptr("mean", m), ptr("istd", s), ptr("dirs", dr), rr, ptr("out", out),
                                 _stream())
    for region in (src, m, s, dr):
        region.bytes()
    if status != 0:
        assert _untouched(out), "a refused call wrote to its output"
        return status, None
    return status, out.values(torch.float32, (R, n))


def _project_case(n, planes, R, seed):
    g = _rng(seed)
    rows = torch.randn((n, planes * 49), generator=g) * 20.0 + 100.0
    mean = torch.randn(planes, generator=g) * 5.0 + 100.0
    istd = torch.rand(planes, generator=g) * 0.1 + 0.02
    dirs = _vm().swd_directions(planes * 49, 1, R, g)[0].contiguous()
    return rows, mean, istd, dirs


@pytest.mark.parametrize("planes", [1, 2, 3, 4])
def test_project_at_every_tile_edge(planes):
    """n around the row tile, R around the direction tile; planes = 4 (196 columns, a multiple of four) takes the 16-byte loads
    when aligned, everything else goes element by element; both give the same bits."""
    worst = 0.0
    for n in (1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 2 * ROW_TILE + 1):
        for R in (1, 127, 128, 129):
            rows, mean, istd, dirs = _project_case(n, planes, R, seed=1000 * planes + n + R)
            status, out = run_project(rows, planes, mean, istd, dirs)
            assert status == 0 and not bool(out.isnan().any()), "an output element was not written"
            hat = su.normalised(rows.numpy(), planes, mean.numpy(), istd.numpy())
            want = (hat @ dirs.double().numpy()).T
            bound = su.projection_bound(rows.numpy(), planes, mean.numpy(), istd.numpy(), dirs.numpy()).T
            err = np.abs(out.double().numpy() - want)
            assert (err <= bound).all(), (n, R, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            if n in (ROW_TILE + 1,) and R in (1, 129):
                status, other = run_project(rows, planes, mean, istd, dirs, shift=4)
                assert status == 0 and torch.equal(other.view(torch.int32), out.view(torch.int32))
    print(f"planes {planes}: worst error / bound {worst:.3f}")


def test_project_refusals():
    einval = _L().MSG_EINVAL
    rows, mean, istd, dirs = _project_case(5, 1, 3, seed=1)
    for dims in ((0, 1, 3), (5, 0, 3), (5, 1, 0), (-1, 1, 3)):
        assert run_project(rows, 1, mean, istd, dirs, dims=dims)[0] == einval
    for name in ("rows", "mean", "istd", "dirs", "out"):
        assert run_project(rows, 1, mean, istd, dirs, null=(name,))[0] == einval
    assert run_project(rows, 1, mean, istd, dirs, shift=2)[0] == einval
    assert run_project(rows, 1, mean, istd, dirs)[0] == 0


# ------------------------------------------------------------------------------------------------------------ msg_sorted_l1
def run_sorted_l1(a, b, shift=0, null=(), dims=None, sums_shift=0):
    lib = _L().lib()
    R, n = a.shape
    rr, nn = dims or (R, n)
    ra, rb = Region.of(a, shift), Region.of(b, shift)
    sums = Region(R * 8, sums_shift)
    nbytes = lib.msg_sorted_l1_workspace(rr, nn)
    ws = Region(max(nbytes, 0) + 8, 0)
    ptr = lambda name, region: None if name in null else region.ptr
    status = lib.msg_sorted_l1(ptr("a", ra), ptr("b", rb), rr, nn, ptr("sums", sums), ptr("ws", ws), _stream())
    ra.bytes()
    rb.bytes()
    ws.bytes()
    if status != 0:
        assert _untouched(sums), "a refused call wrote to its output"
        return status, None
    return status, sums.values(torch.float64, (R,))


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("n", [1, 7, L1_CHUNK - 1, L1_CHUNK, L1_CHUNK + 1, 2 * L1_CHUNK + 8])
def test_sorted_l1(n, R):
    g = _rng(n + R)
    a = torch.randn((R, n), generator=g).sort(dim=1).values
    b = (torch.randn((R, n), generator=g) * 1.2 + 0.1).sort(dim=1).values
    want = (a.double() - b.double()).abs().sum(dim=1)
    for shift in (0, 4):
        status, sums = run_sorted_l1(a, b, shift)
        assert status == 0
        assert bool(((sums - want).abs() <= 2.0 ** -23 * want).all()), (sums, want)
        status, zero = run_sorted_l1(a, a.clone(), shift)
        assert status == 0 and zero.tolist() == [0.0] * R


def test_sorted_l1_refusals():
    einval = _L().MSG_EINVAL
    a, b = torch.zeros(2, 9), torch.ones(2, 9)
    assert _L().lib().msg_sorted_l1_workspace(0, 9) == -1 and _L().lib().msg_sorted_l1_workspace(2, 0) == -1
    for dims in ((0, 9), (2, 0), (2, -9), (70000, 9)):
        assert run_sorted_l1(a, b, dims=dims)[0] == einval
    for name in ("a", "b", "sums", "ws"):
        assert run_sorted_l1(a, b, null=(name,))[0] == einval
    assert run_sorted_l1(a, b, shift=2)[0] == einval and run_sorted_l1(a, b, sums_shift=4)[0] == einval
    status, sums = run_sorted_l1(a, b)
    assert status == 0 and sums.tolist() == [9.0, 9.0]


# ----------------------------------------------------------------------------------------------------- run-to-run identity
def test_every_entry_is_bit_identical_from_run_to_run():
    fine = torch.randn((5, 130, 66), generator=_rng(1)) * 50.0 + 100.0
    first, again = run_level(fine), run_level(fine)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first[1:], again[1:]))
    level, pos = torch.randn((3, 3, 16, 24), generator=_rng(2)), corner_positions(3, 16, 24, 128, seed=2)
    assert torch.equal(run_gather(level, pos)[1].view(torch.int32), run_gather(level, pos)[1].view(torch.int32))
    rows, mean, istd, dirs = _project_case(3 * SUM_ROWS + 7, 3, 129, seed=3)
    assert torch.equal(run_plane_sums(rows, 3)[1].view(torch.int64), run_plane_sums(rows, 3)[1].view(torch.int64))
    one, two = run_project(rows, 3, mean, istd, dirs)[1], run_project(rows, 3, mean, istd, dirs)[1]
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    a = one[:3, :].contiguous().sort(dim=1).values
    b = one[3:6, :].contiguous().sort(dim=1).values
    assert torch.equal(run_sorted_l1(a, b)[1].view(torch.int64), run_sorted_l1(a, b)[1].view(torch.int64))


# --------------------------------------------------------------------------------------------------------------- end to end
def _held(got, a, b, planes, seed, what, normalize=True):
    """``got``, a device score of the fp32 sets ``a``, ``b`` (numpy), against the float64 statement, within the derived bound."""
    dirs = _vm().swd_directions(planes * 49, 4, 128, _rng(seed)).numpy()
    want = su.swd(a, b, planes, dirs, normalize)
    limit = su.score_bound(a, b, planes, dirs, want, normalize)
    print(f"{what}: device {got:.9f}, float64 {want:.9f}, difference {abs(got - want):.3e}, bound {limit:.3e}")
    assert abs(got - want) <= limit and limit < 2e-2 * want, what


def test_sliced_wasserstein_on_device_tensors():
    vm = _vm()
    rows = texture_rows()
    for x, y, lvl in (("A", "C", 0), ("A", "B", 0), ("A", "C", 2)):
        a, b = rows[x][lvl].astype(np.float32), rows[y][lvl].astype(np.float32)
        got = vm.sliced_wasserstein(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 3, generator=_rng(5))
        _held(got, a, b, 3, 5, f"textures {x}-{y}, level {lvl}")
    # 32 x 48 frames, one plane, the whole chain on the device: pyramid, gather, score
    sets = []
    for s in range(2):
        frames = torch.rand((8, 1, 32, 48), generator=_rng(20 + s)) * 200.0 + 50.0 * s
        pos = corner_positions(8, 32, 48, 16, seed=s)
        level = vm.laplacian_pyramid(frames.to(DEV))[0]
        lap = torch.from_numpy(su.pyramid(frames.numpy())[0])
        bound = torch.from_numpy(su.level_bounds(frames.numpy())[1])
        assert bool(((level.cpu().double() - lap).abs() <= bound).all())
        dev_rows = vm.swd_descriptors(level, pos)
        assert torch.equal(dev_rows.cpu(), vm.swd_descriptors(level.cpu(), pos))
        sets.append(dev_rows)
    got = vm.sliced_wasserstein(sets[0], sets[1], 1, generator=_rng(6))
    _held(got, sets[0].cpu().numpy(), sets[1].cpu().numpy(), 1, 6, "32 x 48, one plane")
    raw = vm.sliced_wasserstein(sets[0], sets[1], 1, generator=_rng(6), normalize=False)
    _held(raw, sets[0].cpu().numpy(), sets[1].cpu().numpy(), 1, 6, "32 x 48, one plane, not normalised", normalize=False)
    for value in (3.0, 0.1):
        constant = torch.full((128, 49), value, device=DEV)
        assert math.isnan(vm.sliced_wasserstein(constant, sets[1], 1, generator=_rng(6)))
    with pytest.raises(ValueError, match="rows"):
        vm.sliced_wasserstein(sets[0], sets[1][:100], 1)


@pytest.mark.parametrize("name", ["SWD", "SWVD"])
def test_classes_on_the_device_agree_with_their_cpu_run(name, monkeypatch):
    """Equal seeds, the same images (the stub generator draws on the host): the device run (fp32 pyramid, gather, kernels) against
    the CPU run (float64 statement on fp32-rounded rows), per level within the bound of the CPU run's sets."""
    vm = _vm()
    frames = {"SWD": 1, "SWVD": 3}[name]       # (one frame: the CPU run's latents advance the host generator the time step is drawn from)
    dataset = stub_dataset(3, 4, frames=frames)
    seen = []
    inner = vm.sliced_wasserstein

    def recording(real, fake, planes, repeats, directions, generator):
        state = generator.get_state()
        value = inner(real, fake, planes, repeats, directions, generator)
        if not real.is_cuda:
            seen.append((real.numpy(), fake.numpy(), planes, state, value))
        return value

    monkeypatch.setattr(vm, "sliced_wasserstein", recording)
    scores = {}
    for device in ("cpu", DEV):
        torch.manual_seed(0)
        metric = getattr(vm, name)(device=device, batch_size=4, data_samples=8, descriptors_per_image=16, no_rfp=True,
                                   generator=_rng(3))
        scores[device] = metric(generator=StubGenerator(frames=frames, seed=5), dataset=dataset)
        assert metric.rows_real[0][0].device.type == torch.device(device).type
    flat = lambda pair: [getattr(s, f) for s in pair for f in s._fields[1:]]
    assert scores["cpu"][0]._fields == scores[DEV][0]._fields == ("mean", "r32", "r16") and len(seen) == 4
    for (real, fake, planes, state, value), cpu, dev in zip(seen, flat(scores["cpu"]), flat(scores[DEV])):
        gen = torch.Generator()
        gen.set_state(state)
        dirs = vm.swd_directions(planes * 49, 4, 128, gen).numpy()
        limit = su.score_bound(real, fake, planes, dirs, value)
        print(f"{name}: cpu {cpu:.9f}, device {dev:.9f}, difference {abs(cpu - dev):.3e}, bound {limit:.3e}")
        assert cpu == value and abs(cpu - dev) <= limit and limit < 2e-2 * value
