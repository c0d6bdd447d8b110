"""Metric inputs on the host (multi_stylegan_amd.validation_metrics.metric_inputs; reference validation_metrics.py:44-52,
589-590, 941-943): the float64 statement of tests/metric_input_util.py against torch's own anti-aliased resize, the host path of
``metric_inputs`` against that statement, the argument errors, and the frame draw of the metric classes."""
import pytest
import torch
import torch.nn.functional as F

import metric_input_util as mu


@pytest.mark.parametrize("src,dst", mu.RESIZE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_statement_is_torchs_antialiased_bilinear_resize(src, dst):
    x = torch.rand(2, 3, *src, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = F.interpolate(x, size=dst, mode="bilinear", align_corners=False, antialias=True)
    err = float((mu.resize(x, dst) - want).abs().max())
    print(f"{src} -> {dst}: {err:.3g}")
    assert err <= 1e-12


def test_statement_special_cases():
    x = torch.rand(1, 1, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    assert torch.equal(mu.resize(x, (16, 16)), x)                            # equal size: weights (1, 0), an exact copy
    assert mu.max_taps(7, 13) == 2 and mu.max_taps(16, 16) == 1 and mu.max_taps(20, 5) == 8 and mu.max_taps(64, 8) == 16


@pytest.mark.parametrize("n_in,n_out", [(256, 299), (256, 224), (512, 299), (7, 13), (13, 7), (20, 5), (64, 8), (16, 16), (17, 31)])
def test_package_weights_are_the_statements_rounded_once(n_in, n_out):
    from multi_stylegan_amd import validation_metrics as vm
    got, want = vm._resize_weights(n_in, n_out), mu.axis_weights(n_in, n_out)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert float((got.double() - want).abs().max()) <= 2.0 ** -24           # weights are <= 1: half an ulp at most
    assert torch.equal(got > 0, want > 1e-6)                                 # the taps differ at weights below 1e-6 only


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("t", [0, 2, None])
@pytest.mark.parametrize("normalize", ["source", "resized", None])
@pytest.mark.parametrize("src,dst", [((13, 20), (7, 9)), ((7, 9), (13, 20)), ((20, 12), (5, 9)), ((16, 16), None)],
                         ids=lambda s: "same" if s is None else f"{s[0]}x{s[1]}")
def test_host_path_matches_the_statement(src, dst, normalize, t, planes):
    from multi_stylegan_amd import validation_metrics as vm
    x = mu.frames(2, 3, 3, *src, seed=3)
    size_out = src if dst is None else dst
    for channel in range(3):
        got = vm.metric_inputs(x, channel, t=t, size=dst, normalize=normalize, planes=planes)
        want, spread = mu.reference(x, channel, t, dst, normalize, planes)
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert got.shape == want.shape == (2, planes, 1 if t is not None else 3, *size_out)
        sel = x[:, channel] if t is None else x[:, channel, t:t + 1]
        for b in range(2):
            peak = float(sel[b].abs().max())
            if normalize is None:
                bound = mu.none_bound(src, size_out, peak)
            else:
                assert float(spread[b]) >= 0.1
                bound = mu.normalised_bound(src, size_out, peak, float(spread[b]))
            err = float((got[b].double() - want[b]).abs().max())
            assert err <= bound, (channel, b, err, bound)
        if normalize is not None:
            assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    if dst is None and normalize is None:
        assert torch.equal(vm.metric_inputs(x, 1, t=t, normalize=None, planes=planes)[:, 0], x[:, 1] if t is None else x[:, 1, t:t + 1])


def test_host_path_dtypes_and_degenerate_samples():
    from multi_stylegan_amd import validation_metrics as vm
    x = mu.frames(2, 2, 3, 9, 11, seed=4)
    got = vm.metric_inputs(x.double(), 1, t=1, size=(5, 6), dtype=torch.float64)
    assert got.dtype == torch.float64 and torch.equal(got, vm.metric_inputs(x, 1, t=1, size=(5, 6)).double())
    xb = x.to(torch.bfloat16)
    want, _ = mu.reference(xb, 0, None, (12, 7), "resized")
    got = vm.metric_inputs(xb, 0, size=(12, 7), normalize="resized", dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16 and float((got.double() - want).abs().max()) <= 2.0 ** -7
    # a constant sample: 0 / 0.  (Behind a resize only the constant 0 stays constant: a filter's weights sum to 1 up to rounding,
    #  in any floating-point resize, torch's and the float64 statement included.)
    x[1, 1, 2, 3, 4] = float("nan")
    for normalize, constant in (("source", 0.5), ("resized", 0.0)):
        x[0] = constant
        got = vm.metric_inputs(x, 1, size=(5, 6), normalize=normalize)
        assert bool(got.isnan().all())
        got = vm.metric_inputs(x, 0, size=(5, 6), normalize=normalize)       # channel 0 of sample 1 holds no NaN
        assert bool(got[0].isnan().all()) and not bool(got[1].isnan().any())


def test_argument_errors():
    from multi_stylegan_amd import validation_metrics as vm
    x = torch.rand(2, 3, 3, 8, 8)
    for kwargs in (dict(channel=3), dict(channel=-1), dict(channel=0, t=3), dict(channel=0, t=-1), dict(channel=0, planes=2),
                   dict(channel=0, normalize="batch"), dict(channel=0, size=(0, 8)), dict(channel=0, size=(8, -1))):
        with pytest.raises(ValueError):
            vm.metric_inputs(x, **kwargs)
    with pytest.raises(ValueError, match="B, C, T, H, W"):
        vm.metric_inputs(x[0], 0)
    assert "metric_inputs" in vm.__all__ and "select_frames" in vm.__all__


class _Seen(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x):
        self.seen.append(x)
        return x.flatten(1)[:, :4]


def test_metric_classes_draw_like_select_frames_and_resize():
    """One ``torch.randint`` draw from the global CPU generator per selected batch, in the order of ``select_frames``: equal
    seeds keep giving equal frame choices; ``input_size`` resizes behind (FID, FVD) or in front of (IS) the normalisation."""
    from multi_stylegan_amd import misc, validation_metrics as vm
    x = mu.frames(2, 2, 3, 8, 8, seed=5)
    fid = vm.FID(_Seen(), device="cpu")
    torch.manual_seed(11)
    got = [fid._inputs(x, c) for c in (0, 1, 0)]
    state = torch.get_rng_state()
    torch.manual_seed(11)
    want = [misc.normalize_m1_1_batch(vm.select_frames(x, c))[:, :, 0] for c in (0, 1, 0)]
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(state, torch.get_rng_state())
    assert torch.equal(vm.FVD(_Seen(), device="cpu")._inputs(x, 1), misc.normalize_m1_1_batch(vm.select_clips(x, 1)))
    assert torch.equal(state, torch.get_rng_state())                         # a clip draws nothing

    torch.manual_seed(12)
    t = int(torch.randint(0, 3, (1,)))
    for metric, normalize, size in ((vm.FID(_Seen(), device="cpu", input_size=(12, 10)), "source", (12, 10)),
                                    (vm.IS(_Seen(), device="cpu", input_size=(12, 10)), "resized", (12, 10))):
        torch.manual_seed(12)
        got = metric._inputs(x, 1) if normalize == "source" else metric._preprocessing(x, 1)
        want, spread = mu.reference(x, 1, t, size, normalize)
        assert got.shape == (2, 3, 12, 10)
        for b in range(2):
            bound = mu.normalised_bound((8, 8), size, float(x[b, 1, t].abs().max()), float(spread[b]))
            assert float((got[b].double() - want[b, :, 0]).abs().max()) <= bound
    got = vm.FVD(_Seen(), device="cpu", input_size=(6, 5))._inputs(x, 0)
    want, spread = mu.reference(x, 0, None, (6, 5), "source")
    assert got.shape == (2, 3, 3, 6, 5)
    for b in range(2):
        assert float((got[b].double() - want[b]).abs().max()) <= mu.normalised_bound((8, 8), (6, 5), float(x[b, 0].abs().max()),
                                                                                     float(spread[b]))
