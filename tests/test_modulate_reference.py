"""tests/modulate_util.py is the yardstick of tests/test_hip_modulate.py, so it is checked here against the project's CPU
oracle first (oracle.ops.modulated_conv2d, float64, autograd): the modulated weights, the fold of a per-sample weight gradient
into weight and style gradients, and the second derivative the path-length regulariser takes of it."""
import pytest
import torch

import modulate_util as mu
from conftest import rel_err

B, I, O, HW = 3, 8, 5, 6


def _conv_case(k, demod):
    from oracle import ops as oo
    gen = torch.Generator().manual_seed(10 * k + demod)
    x = mu.draw(gen, B, I, HW, HW)
    W = mu.draw(gen, 1, O, I, k, k).requires_grad_(True)
    s = mu.draw(gen, B, I, mean=1.0, std=0.5).requires_grad_(True)
    gy = mu.draw(gen, B, O, HW, HW)
    v = mu.draw(gen, B, I)
    y = oo.modulated_conv2d(x, W, s, demodulate=demod, upsample=False)
    gW, gs = torch.autograd.grad(y, (W, s), gy, create_graph=True)
    # per-sample weight gradient of the plain convolution, [B,O,T,I] as the kernels lay it out
    g = torch.stack([torch.nn.grad.conv2d_weight(x[b:b + 1], (O, I, k, k), gy[b:b + 1], padding=k // 2)
                     for b in range(B)]).reshape(B, O, I, k * k).permute(0, 1, 3, 2).contiguous()
    return x, W, s, gy, v, g, gW, gs


@pytest.mark.parametrize("demod", [True, False], ids=["demod", "nodemod"])
@pytest.mark.parametrize("k", [3, 1], ids=["3x3", "1x1"])
def test_fold_matches_oracle_autograd(k, demod):
    x, W, s, gy, v, g, gW, gs = _conv_case(k, demod)
    W3, scale = W.detach().reshape(O, I, k * k), mu.conv_scale(I, k * k)
    fW, fs = mu.fold(W3, s.detach(), g, scale, demod)
    assert rel_err(fW, gW.detach().reshape(O, I, k * k)) < 1e-12
    assert rel_err(fs.sum(0), gs.detach()) < 1e-12


@pytest.mark.parametrize("demod", [True, False], ids=["demod", "nodemod"])
@pytest.mark.parametrize("k", [3, 1], ids=["3x3", "1x1"])
def test_fold2_matches_oracle_double_autograd(k, demod):
    """d/dW, d/ds of <v, gs> with the conv operands x and gy held fixed (the convolution is linear in its weights, so its
    per-sample weight gradient g depends on neither W nor s)."""
    x, W, s, gy, v, g, gW, gs = _conv_case(k, demod)
    hW, hs = torch.autograd.grad((v * gs).sum(), (W, s), allow_unused=True)
    W3, scale = W.detach().reshape(O, I, k * k), mu.conv_scale(I, k * k)
    fW, fs = mu.fold2(W3, s.detach(), g, v, scale, demod)
    assert rel_err(fW, hW.reshape(O, I, k * k)) < 1e-12
    if demod:
        assert rel_err(fs.sum(0), hs) < 1e-12
    else:
        assert hs is None or float(hs.abs().max()) == 0.0
        assert float(fs.abs().max()) == 0.0


@pytest.mark.parametrize("demod", [True, False], ids=["demod", "nodemod"])
@pytest.mark.parametrize("k", [3, 1], ids=["3x3", "1x1"])
def test_weights_match_oracle_modulated_weights(k, demod):
    """The oracle does not hand out its per-sample weights; a unit impulse in input channel i at the centre of a k x k map
    reads them off its output, y[b,o,p,q] = w[b,o,i,k-1-p,k-1-q]."""
    from oracle import ops as oo
    gen = torch.Generator().manual_seed(7 + k)
    W = mu.draw(gen, 1, O, I, k, k)
    s = mu.draw(gen, B, I, mean=1.0, std=0.5)
    w, d = mu.weights(W.reshape(O, I, k * k), s, mu.conv_scale(I, k * k), demod)
    assert d.shape == (B, O) and (demod or bool((d == 1).all()))
    got = torch.empty(B, O, I, k, k, dtype=torch.float64)
    for i in range(I):
        x = torch.zeros(B, I, k, k, dtype=torch.float64)
        x[:, i, k // 2, k // 2] = 1.0
        got[:, :, i] = oo.modulated_conv2d(x, W, s, demodulate=demod, upsample=False).flip(-1, -2)
    assert rel_err(w.reshape(B, O, I, k, k), got) < 1e-12


FP32_CASES = [(16, 6, 512, 9), (5, 3, 40, 1), (1, 5, 4, 4), (7, 4, 260, 9), (3, 5, 6, 3)]


@pytest.mark.parametrize("demod", [True, False], ids=["demod", "nodemod"])
@pytest.mark.parametrize("shape", FP32_CASES, ids=["B%d-O%d-I%d-T%d" % c for c in FP32_CASES])
def test_float32_evaluation_is_at_rounding_level(shape, demod):
    """The bounds of tests/test_hip_modulate.py are multiples of the error of this same code run in float32, so that error
    has to be a rounding error: with the test distributions (styles randn * 0.5 + 1; W, g, v randn; scale = sqrt(2 / (I T)))
    the references are O(0.02 to 5) and the cases well conditioned.  max|f32 - f64| / max|f64|, measured on the CPU:
        (B,O,I,T)      demodulated: gW       gs_by_o  hW       hs_by_o    without: gW       gs_by_o  hW       (hs = 0)
        (16,6,512,9)                1.69e-07 1.45e-07 1.75e-07 3.82e-07            2.16e-07 1.00e-07 1.82e-07
        (5,3,40,1)                  1.24e-07 1.06e-07 1.20e-07 2.12e-07            6.81e-08 5.95e-08 8.19e-08
        (1,5,4,4)                   8.65e-08 1.36e-07 2.05e-07 2.37e-07            4.97e-08 9.25e-08 3.70e-08
        (7,4,260,9)                 1.29e-07 1.51e-07 1.42e-07 1.75e-07            1.04e-07 1.29e-07 1.07e-07
        (3,5,6,3)                   8.33e-08 2.80e-07 1.02e-07 3.19e-07            5.88e-08 4.52e-08 9.68e-08
    -- one to three float32 units in the last place (2^-23 = 1.2e-7); the sums are threaded, so the last digit moves from run
    to run.  Held here to 2^-20 = 9.5e-7, eight units: anything above that would be cancellation, not rounding."""
    b, o, i, t = shape
    gen = torch.Generator().manual_seed(sum(shape))
    W, s = mu.draw(gen, o, i, t), mu.draw(gen, b, i, mean=1.0, std=0.5)
    g, v = mu.draw(gen, b, o, t, i), mu.draw(gen, b, i)
    scale = mu.conv_scale(i, t)
    ref = mu.fold(W, s, g, scale, demod) + mu.fold2(W, s, g, v, scale, demod)
    f32 = mu.fold(W.float(), s.float(), g.float(), scale, demod) + mu.fold2(W.float(), s.float(), g.float(), v.float(), scale, demod)
    errs = [rel_err(a, r) for a, r in zip(f32, ref)]
    print(shape, "demod" if demod else "nodemod", " ".join("%.2e" % e for e in errs))
    assert max(errs) < 2.0 ** -20
