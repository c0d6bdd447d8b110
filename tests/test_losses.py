"""The Wasserstein and hinge loss families, their CutMix forms and R2 on CPU tensors (the plain-torch composite the modules use
where the gfx950 kernel does not apply) against tests/golden/losses.npz, which tools/gen_golden_losses.py recorded from the
reference's own modules.  The kernel itself: tests/test_hip_losses.py."""
import math
import re

import pytest
import torch

import losses_util as lu

NEW = ("WassersteinDiscriminatorLoss", "WassersteinDiscriminatorLossCutMix", "WassersteinGeneratorLoss", "HingeGeneratorLoss",
       "HingeDiscriminatorLoss", "HingeDiscriminatorLossCutMix", "R2Regularization")


def test_the_seven_classes_are_exported():
    import multi_stylegan_amd as m
    from multi_stylegan_amd import loss
    for name in NEW:
        assert name in m.__all__ and getattr(m, name) is getattr(loss, name) and issubclass(getattr(m, name), torch.nn.Module)
    assert issubclass(loss.HingeGeneratorLoss, loss.WassersteinGeneratorLoss)
    assert loss.HingeGeneratorLoss is not loss.WassersteinGeneratorLoss


def _module(family, form):
    from multi_stylegan_amd import loss
    return getattr(loss, lu.CLASSES[family][{"disc": 0, "cutmix": 1, "gen": 2}[form]])()


def _call(module, form, real, fake, weight, label):
    if form == "disc":
        return module(real, fake, weight) if weight is not None else module(real, fake)
    if form == "gen":
        return (module(real, weight=weight) if weight is not None else module(real),)
    return module(real, label)


@pytest.mark.parametrize("family", lu.FAMILIES)
@pytest.mark.parametrize("case", ["s", "m", "l"])
def test_modules_on_cpu_match_the_reference(case, family):
    """Values within 1e-6 mean|term| of the reference's fp32 results (the same arithmetic up to the order of a few roundings and
    of the mean's summation); gradients, under the cotangents (0.7, -1.3), to 2e-6 relative (products of at most four fp32
    roundings, 4 x 6e-8; case l against the float64 record, which adds one more), exact zeros where the reference has
    zeros, and -1/2 / +1/2 of the active slope at the hinge's ties."""
    data, man = lu.fixtures()
    c_real, c_fake = man["cotangents"]
    for form, aux in lu.forms(case, man):
        key = f"{case}.{family}.{form}.{aux}"
        real, fake, weight, label = lu.operands(data, case, form, aux)
        real = real.clone().requires_grad_(True)
        fake = None if fake is None else fake.clone().requires_grad_(True)
        out = _call(_module(family, form), form, real, fake, weight, label)
        assert all(v.dtype == torch.float32 and v.ndim == 0 for v in out), key
        want, scale = data[key + ".f32.loss"], data[key + ".f32.absmean"]
        for got, w, s in zip(out, want, scale):
            assert abs(got.item() - w.item()) <= 1e-6 * s.item(), (key, got.item(), w.item(), s.item())
        sum(c * v for c, v in zip((c_real, c_fake), out)).backward()
        prec = "f32" if key + ".f32.grad_real" in data else "f64"
        for name, leaf in (("grad_real", real), ("grad_fake", fake)):
            if leaf is None:
                continue
            ref = data[f"{key}.{prec}.{name}"]
            assert leaf.grad.shape == ref.shape
            assert lu.worst_rel(leaf.grad, ref) <= 2e-6, (key, name, lu.worst_rel(leaf.grad, ref))
            assert lu.zeros_kept(leaf.grad, ref), (key, name)


def test_hinge_ties_get_half_the_slope():
    from multi_stylegan_amd import loss
    real = torch.tensor([[1.0], [0.0], [2.0], [1.0]], requires_grad=True)
    fake = torch.tensor([[-1.0], [0.0], [-2.0], [-1.0]], requires_grad=True)
    l_real, l_fake = loss.HingeDiscriminatorLoss()(real, fake)
    (l_real + l_fake).backward()
    assert real.grad.reshape(-1).tolist() == [-0.125, -0.25, 0.0, -0.125]
    assert fake.grad.reshape(-1).tolist() == [0.125, 0.25, 0.0, 0.125]
    both = torch.tensor([[1.0], [-1.0], [1.0], [-1.0]], requires_grad=True)
    label = torch.tensor([[1.0], [1.0], [0.0], [0.0]])
    l_real, l_fake = loss.HingeDiscriminatorLossCutMix()(both, label)
    (l_real + l_fake).backward()
    assert both.grad.reshape(-1).tolist() == [-0.125, -0.25, 0.25, 0.125]


@pytest.mark.parametrize("family", lu.FAMILIES)
def test_nan_in_gives_nan_out(family):
    """torch.minimum keeps a NaN (fminf would drop it): the trainer's finiteness checks rely on it."""
    real, fake = torch.tensor([[0.5], [float("nan")], [2.0]]), torch.tensor([[0.25], [float("nan")]])
    assert all(math.isnan(v.item()) for v in _module(family, "disc")(real, fake))
    assert math.isnan(_module(family, "gen")(real).item())
    assert all(math.isnan(v.item()) for v in _module(family, "cutmix")(real, torch.tensor([[1.0], [1.0], [0.0]])))
    clean = _module(family, "disc")(real[:1], fake)
    assert math.isfinite(clean[0].item()) and math.isnan(clean[1].item())


def test_modules_take_other_dtypes_and_odd_weight_maps_through_the_composite():
    """float64 stays float64, bf16 / fp16 come back as fp32, and a weight map that does not cover the prediction's last two
    dimensions broadcasts as the reference's multiply does."""
    from multi_stylegan_amd import loss
    x, y = torch.linspace(-2, 2, 12).reshape(3, 1, 2, 2), torch.linspace(-1, 3, 8).reshape(2, 1, 2, 2)
    a = loss.HingeDiscriminatorLoss()(x.double(), y.double())
    b = loss.HingeDiscriminatorLoss()(x.bfloat16(), y.bfloat16())
    assert a[0].dtype == torch.float64 and b[0].dtype == torch.float32 and abs(a[1].item() - b[1].item()) < 1e-2
    w = torch.tensor([[0.5], [2.0]])                                     # [2, 1] against [.., 2, 2]: broadcasts over the last axis
    got = loss.WassersteinGeneratorLoss()(x, weight=w)
    assert torch.allclose(got, -(x * w.view(1, 1, 1, 2, 1)).mean())


def test_r2_regularization():
    """What the reference's R2 states (its own forward raises: PARITY UNPINNED): 0.5 mean_b sum (d sum prediction / d image)^2."""
    from multi_stylegan_amd import loss
    image = torch.linspace(-1.0, 2.0, 2 * 3 * 4 * 5).reshape(2, 3, 4, 5).requires_grad_(True)
    prediction = image.pow(2).sum(1)
    r2 = loss.R2Regularization()(prediction, image)
    want = 0.5 * (4.0 * image.detach().pow(2)).reshape(2, -1).sum(1).mean()
    assert abs(r2.item() - want.item()) <= 1e-6 * want.item()
    r1 = loss.R1Regularization()(image.pow(2).sum(1), image)
    assert torch.equal(r1, r2)
    r2.backward()
    assert image.grad is not None and torch.allclose(image.grad, 4.0 * image.detach() / 2, rtol=1e-6)


def test_header_declares_the_entries_and_the_binding_has_them():
    from multi_stylegan_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in ("msg_gan_loss", "msg_gan_loss_backward", "msg_gan_loss_workspace"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib._SIGNATURES["msg_gan_loss_workspace"][0] is _lib._L
    assert (_lib.MSG_GAN_LOGISTIC, _lib.MSG_GAN_WASSERSTEIN, _lib.MSG_GAN_HINGE) == (0, 1, 2)
    assert (_lib.MSG_GAN_AUX_NONE, _lib.MSG_GAN_AUX_WEIGHT, _lib.MSG_GAN_AUX_LABEL) == (0, 1, 2)
    assert _lib.ABI_VERSION == 5
