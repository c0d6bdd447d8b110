"""The fused adversarial-loss kernel pair (csrc/gan_loss.hip, op_static/gan_loss.py) on the GPU: against tests/golden/losses.npz
(recorded from the reference's modules), against the float64 composite at ragged and multi-workgroup sizes, run-to-run
determinism, double backward, error paths, and through the tiny discriminator and ModelWrapper with the hinge and Wasserstein
families.  Tolerances (all relative errors are element-wise, references below the smallest normal fp32 number measured against
that number):
  values        |got - ref64| <= 1e-5 mean|term|  (blocked fp32 summation; a one-thread serial sum of 98 304 terms would not hold it)
  fp32 grads    2e-6 (Wasserstein, hinge: products of at most four fp32 roundings), 1e-5 (logistic: the exponential)
  bf16 grads    one bf16 unit in the last place of the float64 gradient at the bf16-rounded predictions
  zeros         exact where the reference's gradient is exactly zero (inactive hinge elements, label-masked pixels)
Every test prints the worst errors it measured (pytest -s)."""
import json
import math

import pytest
import torch

import losses_util as lu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_TOL = {"logistic": 1e-5, "wasserstein": 2e-6, "hinge": 2e-6}
COT = (0.7, -1.3)


def _fused(real, fake, kind, weight=None, label=None):
    """gan_loss on the given device tensors (their storage, at its alignment) -> (out [2], grad_real, grad_fake) under COT."""
    from multi_stylegan_amd.op_static.gan_loss import gan_loss
    real = None if real is None else real.detach().requires_grad_(True)
    fake = None if fake is None else fake.detach().requires_grad_(True)
    out = gan_loss(real, fake, kind=kind, weight=weight, label=label)
    assert out.dtype == torch.float32 and out.shape == (2,) and out.is_cuda
    (COT[0] * out[0] + COT[1] * out[1]).backward()
    return out.detach(), None if real is None else real.grad, None if fake is None else fake.grad


def _check(tag, got, ref, kind, dtype, worst):
    """got = _fused(...), ref = dict(loss, absmean, grad_real, grad_fake) in float64."""
    out, g_real, g_fake = got
    for side in range(len(ref["loss"])):
        err = abs(out[side].item() - ref["loss"][side].item())
        scale = ref["absmean"][side].item()
        worst["value"] = max(worst["value"], err / scale if scale > 0 else err)
        assert err <= 1e-5 * scale, (tag, side, out[side].item(), ref["loss"][side].item(), scale)
    for name, g in (("grad_real", g_real), ("grad_fake", g_fake)):
        want = ref.get(name)
        if want is None:
            continue
        assert g.dtype == dtype and g.shape == want.shape, (tag, name)
        assert lu.zeros_kept(g, want), (tag, name)
        if dtype == torch.float32:
            e = lu.worst_rel(g, want)
            worst["grad_fp32_" + kind] = max(worst.get("grad_fp32_" + kind, 0.0), e)
            assert e <= GRAD_TOL[kind], (tag, name, e)
        else:
            e = lu.bf16_ulps(g, want)
            worst["grad_bf16_ulp"] = max(worst.get("grad_bf16_ulp", 0.0), e)
            assert e <= 1.0, (tag, name, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", lu.FAMILIES)
def test_kernel_matches_the_reference_fixtures(family, dtype):
    """Every case, form and aux mode of losses.npz (its predictions are exact in bf16, so the float64 record serves both
    dtypes)."""
    data, man = lu.fixtures()
    worst = {"value": 0.0}
    for case in man["cases"]:
        for form, aux in lu.forms(case, man):
            key = f"{case}.{family}.{form}.{aux}"
            real, fake, weight, label = lu.operands(data, case, form, aux)
            kind = "wasserstein" if (family, form) == ("hinge", "gen") else family   # the generator's hinge loss IS its Wasserstein loss
            got = _fused(real.to(DEV, dtype), None if fake is None else fake.to(DEV, dtype), kind,
                         None if weight is None else weight.to(DEV), None if label is None else label.to(DEV))
            ref = {"loss": data[key + ".f64.loss"], "absmean": data[key + ".f64.absmean"],
                   "grad_real": data[key + ".f64.grad_real"], "grad_fake": data.get(key + ".f64.grad_fake")}
            if form == "cutmix":
                ref["grad_fake"] = None
            _check(key, got, ref, kind, dtype, worst)
            if form == "gen":
                assert got[0][1].item() == 0.0                               # the absent side
    print("gan_loss fixtures", family, dtype, json.dumps(worst))


def _ragged(name):
    """Seeded operands (real, fake, weight, label), fp32 on the CPU."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def pred(*shape):
        x = torch.randn(*shape, generator=g) * 2.0
        flat = x.reshape(-1)
        flat[0] = 1.0
        flat[-1] = -1.0
        return x
    if name == "n1":
        return pred(1), pred(1), None, None
    if name == "5x1":
        return pred(5, 1), pred(3, 1), None, None
    if name == "odd":                                                        # 13 653 elements: odd, two workgroups, a ragged tail
        return pred(3, 1, 37, 41) * 3.0, pred(3, 1, 37, 41), None, None
    if name == "odd_weight":                                                 # P = 1517 divides nothing
        return pred(3, 1, 37, 41), pred(3, 1, 37, 41), torch.rand(37, 41, generator=g) * 2.0, None
    if name == "big_weight":                                                 # 98 304 elements, 48 workgroups, vector weight loads
        return pred(2, 1, 3, 128, 128), pred(2, 1, 3, 128, 128), torch.rand(128, 128, generator=g) * 2.0, None
    if name == "label":
        return pred(3, 1, 37, 41), None, None, (torch.rand(3, 1, 37, 41, generator=g) > 0.4).float()
    if name == "unequal":
        return pred(4, 1, 37, 41), pred(5, 1, 37, 41), None, None
    if name == "unequal_weight":
        return pred(4, 1, 37, 41), pred(5, 1, 37, 41), torch.rand(37, 41, generator=g) + 0.5, None
    if name == "real_only":
        return pred(3, 1, 37, 41), None, None, None
    if name == "fake_only":
        return None, pred(2, 1, 3, 8, 8), None, None
    raise KeyError(name)


RAGGED = ["n1", "5x1", "odd", "odd_weight", "big_weight", "label", "unequal", "unequal_weight", "real_only", "fake_only"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", RAGGED)
def test_ragged_and_multi_workgroup_shapes(name, dtype):
    """n = 1, odd element counts (the scalar tail of the 16-byte path, for bf16 a tail of up to seven), more than one
    workgroup, a weight map whose size divides nothing, unequal sides, an absent side: against the composite in float64 on
    the CPU, evaluated at the values the kernel sees (the bf16-rounded ones for bf16)."""
    real, fake, weight, label = _ragged(name)
    dev = [None if t is None else t.to(DEV, dtype) for t in (real, fake)]
    worst = {"value": 0.0}
    for kind in lu.FAMILIES:
        got = _fused(dev[0], dev[1], kind, None if weight is None else weight.to(DEV), None if label is None else label.to(DEV))
        ref = lu.composite64(dev[0], dev[1], kind, weight, label, COT)
        if dev[0] is None:
            assert got[0][0].item() == 0.0
        if dev[1] is None and label is None:
            assert got[0][1].item() == 0.0
        _check((name, kind), got, ref, kind, dtype, worst)
    print("gan_loss ragged", name, dtype, json.dumps(worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_results_are_bit_identical_from_run_to_run_and_across_alignments(dtype):
    """Forward and backward twice on the 98 304-element case; and the same values at a base address that is not 16-byte
    aligned (the scalar-load path), whose sums are added in the same order."""
    real, fake, weight, _ = _ragged("big_weight")
    real, fake, weight = real.to(DEV, dtype), fake.to(DEV, dtype), weight.to(DEV)
    for kind in lu.FAMILIES:
        for w in (None, weight):
            a, b = _fused(real, fake, kind, w), _fused(real, fake, kind, w)
            assert all(torch.equal(u, v) for u, v in zip(a, b)), kind
            shifted = [torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].reshape(t.shape) for t in (real, fake)]
            assert all(t.data_ptr() % 16 != 0 and t.is_contiguous() for t in shifted)
            c = _fused(shifted[0], shifted[1], kind, w)
            assert all(torch.equal(u, v) for u, v in zip(a, c)), kind
        lab = (real > 0).float()
        a, b = _fused(real, None, kind, label=lab), _fused(real, None, kind, label=lab)
        assert all(torch.equal(u, v) for u, v in zip(a[:2], b[:2])), kind


def test_logistic_kind_matches_the_existing_logistic_modules():
    from multi_stylegan_amd import loss
    real, fake, weight, _ = _ragged("odd_weight")
    real, fake, weight = (real * 3).to(DEV), (fake * 3).to(DEV), weight.to(DEV)
    label = (real > 0.5).float()
    worst = {"value": 0.0, "grad": 0.0}

    def compare(got, want_losses, leaves):
        sum(c * v for c, v in zip(COT, want_losses)).backward()
        for side, want in enumerate(want_losses):                            # (terms are non-negative: mean|term| is the loss)
            err = abs(got[0][side].item() - want.item()) / want.item()
            worst["value"] = max(worst["value"], err)
            assert err <= 1e-5
        for g, leaf in zip(got[1:], leaves):
            e = lu.worst_rel(g, leaf.grad)
            worst["grad"] = max(worst["grad"], e)
            assert e <= 1e-5, e

    for w in (None, weight):
        r, f = real.clone().requires_grad_(True), fake.clone().requires_grad_(True)
        compare(_fused(real, fake, "logistic", w), loss.NonSaturatingLogisticDiscriminatorLoss()(r, f, w), (r, f))
        f = fake.clone().requires_grad_(True)
        compare(_fused(fake, None, "logistic", w), (loss.NonSaturatingLogisticGeneratorLoss()(f, w),), (f,))
    r = real.clone().requires_grad_(True)
    compare(_fused(real, None, "logistic", label=label), loss.NonSaturatingLogisticDiscriminatorLossCutMix()(r, label), (r,))
    print("gan_loss vs logistic modules", json.dumps(worst))


@pytest.mark.parametrize("kind", ["hinge", "logistic"])
def test_double_backward_goes_through_the_composite(kind):
    """A gradient penalty through the loss: predictions = theta * u, first derivative with respect to u under create_graph, its
    contraction with a fixed tensor differentiated again with respect to theta and u -- fused against composite, 1e-5."""
    from multi_stylegan_amd.op_static import gan_loss as op
    real, fake, weight, _ = _ragged("odd_weight")
    v = torch.randn(real.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    results = []
    for fn in (lambda r, f: op.gan_loss(r, f, kind=kind, weight=weight.to(DEV)),
               lambda r, f: torch.stack(op.composite(r, f, kind=kind, weight=weight.to(DEV)))):
        theta = torch.tensor(1.25, device=DEV, requires_grad=True)
        u, f = real.to(DEV).requires_grad_(True), fake.to(DEV).requires_grad_(True)
        out = fn(u * theta, f * theta)
        g_u, = torch.autograd.grad(COT[0] * out[0] + COT[1] * out[1], u, create_graph=True)
        assert g_u.requires_grad
        second = torch.autograd.grad((g_u * v).sum(), (theta, u), allow_unused=True)
        results.append((g_u.detach(), second[0], second[1]))
    (g_a, t_a, u_a), (g_b, t_b, u_b) = results
    assert lu.worst_rel(g_a, g_b) <= 1e-5
    assert abs(t_a.item() - t_b.item()) <= 1e-5 * abs(t_b.item()) and t_b.item() != 0.0
    if kind == "logistic":                                                   # (the hinge is piecewise linear: no second derivative in u)
        scale = u_b.abs().max().item()
        assert scale > 0 and (u_a - u_b).abs().max().item() <= 1e-5 * scale


def test_error_paths():
    from multi_stylegan_amd import _lib, loss
    from multi_stylegan_amd.op_static.gan_loss import gan_loss
    x = torch.randn(3, 1, 4, 4)
    with pytest.raises(_lib.MsgHipError):
        gan_loss(x, x, kind="hinge")                                         # CPU tensors
    with pytest.raises(_lib.MsgHipError):
        gan_loss(x.to(DEV), x.to(DEV).bfloat16(), kind="hinge")              # mismatched dtypes
    with pytest.raises(_lib.MsgHipError):
        gan_loss(x.to(DEV).double(), None, kind="hinge")
    with pytest.raises(_lib.MsgHipError):
        gan_loss(x.to(DEV), None, kind="hinge", label=torch.ones(3, 1, 4, 3, device=DEV))
    with pytest.raises(_lib.MsgHipError):
        gan_loss(x.to(DEV), None, kind="hinge", weight=torch.ones(4, 3, device=DEV))
    with pytest.raises(_lib.MsgHipError):
        gan_loss(x.to(DEV), None, kind="least-squares")
    # the C entries: never a silent no-op
    lib, out = _lib.lib(), torch.zeros(2, device=DEV)
    xd = x.to(DEV)
    args = (xd.data_ptr(), None, None, out.data_ptr())
    assert lib.msg_gan_loss(*args, 7, 0, 0, 48, 0, 0, None, 0, 0) == _lib.MSG_EINVAL          # dtype
    assert lib.msg_gan_loss(*args, 0, 3, 0, 48, 0, 0, None, 0, 0) == _lib.MSG_EINVAL          # kind
    assert lib.msg_gan_loss(*args, 0, 0, 1, 48, 0, 16, None, 0, 0) == _lib.MSG_EINVAL         # a weight mode without a map
    assert lib.msg_gan_loss(None, None, None, out.data_ptr(), 0, 0, 0, 0, 0, 0, None, 0, 0) == _lib.MSG_EINVAL
    assert lib.msg_gan_loss_workspace(1 << 20, 5) > 0
    assert lib.msg_gan_loss(*args, 0, 0, 0, 1 << 20, 0, 0, None, 0, 0) == _lib.MSG_EINVAL     # needs a workspace, has none
    # the modules fall back to the composite instead of raising
    for module in (loss.HingeDiscriminatorLoss(), loss.WassersteinDiscriminatorLoss()):
        a = module(x.to(DEV).double(), x.to(DEV).double())
        assert a[0].dtype == torch.float64 and a[0].is_cuda
        b = module(x, x)
        assert not b[0].is_cuda and abs(a[0].item() - b[0].item()) < 1e-6
    odd = loss.WassersteinGeneratorLoss()(x.to(DEV), weight=torch.tensor([[0.5], [1.0], [1.5], [2.0]], device=DEV))
    assert torch.allclose(odd.cpu(), -(x * torch.tensor([0.5, 1.0, 1.5, 2.0]).view(1, 1, 4, 1)).mean(), atol=1e-6)


class _PlainHinge(torch.nn.Module):
    """Test-local hinge modules in stock torch operators (the reference's formulas)."""

    def __init__(self, form):
        super().__init__()
        self.form = form

    @staticmethod
    def _neg_min(t, w=None):
        t = torch.minimum(torch.zeros((), dtype=t.dtype, device=t.device), t)
        return -(t if w is None else t * w).mean()

    def forward(self, a, b=None, weight=None):
        if self.form == "gen":
            b, weight = None, b if weight is None else weight
        w = None if weight is None else weight.view(1, 1, 1, weight.shape[-2], weight.shape[-1]).to(a.device)
        if self.form == "gen":
            return -(a.float() if w is None else a.float() * w).mean()
        if self.form == "cutmix":
            return self._neg_min(a.float() - 1.0, b), self._neg_min(-a.float() - 1.0, 1.0 - b)
        return self._neg_min(a.float() - 1.0, w), self._neg_min(-b.float() - 1.0, w)


def _tiny(golden):
    """The tiny models of tests/golden/tiny_models.npz, built as test_hip_models._models builds them."""
    from tools.gen_golden import TINY_D, TINY_G
    import multi_stylegan_amd as m
    z = golden("tiny_models")
    g, d = m.MultiStyleGANGenerator(TINY_G), m.MultiStyleGANDiscriminator(TINY_D, no_rfp=True)
    g.load_state_dict(z.state_dict("tinyG.sd.")); d.load_state_dict(z.state_dict("tinyD.sd."))
    return z, g.to(DEV), d.to(DEV)


def test_hinge_loss_through_the_tiny_discriminator(golden):
    """Parameter gradients of the fp32 discriminator under HingeDiscriminatorLoss on both of its outputs (scalar and pixel-wise),
    fused against plain torch: norm-wise 1e-5 per parameter."""
    from multi_stylegan_amd import loss
    z, _, d = _tiny(golden)
    real = z["tinyD.x"].to(DEV)
    fake = torch.rand(real.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    grads = []
    for module in (loss.HingeDiscriminatorLoss(), _PlainHinge("disc")):
        d.zero_grad()
        (s_r, px_r), (s_f, px_f) = d(real), d(fake)
        sum(module(s_r, s_f) + module(px_r, px_f)).backward()
        grads.append({n: p.grad.clone() for n, p in d.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    worst = 0.0
    for n, ref in grads[1].items():
        norm = ref.double().norm().item()
        e = (grads[0][n].double() - ref.double()).norm().item() / (norm if norm > 0 else 1.0)
        worst = max(worst, e)
        assert e <= 1e-5, (n, e)
    print("gan_loss tiny discriminator, worst norm-wise parameter-gradient error", worst)


def _wrapper_run(golden, losses, iterations=2):
    import multi_stylegan_amd as m
    _, g, d = _tiny(golden)
    hp = dict(m.generation_hyperparameters, lazy_discriminator_regularization=2)
    trainer = m.ModelWrapper(g, d, device=DEV, hyperparameters=hp, **losses)
    gen = torch.Generator().manual_seed(77)
    bsz = 4
    before = [[p.detach().clone() for p in net.parameters()] for net in (g, d)]
    logs = []
    for _ in range(iterations):
        noise = lambda n: [torch.randn(n, 1, 4, 4, generator=gen)] + \
            [torch.randn(n, 1, 2 ** (i // 2 + 3), 2 ** (i // 2 + 3), generator=gen) for i in range(6)]
        cut = torch.zeros(1, 1, 1, 32, 32)
        cut[..., 8:24, 4:20] = 1.0
        draws = m.Draws(z_d=[torch.randn(bsz, 16, generator=gen), torch.randn(bsz, 16, generator=gen)], inject_d=2,
                        noise_d=noise(bsz), z_g=torch.randn(bsz, 16, generator=gen), noise_g=noise(bsz), cut_mix=True,
                        cut_mix_map_aug=cut, cut_mix_map_reg=1.0 - cut)
        real = torch.rand(bsz, 2, 3, 32, 32, generator=gen)
        trainer.train_iteration(real.to(DEV), draws.to(DEV))
        logs.append(trainer.pop_logs())
    moved = [sum(int(not torch.equal(a, b)) for a, b in zip(old, net.parameters())) for old, net in zip(before, (g, d))]
    return logs, moved


D_LOGS = ("loss_discriminator_real", "loss_discriminator_fake", "loss_discriminator_real_pixel_wise",
          "loss_discriminator_fake_pixel_wise")


def test_model_wrapper_with_the_hinge_family(golden):
    """Two iterations with the hinge family in the four loss slots (R1 in the regulariser's, which the family does not have),
    lazy R1 every second iteration, CutMix on with fixed maps: finite logs, both networks moved, and the first iteration's
    discriminator losses equal those of an identically seeded wrapper given plain-torch hinge modules (hinge terms are
    non-negative, so mean|term| is the loss itself)."""
    from multi_stylegan_amd import loss
    fused = dict(generator_loss=loss.HingeGeneratorLoss(), discriminator_loss=loss.HingeDiscriminatorLoss(),
                 discriminator_regularization_loss=loss.R1Regularization(),
                 cut_mix_augmentation_loss=loss.HingeDiscriminatorLossCutMix())
    plain = dict(generator_loss=_PlainHinge("gen"), discriminator_loss=_PlainHinge("disc"),
                 discriminator_regularization_loss=loss.R1Regularization(), cut_mix_augmentation_loss=_PlainHinge("cutmix"))
    logs, moved = _wrapper_run(golden, fused)
    for log in logs:
        assert set(D_LOGS) | {"loss_generator", "loss_generator_pixel_wise", "loss_cut_mix_augmentation"} <= set(log)
        assert all(math.isfinite(v) for vals in log.values() for v in vals), log
    assert "loss_discriminator_regularization" in logs[1] and "loss_discriminator_regularization" not in logs[0]
    assert moved[0] > 10 and moved[1] > 10, moved                             # parameter tensors of G and of D that moved
    ref_logs, _ = _wrapper_run(golden, plain, iterations=1)
    worst = 0.0
    for name in D_LOGS:
        got, want = logs[0][name][0], ref_logs[0][name][0]
        worst = max(worst, abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-5 * abs(want), (name, got, want)
    print("gan_loss ModelWrapper hinge, worst relative difference of the first discriminator losses", worst)


def test_model_wrapper_with_the_wasserstein_family(golden):
    from multi_stylegan_amd import loss
    logs, moved = _wrapper_run(golden, dict(
        generator_loss=loss.WassersteinGeneratorLoss(), discriminator_loss=loss.WassersteinDiscriminatorLoss(),
        discriminator_regularization_loss=loss.R1Regularization(),
        cut_mix_augmentation_loss=loss.WassersteinDiscriminatorLossCutMix()))
    assert all(math.isfinite(v) for log in logs for vals in log.values() for v in vals), logs
    assert moved[0] > 10 and moved[1] > 10, moved
