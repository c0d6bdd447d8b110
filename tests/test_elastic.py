"""Elastic deformation on the host: the tests' float64 restatement and the product's CPU function against what the reference's
own function returned (tests/golden/elastic.npz), the dataset hook, and the argument errors.  No GPU."""
import pytest
import torch

from elastic_util import CASES, case, deform64, field64, taps64
from tlfm_util import listing, write_case_tree

# |restatement - reference| measured when the fixture was made: <= 1.1e-5 on outputs in [0, 1]; ~10x for another torch build's
# convolution order.  A missed half-pixel shift, swapped divisors or swapped noise planes move these frames by ~0.28 on average.
TOL = 1e-4


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    c = case(name)
    got = deform64(c["frames"], c["noise"], c["sigma"], c["alpha"])
    err = (got - c["out"].double()).abs().max().item()
    print(f"{name}: |float64 restatement - reference| = {err:.3e}")
    assert err <= TOL
    # the fixture can tell a wrong formulation apart: swapped planes are far outside the tolerance
    swapped = deform64(c["frames"], c["noise"].flip(0), c["sigma"], c["alpha"])
    assert (swapped - c["out"].double()).abs().mean().item() > 50 * TOL


def test_restatement_field_is_the_truncated_unnormalised_gaussian():
    g = taps64(3)
    assert g.numel() == 13 and 0.95 < g.sum().item() < 0.975                   # +-2 sigma of a sampled unit Gaussian, not renormalised
    assert abs(taps64(16).sum().item() - 0.9545) < 5e-3
    ones = torch.ones(2, 40, 56)
    d = field64(ones, 3, 30.0)
    assert abs(d[0, 20, 28].item() - 30.0 * g.sum().item() ** 2) < 1e-12      # interior: the whole kernel
    assert abs(d[1, 0, 0].item() - 30.0 * g[6:].sum().item() ** 2) < 1e-12    # corner: zero padding cuts both sums


@pytest.mark.parametrize("name", CASES)
def test_host_function_reproduces_the_reference_and_its_draws(name):
    from multi_stylegan_amd import ElasticDeformation, elastic_deformation
    from multi_stylegan_amd import tlfm_dataset
    assert tlfm_dataset.elastic_deformation is elastic_deformation and tlfm_dataset.ElasticDeformation is ElasticDeformation
    c = case(name)
    torch.manual_seed(c["seed"])
    got = elastic_deformation(c["frames"], alpha=c["alpha"], sigma=c["sigma"])
    after = torch.rand(1)
    assert got.shape == c["frames"].shape and got.dtype == torch.float32
    err = (got - c["out"]).abs().max().item()
    print(f"{name}: |elastic_deformation - reference| = {err:.3e}")
    assert err <= TOL
    assert torch.equal(after, c["next"])                                       # the global generator is where the reference leaves it
    # a leading 1 is accepted and dropped, as in the reference; the module with a generator of its own leaves the global one alone
    torch.manual_seed(c["seed"])
    assert torch.equal(elastic_deformation(c["frames"][None], alpha=c["alpha"], sigma=c["sigma"]), got)
    module = ElasticDeformation(alpha=c["alpha"], sigma=c["sigma"], generator=torch.Generator().manual_seed(c["seed"]))
    torch.manual_seed(5)
    want_next = torch.rand(1)
    torch.manual_seed(5)
    assert torch.equal(module(c["frames"]), got) and torch.equal(torch.rand(1), want_next)


def test_module_defaults_and_other_sample_modes_on_the_host():
    from multi_stylegan_amd import ElasticDeformation
    module = ElasticDeformation()
    assert (module.sample_mode, module.alpha, module.sigma, module.generator) == ("bilinear", 80, 16, None)
    x = case("tiny")["frames"]
    for mode in ("nearest", "bicubic"):
        torch.manual_seed(3)
        assert ElasticDeformation(sample_mode=mode, alpha=10, sigma=4)(x).shape == x.shape


def test_dataset_hook(tmp_path):
    """ElasticDeformation as the dataset's `transformations` (raw=False): [C, T, H, W] samples, the counts deformed before
    they are normalised, as in the reference's Compose."""
    from multi_stylegan_amd import ElasticDeformation, TFLMDatasetGAN, prepare_tlfm_batch
    rec = listing()["cases"]["c3_plain"]
    write_case_tree(str(tmp_path / "dataset"), rec)
    kw = dict(flip=rec["flip"], no_rfp=rec["no_rfp"], no_gfp=rec["no_gfp"])
    ds = TFLMDatasetGAN(str(tmp_path / "dataset"), transformations=ElasticDeformation(alpha=20, sigma=2), **kw)
    plain = TFLMDatasetGAN(str(tmp_path / "dataset"), transformations=lambda x: x, **kw)
    torch.manual_seed(11)
    sample = ds[0]
    assert sample.shape == plain[0].shape and sample.ndim == 4 and sample.dtype == torch.float32
    assert not torch.equal(sample, plain[0])
    # the same draws by hand: deform the stacked float counts, then normalise
    from multi_stylegan_amd import elastic_deformation
    counts = ds._counts(0)
    torch.manual_seed(11)
    moved = elastic_deformation(torch.from_numpy(counts.numpy().astype("float32")).flatten(0, 1), alpha=20, sigma=2).reshape(counts.shape)
    assert torch.equal(sample, prepare_tlfm_batch(moved[None], None, vertical_flip=rec["flip"])[0])
    with pytest.raises(ValueError, match="raw=True"):
        TFLMDatasetGAN(str(tmp_path / "dataset"), transformations=ElasticDeformation(), raw=True, **kw)


def test_errors():
    from multi_stylegan_amd import ElasticDeformation, elastic_deform_batch, elastic_deformation
    from multi_stylegan_amd._lib import MsgHipError
    from multi_stylegan_amd.data import TLFMDeviceFeed
    with pytest.raises(ValueError, match="F, H, W"):
        elastic_deformation(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="F, H, W"):
        elastic_deformation(torch.zeros(2, 3, 8, 8))                           # 4-D needs a leading 1
    with pytest.raises(ValueError, match="sigma"):
        elastic_deformation(torch.zeros(1, 8, 8), sigma=0)
    # a tensor that is not on the CPU takes the device path, which is bilinear only: refused before anything touches a device
    with pytest.raises(ValueError, match="bicubic"):
        elastic_deformation(torch.empty(2, 8, 8, device="meta"), sample_mode="bicubic")
    with pytest.raises(ValueError, match="nearest"):
        ElasticDeformation(sample_mode="nearest")(torch.empty(2, 8, 8, device="meta"))
    with pytest.raises(ValueError, match="nearest"):
        TLFMDeviceFeed([], "cuda", elastic=ElasticDeformation(sample_mode="nearest"))
    with pytest.raises(ValueError, match="B, C, T, H, W"):
        elastic_deform_batch(torch.zeros(3, 8, 8), alpha=10, sigma=2)
    with pytest.raises(ValueError, match="autograd"):
        elastic_deform_batch(torch.zeros(1, 2, 8, 8, requires_grad=True), alpha=10, sigma=2)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        elastic_deform_batch(torch.zeros(1, 2, 8, 8, dtype=torch.float64), alpha=10, sigma=2)
    with pytest.raises(ValueError, match="noise"):
        elastic_deform_batch(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 4), alpha=10, sigma=2)
    with pytest.raises(ValueError, match="sigma"):
        elastic_deform_batch(torch.zeros(1, 2, 8, 8), alpha=10, sigma=33)
    with pytest.raises(MsgHipError, match="no CPU fallback"):                  # a batch is device work: nothing quiet on the host
        elastic_deform_batch(torch.zeros(1, 2, 8, 8), alpha=10, sigma=2)
