"""CPU-side checks of the product's host logic: C-ABI library exports, module/state_dict surface, losses, the
gradient-bucket reducer and the trainer's data-parallel path under gloo (world size 2)."""
import ctypes
import json
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT, rel_err


def test_library_exports_every_declared_symbol():
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    names = _lib.declared_symbols()
    assert {"msg_upfirdn2d", "msg_fused_bias_act", "msg_bias_act_backward", "msg_abi_version"} <= set(names)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(handle, name), f"{name} declared in include/msg_hip.h but not exported"
    assert _lib.lib().msg_build_arch() == b"gfx950" and _lib.lib().msg_abi_version() >= 1
    # the binding is parsed from the header by a strict reader: it saw every name this loose regex sees, nothing else
    assert set(_lib._SIGNATURES) == set(names) and len(names) >= 69


def _stripped_header():
    from multi_stylegan_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_binding_types_are_the_headers():
    """Pins on the header-derived signatures and constants that do not go through the parser's own output: written here from
    reading include/msg_hip.h.  A shifted or narrowed argument reaches the kernels as a wrong stride or pointer."""
    from multi_stylegan_amd import _lib, conv_ops
    from multi_stylegan_amd.build import build
    build(verbose=False)
    c, sig = ctypes, _lib._SIGNATURES
    P, I, L, F = c.c_void_p, c.c_int, c.c_longlong, c.c_float
    assert sig["msg_strerror"] == (c.c_char_p, [I]) and sig["msg_build_arch"] == (c.c_char_p, [])
    assert sig["msg_abi_version"] == (I, [])
    sizes = [n for n in sig if n.endswith("_workspace")]
    assert len(sizes) >= 6 and all(sig[n][0] is L for n in sizes)
    assert all(res is I for n, (res, _a) in sig.items() if n not in sizes and n not in ("msg_strerror", "msg_build_arch"))
    res, args = sig["msg_conv2d_fprop"]
    assert res is I and len(args) == 22 and args[:5] == [P, P, P, P, I] and args[5:20] == [I] * 15
    assert args[20] is L and args[21] is P                                   # w_batch_stride, stream
    assert sig["msg_conv2d_fprop_plan"] == (I, [I] * 11 + [L])
    assert sig["msg_conv2d_fprop_launch_plan"] == (I, [I] * 16 + [L, I, I, P, I])       # msg_conv2d_fprop's dtype .. w_batch_stride first
    assert sig["msg_conv2d_fprop_launch_plan"][1][:17] == sig["msg_conv2d_fprop"][1][4:21]
    assert sig["msg_conv2d_wgrad_plan"] == (I, [I] * 18 + [P, I]) and sig["msg_conv2d_wgrad_workspace"] == (L, [I] * 18)
    assert sig["msg_flat_adam"] == (I, [P, P, P, P, P, L, P, F, F, F, F, I, F, P])
    assert sig["msg_flat_ema"] == (I, [P, P, L, F, P])
    assert sig["msg_bias_act_backward_workspace"] == (L, [L, I, I, I])
    assert sig["msg_gamma_merge_backward_workspace"] == (L, [])
    assert (_lib.MSG_OK, _lib.MSG_EINVAL, _lib.MSG_EUNSUPPORTED, _lib.MSG_ELAUNCH) == (0, -1, -2, -3)
    assert (_lib.MSG_F32, _lib.MSG_BF16, _lib.MSG_F16, _lib.MSG_F64, _lib.MSG_F32_SPLIT) == (0, 1, 2, 3, 4)
    assert conv_ops.MSG_F32_SPLIT == 4
    assert (_lib.MSG_PLAN_REG, _lib.MSG_PLAN_DMA, _lib.MSG_PLAN_PP, _lib.MSG_PLAN_ROW3, _lib.MSG_PLAN_ROW3N,
            _lib.MSG_PLAN_THIN, _lib.MSG_PLAN_UPCONV, _lib.MSG_FPLAN_FIELDS) == (0, 1, 2, 3, 4, 5, 6, 5)
    # the kernel-clock labels bench.py, profiles/ and the tools key on, and the tile of the sign bytes, per plan
    assert conv_ops._PLANS == {0: ("conv_fprop_reg", None), 1: ("conv_fprop_dma", None), 2: ("conv_fprop_pp", None),
                               3: ("conv_fprop_row3", 256), 4: ("conv_fprop_row3n", 128), 5: ("conv_fprop_thin", None),
                               6: ("conv_fprop_upconv", None)}
    assert _lib.ABI_VERSION == _lib.lib().msg_abi_version() == 5
    assert _lib.lib().msg_strerror(_lib.MSG_EUNSUPPORTED) != _lib.lib().msg_strerror(_lib.MSG_EINVAL)
    # every `msg_name(` of the comment-stripped header became exactly one parsed prototype
    assert len(re.findall(r"\bmsg_[a-z0-9_]+\s*\(", _stripped_header())) == len(sig)


_REFUSED = {
    "msg_new_double": "int msg_new_double(const float* x, double gain, void* stream);",
    "msg_new_struct": "typedef struct { int b, h, w; } msg_shape;\nint msg_new_struct(const void* x, msg_shape shape, void* stream);",
    "msg_new_callback": "int msg_new_callback(const void* x, void (*done)(int), void* stream);",   # (read up to `(*done)`: truncated)
    "msg_new_unnamed": "int msg_new_unnamed(const void*, int, void*);",
    "msg_new_result": "double msg_new_result(const void* x);",
    "msg_strerror": "const char* msg_strerror(int code);",                                         # (declared twice)
}


@pytest.mark.parametrize("name", sorted(_REFUSED))
def test_binding_refuses_what_it_cannot_pass(name):
    """A prototype with a type outside the closed map (pointers, int, long long, float), one the reader would truncate, or a
    second declaration: the import-time parse raises and names the entry -- nothing is skipped or guessed."""
    from multi_stylegan_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    mark = "#ifdef __cplusplus\n}"
    assert text.count(mark) == 1
    assert len(_lib._parse_header(text)[0]) == len(_lib._SIGNATURES)
    with pytest.raises(_lib.MsgHipError, match=name):
        _lib._parse_header(text.replace(mark, _REFUSED[name] + "\n" + mark))
    ok = text.replace(mark, "long long msg_new_fine(const unsigned char* const* x, long long n,\n float g, void* stream);\n" + mark)
    assert _lib._parse_header(ok)[0]["msg_new_fine"] == (ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float,
                                                                            ctypes.c_void_p])


def test_product_modules_keep_reference_surface():
    import multi_stylegan_amd as m
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    g = m.MultiStyleGANGenerator(m.multi_style_gan_generator_config)
    d = m.MultiStyleGANDiscriminator(m.u_net_2d_discriminator_config, no_rfp=True)
    assert {k: list(v.shape) for k, v in g.state_dict().items()} == man["generator"]
    assert {k: list(v.shape) for k, v in d.state_dict().items()} == man["discriminator"]
    assert [len(list(grp["params"])) for grp in g.get_parameters()] == man["generator_param_groups"]
    assert sum(p.numel() for p in g.live_parameters()) == 32565276
    with pytest.raises(Exception, match="no CPU fallback"):
        g(torch.randn(2, 512))                                           # product path refuses CPU tensors


def test_losses_match_oracle(golden):
    from multi_stylegan_amd import loss
    from oracle import train as ot
    torch.manual_seed(0)
    pr, pf = torch.randn(4, 1), torch.randn(4, 1, 1, 8, 8)
    assert rel_err(loss.NonSaturatingLogisticGeneratorLoss()(pf), ot.g_logistic_loss(pf)) < 1e-6
    a, b = loss.NonSaturatingLogisticDiscriminatorLoss()(pr, pr * 2)
    c, d_ = ot.d_logistic_loss(pr, pr * 2)
    assert rel_err(a, c) < 1e-6 and rel_err(b, d_) < 1e-6
    # path length: value, running mean and -- the subtle part -- the gradient through the running mean
    pl_a, pl_b = loss.PathLengthRegularization(), ot.PathLength()
    for _ in range(3):
        g1 = torch.randn(2, 5, 16, requires_grad=True)
        g2 = g1.detach().clone().requires_grad_(True)
        la, _ = pl_a(g1)
        lb, _ = pl_b(g2)
        la.backward(); lb.backward()
        assert rel_err(la, lb) < 1e-6 and rel_err(g1.grad, g2.grad) < 1e-6
    assert rel_err(pl_a.mean_path_length, pl_b.mean_path_length) < 1e-6


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.a = torch.nn.Linear(6, 5)
        self.b = torch.nn.Linear(5, 3)
        self.unused = torch.nn.Parameter(torch.ones(4))

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def _reducer_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from multi_stylegan_amd.dist import GradBucketReducer
    model = _Toy()
    params = [p for n, p in model.named_parameters() if n != "unused"]
    red = GradBucketReducer(params, bucket_bytes=64, overlap=True)       # tiny buckets -> several of them
    assert len(red.buckets) > 1
    torch.manual_seed(100 + rank)
    x = torch.randn(7, 6)
    for attempt in range(2):                                             # second pass exercises zero_grad reuse
        local = [t.clone() for t in torch.autograd.grad(model(x).square().sum(), params)]   # before any collective
        red.zero_grad(); red.arm()
        model(x).square().sum().backward()                 # buckets are all-reduced from the hooks, overlapped
        red.finish()
        gathered = [None] * world
        dist.all_gather_object(gathered, local)
        for i, p in enumerate(params):
            want = sum(g[i] for g in gathered) / world
            assert torch.allclose(p.grad, want, atol=1e-6), (rank, attempt, i)
        total = red.clip_(0.5)
        norm_after = torch.sqrt(sum(p.grad.square().sum() for p in params))
        assert norm_after <= 0.5 + 1e-4 and total > 0
    # gradients arriving in a different order on each rank must not reorder the collectives
    local = [t.clone() for t in torch.autograd.grad(model(x).square().sum(), params)]
    red.zero_grad(); red.arm()
    # (rank r starts its arrival order at a different parameter and odd ranks walk it backwards: four distinct orders at world 4)
    order = [(i + rank) % len(params) for i in range(len(params))]
    if rank % 2:
        order.reverse()
    for i in order:
        params[i].grad.copy_(local[i])
        red._on_grad(params[i])
    red.finish()
    gathered = [None] * world
    dist.all_gather_object(gathered, local)
    for i, p in enumerate(params):
        assert torch.allclose(p.grad, sum(g[i] for g in gathered) / world, atol=1e-6), (rank, "order", i)
    assert model.unused.grad is None
    # ---- labelled backwards: a bucket that a kind of backward never fills must not stall the buckets behind it
    red2 = GradBucketReducer(params + [model.unused], bucket_bytes=16, overlap=True)      # one parameter per bucket,
    cold = next(k for k, b in enumerate(red2.buckets) if b.params[0] is model.unused)     # the never-filled one FIRST
    assert cold == 0 and all(len(b.params) == 1 for b in red2.buckets) and len(red2.buckets) == len(params) + 1
    for attempt in range(3):
        local = [t.clone() for t in torch.autograd.grad(model(x).square().sum(), params)]
        red2.zero_grad(); red2.arm("fwd")
        model(x).square().sum().backward()
        launched = [b.work is not None for b in red2.buckets]          # before finish(): what the hooks managed to send
        if attempt == 0:
            # first time nothing is known: launches are strictly in order and every bucket waits behind the cold one
            assert not any(launched), launched
        else:
            assert not launched[cold] and all(launched[1:]), (attempt, launched)
        red2.finish()
        gathered = [None] * world
        dist.all_gather_object(gathered, local)
        for i, p in enumerate(params):
            assert torch.allclose(p.grad, sum(g[i] for g in gathered) / world, atol=1e-6), (rank, "labelled", attempt, i)
        assert float(model.unused.grad.abs().max()) == 0.0             # exchanged (last), still zero
    # a cold bucket that does receive a gradient after all is simply exchanged last, with that gradient
    red2.zero_grad(); red2.arm("fwd")
    (model(x).square().sum() + (1.0 + rank) * model.unused.sum()).backward()
    red2.finish()
    assert torch.allclose(model.unused.grad, torch.full((4,), 1.0 + (world - 1) / 2.0))       # mean of 1 + rank
    # ... but a gradient that arrives for a bucket ALREADY on the wire is refused loudly, never silently dropped
    red4 = GradBucketReducer(params + [model.unused], bucket_bytes=64, overlap=True)
    mixed = next(b for b in red4.buckets if any(q is model.unused for q in b.params))
    assert len(mixed.params) > 1
    for _ in range(2):
        red4.zero_grad(); red4.arm("fwd")
        model(x).square().sum().backward()
        red4.finish()
    red4.zero_grad(); red4.arm("fwd")
    try:
        (model(x).square().sum() + model.unused.sum()).backward()
        raised = False
    except RuntimeError as exc:
        raised = "use distinct labels" in str(exc)
    red4.finish()
    assert raised
    for p in params:                                                    # hand the gradients back to the first reducer
        p.grad = None
    model.unused.grad = None
    # ---- reduce_scatter exchange: same means, same clip norm as the all-reduce exchange
    red3 = GradBucketReducer(params, bucket_bytes=64, overlap=True, exchange="reduce_scatter")
    local = [t.clone() for t in torch.autograd.grad(model(x).square().sum(), params)]
    red3.zero_grad(); red3.arm("fwd")
    model(x).square().sum().backward()
    red3.finish()
    gathered = [None] * world
    dist.all_gather_object(gathered, local)
    means = [sum(g[i] for g in gathered) / world for i in range(len(params))]
    for i, p in enumerate(params):
        assert torch.allclose(p.grad, means[i], atol=1e-6), (rank, "reduce_scatter", i)
    want_norm = torch.sqrt(sum(m.square().sum() for m in means))
    assert torch.allclose(red3.grad_norm(), want_norm, rtol=1e-5), (red3.grad_norm(), want_norm)
    red3.clip_(0.5)
    assert torch.sqrt(sum(p.grad.square().sum() for p in params)) <= 0.5 + 1e-4
    # ... and the SUM form the fused optimiser path uses: finish(average=False) leaves sums, the norm is the sum's
    red3.zero_grad(); red3.arm("fwd")
    model(x).square().sum().backward()
    inv = red3.finish(average=False)
    assert inv == 1.0 / world and torch.allclose(red3.grad_norm() * inv, want_norm, rtol=1e-5)
    for i, p in enumerate(params):
        assert torch.allclose(p.grad * inv, means[i], atol=1e-6)
    if rank == 0:
        out.put("ok")
    dist.destroy_process_group()


def _run_ranks(worker, world, port, timeout):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    [p.join(timeout) for p in procs]
    hung = [p for p in procs if p.exitcode is None]
    [p.kill() for p in hung]
    assert not hung, "ranks deadlocked"
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert q.get(timeout=5) == "ok"


@pytest.mark.parametrize("world", [2, 4])
def test_bucket_reducer_gloo(world):
    """world 4: four distinct gradient-arrival orders (collectives must still be issued in ONE order), means over four
    shards, both exchanges."""
    _run_ranks(_reducer_worker, world, 29000 + os.getpid() % 400 + 17 * world, 180)


def _trainer_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from multi_stylegan_amd.model_wrapper import ModelWrapper
    from oracle import models as om                      # CPU stand-ins for G/D: the trainer logic is device-agnostic
    from tools.gen_golden import TINY_D, TINY_G
    torch.set_num_threads(max(1, 8 // world))
    torch.manual_seed(10 + rank)                         # different init per rank: broadcast must fix it
    g, d = om.Generator(TINY_G), om.Discriminator(TINY_D, no_rfp=True)
    g.live_parameters = lambda: [p for n, p in g.named_parameters() if not n.startswith("main_convolutions_2.")]
    orig_forward = g.forward
    g.forward = lambda *a, path_length_noise=None, **k: orig_forward(*a, **k)
    # plain SGD: the parameter movement is proportional to the exchanged gradient, so a wrong reduction shows
    tr = ModelWrapper(g, d, device="cpu", bucket_bytes=1 << 16,
                      generator_optimizer=torch.optim.SGD(g.parameters(), lr=1e-3),
                      discriminator_optimizer=torch.optim.SGD(d.parameters(), lr=1e-3))
    from ddp_probe import StepProbe
    probe = StepProbe(tr)
    tr.iteration = 15                                    # next iteration is 16: R1 and path length fire
    torch.manual_seed(1000 + rank)                       # different data per rank
    # rank-distinct style-mixing graphs (what a real job has: every rank draws its own mixing coin and crossover layer):
    # different crossover layers per rank, and the last rank of a world > 2 does not mix at all -- its generator graph has
    # ONE mapping-network pass where the others have two, so gradients become ready in different orders on different ranks
    import random
    import numpy as np
    random.seed(4321 + rank)
    np.random.seed(99 + 7 * rank)
    if world > 2 and rank == world - 1:
        tr.hyperparameters = dict(tr.hyperparameters, p_mixed_noise=0.0)
    tr.train_iteration(torch.rand(2, 2, 3, 32, 32))
    logs = tr.pop_logs()
    # every step == the single-process step with the mean of the two shards' gradients
    assert probe.check(world, lr=1e-3) == ["d", "g", "pl", "r1"]
    assert {"loss_discriminator_regularization", "path_length", "loss_generator"} <= set(logs)
    flat = torch.cat([p.detach().flatten() for p in list(g.parameters()) + list(d.parameters())])
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    assert all(torch.equal(both[0], other) for other in both[1:]), "replicas diverged"
    mpl = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(mpl, tr.path_length_regularization.mean_path_length)
    assert all(torch.equal(mpl[0], other) for other in mpl[1:])
    if rank == 0:
        out.put("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_trainer_data_parallel_gloo(world):
    """One regularised iteration (D, R1, G, path-length steps) on `world` gloo ranks with rank-distinct data, latents and
    style-mixing graphs: every optimiser step is the step of the MEAN of the shards' gradients (tests/ddp_probe.py), the
    replicas and the path-length mean stay bit-identical."""
    _run_ranks(_trainer_worker, world, 29500 + os.getpid() % 300 + 23 * world, 420)


def _cut_mix_gate_worker(rank, world, port, out):
    """Late-training iterations with the RANDOM CutMix gate (no Draws.cut_mix) and rank-distinct Python RNGs, as bench.py
    and the per-rank style-mixing draws leave them: every rank must take the same branch in every iteration."""
    import random
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from multi_stylegan_amd.model_wrapper import ModelWrapper
    from oracle import models as om
    from tools.gen_golden import TINY_D, TINY_G
    torch.manual_seed(10)
    g, d = om.Generator(TINY_G), om.Discriminator(TINY_D, no_rfp=True)
    g.live_parameters = lambda: [p for n, p in g.named_parameters() if not n.startswith("main_convolutions_2.")]
    orig_forward = g.forward
    g.forward = lambda *a, path_length_noise=None, **k: orig_forward(*a, **k)
    random.seed(1234 + rank)
    tr = ModelWrapper(g, d, device="cpu", bucket_bytes=1 << 16,
                      generator_optimizer=torch.optim.SGD(g.parameters(), lr=1e-3),
                      discriminator_optimizer=torch.optim.SGD(d.parameters(), lr=1e-3))
    assert tr._control_rng is not None
    tr.epoch, tr.epochs = 5, 10                          # gate probability 0.25, plus the resume_training coin
    torch.manual_seed(1000 + rank)
    gates = []
    for _ in range(4):
        tr.train_iteration(torch.rand(2, 2, 3, 32, 32), resume_training=True)
        gates.append("loss_cut_mix_augmentation" in tr.pop_logs())
    everyone = [None] * world
    dist.all_gather_object(everyone, gates)
    assert everyone[0] == everyone[1], everyone
    assert any(gates), gates                             # the CutMix branch (two extra discriminator exchanges) was taken
    mine = [None] * world                                # ... while the ranks' own Python RNGs really are distinct
    dist.all_gather_object(mine, random.random())
    assert mine[0] != mine[1]
    flat = torch.cat([p.detach().flatten() for p in list(g.parameters()) + list(d.parameters())])
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    assert torch.equal(both[0], both[1]), "replicas diverged"
    # a checkpoint carries the gate's generator state: a resumed job draws the same continuation on every rank
    state = tr.checkpoint_dict()["multi_stylegan_amd"]["control_rng"]
    nxt = tr._control_random()
    tr._control_rng.setstate(state)
    assert tr._control_random() == nxt
    if rank == 0:
        out.put("ok")
    dist.destroy_process_group()


def test_cut_mix_gate_is_rank_consistent_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 28200 + os.getpid() % 400
    procs = [ctx.Process(target=_cut_mix_gate_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    hung = [p for p in procs if p.exitcode is None]
    [p.kill() for p in hung]
    assert not hung, "ranks disagreed on the CutMix gate and deadlocked"
    assert all(p.exitcode == 0 for p in procs)
    assert q.get(timeout=5) == "ok"


def test_kernel_plans_respect_the_31_bit_offset_limits():
    """Host-side dispatch only (no launch): the kernels that address their operands through buffer descriptors -- 31-bit
    offsets -- must not be planned for tensors of 2 GiB or more (the launch then belongs to the 64-bit-pointer instantiation),
    and the weight-gradient planner must accept the maps one column short of a power of two that it now runs on padded rows.
    The GPU side of the same limits: tests/test_hip_conv.py::test_conv_above_two_gib_of_activations."""
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    lib = _lib.lib()
    bf16 = _lib.MSG_BF16
    plan = lambda b, c, n, hw, k, ws: lib.msg_conv2d_fprop_plan(bf16, b, hw, hw, c, c, hw, hw, n, k, k, ws)
    # 3x3 512 -> 512 @256^2: per-sample weights (one sample per descriptor) and a shared-weight batch of 0.5 GiB: the 256 x 256 tile
    assert plan(16, 512, 512, 256, 3, 512 * 512 * 9) == _lib.MSG_PLAN_ROW3 == 3
    assert plan(8, 512, 512, 256, 3, 0) == _lib.MSG_PLAN_ROW3
    # the same layer over 33 samples with SHARED weights: 2.2 GiB behind one descriptor -> register-staged 128 x 128 kernel
    assert plan(33, 512, 512, 256, 3, 0) == _lib.MSG_PLAN_REG == 0
    # 1x1 512 -> 256 (ping-pong kernel's territory: MSG_PLAN_PP) likewise
    assert plan(16, 512, 256, 256, 1, 0) == _lib.MSG_PLAN_PP == 2
    assert plan(33, 512, 256, 256, 1, 0) == _lib.MSG_PLAN_REG
    # weight-gradient workspace queries (plan only) on the discriminator's stride-2 outputs: 127, 63, 31, 15 wide
    for c, ihw, ohw in ((128, 256, 127), (256, 128, 63), (384, 64, 31), (768, 32, 15)):
        need = lib.msg_conv2d_wgrad_workspace(bf16, 32, ihw, ihw, c, c, ohw, ohw, c, c, c, 3, 3, 2, 0, 0, 0, 1)
        assert need > 0 and need % (c * 9 * c) == 0, (c, ohw, need)          # whole slabs of O x taps x ldgw floats


def test_dispatch_answers_match_the_recorded_table():
    """The host-side answers of the convolution family -- msg_conv2d_fprop_plan, msg_conv2d_fprop_act_backward_workspace,
    msg_conv2d_fprop_upconv_eligible, msg_conv2d_fprop_thin_eligible, msg_conv2d_wgrad_workspace, msg_conv2d_wgrad_plan,
    msg_conv2d_fprop_launch_plan -- over the grid of
    tools/gen_dispatch_table.py (the models' geometries at 256^2 and 512^2, shared and per-sample weights, batch 1 .. 33, and both
    sides of every eligibility threshold), against tests/golden/dispatch_table.json: the answers recorded BEFORE the forward dispatch
    became one selection function.  Equality on every row, except four classes where the recorded answer named a kernel the
    launch never ran and the answer is now what launches (the launch itself is as it was):
      * thin N (<= 8 output channels) with Ck / 32 outside the instantiated {2, 4, 6, 8, 12, 16}: THIN (eligible 1) -> REG (0);
      * MSG_F32_SPLIT with a long K sweep: DMA -> REG (the split-bf16 kernel stages through registers whatever the K length);
      * the up-convolution with per-sample weight sets closer than one set (stride < N * 512): eligible 1 -> 0;
      * thin with per-sample weights and more than 65535 samples (grid.y): THIN -> DMA / PP / REG, whichever tile kernel takes it.
    None of them is a geometry of the models: their thin layers have 128 / 512 channels, the Python layer asks the plan with the
    storage code (never MSG_F32_SPLIT), per-sample weight images are dense and batches are tens of samples.
    msg_conv2d_fprop_launch_plan -- the launch's own arguments, bias and epilogue -- has no exceptions: its table was recorded from
    the commit before it existed, through a query that reported that commit's conv_fprop_select, act_backward_partials and argument
    checks, and every row must equal it.  And the grid does hold
    the models' geometries: every conv_fprop* / conv_wgrad label of the per-shape kernel tables of the benchmark has a row."""
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    from tools import gen_dispatch_table as grid
    build(verbose=False)
    lib = _lib.lib()
    with open(os.path.join(GOLDEN, "dispatch_table.json")) as f:
        table = json.load(f)
    rows = {name: fn() for name, fn in grid.ALL_ROWS.items()}
    for name, r in rows.items():                       # the recorded answers belong to exactly these rows
        assert grid.digest(r) == table["digest"][name] and len(r) == len(table[name]), name
    assert not grid.missing_profile_geometries([os.path.join(ROOT, "profiles", "r05_shape_table.txt"),
                                                os.path.join(ROOT, "profiles", "r05_shape_table_regularised.txt")])
    bf16 = _lib.MSG_BF16
    thin_kc = (2, 4, 6, 8, 12, 16)
    model_channels = (8, 64, 128, 256, 384, 512, 768, 1024)
    truthful = {"plan": 0, "thin_eligible": 0, "upconv_eligible": 0}
    bad, plan_codes = [], []
    for args, ans in zip(rows["plan"], table["plan"]):
        plan, ws0, ws1 = ans if isinstance(ans, list) else (ans, 0, 0)
        dtype, ck, n = args[0], args[5], args[8]
        if plan == _lib.MSG_PLAN_THIN and n <= 8 and ck // 32 not in thin_kc:
            assert ck not in model_channels
            plan, truthful["plan"] = _lib.MSG_PLAN_REG, truthful["plan"] + 1
        elif dtype == _lib.MSG_F32_SPLIT and plan == _lib.MSG_PLAN_DMA:
            plan, truthful["plan"] = _lib.MSG_PLAN_REG, truthful["plan"] + 1
        elif plan == _lib.MSG_PLAN_THIN and args[11] and args[1] > 65535:     # (4x4 maps, 512 or 64 channels: 8 K-steps or 1)
            plan, truthful["plan"] = (_lib.MSG_PLAN_DMA if ck == 512 else _lib.MSG_PLAN_REG), truthful["plan"] + 1
        got = (lib.msg_conv2d_fprop_plan(*args), lib.msg_conv2d_fprop_act_backward_workspace(*args, 0),
               lib.msg_conv2d_fprop_act_backward_workspace(*args, 1))
        if got != (plan, ws0, ws1):
            bad.append(("plan", args, (plan, ws0, ws1), got))
        plan_codes.append((plan, ws0, ws1))
    for args, mode in zip(rows["thin_eligible"], table["thin_eligible"]):
        if mode == 1 and args[4] // 32 not in thin_kc:
            assert args[4] not in model_channels
            mode, truthful["thin_eligible"] = 0, truthful["thin_eligible"] + 1
        if lib.msg_conv2d_fprop_thin_eligible(*args) != mode:
            bad.append(("thin_eligible", args, mode, lib.msg_conv2d_fprop_thin_eligible(*args)))
    for args, ok in zip(rows["upconv_eligible"], table["upconv_eligible"]):
        if ok == 1 and args[14] < args[7] * 512:
            ok, truthful["upconv_eligible"] = 0, truthful["upconv_eligible"] + 1
        if lib.msg_conv2d_fprop_upconv_eligible(*args) != ok:
            bad.append(("upconv_eligible", args, ok, lib.msg_conv2d_fprop_upconv_eligible(*args)))
    for args, need in zip(rows["wgrad_workspace"], table["wgrad_workspace"]):
        if lib.msg_conv2d_wgrad_workspace(*args) != need:
            bad.append(("wgrad_workspace", args, need, lib.msg_conv2d_wgrad_workspace(*args)))
    # weight-gradient plans, recorded from the commit before msg_conv2d_wgrad planned through conv_wgrad_select (its wgrad_impl /
    # conv_wgrad_row3_try, with a query that reported their locals): every field of every row, no exceptions
    for args, ans in zip(rows["wgrad_plan"], table["wgrad_plan"]):
        if grid.wgrad_plan(lib, args) != ans:
            bad.append(("wgrad_plan", args, ans, grid.wgrad_plan(lib, args)))
    for args, ans in zip(rows["fprop_plan"], table["fprop_plan"]):
        if grid.fprop_plan(lib, args) != ans:
            bad.append(("fprop_plan", args, ans, grid.fprop_plan(lib, args)))
    assert not bad, (len(bad), bad[:10])
    # the first rows of the new table are the old plan's rows with its assumptions spelled out, at epilogue 0 without a bias: the
    # recorded plans are the old table's codes (after the truthful classes above), unless the launch refuses the geometry -- which
    # the old query, without the launch's checks, could not say: Ck no multiple of 128 bytes, or a K sweep beyond the zero page
    for args, ans, (plan, _ws0, _ws1) in zip(rows["fprop_plan"], table["fprop_plan"], plan_codes):
        bke = 64 if args[0] == bf16 else 32
        if isinstance(ans, list):
            assert ans[0] == plan, (args, ans, plan)
        else:
            assert ans == _lib.MSG_EUNSUPPORTED and (args[5] % bke or (args[10] * args[11] * (args[5] // bke) + 1) * 128 + 128 > 65536), args
    assert [a[:9] + a[10:12] + a[16:17] for a in rows["fprop_plan"][:len(rows["plan"])]] == rows["plan"]
    assert all(a[9:10] + a[12:16] + a[17:] == [max(8, (a[8] + 7) // 8 * 8), 1, a[10] // 2, 1, 0, 0, 0] for a in rows["fprop_plan"][:len(rows["plan"])])
    # ... and, under the same assumptions at epilogue 3, the old workspace query is act_rows * N (+ act_entries with noise)
    fplans = dict(zip(map(tuple, rows["fprop_plan"]), table["fprop_plan"]))
    for key, ans in fplans.items():
        if key[18] == 3 and isinstance(ans, list) and (key[9], key[12:16]) == (max(8, (key[8] + 7) // 8 * 8), (1, key[10] // 2, 1, 0)):
            act_rows, act_entries = (ans + [0, 0])[3:5]
            old = [lib.msg_conv2d_fprop_act_backward_workspace(*key[:9], *key[10:12], key[16], noise) for noise in (0, 1)]
            assert old == ([act_rows * key[8], act_rows * key[8] + act_entries] if act_rows else [0, 0]), (key, ans, old)
    # what the new table holds that the old queries could not say: every kernel code, the epilogues, and refusals of both kinds
    seen = {(a[18], p[0] if isinstance(p, list) else p) for a, p in fplans.items()}
    assert {(0, _lib.MSG_PLAN_UPCONV), (1, _lib.MSG_PLAN_ROW3), (1, _lib.MSG_PLAN_ROW3N), (1, _lib.MSG_PLAN_PP), (1, _lib.MSG_PLAN_DMA),
            (1, _lib.MSG_PLAN_REG), (2, _lib.MSG_PLAN_THIN), (3, _lib.MSG_PLAN_ROW3), (3, _lib.MSG_PLAN_PP), (0, _lib.MSG_EINVAL),
            (0, _lib.MSG_EUNSUPPORTED)} <= seen and (1, _lib.MSG_PLAN_THIN) not in seen
    assert all(len(p) <= 3 for a, p in fplans.items() if isinstance(p, list) and (a[18] != 3 or p[0] not in (3, 4) or a[9] != a[8]))
    assert any(len(p) == 5 for p in fplans.values() if isinstance(p, list))
    assert any(a[14] == 2 for a in fplans) and any(a[15] and a[9] == a[8] // 4 for a in fplans) and any(a[12] == 2 and a[13] == 0 for a in fplans)
    assert any(a[9] > a[8] >= 128 for a in fplans) and any(a[0] == _lib.MSG_F32_SPLIT and a[9] % 8 == 4 for a in fplans)
    assert len(rows["plan"]) > 2500 and len(rows["wgrad_workspace"]) > 1400
    assert rows["wgrad_plan"][:len(rows["wgrad_workspace"])] == rows["wgrad_workspace"]
    # ... and the grid reaches every branch of the plan (MSG_WPLAN_DMA needs a tuning build's MSG_CONV_VARIANT=1: not covered)
    plans = [(a, p) for a, p in zip(rows["wgrad_plan"], table["wgrad_plan"]) if isinstance(p, list) and a[1] > 0]
    kernel, nz, chunks_per_out, n_out, slice_pixels, owv, ohv, fold, xcd_slices, blocks, need = range(_lib.MSG_WPLAN_FIELDS)
    assert {p[kernel] for _a, p in plans} == {_lib.MSG_WPLAN_GENERIC, _lib.MSG_WPLAN_UNI, _lib.MSG_WPLAN_ROW3, _lib.MSG_WPLAN_ROW3_W32}
    assert {p[fold] for _a, p in plans} == {0, 1} and {p[xcd_slices] for _a, p in plans} == {0, 1}
    assert any(p[owv] != a[7] for a, p in plans) and any(p[ohv] != a[6] for a, p in plans)      # padded rows (15 wide gives both)
    row3 = (_lib.MSG_WPLAN_ROW3, _lib.MSG_WPLAN_ROW3_W32)
    # per-sample weights, k_chunks 1: the row-sharing kernel chose the split (batch 8, 512 -> 512 @128^2: two K-slices per sample)
    own = {tuple(a): p for a, p in plans if p[kernel] in row3 and a[16] and a[17] == 1 and p[chunks_per_out] > 1}
    assert own[(bf16, 8, 128, 128, 512, 512, 128, 128, 512, 512, 512, 3, 3, 1, 1, 0, 1, 1)][chunks_per_out] == 2
    # the row-sharing kernel's geometry handed to the 128 x 128 kernel: 2 GiB behind one descriptor (shared weights: the batch)
    handed = [a for a, p in plans if p[kernel] not in row3 and a[0] == bf16 and a[11:16] == [3, 3, 1, 1, 0] and a[7] % 64 == 0 and
              a[2:4] == a[6:8] and not a[16] and a[1] * a[6] * a[7] * max(a[4], a[8]) * 2 >= 0x7ffffff0]
    assert handed and len(handed) == sum(1 for a, p in plans if a[0] == bf16 and a[11:16] == [3, 3, 1, 1, 0] and a[7] % 64 == 0 and
                                         a[2:4] == a[6:8] and not a[16] and p[kernel] not in row3)
    refused = [p for p in table["wgrad_plan"] if not isinstance(p, list)]
    assert _lib.MSG_EINVAL in refused and _lib.MSG_EUNSUPPORTED in refused
    # the exceptions are exactly the rows the four classes describe (thin-N + split + 65536-sample plans; thin queries; up-conv queries)
    assert truthful == {"plan": 60 + 51 + 2, "thin_eligible": 20, "upconv_eligible": 2}, truthful


def test_weight_gradient_codes_before_any_launch():
    """What msg_conv2d_wgrad answers without reaching a launch, on a geometry of the row-sharing kernel and one of the 128 x 128
    kernel whose sums are split: the codes the commit before conv_wgrad_select returned for the same calls (MSG_EINVAL argument
    checks before MSG_EUNSUPPORTED; alignment only with pointers; the workspace after the plan).  The pointers are fake, 16-byte
    aligned integers: every case returns before one is used."""
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    from tools.gen_dispatch_table import wgrad_plan
    build(verbose=False)
    lib = _lib.lib()
    OK, EINVAL, EUNSUPPORTED = _lib.MSG_OK, _lib.MSG_EINVAL, _lib.MSG_EUNSUPPORTED
    gy, x, gw, ws = 0x10000, 0x20000, 0x30000, 0x40000
    #        dtype          B  IH  IW  Cx  I   OH  OW ldgy  O ldgw kh kw s  p ps per-sample k_chunks
    geoms = {_lib.MSG_WPLAN_ROW3: [_lib.MSG_BF16, 2, 8, 64, 64, 64, 8, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 2],
             _lib.MSG_WPLAN_UNI: [_lib.MSG_BF16, 2, 32, 32, 64, 64, 32, 32, 64, 64, 64, 1, 1, 1, 0, 0, 0, 4]}
    for kernel, geom in geoms.items():
        plan = wgrad_plan(lib, geom)
        need = plan[10]
        assert plan[0] == kernel and plan[2] > 1 and need > 0 and need == lib.msg_conv2d_wgrad_workspace(*geom)

        def call(geom=geom, gy=gy, gw=gw, ws=ws, ws_floats=need):
            return lib.msg_conv2d_wgrad(gy, x, gw, *geom, 1, 0.5, ws, ws_floats, None)

        def changed(index, value):
            return geom[:index] + [value] + geom[index + 1:]
        assert call(gy=None) == EINVAL
        assert call(geom=changed(10, 60)) == EINVAL                     # ldgw < I
        assert call(geom=changed(10, 66)) == EINVAL                     # ldgw % 4
        assert call(gw=gw + 4) == EUNSUPPORTED                          # a misaligned gradient
        assert call(ws=None) == EINVAL
        assert call(ws_floats=need - 1) == EINVAL
        assert call(geom=changed(1, 0)) == OK                           # an empty batch
        assert call(geom=changed(1, 0), gy=None, ws=None, ws_floats=0) == OK
        assert call(geom=changed(17, 0)) == EINVAL                      # k_chunks
        # the queries answer the same codes for what they can see
        assert lib.msg_conv2d_wgrad_workspace(*changed(10, 60)) == EINVAL and wgrad_plan(lib, changed(17, 0)) == EINVAL
        assert lib.msg_conv2d_wgrad_workspace(*changed(1, 0)) == 0 and wgrad_plan(lib, changed(1, 0)) == [0] * _lib.MSG_WPLAN_FIELDS


def test_weight_gradient_auto_split_is_the_python_rule():
    """k_chunks = MSG_WGRAD_K_AUTO is the rule the Python layer used to compute and pass (tools/gen_dispatch_table.py keeps it,
    frozen, as model_k_chunks): over every row of the weight-gradient grid on which that rule gives a split, the plan and the
    workspace under AUTO are those under the rule's number -- every field, or the code -- and on the models' rows, which the grid
    builds with that number, they are therefore the recorded answers too.  Then the corners by direct queries (no launch runs)."""
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    from tools import gen_dispatch_table as grid
    build(verbose=False)
    lib = _lib.lib()
    AUTO, OK, EINVAL, EUNSUPPORTED = _lib.MSG_WGRAD_K_AUTO, _lib.MSG_OK, _lib.MSG_EINVAL, _lib.MSG_EUNSUPPORTED
    assert AUTO == -1
    with open(os.path.join(GOLDEN, "dispatch_table.json")) as f:
        table = json.load(f)

    def rule(r):                 # dtype B IH IW Cx I OH OW ldgy O ldgw kh kw stride pad shuffle per_sample [k_chunks]
        return grid.model_k_chunks(r[1], r[9], r[5], r[11] * r[12], r[6], r[7], r[16], 64 if r[0] == _lib.MSG_BF16 else 32)

    rows = grid.wgrad_plan_rows()
    n_ws = len(grid.wgrad_rows())                                      # (the workspace table is the first rows of the plan table)
    assert len(rows) == len(table["wgrad_plan"]) and grid.digest(rows) == table["digest"]["wgrad_plan"]
    compared, recorded = 0, set()
    for n, r in enumerate(rows):
        if r[1] < 1 or min(r[2], r[3], r[5], r[6], r[7], r[9], r[11], r[12]) < 1 or rule(r) < 1:
            continue
        kc, auto = rule(r), r[:17] + [AUTO]
        assert grid.wgrad_plan(lib, auto) == grid.wgrad_plan(lib, r[:17] + [kc]), (r, kc)
        assert lib.msg_conv2d_wgrad_workspace(*auto) == lib.msg_conv2d_wgrad_workspace(*r[:17], kc), (r, kc)
        compared += 1
        if kc == r[17]:                                                # the row IS the rule's call: the recorded answer
            assert grid.wgrad_plan(lib, auto) == table["wgrad_plan"][n], (r, kc)
            assert n >= n_ws or lib.msg_conv2d_wgrad_workspace(*auto) == table["wgrad_workspace"][n], (r, kc)
            recorded.add(n)
    # the rows wgrad_rows() builds with model_k_chunks -- per (batch, shared / per-sample): the 'same' convs of LAYERS at 1x1 and
    # 3x3, the stride-2 convs, the up-convolutions, then four groups of three thin layers of which the first has it -- all did
    per_block = [2 * sum(len(sizes) for _i, _o, sizes in grid.LAYERS) + sum(len(sizes) for _c, sizes in grid.STRIDE2) +
                 len(grid.SIZES) - 1, 3 * 4]
    model = {blk * sum(per_block) + k for blk in range(2 * len(grid.BATCHES)) for k in range(sum(per_block))
             if k < per_block[0] or (k - per_block[0]) % 3 == 0}
    assert len(model) == 2 * len(grid.BATCHES) * (per_block[0] + 4) and max(model) < n_ws
    assert all(rows[n][0] == _lib.MSG_BF16 and rows[n][17] == rule(rows[n]) for n in model)
    assert model <= recorded and compared >= len(recorded), (compared, len(recorded), len(model))
    assert any(rows[n][17] > 1 for n in model if rows[n][16]) and any(rows[n][17] > 1 for n in model if not rows[n][16])

    bf16 = _lib.MSG_BF16
    gy, x, gw, ws = 0x10000, 0x20000, 0x30000, 0x40000                  # fake, 16-byte aligned: every call returns before using one

    def answers(geom):           # the plan query, the workspace query, and the launch (a code only where it stops before a launch)
        return (grid.wgrad_plan(lib, geom), lib.msg_conv2d_wgrad_workspace(*geom),
                lib.msg_conv2d_wgrad(gy, x, gw, *geom, 0, 1.0, ws, 1 << 40, None))
    # shared weights that cannot fold (B * pixels = 2^31): the only place the shared-weight number reaches the kernel
    big = [bf16, 16384, 512, 256, 64, 64, 512, 256, 64, 64, 64, 1, 1, 1, 0, 0, 0]
    kc = grid.model_k_chunks(16384, 64, 64, 1, 512, 256, 0, 64)
    plan = grid.wgrad_plan(lib, big + [AUTO])
    assert kc >= 1 and plan == grid.wgrad_plan(lib, big + [kc]) and isinstance(plan, list)
    assert plan[7] == 0 and plan[1] == 16384 * kc and plan[2] == plan[1]                 # not folded: k_chunks slices per sample
    assert lib.msg_conv2d_wgrad_workspace(*big, AUTO) == lib.msg_conv2d_wgrad_workspace(*big, kc) == plan[10] > 0
    # shared weights over more than 65535 samples: the rule's loop ends at 0 slices -- MSG_EINVAL, as through the Python layer before
    many = [bf16, 65536, 4, 4, 64, 64, 4, 4, 64, 64, 64, 1, 1, 1, 0, 0, 0]
    assert grid.model_k_chunks(65536, 64, 64, 1, 4, 4, 0, 64) == 0
    assert answers(many + [AUTO]) == (EINVAL, EINVAL, EINVAL)
    assert isinstance(grid.wgrad_plan(lib, many + [1]), list)                            # (the caller's own number is taken)
    small = [bf16, 2, 8, 64, 64, 64, 8, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0]
    changed = lambda index, value: small[:index] + [value] + small[index + 1:]
    assert isinstance(grid.wgrad_plan(lib, small + [AUTO]), list)
    assert answers(changed(1, 0) + [AUTO]) == ([0] * _lib.MSG_WPLAN_FIELDS, 0, OK)        # an empty batch
    assert answers(small + [-2]) == (EINVAL, EINVAL, EINVAL) and answers(small + [0]) == (EINVAL, EINVAL, EINVAL)
    assert answers(changed(10, 60) + [AUTO]) == (EINVAL, EINVAL, EINVAL)                 # ldgw < I
    assert answers(changed(4, 60) + [AUTO]) == (EUNSUPPORTED, EUNSUPPORTED, EUNSUPPORTED)   # Cx: no whole 16-byte vectors
    assert answers(changed(4, 60)[:10] + [60, 3, 3, 1, 1, 0, 0, AUTO]) == (EINVAL, EINVAL, EINVAL)   # ... MSG_EINVAL first


def test_forward_codes_before_any_launch():
    """What msg_conv2d_fprop, msg_conv2d_fprop_act_mask and msg_conv2d_fprop_act_backward answer without reaching a launch, on a
    geometry of the row-sharing kernel and one of the ping-pong kernel: the codes the commit before fprop_check / fprop_plan_for
    returned for the same calls (MSG_EINVAL argument checks before MSG_EUNSUPPORTED; alignment only with pointers; the sign-byte
    and row-sharing gates and the workspace after the plan), and the plan query answers the same codes for what it can see.  The
    pointers are fake, 16-byte aligned integers: every case returns before one is used.
    Two kinds of call answer differently since, both wrong in two ways at once: the argument checks now come before the
    plan everywhere, so (a) a sign-byte mask on a problem of another kernel whose batch is empty or whose arguments are invalid
    gets the checks' answer (it was MSG_EUNSUPPORTED), and (b) the activation backward, which took its plan without them, answers
    MSG_EINVAL for an extent <= 0 (it was MSG_EUNSUPPORTED) and MSG_EUNSUPPORTED for a misaligned x / w / y (it launched)."""
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    from tools.gen_dispatch_table import fprop_plan
    build(verbose=False)
    lib = _lib.lib()
    OK, EINVAL, EUNSUPPORTED = _lib.MSG_OK, _lib.MSG_EINVAL, _lib.MSG_EUNSUPPORTED
    x, w, y, aux, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    #       dtype         B   IH   IW   Cx   Ck   OH   OW   N   ldy kh kw s  p  up ps w_batch_stride
    row3 = [_lib.MSG_BF16, 16, 128, 128, 256, 256, 128, 128, 256, 256, 3, 3, 1, 1, 1, 0, 0]
    pp = [_lib.MSG_BF16, 16, 128, 128, 256, 256, 128, 128, 256, 256, 1, 1, 1, 0, 1, 0, 0]
    assert fprop_plan(lib, row3 + [0, 0]) == fprop_plan(lib, row3 + [0, 1]) == [_lib.MSG_PLAN_ROW3, 256, 256]
    assert fprop_plan(lib, pp + [0, 0]) == fprop_plan(lib, pp + [0, 1]) == fprop_plan(lib, pp + [0, 3]) == [_lib.MSG_PLAN_PP, 256, 256]
    rows, entries = fprop_plan(lib, row3 + [0, 3])[3:]
    assert (rows, entries) == (16 * 64 * 2, 16 * 64 * 4)        # 64 pixel tiles per sample: two wave rows, four waves each

    def changed(geom, index, value):
        return geom[:index] + [value] + geom[index + 1:]

    def fprop(geom, x=x, w=w, y=y):
        return lib.msg_conv2d_fprop(x, w, None, y, *geom, None)

    def act_mask(geom, x=x, w=w, y=y, mask=None, noise=None):
        return lib.msg_conv2d_fprop_act_mask(x, w, y, *geom[:14], geom[16], None, noise, None, 1, 0.2, 1.0, mask, None)

    def act_backward(geom, x=x, w=w, y=y, sign_mask=aux, sign_map=None, tile=256, grad_bias=aux, ws=ws, ws_floats=rows * 256):
        return lib.msg_conv2d_fprop_act_backward(x, w, y, *geom[:14], geom[16], None, 0, sign_mask, tile, tile, sign_map, 256, 0.2, 1.0,
                                                 grad_bias, None, 1, None, ws, ws_floats, None)
    for call in (fprop, act_mask, act_backward):
        assert call(row3, x=None) == EINVAL and call(row3, y=None) == EINVAL
        assert call(changed(row3, 1, -1)) == EINVAL
        assert call(changed(row3, 0, 7)) == EUNSUPPORTED                # no such dtype
        assert call(changed(row3, 5, 224)) == EUNSUPPORTED              # Ck: not whole 128-byte runs
        assert call(changed(row3, 1, 0)) == OK                          # an empty batch
        assert call(changed(row3, 1, 0), x=None, w=None, y=None) == OK
    for call in (fprop, act_mask):
        assert call(row3, w=w + 8) == EUNSUPPORTED                      # a misaligned pointer
        assert call(changed(row3, 2, 0)) == EINVAL and call(changed(row3, 9, 0)) == EINVAL
        assert call(changed(row3, 9, 260)) == EUNSUPPORTED              # ldy: not whole vectors
    assert fprop(changed(changed(row3, 14, 2), 12, 2)) == EUNSUPPORTED  # zero insertion and a stride
    assert fprop(changed(changed(row3, 15, 1), 8, 258)) == EUNSUPPORTED  # pixel shuffle of N % 4
    assert act_mask(row3, noise=aux) == EINVAL                          # noise without its weight
    assert act_mask(pp, mask=aux) == EUNSUPPORTED                       # sign bytes: the row-sharing kernels alone
    assert act_mask(changed(pp, 1, 0), mask=aux) == OK and act_mask(pp, mask=aux, x=None) == EINVAL     # (a) above
    assert act_backward(row3, sign_mask=None) == EINVAL and act_backward(row3, sign_map=aux) == EINVAL   # exactly one sign source
    assert act_backward(pp) == EUNSUPPORTED                             # no row-sharing kernel: no such epilogue
    assert act_backward(changed(row3, 12, 2)) == EUNSUPPORTED and act_backward(changed(row3, 13, 0)) == EUNSUPPORTED
    assert act_backward(changed(row3, 9, 264)) == EUNSUPPORTED          # a pitched output
    assert act_backward(row3, ws=None) == EINVAL and act_backward(row3, ws_floats=rows * 256 - 1) == EINVAL
    assert act_backward(row3, tile=96) == EINVAL                        # sign bytes in tiles the kernel cannot read
    assert act_backward(changed(row3, 2, 0)) == EINVAL and act_backward(row3, y=y + 8) == EUNSUPPORTED   # (b) above
    # the query: the same codes for what it can see, and at epilogue 3 no partial sums where the launch is MSG_EUNSUPPORTED
    for epilogue in (0, 1, 2, 3):
        assert fprop_plan(lib, changed(row3, 1, -1) + [0, epilogue]) == EINVAL
        assert fprop_plan(lib, changed(row3, 0, 7) + [0, epilogue]) == EUNSUPPORTED
        assert fprop_plan(lib, changed(row3, 5, 224) + [0, epilogue]) == EUNSUPPORTED
        assert fprop_plan(lib, changed(row3, 1, 0) + [0, epilogue]) == [0]
        assert fprop_plan(lib, changed(row3, 9, 260) + [0, epilogue]) == EUNSUPPORTED
    assert fprop_plan(lib, changed(changed(row3, 14, 2), 12, 2) + [0, 0]) == EUNSUPPORTED
    assert fprop_plan(lib, changed(changed(row3, 15, 1), 8, 258) + [0, 0]) == EUNSUPPORTED
    for geom in (pp, changed(row3, 12, 2), changed(row3, 13, 0), changed(row3, 9, 264)):
        assert len(fprop_plan(lib, geom + [0, 3])) <= 3


def test_non_square_conv_geometry_is_refused():
    """EqualizedConv2d keeps the reference's (h, w) tuple arguments; a non-square stride / padding must raise instead
    of being computed with the first entry (round-1 advice)."""
    from multi_stylegan_amd import _lib, conv_ops
    assert conv_ops._square((2, 2), "stride") == 2 and conv_ops._square(1, "padding") == 1
    for bad in ((1, 2), (2, 1), (1, 1, 1)):
        with pytest.raises(_lib.MsgHipError, match="square"):
            conv_ops._square(bad, "stride")


def test_weight_image_store_contract():
    """weight_images: an image of a Parameter is kept until that parameter changes -- an in-place write, a step of the
    optimizer that owns it, invalidate_weight_cache for it or for all -- and no longer; a different gain is a different entry;
    a tensor that is no Parameter is never stored.  And the shapes the torch builders give."""
    from multi_stylegan_amd import weight_images as wi
    torch.manual_seed(0)
    w, v = torch.nn.Parameter(torch.randn(24, 16, 3, 3)), torch.nn.Parameter(torch.randn(8, 16, 3, 3))

    def image(p, gain=0.5):
        return wi.forward(p, torch.bfloat16, gain)[0]
    iw, iv = image(w), image(v)
    assert image(w) is iw and image(v) is iv                                   # a second request: the same object
    assert torch.equal(iw, wi._torch_fwd(w.detach(), torch.bfloat16)[0] * 0.5)     # (the gain after the cast, in bf16)
    with torch.no_grad():
        w.add_(1.0)
    assert image(w) is not iw and image(v) is iv                               # an in-place write renews w alone
    iw = image(w)
    w.grad = torch.ones_like(w)
    torch.optim.SGD([w], lr=0.1).step()
    assert image(w) is not iw and image(v) is iv                               # the step of w's optimizer: w alone
    iw = image(w)
    wi.invalidate_weight_cache([v])
    assert image(v) is not iv and image(w) is iw                               # v alone
    iw, iv = image(w), image(v)
    wi.invalidate_weight_cache()
    assert image(w) is not iw and image(v) is not iv                           # both
    iw = image(w)
    other = image(w, 0.25)
    assert other is not iw and image(w) is iw and image(w, 0.25) is other      # a different gain: a different entry
    assert torch.equal(other, wi._torch_fwd(w.detach(), torch.bfloat16)[0] * 0.25)
    plain = w.detach().clone()
    assert image(plain) is not image(plain) and "_msg_relay" not in plain.__dict__      # no Parameter: never stored
    assert torch.equal(image(plain), iw)

    f, ck = wi._torch_fwd(w.detach(), torch.bfloat16)
    d, ok = wi._torch_dgrad(w.detach(), torch.bfloat16, flip=True)
    s2, ok2, taps, pad2 = wi._relay_dgrad_s2(w.detach(), torch.bfloat16, 1)
    assert tuple(f.shape) == (24, 9, 64) and ck == 64
    assert tuple(d.shape) == (16, 9, 64) and ok == 64
    assert tuple(s2.shape) == (64, 4, 64) and (ok2, taps, pad2) == (64, 2, 0)
    assert wi.dgrad(w, torch.bfloat16)[0].shape == d.shape and wi.dgrad_s2(w, torch.bfloat16, 1.0, 1)[1:] == (64, 2, 0)


# ------------------------------------------------------------------------------ trainer surface, host logic
def _cpu_trainer(golden, **kw):
    """The product's ModelWrapper driving the CPU oracle's modules: the trainer's control flow (step order, zeroing,
    late-training branches, top-k, clipping, EMA, checkpoints) is device-agnostic and is checked here without a GPU;
    the same iterations run on the HIP modules in tests/test_hip_models.py."""
    import copy
    from multi_stylegan_amd.model_wrapper import ModelWrapper
    from oracle import models as om
    from tools.gen_golden import TINY_D, TINY_G
    z = golden("train_step")
    g, d = om.Generator(TINY_G), om.Discriminator(TINY_D, no_rfp=True)
    g.load_state_dict(z.state_dict("train.G0.")); d.load_state_dict(z.state_dict("train.D0."))
    ema = copy.deepcopy(g)
    ema.load_state_dict(z.state_dict("train.Gema0."))
    for mod in (g, ema):
        mod.live_parameters = lambda mod=mod: [p for n, p in mod.named_parameters()
                                               if not n.startswith("main_convolutions_2.")]
    orig_forward = g.forward

    def forward(*a, path_length_noise=None, **k):            # the oracle draws the image noise inside (generator.py:195)
        if path_length_noise is None:
            return orig_forward(*a, **k)
        from oracle.train import _pl_grads
        k.pop("return_path_length_grads")
        return _pl_grads(g, k.pop("input"), k.pop("inject_index"), k.pop("noise"), path_length_noise)
    g.forward = forward
    return z, g, d, ModelWrapper(g, d, generator_ema=ema, device="cpu", **kw)


def test_trainer_three_golden_iterations_on_cpu(golden):
    """ModelWrapper.train_iteration (host logic) against the reference-driven golden run, iteration 32 included: wrongly
    ordered reals, CutMix augmentation + consistency, top-k with v = 0.5 -- every optimiser step whole."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import check_step_trace
    from multi_stylegan_amd import loss, model_wrapper
    from test_oracle_golden import GOLDEN_ITERATIONS, STEP_LABELS, load_train_draws, split_trace, step_traces
    z, g, d, tr = _cpu_trainer(golden)
    top_k = loss.TopK(0, 1)
    names = {"cut_mix_aug": "loss_cut_mix_augmentation", "cut_mix_reg": "loss_cut_mix_regularization",
             "loss_g": "loss_generator", "r1": "loss_discriminator_regularization", "loss_pl": "loss_path_length_regularization"}
    for step, (iteration, late) in enumerate(GOLDEN_ITERATIONS):
        real, draws = load_train_draws(z, step, model_wrapper)
        tr.iteration = iteration - 1
        tr.step_trace = {}
        tr.train_iteration(real, draws, resume_training=late, top_k=top_k if late else None)
        log = tr.pop_logs()
        pre = f"train.it{step}."
        want_steps, want_ema = step_traces(z, pre)
        got_steps, got_ema = split_trace(tr.step_trace)
        assert list(got_steps) == STEP_LABELS[iteration]
        for label, want in want_steps.items():
            st = check_step_trace(got_steps[label], want, tol_grad=5e-4, tol_norm=1e-4, tol_delta=2e-3)
            assert st["compared"] > 0.2 * st["total"], (label, st)
        for n, want in want_ema.items():
            assert rel_err(got_ema[n], want) < 2e-3, n
        for short, long in names.items():
            if z.keys(pre + "log." + short):
                want = float(z[pre + "log." + short])
                assert abs(log[long][0] - want) <= 2e-4 * abs(want), (short, log[long][0], want)


def test_checkpoint_round_trip_and_reference_layout(golden, tmp_path):
    """save_checkpoint writes the reference's six entries (model_wrapper.py:181-192); load_checkpoint restores a run
    exactly, and also accepts the reference's own layouts: DataParallel `module.` prefixes, the ADA wrapper's
    `discriminator.` prefix, an empty path-length entry."""
    from multi_stylegan_amd import model_wrapper
    from test_oracle_golden import load_train_draws
    z, g, d, tr = _cpu_trainer(golden)
    real, draws = load_train_draws(z, 1, model_wrapper)
    tr.iteration = 15
    tr.train_iteration(real, draws)                           # both regularisers fire: optimiser state, PL mean
    path = str(tmp_path / "models" / "checkpoint_5.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=False)
    assert list(ck)[:6] == ["generator_ema", "generator", "generator_optimizer", "discriminator",
                            "discriminator_optimizer", "path_length_regularization"]
    assert float(ck["path_length_regularization"]["mean_path_length"]) == float(tr.path_length_regularization.mean_path_length)
    _, g2, d2, tr2 = _cpu_trainer(golden)
    tr2.load_checkpoint(path)
    assert tr2.iteration == 16
    for a, b in ((g, g2), (d, d2), (tr.generator_ema, tr2.generator_ema)):
        for (n, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(p, q), n
    assert torch.equal(tr.path_length_regularization.mean_path_length, tr2.path_length_regularization.mean_path_length)
    # the resumed run continues identically (optimiser moments restored, gradients still inside the flat buckets)
    real, draws = load_train_draws(z, 0, model_wrapper)
    for t in (tr, tr2):
        t.train_iteration(real, draws)
    for p, q in zip(list(g.parameters()) + list(d.parameters()), list(g2.parameters()) + list(d2.parameters())):
        assert torch.equal(p, q)
    assert all(p.grad.data_ptr() >= b.flat.data_ptr() for b in tr2.generator_reducer.buckets for p in b.params)
    # reference layouts
    ref = {"generator": {"module." + k: v for k, v in ck["generator"].items()},
           "generator_ema": {"module." + k: v for k, v in ck["generator_ema"].items()},
           "discriminator": {"discriminator.module." + k: v for k, v in ck["discriminator"].items()},
           "generator_optimizer": ck["generator_optimizer"], "discriminator_optimizer": ck["discriminator_optimizer"],
           "path_length_regularization": {}}
    _, g3, d3, tr3 = _cpu_trainer(golden)
    tr3.path_length_regularization.mean_path_length = torch.tensor([0.25])
    tr3.load_checkpoint(ref)
    assert float(tr3.path_length_regularization.mean_path_length) == 0.25
    for n, q in d3.state_dict().items():
        assert torch.equal(ck["discriminator"][n], q), n
    for n, q in tr3.generator_ema.state_dict().items():
        assert torch.equal(ck["generator_ema"][n], q), n
    wrapped = tr.checkpoint_dict(data_parallel_prefix=True)
    assert all(k.startswith("module.") for k in wrapped["generator_ema"])


def test_train_loop_schedules(golden, tmp_path):
    """train(): top-k marks from the epoch / dataset length (model_wrapper.py:115-125), the wrong-order switch at
    3/4 of the epochs, checkpoints every n epochs."""
    z, g, d, tr = _cpu_trainer(golden)
    seen = []
    tr.train_iteration = lambda real, draws=None, resume_training=False, top_k=None: seen.append(
        (tr.epoch, tr.epoch >= tr.hyperparameters["wrong_order_start"] * tr.epochs, resume_training,
         None if top_k is None else (top_k.starting_iteration, top_k.final_iteration)))
    data = [torch.zeros(2, 2, 3, 32, 32)] * 3
    tr.train(data, epochs=4, save_model_after_n_epochs=2, top_k=True, checkpoint_directory=str(tmp_path))
    assert len(seen) == 12 and seen[0] == (0, False, False, (3, 9)) and seen[-1] == (3, True, False, (3, 9))
    assert sorted(os.listdir(tmp_path)) == ["checkpoint_2.pt", "checkpoint_4.pt"]
    seen.clear()
    tr.train(data, epochs=1, resume_training=True, top_k=True)
    assert seen[0][2:] == (True, (0, 1))


def _topk_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from multi_stylegan_amd import dist as msg_dist
    torch.manual_seed(7)
    everything = torch.randn(world, 6)
    everything[1] -= 5.0 * (world > 1)                      # rank 1 mostly loses ...
    for v, case in ((0.5, everything), (0.5, everything * torch.tensor([[1.0], [0.0]]) + torch.tensor([[0.0], [-9.0]])),
                    (1.0, everything), (0.01, everything)):
        index, factor = msg_dist.global_top_k(case[rank], v)
        k = max(1, int(case.numel() * v))
        kept = torch.topk(case.reshape(-1), k).indices
        mine = sorted((kept[(kept >= rank * 6) & (kept < rank * 6 + 6)] - rank * 6).tolist())
        if mine:
            assert sorted(index.tolist()) == mine and abs(factor - len(mine) * world / k) < 1e-12
        else:
            assert index.tolist() == [0] and factor == 0.0    # ... and sometimes keeps nothing at all
        # the ranks' averaged weighted means equal the mean over the global k best
        local = case[rank][index].mean() * factor
        total = local.clone()
        dist.all_reduce(total)
        assert abs(total.item() / world - case.reshape(-1)[kept].mean().item()) < 1e-6
    if rank == 0:
        out.put("ok")
    dist.destroy_process_group()


def test_global_top_k_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + os.getpid() % 300
    procs = [ctx.Process(target=_topk_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert q.get(timeout=5) == "ok"


def test_ada_controller_on_cpu_matches_oracle():
    """The device-side p controller of AdaptiveDiscriminatorAugmentation is plain tensor arithmetic: on CPU tensors it
    must follow the reference's host-side controller (oracle/ada.py, adaptive_discriminator_augmentation.py:76-94)."""
    from multi_stylegan_amd.adaptive_discriminator_augmentation import AdaptiveDiscriminatorAugmentation
    from oracle import ada as oa
    torch.manual_seed(4)
    ada = AdaptiveDiscriminatorAugmentation(torch.nn.Identity(), p_step=0.02, r_update=3, p_max=0.1)
    ref = oa.Controller(p_step=0.02, r_update=3, p_max=0.1)
    for i in range(45):
        bias = 1.0 if i < 25 else -1.0
        a, b = torch.randn(4, 1) + bias, torch.randn(4, 1, 1, 6, 6) + bias
        ada._observe(a, b)
        ref.observe(a, b, is_real=False)
        assert abs(ada.p - ref.p) < 1e-6, i
    assert len(ada.r_history) == len(ref.r_history) == 15


def test_metric_statistics_match_the_reference_values(golden):
    """multi_stylegan_amd.validation_metrics: the Frechet distance (streamed moments + symmetric eigendecomposition) against
    values the reference's own FID._calc_fid / FVD._calc_fvd produced (tests/golden/metrics.npz), whole and in ragged
    batches with a sample limit; the inception score against the oracle; the range normalisations against the reference's."""
    import numpy as np
    from multi_stylegan_amd import misc, validation_metrics as vm
    from oracle import metrics as omet
    z = golden("metrics")
    for case in ("wide", "few_samples", "shifted"):
        real, fake, want = z[f"frechet.{case}.real"], z[f"frechet.{case}.fake"], float(z[f"frechet.{case}.value"])
        got = vm.frechet_distance(real, fake)
        assert abs(got - want) <= 1e-6 * abs(want), (case, got, want)
        # streamed: ragged batches, float32 features, a limit that cuts the last batch (the reference truncates its lists)
        n = real.shape[0] - 5
        mr, mf = vm.FeatureMoments(limit=n), vm.FeatureMoments(limit=n)
        for lo in range(0, real.shape[0], 37):
            mr.update(real[lo:lo + 37].float()); mf.update(fake[lo:lo + 37].float())
        assert mr.n == mf.n == n and mr.full
        want_cut = omet.frechet_distance(real[:n].float().double().numpy(), fake[:n].float().double().numpy())
        assert abs(vm.frechet_distance_from_moments(mr, mf) - want_cut) <= 1e-6 * abs(want_cut)
    rng = np.random.default_rng(3)
    p = rng.dirichlet(np.ones(11), size=64)
    assert abs(vm.inception_score(torch.from_numpy(p)) - omet.inception_score(p)) < 1e-10
    assert torch.equal(misc.normalize_0_1_batch(z["normalize.x"]), z["normalize.y01"])
    assert torch.equal(misc.normalize_m1_1_batch(z["normalize.x"]), z["normalize.ym11"])
    frames = vm.select_frames(z["normalize.x"], 1, generator=torch.Generator().manual_seed(0))
    t = int(torch.randint(0, 2, (1,), generator=torch.Generator().manual_seed(0)))
    assert frames.shape == (3, 3, 1, 5, 4) and torch.equal(frames, omet.select_frames(z["normalize.x"], 1, t))
    with pytest.raises(ValueError, match="feature network"):
        vm.FID(None)


class _ToyGenerator(torch.nn.Module):
    """Stands in for the generator in the statistics sweeps (any module with `latent_dimensions` mapping latents to
    [B, 2, 3, H, W] images will do; the real one needs the GPU)."""
    latent_dimensions = 6

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, 2 * 3 * 8 * 8)

    def forward(self, input):
        z = input[0] if isinstance(input, (list, tuple)) else input
        return torch.sigmoid(self.lin(z)).view(-1, 2, 3, 8, 8)


class _ToyFeatures(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.rows = []

    def forward(self, x):
        f = torch.stack([x.mean(dim=tuple(range(1, x.ndim))), x.flatten(1).std(dim=1), x.flatten(1)[:, 0],
                         x.flatten(1)[:, -1] * 2.0], dim=1)
        self.rows.append(f.double())
        return f


def _validation_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from multi_stylegan_amd import validation_metrics as vm
    from oracle import metrics as omet
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)
    gen, net = _ToyGenerator(), _ToyFeatures()
    for p_ in gen.parameters():
        dist.broadcast(p_.data, 0)
    dataset = [torch.rand(3, 2, 3, 8, 8) for _ in range(5)]                  # rank-distinct shard: 15 rows
    metric = vm.FID(net, device="cpu", batch_size=3, data_samples=20, no_rfp=True, no_gfp=True)
    got = metric(gen, dataset)
    # every rank swept ceil(20 / 2) = 10 rows of its data (4 batches, the last cut) and 10 generated rows (4 batches)
    assert len(net.rows) == 8
    mine = torch.stack([torch.cat(net.rows[:4])[:10], torch.cat(net.rows[4:])[:10]])
    both = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    real, fake = torch.cat([b[0] for b in both]), torch.cat([b[1] for b in both])
    want = omet.frechet_distance(real.numpy(), fake.numpy())
    assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (got, want)
    assert metric.moments_real[0].n == 20
    scores = [torch.tensor([got], dtype=torch.float64) for _ in range(world)]
    dist.all_gather(scores, torch.tensor([got], dtype=torch.float64))
    assert scores[0].item() == scores[1].item()                            # the same score on every rank
    # inception score: every rank's 10 probability rows gathered
    net2 = _ToyFeatures()
    is_got = vm.IS(net2, device="cpu", batch_size=5, data_samples=20, no_rfp=True, no_gfp=True, input_size=None)(gen)
    probs = torch.cat(net2.rows).float().softmax(dim=1)
    parts = [torch.empty_like(probs) for _ in range(world)]
    dist.all_gather(parts, probs)
    assert abs(is_got - omet.inception_score(torch.cat(parts).numpy())) < 1e-6
    # a dataset that runs out before data_samples rows: says so instead of caching short statistics silently
    short = vm.FID(_ToyFeatures(), device="cpu", batch_size=3, data_samples=40, no_rfp=True, no_gfp=True)
    with pytest.warns(UserWarning, match="fewer than data_samples"):
        short(gen, dataset)
    assert short.moments_real[0].n == 30
    if rank == 0:
        out.put("ok")
    dist.destroy_process_group()


def test_validation_statistics_are_shared_over_ranks_gloo_world2():
    """A data-parallel validation pass: each rank sweeps its share of the samples, the additive moments (and the inception
    score's probability rows) are exchanged, every rank reports the statistic of the union (advisor, round 4)."""
    _run_ranks(_validation_worker, 2, 29100 + os.getpid() % 300, 120)


def test_generated_call_wrappers_bind_every_entry_point():
    """multi_stylegan_amd._msg_fastcall (generated by csrc_host/gen_fastcall.py, built by build()): one wrapper per entry point
    that returns a status / size, bound to the dlopen handle ctypes holds; same results as ctypes on the entry points that
    need no GPU, argument-count and range errors raised like ctypes raises them."""
    from multi_stylegan_amd import _lib
    h = _lib.lib()
    assert h.fastcall, "build() did not produce _msg_fastcall.so (or MSG_NO_FASTCALL is set)"
    from multi_stylegan_amd import _msg_fastcall as fast
    ints = [n for n, (res, _a) in _lib._SIGNATURES.items() if res in (_lib._I, _lib._L)]
    assert all(callable(getattr(fast, n)) for n in ints)
    assert all(getattr(h, n) is getattr(fast, n) for n in ints)            # lib() hands out the wrappers ...
    assert h.msg_build_arch() == b"gfx950"                                # ... and ctypes for the string-valued entries
    assert h.msg_abi_version() == h._ctypes.msg_abi_version() == _lib.ABI_VERSION
    geoms = [(1, 16, 256, 256, 512, 512, 256, 256, 512, 3, 3, 0), (1, 32, 256, 256, 128, 128, 256, 256, 128, 3, 3, 0),
             (1, 16, 4, 4, 512, 512, 4, 4, 512, 3, 3, 512 * 9 * 512), (0, 2, 9, 9, 16, 32, 9, 9, 24, 3, 3, 0)]
    for g in geoms:
        assert h.msg_conv2d_fprop_plan(*g) == h._ctypes.msg_conv2d_fprop_plan(*g)
    assert h.msg_bias_act_backward_workspace(1 << 20, 1, 512, 1) == h._ctypes.msg_bias_act_backward_workspace(1 << 20, 1, 512, 1)
    assert h.msg_softmax_rows(None, None, 0, 4, 1024, None) == -1         # MSG_EINVAL: None is a NULL pointer, as with ctypes
    with pytest.raises(TypeError):
        h.msg_conv2d_fprop_plan(1, 2, 3)
    with pytest.raises(OverflowError):
        h.msg_conv2d_fprop_plan(1 << 40, *geoms[0][1:])
    with pytest.raises(TypeError):
        h.msg_conv2d_fprop_plan("1", *geoms[0][1:])


def test_bench_multi_rank_fields():
    """What bench.py's JSON line reports about the ranks (the fields the 8-GPU run is read by), on canned timings."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    f = bench.multi_rank_fields(4, "nccl", False, 16, 20, [2.0, 2.5, 2.2, 2.4], 131.0)
    assert f["rccl_ranks"] == 4 and f["backend"] == "nccl" and f["rehearsal_shared_gpu"] is False
    assert f["per_rank_img_per_s"] == [160.0, 128.0, 145.45, 133.33]
    assert f["overlap"] == {"on_ms_per_step": 125.0, "off_ms_per_step": 131.0}        # the slowest rank's 2.5 s / 20 steps
    one = bench.multi_rank_fields(1, None, False, 16, 20, [2.25], None)
    assert one["rccl_ranks"] == 1 and one["backend"] is None and one["overlap"] is None
    reh = bench.multi_rank_fields(2, "gloo", True, 4, 3, [1.0, 1.0], 340.0)
    assert reh["backend"] == "gloo" and reh["rehearsal_shared_gpu"] is True


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last step's losses in float64, every model's parameters in float32 -- whole, or a seeded
    sample of DUMP_SAMPLE of them that is the same in every run and holds the parameters' own values."""
    import importlib.util
    import types
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert 3 * bench.DUMP_SAMPLE * 4 <= 64 * 2 ** 20                      # the dump stays within 64 MB at any size
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    torch.manual_seed(0)
    big, small = torch.nn.Linear(8, 8), torch.nn.Linear(2, 3)            # 72 parameters (sampled) and 9 (whole)
    trainer = types.SimpleNamespace(generator=big, discriminator=small, generator_ema=big)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), trainer, {"loss_generator": [0.25], "path_length": [1.5]})
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["discriminator_params.npy", "generator_ema_params.npy",
                                                            "generator_params.npy", "loss_generator.npy", "path_length.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == (np.float64 if n.startswith(("loss", "path")) else np.float32) and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "path_length.npy").tolist() == [1.5]
    whole = torch.cat([p.detach().reshape(-1) for p in small.parameters()]).numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "discriminator_params.npy"), whole)
    sample = np.load(tmp_path / "a" / "generator_params.npy")
    flat = torch.cat([p.detach().reshape(-1) for p in big.parameters()]).numpy()
    assert sample.shape == (50,) and np.isin(sample, flat).all()


def test_conv_kernel_case_table_selects_the_kernels_it_names():
    """tests/conv_kernel_cases.py, the shapes the float64-referenced GPU tests of the large-tile kernels run (test_hip_conv.py::
    test_large_tile_kernels_against_float64): msg_conv2d_fprop_launch_plan on the launches each case turns into names the kernel the
    case is for -- the forward launch plain, with a bias, with the fused activation and with the residual merge (the last three for
    the stride-1 convs, the launches that take them), then the data gradient.  Two shapes one tile below a floor name the 128 x 128
    kernels: an eligibility rule that moves shows up here, on any machine, not as coverage that quietly went elsewhere.  Then the
    table as a whole: every large-tile kernel with both weight modes and as a data gradient, and the tails and map widths the
    kernels branch on."""
    import conv_kernel_cases as table
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    from tools.gen_dispatch_table import fprop_plan
    build(verbose=False)
    lib = _lib.lib()
    code = lambda kernel: getattr(_lib, "MSG_PLAN_" + kernel)
    names = [c.name for c in table.CASES + table.GUARD_CASES]
    assert len(set(names)) == len(names) and set(table.EPILOGUE_CASES) <= set(table.BY_NAME)
    large = {"PP", "ROW3", "ROW3N"}
    fwd, dgrad = [], []                      # (case, launch) of the launches that run on a large tile
    for c in table.CASES + table.GUARD_CASES:
        f, d = table.launches(c, _lib.MSG_BF16)
        assert fprop_plan(lib, list(f))[0] == code(c.fwd), (c.name, "forward")
        if c.kind == "conv" and c.stride == 1:
            for has_bias, epilogue in ((1, 0), (0, 1), (0, 2)):
                leg = table.launches(c, _lib.MSG_BF16, has_bias, epilogue)[0]
                assert fprop_plan(lib, list(leg))[0] == code(c.fwd), (c.name, "forward", has_bias, epilogue)
        if c.dgrad is None:                  # a guard row
            assert c.fwd not in large
            continue
        assert fprop_plan(lib, list(d))[0] == code(c.dgrad), (c.name, "data gradient")
        assert c.fwd in large or c.dgrad in large, c.name
        fwd += [(c, f)] if c.fwd in large else []
        dgrad += [(c, d)] if c.dgrad in large else []
    assert {c.fwd for c, _ in fwd if not c.per_sample} == large and {c.fwd for c, _ in fwd if c.per_sample} == large
    assert {c.dgrad for c, _ in dgrad} == large
    T = table
    pp = [(c, a) for c, a in fwd if c.fwd == "PP"] + [(c, a) for c, a in dgrad if c.dgrad == "PP"]
    assert any(a[T.PIXEL_SHUFFLE] for c, a in fwd if c.fwd == "PP") and any(a[T.PIXEL_SHUFFLE] for c, a in dgrad if c.dgrad == "PP")
    assert any(table.gemm_rows(a) % 256 for _, a in pp), "ragged last M tile"
    assert any(a[T.N_] % 256 for _, a in pp), "N tail"
    assert any(a[T.CX] < a[T.CK] for _, a in pp), "Cx < Ck"
    row_sharing = [a for c, a in fwd if c.fwd != "PP"] + [a for c, a in dgrad if c.dgrad != "PP"]
    assert {32, 64, 128, 256, 512} <= {a[T.OW] for a in row_sharing}


def test_streaming_conv_case_tables_select_the_kernels_they_name():
    """THIN_CASES, UPCONV_CASES and STREAM_GUARD_CASES of tests/conv_kernel_cases.py, the shapes test_hip_conv.py runs on
    conv_thin.hip and conv_upconv.hip: msg_conv2d_fprop_launch_plan names THIN for every thin row plain and with a bias, and for
    the thin K rows with the residual epilogue too; UPCONV for every up-convolution row; and for each guard row, one step outside
    a rule, the other kernel the row names.  Then the tables as a whole: every instantiation of the thin kernels (KC = Ck / 32, NV =
    N / 8), the output counts either side of the half-wave boundary, both weight modes, ragged pixel counts, every
    groups_per_wave the grid rule gives (through the table's mirror of thin_grid), and for the up-convolution fewer slices than
    waves, a ragged round of slices, both workgroup orders and a ragged last tile."""
    import conv_kernel_cases as table
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    from tools.gen_dispatch_table import fprop_plan
    build(verbose=False)
    lib, T, bf16 = _lib.lib(), table, _lib.MSG_BF16
    code = lambda kernel: getattr(_lib, "MSG_PLAN_" + kernel)
    names = [c.name for c in T.THIN_CASES + T.UPCONV_CASES] + [c.name for _, c, _ in T.STREAM_GUARD_CASES]
    assert len(set(names)) == len(names)
    assert set(T.THIN_LARGE) | set(T.THIN_K_RESIDUAL_CASES) <= set(T.THIN_BY_NAME)
    thin_n, thin_k = [], []
    for c in T.THIN_CASES:
        legs = [(0, 0), (1, 0)] + ([(0, 2)] if c.O > 8 else [])
        for has_bias, epilogue in legs:
            assert fprop_plan(lib, list(T.thin_launch(c, bf16, has_bias, epilogue)))[0] == code("THIN"), (c.name, has_bias, epilogue)
        (thin_n if c.O <= 8 else thin_k).append((c, T.thin_launch(c, bf16)))
    assert all(a[T.CX] >= a[T.CK] for _, a in thin_n) and all(a[T.CX] == 8 for _, a in thin_k)      # which of the two modes a row is
    assert all(T.THIN_BY_NAME[n].O > 8 for n in T.THIN_K_RESIDUAL_CASES)
    for c in T.UPCONV_CASES:
        assert fprop_plan(lib, list(T.upconv_launch(c, bf16)))[0] == code("UPCONV"), c.name
    for family, c, kernel in T.STREAM_GUARD_CASES:
        assert kernel not in ("THIN", "UPCONV")
        args = T.thin_launch(c, bf16) if family == "thin" else T.upconv_launch(c, bf16)
        assert fprop_plan(lib, list(args))[0] == code(kernel), (c.name, "guard")
    # the N = 1 and N = 4 rows differ in N only: one side and the other of the half-wave boundary on the same pixels
    n1, n4 = T.THIN_BY_NAME["n_n1_ragged"], T.THIN_BY_NAME["n_n4_ragged"]
    assert n1._replace(name="", O=0) == n4._replace(name="", O=0) and (n1.O, n4.O) == (1, 4)
    # thin N
    assert {a[T.CK] // 32 for _, a in thin_n} == {2, 4, 6, 8, 12, 16}, "KC"
    assert {1, 4, 5, 8} <= {a[T.N_] for _, a in thin_n}, "N"
    assert {c.per_sample for c, _ in thin_n} == {False, True}
    assert any(T.gemm_rows(a) % 16 for _, a in thin_n), "ragged last group"
    assert any(T.gemm_rows(a) % 16 == 1 for _, a in thin_n), "a last group of one pixel"
    assert any(a[T.CX] > a[T.CK] for _, a in thin_n), "a channel slice of a wider map"
    assert {T.thin_groups_per_wave(a) for _, a in thin_n} == {1, 2, 8}
    # thin K
    assert {a[T.N_] // 8 for _, a in thin_k} == {8, 16, 32, 64}, "NV"
    assert {c.per_sample for c, _ in thin_k} == {False, True}
    assert {T.thin_groups_per_wave(a) for _, a in thin_k} == {8, 16}
    nv64 = [(c, a) for c, a in thin_k if a[T.N_] == 512]
    # (conv_thin_launch: the scalar-load kernel takes NV 64 when a sample is a whole number of 64-byte runs, 4 pixels)
    assert any(c.per_sample and c.H * c.W % 4 for c, _ in nv64) and any(not c.per_sample for c, _ in nv64)
    assert {T.THIN_BY_NAME[n].O // 8 for n in T.THIN_K_RESIDUAL_CASES} == {8, 32, 64}
    assert sorted(T.THIN_BY_NAME[n].per_sample for n in T.THIN_K_RESIDUAL_CASES if T.THIN_BY_NAME[n].O == 512) == [False, True]
    # the layers run forward and backward: both launches are thin
    for b, i, o, h, w, ps in T.THIN_DGRAD_LAYERS:
        for cin, cout in ((i, o), (o, i)):
            assert fprop_plan(lib, list(T.thin_launch(T.Thin("", b, cin, cout, h, w, ps), bf16)))[0] == code("THIN"), (b, cin, cout, h, w)
    # up-convolution
    up = [T.upconv_launch(c, bf16) for c in T.UPCONV_CASES]
    assert any(a[T.N_] // 64 < 8 for a in up), "fewer slices than waves"
    assert any(a[T.N_] // 64 % 8 for a in up if a[T.N_] // 64 > 8), "a ragged round of slices"
    assert any(a[T.B_] % 8 == 0 and a[T.B_] > 8 for a in up) and any(a[T.B_] % 8 for a in up), "both workgroup orders"
    assert any(a[T.OH] * a[T.OW] % 128 for a in up), "ragged last tile"
    assert any(a[T.OW] % 2 for a in up), "odd W"
