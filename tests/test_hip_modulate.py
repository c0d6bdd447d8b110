"""csrc/modulate.hip through the C ABI (include/msg_hip.h), entry by entry, against the float64 definitions of
tests/modulate_util.py (themselves checked against the CPU oracle in tests/test_modulate_reference.py) -- at the shapes where
each branch of the kernels and of their launch rules can go wrong: sample groups with a ragged last group, the generic fold,
the limits of the four-channel folds, the second passes of the tiling loops, the zero padding of the weight images.

Bounds.  Entries with a reduction (msg_demod_coeff, the d of msg_modulate_weights, both folds): max(8 * e32, 2^-21) on
max|got - ref| / max|ref|, e32 being the same error of modulate_util run in float32 on the CPU for the same case -- the factor 8
covers another summation order and the hardware reciprocal square root.  Element-wise images: per element 2^-21 |ref| in f32 (at
most five fp32 roundings), one bf16 unit in the last place in bf16, where the bf16 image must also be the f32 image rounded to
nearest even once; columns c >= C exactly zero.  Every output is pre-filled with NaN and followed by a guard row: all of it must
be written, nothing behind it.

Largest errors measured on the MI355X (the case closest to its bound, per entry and quantity), next to that bound:
    msg_demod_coeff           d         6.5e-08  of 4.8e-07   (B,O,I,T) = (2,3,512,9); 3.8e-08 from msg_modulate_weights' d_out
    msg_modulate_weights      d         9.0e-08  of 4.8e-07   reduce-C256;  f32 image 0.20 x its per-element bound (B17 groups)
    msg_modulate_backward     gW        1.9e-07  of 6.4e-07   v4 B5 O3 g1 I40 T4;   generic kernel 1.0e-07 of 4.8e-07
                              gs_part   1.0e-07  of 4.9e-07   v4 B3 I12 T4;         generic kernel 1.4e-07 of 7.9e-07
    msg_modulate_backward2    gW        1.3e-07  of 5.2e-07   v4 B3 I4 T4
                              gs_part   2.7e-07  of 6.9e-07   v4 B3 I512 T1
    msg_scale_rows_cols       f32 image 0.37 x its per-element bound (2^-21 |ref|); bf16 image 1 bf16 unit at most
    msg_scale_rows_cols2      f32 image 0.40 x its per-element bound;               bf16 image 1 bf16 unit at most
Every reduction stayed under 0.4 of its bound.  Each case prints its own figures; the fixture prints the largest.
"""
import functools

import pytest
import torch

import modulate_util as mu
from abi_util import DEV, Guarded, _ptr, _shifted, _stream
from conftest import rel_err

pytestmark = pytest.mark.gpu
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
FLOOR = 2.0 ** -21
GAIN = 0.37
EPS = 1e-8
WORST = {}                              # entry / quantity -> (error, bound, case): printed when the module is done


@pytest.fixture(scope="module")
def lib():
    from multi_stylegan_amd import _lib
    yield _lib.lib()
    for key in sorted(WORST):
        print("\nworst %-38s %.2e  (bound %.2e, %s)" % ((key,) + WORST[key]), end="")
    print()


def _note(key, err, bound, case):
    print("%s %s: %.2e (bound %.2e)" % (key, case, err, bound))
    if key not in WORST or err / bound > WORST[key][0] / WORST[key][1]:
        WORST[key] = (err, bound, case)


def _dev(t):
    return t.to(DEV, torch.float32).contiguous()


# ------------------------------------------------------------------------------------------- element-wise images
def _check_image(entry, case, got, ref, mag, code, c, rel=FLOOR, got_f32=None):
    """got [B,R,T,Ck] against ref [B,R,T,C], sample by sample: a wrong sample index shows as a whole wrong sample."""
    assert bool((got[..., c:] == 0).all()), f"{entry} {case}: columns c >= C are not all zero"
    body = got[..., :c]
    if code == F32:
        err, bound = (body - ref).abs(), rel * mag
    else:
        err, bound = (body - mu.bf16_rne(ref)).abs(), mu.bf16_ulp(ref)
        assert torch.equal(got, mu.bf16_rne(got_f32)), f"{entry} {case}: the bf16 image is not the f32 image rounded once (RNE)"
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30)
    _note(entry + (" f32" if code == F32 else " bf16") + " [x bound]", float(ratio.max()), 1.0, case)
    bad = (err > bound).flatten(1).any(dim=1)
    assert not bool(bad.any()), f"{entry} {case}: samples {bad.nonzero().flatten().tolist()} are outside the bound " \
                                f"(worst element at {float(ratio.max()):.3g} x bound)"


SRC_GROUPS = {1: "bg1", 2: "bg2", 3: "bg2+1-ragged", 5: "bg4+1-ragged", 8: "bg8", 9: "bg8+1-ragged", 16: "bg8+8",
              17: "bg8+8+1-ragged"}
# id, B, R, T, C, Ck, storage codes
SRC_CASES = [("groups-%s-B%d" % (SRC_GROUPS[b], b), b, 2048, 1, 8, 8, (F32, BF16)) for b in SRC_GROUPS] + [
    ("columns-C3-elementwise-pad-to-8", 2, 3, 9, 3, 8, (F32, BF16)),
    ("columns-C6-run-ends-mid-vector", 2, 3, 9, 6, 8, (F32, BF16)),
    ("columns-C7-pad-to-16", 2, 3, 9, 7, 16, (F32, BF16)),
    ("columns-C40-zero-vectors-to-64", 2, 3, 9, 40, 64, (F32, BF16)),
    ("columns-C40-no-padding", 2, 3, 9, 40, 40, (F32,)),
    ("columns-C264-no-padding", 2, 3, 9, 264, 264, (F32, BF16)),
    ("columns-C512-no-padding", 2, 3, 9, 512, 512, (F32, BF16)),
    ("loops-cvecs258-second-column-pass", 2, 2, 9, 1032, 1032, (F32,)),
    ("loops-cvecs256-tstep1-T9-second-tap-pass", 2, 2, 9, 1024, 1024, (F32,)),
    ("loops-cvecs257-bf16-second-column-pass", 2, 2, 4, 2056, 2056, (BF16,)),
]
SRC_PARAMS = [pytest.param(c[:6], code, id=c[0] + ("-f32" if code == F32 else "-bf16")) for c in SRC_CASES for code in c[6]]


@functools.lru_cache(maxsize=None)
def _src_inputs(b, r, t, c):
    gen = torch.Generator().manual_seed(1000 * b + 10 * c + t)
    style = functools.partial(mu.draw, gen, mean=1.0, std=0.5)
    return {"base": mu.draw(gen, r, t, c), "row1": style(b, r), "col1": style(b, c), "row2": style(b, r), "col2": style(b, c)}


def _scale_rows_cols(lib, code, base, row, col, b, r, t, c, ck, out_shift=0):
    out = Guarded((b, r, t, ck), ck, TORCH_DTYPE[code])
    rc = lib.msg_scale_rows_cols(base, row, col, out.ptr + out_shift, code, b, r, t, c, ck, GAIN, _stream())
    return rc, out


def _scale_rows_cols2(lib, code, base, row1, col1, row2, col2, b, r, t, c, ck, out_shift=0):
    out = Guarded((b, r, t, ck), ck, TORCH_DTYPE[code])
    rc = lib.msg_scale_rows_cols2(base, row1, col1, row2, col2, out.ptr + out_shift, code, b, r, t, c, ck, GAIN, _stream())
    return rc, out


@pytest.mark.parametrize("case,code", SRC_PARAMS)
def test_scale_rows_cols(lib, case, code):
    name, b, r, t, c, ck = case
    x = _src_inputs(b, r, t, c)
    base, row, col = _dev(x["base"]), _dev(x["row1"]), _dev(x["col1"])
    for has_row, has_col in ((True, True), (True, False), (False, True), (False, False)):
        hr, hc = (x["row1"] if has_row else None), (x["col1"] if has_col else None)
        ref = mu.scaled(x["base"], hr, hc, GAIN).expand(b, r, t, c)
        args = (base.data_ptr(), _ptr(row if has_row else None), _ptr(col if has_col else None), b, r, t, c, ck)
        rc, out = _scale_rows_cols(lib, F32, *args)
        assert rc == OK
        got32 = out.read()
        what = f"{name} rowscale={'yes' if has_row else 'NULL'} colscale={'yes' if has_col else 'NULL'}"
        if code == F32:
            _check_image("scale_rows_cols", what, got32, ref, ref.abs(), F32, c)
        else:
            rc, out = _scale_rows_cols(lib, BF16, *args)
            assert rc == OK
            _check_image("scale_rows_cols", what, out.read(), ref, ref.abs(), BF16, c, got_f32=got32)


@pytest.mark.parametrize("case,code", SRC_PARAMS)
def test_scale_rows_cols2(lib, case, code):
    name, b, r, t, c, ck = case
    x = _src_inputs(b, r, t, c)
    ref = mu.scaled2(x["base"], x["row1"], x["col1"], x["row2"], x["col2"], GAIN)
    # the two terms may cancel: the bound is on what was added, not on the sum
    mag = mu.scaled2(x["base"].abs(), x["row1"].abs(), x["col1"].abs(), x["row2"].abs(), x["col2"].abs(), GAIN)
    ops = [_dev(x[k]) for k in ("base", "row1", "col1", "row2", "col2")]
    args = tuple(o.data_ptr() for o in ops) + (b, r, t, c, ck)
    rc, out = _scale_rows_cols2(lib, F32, *args)
    assert rc == OK
    got32 = out.read()
    if code == F32:
        _check_image("scale_rows_cols2", name, got32, ref, mag, F32, c)
    else:
        rc, out = _scale_rows_cols2(lib, BF16, *args)
        assert rc == OK
        _check_image("scale_rows_cols2", name, out.read(), ref, mag, BF16, c, got_f32=got32)


@pytest.mark.parametrize("code", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["base", "colscale"])
def test_scale_rows_cols_unaligned_operand_takes_the_elementwise_loads(lib, which, code):
    """C = 8 with `base` or `colscale` 4 bytes off a 16-byte boundary (al = false in the kernels): bit for bit the aligned result."""
    b, r, t, c, ck = 2, 3, 9, 8, 8
    x = _src_inputs(b, r, t, c)
    ops = {k: _dev(v) for k, v in x.items()}
    ptrs = {k: v.data_ptr() for k, v in ops.items()}
    keep, moved = _shifted(ops["base" if which == "base" else "col1"])
    off = dict(ptrs, **{"base" if which == "base" else "col1": moved})
    keep2, moved2 = _shifted(ops["col2"])
    results = []
    for p in (ptrs, off):
        rc, out = _scale_rows_cols(lib, code, p["base"], p["row1"], p["col1"], b, r, t, c, ck)
        assert rc == OK
        results.append(out.read())
    assert torch.equal(results[0], results[1])
    off2 = dict(off, col2=moved2) if which == "colscale" else off
    results = []
    for p in (ptrs, off2):
        rc, out = _scale_rows_cols2(lib, code, p["base"], p["row1"], p["col1"], p["row2"], p["col2"], b, r, t, c, ck)
        assert rc == OK
        results.append(out.read())
    assert torch.equal(results[0], results[1])


def test_scale_rows_cols_refusals_leave_the_output_alone(lib):
    b, r, t, c = 2, 3, 9, 8
    x = {k: _dev(v) for k, v in _src_inputs(b, r, t, c).items()}
    p = {k: v.data_ptr() for k, v in x.items()}
    one = lambda code, ck, **kw: _scale_rows_cols(lib, code, p["base"], p["row1"], p["col1"], b, r, t, c, ck, **kw)
    two = lambda code, ck, row1=p["row1"], **kw: _scale_rows_cols2(lib, code, p["base"], row1, p["col1"], p["row2"], p["col2"],
                                                                  b, r, t, c, ck, **kw)
    for call in (one, two):
        for rc_want, (rc, out) in ((EUNSUPPORTED, call(BF16, 12)),            # Ck % 8 in bf16
                                   (EUNSUPPORTED, call(F32, 10)),             # Ck % 4 in f32
                                   (EUNSUPPORTED, call(F32, 8, out_shift=4)),  # misaligned output
                                   (EINVAL, call(F32, 4))):                   # Ck < C
            assert rc == rc_want
            out.assert_untouched()
    rc, out = two(F32, 8, row1=None)
    assert rc == EINVAL
    out.assert_untouched()


# ------------------------------------------------------------------------------------------- msg_modulate_weights / msg_demod_coeff
# id, B, O, R, T, C, Ck
MODW_CASES = [
    ("groups-bg2-O1024-B2", 2, 1024, 1024, 1, 8, 8),
    ("groups-bg2+1-ragged-O1024-B3", 3, 1024, 1024, 1, 8, 8),
    ("groups-bg8+1-ragged-O1024-B9", 9, 1024, 1024, 1, 8, 8),
    ("groups-bg4+1-ragged-O512-T9-B5", 5, 512, 512, 9, 8, 8),
    ("groups-bg8+8+1-ragged-O512-T9-B17", 17, 512, 512, 9, 8, 8),
    ("groups-bg1-O8-T9-C40-pad-to-64", 3, 8, 8, 9, 40, 64),
    ("upconv-rows-O6-R24-C40-pad-to-64", 3, 6, 24, 1, 40, 64),
] + [("reduce-C%d-O3-T9" % c, 2, 3, 3, 9, c, 8 * ((c + 7) // 8)) for c in (4, 6, 252, 256, 260, 512)]


@functools.lru_cache(maxsize=None)
def _modw_case(b, o, r, t, c):
    """base [R][T][C] with rows r = q * O + o (q: the sub-pixel of the 2x2 transposed conv, one tap each; q = 0 for a conv) is
    the weight W[o][c][(q, t)] -> the inputs and the float64 d [B,O] and image [B,R,T,C]."""
    gen = torch.Generator().manual_seed(7 * b + o + 3 * r + t + 11 * c)
    base, style = mu.draw(gen, r, t, c), mu.draw(gen, b, c, mean=1.0, std=0.5)
    q = r // o
    W = base.reshape(q, o, t, c).permute(1, 3, 0, 2).reshape(o, c, q * t)
    scale = mu.conv_scale(c, q * t)
    w, d = mu.weights(W, style, scale, True, EPS)
    ref = w.reshape(b, o, c, q, t).permute(0, 3, 1, 4, 2).reshape(b, r, t, c)
    d32 = mu.weights(W.float(), style.float(), scale, True, EPS)[1]
    wsq = W.square().sum(dim=2).float()                        # [O][C], float64 sum rounded once
    return {"base": base, "style": style, "wsq": wsq, "scale": scale, "d": d, "ref": ref, "W": W,
            "d_bound": max(8 * rel_err(d32, d), FLOOR)}


def _modulate_weights(lib, code, x, b, o, r, t, c, ck, with_d=True):
    ops = [_dev(x[k]) for k in ("base", "wsq", "style")]
    out, d_out = Guarded((b, r, t, ck), ck, TORCH_DTYPE[code]), Guarded((b, o), o)
    rc = lib.msg_modulate_weights(*(v.data_ptr() for v in ops), out.ptr, d_out.ptr if with_d else None, code, b, r, o, t, c, ck,
                                  x["scale"], EPS, _stream())
    assert rc == OK
    if not with_d:
        d_out.assert_untouched()
    return out.read(), (d_out.read() if with_d else None)


@pytest.mark.parametrize("code", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", MODW_CASES, ids=[c[0] for c in MODW_CASES])
def test_modulate_weights(lib, case, code):
    name, b, o, r, t, c, ck = case
    x = _modw_case(b, o, r, t, c)
    got32, d_got = _modulate_weights(lib, F32, x, b, o, r, t, c, ck)
    _note("modulate_weights d", rel_err(d_got, x["d"]), x["d_bound"], name)
    assert rel_err(d_got, x["d"]) <= x["d_bound"]
    for with_d in (True, False):
        got32_n = got32 if with_d else _modulate_weights(lib, F32, x, b, o, r, t, c, ck, with_d=False)[0]
        assert torch.equal(got32_n, got32), "d_out = NULL changed the image"
        if code == F32:
            _check_image("modulate_weights", name, got32_n, x["ref"], x["ref"].abs(), F32, c, rel=x["d_bound"] + FLOOR)
        else:
            got, d16 = _modulate_weights(lib, BF16, x, b, o, r, t, c, ck, with_d=with_d)
            assert d16 is None or rel_err(d16, x["d"]) <= x["d_bound"]
            err = (got[..., :c] - mu.bf16_rne(x["ref"])).abs()
            assert bool((err <= mu.bf16_ulp(x["ref"])).all()), f"{name}: more than one bf16 unit from the reference"
            assert bool((got[..., c:] == 0).all()), f"{name}: columns c >= C are not all zero"
            assert torch.equal(got, mu.bf16_rne(got32)), f"{name}: the bf16 image is not the f32 image rounded once (RNE)"


DEMOD_CASES = [(3, 5, 6, 3), (2, 3, 512, 9), (1, 2, 700, 1), (16, 1, 4, 4)]


def _demod_coeff(lib, W, s, b, o, i, t, scale):
    wd, sd, d = _dev(W), _dev(s), Guarded((b, o), o)
    assert lib.msg_demod_coeff(wd.data_ptr(), sd.data_ptr(), d.ptr, b, o, i, t, scale, EPS, _stream()) == OK
    return d


@pytest.mark.parametrize("shape", DEMOD_CASES, ids=["demod_coeff-B%d-O%d-I%d-T%d" % c for c in DEMOD_CASES])
def test_demod_coeff(lib, shape):
    b, o, i, t = shape
    x = _modw_case(b, o, o, t, i)                                  # (the conv image [O][T][I] of the same weight)
    W = x["W"].contiguous()                                        # [O][I][T]
    got = _demod_coeff(lib, W, x["style"], b, o, i, t, x["scale"]).read()
    _note("demod_coeff d", rel_err(got, x["d"]), x["d_bound"], str(shape))
    assert rel_err(got, x["d"]) <= x["d_bound"]
    _, d_fused = _modulate_weights(lib, F32, x, b, o, o, t, i, 4 * ((i + 3) // 4))
    _note("demod_coeff vs modulate_weights d", rel_err(got, d_fused), FLOOR, str(shape))
    assert rel_err(got, d_fused) <= FLOOR


@pytest.mark.parametrize("code", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [MODW_CASES[6], MODW_CASES[5]], ids=["upconv-rows", "conv"])
def test_demod_coeff_then_scale_rows_cols_is_modulate_weights(lib, case, code):
    name, b, o, r, t, c, ck = case
    x = _modw_case(b, o, r, t, c)
    fused, _ = _modulate_weights(lib, code, x, b, o, r, t, c, ck)
    q = r // o
    d = _demod_coeff(lib, x["W"].contiguous(), x["style"], b, o, c, q * t, x["scale"])
    d.read()
    rows = d.buf[:b * o].reshape(b, o).repeat(1, q).contiguous()   # rowscale[b][r] = d[b][r % O]
    base, style = _dev(x["base"]), _dev(x["style"])
    out = Guarded((b, r, t, ck), ck, TORCH_DTYPE[code])
    assert lib.msg_scale_rows_cols(base.data_ptr(), rows.data_ptr(), style.data_ptr(), out.ptr, code, b, r, t, c, ck,
                                   x["scale"], _stream()) == OK
    split = out.read()
    ref = x["ref"]
    each = (x["d_bound"] + FLOOR) * ref.abs() if code == F32 else mu.bf16_ulp(ref)
    assert bool(((split[..., :c] - fused[..., :c]).abs() <= 2 * each).all())
    assert bool((split[..., c:] == 0).all())


# ------------------------------------------------------------------------------------------- the folds
def _grouped(by_o, og):
    """[O,B,I] -> [ceil(O / og),B,I]: what one workgroup of the fold adds up."""
    return torch.stack([by_o[k:k + og].sum(dim=0) for k in range(0, by_o.shape[0], og)])


@functools.lru_cache(maxsize=None)
def _fold_inputs(b, o, i, t):
    gen = torch.Generator().manual_seed(b + 17 * o + 131 * i + 7 * t)
    W, s = mu.draw(gen, o, i, t), mu.draw(gen, b, i, mean=1.0, std=0.5)
    g, v = mu.draw(gen, b, o, t, i), mu.draw(gen, b, i)
    scale = mu.conv_scale(i, t)
    return {"W": W, "s": s, "g": g, "v": v, "scale": scale, "d": mu.weights(W, s, scale, True)[1]}


@functools.lru_cache(maxsize=None)
def _fold_ref(b, o, i, t, demod, second):
    """-> (float64 (gW, by_o), the same evaluated in float32)."""
    x = _fold_inputs(b, o, i, t)
    ops = (x["W"], x["s"], x["g"]) + ((x["v"],) if second else ())
    fn = mu.fold2 if second else mu.fold
    return fn(*ops, x["scale"], demod), fn(*(a.float() for a in ops), x["scale"], demod)


def _fold(lib, x, b, o, i, t, ldg, og, demod, second=False, gwk_shift=False, v_shift=False):
    """One call of msg_modulate_backward[2] on guarded outputs -> (rc, gW, gs_part); columns i >= I of gwk hold NaN."""
    gwk = torch.full((b, o, t, ldg), float("nan"), dtype=torch.float64)
    gwk[..., :i] = x["g"]
    gwk, W, s, d, v = _dev(gwk), _dev(x["W"]), _dev(x["s"]), _dev(x["d"]), _dev(x["v"])
    gp, vp = gwk.data_ptr(), v.data_ptr()
    if gwk_shift:
        keep_g, gp = _shifted(gwk)
    if v_shift:
        keep_v, vp = _shifted(v)
    groups = (o + og - 1) // og
    gW, gs_part = Guarded((o, i, t), i * t), Guarded((groups, b, i), i)
    head = (gp, W.data_ptr(), s.data_ptr(), d.data_ptr() if demod else None)
    tail = (gW.ptr, gs_part.ptr, b, o, i, t, ldg, og, x["scale"], _stream())
    rc = lib.msg_modulate_backward2(*head, vp, *tail) if second else lib.msg_modulate_backward(*head, *tail)
    torch.cuda.synchronize()
    return rc, gW, gs_part


def _check_fold(lib, entry, case, b, o, og, i, t, ldg, second=False, **kw):
    x = _fold_inputs(b, o, i, t)
    out = {}
    for demod in (True, False):
        (gW_ref, by_o), (gW_32, by_o_32) = _fold_ref(b, o, i, t, demod, second)
        part_ref, part_32 = _grouped(by_o, og), _grouped(by_o_32, og)
        rc, gW, gs_part = _fold(lib, x, b, o, i, t, ldg, og, demod, second, **kw)
        assert rc == OK
        gW, gs_part = gW.read(), gs_part.read()
        tag = f"{case} {'demod' if demod else 'd=NULL'}"
        bound = max(8 * rel_err(gW_32, gW_ref), FLOOR)
        _note(entry + " gW", rel_err(gW, gW_ref), bound, tag)
        assert rel_err(gW, gW_ref) <= bound, f"{tag}: gW"
        if second and not demod:
            assert float(gs_part.abs().max()) == 0.0, f"{tag}: gs_part must be written as exact zeros without demodulation"
        else:
            bound = max(8 * rel_err(part_32, part_ref), FLOOR)
            rows = [rel_err(gs_part[k], part_ref[k]) * float(part_ref[k].abs().max() / part_ref.abs().max())
                    for k in range(part_ref.shape[0])]
            _note(entry + " gs_part", max(rows), bound, tag)
            assert max(rows) <= bound, f"{tag}: gs_part rows (error of each, of max|ref|): {rows}"
            total_ref = by_o.sum(dim=0)
            bound = max(8 * rel_err(by_o_32.sum(dim=0), total_ref), FLOOR)
            assert rel_err(gs_part.sum(dim=0), total_ref) <= bound, f"{tag}: gs_part summed over the groups"
        out[demod] = (gW, gs_part)
    return out


def _v4_cases():
    cases = []
    for n, (i, t) in enumerate((i, t) for i in (4, 12, 252, 256, 260, 508, 512) for t in (1, 4, 9)):
        cases.append((3, 5, 2, i, t, i + 24 * (n % 2)))
    cases += [(1, 5, 2, 260, 9, 260), (2, 5, 2, 260, 9, 284), (15, 5, 2, 260, 9, 260), (16, 5, 2, 260, 9, 284)]
    cases += [(5, 5, 2, 40, 4, 40), (5, 3, 1, 40, 4, 64), (5, 4, 4, 40, 4, 40), (5, 3, 8, 40, 4, 64)]
    return cases


def _fold_id(kernel, c):
    b, o, og, i, t, ldg = c
    notes = [n for n, hit in (("one-lane", i == 4), ("all-lanes", i == 512), ("wave-boundary", i in (256, 260)),
                              ("half1-idle", b == 1), ("all-slots", b == 16), ("ragged-last-group", o % og and og < o),
                              ("group-beyond-O", og > o), ("padded-rows", ldg > i)) if hit]
    return "-".join(["%s-B%d-O%dg%d-I%d-T%d-ldg%d" % (kernel, b, o, og, i, t, ldg)] + notes)


V4_CASES = _v4_cases()
# the generic kernel, reached by legal arguments only: I % 4 != 0, ldg % 4 != 0, taps outside {1, 4, 9}
GENERIC_CASES = [(3, 5, 2, i, t, i + 3 * (n % 2)) for n, (i, t) in enumerate((i, t) for i in (6, 258, 511) for t in (2, 3, 9))] + [
    (3, 5, 2, 8, 4, 9), (3, 5, 2, 8, 5, 8), (1, 5, 2, 6, 3, 6), (16, 5, 2, 6, 3, 7)]


def _sum_rows_agrees(lib, gs_part):
    """msg_sum_rows over the groups (what the operator runs behind the fold) against the same sum in float64."""
    groups, b, i = gs_part.shape
    part, out = _dev(gs_part), Guarded((b, i), i)
    assert lib.msg_sum_rows(part.data_ptr(), out.ptr, groups, b * i, _stream()) == OK
    want = part.cpu().double().sum(dim=0)
    # `groups` fp32 additions in index order: (groups - 1) roundings of partial sums that stay below sum |part|
    bound = (groups - 1) * 2.0 ** -24 * part.cpu().double().abs().sum(dim=0)
    assert bool(((out.read() - want).abs() <= bound).all())


@pytest.mark.parametrize("case", V4_CASES, ids=[_fold_id("v4", c) for c in V4_CASES])
def test_modulate_backward_v4(lib, case):
    b, o, og, i, t, ldg = case
    out = _check_fold(lib, "modulate_backward v4", _fold_id("v4", case), b, o, og, i, t, ldg)
    _sum_rows_agrees(lib, out[True][1])


@pytest.mark.parametrize("case", GENERIC_CASES, ids=[_fold_id("generic", c) for c in GENERIC_CASES])
def test_modulate_backward_generic(lib, case):
    b, o, og, i, t, ldg = case
    out = _check_fold(lib, "modulate_backward generic", _fold_id("generic", case), b, o, og, i, t, ldg)
    _sum_rows_agrees(lib, out[True][1])


def test_modulate_backward_generic_by_unaligned_gradient_agrees_with_v4(lib):
    """I = 40, T = 9: gwk 4 bytes off a 16-byte boundary sends the same problem to the generic kernel."""
    b, o, og, i, t, ldg = 5, 5, 2, 40, 9, 40
    v4 = _check_fold(lib, "modulate_backward v4", "I40-T9-aligned", b, o, og, i, t, ldg)
    gen = _check_fold(lib, "modulate_backward generic", "I40-T9-gwk+4B", b, o, og, i, t, ldg, gwk_shift=True)
    for demod in (True, False):
        (gW_ref, by_o), (gW_32, by_o_32) = _fold_ref(b, o, i, t, demod, False)
        part_ref = _grouped(by_o, og)
        for a, c, ref, r32 in ((v4[demod][0], gen[demod][0], gW_ref, gW_32),
                               (v4[demod][1], gen[demod][1], part_ref, _grouped(by_o_32, og))):
            assert float((a - c).abs().max()) <= 2 * max(8 * rel_err(r32, ref), FLOOR) * float(ref.abs().max())


def test_modulate_backward_refusals_leave_the_outputs_alone(lib):
    x = _fold_inputs(3, 5, 8, 4)
    for want, kw in ((EUNSUPPORTED, dict(b=17)), (EUNSUPPORTED, dict(i=516, ldg=516)), (EUNSUPPORTED, dict(t=10)),
                     (EINVAL, dict(ldg=4)), (OK, dict(b=0))):
        a = dict(b=3, o=5, i=8, t=4, ldg=8)
        a.update(kw)
        for demod in (True, False):
            # (nothing is launched: the operands only have to be valid pointers)
            gwk, W, s, d = (torch.zeros(64, device=DEV) for _ in range(4))
            gW, gs_part = Guarded((64,), 64), Guarded((64,), 64)
            rc = lib.msg_modulate_backward(gwk.data_ptr(), W.data_ptr(), s.data_ptr(), d.data_ptr() if demod else None, gW.ptr,
                                           gs_part.ptr, a["b"], a["o"], a["i"], a["t"], a["ldg"], 2, x["scale"], _stream())
            assert rc == want, kw
            gW.assert_untouched()
            gs_part.assert_untouched()


@pytest.mark.parametrize("case", V4_CASES, ids=[_fold_id("v4", c) for c in V4_CASES])
def test_modulate_backward2_v4(lib, case):
    b, o, og, i, t, ldg = case
    _check_fold(lib, "modulate_backward2", _fold_id("v4", case), b, o, og, i, t, ldg, second=True)


def test_modulate_backward2_refusals_leave_the_outputs_alone(lib):
    for kw in (dict(i=6, ldg=8), dict(i=516, ldg=516), dict(t=3), dict(b=17), dict(v_off=4)):
        a = dict(b=3, o=5, i=8, t=4, ldg=8, v_off=0)
        a.update(kw)
        gwk, W, s, d, v = (torch.zeros(64, device=DEV) for _ in range(5))
        gW, gs_part = Guarded((64,), 64), Guarded((64,), 64)
        rc = lib.msg_modulate_backward2(gwk.data_ptr(), W.data_ptr(), s.data_ptr(), d.data_ptr(), v.data_ptr() + a["v_off"], gW.ptr,
                                        gs_part.ptr, a["b"], a["o"], a["i"], a["t"], a["ldg"], 2, 0.25, _stream())
        assert rc == EUNSUPPORTED, kw
        gW.assert_untouched()
        gs_part.assert_untouched()
