"""Kernel-level tests of the launches of the mixed modes (mix_mx, mix_mx4) that only the model path reaches, and of their formats: the FFN conv on mx4
operands (gemm_pl_bf16<1, 256, false, 3>) and on mx operands (ARITH = 2) with planes in and mx planes out, LayerNorm -> mx4 planes + scale record
(gemm_row4_bf16 EPI 4), FFN2 + LN2 in the mx arithmetic (ARITH = 2, RES = 2) with the residual from mx and from mx4 planes, and the weight repacks of
csrc/gemm_mx.h -- each launched on the shipped library through fs2_op_launch_gemm / fs2_op_repack_weight into sentinel buffers, its plan asserted (the same
blocks are planned on the CPU first: tests/test_gemm_raw_host.py).

Operands are the tuples the kernels read (tests/gemm_raw.py: the formats' one CPU statement), and every launch is held against the float64 value of ITS OWN
formula on those tuples -- ah.wh + scaled (ra.wh + ah.rw) in e4m3 or e2m1, not the ideal product -- so only fp32 accumulation separates the two, and a wrong
scale-byte position, swapped nibbles or a residual read at the wrong offset (2^-11 of a product, 1e-4 on the mel: below every whole-model bar) shows as an
error of 8 bars or more on the coherent operands (checked on the CPU, on the formula's mutants: test_conv_formula_tells_every_mutant_apart).

Bars (tests/gemm_raw.py: MX_BAR, with the measured figures next to them): 5 x the worst max-abs measured on the MI355X per launch, none above GEMM_TOL["bf16x3"];
the host tests hold the mutants at 8 of these bars.  Outputs read back from mx planes carry the planes' rounding on top: fp16 + e4m3 of the residual, 2^-14 |ref|
per element."""
import pytest
import torch

from tests import gemm_raw as G
from tests.test_gpu_ops import GEMM_TOL

pytestmark = pytest.mark.gpu

CEILING = GEMM_TOL["bf16x3"]
BAR = G.MX_BAR
_cache = {}


def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"


def _record(name, value, bar):
    from tests.conftest import record_measurement
    print("%s: max-abs %.3e (bar %.3e)" % (name, value, bar))
    record_measurement("mx_kernel_%s_maxabs" % name, value)


def test_bars_lie_at_or_below_the_ceiling():
    assert G.MX_CEILING == CEILING and all(0 < b <= CEILING for b in BAR.values())


# ------------------------------------------------------------------ the repacks
@pytest.mark.parametrize("fmt", ["mx", "mx4"])
@pytest.mark.parametrize("shape", [(256, 384, 3), (1024, 384, 9), (384, 1024, 1)], ids=lambda s: "N%d-C%d-k%d" % s)
def test_repack_images_equal_the_cpu_encoders(shape, fmt):
    """repack_weight_mx / repack_weight_mx4 as fs2_load_weights runs them (fs2_op_repack_weight) against tests/gemm_raw.py's encoders, byte for byte, with the
    static exponent kw and the scale image.  The weights avoid exact ties of the e2m1 conversion (G.repack_weights), where the byte would state the tie rule of
    the hardware instruction and nothing about positions; e4m3 ties stay in: the conversion rounds them to even, as the CPU's does."""
    _need_gpu()
    N, Cc, k = shape
    w = G.repack_weights(N, Cc, k, seed=N + Cc + k)
    img, sc, kw = G.repack_weight(w, fmt)
    want_kw = G.fp8_scale_exponent(float(w.abs().max()))
    assert kw == want_kw
    if fmt == "mx":
        want = G.image_w_mx(G.split_mx3(w, want_kw)).reshape(-1)
        assert sc is None
    else:
        want, want_sc = G.image_w_mx4(G.split_mx4(w, 0, slot_dim=1))
        want = want.reshape(-1)
        assert int((sc != want_sc.reshape(-1)).sum()) == 0, "%d bytes of the scale image differ" % int((sc != want_sc.reshape(-1)).sum())
        assert len(torch.unique(sc)) > 4
    diff = img != want
    assert int(diff.sum()) == 0, "%d of %d bytes of the %s image differ, the first at byte %d" % (int(diff.sum()), img.numel(), fmt, int(diff.nonzero()[0]))


# ------------------------------------------------------------------ the FFN conv
def _conv_results(key, x_from=None):
    """Both output forms of one conv case, once per session: (ops, {out: (plan, yp bytes, y bytes)})."""
    if key not in _cache:
        _need_gpu()
        arith, case, dist = key[:3]
        if x_from is None:
            ops = G.ConvOperands(arith, *case, dist)
            dev = G.ConvCase(ops)
        else:
            tuples, planes, rec = x_from
            ops = G.ConvOperands(arith, *case, dist, x_tuples=tuples)
            dev = G.ConvCase(ops, x_planes=planes, x_rowscale=rec)
        runs = {}
        for out in G.CONV_OUTS:
            plan, yp, y = dev.run(out)
            want = G.conv_expected(arith)
            assert {f: getattr(plan, f) for f in want} == want and not plan.rows_pass and not plan.build_planes, (key, out, plan)
            runs[out] = (plan, yp, y)
        _cache[key] = (ops, runs)
    return _cache[key]


def _check_conv(ops, runs, bar):
    """-> max-abs of the fp32 rows against the formula (the launch's own error: the planes, the same bytes with and without fp32 rows, add their rounding);
    asserts the bar on rows and planes, the untouched rows and guards, zero gap rows."""
    R, N = ops.R, ops.N
    n = R * N * 4
    gap = ops.pos[:R] < 0
    worst = 0.0
    for out, (_, yp, y) in runs.items():
        h, e8, a8 = G.decode_mx(yp, R, N)
        got = G.mx_value(h, e8, ops.kh)
        assert bool(torch.isfinite(got).all()), "%s: non-finite / unwritten planes in rows < R" % out
        err = (got - ops.ref).abs()
        print("conv %s k %d N %d R %d %s %s: planes max-abs %.3e (max |ref| %.2f)" % (ops.arith, ops.k, N, R, ops.dist, out, float(err.max()), float(ops.ref.abs().max())))
        assert bool((err < bar + 2.0 ** -14 * ops.ref.abs()).all()), "%s: max-abs %g" % (out, float(err.max()))
        assert G.untouched(yp, n), "%s wrote planes of a row >= R" % out
        assert int(yp[:n].reshape(R, -1)[gap].max()) == 0, "%s: a gap row is not zero" % out
        assert torch.equal(a8, G.e4m3_of((h.float() * 2.0 ** ops.kh).clamp(-448.0, 448.0))), "%s: the ah8 block is not e4m3(fp16 2^kh)" % out
        assert not bool(((e8 & 0x7F) == 0x7F).any())
        if out == "y_yp":
            rows = y[:n].view(torch.float32).reshape(R, N).double()
            assert bool(torch.isfinite(rows).all())
            e32 = float((rows - ops.ref).abs().max())
            print("    fp32 rows max-abs %.3e" % e32)
            worst = max(worst, e32)
            assert e32 < bar and G.untouched(y, n) and float(rows[gap].abs().max()) == 0.0
            assert bool(((rows - got).abs() <= 2.0 ** -14 * rows.abs() + 2.0 ** -24).all())
        else:
            assert G.untouched(y, 0)
    assert torch.equal(runs["yp"][1], runs["y_yp"][1]), "the planes differ between the two output forms"
    return worst


CONV_KEYS = [(a, c, d) for a in G.CONV_ARITHS for c in G.CONV_CASES for d in G.DISTS]


@pytest.mark.parametrize("key", CONV_KEYS, ids=["%s-k%d-N%d-R%d-%s" % ((k[0],) + k[1] + (k[2],)) for k in CONV_KEYS])
def test_conv_against_its_float64_formula(key):
    """The FFN conv (k taps, bias, ReLU, mx planes out, with and without fp32 rows) on mx4 planes + row scales + the mx4 weight image and its scale image, and
    on mx planes + the mx weight image under static scales, against the float64 value of the kernel's formula on the same tuples.  Behind row R the planes and
    the scale records hold 0xFF: the rows outside [0, R) count as zeros whatever lies there.
    Measured on the MI355X, fp32 rows, worst over the cases: mx4 8.44e-6, mx 9.68e-6 (k = 9, coherent operands); bars 4.2e-5 / 4.8e-5.  Read back from the mx
    planes the worst was 6.4e-5 at |ref| = 5.8, of which 2^-14 |ref| = 3.5e-4 is the planes' allowance."""
    ops, runs = _conv_results(key)
    name = "conv_" + key[0]
    worst = _check_conv(ops, runs, BAR[name])
    _record(name, worst, BAR[name])


# ------------------------------------------------------------------ LayerNorm -> mx4 planes (EPI 4) and the hand-off to the conv
def _epi4_results(case, fs2_option):
    if ("epi4",) + case not in _cache:
        _need_gpu()
        form, R, Cc = case
        ops = G.LnOperands(form, R, Cc)
        dev = G.LnCase(ops)
        runs = {}
        for side, mt in G.ROW4_RUNS:
            plan, yp, y = dev.run(side, mt, fs2_option)
            assert (plan.kernel, plan.epi, plan.res, plan.mt) == G.ln_expected(form, side, mt), (case, mt, plan)
            assert plan.nsplit == 3 and plan.ksplit == 1 and not plan.rows_pass and not plan.build_planes, plan
            assert G.untouched(y, 0)
            runs[mt] = (yp, dev.rowscale)
        _cache[("epi4",) + case] = (ops, runs)
    return _cache[("epi4",) + case]


EPI4_IDS = ["%s-R%d-C%d" % c for c in G.EPI4_CASES]


@pytest.mark.parametrize("case", G.EPI4_CASES, ids=EPI4_IDS)
def test_epi4_value_and_heights(case, fs2_option):
    """The value the planes state to a residual reader, fp16 + e4m3 residual 2^-(ka+11), against float64 with the bar of the mx-planes form; both tile heights the
    same bytes in planes and scale record; rows >= R, the guards and the eight record bytes no slot owns untouched; gap rows all-zero planes with the clamped byte.
    Measured on the MI355X: 6.33e-5 at |ref| <= 7.4 (R = 333), 6.30e-5 (R = 128); the bar is the mx-planes form's, 1.5e-4 + 2^-14 |ref|."""
    ops, runs = _epi4_results(case, fs2_option)
    R, n = ops.R, ops.R * G.N_OUT * 4
    gap = ops.pos[:R] < 0
    worst = 0.0
    for mt, (yp, rec) in runs.items():
        got, _ = ops.decode(yp)
        assert bool(torch.isfinite(got).all())
        err = (got - ops.ref).abs()
        print("epi4 R %d mt %d: max-abs %.3e (max |ref| %.2f)" % (R, mt, float(err.max()), float(ops.ref.abs().max())))
        worst = max(worst, float(err.max()))
        assert bool((err < BAR["epi4"] + 2.0 ** -14 * ops.ref.abs()).all()), "mt %d: max-abs %g" % (mt, float(err.max()))
        assert G.untouched(yp, n) and G.untouched(rec, R * 32)
        assert int(yp[:n].reshape(R, -1)[gap].max()) == 0, "mt %d: a gap row is not zero" % mt
        r = rec[:R * 32].reshape(R, 32)
        assert bool((r[:, 24:] == 0xFF).all()), "mt %d wrote record bytes no slot owns" % mt
        assert bool((r[gap][:, :24] == 40 - 11).all())
    assert torch.equal(runs[4][0][:n], runs[5][0][:n]) and torch.equal(runs[4][1][:R * 32], runs[5][1][:R * 32]), "the two heights differ"
    _record("epi4", worst, BAR["epi4"])


@pytest.mark.parametrize("case", G.EPI4_CASES, ids=EPI4_IDS)
def test_epi4_scale_record_and_nibbles(case, fs2_option):
    """The scale record exactly: every byte is the rule of csrc/common.h applied to the reference's slot maximum (a slot whose maximum lies within the bar of a
    binade edge may take either neighbour: counted, below 1 % -- tests/test_gemm_raw_host.py holds that on the reference alone); every ah4 nibble is the CPU e2m1
    code of the kernel's own fp16 value under the kernel's own scale byte; every ra4 nibble lies among the codes that the residuals rounding to the observed e4m3
    byte produce under that scale byte."""
    ops, runs = _epi4_results(case, fs2_option)
    R = ops.R
    yp, rec = runs[4]
    t = G.decode_mx4(yp, rec, R, G.N_OUT)
    lo, hi = G.epi4_scale_bounds(ops.ref, BAR["epi4"] + 2.0 ** -14 * ops.ref.abs())
    bad = (t.sb < lo) | (t.sb > hi)
    edge = int((lo != hi).sum())
    print("epi4 R %d: %d edge slots of %d; scale bytes %d .. %d" % (R, edge, lo.numel(), int(t.sb.min()), int(t.sb.max())))
    assert not bool(bad.any()), "%d scale bytes off the rule, the first at (row, slot) %s: %d, want %d .. %d" % (
        int(bad.sum()), tuple(bad.nonzero()[0].tolist()), int(t.sb[bad][0]), int(lo[bad][0]), int(hi[bad][0]))
    assert edge < 0.01 * lo.numel()
    inv = G.mx4_inv_scale(t.sb).repeat_interleave(16, dim=1)
    want_h4 = G.e2m1_encode(t.h.double() * inv)
    assert int((t.h4 != want_h4).sum()) == 0, "%d ah4 nibbles are not e2m1(fp16 / s)" % int((t.h4 != want_h4).sum())
    clo, chi = G.e4m3_cell(t.e8)
    f = 2.0 ** -G.KA_OUT * inv                                   # e4m3 holds r 2^(ka+11), the nibble e2m1(r 2^11 / s)
    vlo, vhi, v = G.e2m1_decode(G.e2m1_encode(clo * f)), G.e2m1_decode(G.e2m1_encode(chi * f)), G.e2m1_decode(t.r4)
    off = (v < vlo) | (v > vhi)
    assert not bool(off.any()), "%d ra4 nibbles outside the codes of their e4m3 residual" % int(off.sum())
    assert int((t.r4 & 7).max()) >= 2 and len(torch.unique(t.sb)) >= 6      # the residual nibbles are not all flushed; the slots take different bytes


def test_epi4_output_feeds_the_mx4_conv_as_it_is(fs2_option):
    """The hand-off: EPI 4's own output bytes -- planes and scale record -- are the A operand of the mx4 conv, and the conv's result is the float64 formula on those
    decoded bytes: the producer's and the consumer's position rules agree (scale byte of slot s at 8 u + 2 (s & 3) + (s >> 2), nibble pairs, units).  The CPU
    encoder puts the decoded tuples back into the same bytes.  Measured on the MI355X: 8.98e-7 on the fp32 rows; the launch is the mx4 conv's and so is the bar."""
    case = G.EPI4_CASES[0]
    lops, lruns = _epi4_results(case, fs2_option)
    R, Cc = lops.R, G.N_OUT
    yp, rec = lruns[5]
    Rp = G.rpad(R)
    t = G.decode_mx4(yp, rec, R, Cc)
    pad = lambda x: torch.cat([x, torch.zeros((Rp - R,) + x.shape[1:], dtype=x.dtype)])
    tuples = G.Mx4(*[pad(x) for x in t])
    planes, record = yp[:Rp * 4 * Cc].reshape(Rp, 4 * Cc), rec[:Rp * 32].reshape(Rp, 32)
    assert len(torch.unique(t.sb)) >= 6
    ops, runs = _conv_results(("mx4", (9, 256, R), "model", "handoff"), x_from=(tuples, planes, record))
    assert torch.equal(ops.x_planes[:R], planes[:R]) and torch.equal(ops.x_rowscale[:R, :24], record[:R, :24])
    worst = _check_conv(ops, runs, BAR["conv_mx4"])
    _record("handoff", worst, BAR["conv_mx4"])


# ------------------------------------------------------------------ FFN2 + LN2 in the mx arithmetic
FFN2_KEYS = [c + (d,) for c in G.FFN2_CASES for d in G.DISTS]


@pytest.mark.parametrize("key", FFN2_KEYS, ids=["C%d-R%d-rm%d-%s" % k for k in FFN2_KEYS])
def test_ffn2_mx_against_its_float64_formula(key, fs2_option):
    """FFN2 + LN2 in the mx arithmetic (k = 1, A as mx planes, the mx weight image, static scale bytes) with the residual from mx planes (rm 1) and from mx4
    planes (rm 2: the e4m3 residual at byte 3 C), at both tile heights, against the float64 formula -> LayerNorm; the heights write the same bytes.  The same
    values on the split-bf16 arithmetic (ARITH = 0, the epi0_res2 form) stay within the two bars of the formula (on the CPU the formula lies up to 1.8e-4 from
    the product of the bf16 pairs on the coherent operands: the e4m3 rounding of cross terms that all point one way).
    Measured on the MI355X: worst 3.08e-5 (C = 1024, R = 333, residual from mx4 planes, coherent); 5 x that passes the ceiling, so the bar is the ceiling 1.5e-4.
    The split-bf16 sibling: worst 1.86e-4 from the formula, against 3.0e-4."""
    _need_gpu()
    ops = G.Ffn2Operands(*key)
    dev = G.Ffn2Case(ops)
    R, n = ops.R, ops.R * G.N_OUT * 4
    gap = ops.pos[:R] < 0
    worst, planes = 0.0, {}
    for mt in (4, 5):
        plan, yp = dev.run(mt, fs2_option)
        assert (plan.kernel, plan.epi, plan.arith, plan.res, plan.mt) == ("row4", 0, 2, 2, mt), plan
        assert plan.nsplit == 3 and plan.ksplit == 1 and not plan.rows_pass and not plan.build_planes, plan
        got = G.pair_value(*G.decode_planes(yp, R, G.N_OUT))
        assert bool(torch.isfinite(got).all())
        err = float((got - ops.ref).abs().max())
        print("ffn2 mx C %d R %d rm %d %s mt %d: max-abs %.3e" % (key + (mt, err)))
        worst = max(worst, err)
        assert err < BAR["ffn2_mx"], "mt %d: max-abs %g" % (mt, err)
        assert G.untouched(yp, n) and int(yp[:n].reshape(R, -1)[gap].max()) == 0
        planes[mt] = yp[:n]
    assert torch.equal(planes[4], planes[5]), "the two heights differ"
    plan, yp = dev.run_split_bf16(fs2_option)
    assert (plan.kernel, plan.epi, plan.arith, plan.res, plan.mt) == ("row4", 0, 0, 2, 4), plan
    sib = float((G.pair_value(*G.decode_planes(yp, R, G.N_OUT)) - ops.ref).abs().max())
    print("    the split-bf16 arithmetic on the same values: %.3e from the mx formula" % sib)
    assert sib < BAR["ffn2_mx"] + CEILING
    _record("ffn2_mx", worst, BAR["ffn2_mx"])
