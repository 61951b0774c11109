"""Kernel-level tests of the row-complete GEMMs the benchmark's default configuration runs and fs2_op_conv_gemm cannot reach: gemm_row4_bf16 in its
four planes-only LayerNorm forms, the QKV passes on it (EPI 3), gemm_qkv8_bf16, the positional-encoding epilogue of the row kernels, planes output in both
formats -- each launched on the audited library itself through fs2_op_launch_gemm (tests/gemm_raw.py), on operands whose exact values are known.

Every launch is held against a float64 reference of the same operation, and every form against its siblings bit for bit: gemm_row8_bf16 at both tile
heights (fp32 rows in and out, the residual reconstructed from the planes, which is exact in fp32) and gemm_row4_bf16 at both of its heights must write
the same planes; gemm_qkv8_bf16 (two heights, passes together and apart) and the passes on gemm_row4_bf16 the same Q | K and V^T planes.  The plan the
library reports is asserted for every launch, so no case can quietly run another kernel (the same blocks are planned on the CPU first:
tests/test_gemm_raw_host.py).

Tolerances: bit-identity is exact (QKV: +0 == -0 per 16-bit half, rows that are padding leave as v x 0).  Split-bf16 outputs against float64: the
project's GEMM_TOL["bf16x3"] (5 x the worst error measured on these distributions, forced gemm_row8_bf16 at N = 384 included; the rounding of a hi + lo
plane adds at most 2^-17 |y| ~ 4e-5 at |y| <= 5).  mx planes out keep fp16 + an e4m3 rounding of the fp16 residual, at most 2^-4 of half an fp16 ulp
<= 2^-14 |ref|: the bar per element is GEMM_TOL["bf16x3"] + 2^-14 |ref|."""
import pytest
import torch

from tests import gemm_raw as G
from tests.test_gpu_ops import GEMM_TOL

pytestmark = pytest.mark.gpu

TOL = GEMM_TOL["bf16x3"]
_cache = {}


def _ln_results(case, fs2_option):
    """All four runs of a LayerNorm-fused case, once per session: {(side, mt): (plan, planes bytes, fp32 row bytes)}."""
    if case not in _cache:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        form, R, Cc = case
        ops = G.LnOperands(form, R, Cc)
        dev = G.LnCase(ops)
        runs = {}
        for side, mt in G.LN_RUNS:
            plan, yp, y = dev.run(side, mt, fs2_option)
            assert (plan.kernel, plan.epi, plan.res, plan.mt) == G.ln_expected(form, side, mt), (case, side, mt, plan)
            assert plan.nsplit == 3 and plan.ksplit == 1 and not plan.rows_pass and not plan.build_planes, plan
            runs[(side, mt)] = (plan, yp, y)
        _cache[case] = (ops, runs)
    return _cache[case]


def _qkv_results(D, fs2_option):
    if ("qkv", D) not in _cache:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        ops = G.QkvOperands(D)
        dev = G.QkvCase(ops)
        runs = {}
        for kind, mt, split in G.QKV_RUNS[D]:
            plan, out = dev.run(kind, mt, split, fs2_option)
            assert (plan.kernel, plan.epi, plan.res, plan.mt, plan.apart, plan.bm) == G.qkv_expected(kind, mt, split), (D, kind, mt, split, plan)
            assert plan.nsplit == 3 and plan.ksplit == 1 and not plan.rows_pass and not plan.build_planes, plan
            runs[(kind, mt, split)] = out
        _cache[("qkv", D)] = (ops, dev, runs)
    return _cache[("qkv", D)]


LN_IDS = ["%s-R%d-C%d" % c for c in G.LN_CASES]


@pytest.mark.parametrize("case", G.LN_CASES, ids=LN_IDS)
def test_layernorm_forms_against_float64(case, fs2_option):
    """Every run of the case -- gemm_row8_bf16 at 128 / 192 rows, gemm_row4_bf16 (planes only) at 128 / 160 -- against float64 on the exact operand values."""
    from tests.conftest import record_measurement
    ops, runs = _ln_results(case, fs2_option)
    bar = TOL + (2.0 ** -14 * ops.ref.abs() if ops.epi == 1 else 0.0)
    worst, bad = 0.0, []
    for (side, mt), (_, yp, _) in runs.items():
        got, _ = ops.decode(yp)
        assert bool(torch.isfinite(got).all()), "%s mt %d: non-finite / unwritten planes in rows < R" % (side, mt)
        err = (got - ops.ref).abs()
        print("%s %s mt %d: max-abs %.3e (max |ref| %.2f)" % (ops.form, side, mt, float(err.max()), float(ops.ref.abs().max())))
        worst = max(worst, float(err.max()))
        if bool((err >= bar).any()):
            bad.append("%s mt %d: max-abs %g, %d elements beyond the bar" % (side, mt, float(err.max()), int((err >= bar).sum())))
    record_measurement("row_kernel_%s_maxabs" % ops.form, worst)
    assert not bad, bad


@pytest.mark.parametrize("case", G.LN_CASES, ids=LN_IDS)
def test_layernorm_forms_write_the_same_planes_bit_for_bit(case, fs2_option):
    """The output planes of all four runs are the same bytes over rows < R; nobody writes a row >= R or behind the buffer; gap rows are zero bytes."""
    ops, runs = _ln_results(case, fs2_option)
    n = ops.R * G.N_OUT * 4
    ref = runs[("row8", 2)][1]
    gap = (ops.pos[:ops.R] < 0)
    for key, (_, yp, y) in runs.items():
        diff = int((yp[:n] != ref[:n]).sum())
        assert diff == 0, "%s mt %d: %d bytes of the planes differ from gemm_row8_bf16 at 128 rows" % (key + (diff,))
        assert G.untouched(yp, n), "%s mt %d wrote planes of a row >= R" % key
        assert int(yp[:n].reshape(ops.R, -1)[gap].max()) == 0, "%s mt %d: a gap row is not zero" % key
        if key[0] == "row4":
            assert G.untouched(y, 0)          # (Y is null there: the buffer was never handed over)
        else:
            assert G.untouched(y, n), "%s mt %d wrote fp32 rows >= R" % key


@pytest.mark.parametrize("case", G.LN_CASES, ids=LN_IDS)
def test_layernorm_forms_fp32_rows_agree_with_the_planes(case, fs2_option):
    """gemm_row8_bf16 writes the same result twice: its fp32 rows equal what its planes hold to within the planes' rounding (split-bf16: 2^-16 |y|; mx: fp16
    + e4m3 residual, 2^-14 |y| + the e4m3 underflow 2^-24), gap rows exactly zero in both; the third block of mx planes is e4m3(fp16 2^ka)."""
    ops, runs = _ln_results(case, fs2_option)
    n = ops.R * G.N_OUT * 4
    gap = (ops.pos[:ops.R] < 0)
    for mt in (2, 3):
        _, yp, y = runs[("row8", mt)]
        rows = y[:n].view(torch.float32).reshape(ops.R, G.N_OUT).double()
        got, blocks = ops.decode(yp)
        assert bool(torch.isfinite(rows).all())
        slack = (2.0 ** -14 * rows.abs() + 2.0 ** -24) if ops.epi == 1 else 2.0 ** -16 * rows.abs()
        assert bool(((rows - got).abs() <= slack).all()), "mt %d: rows and planes differ by %g" % (mt, float((rows - got).abs().max()))
        assert float(rows[gap].abs().max()) == 0.0 and float(got[gap].abs().max()) == 0.0
        assert float((rows - ops.ref).abs().max()) < TOL
    if ops.epi == 1:
        for key, (_, yp, _) in runs.items():
            h, e8, a8 = ops.decode(yp)[1]
            assert not bool(((e8 & 0x7F) == 0x7F).any()) and not bool(((a8 & 0x7F) == 0x7F).any())
            assert torch.equal(a8, G.e4m3_of(h.float() * 2.0 ** G.KA_OUT)), "%s mt %d: the ah8 block is not e4m3(fp16 x 8)" % key


@pytest.mark.parametrize("D", [384, 256])
def test_qkv_forms_against_float64(D, fs2_option):
    """Q x q_scale, K and V (each hi + lo) of every form -- gemm_qkv8_bf16 at both heights, passes together and apart, the passes on gemm_row4_bf16 at both
    of its heights (D = 384), gemm_pl_bf16's fused-QKV epilogue -- against float64; rows that are gaps or padding are zeros in all four planes."""
    from tests.conftest import record_measurement
    ops, dev, runs = _qkv_results(D, fs2_option)
    R = ops.R
    live = ops.pos >= 0
    bad = []
    worst = {"row": 0.0, "pl": 0.0}
    for key, out in runs.items():
        for name, nbytes in (("qk_hi", dev.qk_bytes), ("qk_lo", dev.qk_bytes), ("vt_hi", dev.vt_bytes), ("vt_lo", dev.vt_bytes)):
            assert G.untouched(out[name], nbytes), "%s wrote behind %s" % (key, name)
        q, k, v = dev.decode(out)
        assert bool(torch.isfinite(q).all() and torch.isfinite(k).all() and torch.isfinite(v).all()), "%s: unwritten rows below Rvt" % (key,)
        assert float(max(t[~live].abs().max() for t in (q, k, v))) == 0.0, "%s: a gap / padding row is not zero" % (key,)
        err = max(float((g[:R] - r).abs().max()) for g, r in zip((q, k, v), ops.ref))
        print("qkv D %d %s: max-abs %.3e" % (D, key, err))
        worst["pl" if key[0] == "pl" else "row"] = max(worst["pl" if key[0] == "pl" else "row"], err)
        if err >= TOL:
            bad.append("%s: max-abs %g" % (key, err))
    record_measurement("row_kernel_qkv%d_maxabs" % D, worst["row"])
    record_measurement("row_kernel_qkv%d_pl_maxabs" % D, worst["pl"])
    assert not bad, bad


@pytest.mark.parametrize("D", [384, 256])
def test_qkv_forms_write_the_same_planes_bit_for_bit(D, fs2_option):
    """All 8-wave and one-wave forms agree in Q | K hi, Q | K lo, V^T hi and V^T lo over all Rvt rows (+0 == -0 per 16-bit half)."""
    _, dev, runs = _qkv_results(D, fs2_option)
    ref = runs[("qkv8", 2, 1)]
    for key, out in runs.items():
        if key[0] == "pl":
            continue          # (another accumulation order: held against float64 only)
        for name, nbytes in (("qk_hi", dev.qk_bytes), ("qk_lo", dev.qk_bytes), ("vt_hi", dev.vt_bytes), ("vt_lo", dev.vt_bytes)):
            diff = int((G.canon_zero16(out[name][:nbytes]) != G.canon_zero16(ref[name][:nbytes])).sum())
            assert diff == 0, "%s: %d words of %s differ from gemm_qkv8_bf16 (128 rows, passes apart)" % (key, diff, name)
