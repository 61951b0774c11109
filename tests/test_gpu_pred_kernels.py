"""Kernel-level tests of the LayerNorm-terminated convolutions of the duration, pitch and energy predictors: gemm_row8c_bf16 as row8c (both tile heights, nb 2 and 3,
with and without the scalar head, with the column offset that lets energy.conv0 / pitch.conv0 fill the halves of one stacked plane buffer), as row8c_two_ln
(var.conv0: one LayerNorm per N-wave) and as row8c_grouped (var.conv1: grid.y = group), and their small-batch siblings, gemm_pl_bf16's conv form followed by ln_rows,
without and with split-K -- each launched on the library itself through fs2_op_launch_gemm (tests/gemm_raw.py) on operands whose values are known exactly, formed
as csrc/model_launches.h forms them.  The plan the library reports is asserted for every launch (the same blocks are planned on the CPU first:
tests/test_gemm_raw_host.py).

Every run is held against a float64 reference of the same operation (tests/gemm_raw.py: ref_pred) on the pair values.  The bars are shares of a ceiling derived from
GEMM_TOL["bf16x3"] and the LayerNorm's own amplification, the shares from the fp32 statement of the kernels' arithmetic on the CPU alone (gemm_raw.py:
PRED_BAR_SHARE / PRED_HEAD_SHARE); tests/test_gemm_raw_host.py holds every mutant -- taps reversed, a halo tap missing at a tile edge, the tap in front of row 0
reading a row, groups crossed, one LayerNorm over both groups, eps = 1e-5, no ReLU, ReLU per split-K partial, dot_b[0] for dot_b[g], the heads swapped -- at 8 bars or
more.  The x planes hold NaN behind row R, so a kernel that reads them fails the comparison.  The two tile heights of a row kernel must write the same bits; the
row kernel and its sibling sum the LayerNorm in another order and must agree within the sum of their bars.  The grouped launch writes no planes (as in the model):
its two heads are compared."""
import pytest
import torch

from tests import gemm_raw as G

pytestmark = pytest.mark.gpu

_cache = {}


def _results(case, fs2_option):
    """Every run of a case (gemm_raw.pred_runs), once per session: (operands, device case, {(run, mt): (plan, {yp, dot, scratch, kpart: bytes})})."""
    if case not in _cache:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        ops = G.PredOperands(*case)
        dev = G.PredCase(ops)
        runs, halves = {}, {}
        for run, mt in G.pred_runs(ops.form):
            half = run.startswith("half")
            plan, out, yp = dev.run(run, mt, fs2_option, yp=halves.get(mt) if half else None)
            if half:
                halves[mt] = yp                  # (the second half launch of a height goes into the buffer of the first)
            want = G.pred_expected(*case, run, mt)
            assert {k: getattr(plan, k) for k in want} == want and not plan.build_planes, (case, run, mt, plan)
            assert (plan.ksplit > 1) == (run == "sibk") and bool(plan.rows_pass) == (run in ("sib", "sibk")), (case, run, mt, plan)
            runs[(run, mt)] = (plan, out)
        _cache[case] = (ops, dev, runs)
    return _cache[case]


def _planes(ops, out):
    return G.pair_value(*G.decode_planes(out["yp"], ops.R, ops.Nrow))


def _heads(ops, dev, out):
    """[R, G] of the groups' head arrays."""
    return dev.heads(out["dot"])[:ops.lg, :ops.R].t().double()


def _whole_runs(runs):
    return [(key, v) for key, v in runs.items() if not key[0].startswith("half")]


TWO_LN = [(c, i) for c, i in zip(G.PRED_CASES, G.PRED_IDS) if c[0] == "two_ln"]


@pytest.mark.parametrize("case", G.PRED_CASES, ids=G.PRED_IDS)
def test_pred_launches_against_float64(case, fs2_option):
    """The row kernel at both heights and the sibling without and with split-K against float64: the planes, or both heads where the form writes heads; every
    row < R finite, i.e. written (and no NaN row of x read).  dead_window: the rows whose whole window is zero hold exactly beta as the planes round it / the head
    of beta within the head bar at rstd-free ceiling (their pre-LayerNorm values are exactly zero: only the fp32 order of Sum beta dot_w is left)."""
    from tests.conftest import record_measurement
    ops, dev, runs = _results(case, fs2_option)
    bar_v, bar_h = ops.bars()
    worst, bad = 0.0, []
    for (run, mt), (_, out) in _whole_runs(runs):
        if ops.has_head:
            got, ref, ceil, bar = _heads(ops, dev, out), ops.ref.head, ops.head_ceiling, bar_h
        else:
            got, ref, ceil, bar = _planes(ops, out), ops.ref.v, ops.ceiling, bar_v
        assert bool(torch.isfinite(got).all()), "%s mt %d: non-finite / unwritten output in rows < R" % (run, mt)
        err = (got - ref).abs()
        ratio = float((err / ceil).max())
        print("%s %s mt %d: max-abs %.3e, worst error / ceiling %.4g (share %.4g)" % (G.PRED_IDS[G.PRED_CASES.index(case)], run, mt, float(err.max()), ratio,
                                                                                    G.PRED_HEAD_SHARE if ops.has_head else G.PRED_BAR_SHARE))
        worst = max(worst, ratio)
        if bool((err >= bar).any()):
            bad.append("%s mt %d: max-abs %g, error / ceiling %g, %d elements beyond the bar" % (run, mt, float(err.max()), ratio, int((err >= bar).sum())))
        if ops.dead and ops.has_head:
            want = float(ops.beta.double() @ ops.dot_w.double() + ops.dot_b.double()[0])
            slack = G.PRED_HEAD_SHARE * (G.PRED_TOL * float(ops.dot_w.double().abs().sum()) + G.PRED_TOL)
            assert float((got[ops.dead, 0] - want).abs().max()) <= slack, "%s mt %d: the head of a dead row is %s, beta . dot_w + dot_b = %g" % (run, mt, got[ops.dead, 0].tolist(), want)
        elif ops.dead:
            assert torch.equal(got[ops.dead], G.pair_value(*G.split_bf16(ops.beta)).unsqueeze(0).expand(len(ops.dead), -1)), "%s mt %d: a dead row is not beta" % (run, mt)
    record_measurement("pred_kernel_%s_%s_ratio" % (ops.form, "head" if ops.has_head else "planes"), worst)
    assert not bad, bad


@pytest.mark.parametrize("case", G.PRED_CASES, ids=G.PRED_IDS)
def test_pred_heights_write_the_same_bits_and_siblings_agree(case, fs2_option):
    """Results do not depend on MT: row8c / row8c_grouped at 128 and 192 rows write the same plane bytes and the same dot_out bits.  The row kernel and the sibling
    (without and with split-K) are not promised equal bits -- the LayerNorm sums run in another order: they agree within the sum of their two bars."""
    ops, dev, runs = _results(case, fs2_option)
    bar_v, bar_h = ops.bars()
    if ops.form != "two_ln":
        a, b = runs[("row", 2)][1], runs[("row", 3)][1]
        for name in ("yp", "dot"):
            diff = int((a[name] != b[name]).sum())
            assert diff == 0, "%d bytes of %s differ between 128-row and 192-row tiles" % (diff, name)
    value = (lambda out: _heads(ops, dev, out)) if ops.has_head else (lambda out: _planes(ops, out))
    row = value(runs[("row", 2)][1])
    for run in ("sib", "sibk"):
        d = (value(runs[(run, 0)][1]) - row).abs()
        assert bool((d <= 2 * (bar_h if ops.has_head else bar_v)).all()), "%s and the row kernel differ by %g" % (run, float(d.max()))


@pytest.mark.parametrize("case", [c for c, _ in TWO_LN], ids=[i for _, i in TWO_LN])
def test_pred_halves_fill_one_stacked_buffer(case, fs2_option):
    """energy.conv0 / pitch.conv0: two N = 256 launches into the halves of 512-column plane rows (yp_col_off).  After one half alone every byte of the other half's
    columns still holds the sentinel, in every row; together they hold the reference of the stacked launch, within the bars, and agree with row8c_two_ln within
    the sum of the bars (another LayerNorm order); the pair at 128-row tiles and the pair at 192-row tiles, sent in the other order, write the same bytes."""
    from tests.conftest import record_measurement
    ops, dev, runs = _results(case, fs2_option)
    R, Rp = ops.R, G.rpad(ops.R)
    rows = lambda out: out["yp"][:dev.yp_bytes].reshape(Rp, 2048)            # 16 chunks of 128 bytes; the columns 256 .. 511 are the bytes 1024 .. 2047 of a row
    first0, both2, first1, both3 = (runs[k][1] for k in (("half0", 2), ("half1", 2), ("half1", 3), ("half0", 3)))
    assert bool((rows(first0)[:, 1024:] == 0xFF).all()), "half0 wrote into the columns of half1"
    assert bool((rows(first1)[:, :1024] == 0xFF).all()), "half1 wrote into the columns of half0"
    assert torch.equal(rows(first0)[:, :1024], rows(both2)[:, :1024]) and torch.equal(rows(first1)[:, 1024:], rows(both3)[:, 1024:])      # (the second launch left the first half alone)
    assert torch.equal(both2["yp"], both3["yp"]), "the halves at 128-row and at 192-row tiles differ"
    bar_v, _ = ops.bars()
    got = _planes(ops, both2)
    assert bool(torch.isfinite(got).all())
    err = (got - ops.ref.v).abs()
    ratio = float((err / ops.ceiling).max())
    print("%s halves: max-abs %.3e, worst error / ceiling %.4g" % (case, float(err.max()), ratio))
    record_measurement("pred_kernel_halves_planes_ratio", ratio)
    assert bool((err < bar_v).all()), (float(err.max()), ratio)
    assert bool(((got - _planes(ops, runs[("row", 2)][1])).abs() <= 2 * bar_v).all())
    for out in (first0, both2, first1, both3):
        assert G.untouched(out["yp"], R * 2048) and G.untouched(out["scratch"], 0) and G.untouched(out["dot"], 0) and G.untouched(out["kpart"], 0)
    gap = ops.pos[:R] < 0
    assert int(rows(both2)[:R][gap].max()) == 0, "a gap row is not zero"


@pytest.mark.parametrize("case", G.PRED_CASES, ids=G.PRED_IDS)
def test_pred_launches_write_nothing_else(case, fs2_option):
    """Planes of rows >= R and the guard stay untouched; dot_out[r >= R] of both group arrays, the gap between them and the array of a group the launch does not
    have; gap rows are zero bytes in the planes and +0.0 in dot_out; a row kernel never touches the scratch rows or the split-K scratch (nothing but its planes /
    dot_out leaves), the sibling writes scratch rows < R only and, split, the partial slabs it was given the count of."""
    ops, dev, runs = _results(case, fs2_option)
    R, N = ops.R, ops.N
    gap = ops.pos[:R] < 0
    for (run, mt), (plan, out) in _whole_runs(runs):
        who = "%s mt %d" % (run, mt)
        if ops.has_head:
            assert G.untouched(out["yp"], 0), who + ": planes were never handed over"
            bits = out["dot"][:dev.dot_bytes].view(torch.int32).reshape(2, dev.gstride)
            for g in range(2):
                assert bool((bits[g, (R if g < ops.lg else 0):] == -1).all()), "%s wrote dot_out behind row R of group %d" % (who, g)
            assert G.untouched(out["dot"], dev.dot_bytes)
            assert not bool(bits[:ops.lg, :R][:, gap].any()), who + ": dot_out of a gap row is not +0.0"
        else:
            assert G.untouched(out["dot"], 0), who + ": dot_out was never handed over"
            assert G.untouched(out["yp"], R * ops.Nrow * 4), who + " wrote planes of a row >= R"
            assert int(out["yp"][:R * ops.Nrow * 4].reshape(R, -1)[gap].max()) == 0, who + ": a gap row is not zero"
        if run == "row":
            assert G.untouched(out["scratch"], 0) and G.untouched(out["kpart"], 0), who + " touched a scratch buffer"
        else:
            assert G.untouched(out["scratch"], R * N * 4), who + " wrote scratch rows >= R"
            slabs = (plan.ksplit - 1) * R * N * 4
            assert G.untouched(out["kpart"], slabs), who + " wrote behind its partial slabs"
            assert run != "sibk" or not bool((out["kpart"][:slabs].view(torch.int32) == -1).any()), who + ": a partial sum was not written"
