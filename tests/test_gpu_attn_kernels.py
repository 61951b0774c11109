"""Kernel-level tests of the self-attention launches: attn_f32, attn_bf16 with three terms and with one, attn_w32 and qkv_split, each launched on the library itself
through fs2_op_launch_attention (tests/attn_raw.py) on operand planes whose values are known exactly, laid out as the kernels read them, with NaN in every K / V^T
element that is no live key and in every Q row that is no query.  The plan the library reports is asserted for every launch, on every field.

Every run is held against a float64 reference of the same operation on the pair values (attn_f32: on its fp32 rows).  The bars come from the fp32 statement of the
kernels' arithmetic on the CPU, capped by the ceilings of tests/test_gpu_ops.py (attn_raw.BAR); tests/test_attn_raw_host.py holds every mutant -- q_lo . k_hi dropped,
P's lo part dropped, the natural base, a tile's keys permuted against V^T, the other head's V, the last key left out -- at 8 bars or more.  One batch of ten utterances
(1 to 9 key tiles, every query edge, an empty utterance) runs with klen = len and with every klen < len, under mask_q 0 and 1, in every output form (fp32 rows, planes
only -- the model's --, both) and with the work list in its three forms: plain, dealt and padded as the model's, and counted (a capacity-sized grid, the count read on
the device, the items behind it naming a ghost utterance whose rows must stay untouched).

The rows a launch may write are exactly the rows [start, start + len) of the utterances its valid items name (attn_raw.AttnOperands.written_rows: every store of the
four kernels is guarded by its own row index against len); everything else -- the gaps, the ghost, the rows behind the batch, the guard -- must still hold the sentinel.

attn_w32's slow path is driven by three spike cases whose count of leaving waves the float64 reference predicts unambiguously (host test); the count, and every row
of the leaving wave's siblings, is asserted."""
import numpy as np
import pytest
import torch

from tests import attn_raw as A
from tests import gemm_raw as G

pytestmark = pytest.mark.gpu

OUTS = {"f32": ("rows",), "x3": ("rows", "planes", "both"), "x1": ("rows", "planes", "both"), "w32": ("rows", "planes", "both")}
WORKS = ("plain", "dealt", "counted")
CASES = [(D, h, v, mq) for D, h in A.HEADS for v, mq in A.BATCHES]
IDS = ["D%d-h%d-%s-mq%d" % c for c in CASES]

_cases, _cache = {}, {}


def _case(key):
    if key not in _cases:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        _cases[key] = A.AttnCase(A.operands(*key))
    return _cases[key]


def _ariths(D, heads):
    return [a for a in A.ARITHS if a != "w32" or (D, heads) in A.W32_HEADS]


def _results(case, fs2_option):
    """Every launch of a case, once per session: {(arithmetic, output form, work-list form): (ctx bytes, ctxp bytes, slow_count)}; the plan of each is asserted here."""
    if case not in _cache:
        D, heads, variant, mq = case
        dev = _case((D, heads, variant, None))
        runs = {}
        for arith in _ariths(D, heads):
            for out in OUTS[arith]:
                for work in WORKS:
                    plan, ctx, ctxp, slow = dev.run(arith, out, work, mq, fs2_option)
                    assert plan == A.expected_plan(arith, D // heads, heads, len(dev.work[work][0])), (case, arith, out, work, plan)
                    runs[(arith, out, work)] = (ctx, ctxp, slow)
        if (D, heads) not in A.W32_HEADS:      # no attn_w32 at head dims 64 and 256: forced on, the plan is attn_bf16's and so are the bits
            for out in OUTS["x3"]:
                plan, ctx, ctxp, slow = dev.run("x3", out, "dealt", mq, fs2_option, w32_option=1)
                assert plan == A.expected_plan("x3", D // heads, heads, len(dev.work["dealt"][0])), (case, out, plan)
                runs[("x3/forced", out, "dealt")] = (ctx, ctxp, slow)
        _cache[case] = (dev, runs)
    return _cache[case]


def _values(dev, arith, out, ctx, ctxp):
    """-> [(form, float64 [Rvt, D], bar function)] of a run's outputs."""
    got = []
    if ctx is not None:
        got.append(("rows", dev.rows(ctx).double(), lambda ref: torch.full_like(ref, A.BAR[arith])))
    if ctxp is not None:
        got.append(("planes", dev.plane_values(ctxp), lambda ref: A.planes_bar(arith, ref)))
    return got


def _check_against(ops, dev, arith, out, ctx, ctxp, ref, mask_q, who):
    """Every live row finite (written, and no NaN key or query read), within the bar; dead query rows exactly zero.  -> worst error / bar."""
    live, worst = ops.written_rows(), 0.0
    for form, v, bar in _values(dev, arith, out, ctx, ctxp):
        assert bool(torch.isfinite(v[live]).all()), "%s %s: a dead key reached the output, or a live query row was never written" % (who, form)
        err, b = (v[live] - ref[live]).abs(), bar(ref[live])
        ratio = float((err / b).max())
        print("%s %s: max-abs %.3e, worst error / bar %.3f" % (who, form, float(err.max()), ratio))
        worst = max(worst, ratio)
        assert bool((err < b).all()), "%s %s: max-abs %g, %d elements beyond the bar (worst %.3g bars)" % (who, form, float(err.max()), int((err >= b).sum()), ratio)
        if mask_q:
            for s, n, kn in ops.utterances():
                if kn < n:
                    assert float(v[s + kn:s + n].abs().max()) == 0.0, "%s %s: dead query rows of the utterance at row %d are not exactly zero" % (who, form, s)
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_launches_against_float64(case, fs2_option):
    from tests.conftest import record_measurement
    D, heads, variant, mq = case
    dev, runs = _results(case, fs2_option)
    ops = dev.ops
    refs = {a: A.reference(ops, a, mq) for a in ("f32", "x3")}
    worst = {}
    for (arith, out, work), (ctx, ctxp, slow) in runs.items():
        base = arith.split("/")[0]
        r = _check_against(ops, dev, base, out, ctx, ctxp, refs["f32" if base == "f32" else "x3"], mq, "%s %s %s %s" % (IDS[CASES.index(case)], arith, out, work))
        worst[base] = max(worst.get(base, 0.0), r)
        assert slow == 0, "%s %s %s: %d waves counted on the slow path of a batch that sends none there" % (arith, out, work, slow)
    for a, r in worst.items():
        record_measurement("attn_kernel_%s_dk%d_error_to_bar" % (a, D // heads), r)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_output_forms_agree_bit_for_bit(case, fs2_option):
    """Written together, the planes are the split of the rows; the rows alone and the planes alone (attn_w32: the LDS-staged whole-row epilogue) hold the same bits as
    the pair written together."""
    D, heads, _, _ = case
    dev, runs = _results(case, fs2_option)
    live = dev.ops.written_rows()
    for arith in _ariths(D, heads):
        if arith == "f32":
            continue
        for work in WORKS:
            rows, planes, (both_r, both_p, _) = runs[(arith, "rows", work)][0], runs[(arith, "planes", work)][1], runs[(arith, "both", work)]
            hi, lo = G.decode_planes(both_p, dev.ops.Rvt, D)
            want_hi, want_lo = G.split_bf16(dev.rows(both_r)[live])
            assert torch.equal(hi[live].view(torch.int16), want_hi.view(torch.int16)) and torch.equal(lo[live].view(torch.int16), want_lo.view(torch.int16)), \
                "%s %s: the planes are not the split of the rows written with them" % (arith, work)
            assert torch.equal(rows, both_r), "%s %s: the rows alone differ from the rows written with planes" % (arith, work)
            assert torch.equal(planes, both_p), "%s %s: the planes alone differ from the planes written with rows" % (arith, work)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_work_list_forms_give_the_same_bits(case, fs2_option):
    """plain, dealt (longest key range first into interleaved queues, padded with (-1, 0)) and counted (capacity-sized grid, *nwork on the device) write the same bytes
    in every row of every utterance -- and everywhere else: the whole buffers are compared, guard included.  Head dims 64 and 256: FS2_ATTN_W32 = 1 changes nothing."""
    D, heads, _, _ = case
    dev, runs = _results(case, fs2_option)
    for arith in _ariths(D, heads):
        for out in OUTS[arith]:
            ref = runs[(arith, out, "plain")]
            for work in WORKS[1:]:
                got = runs[(arith, out, work)]
                for name, a, b in (("ctx", ref[0], got[0]), ("ctxp", ref[1], got[1])):
                    assert (a is None and b is None) or torch.equal(a, b), "%s %s: %s of the %s list differs from the plain list's in %d bytes" % (arith, out, name, work, int((a != b).sum()))
    for (arith, out, work), got in runs.items():
        if arith == "x3/forced":
            ref = runs[("x3", out, work)]
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ref[:2], got[:2])), "FS2_ATTN_W32 = 1 changed the bits at head dim %d" % (D // heads)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_launches_write_nothing_else(case, fs2_option):
    """Outside the rows [start, start + len) of the real utterances every byte of both output buffers still holds the sentinel: the gaps (behind len: nothing of a
    16-query tile or of attn_w32's staged 32-row epilogue), the ghost's rows (counted: the items behind the count), every row >= rows used, the guard.  A buffer the
    launch was not given cannot be checked here; the one it was given and the form does not fill does not exist."""
    dev, runs = _results(case, fs2_option)
    for (arith, out, work), (ctx, ctxp, _) in runs.items():
        for name, buf in (("ctx", ctx), ("ctxp", ctxp)):
            assert buf is None or dev.untouched_outside(buf), "%s %s %s wrote %s outside its utterances" % (arith, out, work, name)
    ops = dev.ops
    gs, gn = ops.starts[-1], ops.lens[-1]
    assert gn > 0 and not bool(ops.written_rows()[gs:gs + gn].any())      # (the ghost's rows are among those held above)


@pytest.mark.parametrize("spike", A.SPIKES)
@pytest.mark.parametrize("D,heads", A.W32_HEADS)
def test_attn_w32_slow_path_counts_the_predicted_waves(D, heads, spike, fs2_option):
    """One utterance of 160 queries, key 97 (`first`: key 17) aligned with four queries of the wave of queries 64 .. 95.  below: P reaches ~2^45 on the fast path and no
    wave leaves; exit: exactly that wave leaves, in every head -- slow_count = heads --, its siblings keep computing while it only feeds the DMA ring, and all 160 rows
    pass; first: the spike is the reference maximum and no wave leaves.  The 64-query kernels take the rescale branch on the same operands and stay within their bars."""
    from tests.conftest import record_measurement
    dev = _case((D, heads, "full", spike))
    ops = dev.ops
    want = A.w32_exits(ops)[0]
    assert want == (heads if spike == "exit" else 0)
    refs = {a: A.reference(ops, a, 0) for a in ("f32", "x3")}
    for arith, outs in (("w32", ("rows", "planes")), ("x3", ("rows",)), ("f32", ("rows",))):
        for out in outs:
            plan, ctx, ctxp, slow = dev.run(arith, out, "dealt", 0, fs2_option)
            assert plan == A.expected_plan(arith, D // heads, heads, len(dev.work["dealt"][0])), (arith, out, plan)
            assert slow == (want if arith == "w32" else 0), "%s %s: %d waves left the fast path, the reference predicts %d" % (arith, out, slow, want)
            r = _check_against(ops, dev, arith, out, ctx, ctxp, refs["f32" if arith == "f32" else "x3"], 0, "spike %s dk %d %s %s" % (spike, D // heads, arith, out))
            record_measurement("attn_kernel_%s_dk%d_spike_%s_error_to_bar" % (arith, D // heads, spike), r)
            for buf in (ctx, ctxp):
                assert buf is None or dev.untouched_outside(buf)


@pytest.mark.parametrize("D,heads", A.W32_HEADS)
def test_attn_w32_falls_back_when_the_lo_planes_sit_in_front(D, heads, fs2_option):
    """attn_w32 reaches the lo planes with 32-bit offsets from the hi planes: 0 .. 2 GB behind them.  With the lo planes allocated in front, the plan is attn_bf16 with
    three terms although FS2_ATTN_W32 = 1, and the bits are those of the 64-query kernel on the usual arrangement."""
    dev, runs = _results((D, heads, "short", 1), fs2_option)
    n = len(dev.work["dealt"][0])
    for out in ("rows", "planes"):
        plan, ctx, ctxp, slow = dev.run("w32", out, "dealt", 1, fs2_option, lo_first=True)
        assert plan == A.expected_plan("w32", D // heads, heads, n, kernel="b16") and plan.nsplit == 3, plan
        ref = runs[("x3", out, "dealt")]
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ref[:2], (ctx, ctxp))) and slow == 0
    # (and behind them, as everywhere else in this file, FS2_ATTN_W32 = 1 does plan attn_w32)
    assert dev.run("w32", "rows", "dealt", 1, fs2_option)[0].kernel == "w32"


def _written(lay):
    m = torch.zeros(lay.Rvt, dtype=torch.bool)
    for s, n, _ in lay.utts:
        m[s:s + n] = True
    return m


def test_qkv_split_through_the_hook(fs2_option):
    """fp32 QKV rows in (R = 333, D = 384): the split pass writes the four planes -- fl32(q scale), K and V split into hi + lo bit for bit, V^T zero from R to Rvt, Q | K
    rows >= R not written, nothing behind the planes -- and the attention that follows reads them."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    D, heads, R, Rvt = 384, 2, 333, 384
    lay = A.Layout(D, heads, R, Rvt, [(8, 100, 100), (120, 97, 90), (232, 101, 101)])
    rs = np.random.RandomState(333)
    qkv = torch.zeros(Rvt, 3 * D)
    qkv[:R] = G._uni(rs, R, 3 * D, scale=2.0)
    qkv[R:] = float("nan")                              # rows >= R are not the call's data
    qk_bytes, vt_bytes = Rvt * 2 * D * 2, D * Rvt * 2
    out = dict(qk_hi=G.sentinel(qk_bytes), qk_lo=G.sentinel(qk_bytes), vt_hi=G.sentinel(vt_bytes), vt_lo=G.sentinel(vt_bytes))
    qd = qkv.to(G._dev())
    plan, n, ctx, _ = A.launch_on(lay, {k: t.data_ptr() for k, t in out.items()}, "x3", fs2_option, qkv=qd.data_ptr())
    assert plan == A.expected_plan("x3", D // heads, heads, n, split_pass=True), plan
    got = {k: t.cpu() for k, t in out.items()}
    for k, nb in (("qk_hi", qk_bytes), ("qk_lo", qk_bytes), ("vt_hi", vt_bytes), ("vt_lo", vt_bytes)):
        assert G.untouched(got[k], nb), "the split wrote behind %s" % k
    q = qkv[:R, :D] * torch.tensor(A.softmax_scale(D // heads))
    qk = [torch.cat([a, b], 1) for a, b in zip(G.split_bf16(q), G.split_bf16(qkv[:R, D:2 * D]))]
    vt = [t.t().contiguous() for t in G.split_bf16(qkv[:R, 2 * D:])]
    for i, part in enumerate(("hi", "lo")):
        w = got["qk_" + part][:qk_bytes].view(torch.int16).reshape(Rvt, 2 * D)
        assert torch.equal(w[:R], qk[i].contiguous().view(torch.int16)), "Q | K %s planes differ from the CPU split" % part
        assert bool((w[R:] == -1).all()), "Q | K %s rows >= R were written" % part
        w = got["vt_" + part][:vt_bytes].reshape(D, Rvt * 2)
        assert torch.equal(w[:, :2 * R].contiguous().view(torch.int16), vt[i].view(torch.int16)), "V^T %s plane differs from the CPU split" % part
        assert not bool(G.canon_zero16(w[:, 2 * R:]).any()), "V^T %s is not zero from R to Rvt" % part
    # the attention behind the split, on the pairs it left
    Q, K = G.pair_value(qk[0], qk[1])[:, :D], G.pair_value(qk[0], qk[1])[:, D:]
    V = G.pair_value(vt[0], vt[1]).t()
    pad = lambda t: torch.cat([t, torch.zeros(Rvt - R, D, dtype=torch.float64)])
    ref = A.ref64(pad(Q), pad(K), pad(V), lay, 0)
    live = _written(lay)
    v = ctx[:Rvt * D * 4].view(torch.float32).reshape(Rvt, D).double()
    assert bool(torch.isfinite(v[live]).all()) and float((v[live] - ref[live]).abs().max()) < A.BAR["x3"]
    assert bool((ctx[:Rvt * D * 4].reshape(Rvt, D * 4)[~live] == 0xFF).all()) and G.untouched(ctx, Rvt * D * 4)


def test_attention_reads_the_planes_a_fused_qkv_projection_left(fs2_option):
    """The model's hand-off: one gemm_row4_bf16 EPI 3 launch (qkv4, 128-row tiles, D = 384) writes Q | K and V^T planes into one device buffer, and the attention hook
    reads those same buffers -- attn_w32 writing planes only, as the decoder runs it, and the 64-query kernel -- against float64 of the planes as decoded."""
    from tests.conftest import record_measurement
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    D, heads = 384, 2
    qc = G.QkvCase(G.QkvOperands(D))
    R, Rvt = qc.ops.R, qc.Rvt
    sizes = [("qk_hi", qc.qk_bytes), ("qk_lo", qc.qk_bytes), ("vt_hi", qc.vt_bytes), ("vt_lo", qc.vt_bytes)]
    buf = G.sentinel(sum(nb for _, nb in sizes))
    views, off = {}, 0
    for k, nb in sizes:
        views[k] = buf[off:off + nb]
        off += nb
    plan, planes = qc.run("qkv4", 4, 0, fs2_option, out=views)
    want = G.qkv_expected("qkv4", 4, 0)
    assert (plan.kernel, plan.epi, plan.res, plan.mt, plan.apart, plan.bm) == want and G.untouched(buf, off), plan
    # utterances inside the projection's live rows (its row pattern: 4 gap rows in front of every 105), starts 8-aligned
    lay = A.Layout(D, heads, R, Rvt, [(8, 100, 100), (120, 97, 97), (224, 102, 97)])
    assert all(bool((qc.ops.pos[s:s + n] >= 0).all()) for s, n, _ in lay.utts)
    bf = lambda k, nb: planes[k][:nb].view(torch.bfloat16)
    qk = G.pair_value(bf("qk_hi", qc.qk_bytes), bf("qk_lo", qc.qk_bytes)).reshape(Rvt, 2 * D)
    vt = G.pair_value(bf("vt_hi", qc.vt_bytes), bf("vt_lo", qc.vt_bytes)).reshape(D, Rvt)
    live = _written(lay)
    ptr = {k: t.data_ptr() for k, t in views.items()}
    for mq in (0, 1):
        ref = A.ref64(qk[:, :D], qk[:, D:], vt.t(), lay, mq)
        for arith, out in (("w32", "planes"), ("x3", "rows")):
            plan, n, ctx, ctxp = A.launch_on(lay, ptr, arith, fs2_option, out=out, mask_q=mq)
            assert plan == A.expected_plan(arith, D // heads, heads, n), plan
            if out == "planes":
                v, bar, raw = G.pair_value(*G.decode_planes(ctxp, Rvt, D)), A.planes_bar(arith, ref[live]), ctxp
            else:
                v, bar, raw = ctx[:Rvt * D * 4].view(torch.float32).reshape(Rvt, D).double(), A.BAR[arith], ctx
            err = (v[live] - ref[live]).abs()
            assert bool(torch.isfinite(v[live]).all()) and bool((err < bar).all()), (arith, mq, float(err.max()))
            record_measurement("attn_kernel_%s_handoff_error_to_bar" % arith, float((err / bar).max()))
            assert bool((raw[:Rvt * D * 4].reshape(Rvt, D * 4)[~live] == 0xFF).all()) and G.untouched(raw, Rvt * D * 4)
            if mq:
                assert float(v[224 + 97:224 + 102].abs().max()) == 0.0
    assert torch.equal(buf.cpu()[:off], torch.cat([planes[k][:nb] for k, nb in sizes])), "an attention launch wrote into its operand planes"
