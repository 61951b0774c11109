"""CPU checks of tests/attn_raw.py, the helper of the kernel-level attention tests (tests/test_gpu_attn_kernels.py): all of them must pass before a launch is sent to a GPU.

(a) the ctypes mirror of fs2_op_attn_args against include/fs2.h as the host compiler lays it out (tests/attn_raw_probe.cpp), the kernel names against the enumerators of
    AttnKernel, the slow-path limit against csrc/attn_w32.h;
(b) the dealing rule stated in Python against csrc/layout_rule.h (tests/layout_probe.cpp), the plain and the counted forms, and that no item of any list the GPU tests
    send names an utterance, a block or a row outside the buffers;
(c) the operands: pairs exact, NaN exactly where no live key / no query is, the images where the kernels read them;
(d) the float64 reference: base-2 softmax on pre-scaled Q equals torch.softmax on natural scores;
(e) the fp32 statement of the kernels' arithmetic: the recorded figures behind the bars (recorded >= computed, <= 1.25 x computed), the planes' rounding within its
    allowance;
(f) DISCRIMINATION: every mutant at 8 bars or more from the reference on the cases' own operands;
(g) the spike cases: by the float64 reference every wave sits at least 2^8 from attn_w32's limit, and the count of leaving waves is the one the GPU test expects."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib
from tests import attn_raw as A
from tests import gemm_raw as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")


def _probe(tmp_path_factory, name, src):
    exe = str(tmp_path_factory.mktemp(name) / "probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", src), "-o", exe], check=True)
    return lambda *args: [l.split() for l in subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip().split("\n")]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _probe(tmp_path_factory, "attn_raw", "attn_raw_probe.cpp")


@pytest.fixture(scope="module")
def layout_probe(tmp_path_factory):
    return _probe(tmp_path_factory, "attn_layout", "layout_probe.cpp")


def test_argument_struct_mirror_matches_the_compiled_header(probe):
    lines = probe("layout")
    assert lines[0] == ["sizeof", str(ctypes.sizeof(_lib.OpAttnArgs))]
    assert lines[-1] == ["plan_fields", str(_lib.ATTN_PLAN_FIELDS)] and len(A.Plan._fields) == _lib.ATTN_PLAN_FIELDS
    fields = lines[1:-1]
    assert [l[0] for l in fields] == [f[0] for f in _lib.OpAttnArgs._fields_]
    for name, off in fields:
        assert getattr(_lib.OpAttnArgs, name).offset == int(off), name
    last = _lib.OpAttnArgs._fields_[-1][0]
    assert ctypes.sizeof(_lib.OpAttnArgs) - getattr(_lib.OpAttnArgs, last).offset - getattr(_lib.OpAttnArgs, last).size < 8
    assert _lib.OpAttnArgs().struct_size == ctypes.sizeof(_lib.OpAttnArgs)


def test_kernel_names_follow_the_enumerators_and_the_limit_is_the_kernels(probe):
    assert [(int(v), n) for v, n in probe("kernels")] == list(enumerate(A.KERNELS))
    src = open(os.path.join(CSRC, "attn_w32.h")).read()
    assert float(np.float32(float(re.search(r"kW32SumLimit = ([0-9.e+]+)f;", src).group(1)))) == A.W32_SUM_LIMIT
    assert 2.0 ** 59.9 < A.W32_SUM_LIMIT < 2.0 ** 60
    consts = open(os.path.join(CSRC, "layout_rule.h")).read()
    for name, v in (("kAttAlign", A.ATT_ALIGN), ("kAttBlk", A.ATT_BLK), ("kXcds", A.XCDS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, consts).group(1)) == v


def _probe_work(layout_probe, valid, compat, masked):
    lines = {l[0]: l[1:] for l in layout_probe("layout", 8, compat, masked, *valid)}
    return ([int(v) for v in lines["len"]], [int(v) for v in lines["klen"]], [tuple(int(x) for x in w.split(":")) for w in lines["work"]], int(lines["depth"][0]))


def test_dealing_rule_is_the_one_of_layout_rule_h(layout_probe):
    """The rule's own statement deals the lists of the GPU tests' batches (per-utterance lengths: klen = len) and, under padded-batch semantics with masking (len = the
    longest, klen = the valid count), lists in which the key ranges order the utterances and not their rows."""
    rs = np.random.RandomState(3)
    batches = [[n for n in A.LENS if n > 0], [A.SPIKE_LEN], [129, 1, 128, 127, 300, 77, 77, 77, 513], rs.randint(1, 400, size=19).tolist()]
    for valid in batches:
        for compat, masked in ((0, 0), (1, 1)):
            lens, klens, work, depth = _probe_work(layout_probe, valid, compat, masked)
            mine = A.work_dealt(lens, klens)
            assert mine == work and len(mine) == depth * A.XCDS, (valid, compat, masked)
    # an empty utterance takes no item and changes nobody's place (the probe's driver takes valid counts >= 1 only where the batch is padded, so it is held here):
    # the list of a batch with an empty utterance is the list without it, the later utterances renumbered
    with_empty, without = A.work_dealt(A.LENS, A.LENS), A.work_dealt([n for n in A.LENS if n > 0], [n for n in A.LENS if n > 0])
    ren = {b: b - sum(1 for n in A.LENS[:b] if n == 0) for b in range(len(A.LENS))}
    assert [(ren[b] if b >= 0 else -1, q) for b, q in with_empty] == without


@pytest.mark.parametrize("variant", ["full", "short"])
def test_work_list_forms_name_the_same_items_and_nothing_outside(variant):
    lens, klens, (glen, _) = A.LENS, A.KLENS[variant], A.GHOST[variant]
    B = len(lens)
    plain, dealt = A.work_plain(lens), A.work_dealt(lens, klens)
    counted, count = A.work_counted(lens, klens, B, glen)
    real = lambda w: sorted(i for i in w if i[0] >= 0)
    assert real(dealt) == plain == sorted(plain) and len(set(plain)) == len(plain)
    assert plain == [(b, q) for b in range(B) for q in range((lens[b] + 127) // 128)]
    assert len(dealt) % A.XCDS == 0 and all(i == (-1, 0) for i in dealt if i[0] < 0) and (-1, 0) in dealt
    assert counted[:count] == dealt and count == len(dealt) and len(counted) > count + A.XCDS and len(counted) % A.XCDS != 0
    assert all(b == B and 0 <= q * 128 < glen for b, q in counted[count:])
    # longest key range first: the first item of the list is the utterance with the most keys
    assert dealt[0] == (max(range(B), key=lambda b: (klens[b], -b)), 0)
    ops = A.operands(256, 2, variant)
    for b, q in counted:
        assert -1 <= b <= B and (b < 0 or q * 128 < ops.lens[b])
    for s, n, kn in zip(ops.starts, ops.lens, ops.klens):
        assert s % A.ATT_ALIGN == 0 and s >= 8 and 0 <= kn <= n and s + n + 8 <= ops.R <= ops.Rvt and ops.Rvt % 128 == 0
    assert all(klens[b] < lens[b] for b in range(B) if lens[b]) == (variant == "short")
    assert variant == "full" or any(k % 8 for k in klens)


@pytest.mark.parametrize("D,heads", A.HEADS)
def test_operands_are_exact_pairs_with_nan_where_nothing_lives(D, heads):
    ops = A.operands(D, heads, "short")
    dk = D // heads
    for (hi, lo), keep in ((ops.Q, ops.is_q), (ops.K, ops.is_k), (ops.V, ops.is_k)):
        assert bool(torch.isnan(hi[~keep].float()).all()) and bool(torch.isnan(lo[~keep].float()).all())
        v = G.pair_value(hi[keep], lo[keep])
        assert bool(torch.isfinite(v).all()) and bool((v.float().double() == v).all())
        assert float((lo[keep].float().abs() - 2.0 ** -8 * hi[keep].float().abs()).max()) <= 0.0
    # Q is the fp32 product with the plan's scale, split; K and V are the split of the fp32 rows attn_f32 reads
    sc = torch.tensor(A.softmax_scale(dk))
    assert float(sc) == float(np.float32(A.LOG2E) / np.sqrt(np.float32(dk)))
    q = ops.q32[ops.is_q] * sc
    assert torch.equal(G.pair_value(ops.Q[0][ops.is_q], ops.Q[1][ops.is_q]), G.pair_value(*G.split_bf16(q)))
    assert float((G.pair_value(ops.K[0][ops.is_k], ops.K[1][ops.is_k]) - ops.k32[ops.is_k].double()).abs().max()) <= 2.0 ** -17 * 2
    # gaps, dead keys of an utterance, the rows behind the last utterance and the tail are no live key; the ghost's rows are (its own)
    s, n, kn = ops.utterances()[5]
    assert bool(ops.is_k[s:s + kn].all()) and not bool(ops.is_k[s + kn:s + n + 8].any()) and bool(ops.is_q[s:s + n].all()) and not bool(ops.is_q[s + n:s + n + 8].any())
    gs, gn, gk = ops.starts[-1], ops.lens[-1], ops.klens[-1]
    assert bool(ops.is_k[gs:gs + gk].all()) and not bool(ops.is_k[gs + gn:].any()) and not bool(ops.written_rows()[gs:].any())
    # the images: qk [Rvt][Q | K], vt [D][Rvt]
    qk_hi, qk_lo, vt_hi, vt_lo = ops.images()
    assert qk_hi.shape == (ops.Rvt, 2 * D) and vt_lo.shape == (D, ops.Rvt) and qk_hi.is_contiguous() and vt_hi.is_contiguous()
    r, c = s + 3, dk + 5 if heads > 1 else 5
    assert qk_hi[r, c] == ops.Q[0][r, c] and qk_lo[r, D + c] == ops.K[1][r, c] and vt_hi[c, r] == ops.V[0][r, c] and vt_lo[c, r] == ops.V[1][r, c]
    rows = ops.qkv_rows()
    assert rows.shape == (ops.Rvt, 3 * D) and rows[r, c] == ops.q32[r, c] and rows[r, D + c] == ops.k32[r, c] and rows[r, 2 * D + c] == ops.v32[r, c]


@pytest.mark.parametrize("D,heads", A.HEADS)
def test_base_2_softmax_on_prescaled_q_is_softmax_on_natural_scores(D, heads):
    """float64: softmax_2((q log2 e / sqrt dk) . k) = softmax(q . k / sqrt dk), on this file's reference and on a plain torch.softmax statement."""
    ops = A.operands(D, heads, "short")
    dk = D // heads
    q, k, v = ops.q32.double(), ops.k32.double(), ops.v32.double()
    for mq in (0, 1):
        two = A.ref64(q * (A.LOG2E / math.sqrt(dk)), k, v, ops, mq)
        nat = A.ref64(q, k, v, ops, mq, base2=False, scale=1.0 / math.sqrt(dk))
        live = ops.written_rows()
        assert bool(torch.isfinite(two[live]).all()) and bool(torch.isnan(two[~live]).all())
        assert float((two[live] - nat[live]).abs().max()) < 1e-13
        for s, n, kn in ops.utterances():
            if n == 0 or kn == 0:
                assert n == 0 or float(nat[s:s + n].abs().max()) == 0.0
                continue
            qq = q[s:s + n].reshape(n, heads, dk).transpose(0, 1)
            kk, vv = (t[s:s + kn].reshape(kn, heads, dk).transpose(0, 1) for t in (k, v))
            o = (torch.softmax(qq @ kk.transpose(1, 2) / math.sqrt(dk), -1) @ vv).transpose(0, 1).reshape(n, D)
            if mq:
                o[kn:] = 0.0
            assert float((two[s:s + n] - o).abs().max()) < 1e-13


_fp32_figures = {}


def _figures():
    """max-abs of attn_fp32 against float64 per (case, arithmetic), once per session."""
    if not _fp32_figures:
        for key, a in A.all_cases():
            ops = A.operands(*key)
            live = ops.written_rows()
            ref, got = A.reference(ops, a, 0), A.attn_fp32(ops, a, 0)
            assert bool(torch.isfinite(got[live]).all()) and bool(torch.isnan(got[~live]).all())
            _fp32_figures[(key, a)] = float((got[live] - ref[live]).abs().max())
    return _fp32_figures


def test_recorded_cpu_figures_behind_the_bars():
    """The recorded worst error of the kernels' arithmetic in fp32 is at least the computed one and at most 1.25 x it; every bar is min(8 x recorded, ceiling)."""
    figs = _figures()
    for a in A.ARITHS:
        worst = max(v for (k, aa), v in figs.items() if aa == a)
        where = [k for (k, aa), v in figs.items() if aa == a and v == worst][0]
        print("%s: worst %.4g at %s; recorded %.4g; 8 x = %.3g, ceiling %.3g -> bar %.3g" % (a, worst, where, A.ATTN_FP32_ERR[a], 8 * A.ATTN_FP32_ERR[a], A.CEILING[a], A.BAR[a]))
        assert worst <= A.ATTN_FP32_ERR[a] <= 1.25 * worst, (a, worst, A.ATTN_FP32_ERR[a])
        assert A.BAR[a] == min(8 * A.ATTN_FP32_ERR[a], A.CEILING[a]) and A.BAR[a] <= A.CEILING[a]
        assert worst < A.BAR[a], "the fp32 statement itself misses the bar"
    from tests.test_gpu_ops import ATT_TOL
    assert A.CEILING == {"f32": ATT_TOL["fp32"], "x3": ATT_TOL["bf16x3"], "w32": ATT_TOL["bf16x3"], "x1": ATT_TOL["bf16"]}


def test_planes_rounding_stays_within_its_allowance_and_mask_q_zeroes_exactly():
    ops = A.operands(384, 2, "short")
    live = ops.written_rows()
    for a in ("x3", "w32"):
        rows, planes = A.attn_fp32(ops, a, 1), A.attn_fp32(ops, a, 1, planes=True)
        assert bool(((planes[live] - rows[live]).abs() <= A.PLANES_ROUNDING * rows[live].abs()).all())
        ref = A.reference(ops, a, 1)
        assert bool(((planes[live] - ref[live]).abs() < A.planes_bar(a, ref[live])).all())
        for s, n, kn in ops.utterances():
            assert n == kn or float(rows[s + kn:s + n].abs().max()) == 0.0 == float(ref[s + kn:s + n].abs().max())


def _mutant_cases():
    return [(k, a) for k, a in A.all_cases()]


def test_every_mutant_sits_at_8_bars_or_more():
    """On the cases' own operands, per case, arithmetic and mask_q: what a kernel that broke one rule would compute differs from the reference by 8 bars or more
    somewhere, so a GPU result within one bar of the reference cannot be the mutant's.  The split rules (q_lo . k_hi, P's lo) concern the three-term arithmetics only."""
    worst = {}
    for key, a in _mutant_cases():
        ops = A.operands(*key)
        live = ops.written_rows()
        for mq in ((0, 1) if key[3] is None else (0,)):
            ref = A.reference(ops, a, mq)
            for mu in A.MUTANTS:
                if mu in A.SPLIT_MUTANTS and a not in ("x3", "w32"):
                    continue
                d = float((A.reference(ops, a, mq, mutant=mu)[live] - ref[live]).abs().max()) / A.BAR[a]
                worst[(a, mu)] = min(worst.get((a, mu), float("inf")), d)
                assert d >= 8.0, (key, a, mq, mu, d)
    for k in sorted(worst):
        print("%s %s: >= %.1f bars" % (k + (worst[k],)))


@pytest.mark.parametrize("D,heads", A.W32_HEADS)
def test_spike_cases_leave_the_fast_path_exactly_as_predicted(D, heads):
    """below: the spike lifts P to ~2^45 and no wave leaves; exit: exactly the chosen wave leaves, in every head; first: the spike sits in the first tile -- the reference
    maximum -- and no wave leaves.  Every wave is at least 2^8 from the limit."""
    for spike, want in (("below", 0), ("exit", heads), ("first", 0)):
        ops = A.operands(D, heads, "full", spike)
        count, found = A.w32_exits(ops)
        assert count == want, (spike, count)
        assert len(found) == 5 * heads                     # 160 queries: four waves of item 0, one of item 1
        for b, item, wave, h, x in found:
            assert x <= A.W32_SUM_LIMIT / A.W32_MARGIN or x >= A.W32_SUM_LIMIT * A.W32_MARGIN, (spike, item, wave, h, x)
            assert (x >= A.W32_SUM_LIMIT) == (spike == "exit" and (item, wave) == (0, A.SPIKE_WAVE))
        top = max(x for *_, x in found)
        assert spike != "below" or 2.0 ** 40 < top < 2.0 ** 52      # probabilities far above 1 on the fast path
    # and the batches send no wave there
    for variant in ("full", "short"):
        assert A.w32_exits(A.operands(D, heads, variant))[0] == 0
    assert all(A.SPIKE_WAVE * 32 <= q < A.SPIKE_WAVE * 32 + 32 for q in A.SPIKE_QUERIES) and A.SPIKE_KEY // 32 == 3


def test_expected_plans():
    p = A.expected_plan("w32", 192, 2, 13)
    assert p == A.Plan("w32", 192, 0, 13, 2, 0, p.scale_bits)
    assert A.expected_plan("x3", 128, 2, 13)[:6] == ("b16", 128, 3, 32, 2, 0) and A.expected_plan("x1", 64, 2, 16)[:6] == ("b16", 64, 1, 32, 2, 0)
    assert A.expected_plan("f32", 256, 1, 17)[:6] == ("f32", 256, 0, 48, 1, 0)
    assert np.array([A.expected_plan("f32", 256, 1, 1).scale_bits], dtype=np.int32).view(np.float32)[0] == np.float32(1.0 / 16)
