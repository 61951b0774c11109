"""Forced alignment on the MI355X (fs2_op_align: fastspeech2_amd.align, csrc/align.h) against the numpy float64 oracle of the same
definition (tests/align_oracle.py, itself held to a brute-force enumeration in tests/test_align_host.py).

Bars.  The integer results are exact: ``state``, ``durations`` and the record entries 0, 1, 2, 4, 5, 6.  The cost is within 1e-12
relative of the oracle: both sides perform the same IEEE double operations in the same order, so only a last-bit difference of the
device's sqrt could enter -- 1.1e-16 relative per term over at most about 600 non-negative terms (one per frame), the derivation of
tests/test_gpu_dtw.py's bar.  Condition, asserted on the oracle side: the smallest relative gap between the best and the second-best
finite predecessor of any cell is >= 1e-9, so no last-bit difference can flip a choice.  D = 1 is left out: exact ties of exact
arithmetic, as tests/test_gpu_dtw.py explains.  The ties, independence, the NaN case, graph replay and sync=False are held with
EQUALITY."""
import numpy as np
import pytest
import torch

from tests import align_oracle as A
from tests import dtw_oracle as O

pytestmark = pytest.mark.gpu

W = 256               # csrc/align.h: kAlignThreads, the threads of align_sweep  } tests/test_align_kernel_host.py checks that
T = 64                # csrc/dtw.h: kDtwTile, the tile of dtw_dist               } these agree with the headers
DEV = "cuda:0"
GAP = 1e-9
ALL = 1 << 40

_edges = {}


def edge(D):
    if D not in _edges:
        e = A.Edge(W, T, D)
        e.dev = {k: torch.from_numpy(getattr(e, k)).to(DEV) for k in ("a", "b", "labels")}
        _edges[D] = e
    return _edges[D]


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _call(e, order=None, labels=True, S=2, **kw):
    """monotonic_align on the pairs ``order`` of an edge batch, packed in that order."""
    from fastspeech2_amd import monotonic_align
    order = list(range(len(e.pairs))) if order is None else order
    cat = lambda xs, shape, dt: _dev(np.concatenate([np.asarray(x, dt).reshape(shape) for x in xs]))
    a = cat([e.pairs[n][0] for n in order], (-1, e.D), np.float32)
    b = cat([e.pairs[n][1] for n in order], (-1, e.D), np.float32)
    lab = cat([e.pair_labels[n] for n in order], (-1,), np.int32) if labels else None
    return monotonic_align(a, e.a_lens[order], b, e.b_lens[order], labels=lab, n_labels=e.n_labels[order] if labels else None, max_step=S, **kw)


def _same(x, y):
    return (_bits(x.terms, y.terms) and _bits(x.batch, y.batch) and torch.equal(x.durations, y.durations) and torch.equal(x.state, y.state))


def _check(got, res, what=""):
    """An Alignment over packed pairs against the oracle's results, in the same order."""
    rows, batch = A.records(res)
    assert np.array_equal(got.terms[:, A.INTS], rows[:, A.INTS]), what
    rel = np.abs(got.terms[:, A.COST] - rows[:, A.COST]) / np.maximum(np.abs(rows[:, A.COST]), 1e-300)
    print("%s worst relative difference of a cost: %.3g" % (what, rel.max() if rel.size else 0.0))
    assert O.close(got.terms[:, A.COST], rows[:, A.COST]) and np.all(got.terms[:, 7] == 0), what
    assert np.array_equal(got.batch[A.INTS], batch[A.INTS]) and O.close(got.batch[A.COST], batch[A.COST]), what
    dur = got.durations.cpu().numpy()
    for n, r in enumerate(res):
        assert np.array_equal(dur[n, :len(r.durations)], r.durations) and not dur[n, len(r.durations):].any(), (what, n)
    want_state = np.concatenate([r.state for r in res] + [np.zeros(0, np.int32)])
    assert np.array_equal(got.state.cpu().numpy()[:len(want_state)], want_state), what
    assert np.array_equal(got.ok, rows[:, A.FLAGS] == 0)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("D", [3, 13, 80])
def test_edge_batch_equals_the_oracle(D, S):
    e = edge(D)
    gaps = e.gaps(S)
    print("D = %d, S = %d: smallest gap %.3g" % (D, S, min(gaps)))
    assert all(g >= GAP for g in gaps)
    for labels in (False, True):
        res = e.oracle(S, labels)[0]
        got = _call(e, labels=labels, S=S, workspace_cap=ALL)
        _check(got, res, "D = %d, S = %d, labels %s:" % (D, S, labels))
        feasible = [n for n, (N, M) in enumerate(e.shapes) if A.feasible(N, M, S)]
        assert np.array_equal(got.durations.sum(1).cpu().numpy()[feasible], e.b_lens[feasible])
        assert got.durations.shape == (len(e.pairs), int((e.n_labels if labels else e.a_lens).max())) and got.D == D and len(got) == 15
    pu = got.per_utterance()
    rows = e.oracle(S, True)[1]
    assert np.array_equal(pu["flags"], rows[:, A.FLAGS].astype(np.int64)) and np.array_equal(pu["empty_labels"], rows[:, A.EMPTY_LABELS].astype(np.int64))
    assert np.array_equal(pu["longest_stay"], rows[:, A.LONGEST_STAY].astype(np.int64))


def test_ties():
    """d is exactly 0 or exactly equal here whatever sqrt does: every comparison is exact, and so is every result."""
    from fastspeech2_amd import monotonic_align
    rng = np.random.default_rng(7)
    D = 5
    x, y = rng.normal(0, 1, (W + 44, D)).astype(np.float32), rng.normal(0, 1, (100, D)).astype(np.float32)
    const = lambda n, c: np.full((n, D), c, np.float32)
    pairs = [(x, x), (y, np.repeat(y, 3, axis=0)), (const(70, 1.5), const(W + 44, -2.0)), (const(W + 1, 0.0), const(W + 1, 0.0))]
    for S in (1, 2):
        res = [A.align_fast(a, b, max_step=S) for a, b in pairs]
        assert np.array_equal(res[0].state, np.arange(W + 44)) and res[0].record[A.COST] == 0
        assert np.all(res[1].durations == 3) and res[1].record[A.COST] == 0
        first = -(-69 // S)                                                 # constant features: the last state from frame ceil((N-1) / S) on,
        assert np.all(res[2].state[first:] == 69) and np.array_equal(res[2].state[:first + 1], np.minimum(S * np.arange(first + 1), 69))
        assert np.all(res[3].state[-(-W // S):] == W) and res[3].record[A.COST] == 0                  # the forced advance before it
        got = monotonic_align(_dev(np.concatenate([p[0] for p in pairs])), [len(p[0]) for p in pairs],
                              _dev(np.concatenate([p[1] for p in pairs])), [len(p[1]) for p in pairs], max_step=S)
        rows, batch = A.records(res)
        assert _bits(got.terms, rows) and _bits(got.batch, batch)
        assert np.array_equal(got.state.cpu().numpy(), np.concatenate([r.state for r in res]))
        for n, r in enumerate(res):
            assert np.array_equal(got.durations[n, :len(r.durations)].cpu().numpy(), r.durations)


def test_independence_bit_for_bit():
    from fastspeech2_amd import monotonic_align
    e = edge(13)
    whole = _call(e, workspace_cap=ALL)
    rows, dur, state = whole.terms, whole.durations.cpu().numpy(), whole.state.cpu().numpy()
    B = len(e.pairs)
    frames = lambda n: state[e.b_starts[n]:e.b_starts[n] + e.b_lens[n]]
    for n in range(B):
        alone = _call(e, [n])
        assert _bits(alone.terms[0], rows[n]), n
        assert np.array_equal(alone.durations[0].cpu().numpy(), dur[n, :alone.durations.shape[1]]) and not dur[n, alone.durations.shape[1]:].any(), n
        assert np.array_equal(alone.state.cpu().numpy(), frames(n)), n
    order = [7, 13, 0, 9, 3, 11, 1, 14, 8, 5, 2, 6, 12, 4, 10]
    shuffled = _call(e, order, workspace_cap=ALL)
    assert _bits(shuffled.terms, rows[order]) and np.array_equal(shuffled.durations.cpu().numpy(), dur[order])
    assert np.array_equal(shuffled.state.cpu().numpy(), np.concatenate([frames(n) for n in order]))
    a, b, lab = e.padded()

    def assert_padded(got):
        assert _bits(got.terms, rows) and _bits(got.batch, whole.batch) and np.array_equal(got.durations.cpu().numpy(), dur)
        st = got.state.cpu().numpy()
        assert st.shape == b.shape[:2]
        for n in range(B):
            assert np.array_equal(st[n, :e.b_lens[n]], frames(n)) and np.all(st[n, e.b_lens[n]:] == -1), n
    assert_padded(monotonic_align(_dev(a), e.a_lens, _dev(b), e.b_lens, labels=_dev(lab), n_labels=e.n_labels))
    wide_a, wide_b = torch.zeros(B, a.shape[1] + 5, 13, device=DEV), torch.full((B, b.shape[1] + 9, 13), float("nan"), device=DEV)
    wide_lab = torch.full((B, a.shape[1] + 2), -1, dtype=torch.int32, device=DEV)          # views with wider strides; the labels' stride differs
    wide_a[:, :a.shape[1]], wide_b[:, :b.shape[1]], wide_lab[:, :a.shape[1]] = _dev(a), _dev(b), _dev(lab)
    assert_padded(monotonic_align(wide_a[:, :a.shape[1]], e.a_lens, wide_b[:, :b.shape[1]], e.b_lens, labels=wide_lab[:, :a.shape[1]], n_labels=e.n_labels))
    assert _same(_call(e, workspace_cap=0), whole)                          # one pair per group
    in_order = A.records([A.Result(None, None, r) for r in rows])[1]
    assert _bits(whole.batch, in_order)


def test_nan():
    e = edge(13)
    whole = _call(e, workspace_cap=ALL)
    e2 = A.Edge(W, T, 13)                                                   # (the same seed: the same batch)
    x, y = e2.pairs[9]
    y = y.copy()
    y[20, 0] = np.nan                                                       # (W, W + 1): a frame of the recording -- every path passes through it
    e2.pairs[9] = (x, y)
    got = _call(e2, workspace_cap=ALL)
    assert got.terms[9, A.FLAGS] == 2 and np.isnan(got.terms[9, A.COST]) and np.all(got.terms[9, 4:] == 0) and np.array_equal(got.terms[9, :2], [W, W + 1])
    assert not got.durations[9].any() and not got.ok[9]
    st, want = got.state.cpu().numpy(), whole.state.cpu().numpy()
    mine = slice(e.b_starts[9], e.b_starts[9] + e.b_lens[9])
    assert np.all(st[mine] == -1)
    others = [n for n in range(len(e.pairs)) if n != 9]
    assert _bits(got.terms[others], whole.terms[others]) and torch.equal(got.durations[others], whole.durations[others])
    assert np.array_equal(np.delete(st, np.arange(mine.start, mine.stop)), np.delete(want, np.arange(mine.start, mine.stop)))
    assert got.batch[A.FLAGS] == whole.batch[A.FLAGS] + 1 and np.isfinite(got.batch[A.COST])


def test_sync_false_and_graph_replay():
    e = edge(13)
    whole = _call(e, workspace_cap=ALL)
    later = _call(e, sync=False)
    assert later._device is not None and later._terms is None              # nothing was read back
    assert _same(later, whole) and later._device is None
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    from fastspeech2_amd import monotonic_align
    args = (e.dev["a"], e.a_lens, e.dev["b"], e.b_lens)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = monotonic_align(*args, labels=e.dev["labels"], n_labels=e.n_labels, sync=False, workspace_cap=1 << 20)      # several groups
        captured._device.fill_(float("nan"))                              # whatever the capture left: only a replay's numbers count
        captured.durations.fill_(-5)
        captured.state.fill_(-5)
        graph.replay()
    side.synchronize()
    assert _same(captured, whole)


def test_many_pairs_and_none():
    from fastspeech2_amd import monotonic_align
    B = 200                            # beyond the 96 records of one upload launch
    rng = np.random.default_rng(200)
    pairs = [O.warped_pair(rng, int(n), int(m), 4)[:2] for n, m in zip(rng.integers(1, 6, B), rng.integers(1, 6, B))]
    res = [A.align_fast(a, b) for a, b in pairs]
    assert min(A.min_gap(r.Q, 2) for r in res if r.Q is not None) >= GAP
    got = monotonic_align(_dev(np.concatenate([p[0] for p in pairs])), [len(p[0]) for p in pairs],
                          _dev(np.concatenate([p[1] for p in pairs])), [len(p[1]) for p in pairs])
    _check(got, res, "B = 200:")
    none = monotonic_align(torch.zeros(0, 4, device=DEV), [], torch.zeros(0, 4, device=DEV), [])
    assert len(none) == 0 and np.all(none.batch == 0) and none.terms.shape == (0, A.TERMS) and none.durations.shape == (0, 0)


def test_mcep_features_and_argument_errors():
    from fastspeech2_amd import monotonic_align
    from fastspeech2_amd.dtw import mcep
    rng = np.random.default_rng(5)
    pairs = [O.warped_pair(rng, n, m, 80)[:2] for n, m in ((50, 61), (90, W + 3))]
    proj = [(mcep(_dev(a)).cpu().numpy(), mcep(_dev(b)).cpu().numpy()) for a, b in pairs]
    res = [A.align_fast(a, b) for a, b in proj]
    assert min(A.min_gap(r.Q, 2) for r in res) >= GAP
    a, b = _dev(np.concatenate([p[0] for p in pairs])), _dev(np.concatenate([p[1] for p in pairs]))
    got = monotonic_align(a, [50, 90], b, [61, W + 3], features="mcep")
    _check(got, res, "mcep:")
    assert got.features == "mcep" and got.D == 13
    with pytest.raises(ValueError, match="max_step"):
        monotonic_align(a, [50, 90], b, [61, W + 3], max_step=3)
    with pytest.raises(ValueError, match="together"):
        monotonic_align(a, [50, 90], b, [61, W + 3], labels=torch.zeros(140, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="int32"):
        monotonic_align(a, [50, 90], b, [61, W + 3], labels=torch.zeros(140, dtype=torch.int64, device=DEV), n_labels=[1, 1])
    with pytest.raises(ValueError, match="rows"):
        monotonic_align(a, [50, 91], b, [61, W + 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monotonic_align(a.cpu(), [50, 90], b, [61, W + 3])


@pytest.fixture(scope="module")
def model():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import ljspeech_durations, portable_state_dict
    hp = default_hparams()
    m = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    m.load_state_dict(ljspeech_durations(portable_state_dict(m.state_dict(), seed=0)))
    return m.to(DEV)


TLENS = [12, 40, 9, 23, 17]


def _oracle_of_run(r, ilens, ys, olens, S=2):
    """align_oracle on the downloaded outputs of a free-running forward and the recordings."""
    after, lr, L = r["after"].cpu().numpy(), r["lr_index"].cpu().numpy(), r["olens"].tolist()
    return [A.align_fast(after[n, :L[n]], ys[n, :int(olens[n])], lr[n, :L[n]], int(ilens[n]), S) for n in range(len(L))]


def test_align_durations_of_the_models_own_mels(model):
    """(a) the model's own mels against themselves: the durations the synthesis used, cost exactly 0."""
    from fastspeech2_amd.synthetic import make_batch
    b = make_batch("c2", B=5, tlens=TLENS, seed=11)
    xs = b["xs"].to(DEV)
    with torch.no_grad():
        r = model._run(xs, b["ilens"], is_inference=True, want=("after", "lr_index"))
        own, own_olens = r["after"], r["olens"]
        print("free-running frames %s" % own_olens.tolist())
        used = r["d_int"].cpu().clone()
        for n in range(5):
            used[n, int(b["ilens"][n]):] = 0
            if int(used[n].sum()) == 0:                                     # the length regulator's rule for a row of zeros: one frame per token
                used[n, :int(b["ilens"][n])] = 1
        assert torch.equal(used.sum(1), own_olens)
        mel = own.cpu().numpy()
        for n in range(5):                                                  # the condition: no two different frames of an utterance are equal
            d = O.dist(mel[n, :int(own_olens[n])], mel[n, :int(own_olens[n])])
            assert np.all(d[~np.eye(len(d), dtype=bool)] > 0)
        al = model.align_durations(xs, b["ilens"], own, own_olens)
        assert al.durations.shape == (5, 40) and al.durations.dtype == torch.int64
        assert torch.equal(al.durations.cpu(), used) and np.all(al.terms[:, A.COST] == 0) and al.ok.all()
        st = al.state.cpu().numpy()
        for n in range(5):
            assert np.array_equal(st[n, :int(own_olens[n])], np.arange(int(own_olens[n]))) and np.all(st[n, int(own_olens[n]):] == -1)


def test_align_durations_equal_the_oracle_and_feed_evaluate_batch(model):
    """(b) alpha = 1.5 and 0.7 against the oracle on the downloaded outputs; (c) a recording a third of its synthesis has no
    alignment, and only that one; (d) the durations are accepted by evaluate_batch."""
    from fastspeech2_amd.synthetic import make_batch
    b = make_batch("c2", B=5, tlens=TLENS, seed=11)
    xs = b["xs"].to(DEV)
    rng = np.random.default_rng(12)
    with torch.no_grad():
        base = model._run(xs, b["ilens"], is_inference=True, want=("after",))
        # recordings: the model's own mels, time-warped to within a tenth of their own length, plus noise.  Feasible at both alphas:
        # N <= 1.5 L + T (each of the T tokens rounds up by less than one frame) against 2 M >= 1.8 L
        olens = torch.from_numpy(np.rint(base["olens"].numpy() * rng.uniform(0.9, 1.1, 5)).astype(np.int64))
        mel = base["after"].cpu().numpy()
        ys = np.zeros((5, int(olens.max()) + 2, 80), np.float32)
        for n in range(5):
            src = np.sort(rng.integers(0, int(base["olens"][n]), int(olens[n])))
            ys[n, :int(olens[n])] = mel[n, src] + 0.05 * rng.normal(0, 1, (int(olens[n]), 80)).astype(np.float32)
        for alpha in (1.5, 0.7):
            r = model._run(xs, b["ilens"], is_inference=True, want=("after", "lr_index"), alpha=alpha)
            res = _oracle_of_run(r, b["ilens"], ys, olens)
            gaps = [A.min_gap(q.Q, 2) for q in res if q.Q is not None]
            print("alpha = %.1f: synthesized frames %s, recorded %s, smallest gap %.3g" % (alpha, r["olens"].tolist(), olens.tolist(), min(gaps)))
            assert min(gaps) >= GAP
            al = model.align_durations(xs, b["ilens"], _dev(ys), olens, alpha=alpha)
            rows, _ = A.records(res)
            assert np.array_equal(al.terms[:, A.INTS], rows[:, A.INTS]) and O.close(al.terms[:, A.COST], rows[:, A.COST])
            dur, st = al.durations.cpu().numpy(), al.state.cpu().numpy()
            assert dur.shape == (5, 40)
            for n, q in enumerate(res):
                assert np.array_equal(dur[n, :len(q.durations)], q.durations) and not dur[n, len(q.durations):].any()
                assert np.array_equal(st[n, :int(olens[n])], q.state) and np.all(st[n, int(olens[n]):] == -1)
                if q.record[A.FLAGS] == 0:
                    assert dur[n].sum() == int(olens[n])
            assert rows[:, A.FLAGS].tolist() == [0] * 5                    # (the frame counts printed above: every pair is feasible)
        # (c) utterance 1's recording cut to a third of its synthesized length
        short = olens.clone()
        short[1] = int(base["olens"][1]) // 3
        al = model.align_durations(xs, b["ilens"], _dev(ys), short)
        assert al.ok.tolist() == [True, False, True, True, True] and not al.durations[1].any() and al.terms[1, A.FLAGS] == 1
        # (d)
        al = model.align_durations(xs, b["ilens"], _dev(ys), olens)
        assert al.ok.all() and torch.equal(al.durations.sum(1).cpu(), olens)
        es = torch.from_numpy(rng.normal(0, 1, (5, ys.shape[1])).astype(np.float32))
        ps = torch.from_numpy(rng.normal(0, 1, (5, ys.shape[1])).astype(np.float32))
        terms = model.evaluate_batch(xs, b["ilens"], _dev(ys), olens, al.durations, es.to(DEV), ps.to(DEV))
        assert np.all(np.isfinite(terms.terms)) and all(np.isfinite(v) for v in terms.evaluate())
        model.reduction_factor, keep = 2, model.reduction_factor
        try:
            with pytest.raises(NotImplementedError):
                model.align_durations(xs, b["ilens"], _dev(ys), olens)
        finally:
            model.reduction_factor = keep
