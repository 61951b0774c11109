"""DTW validation numbers on the MI355X (fs2_op_dtw: fastspeech2_amd.dtw, csrc/dtw.h) against the numpy float64 oracle of the same
definition (tests/dtw_oracle.py, itself held to a brute-force minimum and to backtracking in tests/test_dtw_host.py).

Bars.  The integer entries of a record (0, 1, 2, 6, 8: lengths, steps, counts) are exact.  The floating entries are within 1e-12
relative of the oracle: both sides perform the same IEEE double operations in the same order, so only a last-bit difference of the
device's sqrt could enter -- 1.1e-16 relative per term over at most N + M ~ 1e3 non-negative terms, about 1e-13.  Condition, asserted
on the oracle side: the smallest relative gap between the best and the second-best finite predecessor of any cell is >= 1e-9, so no
last-bit difference can flip a predecessor choice.  At D = 1 that condition cannot hold for any data: d = |a - b| and every cost is
a sum of fewer than 2^10 differences of float32 values, which is EXACT in double, so the ties of exact arithmetic (paths whose
differences telescope to the same sum) are exact ties here; there the test asserts that every gap is either exactly 0 -- decided by
the tie rule, like the cases of test_ties -- or >= 1e-9.  Independence, the NaN cases, graph replay and sync=False are held with
EQUALITY of bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dtw_oracle as O

pytestmark = pytest.mark.gpu

W = 256               # csrc/dtw.h: kDtwCols, the columns of a column block of dtw_sweep  } tests/test_dtw_kernel_host.py checks that
T = 64                # csrc/dtw.h: kDtwTile, the tile of dtw_dist                         } these agree with the header
INTS = [O.N_, O.M_, O.STEPS, O.VOICED, O.VUV]
FLOATS = [O.COST, O.ENERGY_L1, O.PITCH_L1, O.PITCH_L1_VOICED]
ERR_ARG, ERR_WORKSPACE = -1, -5      # include/fs2.h
DEV = "cuda:0"
GAP = 1e-9
ALL = 1 << 40

_edges = {}


def edge(D):
    """The edge batch at width D with its packed device tensors and the device's records (one call, everything at once)."""
    if D not in _edges:
        from fastspeech2_amd import mel_dtw
        e = O.Edge(W, T, D)
        e.dev = {k: torch.from_numpy(getattr(e, k)).to(DEV) for k in ("a", "b", "e_a", "e_b", "p_a", "p_b")}
        e.got = mel_dtw(e.dev["a"], e.a_lens, e.dev["b"], e.b_lens, e=(e.dev["e_a"], e.dev["e_b"]), p=(e.dev["p_a"], e.dev["p_b"]), workspace_cap=ALL)
        _edges[D] = e
    return _edges[D]


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _check(got_rows, want_rows, what=""):
    assert np.array_equal(got_rows[:, INTS], want_rows[:, INTS]), what
    rel = np.abs(got_rows[:, FLOATS] - want_rows[:, FLOATS]) / np.maximum(np.abs(want_rows[:, FLOATS]), 1e-300)
    print("%s worst relative difference of a floating entry: %.3g" % (what, rel.max() if rel.size else 0.0))
    assert O.close(got_rows[:, FLOATS], want_rows[:, FLOATS]), what
    assert np.all(got_rows[:, 9:] == 0)


def _call(pairs, order=None, **kw):
    """mel_dtw on a list of oracle pairs (a, b, e, p), packed in the given order."""
    from fastspeech2_amd import mel_dtw
    order = list(range(len(pairs))) if order is None else order
    q = [pairs[i] for i in order]
    D = q[0][0].shape[1]
    cat = lambda xs, w=None: _dev(np.concatenate([np.asarray(x, np.float32).reshape((-1, w) if w else (-1,)) for x in xs]))
    return mel_dtw(cat([x[0] for x in q], D), [len(x[0]) for x in q], cat([x[1] for x in q], D), [len(x[1]) for x in q],
                   e=(cat([x[2][0] for x in q]), cat([x[2][1] for x in q])), p=(cat([x[3][0] for x in q]), cat([x[3][1] for x in q])), **kw)


@pytest.mark.parametrize("D", [1, 3, 13, 80])
def test_edge_batch_equals_the_oracle(D):
    e = edge(D)
    assert e.shapes == [(1, 1), (1, W + 1), (W + 1, 1), (2, 2), (T - 1, T + 1), (T, T), (W - 1, W), (W, W + 1), (2 * W + 1, 40), (40, 2 * W + 1),
                        (0, 5), (5, 0)]
    if D == 1:                # (see the docstring: exact ties of exact arithmetic, otherwise the same condition)
        gaps = e.gaps(nonzero=True)
        print("D = 1: smallest non-zero gap %.3g, %d exact ties" % (min(g for g, _ in gaps), sum(n for _, n in gaps)))
        assert all(g >= GAP for g, _ in gaps)
        for a, b, _, _ in e.pairs:
            if len(a) and len(b):
                assert np.array_equal(O.dist(a, b), np.abs(a.astype(np.float64) - b.astype(np.float64).T))
    else:
        gaps = e.gaps()
        print("D = %d: smallest gap %.3g" % (D, min(gaps)))
        assert all(g >= GAP for g in gaps)
    _check(e.got.terms, e.rows, "D = %d:" % D)
    assert np.array_equal(e.got.batch[INTS], e.batch[INTS]) and O.close(e.got.batch[FLOATS], e.batch[FLOATS]) and np.all(e.got.batch[9:] == 0)
    assert np.all(e.got.terms[10:, 2:] == 0)                               # N = 0 / M = 0: the lengths and zeros
    assert e.got.D == D and e.got.features == "mel" and len(e.got) == 12
    pu, want = e.got.per_utterance(), e.rows
    assert np.array_equal(pu["steps"], want[:, O.STEPS].astype(np.int64))
    assert np.allclose(pu["lsd_db"][:10], 20 / np.log(10) * want[:10, O.COST] / want[:10, O.STEPS] / np.sqrt(D), rtol=1e-12, atol=0)


def test_ties():
    """d is exactly equal or exactly 0 here whatever sqrt does: steps and every count are exactly the tie rule's."""
    rng = np.random.default_rng(7)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    D = 5
    x, y = f(W + 44, D), f(100, D)
    tx = (np.abs(f(len(x))), np.where(rng.random(len(x)) < 0.4, 0, 100 + np.abs(f(len(x)))).astype(np.float32))
    ty = (np.abs(f(len(y))), np.where(rng.random(len(y)) < 0.4, 0, 100 + np.abs(f(len(y)))).astype(np.float32))
    rep = lambda v, r: np.repeat(v, r, axis=0)
    const = lambda n, c: np.full((n, D), c, np.float32)
    ones = lambda n, c=1.0: np.full(n, c, np.float32)
    pairs = [(x, x, (tx[0], tx[0]), (tx[1], tx[1])),                                        # identical: cost 0, steps N
             (rep(y, 3), y, (rep(ty[0], 3), ty[0]), (rep(ty[1], 3), ty[1])),                # every frame three times: cost 0, steps max(N, M)
             (y, rep(y, 3), (ty[0], rep(ty[0], 3)), (ty[1], rep(ty[1], 3))),
             (const(70, 1.5), const(W + 44, -2.0), (ones(70), ones(W + 44, 3.0)), (ones(70, 0.0), ones(W + 44, 120.0))),     # constant: every d equal
             (const(W + 1, 0.0), const(T + 1, 0.0), (ones(W + 1), ones(T + 1)), (ones(W + 1, 90.0), ones(T + 1, 0.0)))]      # all zeros
    want = np.stack([O.record_fast(*q) for q in pairs])
    for q, w in zip(pairs[:3], want[:3]):
        assert w[O.COST] == 0 and w[O.STEPS] == max(len(q[0]), len(q[1])) and w[O.ENERGY_L1] == 0 and w[O.PITCH_L1] == 0 and w[O.VUV] == 0
    assert want[3, O.STEPS] == W + 44 and want[3, O.VUV] == W + 44 and want[4, O.STEPS] == W + 1 and want[4, O.COST] == 0
    got = _call(pairs, workspace_cap=ALL).terms
    _check(got, want, "ties:")
    assert np.all(got[[0, 1, 2, 4], O.COST] == 0) and _bits(got[:3, 4:9], want[:3, 4:9])


def test_independence_bit_for_bit():
    e = edge(13)
    rows = e.got.terms
    B = len(e.pairs)
    for n in range(B):
        alone = _call(e.pairs, [n])
        assert _bits(alone.terms[0], rows[n]) and _bits(alone.batch, rows[n]), n
    order = [7, 10, 0, 9, 3, 11, 1, 8, 5, 2, 6, 4]
    assert _bits(_call(e.pairs, order, workspace_cap=ALL).terms, rows[order])
    from fastspeech2_amd import _lib, mel_dtw
    a, b, te, tp = e.padded()
    padded = mel_dtw(_dev(a), e.a_lens, _dev(b), e.b_lens, e=(_dev(te[0]), _dev(te[1])), p=(_dev(tp[0]), _dev(tp[1])))
    assert _bits(padded.terms, rows)
    wide_a, wide_e = torch.zeros(B, a.shape[1] + 5, 13, device=DEV), torch.zeros(B, a.shape[1] + 9, device=DEV)      # views with wider strides;
    wide_a[:, :a.shape[1]] = _dev(a)                                                                                 # the tracks' stride differs
    wide_e[:, :a.shape[1]] = _dev(te[0])
    strided = mel_dtw(wide_a[:, :a.shape[1]], e.a_lens, _dev(b), e.b_lens, e=(wide_e[:, :a.shape[1]], _dev(te[1])), p=(_dev(tp[0]), _dev(tp[1])))
    assert _bits(strided.terms, rows)
    one_per_group = _call(e.pairs, workspace_cap=0)
    assert _bits(one_per_group.terms, rows) and _bits(one_per_group.batch, e.got.batch)
    i32p = C.POINTER(C.c_int32)
    lens = (e.a_lens.ctypes.data_as(i32p), e.b_lens.ctypes.data_as(i32p))
    least, everything = (int(_lib.lib().fs2_op_dtw_workspace_bytes(B, *lens, cap)) for cap in (0, ALL))
    assert least < (least + everything) // 2 < everything
    some = _call(e.pairs, workspace_cap=(least + everything) // 2)        # groups of several pairs
    assert _bits(some.terms, rows) and _bits(some.batch, e.got.batch)
    in_order = np.zeros(O.TERMS)
    for r in rows:
        in_order = in_order + r
    assert _bits(e.got.batch, in_order)


def test_nan():
    from fastspeech2_amd import mel_dtw
    e = edge(13)
    rows = e.got.terms
    a, b, te, tp = e.padded()
    for n, (x, y, _, _) in enumerate(e.pairs):                              # a NaN parked in the pad rows changes no bit
        for t, L in ((a, len(x)), (te[0], len(x)), (tp[0], len(x)), (b, len(y)), (te[1], len(y)), (tp[1], len(y))):
            t[n, L:] = np.nan
    parked = mel_dtw(_dev(a), e.a_lens, _dev(b), e.b_lens, e=(_dev(te[0]), _dev(te[1])), p=(_dev(tp[0]), _dev(tp[1])))
    assert _bits(parked.terms, rows) and _bits(parked.batch, e.got.batch)
    # a NaN in a valid frame: frame i of a poisons row i of the matrix; C(N-1, M-1) is NaN when M >= N - i (else +inf: the first
    # columns of the rows below have only +inf and NaN predecessors, and NaN < inf is false) -- both cases below have M >= N - i
    pairs = [tuple(np.copy(t) if isinstance(t, np.ndarray) else tuple(np.copy(u) for u in t) for t in q) for q in e.pairs]
    pairs[7][0][W - 1, 3] = np.nan                                          # (W, W + 1): the last frame, in the second column block's reach
    pairs[5][1][20, 0] = np.nan                                             # (T, T): frame 20 of b
    got = _call(pairs, workspace_cap=ALL)
    for n in (5, 7):
        assert np.isnan(got.terms[n, O.COST]) and np.isnan(O.record_fast(*pairs[n])[O.COST]), n
    others = [n for n in range(len(pairs)) if n not in (5, 7)]
    assert _bits(got.terms[others], rows[others])
    assert np.isnan(got.batch[O.COST]) and np.array_equal(got.batch[[0, 1]], e.got.batch[[0, 1]])


def test_sync_false_and_graph_replay():
    e = edge(13)
    args = (e.dev["a"], e.a_lens, e.dev["b"], e.b_lens)
    kw = dict(e=(e.dev["e_a"], e.dev["e_b"]), p=(e.dev["p_a"], e.dev["p_b"]))
    from fastspeech2_amd import mel_dtw
    later = mel_dtw(*args, sync=False, **kw)
    assert later._device is not None and later._terms is None             # nothing was read back
    assert _bits(later.terms, e.got.terms) and _bits(later.batch, e.got.batch) and later._device is None
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = mel_dtw(*args, sync=False, workspace_cap=1 << 20, **kw)      # several groups: the workspace is reused inside the graph
        captured._device.fill_(float("nan"))                              # whatever the capture left: only a replay's numbers count
        graph.replay()
    side.synchronize()
    assert _bits(captured.terms, e.got.terms) and _bits(captured.batch, e.got.batch)


def test_many_pairs_and_none():
    B = 200                            # beyond the 96 records of one upload launch
    rng = np.random.default_rng(200)
    pairs = [O.warped_pair(rng, int(n), int(m), 4) for n, m in zip(rng.integers(1, 6, B), rng.integers(1, 6, B))]
    rows, batch = O.records(pairs)
    got = _call(pairs)
    _check(got.terms, rows, "B = 200:")
    assert np.array_equal(got.batch[INTS], batch[INTS]) and O.close(got.batch[FLOATS], batch[FLOATS])
    from fastspeech2_amd import mel_dtw
    none = mel_dtw(torch.zeros(0, 4, device=DEV), [], torch.zeros(0, 4, device=DEV), [])
    assert len(none) == 0 and np.all(none.batch == 0) and none.terms.shape == (0, O.TERMS)


def test_mcep_features():
    """The projection is plumbing (a torch float64 matmul rounded to float32): it agrees with numpy's to float32 rounding, and the
    records are the oracle's on the projected values."""
    from fastspeech2_amd import mel_dtw
    from fastspeech2_amd.dtw import mcep
    rng = np.random.default_rng(5)
    pairs = [O.warped_pair(rng, n, m, 80) for n, m in ((50, 61), (W + 3, 90))]
    proj = [(mcep(_dev(a)).cpu().numpy(), mcep(_dev(b)).cpu().numpy(), e, p) for a, b, e, p in pairs]
    for (a, _, _, _), (pa, _, _, _) in zip(pairs, proj):
        assert pa.shape == (len(a), 13) and np.allclose(pa, O.mcep(a), rtol=0, atol=4e-7 * np.abs(O.mcep(a)).max())
    assert min(O.min_gap(O.dist(a, b)) for a, b, _, _ in proj) >= GAP
    got = _call(pairs, features="mcep")
    _check(got.terms, np.stack([O.record_fast(*q) for q in proj]), "mcep:")
    assert got.features == "mcep" and got.D == 13
    pu = got.per_utterance()
    assert "lsd_db" not in pu and np.allclose(pu["mcd_db"], 10 * np.sqrt(2) / np.log(10) * got.terms[:, O.COST] / got.terms[:, O.STEPS], rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="features"):
        got.merge(edge(13).got)


@pytest.fixture(scope="module")
def model():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import ljspeech_durations, portable_state_dict
    hp = default_hparams()
    m = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    m.load_state_dict(ljspeech_durations(portable_state_dict(m.state_dict(), seed=0)))
    return m.to(DEV)


def test_evaluate_free_running(model):
    from fastspeech2_amd.synthetic import make_batch
    b = make_batch("c2", B=3, tlens=[12, 7, 9], seed=11)
    rng = np.random.default_rng(11)
    ys = torch.from_numpy(rng.normal(-5, 2, (3, int(b["olens"].max()) + 2, 80)).astype(np.float32))
    xs = b["xs"].to(DEV)
    with torch.no_grad():
        got = model.evaluate_free_running(xs, b["ilens"], ys.to(DEV), b["olens"], b["es"].to(DEV), b["ps"].to(DEV))
        mels, olens = model.inference_batch(xs, b["ilens"])
        r = model._run(xs, b["ilens"], is_inference=True, want=("after", "e_outs", "p_outs"))
        assert torch.equal(r["after"], mels) and torch.equal(r["olens"], olens)
        print("free-running frames %s against %s recorded" % (olens.tolist(), b["olens"].tolist()))
        assert int(olens.min()) > 0
        mel_np, e_np, p_np = (r[k].cpu().numpy() for k in ("after", "e_outs", "p_outs"))
        pairs = []
        for n in range(3):
            L, M = int(olens[n]), int(b["olens"][n])
            pairs.append((mel_np[n, :L], ys[n, :M].numpy(), (e_np[n, :L], b["es"][n, :M].numpy()), (p_np[n, :L], b["ps"][n, :M].numpy())))
        gaps = [O.min_gap(O.dist(q[0], q[1])) for q in pairs]
        print("smallest gap %.3g" % min(gaps))
        assert min(gaps) >= GAP
        rows, batch = O.records(pairs)
        _check(got.terms, rows, "evaluate_free_running:")
        assert np.allclose(got.evaluate(), (np.mean(rows[:, O.PITCH_L1] / rows[:, O.STEPS]), np.mean(rows[:, O.ENERGY_L1] / rows[:, O.STEPS]),
                                            np.mean(rows[:, O.COST] / rows[:, O.STEPS])), rtol=1e-12, atol=0)
        # against its own outputs: the diagonal, nothing to add up
        own = model.evaluate_free_running(xs, b["ilens"], r["after"], olens, r["e_outs"], r["p_outs"], sync=False)
        t = own.terms
        assert np.array_equal(t[:, O.STEPS], olens.numpy().astype(np.float64)) and np.array_equal(t[:, :2], np.stack([olens.numpy()] * 2, 1))
        assert np.all(t[:, [O.COST, O.ENERGY_L1, O.PITCH_L1, O.PITCH_L1_VOICED, O.VUV]] == 0)
        assert np.array_equal(t[:, O.VOICED], np.asarray([(p_np[n, :int(olens[n])] != 0).sum() for n in range(3)], np.float64))
        with pytest.raises(ValueError, match="features"):
            model.evaluate_free_running(xs, b["ilens"], ys.to(DEV), b["olens"], features="mfcc")


def test_argument_errors():
    from fastspeech2_amd import _lib, mel_dtw
    e = edge(13)
    a, b = e.dev["a"], e.dev["b"]
    with pytest.raises(ValueError, match="both sides"):
        mel_dtw(a, e.a_lens, b, e.b_lens, e=(e.dev["e_a"], None))
    with pytest.raises(ValueError, match="128"):
        mel_dtw(torch.zeros(4, 129, device=DEV), [4], torch.zeros(4, 129, device=DEV), [4])
    with pytest.raises(ValueError, match="rows"):
        mel_dtw(a, e.a_lens + 1, b, e.b_lens)                              # packed: the lengths add up to more rows than there are
    with pytest.raises(ValueError, match="frames per sequence"):
        mel_dtw(torch.zeros(2, 5, 13, device=DEV), [5, 6], torch.zeros(2, 5, 13, device=DEV), [5, 5])
    with pytest.raises(ValueError, match="entries"):
        mel_dtw(a, e.a_lens, b, e.b_lens, p=(e.dev["p_a"][:-1], e.dev["p_b"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_dtw(a.cpu(), e.a_lens, b, e.b_lens)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_dtw(a, e.a_lens, b, e.b_lens, e=(e.dev["e_a"].cpu(), e.dev["e_b"]))
    # the bare binding: a workspace one byte short, a track for one side only, D out of range
    lib = _lib.lib()
    i32p = C.POINTER(C.c_int32)
    p32 = lambda x: x.ctypes.data_as(i32p)
    B = len(e.a_lens)
    need = int(lib.fs2_op_dtw_workspace_bytes(B, p32(e.a_lens), p32(e.b_lens), 0))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rec = torch.empty(B + 1, O.TERMS, dtype=torch.float64, device=DEV)

    def raw(short=0, D=13, e_b=e.dev["e_b"].data_ptr()):
        x = _lib.OpDtwArgs(B, D, max(D, 13), max(D, 13), a.data_ptr(), b.data_ptr(), e.dev["e_a"].data_ptr(), e_b, None, None,
                           p32(e.a_starts), p32(e.a_lens), p32(e.b_starts), p32(e.b_lens), ws.data_ptr(), need - short, rec.data_ptr(), rec[B].data_ptr())
        return lib.fs2_op_dtw(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x))
    assert raw() == 0
    torch.cuda.synchronize()
    assert _bits(rec.cpu().numpy()[:-1, :5], e.got.terms[:, :5])           # (no pitch track: its entries are 0)
    assert raw(short=1) == ERR_WORKSPACE and "workspace" in lib.fs2_last_error(None).decode()
    assert raw(e_b=None) == ERR_ARG and raw(D=129) == ERR_ARG and raw(D=0) == ERR_ARG
