"""The definition of the forced alignment (fs2_op_align: fastspeech2_amd/csrc/align.h, fastspeech2_amd/align.py; DESIGN.md section
14.7), in numpy float64.  TEST INFRASTRUCTURE: the single statement of truth the kernels, the stand-in run and the GPU tests are held to.

Per pair: states a [N, D] (the synthesized frames), frames b [M, D] (the recording), float32; an optional non-decreasing labels [N]
(int32 in [0, n_labels)); a step limit S = max_step in {1, 2}.  d(i, j) is tests/dtw_oracle.py's ``dist``.  Q(0, 0) = d(0, 0),
Q(i, 0) = +inf for i > 0, Q(i, j) = d(i, j) + min over k = 0 .. S of Q(i - k, j - 1): start with k = 0, take k = 1 if strictly
smaller, then k = 2 if strictly smaller than the best so far; a predecessor outside the matrix counts as +inf (it is never
compared).  Every frame j is assigned to one state s(j): s(M-1) = N-1, s(j-1) = s(j) - k(s(j), j).  An alignment exists iff
N >= 1, M >= 1 and N - 1 <= S (M - 1).

The record (TERMS = 8 doubles): [0] N, [1] M, [2] flags (0 fine, 1 no alignment exists, 2 the cost is not finite), [3] the cost
Q(N-1, M-1), [4] the states that received a frame, [5] the longest run of frames in one state, [6] the labels in [0, n_labels)
that received no frame, [7] 0.  With flags != 0 the durations are zeros, the states -1 and [4] .. [6] are 0; [3] is 0 for flag 1.

``align`` is the cell-by-cell statement; ``align_fast`` computes a column at a time with numpy and performs the same operations in
the same order per cell (tests/test_align_host.py holds the two to equality of bits)."""
import itertools

import numpy as np

from tests.dtw_oracle import dist

TERMS = 8
N_, M_, FLAGS, COST, STATES_USED, LONGEST_STAY, EMPTY_LABELS = range(7)
INTS = [N_, M_, FLAGS, STATES_USED, LONGEST_STAY, EMPTY_LABELS]
F64 = np.float64


def feasible(N, M, S):
    return N >= 1 and M >= 1 and N - 1 <= S * (M - 1)


class Result:
    """state [M] int32, durations [n_labels] int64, record [8] float64 (and Q [N, M] where it was computed)."""

    def __init__(self, state, durations, record, Q=None):
        self.state, self.durations, self.record, self.Q = state, durations, record, Q


def _labels(N, labels, n_labels):
    if labels is None:
        return np.arange(N, dtype=np.int64), N
    labels = np.asarray(labels, np.int64)
    assert len(labels) == N and n_labels is not None
    assert N == 0 or (np.all(np.diff(labels) >= 0) and labels[0] >= 0 and labels[-1] < n_labels), "labels: non-decreasing, in [0, n_labels)"
    return labels, int(n_labels)


def _flagged(N, M, n_labels, flag, cost=0.0):
    r = np.zeros(TERMS, F64)
    r[N_], r[M_], r[FLAGS], r[COST] = N, M, flag, cost
    return Result(np.full(M, -1, np.int32), np.zeros(n_labels, np.int64), r)


def _finish(Q, S, labels, n_labels):
    """The backtrace over a cost matrix, with the same comparisons in the same order as the recurrence, and the counts."""
    N, M = Q.shape
    cost = Q[N - 1, M - 1]
    if not np.isfinite(cost):
        out = _flagged(N, M, n_labels, 2, cost)
        out.Q = Q
        return out
    state = np.zeros(M, np.int32)
    s = N - 1
    for j in range(M - 1, 0, -1):
        state[j] = s
        best, k = Q[s, j - 1], 0
        for c in range(1, S + 1):
            if s - c >= 0 and Q[s - c, j - 1] < best:
                best, k = Q[s - c, j - 1], c
        s -= k
    assert s == 0
    state[0] = s
    durations = np.bincount(labels[state], minlength=n_labels).astype(np.int64)
    runs = np.diff(np.flatnonzero(np.concatenate([[True], np.diff(state) != 0, [True]])))
    r = np.zeros(TERMS, F64)
    r[N_], r[M_], r[COST] = N, M, cost
    r[STATES_USED], r[LONGEST_STAY], r[EMPTY_LABELS] = len(runs), runs.max(), int((durations == 0).sum())
    return Result(state, durations, r, Q)


def align(a, b, labels=None, n_labels=None, max_step=2, d=None):
    """One pair, cell by cell -> Result."""
    N, M, S = len(a), len(b), int(max_step)
    assert S in (1, 2)
    labels, n_labels = _labels(N, labels, n_labels)
    if not feasible(N, M, S):
        return _flagged(N, M, n_labels, 1)
    d = dist(a, b) if d is None else d
    inf = F64(np.inf)
    Q = np.full((N, M), inf)
    Q[0, 0] = d[0, 0]
    with np.errstate(invalid="ignore"):
        for j in range(1, M):
            for i in range(N):
                best = Q[i, j - 1]
                for k in range(1, S + 1):
                    if i - k >= 0 and Q[i - k, j - 1] < best:
                        best = Q[i - k, j - 1]
                Q[i, j] = d[i, j] + best
    return _finish(Q, S, labels, n_labels)


def align_fast(a, b, labels=None, n_labels=None, max_step=2, d=None):
    """``align`` a column at a time: the same operations per cell in the same order, so the same bits."""
    N, M, S = len(a), len(b), int(max_step)
    assert S in (1, 2)
    labels, n_labels = _labels(N, labels, n_labels)
    if not feasible(N, M, S):
        return _flagged(N, M, n_labels, 1)
    d = dist(a, b) if d is None else d
    Q = np.full((N, M), np.inf)
    Q[0, 0] = d[0, 0]
    with np.errstate(invalid="ignore"):
        for j in range(1, M):
            prev = Q[:, j - 1]
            best = prev.copy()
            for k in range(1, S + 1):
                cand = np.concatenate([np.full(min(k, N), np.inf), prev[:max(N - k, 0)]])      # outside the matrix: never smaller
                m = cand < best
                best[m] = cand[m]
            Q[:, j] = d[:, j] + best
    return _finish(Q, S, labels, n_labels)


def brute_force(d, S):
    """(the minimum of sum d over ALL admissible state sequences, one sequence that reaches it) or (None, None) if there is none;
    N <= 5, M <= 6."""
    N, M = d.shape
    assert N <= 5 and M <= 6
    best, arg = None, None
    for steps in itertools.product(range(S + 1), repeat=M - 1):
        if sum(steps) != N - 1:
            continue
        s = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
        c = F64(0)
        for j in range(M):
            c = c + d[s[j], j]
        if best is None or c < best:
            best, arg = c, s
    return best, arg


def min_gap(Q, S):
    """The smallest relative difference (second - best) / second between the best and the second-best FINITE predecessor
    Q(i - k, j - 1), k = 0 .. S, over all cells that have two (inf if no cell has): a last-bit difference of d can flip a choice
    only where this is ~ 1e-13."""
    N, M = Q.shape
    P = np.full((N + S, M), np.inf)
    P[S:] = Q
    cand = np.sort(np.stack([P[S - k:N + S - k, :-1] for k in range(S + 1)]), axis=0)      # the predecessors of columns 1 .. M-1, ascending
    best, second = cand[0], cand[1]
    ok = np.isfinite(second)
    if not ok.any():
        return np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(second[ok] > 0, (second[ok] - best[ok]) / second[ok], 0.0)
    return float(gap.min())


def records(results):
    """[Result] -> (rows [B, 8], batch [8]): [2] counts the pairs with flags != 0, every other entry is summed over the pairs with
    flags 0, in index order."""
    rows = np.stack([r.record for r in results]) if results else np.zeros((0, TERMS))
    batch = np.zeros(TERMS, F64)
    for r in rows:
        if r[FLAGS] != 0:
            batch[FLAGS] += 1
        else:
            keep = batch[FLAGS]
            batch = batch + r
            batch[FLAGS] = keep
    return rows, batch


def random_labels(rng, N):
    """A random non-decreasing map of N states onto about N / 4 phonemes, some of them empty -> (labels int32 [N], n_labels)."""
    n = max(1, N // 4) + int(rng.integers(0, 3))
    return np.sort(rng.integers(0, n, N)).astype(np.int32), n


def edge_shapes(W, T):
    """The (N, M) pairs of the edge batch for W threads of align_sweep and the distance tile T."""
    return [(1, 1), (1, 5), (2, 1), (3, 2), (5, 2), (2, 2), (T - 1, T + 1), (T + 1, T), (W - 1, W), (W, W + 1), (W + 1, W // 2 + 1),
            (2 * W + 3, W + 40), (40, 2 * W + 1), (0, 5), (5, 0)]


class Edge:
    """The edge batch at feature width D: the pairs (tests/dtw_oracle.py: warped_pair), their labels, the packed arrays with their row
    offsets, and the oracle's results ``want[(S, with_labels)]`` = (results, rows, batch, durations [B, dur_stride], state [rows of b])."""

    def __init__(self, W, T, D, seed=0):
        from tests.dtw_oracle import warped_pair
        rng = np.random.default_rng(1000 * D + 77 + seed)
        self.D, self.shapes = D, edge_shapes(W, T)
        self.pairs = [warped_pair(rng, N, M, D)[:2] for N, M in self.shapes]
        lab = [random_labels(rng, N) for N, _ in self.shapes]
        self.pair_labels, self.n_labels = [x[0] for x in lab], np.asarray([x[1] for x in lab], np.int32)
        self.a_lens = np.asarray([s[0] for s in self.shapes], np.int32)
        self.b_lens = np.asarray([s[1] for s in self.shapes], np.int32)
        self.a_starts = (np.cumsum(self.a_lens) - self.a_lens).astype(np.int32)
        self.b_starts = (np.cumsum(self.b_lens) - self.b_lens).astype(np.int32)
        self.a = np.concatenate([q[0].reshape(-1, D) for q in self.pairs]).astype(np.float32)
        self.b = np.concatenate([q[1].reshape(-1, D) for q in self.pairs]).astype(np.float32)
        self.labels = np.concatenate(self.pair_labels).astype(np.int32)
        self.dur_stride = int(max(self.a_lens.max(), self.n_labels.max())) + 3
        self._d = [dist(x, y) if len(x) and len(y) else None for x, y in self.pairs]
        self.want = {}

    def oracle(self, S, with_labels):
        key = (S, bool(with_labels))
        if key not in self.want:
            res = [align_fast(x, y, self.pair_labels[n] if with_labels else None, int(self.n_labels[n]) if with_labels else None, S, d=self._d[n])
                   for n, (x, y) in enumerate(self.pairs)]
            rows, batch = records(res)
            dur = np.zeros((len(res), self.dur_stride), np.int64)
            for n, r in enumerate(res):
                dur[n, :len(r.durations)] = r.durations
            self.want[key] = (res, rows, batch, dur, np.concatenate([r.state for r in res]).astype(np.int32))
        return self.want[key]

    def gaps(self, S):
        return [min_gap(r.Q, S) for r in self.oracle(S, False)[0] if r.Q is not None]

    def padded(self, extra_a=3, extra_b=7):
        """The same batch as [B, Sa, D] / [B, Sb, D] arrays and labels [B, Sa] (pads 0 / -1), wider than the longest pair."""
        B, Sa, Sb = len(self.pairs), int(self.a_lens.max()) + extra_a, int(self.b_lens.max()) + extra_b
        a, b, lab = np.zeros((B, Sa, self.D), np.float32), np.zeros((B, Sb, self.D), np.float32), np.full((B, Sa), -1, np.int32)
        for n, (x, y) in enumerate(self.pairs):
            a[n, :len(x)], b[n, :len(y)], lab[n, :len(x)] = x, y, self.pair_labels[n]
        return a, b, lab
