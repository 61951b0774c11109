"""The definition of the DTW validation numbers (fs2_op_dtw: fastspeech2_amd/csrc/dtw.h, fastspeech2_amd/dtw.py; DESIGN.md section
14.6), in numpy float64.  TEST INFRASTRUCTURE: the single statement of truth the kernels, the stand-in run and the GPU tests are held to.

Per pair: a [N, D] (synthesized), b [M, D] (reference), float32; optional scalar tracks e_a [N], e_b [M] (energy) and p_a, p_b (pitch,
0 = unvoiced).  d(i, j) = sqrt(sum_k (double(a[i, k]) - double(b[j, k]))^2), k in increasing order, each square one multiply and the
accumulation one add.  C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)): start with the diagonal, take (i-1, j) if
strictly smaller, then (i, j-1) if strictly smaller than the best so far; outside the matrix: +inf; C(0, 0) = d(0, 0).  A cell
carries the record of its path (copied from the chosen predecessor, extended by its own pair): steps, sum |de|, sum |dp|, the
pairs with both pitches non-zero and sum |dp| over those, the pairs with exactly one pitch non-zero; sums in double in path order.

``record`` is the cell-by-cell statement; ``record_fast`` walks the anti-diagonals with numpy and performs the same operations
in the same order per cell (tests/test_dtw_host.py holds the two to equality of bits)."""
import numpy as np

TERMS = 12
N_, M_, STEPS, COST, ENERGY_L1, PITCH_L1, VOICED, PITCH_L1_VOICED, VUV = range(9)
F64 = np.float64


def dist(a, b):
    """d [N, M] float64."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), F64)
    for k in range(a.shape[1]):
        df = a[:, k].astype(F64)[:, None] - b[:, k].astype(F64)[None, :]
        acc = acc + df * df
    return np.sqrt(acc)


def _tracks(N, M, e, p):
    ea, eb = (np.zeros(N, np.float32), np.zeros(M, np.float32)) if e is None else (np.asarray(e[0], np.float32), np.asarray(e[1], np.float32))
    pa, pb = (np.zeros(N, np.float32), np.zeros(M, np.float32)) if p is None else (np.asarray(p[0], np.float32), np.asarray(p[1], np.float32))
    return ea, eb, pa, pb


def _zero_record(N, M):
    r = np.zeros(TERMS, F64)
    r[N_], r[M_] = N, M
    return r


def record(a, b, e=None, p=None, d=None, want_choice=False):
    """The record [12] of one pair, cell by cell.  ``want_choice``: also the cost matrix and the chosen predecessor of every cell
    (0 diagonal, 1 (i-1, j), 2 (i, j-1); -1 at (0, 0))."""
    N, M = len(a), len(b)
    if N == 0 or M == 0:
        return (_zero_record(N, M), None, None) if want_choice else _zero_record(N, M)
    d = dist(a, b) if d is None else d
    ea, eb, pa, pb = _tracks(N, M, e, p)
    inf = F64(np.inf)
    C = np.full((N, M), inf)
    choice = np.full((N, M), -1, np.int8)
    cells = [[None] * M for _ in range(N)]
    outside = (inf, 0, F64(0), F64(0), 0, F64(0), 0)
    for i in range(N):
        for j in range(M):
            if i == 0 and j == 0:
                best, sel = (F64(0),) + outside[1:], -1
            else:
                best, sel = (cells[i - 1][j - 1] if i > 0 and j > 0 else outside), 0
                up = cells[i - 1][j] if i > 0 else outside
                left = cells[i][j - 1] if j > 0 else outside
                if up[0] < best[0]:
                    best, sel = up, 1
                if left[0] < best[0]:
                    best, sel = left, 2
            cost, steps, se, sp, nv, spv, mis = best
            de = abs(F64(ea[i]) - F64(eb[j]))
            dp = abs(F64(pa[i]) - F64(pb[j]))
            va, vb = pa[i] != 0, pb[j] != 0
            if va and vb:
                nv, spv = nv + 1, spv + dp
            elif va != vb:
                mis += 1
            cells[i][j] = (d[i, j] + cost, steps + 1, se + de, sp + dp, nv, spv, mis)
            C[i, j], choice[i, j] = cells[i][j][0], sel
    cost, steps, se, sp, nv, spv, mis = cells[N - 1][M - 1]
    r = _zero_record(N, M)
    r[STEPS:VUV + 1] = steps, cost, se, sp, nv, spv, mis
    return (r, C, choice) if want_choice else r


def backtrack(choice):
    """The path [(i, j)] from (N-1, M-1) back to (0, 0) along the recorded choices, in path order."""
    i, j = choice.shape[0] - 1, choice.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        c = choice[i, j]
        i, j = (i - 1, j - 1) if c == 0 else (i - 1, j) if c == 1 else (i, j - 1)
        path.append((i, j))
    return path[::-1]


def brute_force_min(d):
    """The minimum of sum d over ALL monotone paths from (0, 0) to (N-1, M-1) (steps (1,1), (1,0), (0,1)); N, M <= 5."""
    N, M = d.shape
    assert N <= 5 and M <= 5
    best = [np.inf]

    def walk(i, j, s):
        s = s + d[i, j]
        if i == N - 1 and j == M - 1:
            best[0] = min(best[0], s)
            return
        if i + 1 < N and j + 1 < M:
            walk(i + 1, j + 1, s)
        if i + 1 < N:
            walk(i + 1, j, s)
        if j + 1 < M:
            walk(i, j + 1, s)
    walk(0, 0, 0.0)
    return best[0]


def _padded(N, M, fill, dtype=F64):
    return np.full((N + 1, M + 1), fill, dtype)


def record_fast(a, b, e=None, p=None, d=None, want_cost=False):
    """``record`` along the anti-diagonals: the same operations per cell in the same order, so the same bits."""
    N, M = len(a), len(b)
    if N == 0 or M == 0:
        return (_zero_record(N, M), None) if want_cost else _zero_record(N, M)
    d = dist(a, b) if d is None else d
    ea, eb, pa, pb = _tracks(N, M, e, p)
    # matrices shifted by one: row 0 / column 0 are "outside" (+inf, empty record); [0, 0] is the empty path (0.0) before (0, 0)
    C = _padded(N, M, np.inf)
    C[0, 0] = 0.0
    F = {k: _padded(N, M, 0, t) for k, t in (("steps", np.int64), ("se", F64), ("sp", F64), ("nv", np.int64), ("spv", F64), ("mis", np.int64))}
    with np.errstate(invalid="ignore"):
        for k in range(N + M - 1):
            i = np.arange(max(0, k - M + 1), min(N - 1, k) + 1)
            j = k - i
            best, si, sj = C[i, j].copy(), i.copy(), j.copy()              # diagonal: (i-1, j-1) is [i, j] of the shifted matrix
            up, left = C[i, j + 1], C[i + 1, j]
            m = up < best
            best[m], si[m], sj[m] = up[m], i[m], (j + 1)[m]
            m = left < best
            best[m], si[m], sj[m] = left[m], (i + 1)[m], j[m]
            de = np.abs(ea[i].astype(F64) - eb[j].astype(F64))
            dp = np.abs(pa[i].astype(F64) - pb[j].astype(F64))
            va, vb = pa[i] != 0, pb[j] != 0
            both, one = va & vb, va != vb
            C[i + 1, j + 1] = d[i, j] + best
            F["steps"][i + 1, j + 1] = F["steps"][si, sj] + 1
            F["se"][i + 1, j + 1] = F["se"][si, sj] + de
            F["sp"][i + 1, j + 1] = F["sp"][si, sj] + dp
            F["nv"][i + 1, j + 1] = F["nv"][si, sj] + both
            F["spv"][i + 1, j + 1] = np.where(both, F["spv"][si, sj] + dp, F["spv"][si, sj])
            F["mis"][i + 1, j + 1] = F["mis"][si, sj] + one
            if k == 0:
                C[0, 0] = np.inf                                           # the empty path precedes (0, 0) only
    r = _zero_record(N, M)
    r[STEPS:VUV + 1] = F["steps"][N, M], C[N, M], F["se"][N, M], F["sp"][N, M], F["nv"][N, M], F["spv"][N, M], F["mis"][N, M]
    return (r, C[1:, 1:]) if want_cost else r


def min_gap(d, nonzero=False):
    """The smallest relative difference (second - best) / second between the best and the second-best FINITE predecessor over all
    cells that have two (inf if no cell has): a last-bit difference of d can flip a predecessor choice only where this is ~ 1e-13.
    ``nonzero=True``: -> (the smallest difference that is not 0, the number of cells where it is exactly 0)."""
    N, M = d.shape
    _, C = record_fast(np.zeros((N, 1), np.float32), np.zeros((M, 1), np.float32), d=d, want_cost=True)
    P = np.full((N + 1, M + 1), np.inf)
    P[1:, 1:] = C
    cand = np.sort(np.stack([P[:-1, :-1], P[:-1, 1:], P[1:, :-1]]), axis=0)   # the three predecessors of every cell, ascending
    best, second = cand[0], cand[1]
    ok = np.isfinite(second)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(second[ok] > 0, (second[ok] - best[ok]) / second[ok], 0.0)
    if nonzero:
        return (float(gap[gap > 0].min()) if (gap > 0).any() else np.inf), int((gap == 0).sum())
    return float(gap.min()) if gap.size else np.inf


def records(pairs):
    """[(a, b, e, p)] -> (rows [B, 12], batch [12]); the batch record is the sum over the pairs in index order."""
    rows = np.zeros((len(pairs), TERMS), F64)
    batch = np.zeros(TERMS, F64)
    for n, (a, b, e, p) in enumerate(pairs):
        rows[n] = record_fast(a, b, e, p)
        batch = batch + rows[n]
    return rows, batch


def dct_basis(D, n_mcep):
    """Orthonormal DCT-II, coefficients 1 .. n_mcep of D inputs: [D, n_mcep] float64."""
    n = np.arange(D, dtype=F64)[:, None]
    k = np.arange(1, n_mcep + 1, dtype=F64)[None, :]
    return np.sqrt(2.0 / D) * np.cos(np.pi / D * (n + 0.5) * k)


def mcep(x, n_mcep=13):
    x = np.asarray(x, np.float32)
    return (x.astype(F64) @ dct_basis(x.shape[-1], n_mcep)).astype(np.float32)


def close(got, want, rel=1e-12):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return bool(np.all(np.abs(got - want) <= rel * np.maximum(np.abs(want), 1e-300)))


def warped_pair(rng, N, M, D, noise=0.05):
    """a [N, D] random; b [M, D] a time-warped copy of a plus noise; energy and pitch tracks for both sides (about a third of the
    pitch values 0 = unvoiced, warped with the frames and flipped here and there)."""
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    a = f(N, D)
    ea, pa = np.abs(f(N)), np.where(rng.random(N) < 0.33, 0, 100 + 50 * np.abs(f(N))).astype(np.float32)
    if N == 0 or M == 0:
        return a, f(M, D), (ea, np.abs(f(M))), (pa, np.abs(f(M)))
    src = np.sort(rng.integers(0, N, M))
    b = (a[src] + noise * f(M, D)).astype(np.float32)
    eb = (ea[src] + noise * f(M)).astype(np.float32)
    pb = np.where(rng.random(M) < 0.1, 0, pa[src] + np.float32(3) * f(M)).astype(np.float32)
    return a, b, (ea, eb), (pa, pb)


def edge_shapes(W, T):
    """The (N, M) pairs of the edge batch for kDtwCols = W and the distance tile T."""
    return [(1, 1), (1, W + 1), (W + 1, 1), (2, 2), (T - 1, T + 1), (T, T), (W - 1, W), (W, W + 1), (2 * W + 1, 40), (40, 2 * W + 1),
            (0, 5), (5, 0)]


class Edge:
    """The edge batch at feature width D: pairs (a, b, e, p), the packed tensors with their row offsets, the oracle's records."""

    def __init__(self, W, T, D, seed=0):
        rng = np.random.default_rng(1000 * D + seed)
        self.D, self.shapes = D, edge_shapes(W, T)
        self.pairs = [warped_pair(rng, N, M, D) for N, M in self.shapes]
        self.a_lens = np.asarray([s[0] for s in self.shapes], np.int32)
        self.b_lens = np.asarray([s[1] for s in self.shapes], np.int32)
        self.a_starts = (np.cumsum(self.a_lens) - self.a_lens).astype(np.int32)
        self.b_starts = (np.cumsum(self.b_lens) - self.b_lens).astype(np.int32)
        cat = lambda xs, w=None: np.concatenate([np.asarray(x, np.float32).reshape((-1, w) if w else (-1,)) for x in xs])
        self.a, self.b = cat([q[0] for q in self.pairs], D), cat([q[1] for q in self.pairs], D)
        self.e_a, self.e_b = cat([q[2][0] for q in self.pairs]), cat([q[2][1] for q in self.pairs])
        self.p_a, self.p_b = cat([q[3][0] for q in self.pairs]), cat([q[3][1] for q in self.pairs])
        self.rows, self.batch = records(self.pairs)

    def gaps(self, nonzero=False):
        """``min_gap`` of every pair with a matrix."""
        return [min_gap(dist(q[0], q[1]), nonzero) for q in self.pairs if len(q[0]) and len(q[1])]

    def padded(self, extra_a=3, extra_b=7):
        """The same batch as [B, Sa, D] / [B, Sb, D] and [B, Sa] / [B, Sb] arrays (pads 0), wider than the longest pair."""
        B, Sa, Sb = len(self.pairs), int(self.a_lens.max()) + extra_a, int(self.b_lens.max()) + extra_b
        a, b = np.zeros((B, Sa, self.D), np.float32), np.zeros((B, Sb, self.D), np.float32)
        ea, pa, eb, pb = np.zeros((B, Sa), np.float32), np.zeros((B, Sa), np.float32), np.zeros((B, Sb), np.float32), np.zeros((B, Sb), np.float32)
        for n, (x, y, e, p) in enumerate(self.pairs):
            a[n, :len(x)], b[n, :len(y)] = x, y
            ea[n, :len(x)], eb[n, :len(y)], pa[n, :len(x)], pb[n, :len(y)] = e[0], e[1], p[0], p[1]
        return a, b, (ea, eb), (pa, pb)
