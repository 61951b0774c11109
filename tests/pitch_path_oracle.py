"""Float64 numpy statement of the pitch path search of fastspeech2_amd.vocoder.pitch_candidates / pitch_path / pitch_track
(csrc/gl_pitch.h: gl_candidates; csrc/pitch_path.h: pitch_path, records_combine<8, 1, 5>), on top of
tests/pitch_oracle.py, whose frames, rho and candidate rule are used as they are.

Candidates.  Per frame the candidates of tests/pitch_oracle.py (integer lags t with rho[t] > rho[t-1], rho[t] >= rho[t+1], rho[t] > 0,
refined to t*, p, S) are put in the order "larger S, then smaller t" and the first K are kept: cand_f0 [frames, K] = sr / t*,
cand_strength [frames, K] = p, empty slots 0 / 0.

Path.  Per utterance of T frames; state 0 is "unvoiced", state c = 1 .. K is candidate c - 1, which exists iff cand_f0 > 0.  All in
double, from the float32 inputs:
  u(t, 0) = voicing_threshold;  u(t, c) = p - octave_cost * log2(f0_floor / f)
  trans(j -> c) = 0 (both unvoiced) | vu (exactly one unvoiced) | oj * |log2 f_j - log2 f_c| (both voiced), with
  vu = voiced_unvoiced_cost * s, oj = octave_jump_cost * s, s = 0.01 / time_step
  D(0, c) = u(0, c);  D(t, c) = u(t, c) + max over the existing j, ascending, of [D(t-1, j) - trans(j -> c)], a strict ">" (a tie keeps
  the smaller j); the end state is the largest D(T-1, c), a tie to the smaller c; then the walk back.
Results: f0 / state (c - 1, -1 unvoiced) / strength per frame and a record of TERMS doubles (the indices below).  A candidate value
(f0 or strength) that is not finite or is negative anywhere in the utterance: flags 2, outputs 0 / -1 / 0, the other entries 0.
Test infrastructure only."""
import itertools
from typing import NamedTuple

import numpy as np

from tests import pitch_oracle as P

TERMS = 8
N_FRAMES, FLAGS, SCORE, VOICED, SWITCHES, MAX_STEP, CHANGED = range(7)
MAX_CANDS = 8
DEFAULTS = dict(f0_floor=71.0, voicing_threshold=0.45, octave_cost=0.02, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14)


# ---- candidates ----
class Cands(NamedTuple):
    f0: np.ndarray          # [frames, K] sr / t*, 0 = empty slot
    strength: np.ndarray    # [frames, K] p
    S: np.ndarray           # [frames, K] the score the slots are ordered by, -inf = empty
    lag: np.ndarray         # [frames, K] integer lag, -1 = empty
    prominent: np.ndarray   # [frames, K] bool: max(c - a, c - b) >= 1e-4 and c >= 1e-4
    rho: np.ndarray         # [frames, tmax - tmin + 3] rho at the lags tmin - 1 .. tmax + 1
    tmin: int


def candidates(sig, n_fft, hop, win, sr, K=MAX_CANDS, f0_floor=71.0, f0_ceil=800.0, octave_cost=0.02, rho_noise=None, **_):
    """The first K candidates per frame.  ``rho_noise``: (amplitude, seed) of uniform noise added to rho, the size of a float32
    implementation's error (the stability experiments of tests/test_pitch_path_host.py)."""
    tmin, tmax = P.lag_range(sr, win, f0_floor, f0_ceil)
    y = P.frames_of(sig, n_fft, hop, win)
    L = y.shape[0]
    r = np.fft.irfft(np.abs(np.fft.rfft(y, axis=1)) ** 2, n=n_fft, axis=1)
    w = P.hann_padded(n_fft, win)
    rw = np.fft.irfft(np.abs(np.fft.rfft(w)) ** 2, n=n_fft)
    live = r[:, 0] > 1e-12
    lags = np.arange(tmin - 1, tmax + 2)
    rho = np.zeros((L, lags.size))
    rho[live] = (r[live][:, lags] / r[live, :1]) / (rw[lags] / rw[0])[None, :]
    if rho_noise is not None:
        rho = rho + rho_noise[0] * np.random.RandomState(rho_noise[1]).uniform(-1, 1, rho.shape) * live[:, None]
    a, c, b = rho[:, :-2], rho[:, 1:-1], rho[:, 2:]
    cand = (c > a) & (c >= b) & (c > 0) & live[:, None]
    den = np.where(cand, a - 2 * c + b, -1.0)
    d = 0.5 * (a - b) / den
    ts = lags[1:-1][None, :] + d
    p = c - 0.25 * (a - b) * d
    S = np.where(cand, p - octave_cost * np.log2(np.where(cand, f0_floor * ts / sr, 1.0)), -np.inf)
    order = np.argsort(-S, axis=1, kind="stable")[:, :K]          # larger S first, equal S: the smaller lag
    if order.shape[1] < K:
        order = np.concatenate([order, np.zeros((L, K - order.shape[1]), np.int64)], axis=1)
        pad = np.arange(K)[None, :] >= S.shape[1]
    else:
        pad = np.zeros((L, K), bool)
    rows = np.arange(L)[:, None]
    has = cand[rows, order] & ~pad
    prom = has & (np.maximum(c - a, c - b)[rows, order] >= 1e-4) & (c[rows, order] >= 1e-4)
    return Cands(np.where(has, sr / np.where(has, ts[rows, order], 1.0), 0.0), np.where(has, p[rows, order], 0.0),
                 np.where(has, S[rows, order], -np.inf), np.where(has, lags[1:-1][order], -1), prom, rho, tmin)


def score(f0, strength, f0_floor=71.0, octave_cost=0.02):
    """S of a slot recomputed in double from its f0 and strength (u(t, c) of the path); -inf for an empty slot."""
    f = np.asarray(f0, np.float64)
    has = f > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(has, np.asarray(strength, np.float64) - octave_cost * np.log2(f0_floor / np.where(has, f, 1.0)), -np.inf)


# ---- the path ----
class Path(NamedTuple):
    f0: np.ndarray          # [T] float32
    state: np.ndarray       # [T] int32
    strength: np.ndarray    # [T] float32
    record: np.ndarray      # [TERMS] float64
    D: np.ndarray           # [T, K + 1] float64, -inf at missing states (None when flagged)
    gap: float              # smallest (best - second-best predecessor) / |cell| over all cells (inf without a second one)


def _costs(time_step, octave_jump_cost, voiced_unvoiced_cost):
    s = 0.01 / float(time_step)
    return float(octave_jump_cost) * s, float(voiced_unvoiced_cost) * s


def _local(cand_f0, cand_strength, f0_floor, voicing_threshold, octave_cost):
    """(exists [T, K + 1], u [T, K + 1], lg [T, K + 1]) in double; u and lg are 0 at missing states."""
    f = np.asarray(cand_f0, np.float32).astype(np.float64)
    p = np.asarray(cand_strength, np.float32).astype(np.float64)
    T, K = f.shape
    ex = np.ones((T, K + 1), bool)
    ex[:, 1:] = f > 0
    safe = np.where(ex[:, 1:], f, 1.0)
    u = np.full((T, K + 1), float(voicing_threshold))
    u[:, 1:] = np.where(ex[:, 1:], p - float(octave_cost) * np.log2(float(f0_floor) / safe), 0.0)
    lg = np.zeros((T, K + 1))
    lg[:, 1:] = np.where(ex[:, 1:], np.log2(safe), 0.0)
    return ex, u, lg


def flagged(cand_f0, cand_strength):
    x = np.concatenate([np.asarray(cand_f0, np.float32).ravel(), np.asarray(cand_strength, np.float32).ravel()])
    return bool(np.any(~np.isfinite(x) | (x < 0)))


def _trans(j, c, lgj, lgc, oj, vu):
    if j == 0 and c == 0:
        return 0.0
    if j == 0 or c == 0:
        return vu
    return oj * abs(lgj - lgc)


def _finish(cand_f0, cand_strength, ex, u, lg, D, bp, gap):
    """End state, walk back, outputs and the record."""
    f32, p32 = np.asarray(cand_f0, np.float32), np.asarray(cand_strength, np.float32)
    T, K = f32.shape
    end, best = 0, D[T - 1, 0]
    for c in range(1, K + 1):
        if ex[T - 1, c] and D[T - 1, c] > best:
            end, best = c, D[T - 1, c]
    st = np.zeros(T, np.int64)
    st[T - 1] = end
    for t in range(T - 1, 0, -1):
        st[t - 1] = bp[t, st[t]]
    rows = np.arange(T)
    v = st > 0
    f0 = np.where(v, f32[rows, np.maximum(st - 1, 0)], np.float32(0)).astype(np.float32)
    strength = np.where(v, p32[rows, np.maximum(st - 1, 0)], np.float32(0)).astype(np.float32)
    frame_best = np.zeros(T, np.int64)                      # the per-frame argmax of u: strict ">", ascending, a tie keeps the smaller state
    for t in range(T):
        b = u[t, 0]
        for c in range(1, K + 1):
            if ex[t, c] and u[t, c] > b:
                frame_best[t], b = c, u[t, c]
    both = v[1:] & v[:-1]
    steps = np.abs(lg[rows[:-1], st[:-1]] - lg[rows[1:], st[1:]])[both]
    rec = np.zeros(TERMS)
    rec[N_FRAMES], rec[SCORE], rec[VOICED] = T, best, v.sum()
    rec[SWITCHES] = (v[1:] != v[:-1]).sum()
    rec[MAX_STEP] = steps.max() if steps.size else 0.0
    rec[CHANGED] = (st != frame_best).sum()
    return Path(f0, (st - 1).astype(np.int32), strength, rec, D, gap)


def _empty_or_flagged(cand_f0, cand_strength):
    T = np.asarray(cand_f0).shape[0]
    rec = np.zeros(TERMS)
    rec[N_FRAMES] = T
    if T and flagged(cand_f0, cand_strength):
        rec[FLAGS] = 2
    if T == 0 or rec[FLAGS]:
        return Path(np.zeros(T, np.float32), np.full(T, -1, np.int32), np.zeros(T, np.float32), rec, None, np.inf)
    return None


def path_cells(cand_f0, cand_strength, time_step, f0_floor=71.0, voicing_threshold=0.45, octave_cost=0.02, octave_jump_cost=0.35,
               voiced_unvoiced_cost=0.14):
    """The definition, cell by cell in Python floats."""
    out = _empty_or_flagged(cand_f0, cand_strength)
    if out is not None:
        return out
    oj, vu = _costs(time_step, octave_jump_cost, voiced_unvoiced_cost)
    ex, u, lg = _local(cand_f0, cand_strength, f0_floor, voicing_threshold, octave_cost)
    T, K1 = ex.shape
    D = np.full((T, K1), -np.inf)
    bp = np.zeros((T, K1), np.int64)
    D[0] = np.where(ex[0], u[0], -np.inf)
    gap = np.inf
    for t in range(1, T):
        for c in range(K1):
            if not ex[t, c]:
                continue
            best, bj, second = None, 0, None
            for j in range(K1):
                if not ex[t - 1, j]:
                    continue
                v = float(D[t - 1, j]) - _trans(j, c, float(lg[t - 1, j]), float(lg[t, c]), oj, vu)
                if best is None:
                    best, bj = v, j
                elif v > best:
                    second, best, bj = best, v, j
                elif second is None or v > second:
                    second = v
            D[t, c] = float(u[t, c]) + best
            bp[t, c] = bj
            if second is not None:
                gap = min(gap, (best - second) / abs(D[t, c]) if D[t, c] != 0 else np.inf)
    return _finish(cand_f0, cand_strength, ex, u, lg, D, bp, gap)


def path(cand_f0, cand_strength, time_step, f0_floor=71.0, voicing_threshold=0.45, octave_cost=0.02, octave_jump_cost=0.35,
         voiced_unvoiced_cost=0.14):
    """The same, a frame at a time: the same double operations per cell (a missing predecessor is -inf, which a strict ">" never
    takes over state 0's finite value), so the same bits (tests/test_pitch_path_host.py compares the two)."""
    out = _empty_or_flagged(cand_f0, cand_strength)
    if out is not None:
        return out
    oj, vu = _costs(time_step, octave_jump_cost, voiced_unvoiced_cost)
    ex, u, lg = _local(cand_f0, cand_strength, f0_floor, voicing_threshold, octave_cost)
    T, K1 = ex.shape
    D = np.full((T, K1), -np.inf)
    bp = np.zeros((T, K1), np.int64)
    D[0] = np.where(ex[0], u[0], -np.inf)
    gap = np.inf
    cells = np.arange(K1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, T):
            tr = oj * np.abs(lg[t - 1][:, None] - lg[t][None, :])          # [j, c]
            tr[0, :] = vu
            tr[:, 0] = vu
            tr[0, 0] = 0.0
            v = D[t - 1][:, None] - tr                                      # -inf rows at missing predecessors
            bj = np.argmax(v, axis=0)                                       # the first of equal maxima: the smaller j
            best = v[bj, cells]
            D[t] = np.where(ex[t], u[t] + best, -np.inf)
            bp[t] = np.where(ex[t], bj, 0)
            if ex[t - 1].sum() >= 2:
                v2 = v.copy()
                v2[bj, cells] = -np.inf
                rel = (best - v2.max(axis=0)) / np.abs(D[t])
                rel = rel[ex[t] & (D[t] != 0)]
                if rel.size:
                    gap = min(gap, float(rel.min()))
    return _finish(cand_f0, cand_strength, ex, u, lg, D, bp, gap)


def brute(cand_f0, cand_strength, time_step, f0_floor=71.0, voicing_threshold=0.45, octave_cost=0.02, octave_jump_cost=0.35,
          voiced_unvoiced_cost=0.14):
    """(best score, [state sequences (c, not c - 1) that reach it within 1e-12]) by enumerating all (K + 1)^T sequences."""
    oj, vu = _costs(time_step, octave_jump_cost, voiced_unvoiced_cost)
    ex, u, lg = _local(cand_f0, cand_strength, f0_floor, voicing_threshold, octave_cost)
    T, K1 = ex.shape
    scored = []
    for seq in itertools.product(range(K1), repeat=T):
        if not all(ex[t, c] for t, c in enumerate(seq)):
            continue
        s = sum(u[t, c] for t, c in enumerate(seq))
        s -= sum(_trans(seq[t - 1], seq[t], lg[t - 1, seq[t - 1]], lg[t, seq[t]], oj, vu) for t in range(1, T))
        scored.append((s, seq))
    top = max(s for s, _ in scored)
    return top, [seq for s, seq in scored if abs(s - top) <= 1e-12]


def frame_argmax(cand_f0, cand_strength, f0_floor=71.0, voicing_threshold=0.45, octave_cost=0.02):
    """state [T] (c - 1, -1 unvoiced) of the per-frame argmax of u, ties to the smaller state: the path at zero costs."""
    ex, u, _ = _local(cand_f0, cand_strength, f0_floor, voicing_threshold, octave_cost)
    return (np.argmax(np.where(ex, u, -np.inf), axis=1) - 1).astype(np.int32)


def records(paths):
    """(rows [B, TERMS], batch [TERMS]): entry FLAGS of the batch counts the flagged utterances, MAX_STEP is the maximum and every
    other entry the sum over the unflagged ones, added in index order."""
    rows = np.stack([p.record for p in paths]) if len(paths) else np.zeros((0, TERMS))
    batch = np.zeros(TERMS)
    for r in rows:
        if r[FLAGS] != 0:
            batch[FLAGS] += 1.0
            continue
        for i in range(TERMS):
            if i == MAX_STEP:
                batch[i] = max(batch[i], r[i])
            elif i != FLAGS:
                batch[i] += r[i]
    return rows, batch


# ---- signals and counts ----
def gross_errors(f0, truth, n_fft, hop):
    """Interior frames that are unvoiced or more than 20 % off the truth -> (errors, interior frames)."""
    ok = P.interior(len(truth), n_fft, hop)
    f0 = np.asarray(f0, np.float64)
    bad = (f0 <= 0) | (np.abs(f0 / truth - 1.0) > 0.2)
    return int((bad & ok).sum()), int(ok.sum())


NOISY_F0 = (220, 440)
NOISY_LEVELS = (0.3, 0.5)


def noisy_signals(geom):
    """[(label, signal, truth, f0, noise)] of one geometry: const(f0, noise, n_hops=90, seed=7) for f0 in {220, 440} x noise in
    {0.3, 0.5}, and f0 = 110 at noise 0.3 where the geometry's lowest F0 allows it."""
    _, n_fft, hop, win, sr, opt, lo = geom
    out = []
    for f0, nz in [(f, n) for f in NOISY_F0 for n in NOISY_LEVELS] + [(110, 0.3)]:
        if f0 >= lo:
            sig, truth = P.const(f0, nz, sr, hop, n_hops=90, seed=7)
            out.append(("noisy_%g_%g" % (f0, nz), sig, truth, f0, nz))
    return out


def track(sig, geom, K=MAX_CANDS, **costs):
    """(Cands, Path) of one waveform in one geometry: the oracle's own candidates (rounded to float32, as the kernel hands them
    over) and its own path."""
    _, n_fft, hop, win, sr, opt, _ = geom
    o = dict(DEFAULTS, **opt)
    o.update(costs)
    c = candidates(np.asarray(sig, np.float64), n_fft, hop, win, sr, K=K, f0_floor=o["f0_floor"], f0_ceil=o.get("f0_ceil", 800.0),
                   octave_cost=o["octave_cost"])
    return c, path(c.f0.astype(np.float32), c.strength.astype(np.float32), hop / sr, o["f0_floor"], o["voicing_threshold"],
                   o["octave_cost"], o["octave_jump_cost"], o["voiced_unvoiced_cost"])


_cases = {}


def cases(geom):
    """[(label, [float32 waveforms], [Cands], [Path], truth or None)] of one geometry, computed once: P.packed_cases(geom) (three
    waveforms each) and the noisy signals (one waveform each, with its ground truth), at K = 8 and the default costs."""
    if geom[0] not in _cases:
        todo = [(label, waves, None) for label, waves in P.packed_cases(geom)]
        todo += [(label, [sig.astype(np.float32)], truth) for label, sig, truth, _, _ in noisy_signals(geom)]
        out = []
        for label, waves, truth in todo:
            res = [track(w, geom) for w in waves]
            out.append((label, waves, [r[0] for r in res], [r[1] for r in res], truth))
        _cases[geom[0]] = out
    return _cases[geom[0]]


def edge_lens(C):
    return [0, 1, 2, C - 1, C, C + 1, 2 * C + 3]


def synthetic_batch(C, K, seed=0):
    """The edge batch of the kernel tests: [(cand_f0 [T, K], cand_strength [T, K]) float32] with T over edge_lens(C), then one
    utterance with no candidate anywhere, one with all slots full, and one with a NaN candidate (each C + 1 frames).  Random slots are
    empty with probability 0.3 and some frames have none; frequencies 60 .. 700 Hz, strengths 0 .. 1."""
    rs = np.random.RandomState(1000 * K + seed)
    out = []

    def one(T, p_empty):
        f = rs.uniform(60.0, 700.0, (T, K)).astype(np.float32)
        p = rs.uniform(0.0, 1.0, (T, K)).astype(np.float32)
        gone = rs.uniform(size=(T, K)) < p_empty
        gone[rs.uniform(size=T) < 0.1] = True
        f[gone] = 0
        p[gone] = 0
        return f, p
    for T in edge_lens(C):
        out.append(one(T, 0.3))
    f, p = one(C + 1, 0.0)
    out.append((np.zeros_like(f), np.zeros_like(p)))
    out.append(one(C + 1, 0.0))
    out[-1][0][out[-1][0] == 0] = 123.0
    f, p = one(C + 1, 0.3)
    f[C // 2, K - 1] = np.nan
    out.append((f, p))
    return out


def boundary_batch(C, per_launch, K=2, seed=0):
    """per_launch + 1 utterances of 0 .. 3 frames, the last one of the first launch with C + 1 frames (one more than a chunk): the
    second launch's only utterance follows it in the workspace's words and in the records.  Same slots as synthetic_batch."""
    rs = np.random.RandomState(77 + seed)
    out = []
    for i in range(per_launch + 1):
        T = C + 1 if i == per_launch - 1 else (i + 1) % 4
        f = rs.uniform(60.0, 700.0, (T, K)).astype(np.float32)
        p = rs.uniform(0.0, 1.0, (T, K)).astype(np.float32)
        gone = rs.uniform(size=(T, K)) < 0.3
        f[gone] = 0
        p[gone] = 0
        out.append((f, p))
    return out
