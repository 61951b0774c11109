"""Numpy restatement of the training-target cleaning of fastspeech2_amd.targets (csrc/targets.h: tg_clean, tg_combine): the
reference's remove_outlier (utils/util.py:26-49) in float32, operation by operation, and the corpus statistics of its
compute_statistics.py in float64.  It imports nothing of the reference; tests/golden/g12_targets.npz holds what the reference's own
function returned, and tests/test_targets_host.py holds this file to it with np.array_equal.

For one utterance x (float32, n >= 1 values), every operation rounded to float32 on its own:
  s = sort(x); for q in {1, 3}: h = q (n - 1), j = h div 4, g = (h mod 4) / 4, a = s[j], b = s[min(j + 1, n - 1)], d = b - a,
  p = a + d g if g < 0.5 else b - d (1 - g)                  (numpy's _lerp; g and 1 - g are exact): p25, p75
  iqr = p75 - p25, w = 1.5 iqr, lower = p25 - w, upper = p75 + w; x[i] is an outlier iff x[i] <= lower or x[i] >= upper
  M = max_i (0 if outlier_i else x[i]);  y[i] = 0 if x[i] == 0 else M if outlier_i else x[i]
(p25 == p75 makes every value an outlier and the utterance all zero: the reference's behaviour.)  An utterance with a NaN or an
infinity is copied unchanged, its quartiles are NaN and its outlier count 0; it is left out of the statistics and counted in
n_nonfinite.  An utterance of 0 values produces nothing (quartiles NaN, count 0).
Test infrastructure only (host tests and GPU tests compare against it)."""
from typing import NamedTuple

import numpy as np

F = np.float32


def quartiles(x):
    """(p25, p75) of a finite float32 array of n >= 1 values, as np.percentile(x, 25 / 75) gives them under numpy 2.x."""
    s = np.sort(np.asarray(x, F))
    n = s.size
    out = []
    for q in (1, 3):
        h = q * (n - 1)
        j, g = h // 4, F((h % 4) / 4.0)
        a, b = s[j], s[min(j + 1, n - 1)]
        with np.errstate(over="ignore", invalid="ignore"):
            d = F(b - a)
            out.append(F(a + F(d * g)) if g < 0.5 else F(b - F(d * F(F(1) - g))))
    return out[0], out[1]


def thresholds(p25, p75):
    with np.errstate(over="ignore", invalid="ignore"):
        w = F(F(1.5) * F(p75 - p25))
        return F(p25 - w), F(p75 + w)


def fused_thresholds(p25, p75):
    """What a fused multiply-add makes of the thresholds: lower = fma(iqr, -1.5, p25), upper = fma(iqr, 1.5, p75), one rounding
    where ``thresholds`` has two (1.5 iqr is exact in float64, and so is the sum before its rounding, up to a double rounding that
    the callers' strict inequalities do not depend on).  NOT the semantics: tests use it to build utterances on which a kernel
    that contracts the threshold arithmetic gives another answer than the reference."""
    iqr = np.float64(F(p75 - p25))
    return F(np.float64(p25) - 1.5 * iqr), F(np.float64(p75) + 1.5 * iqr)


class Cleaned(NamedTuple):
    y: np.ndarray           # [n] float32
    p25: np.float32
    p75: np.float32
    n_outliers: int
    finite: bool


def clean(x):
    """remove_outlier of one utterance."""
    x = np.asarray(x, F)
    if x.size == 0 or not np.isfinite(x).all():
        return Cleaned(x.copy(), F(np.nan), F(np.nan), 0, bool(x.size == 0 or np.isfinite(x).all()))
    p25, p75 = quartiles(x)
    lower, upper = thresholds(p25, p75)
    with np.errstate(invalid="ignore"):
        out = (x <= lower) | (x >= upper)
    M = np.where(out, F(0), x).max()
    y = np.where(x == 0, F(0), np.where(out, M, x)).astype(F)
    return Cleaned(y, p25, p75, int(out.sum()), True)


class Stats(NamedTuple):
    """The fields of fastspeech2_amd.targets.TargetStats, in its order."""
    n_total: int
    n_outliers: int
    n_nonfinite: int
    n_no_positive: int
    n: int
    min: float
    nonzero_min: float
    max: float
    mean: float
    std: float
    M2: float


def statistics(cleaned):
    """Statistics of a batch (a list of Cleaned) over the cleaned values of its finite utterances: float64, plain numpy on the
    concatenation."""
    fin = [c for c in cleaned if c.finite and c.y.size]
    n_nonfinite = sum(1 for c in cleaned if not c.finite)
    if not fin:
        return Stats(0, 0, n_nonfinite, 0, 0, float("inf"), float("inf"), float("-inf"), 0.0, 0.0, 0.0)
    y = np.concatenate([c.y for c in fin]).astype(np.float64)
    nz = y[y != 0]
    pos = y[y > 0]
    mean = float(nz.mean()) if nz.size else 0.0
    M2 = float(((nz - mean) ** 2).sum()) if nz.size else 0.0
    return Stats(n_total=int(y.size), n_outliers=sum(c.n_outliers for c in fin), n_nonfinite=n_nonfinite,
                 n_no_positive=sum(1 for c in fin if not (c.y > 0).any()), n=int(nz.size), min=float(y.min()),
                 nonzero_min=float(pos.min()) if pos.size else float("inf"), max=float(y.max()), mean=mean,
                 std=float(np.sqrt(M2 / nz.size)) if nz.size else 0.0, M2=M2)


def clean_batch(utterances):
    """([Cleaned per utterance], Stats) of a list of float32 arrays."""
    c = [clean(u) for u in utterances]
    return c, statistics(c)


# ---- seeded synthetic utterances (the kinds of tests/golden/g12_targets.npz and of the GPU tests) ----
def energy_like(rng, n):
    """Positive, a few per cent of near-silent frames and a few loud spikes."""
    x = rng.lognormal(2.0, 0.6, n)
    x[rng.random(n) < 0.05] *= 0.01
    x[rng.random(n) < 0.03] *= 8.0
    return x.astype(F)


def f0_like(rng, n):
    """12 .. 48 % unvoiced zeros (30 % on average, so p25 is zero in some utterances and not in others), a slowly moving contour,
    octave-jump spikes."""
    t = np.arange(n)
    x = 180.0 + 40.0 * np.sin(2 * np.pi * t / 97.0 + rng.uniform(0, 6.28)) + rng.normal(0, 6.0, n)
    x[rng.random(n) < 0.04] *= 2.0
    x[rng.random(n) < 0.02] *= 0.5
    x[rng.random(n) < rng.uniform(0.1, 0.4) * 1.2] = 0.0
    return x.astype(F)


def tie_heavy(rng, n):
    """Small integers with a few larger ones: the quartile neighbours and the (integer or half-integer) thresholds tie with values."""
    x = rng.integers(0, int(rng.integers(2, 12)), n)
    x[rng.random(n) < 0.06] += rng.integers(3, 30)
    return x.astype(F)


KINDS = (("energy", energy_like), ("f0", f0_like), ("ties", tie_heavy))
