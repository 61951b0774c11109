"""CPU: the numpy oracle of the target cleaning (tests/targets_oracle.py) against what the reference's own remove_outlier and
compute_statistics.py recorded (tests/golden/g12_targets.npz, tools/gen_golden_targets.py) and against np.percentile; the host side
of fastspeech2_amd.targets (TargetStats.merge, hp_data, the checks made before the library is loaded)."""
import math

import numpy as np
import pytest
import torch

from fastspeech2_amd import targets          # the feature under test: without it this file fails at import
from fastspeech2_amd.targets import TargetStats, hp_data
from tests import targets_oracle as O

KINDS = [k for k, _ in O.KINDS]

# |recorded / oracle - 1| of the reference's float32 mean and std (compute_statistics.py: np.mean / np.std of the float32
# concatenation, saved as float32) from the float64 oracle, measured on the CPU that recorded the fixture; the test holds the
# comparison to 10x these.
MEASURED_REL = {"energy": (1.129e-09, 1.632e-08), "f0": (8.141e-08, 1.224e-08), "ties": (1.094e-08, 1.083e-07)}


@pytest.fixture(scope="module")
def g12(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "g12_targets.npz"))


def _utterances(g, kind, key="x"):
    lens = g[kind + "/lens"]
    o = np.concatenate([[0], np.cumsum(lens)])
    return [g[kind + "/" + key][o[i]:o[i + 1]] for i in range(len(lens))]


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_the_reference_recordings(g12, kind):
    xs, ys = _utterances(g12, kind), _utterances(g12, kind, "y")
    assert len(xs) == 16 and {1, 2, 3, 4, 5, 400} <= {x.size for x in xs}
    changed = 0
    for i, (x, y) in enumerate(zip(xs, ys)):
        c = O.clean(x)
        assert c.y.dtype == np.float32 and np.array_equal(c.y, y), (kind, i)
        assert c.p25 == g12[kind + "/p25"][i] and c.p75 == g12[kind + "/p75"][i], (kind, i)
        changed += int((x != y).sum())
    assert changed > 20, changed          # the recordings do exercise the replacement


def _percentile_cases():
    rng = np.random.default_rng(5)
    for n in list(range(1, 41)) + [255, 256, 257, 1023, 1024, 1025]:
        yield n, "normal", rng.normal(0, 3, n).astype(np.float32)
        yield n, "energy", O.energy_like(rng, n)
        yield n, "f0", O.f0_like(rng, n)
        yield n, "ties", O.tie_heavy(rng, n)
        yield n, "two_values", rng.choice(np.asarray([-1.5, 2.25], np.float32), n)


def test_oracle_quartiles_equal_numpy_percentile():
    """p25 / p75 of the restatement equal np.percentile's bits for every n in 1 .. 40 and around 256 and 1024, ties included.
    (np.percentile of float32 data interpolates in float32 since numpy 2.0; the fixture records which numpy pinned it.)"""
    n_cases = 0
    for n, label, x in _percentile_cases():
        p25, p75 = O.quartiles(x)
        assert p25 == np.percentile(x, 25) and p75 == np.percentile(x, 75), (n, label)
        assert np.percentile(x, 25).dtype == np.float32
        n_cases += 1
    assert n_cases == 46 * 5


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_statistics_against_compute_statistics(g12, kind):
    """The reference script's printed minima / maxima are equal to the oracle's; its float32 mean and std are within 10x the distance
    measured when the fixture was recorded (MEASURED_REL: energy 1.129e-09 / 1.632e-08, f0 8.141e-08 / 1.224e-08, ties 1.094e-08 /
    1.083e-07 for mean / std -- float32 rounding of the saved value and of np.mean's float32 pairwise sum)."""
    xs = _utterances(g12, kind)
    _, s = O.clean_batch([xs[i] for i in g12[kind + "/stats_index"]])
    assert s.nonzero_min == float(g12[kind + "/stats_nonzero_min"]) and s.max == float(g12[kind + "/stats_max"])
    if kind != "energy":
        assert s.min == float(g12[kind + "/stats_min"]) and s.n_no_positive == int(g12[kind + "/stats_bad"]) > 0
    rel_mean = abs(float(g12[kind + "/stats_mean"]) / s.mean - 1.0)
    rel_std = abs(float(g12[kind + "/stats_std"]) / s.std - 1.0)
    print("%s: mean rel %.3e, std rel %.3e" % (kind, rel_mean, rel_std))
    assert rel_mean <= 10 * MEASURED_REL[kind][0] and rel_std <= 10 * MEASURED_REL[kind][1]
    assert s.n_nonfinite == 0 and s.n_total == sum(xs[i].size for i in g12[kind + "/stats_index"])


def test_oracle_edge_cases():
    c = O.clean(np.full(7, 3.5, np.float32))                     # p25 == p75: everything is an outlier, all zero
    assert c.n_outliers == 7 and not c.y.any()
    x = np.asarray([1, 2, np.nan, 4], np.float32)
    c = O.clean(x)
    assert not c.finite and np.array_equal(c.y, x, equal_nan=True) and math.isnan(c.p25) and c.n_outliers == 0
    c, s = O.clean_batch([x, np.zeros(0, np.float32), np.asarray([np.inf], np.float32)])
    assert s.n_nonfinite == 2 and s.n_total == 0 and s.n == 0 and s.nonzero_min == math.inf


@pytest.mark.parametrize("which", ["upper", "lower"])
def test_threshold_tie_utterances_tell_a_fused_threshold_apart(which):
    """The GPU test's on_upper / on_lower utterances: the reference flags the value on the threshold, a fused
    ``p +- 1.5 iqr`` (one rounding) does not."""
    from tests.test_gpu_targets import _threshold_utterance
    x = _threshold_utterance(which)
    c = O.clean(x)
    lower, upper = O.thresholds(c.p25, c.p75)
    flower, fupper = O.fused_thresholds(c.p25, c.p75)
    i = int(np.argmax(x)) if which == "upper" else int(np.argmin(x))
    assert x[i] == (upper if which == "upper" else lower) and c.y[i] != x[i]
    assert (fupper > upper) if which == "upper" else (flower < lower)
    fused_flags = int(((x <= flower) | (x >= fupper)).sum())
    assert fused_flags == c.n_outliers - 1


def _as_target_stats(s):
    return TargetStats(*s)


@pytest.fixture(scope="module")
def forty():
    rng = np.random.default_rng(40)
    utts = [O.KINDS[i % 3][1](rng, int(rng.integers(1, 300))) for i in range(40)]
    utts[7] = np.asarray([1.0, np.nan], np.float32)
    utts[11] = np.zeros(0, np.float32)
    return utts


@pytest.mark.parametrize("parts", [2, 3, 7])
def test_target_stats_merge(forty, parts):
    """Oracle statistics of the parts of a 40-utterance batch merge to those of the whole: counts and extrema exactly, mean, std
    and M2 within 1e-12 relative, for several splits and both merge orders; empty() is the identity."""
    whole = _as_target_stats(O.clean_batch(forty)[1])
    assert whole.n_nonfinite == 1 and whole.n > 1000
    rng = np.random.default_rng(parts)
    for trial in range(4):
        cuts = [0] + sorted(int(v) for v in rng.choice(np.arange(1, 40), parts - 1, replace=False)) + [40]
        pieces = [_as_target_stats(O.clean_batch(forty[a:b])[1]) for a, b in zip(cuts[:-1], cuts[1:])]
        if trial % 2:
            pieces.reverse()
        m = TargetStats.empty()
        for p in pieces:
            m = TargetStats.merge(m, p)
        assert m[:8] == whole[:8], (cuts, m, whole)
        for a, b in zip(m[8:], whole[8:]):
            assert abs(a / b - 1.0) <= 1e-12, (cuts, m, whole)
    e = TargetStats.empty()
    assert TargetStats.merge(e, whole) == whole and TargetStats.merge(whole, e) == whole and TargetStats.merge(e, e) == e
    assert e.n_total == 0 and e.min == math.inf and e.max == -math.inf and e.nonzero_min == math.inf and e.std == 0.0


def test_hp_data_maps_and_raises(forty):
    rng = np.random.default_rng(1)
    es = _as_target_stats(O.clean_batch([O.energy_like(rng, 200) for _ in range(5)])[1])
    ps = _as_target_stats(O.clean_batch([O.f0_like(rng, 200) for _ in range(5)])[1])
    d = hp_data(es, ps)
    assert d == dict(e_min=es.nonzero_min, e_max=es.max, p_min=ps.nonzero_min, p_max=ps.max, e_mean=es.mean, e_std=es.std,
                     f0_mean=ps.mean, f0_std=ps.std)
    assert 0 < d["e_min"] < d["e_max"] and ps.min == 0.0 < d["p_min"] < d["p_max"]
    with pytest.raises(ValueError, match="pitch statistics hold no positive value"):
        hp_data(es, TargetStats.empty())
    with pytest.raises(ValueError, match="energy statistics hold no positive value"):
        hp_data(_as_target_stats(O.clean_batch([np.zeros(9, np.float32)])[1]), ps)


def test_entry_points_refuse_before_loading_the_library(monkeypatch):
    from fastspeech2_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", no_library)
    x = torch.zeros(10)
    for call in (lambda: targets.clean_targets(x, [10]), lambda: targets.remove_outlier(x, [4, 6]),
                 lambda: targets.training_targets(torch.zeros(4096), [4096])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        targets.clean_targets([0.0] * 10, [10])
    if torch.cuda.is_available():
        xg = torch.zeros(10, device="cuda")
        with pytest.raises(ValueError, match="lens sum to 9"):
            targets.clean_targets(xg, [4, 5])
        with pytest.raises(ValueError, match=">= 0"):
            targets.clean_targets(xg, [12, -2])
        with pytest.raises(TypeError, match="float32"):
            targets.clean_targets(xg.double(), [10])
    else:
        # without a GPU a cuda tensor cannot exist: the length checks behind the device check, on their own
        monkeypatch.setattr(targets, "_require_cuda", lambda *a: None)
        with pytest.raises(ValueError, match="lens sum to 9"):
            targets.clean_targets(x, [4, 5])
        with pytest.raises(ValueError, match=">= 0"):
            targets.clean_targets(x, [12, -2])
        with pytest.raises(ValueError, match="1-D"):
            targets.clean_targets(x.reshape(2, 5), [10])
