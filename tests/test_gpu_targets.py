"""Target cleaning on the MI355X (fs2_op_clean_targets: fastspeech2_amd.targets) against the numpy oracle of the same definition
(tests/targets_oracle.py, itself held to the reference's recordings and to np.percentile in tests/test_targets_host.py).  The cleaned
values, the quartiles and the outlier counts are compared with equality (+0 and -0 equal, NaN positions equal): no tolerance, no
value left out.  The float64 statistics are held to 1e-9 relative, a bar that is derived, not measured: a reordered double sum of n
terms moves by at most n 2^-53 (1.1e-11 at n = 1e5), times the conditioning of the variance 1 + mean^2 / std^2 <= 101 on data with
mean <= 10 std.

Measured on an MI355X (the edge batch, n = 16,181 non-zero values): mean, std and M2 each 2.2e-16 relative from the oracle."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import targets_oracle as O

pytestmark = pytest.mark.gpu

STAGE = 4096          # csrc/targets.h: kTgStage, the keys of an utterance the kernel keeps in LDS; a longer one is re-read per sweep
F = np.float32


def _threshold_utterance(which):
    """An utterance holding a value exactly equal to its own ``upper`` (or ``lower``) threshold, on which a fused
    ``p75 + 1.5 iqr`` (``p25 - 1.5 iqr``) rounds to the float32 beyond the reference's two-step threshold: the reference flags the
    value, a kernel that contracts the threshold arithmetic does not.  Seeds are searched on the CPU for such an utterance; its
    largest (smallest) value is then replaced by the oracle's threshold, which leaves the quartiles (interior order statistics)
    where they were."""
    for seed in range(100000):
        x = np.random.default_rng([seed, 101]).normal(5.0, 1.0, 101).astype(F)
        q = O.quartiles(x)
        (lower, upper), (flower, fupper) = O.thresholds(*q), O.fused_thresholds(*q)
        if (fupper > upper) if which == "upper" else (flower < lower):
            break
    else:
        raise AssertionError("no utterance found whose fused %s threshold differs" % which)
    i = int(np.argmax(x)) if which == "upper" else int(np.argmin(x))
    x[i] = upper if which == "upper" else lower
    c = O.clean(x)
    assert O.thresholds(c.p25, c.p75) == (lower, upper) and O.fused_thresholds(c.p25, c.p75) == (flower, fupper)
    M = np.where((x <= lower) | (x >= upper), F(0), x).max()
    assert c.y[i] == M != x[i], "the value on the threshold must be flagged"
    assert not (x[i] >= fupper or x[i] <= flower), "a fused threshold must miss it"
    return x


def _edge_utterances():
    rng = np.random.default_rng(2024)
    u = []
    for n in range(10):                                           # every residue of (n - 1) mod 4, the one- and two-value cases, n = 0
        u.append(("n%d" % n, rng.normal(1.0, 2.0, n).astype(F)))
    for i, n in enumerate((63, 64, 65, 255, 256, 257, 1023, 1024, 1025)):
        u.append(("n%d" % n, O.KINDS[i % 3][1](rng, n)))
    u.append(("long", O.energy_like(rng, 3 * STAGE + 37)))        # beyond the LDS staging buffer
    u.append(("all_zero", np.zeros(50, F)))
    u.append(("constant", np.full(33, 2.5, F)))                   # everything is an outlier: all zero
    x = np.zeros(100, F)
    x[rng.choice(100, 20, replace=False)] = rng.uniform(1, 9, 20).astype(F)
    u.append(("zeros80", x))                                      # p25 == p75 == 0
    u.append(("ties", O.tie_heavy(rng, 300)))
    x = rng.normal(0.0, 1.0, 77).astype(F)
    x[5], x[9] = -0.0, 0.0
    u.append(("negative", x))
    one, two = F(1), F(2)
    x = np.asarray([0.5, one, np.nextafter(one, two), two, np.nextafter(two, F(3)), 3.0], F)      # s[1], s[2] and s[3], s[4]: one ulp
    u.append(("ulp", x[rng.permutation(6)]))
    u.append(("on_upper", _threshold_utterance("upper")))
    u.append(("on_lower", _threshold_utterance("lower")))
    x = O.energy_like(rng, 40)
    x[17] = np.nan
    u.append(("nan", x))
    x = O.f0_like(rng, 40)
    x[3] = np.inf
    u.append(("inf", x))
    return u


def _many_utterances():
    """501 utterances of 0 .. 3 values: one more than an upload launch of records holds (csrc/targets.h: kTgRecsPerChunk = 500).  Most
    are empty (the host stand-in runs a workgroup's 256 threads as threads); the ends of the batch and every 50th utterance are not."""
    rng = np.random.default_rng(501)
    return [("u%d" % i, rng.normal(1.0, 2.0, (i + 3) % 4 if i < 4 or i > 495 or i % 50 == 0 else 0).astype(F)) for i in range(501)]


class Edge:
    def __init__(self, named=None):
        self.named = _edge_utterances() if named is None else named
        self.names = [n for n, _ in self.named]
        self.utts = [x for _, x in self.named]
        self.lens = [x.size for x in self.utts]
        self.cleaned, self.stats = O.clean_batch(self.utts)
        self._x = None

    @property
    def x(self):
        if self._x is None:
            self._x = torch.from_numpy(np.concatenate(self.utts)).cuda()
        return self._x

    def oracle_y(self, order=None):
        order = range(len(self.utts)) if order is None else order
        return np.concatenate([self.cleaned[i].y for i in order])


@pytest.fixture(scope="module")
def edge():
    return Edge()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)          # (+0 == -0; NaN where NaN)


def _stats_close(s, o, rel=1e-9):
    assert tuple(s[:8]) == tuple(o[:8]), (s, o)                                   # counts, min, nonzero_min, max: exactly
    for a, b in zip(s[8:], o[8:]):                                                # mean, std, M2
        assert abs(a - b) <= rel * abs(b), (s, o)


def test_edge_batch_equals_the_oracle(edge):
    from fastspeech2_amd.targets import clean_targets, remove_outlier
    y, st, q, no = clean_targets(edge.x, edge.lens, return_quartiles=True)
    y, q, no = y.cpu().numpy(), q.cpu().numpy(), no.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(edge.lens)])
    for i, (name, c) in enumerate(zip(edge.names, edge.cleaned)):
        assert _same(y[off[i]:off[i + 1]], c.y), name
        assert _same(q[i], [c.p25, c.p75]), (name, q[i], c.p25, c.p75)
        assert no[i] == c.n_outliers, (name, no[i], c.n_outliers)
    assert y.dtype == np.float32 and not np.signbit(y[y == 0]).any()             # zeros are written as +0
    k = edge.names.index("constant")
    assert not y[off[k]:off[k + 1]].any() and no[k] == 33
    assert not y[off[edge.names.index("zeros80")]:off[edge.names.index("zeros80") + 1]].any()
    assert no[edge.names.index("long")] > 100 and no[edge.names.index("on_upper")] >= 1 and no[edge.names.index("on_lower")] >= 1
    assert st.n_nonfinite == 2 and st.n_total == sum(edge.lens) - 80
    assert _same(remove_outlier(edge.x, edge.lens).cpu().numpy(), y)


def test_more_utterances_than_an_upload_chunk():
    """Record 500 travels alone in a second upload launch: every utterance still finds its own (start, length)."""
    from fastspeech2_amd.targets import clean_targets
    many = Edge(_many_utterances())
    assert len(many.utts) == 501 and sorted(set(many.lens)) == [0, 1, 2, 3] and many.lens[500] == 3
    assert many.stats.mean <= 10 * many.stats.std
    y, st, q, no = clean_targets(many.x, many.lens, return_quartiles=True)
    y, q, no = y.cpu().numpy(), q.cpu().numpy(), no.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(many.lens)])
    for i, (name, c) in enumerate(zip(many.names, many.cleaned)):
        assert _same(y[off[i]:off[i + 1]], c.y), name
        assert _same(q[i], [c.p25, c.p75]), (name, q[i], c.p25, c.p75)
        assert no[i] == c.n_outliers, (name, no[i], c.n_outliers)
    _stats_close(st, many.stats)


def test_batch_invariance(edge):
    """An utterance alone, in the batch and in the reversed batch: the same bits."""
    from fastspeech2_amd.targets import clean_targets
    y, _, q, no = clean_targets(edge.x, edge.lens, return_quartiles=True)
    order = list(range(len(edge.utts)))[::-1]
    xr = torch.from_numpy(np.concatenate([edge.utts[i] for i in order])).cuda()
    yr, _, qr, nor = clean_targets(xr, [edge.lens[i] for i in order], return_quartiles=True)
    off = np.concatenate([[0], np.cumsum(edge.lens)])
    offr = np.concatenate([[0], np.cumsum([edge.lens[i] for i in order])])
    for name in ("n1025", "long", "ties"):
        i = edge.names.index(name)
        r = order.index(i)
        ya, _, qa, noa = clean_targets(torch.from_numpy(edge.utts[i]).cuda(), [edge.lens[i]], return_quartiles=True)
        for yy, qq, nn in ((y[off[i]:off[i + 1]], q[i], no[i]), (yr[offr[r]:offr[r + 1]], qr[r], nor[r])):
            assert torch.equal(ya, yy) and torch.equal(qa[0], qq) and int(noa[0]) == int(nn), name


def test_in_place(edge):
    from fastspeech2_amd.targets import clean_targets
    y, st = clean_targets(edge.x, edge.lens)
    x2 = edge.x.clone()
    y2, st2 = clean_targets(x2, edge.lens, out=x2)
    assert y2 is x2 and _same(y2.cpu().numpy(), y.cpu().numpy()) and st2 == st
    assert _same(y.cpu().numpy(), edge.oracle_y())


def test_golden_through_the_kernel(golden_dir):
    """The reference's own remove_outlier outputs (tests/golden/g12_targets.npz), all three kinds, exactly."""
    import os
    from fastspeech2_amd.targets import clean_targets
    g = np.load(os.path.join(golden_dir, "g12_targets.npz"))
    for kind, _ in O.KINDS:
        lens = g[kind + "/lens"].tolist()
        y, _, q, _ = clean_targets(torch.from_numpy(g[kind + "/x"]).cuda(), lens, return_quartiles=True)
        assert np.array_equal(y.cpu().numpy(), g[kind + "/y"]), kind
        assert np.array_equal(q.cpu().numpy(), np.stack([g[kind + "/p25"], g[kind + "/p75"]], 1)), kind


def test_statistics(edge):
    from fastspeech2_amd.targets import TargetStats, clean_targets
    o = edge.stats
    assert o.mean <= 10 * o.std and o.n <= 10 ** 5 and o.n_no_positive >= 3 and o.min < 0
    _, st = clean_targets(edge.x, edge.lens)
    print("gpu   ", st)
    print("oracle", o)
    _stats_close(st, o)
    assert abs(st.std - math.sqrt(st.M2 / st.n)) <= 1e-15 * st.std
    _, again = clean_targets(edge.x, edge.lens)
    assert again == st                                                            # the same bits on every call
    h = len(edge.utts) // 2
    n0 = sum(edge.lens[:h])
    _, a = clean_targets(edge.x[:n0].clone(), edge.lens[:h])
    _, b = clean_targets(edge.x[n0:].clone(), edge.lens[h:])
    _stats_close(TargetStats.merge(a, b), st, rel=1e-12)
    # a second set of data of another scale: F0-like, 64 utterances
    rng = np.random.default_rng(7)
    utts = [O.f0_like(rng, int(rng.integers(200, 900))) for _ in range(64)]
    _, o2 = O.clean_batch(utts)
    assert o2.mean <= 10 * o2.std
    _, s2 = clean_targets(torch.from_numpy(np.concatenate(utts)).cuda(), [u.size for u in utts])
    _stats_close(s2, o2)


def test_training_targets():
    from fastspeech2_amd.targets import clean_targets, remove_outlier, training_targets
    from fastspeech2_amd.vocoder import wav_features
    sr = 22050
    t = np.arange(16000) / sr
    tone = 0.4 * np.sin(2 * np.pi * np.cumsum(180.0 + 80.0 * t / t[-1]) / sr) * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * t))      # 180 -> 260 Hz
    tone[6000:10000] = 0.0                                                        # a silent stretch: unvoiced frames, energy 0
    noise = 0.1 * np.random.default_rng(3).normal(size=9000)
    wav = torch.from_numpy(np.concatenate([tone, noise]).astype(F)).cuda()
    lens = [16000, 9000]
    lm, en, f0 = wav_features(wav, lens)
    tt = training_targets(wav, lens)
    assert tt.frame_lens.tolist() == [16000 // 256 + 1, 9000 // 256 + 1] and en.numel() == int(tt.frame_lens.sum())
    assert torch.equal(tt.logmel, lm)
    assert torch.equal(tt.energy, remove_outlier(en, tt.frame_lens)) and torch.equal(tt.f0, remove_outlier(f0, tt.frame_lens))
    assert tt.energy_stats == clean_targets(en, tt.frame_lens)[1] and tt.pitch_stats == clean_targets(f0, tt.frame_lens)[1]
    silent = slice(6000 // 256 + 3, 10000 // 256 - 2)                            # frames wholly inside the silent stretch
    assert (f0[silent] == 0).all() and (tt.f0[silent] == 0).all() and (tt.f0[f0 == 0] == 0).all() and (tt.f0 > 0).any()
    assert (tt.energy[en == 0] == 0).all()
    assert tt.pitch_stats.n_total == en.numel() and tt.pitch_stats.n == int((tt.f0 != 0).sum())


def test_empty_batches():
    from fastspeech2_amd import _lib
    from fastspeech2_amd.targets import TargetStats, clean_targets
    e = torch.zeros(0, device="cuda")
    y, st = clean_targets(e, [])
    assert y.shape == (0,) and st == TargetStats.empty()
    y, st, q, no = clean_targets(e, [0, 0, 0], return_quartiles=True)
    assert y.shape == (0,) and st == TargetStats.empty() and q.shape == (3, 2) and torch.isnan(q).all() and not no.any()
    # the entry point itself: B = 0 with a statistics record, and a batch of empty utterances only
    lib = _lib.lib()
    rec = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.fs2_op_clean_targets(stream, None, 0, None, None, None, 0, None, None, None, rec.data_ptr()))
    assert TargetStats.from_record(rec.cpu().tolist()) == TargetStats.empty()
    z = (C.c_int32 * 3)(0, 0, 0)
    nb = int(lib.fs2_op_targets_workspace_bytes(3))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rec.fill_(7.0)
    _lib.check(lib.fs2_op_clean_targets(stream, None, 3, z, z, ws.data_ptr(), nb, None, None, None, rec.data_ptr()))
    assert TargetStats.from_record(rec.cpu().tolist()) == TargetStats.empty()
    assert lib.fs2_op_targets_workspace_bytes(-1) == 0
    assert lib.fs2_op_clean_targets(stream, None, 3, z, z, ws.data_ptr(), nb - 1, None, None, None, None) != 0      # workspace too small
