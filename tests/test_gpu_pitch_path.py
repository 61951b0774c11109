"""The pitch path search on the MI355X (fastspeech2_amd.vocoder: pitch_candidates, pitch_path, pitch_track, wav_features(...,
f0_method="path"); csrc/gl_pitch.h: gl_candidates; csrc/pitch_path.h) against the float64 oracle of the same definition
(tests/pitch_path_oracle.py, itself held to a brute-force search and to ground truth in tests/test_pitch_path_host.py).

Candidates are compared by VALUE, never as sets of integer lags: a true period between two lags makes either of them "the" candidate
on the last bit, and float32 noise creates and removes flat local maxima.  The path kernel is compared EXACTLY, on the kernel's own
candidates.  All waveforms of a geometry (its packed cases and the noisy signals) go through one call.

Measured on an MI355X (this file), the largest difference between a prominent candidate of the oracle and its match in the kernel's
list, f0 relative / strength absolute: 1024_256_1024 1.029e-06 / 3.704e-07, 2048_300_1200 1.076e-06 / 3.592e-07, 1024_200_800
1.598e-06 / 2.644e-05, 512_160_400 9.875e-07 / 7.232e-07 (17,492 / 17,492 / 17,536 / 12,373 candidates held); each geometry is held
to 10x its value (TOL_F, TOL_P), all far below the 1e-3 the requirement started from.  On the same run: S never rose along a row,
the path kernel equalled the oracle on the kernel's own candidates in every case, no frame of any case was off the pure oracle's
track, and pitch_track left 0 gross errors on every noisy signal where pitch left 10 to 55."""
import numpy as np
import pytest
import torch

from tests import pitch_oracle as P
from tests import pitch_path_oracle as Q
from tests.test_pitch_path_kernel_host import COSTS, assert_records, chunk, utts_per_launch

pytestmark = pytest.mark.gpu

GEOM_IDS = [g[0] for g in P.GEOMS]
K = Q.MAX_CANDS
CAP = 1e-3      # the requirement section 14.3 of DESIGN.md started from: no tolerance below is wider
# the largest difference of a prominent oracle candidate to its match in the kernel's list: 10x the value measured on an MI355X
TOL_F = {"1024_256_1024": 1.03e-5, "2048_300_1200": 1.08e-5, "1024_200_800": 1.6e-5, "512_160_400": 9.9e-6}
TOL_P = {"1024_256_1024": 3.7e-6, "2048_300_1200": 3.6e-6, "1024_200_800": 2.65e-4, "512_160_400": 7.3e-6}
assert max(max(TOL_F.values()), max(TOL_P.values())) <= CAP
S_MARGIN = 1e-4     # with a full list, only oracle candidates this far above the kernel's last slot must be in it
# S recomputed in double from a slot's float32 f0 and strength against the kernel's own float32 S: |S| < 2, so an ulp is 1.2e-7; the
# kernel rounds log2f (2 ulp of a value below 4, times octave_cost), the product and the difference, and sr / t* and p are rounded
# once more on the way out: below 4e-7 per slot, 1e-6 for a pair of slots
S_SORTED = 1e-6


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


def _hp(geom):
    from fastspeech2_amd.hparams import DotDict
    _, n_fft, hop, win, sr, _, _ = geom
    return DotDict({"audio": {"sample_rate": sr, "n_fft": n_fft, "hop_length": hop, "win_length": win, "num_mels": 80}})


def _opt(geom, *names):
    o = dict(Q.DEFAULTS, f0_ceil=800.0, **geom[5])
    return {k: o[k] for k in names}


class Dev:
    """One geometry on the device, computed once: every waveform of Q.cases(geom) packed into one batch, the kernel's candidates
    (K = 8), and per waveform its rows."""

    def __init__(self, geom):
        from fastspeech2_amd.vocoder import pitch_candidates
        self.geom = geom
        _, n_fft, hop, win, sr, opt, _ = geom
        self.hp, self.hop, self.time_step = _hp(geom), hop, hop / sr
        self.cases = Q.cases(geom)
        self.waves = [w for _, waves, _, _, _ in self.cases for w in waves]
        self.case_of = [i for i, (_, waves, _, _, _) in enumerate(self.cases) for _ in waves]
        self.oracle_cands = [c for _, _, cands, _, _ in self.cases for c in cands]
        self.oracle_paths = [p for _, _, _, paths, _ in self.cases for p in paths]
        self.lens = [len(w) for w in self.waves]
        self.frame_lens = np.asarray([n // hop + 1 for n in self.lens])
        self.starts = np.concatenate([[0], np.cumsum(self.frame_lens)[:-1]])
        self.x = torch.from_numpy(np.concatenate(self.waves)).cuda()
        self.cf, self.cs = pitch_candidates(self.x, self.lens, hp=self.hp, n_candidates=K, **_opt(geom, "f0_floor", "f0_ceil", "octave_cost"))
        self.cf_np, self.cs_np = self.cf.cpu().numpy(), self.cs.cpu().numpy()

    def rows(self, i):
        return slice(int(self.starts[i]), int(self.starts[i] + self.frame_lens[i]))

    def wave_index(self, label, which=0):
        return [i for i, c in enumerate(self.case_of) if self.cases[c][0] == label][which]


_dev = {}


def dev(geom):
    if geom[0] not in _dev:
        _dev[geom[0]] = Dev(geom)
    return _dev[geom[0]]


def _path(d, cf, cs, frame_lens, costs):
    from fastspeech2_amd.vocoder import pitch_path
    return pitch_path(cf, cs, frame_lens, d.time_step, **costs)


def _assert_track_equals_oracle(track, cf_np, cs_np, frame_lens, time_step, costs, label):
    """pitch_path's outputs against the float64 oracle run on the same float32 candidates, utterance by utterance."""
    f0, state, strength = track.f0.cpu().numpy(), track.state.cpu().numpy(), track.strength.cpu().numpy()
    want, r = [], 0
    for n in frame_lens:
        w = Q.path(cf_np[r:r + n], cs_np[r:r + n], time_step, **costs)
        assert np.array_equal(state[r:r + n], w.state), (label, len(want))
        assert np.array_equal(f0[r:r + n].view(np.uint32), w.f0.view(np.uint32)) and np.array_equal(strength[r:r + n].view(np.uint32), w.strength.view(np.uint32))
        want.append(w)
        r += n
    rows, batch = Q.records(want)
    assert_records(track.terms, rows)
    assert_records(track.batch, batch)
    return want


# ---- 1. slot 0 and the parent's bits ----
@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_slot_0_and_parent_bits(geom):
    from fastspeech2_amd.vocoder import mel_energy, pitch, pitch_candidates, wav_features
    d = dev(geom)
    f0, st = pitch(d.x, d.lens, hp=d.hp, return_strength=True, **geom[5])
    assert d.cf.shape == d.cs.shape == (f0.numel(), K) and d.cf.dtype == d.cs.dtype == torch.float32
    assert torch.equal(d.cs[:, 0], st)
    voiced = f0 != 0
    assert voiced.sum() > 1000 and torch.equal(d.cf[:, 0][voiced], f0[voiced])
    lm, en, _ = wav_features(d.x, d.lens, hp=d.hp, f0_method="path", **geom[5])
    lm0, en0 = mel_energy(d.x, d.lens, hp=d.hp)
    assert torch.equal(lm, lm0) and torch.equal(en, en0)
    for k in (1, 3):                                                # fewer slots: the first slots of the full list
        cf, cs = pitch_candidates(d.x, d.lens, hp=d.hp, n_candidates=k, **_opt(geom, "f0_floor", "f0_ceil", "octave_cost"))
        assert torch.equal(cf, d.cf[:, :k]) and torch.equal(cs, d.cs[:, :k])
    S = Q.score(d.cf_np, d.cs_np, **_opt(geom, "f0_floor", "octave_cost"))
    has = d.cf_np > 0
    assert np.isfinite(d.cf_np).all() and np.isfinite(d.cs_np).all() and (d.cf_np >= 0).all()
    assert not (has[:, 1:] & ~has[:, :-1]).any()                   # empty slots come last
    assert (d.cs_np[~has] == 0).all()
    both = has[:, 1:] & has[:, :-1]
    rise = (np.where(both, S[:, 1:], 0.0) - np.where(both, S[:, :-1], 0.0))[both]
    print(geom[0], "slots %d of %d full, largest rise of S along a row %.3e" % (has.sum(), has.size, rise.max()))
    assert rise.max() <= S_SORTED


# ---- 2. candidates against the oracle, by value ----
@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_candidates_against_the_oracle(geom):
    name, n_fft, hop, win, sr, opt, _ = geom
    d = dev(geom)
    o = _opt(geom, "f0_floor", "octave_cost")
    worst_f = worst_p = 0.0
    n_prom = n_held = n_kernel = 0
    for i, c in enumerate(d.oracle_cands):
        kf, kp = d.cf_np[d.rows(i)].astype(np.float64), d.cs_np[d.rows(i)].astype(np.float64)
        khas = kf > 0
        # completeness: every prominent oracle candidate (above the last slot by S_MARGIN where the kernel's list is full) has a match
        kS = Q.score(kf, kp, **o)
        full = khas[:, -1]
        held = c.prominent & (~full[:, None] | (c.S >= (kS[:, -1] + S_MARGIN)[:, None]))
        with np.errstate(divide="ignore", invalid="ignore"):
            df = np.where(khas[:, None, :], np.abs(kf[:, None, :] / np.where(c.f0 > 0, c.f0, 1.0)[:, :, None] - 1.0), np.inf)      # [frame, oracle slot, kernel slot]
        match = np.argmin(df, axis=2)
        rows = np.arange(len(kf))[:, None]
        mf = df[rows, np.arange(K)[None, :], match]
        mp = np.abs(kp[rows, match] - c.strength)
        n_prom += int(c.prominent.sum())
        n_held += int(held.sum())
        if held.any():
            worst_f, worst_p = max(worst_f, mf[held].max()), max(worst_p, mp[held].max())
        assert (mf[held] <= TOL_F[name]).all() and (mp[held] <= TOL_P[name]).all(), (i, mf[held].max(), mp[held].max())
        # soundness: every kernel candidate lies within one sample of a relaxed local maximum of the oracle's rho
        rho = c.rho
        relaxed = np.zeros(rho.shape, bool)
        relaxed[:, 1:-1] = (rho[:, 1:-1] > rho[:, :-2] - 1e-4) & (rho[:, 1:-1] >= rho[:, 2:] - 1e-4) & (rho[:, 1:-1] > -1e-4)
        tau = sr / np.where(khas, kf, 1.0)
        sound = np.zeros(kf.shape, bool)
        for lag in (np.ceil(tau - 1.0), np.ceil(tau - 1.0) + 1, np.floor(tau + 1.0)):
            idx = lag.astype(np.int64) - (c.tmin - 1)
            inside = (idx >= 0) & (idx < rho.shape[1]) & (np.abs(lag - tau) <= 1.0)
            sound |= inside & relaxed[rows, np.clip(idx, 0, rho.shape[1] - 1)]
        n_kernel += int(khas.sum())
        assert sound[khas].all(), (i, np.argwhere(khas & ~sound)[:5])
    print("%s: %d prominent oracle candidates, %d held, %d kernel candidates; worst f0 rel %.3e, strength abs %.3e" % (name, n_prom, n_held, n_kernel, worst_f, worst_p))
    _record("pitch_path_%s_cand_f0_rel" % name, worst_f)
    _record("pitch_path_%s_cand_strength_abs" % name, worst_p)
    assert n_held >= 0.9 * n_prom and n_held > 5000


# ---- 3. the path kernel, exactly ----
@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_path_kernel_equals_the_oracle_on_its_own_candidates(geom):
    d = dev(geom)
    o = _opt(geom, "f0_floor")
    for which, costs in COSTS.items():
        costs = dict(costs, **(o if which != "second" else {}))
        track = _path(d, d.cf, d.cs, d.frame_lens, costs)
        want = _assert_track_equals_oracle(track, d.cf_np, d.cs_np, d.frame_lens, d.time_step, costs, which)
        if which == "zero":                                          # the per-frame argmax of u, exactly
            arg = np.concatenate([Q.frame_argmax(d.cf_np[d.rows(i)], d.cs_np[d.rows(i)], costs["f0_floor"], costs["voicing_threshold"], costs["octave_cost"])
                                  for i in range(len(d.waves))])
            assert np.array_equal(track.state.cpu().numpy(), arg) and track.batch[Q.CHANGED] == 0
        elif which == "default":                                     # the path does decide frames: the table's signals have 10 or more each
            assert sum(w.record[Q.CHANGED] for w in want) >= 10
        # (condition (b) of tests/test_pitch_path_host.py, here on the kernel's own candidates: what keeps a last bit of log2 harmless)
        print(geom[0], which, "smallest relative gap between a cell's two best predecessors %.3g" % min(w.gap for w in want))
    some = list(range(0, len(d.waves), 4)) + [d.wave_index(c[0]) for c in d.cases if c[4] is not None]
    for k in (1, 3):
        cf = torch.cat([d.cf[d.rows(i), :k] for i in some]).contiguous()
        cs = torch.cat([d.cs[d.rows(i), :k] for i in some]).contiguous()
        costs = dict(COSTS["default"], **o)
        _assert_track_equals_oracle(_path(d, cf, cs, d.frame_lens[some], costs), cf.cpu().numpy(), cs.cpu().numpy(), d.frame_lens[some], d.time_step, costs, k)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_path_kernel_on_the_edge_lengths(k):
    from fastspeech2_amd.vocoder import pitch_path
    utts = Q.synthetic_batch(chunk(), k)
    lens = np.asarray([len(f) for f, _ in utts])
    cf_np, cs_np = np.concatenate([f for f, _ in utts]), np.concatenate([p for _, p in utts])
    cf, cs = torch.from_numpy(cf_np).cuda(), torch.from_numpy(cs_np).cuda()
    ts = 256 / 22050
    for costs in COSTS.values():
        track = pitch_path(cf, cs, lens, ts, **costs)
        want = _assert_track_equals_oracle(track, cf_np, cs_np, lens, ts, costs, k)
        assert [int(w.record[Q.FLAGS]) for w in want] == [0] * 9 + [2] and track.per_utterance()["flags"].tolist() == [0] * 9 + [2]
        assert track.batch[Q.FLAGS] == 1 and track.batch[Q.N_FRAMES] == lens[:-1].sum()


def test_more_utterances_than_one_launch_holds():
    """129 utterances at K = 2: the last one travels with a second launch, behind an utterance one frame longer than a chunk."""
    from fastspeech2_amd.vocoder import pitch_path
    utts = Q.boundary_batch(chunk(), utts_per_launch())
    lens = np.asarray([len(f) for f, _ in utts])
    assert len(utts) == 129 and lens[127] == 65 and lens[128] > 0 and np.delete(lens, 127).max() == 3
    cf_np, cs_np = np.concatenate([f for f, _ in utts]), np.concatenate([p for _, p in utts])
    ts = 256 / 22050
    track = pitch_path(torch.from_numpy(cf_np).cuda(), torch.from_numpy(cs_np).cuda(), lens, ts, **COSTS["default"])
    _assert_track_equals_oracle(track, cf_np, cs_np, lens, ts, COSTS["default"], "boundary")
    assert track.batch[Q.FLAGS] == 0 and track.batch[Q.N_FRAMES] == lens.sum()


# ---- 4. end to end against the pure oracle ----
@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_end_to_end_against_the_pure_oracle(geom):
    from fastspeech2_amd.vocoder import pitch_track
    name = geom[0]
    d = dev(geom)
    track = pitch_track(d.x, d.lens, hp=d.hp, **geom[5])
    f0 = track.f0.cpu().numpy().astype(np.float64)
    worst = 0
    for c, (label, waves, _, _, _) in enumerate(d.cases):
        off = frames = 0
        for i in [i for i, cc in enumerate(d.case_of) if cc == c]:
            got, want = f0[d.rows(i)], d.oracle_paths[i].f0.astype(np.float64)
            v = (got > 0) & (want > 0)
            bad = (got > 0) != (want > 0)
            bad[v] |= np.abs(got[v] / want[v] - 1.0) > TOL_F[name]
            off, frames = off + int(bad.sum()), frames + len(got)
        worst = max(worst, off)
        assert off <= max(1, frames // 100), (label, off, frames)
    print(name, "most frames of a case off the pure oracle's track:", worst)
    _record("pitch_path_%s_track_frames_off" % name, worst)


# ---- 5. ground truth on the device ----
@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_ground_truth_on_the_device(geom):
    from fastspeech2_amd.vocoder import pitch, pitch_track
    name, n_fft, hop, win, sr, opt, _ = geom
    d = dev(geom)
    tracked = pitch_track(d.x, d.lens, hp=d.hp, **opt).f0.cpu().numpy()
    framewise = pitch(d.x, d.lens, hp=d.hp, **opt).cpu().numpy()
    for label, _, _, _, truth in d.cases:
        if truth is None:
            continue
        r = d.rows(d.wave_index(label))
        e_path, n = Q.gross_errors(tracked[r], truth, n_fft, hop)
        e_frame, _ = Q.gross_errors(framewise[r], truth, n_fft, hop)
        print(name, label, "gross errors of %d interior frames: pitch %d, pitch_track %d" % (n, e_frame, e_path))
        assert e_path <= 2, (label, e_path)
        unmeasured = name == "512_160_400" and label in ("noisy_220_0.3", "noisy_440_0.3")
        at_the_bar = label == "noisy_110_0.3" or (name == "2048_300_1200" and label == "noisy_220_0.3")
        if not (unmeasured or at_the_bar):
            assert e_frame >= 10, (label, e_frame)
    for which in range(3):
        assert not tracked[d.rows(d.wave_index("white", which))].any()
    ok, truth = P.mixed_interior(n_fft, hop)
    assert not ((tracked[d.rows(d.wave_index("mixed"))] > 0) != truth)[ok].any()


# ---- 6. invariances and errors ----
def test_invariances_and_a_poisoned_batch_mate():
    geom = P.GEOMS[0]
    d = dev(geom)
    costs = dict(COSTS["default"])
    pick = [d.wave_index("mixed"), d.wave_index("noisy_220_0.5"), d.wave_index("white", 1), d.wave_index("glide_120_400"), d.wave_index("zeros", 2)]
    whole = _path(d, d.cf, d.cs, d.frame_lens, costs)

    def cut(order, poison=False):
        cf = torch.cat([d.cf[d.rows(i)] for i in order]).contiguous()
        cs = torch.cat([d.cs[d.rows(i)] for i in order]).contiguous()
        lens = [int(d.frame_lens[i]) for i in order]
        if poison:
            bad = torch.rand(37, K, device="cuda") * 300 + 80
            bad[20, 3] = float("nan")
            cf, cs, lens = torch.cat([cf[:lens[0]], bad, cf[lens[0]:]]), torch.cat([cs[:lens[0]], torch.rand(37, K, device="cuda"), cs[lens[0]:]]), lens[:1] + [37] + lens[1:]
        return _path(d, cf, cs, lens, costs), lens

    def same(track, lens, order, skip=()):
        r = 0
        for n, L in enumerate(lens):
            if n not in skip:
                i = order[n - sum(1 for s in skip if s < n)]
                for a, b in ((track.f0, whole.f0), (track.state, whole.state), (track.strength, whole.strength)):
                    assert torch.equal(a[r:r + L], b[d.rows(i)])
                assert np.array_equal(track.terms[n].view(np.uint64), whole.terms[i].view(np.uint64))
            r += L

    same(*cut(pick), pick)
    shuffled = [pick[3], pick[0], pick[4], pick[2], pick[1]]
    same(*cut(shuffled), shuffled)
    for i in pick[:2]:
        same(*cut([i]), [i])
    poisoned, lens = cut(pick, poison=True)
    same(poisoned, lens, pick, skip=(1,))
    r = slice(lens[0], lens[0] + 37)
    assert poisoned.terms[1].tolist() == [37, 2, 0, 0, 0, 0, 0, 0] and poisoned.batch[Q.FLAGS] == 1
    assert not poisoned.f0[r].any() and (poisoned.state[r] == -1).all() and not poisoned.strength[r].any()
    assert poisoned.per_utterance()["flags"].tolist() == [0, 2, 0, 0, 0, 0]
    # a waveform of at most n_fft / 2 samples comes out unvoiced (the third waveform of every packed case)
    for c in ("const_220_0", "white", "mixed"):
        r = d.rows(d.wave_index(c, 2))
        assert not whole.f0[r].any() and (whole.state[r] == -1).all() and not d.cf[r].any()
    empty = _path(d, d.cf[:0], d.cs[:0], [], costs)
    assert empty.f0.shape == (0,) and empty.terms.shape == (0, 8) and not empty.batch.any()


def test_a_captured_call_replays_to_the_eager_result():
    """fs2_op_pitch_path allocates nothing, reads nothing back and does not synchronise: pitch_path can be captured."""
    geom = P.GEOMS[2]
    d = dev(geom)
    costs = dict(COSTS["default"])
    eager = _path(d, d.cf, d.cs, d.frame_lens, costs)
    terms, batch = eager.terms.copy(), eager.batch.copy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = _path(d, d.cf, d.cs, d.frame_lens, costs)
        captured._device.fill_(float("nan"))                          # whatever the capture left: only a replay's numbers count
        captured.f0.fill_(-5)
        captured.state.fill_(-5)
        captured.strength.fill_(-5)
        graph.replay()
    side.synchronize()
    assert torch.equal(captured.f0, eager.f0) and torch.equal(captured.state, eager.state) and torch.equal(captured.strength, eager.strength)
    assert np.array_equal(captured.terms.view(np.uint64), terms.view(np.uint64)) and np.array_equal(captured.batch.view(np.uint64), batch.view(np.uint64))


def test_value_errors_on_the_gpu_machine_too():
    from fastspeech2_amd.vocoder import pitch_candidates, pitch_path, pitch_track, wav_features
    w = torch.zeros(4096, device="cuda")
    z = torch.zeros(6, 3, device="cuda")
    for call, text in ((lambda: pitch_candidates(w, [4096], n_candidates=0), "n_candidates"), (lambda: pitch_candidates(w, [4096], n_candidates=9), "n_candidates"),
                       (lambda: pitch_track(w, [4096], voiced_unvoiced_cost=-1.0), "voiced_unvoiced_cost"),
                       (lambda: pitch_path(z, z, [6], 0.0), "time_step"), (lambda: pitch_path(z, z, [6], 0.01, f0_floor=-1.0), "f0_floor"),
                       (lambda: pitch_path(z, z, [6], 0.01, octave_jump_cost=float("nan")), "octave_jump_cost"),
                       (lambda: pitch_path(z, z, [5], 0.01), "frame_lens"), (lambda: pitch_path(z, z[:, :2], [6], 0.01), "one shape"),
                       (lambda: pitch_path(torch.zeros(6, 9, device="cuda"), torch.zeros(6, 9, device="cuda"), [6], 0.01), r"1 \.\. 8"),
                       (lambda: wav_features(w, [4096], f0_method="best"), "f0_method"),
                       (lambda: pitch_track(w, [4096], hp=_hp(P.GEOMS[3])), r"110\.25")):
        with pytest.raises(ValueError, match=text):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch_path(z.cpu(), z.cpu(), [6], 0.01)
    tr = pitch_track(torch.zeros(0, device="cuda"), [])
    assert tr.f0.shape == (0,) and len(tr) == 0


# ---- 7. plumbing ----
def test_wav_features_and_training_targets_with_the_path():
    from fastspeech2_amd import clean_targets, mel_energy, pitch_track, training_targets, wav_features
    geom = P.GEOMS[0]
    d = dev(geom)
    pick = [d.wave_index("mixed"), d.wave_index("noisy_440_0.5"), d.wave_index("glide_90_300", 1)]
    x = torch.from_numpy(np.concatenate([d.waves[i] for i in pick])).cuda()
    lens = [d.lens[i] for i in pick]
    kw = dict(octave_jump_cost=0.5, voiced_unvoiced_cost=0.1, n_candidates=5, voicing_threshold=0.4)
    for o in (dict(), kw):
        lm, en, f0 = wav_features(x, lens, f0_method="path", **o)
        lm0, en0 = mel_energy(x, lens)
        track = pitch_track(x, lens, **o)
        assert torch.equal(f0, track.f0) and torch.equal(lm, lm0) and torch.equal(en, en0)
        tt = training_targets(x, lens, f0_method="path", **o)
        frame_lens = [n // 256 + 1 for n in lens]
        want_f0, want_stats = clean_targets(f0, frame_lens)
        want_en, _ = clean_targets(en0, frame_lens)
        assert torch.equal(tt.f0, want_f0) and torch.equal(tt.energy, want_en) and torch.equal(tt.logmel, lm0) and tt.pitch_stats == want_stats
    assert not torch.equal(wav_features(x, lens, f0_method="path")[2], wav_features(x, lens, f0_method="path", **kw)[2])
    bare, frame = wav_features(x, lens), wav_features(x, lens, f0_method="frame")
    from fastspeech2_amd.vocoder import pitch
    assert all(torch.equal(a, b) for a, b in zip(bare, frame)) and torch.equal(bare[2], pitch(x, lens))
    t0, t1 = training_targets(x, lens), training_targets(x, lens, f0_method="frame")
    assert torch.equal(t0.f0, t1.f0) and torch.equal(t0.energy, t1.energy) and t0.pitch_stats == t1.pitch_stats
    assert torch.equal(t0.f0, clean_targets(bare[2], [n // 256 + 1 for n in lens])[0])
