"""CPU: the float64 oracle of the pitch path search (tests/pitch_path_oracle.py) against a brute-force enumeration and its own
consequences, the ground truth it reaches where the per-frame estimator fails, and the conditions on the oracle alone that the GPU
tests (tests/test_gpu_pitch_path.py) and the kernel's host build (tests/test_pitch_path_kernel_host.py) rely on."""
import numpy as np
import pytest

from tests import pitch_oracle as P
from tests import pitch_path_oracle as Q

TS = 256 / 22050


def _random(rs, T, K, p_empty=0.3, p_none=0.15):
    f = rs.uniform(60.0, 700.0, (T, K)).astype(np.float32)
    p = rs.uniform(0.0, 1.0, (T, K)).astype(np.float32)
    gone = rs.uniform(size=(T, K)) < p_empty
    gone[rs.uniform(size=T) < p_none] = True
    f[gone] = 0
    p[gone] = 0
    return f, p


def test_oracle_equals_brute_force():
    rs = np.random.RandomState(3)
    seen_empty = seen_none = 0
    for T in range(1, 6):
        for K in (1, 2):
            for costs in (dict(), dict(octave_jump_cost=1.5, voiced_unvoiced_cost=0.02), dict(octave_jump_cost=0.0, voiced_unvoiced_cost=0.4)):
                for _ in range(6):
                    f, p = _random(rs, T, K)
                    seen_empty += int((f == 0).any() and (f > 0).any())
                    seen_none += int((~(f > 0).any(axis=1)).any())
                    got = Q.path(f, p, TS, **costs)
                    top, seqs = Q.brute(f, p, TS, **costs)
                    assert abs(got.record[Q.SCORE] - top) <= 1e-12 * max(1.0, abs(top))
                    assert tuple(got.state + 1) in seqs and len(seqs) == 1
    assert seen_empty > 50 and seen_none > 50


def test_frame_form_equals_cell_form():
    rs = np.random.RandomState(4)
    for T, K in ((1, 1), (2, 3), (7, 8), (40, 2), (33, 8)):
        f, p = _random(rs, T, K)
        for costs in (dict(), dict(octave_jump_cost=0.0, voiced_unvoiced_cost=0.0)):
            a, b = Q.path_cells(f, p, TS, **costs), Q.path(f, p, TS, **costs)
            assert np.array_equal(a.state, b.state) and np.array_equal(a.record.view(np.uint64), b.record.view(np.uint64))
            assert np.array_equal(a.D.view(np.uint64), b.D.view(np.uint64)) and a.gap == b.gap


def test_zero_costs_give_the_per_frame_argmax():
    rs = np.random.RandomState(5)
    for K in (1, 3, 8):
        f, p = _random(rs, 60, K)
        p[5, :] = 0                                                   # a frame whose candidates all score below the threshold
        f[6, 0], p[6, 0] = 71.0, 0.45                                 # u = 0.45 - 0.02 log2(1) = the threshold exactly: a tie goes to unvoiced
        r = Q.path(f, p, TS, octave_jump_cost=0.0, voiced_unvoiced_cost=0.0)
        assert np.array_equal(r.state, Q.frame_argmax(f, p)) and r.record[Q.CHANGED] == 0
        if K == 1:
            assert r.state[6] == -1
            S = Q.score(f[:, 0], p[:, 0])
            assert np.array_equal(r.state == 0, S > 0.45)
        assert r.state[5] == -1


def test_a_huge_voicing_change_cost_keeps_one_voicing():
    rs = np.random.RandomState(6)
    kinds = set()
    for i in range(12):
        f, p = _random(rs, 30, 3, p_empty=0.2, p_none=0.0)
        f[:, 0] = np.where(f[:, 0] > 0, f[:, 0], 150.0)               # every frame has a candidate
        p = (p * (0.3 + 0.1 * i)).astype(np.float32)
        v = Q.path(f, p, TS, voiced_unvoiced_cost=1e6).state >= 0
        assert v.all() or not v.any()
        kinds.add(bool(v.all()))
    assert kinds == {True, False}


def test_flags_and_records():
    rs = np.random.RandomState(7)
    f, p = _random(rs, 9, 2)
    good = Q.path(f, p, TS)
    for bad_value, where in ((np.nan, "f"), (np.inf, "p"), (-1.0, "f"), (-0.5, "p")):
        f2, p2 = f.copy(), p.copy()
        (f2 if where == "f" else p2)[4, 1] = bad_value
        r = Q.path(f2, p2, TS)
        assert r.record.tolist() == [9, 2, 0, 0, 0, 0, 0, 0] and np.all(r.state == -1) and not r.f0.any() and not r.strength.any()
    empty = Q.path(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), TS)
    assert empty.record.tolist() == [0] * 8 and empty.f0.shape == (0,)
    other = Q.path(*_random(rs, 5, 2), TS)
    rows, batch = Q.records([good, r, empty, other])
    assert batch[Q.FLAGS] == 1 and batch[Q.N_FRAMES] == 14 and batch[Q.MAX_STEP] == max(good.record[Q.MAX_STEP], other.record[Q.MAX_STEP])
    assert batch[Q.SCORE] == good.record[Q.SCORE] + 0.0 + other.record[Q.SCORE] and batch[7] == 0
    # the record's counts, restated
    v = good.state >= 0
    assert good.record[Q.VOICED] == v.sum() and good.record[Q.SWITCHES] == (v[1:] != v[:-1]).sum()
    assert good.record[Q.CHANGED] == (good.state != Q.frame_argmax(f, p)).sum()


@pytest.mark.parametrize("geom", P.GEOMS, ids=[g[0] for g in P.GEOMS])
def test_ground_truth_where_the_per_frame_estimator_fails(geom):
    """The table of DESIGN.md section 14.11: gross errors (unvoiced, or more than 20 % off) on interior frames."""
    name, n_fft, hop, win, sr, opt, lo = geom
    seen = 0
    for label, waves, _, paths, truth in Q.cases(geom):
        if truth is None:
            continue
        seen += 1
        frame = P.pitch(waves[0].astype(np.float64), n_fft, hop, win, sr, **opt)
        e_frame, n = Q.gross_errors(frame.f0, truth, n_fft, hop)
        e_path, _ = Q.gross_errors(paths[0].f0, truth, n_fft, hop)
        print(name, label, "per frame %d of %d, path %d" % (e_frame, n, e_path))
        assert e_path == 0
        at_the_bar = label == "noisy_110_0.3" or (name == "2048_300_1200" and label == "noisy_220_0.3")
        if not at_the_bar:
            assert e_frame >= 10
    assert seen == (4 if lo > 110 else 5)
    by = {label: paths for label, _, _, paths, _ in Q.cases(geom)}
    assert all(r.record[Q.VOICED] == 0 for r in by["white"])
    ok, truth = P.mixed_interior(n_fft, hop)
    assert not ((by["mixed"][0].f0 > 0) != truth)[ok].any()


@pytest.mark.parametrize("geom", P.GEOMS, ids=[g[0] for g in P.GEOMS])
def test_conditions_the_gpu_tests_rely_on(geom):
    """(a) at least 95 % of the oracle's top-8 candidates are prominent (max(c - a, c - b) >= 1e-4 and c >= 1e-4): the ones a float32
    implementation is held to find.  (b) no Viterbi cell's best and second-best predecessor are closer than 1e-9 of the cell's value,
    so a last-bit difference in a log2 cannot flip a choice."""
    n = prominent = 0
    gap = np.inf
    for label, _, cands, paths, _ in Q.cases(geom):
        for c, r in zip(cands, paths):
            n += int((c.lag >= 0).sum())
            prominent += int(c.prominent.sum())
            assert r.record[Q.FLAGS] == 0
            gap = min(gap, r.gap)
    print(geom[0], "prominent %d of %d = %.4f, smallest relative gap %.3g" % (prominent, n, prominent / n, gap))
    assert prominent >= 0.95 * n
    assert gap >= 1e-9


@pytest.mark.parametrize("geom", P.GEOMS, ids=[g[0] for g in P.GEOMS])
def test_the_track_is_stable_under_noise_of_float32_size(geom):
    """2e-6 of uniform noise on rho (a float32 implementation's error) changes candidate lists but not one frame of the track."""
    name, n_fft, hop, win, sr, opt, _ = geom
    o = dict(Q.DEFAULTS, **opt)
    changed = frames = 0
    for label, waves, _, paths, truth in Q.cases(geom):
        if truth is None:
            continue
        c = Q.candidates(waves[0].astype(np.float64), n_fft, hop, win, sr, f0_floor=o["f0_floor"], octave_cost=o["octave_cost"], rho_noise=(2e-6, 11))
        r = Q.path(c.f0.astype(np.float32), c.strength.astype(np.float32), hop / sr, o["f0_floor"], o["voicing_threshold"], o["octave_cost"],
                   o["octave_jump_cost"], o["voiced_unvoiced_cost"])
        v = paths[0].f0 > 0
        changed += int(((r.f0 > 0) != v).sum()) + int((np.abs(r.f0[v & (r.f0 > 0)] / paths[0].f0[v & (r.f0 > 0)] - 1) > 1e-3).sum())
        frames += len(v)
    assert changed == 0 and frames > 300


def test_candidates_slot_0_is_the_per_frame_winner():
    for geom in P.GEOMS:
        name, n_fft, hop, win, sr, opt, _ = geom
        for label, waves, cands, _, _ in Q.cases(geom)[::7]:
            o = P.pitch(waves[0].astype(np.float64), n_fft, hop, win, sr, **opt)
            assert np.array_equal(cands[0].strength[:, 0], o.strength)
            assert np.array_equal(cands[0].f0[o.voiced, 0], o.f0[o.voiced])
            S = cands[0].S
            assert np.all(S[:, :-1] >= S[:, 1:]) and np.all((cands[0].f0 > 0) == np.isfinite(S))


def test_ctypes_mirror_of_the_argument_struct_matches_the_compiled_header(tmp_path):
    """fs2_op_pitch_path_args as gcc sees include/fs2.h: sizeof and the offset of every field equal those of _lib.OpPitchPathArgs."""
    import ctypes
    import os
    import re
    import subprocess
    from fastspeech2_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in _lib.OpPitchPathArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fs2.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(fs2_op_pitch_path_args));', '  printf("FS2_PITCH_PATH_TERMS %d\\n", FS2_PITCH_PATH_TERMS);',
           '  printf("FS2_PITCH_MAX_CANDS %d\\n", FS2_PITCH_MAX_CANDS);', '  printf("FS2_ABI_VERSION %d\\n", FS2_ABI_VERSION);']
    src += ['  printf("%s %%zu\\n", offsetof(fs2_op_pitch_path_args, %s));' % (f, f) for f in fields] + ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", exe], check=True)
    probe = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert probe["sizeof"] == ctypes.sizeof(_lib.OpPitchPathArgs) == _lib.OpPitchPathArgs().struct_size
    assert probe["FS2_PITCH_PATH_TERMS"] == _lib.PITCH_PATH_TERMS == Q.TERMS
    assert probe["FS2_PITCH_MAX_CANDS"] == _lib.PITCH_MAX_CANDS == Q.MAX_CANDS
    assert probe["FS2_ABI_VERSION"] == _lib.ABI_VERSION == 4                # the addition is additive
    for f in fields:
        assert getattr(_lib.OpPitchPathArgs, f).offset == probe[f], f
    hdr = open(os.path.join(root, "include", "fs2.h")).read()
    body = hdr[hdr.index("struct fs2_op_pitch_path_args {"):hdr.index("typedef struct fs2_op_pitch_path_args")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[*\s,](\w+)\s*[,;]", body[body.index("{"):])
    assert declared == fields, (declared, fields)


def test_python_layer_on_the_host():
    """PitchTrack from host arrays, and the refusals that come before anything touches the GPU."""
    import torch
    import fastspeech2_amd as fs
    from fastspeech2_amd import vocoder as V
    rs = np.random.RandomState(8)
    res = [Q.path(*_random(rs, T, 3), TS) for T in (12, 0, 30)]
    rows, batch = Q.records(res)
    tr = fs.PitchTrack(None, None, None, rows, batch)
    pu = tr.per_utterance()
    assert len(tr) == 3 and pu["flags"].tolist() == [0, 0, 0] and pu["vuv_switches"].tolist() == [int(r.record[Q.SWITCHES]) for r in res]
    assert pu["voiced_share"][0] == rows[0, Q.VOICED] / 12 and np.isnan(pu["voiced_share"][1])
    assert pu["changed_frames"].tolist() == [int(r.record[Q.CHANGED]) for r in res] and pu["max_octave_step"][2] == rows[2, Q.MAX_STEP]
    assert (V.PATH_FRAMES, V.PATH_FLAGS, V.PATH_SCORE, V.PATH_VOICED, V.PATH_SWITCHES, V.PATH_MAX_STEP, V.PATH_CHANGED) == tuple(range(7))
    z, w = torch.zeros(4, 2), torch.zeros(2048)
    for kw in (dict(time_step=0.0), dict(time_step=float("nan")), dict(f0_floor=0.0), dict(voicing_threshold=float("inf")), dict(octave_cost=float("nan")),
               dict(octave_jump_cost=-0.1), dict(voiced_unvoiced_cost=float("inf"))):
        with pytest.raises(ValueError):
            fs.pitch_path(z, z, [4], **dict(dict(time_step=TS), **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs.pitch_path(z, z, [4], TS)
    for call in (lambda: fs.pitch_candidates(w, [2048], n_candidates=0), lambda: fs.pitch_candidates(w, [2048], n_candidates=9),
                 lambda: fs.pitch_track(w, [2048], n_candidates=2.5), lambda: fs.pitch_track(w, [2048], octave_jump_cost=-1.0),
                 lambda: fs.pitch_track(w, [2048], f0_floor=10.0), lambda: fs.wav_features(w, [2048], f0_method="viterbi"),
                 lambda: fs.wav_features(w, [2048], f0_method="path", n_candidates=0),
                 lambda: fs.wav_features(w, [2048], f0_method="path", voiced_unvoiced_cost=float("nan")),
                 lambda: fs.training_targets(w, [2048], f0_method="dio")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError, match="unknown pitch option"):
        fs.wav_features(w, [2048], octave_jump_cost=0.35)            # a path option without f0_method="path"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fs.wav_features(w, [2048], f0_method="path")
