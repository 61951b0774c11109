"""CPU: the F0 estimator's definition (tests/pitch_oracle.py, float64) against ground truth on synthetic signals whose F0 is known, and
the argument checks of fastspeech2_amd.vocoder.pitch / wav_features that need no GPU.  The estimator is an autocorrelation one
(Boersma 1993 without the path search), not the reference's DIO; tests/test_gpu_pitch.py holds the kernel to this oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pitch_oracle as P

GEOM_IDS = [g[0] for g in P.GEOMS]


@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_oracle_finds_the_known_f0_on_every_interior_frame(geom):
    """const (11 F0s x noise 0 / 0.05) and glides: every interior frame voiced, relative F0 error <= 1e-2 (the prototype's worst was
    3.96e-3 over about 6,900 frames: 2.5x margin)."""
    _, n_fft, hop, win, sr, opt, _ = geom
    worst, n = 0.0, 0
    for label, sig, truth in P.signals(geom):
        r = P.pitch(sig, n_fft, hop, win, sr, **opt)
        assert r.f0.shape == truth.shape == (sig.size // hop + 1,)
        ok = P.interior(truth.size, n_fft, hop)
        assert r.voiced[ok].all(), (label, np.nonzero(ok & ~r.voiced)[0])
        err = np.abs(r.f0[ok] / truth[ok] - 1.0).max()
        worst, n = max(worst, err), n + int(ok.sum())
        assert err <= 1e-2, (label, err)
    print("%s: worst relative F0 error %.3e over %d interior frames" % (geom[0], worst, n))
    assert n > 900


@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_oracle_noise_and_silence_are_unvoiced(geom):
    _, n_fft, hop, win, sr, opt, _ = geom
    r = P.pitch(P.white(0.3, sr, hop, 200, seed=5), n_fft, hop, win, sr, **opt)
    print("%s: largest p on white noise %.3f" % (geom[0], r.strength.max()))
    assert not r.voiced.any() and (r.f0 == 0).all()
    z = P.pitch(np.zeros(60 * hop), n_fft, hop, win, sr, **opt)
    assert not z.voiced.any() and (z.f0 == 0).all() and (z.strength == 0).all()
    short = P.pitch(0.5 * np.ones(n_fft // 2), n_fft, hop, win, sr, **opt)         # <= n_fft / 2 samples: 0 / 0 on all its frames
    assert short.f0.size == (n_fft // 2) // hop + 1 and (short.f0 == 0).all() and (short.strength == 0).all()


@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_oracle_voicing_follows_the_segments_of_mixed(geom):
    _, n_fft, hop, win, sr, opt, _ = geom
    r = P.pitch(P.mixed(sr, hop), n_fft, hop, win, sr, **opt)
    inner, label = P.mixed_interior(n_fft, hop)
    assert r.voiced.shape == inner.shape
    wrong = np.nonzero(inner & (r.voiced != label))[0]
    print("%s: %d voicing errors of %d interior frames" % (geom[0], wrong.size, int(inner.sum())))
    assert wrong.size == 0, wrong
    assert {"1024_256_1024": 165, "2048_300_1200": 145}.get(geom[0], int(inner.sum())) == int(inner.sum())


@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_oracle_leaves_the_gpu_cases_decidable(geom):
    """The packed cases tests/test_gpu_pitch.py runs: in the oracle alone at most 1 % of a case's frames have their two best
    candidates, or the winner and the voicing threshold, within 1e-4 (those frames a float32 kernel may decide the other way)."""
    n = 0
    for label, waves in P.packed_cases(geom):
        assert len({len(w) for w in waves}) == 3 and min(len(w) for w in waves) <= geom[1] // 2
        o = P.pitch_packed(waves, geom)
        assert 1.0 - P.compared(o).mean() <= 0.01, label
        n += o.f0.size
    assert n > 2500


def test_oracle_tie_and_candidate_rules():
    """A pure tone at an integer period: the candidates at t, 2t, .. have equal p; the octave cost makes the smallest lag win."""
    n_fft, hop, win, sr = 1024, 256, 1024, 22050
    t = np.arange(60 * hop)
    r = P.pitch(np.sin(2 * np.pi * t / 63.0), n_fft, hop, win, sr)
    ok = P.interior(r.f0.size, n_fft, hop)
    assert np.abs(r.f0[ok] / (sr / 63.0) - 1).max() < 1e-3 and (r.gap[ok] > 0.015).all()


def _hp(n_fft, hop, win, sr):
    from fastspeech2_amd.hparams import DotDict
    return DotDict({"audio": {"sample_rate": sr, "n_fft": n_fft, "hop_length": hop, "win_length": win, "num_mels": 80}})


def test_python_lag_rule_is_the_oracles():
    from fastspeech2_amd.vocoder import pitch_lags
    for _, n_fft, hop, win, sr, opt, _ in P.GEOMS:
        o = dict(P.DEFAULTS, **opt)
        assert pitch_lags(sr, win, o["f0_floor"], o["f0_ceil"]) == P.lag_range(sr, win, o["f0_floor"], o["f0_ceil"])
    assert pitch_lags(22050, 400, 110.25, 800.0) == (27, 200)          # the lowest usable floor itself
    for bad in ((22050, 400, 110.2, 800.0), (22050, 1024, 71.0, 11026.0), (22050, 1024, 0.0, 800.0), (22050, 1024, 300.0, 200.0)):
        with pytest.raises(ValueError):
            pitch_lags(*bad)


def test_validation_without_a_gpu():
    import fastspeech2_amd as fs
    from fastspeech2_amd.hparams import DotDict
    x, n = torch.zeros(4096), [4096]
    for call in (lambda **kw: fs.pitch(x, n, **kw), lambda **kw: fs.wav_features(x, n, **kw)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(hp=_hp(512, 160, 400, 22050), f0_floor=110.4)
        with pytest.raises(ValueError, match=r"110\.25"):                # before the tensors are looked at: nothing is launched
            call(hp=_hp(512, 160, 400, 22050))
        with pytest.raises(ValueError, match="f0_ceil"):
            call(f0_ceil=20000.0)
        with pytest.raises(ValueError, match="must name n_fft, hop_length and win_length together"):
            call(hp=DotDict({"audio": {"n_fft": 2048}}))
    with pytest.raises(TypeError):
        fs.wav_features(x, n, return_strength=True)
    with pytest.raises(TypeError, match="bogus"):
        fs.wav_features(x, n, bogus=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # the parent's functions, as before
        fs.mel_energy(x, n)


@pytest.fixture(scope="module")
def lib():
    from fastspeech2_amd import _lib
    _lib.build()
    return _lib.lib()


OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -5, -6      # include/fs2.h
PTR = 0x1000           # stands for a device pointer: no call below gets as far as using one


def _i32s(v):
    return (C.c_int32 * len(v))(*v)


def _call(lib, g=(1024, 256, 1024, 80), lens=(3000, 700), ws=PTR, ws_bytes=0, sr=22050, floor=71.0, ceil=800.0, thr=0.45, oc=0.02, f0=PTR, wav=PTR):
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    return lib.fs2_op_stft_pitch_geom(None, *g, wav, len(lens), _i32s(starts), _i32s(lens), ws, ws_bytes, None, None, None, None, sr, floor, ceil,
                                      thr, oc, f0, None)


def test_c_entry_point_refuses_before_any_launch(lib):
    from fastspeech2_amd import _lib
    assert "fs2_op_stft_pitch_geom" in _lib.EXPORTS and "fs2_op_stft_pitch_workspace_bytes_geom" in _lib.EXPORTS
    lens = _i32s((3000, 700))
    for g in ((1024, 256, 1024, 80), (512, 160, 400, 80), (2048, 300, 1200, 80), (1024, 200, 800, 80)):
        base = int(lib.fs2_op_stft_workspace_bytes_geom(*g, 2, lens))
        need = int(lib.fs2_op_stft_pitch_workspace_bytes_geom(*g, 2, lens))
        assert need == base + -(-4 * (g[0] // 2 + 2) // 256) * 256, g        # the one table more: n_fft / 2 + 2 floats, 256-aligned
    need = int(lib.fs2_op_stft_pitch_workspace_bytes_geom(1024, 256, 1024, 80, 2, lens))
    assert lib.fs2_op_stft_pitch_workspace_bytes_geom(1000, 256, 1000, 80, 2, lens) == 0
    assert _call(lib, ws_bytes=need - 1) == ERR_WORKSPACE
    assert b"workspace" in lib.fs2_last_error(None)
    assert _call(lib, g=(512, 160, 400, 80)) == ERR_UNSUPPORTED
    assert b"110.25" in lib.fs2_last_error(None)
    assert _call(lib, ceil=20000.0) == ERR_UNSUPPORTED
    assert _call(lib, g=(512, 160, 400, 80), floor=110.4) == ERR_WORKSPACE       # accepted: only the workspace stops it
    assert _call(lib, floor=0.0) == ERR_ARG
    assert _call(lib, floor=900.0) == ERR_ARG
    assert _call(lib, sr=0) == ERR_ARG
    assert _call(lib, thr=float("nan")) == ERR_ARG
    assert _call(lib, wav=None, ws_bytes=need) == ERR_ARG
    assert _call(lib, ws=None, ws_bytes=need) == ERR_ARG
    assert _call(lib, lens=(), wav=None, ws=None) == OK                          # no waveform: nothing to do
    # without f0 and strength it is fs2_op_stft_geom, and without any output it is empty
    assert _call(lib, f0=None, wav=None, ws=None) == OK
