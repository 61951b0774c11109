"""F0 beside the analysis STFT on the MI355X (fs2_op_stft_pitch_geom: fastspeech2_amd.vocoder.pitch / wav_features) against the
float64 oracle of the same definition (tests/pitch_oracle.py, itself held to ground truth in tests/test_pitch_host.py).  The
estimator is an autocorrelation one, not the reference's DIO.

Measured on an MI355X (this file, every compared voiced frame of a geometry), the largest relative F0 difference to the oracle:
1024_256_1024 6.89e-07, 2048_300_1200 3.69e-06, 1024_200_800 5.14e-07, 512_160_400 4.12e-07; the largest strength difference
2.6e-05 (1024_200_800; the other geometries 3.3e-07 .. 1.0e-06).  The requirement was 1e-3 (a tenth of the method's own 1e-2 bar
against ground truth); every geometry measured below 1e-5, so each is held to 10x its measured value (F0_REL)."""
import numpy as np
import pytest
import torch

from tests import pitch_oracle as P

pytestmark = pytest.mark.gpu

GEOM_IDS = [g[0] for g in P.GEOMS]
# relative F0 difference to the oracle on compared voiced frames: 10x the value measured on an MI355X (all below 1e-5; the
# requirement before any measurement was 1e-3, a tenth of the method's own 1e-2 bar in tests/test_pitch_host.py)
F0_REL = {"1024_256_1024": 6.9e-6, "2048_300_1200": 3.7e-5, "1024_200_800": 5.2e-6, "512_160_400": 4.2e-6}
STRENGTH_ABS = 1e-4
GAP_MIN = 1e-4         # frames whose two best candidates, or whose winner and the voicing threshold, are closer than this in the
                       # oracle are not compared: fp32 may legitimately decide them the other way
EXCLUDED_SHARE = 0.01


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


def _hp(geom):
    from fastspeech2_amd.hparams import DotDict
    _, n_fft, hop, win, sr, _, _ = geom
    return DotDict({"audio": {"sample_rate": sr, "n_fft": n_fft, "hop_length": hop, "win_length": win, "num_mels": 80}})


_cases = P.packed_cases


def _pack(waves):
    return torch.from_numpy(np.concatenate(waves)).cuda(), [len(w) for w in waves]


@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_parent_bits_and_oracle(geom):
    """logmel and energy are mel_energy's bits, pitch() is wav_features()[2], and f0 / strength / voicing follow the oracle."""
    from fastspeech2_amd.vocoder import mel_energy, pitch, wav_features
    name, n_fft, hop, win, sr, opt, _ = geom
    hp = _hp(geom)
    thr = P.DEFAULTS["voicing_threshold"]
    worst_f0, worst_p, n_cmp, n_voiced = 0.0, 0.0, 0, 0
    for label, waves in _cases(geom):
        x, lens = _pack(waves)
        lm, en, f0 = wav_features(x, lens, hp=hp, **opt)
        lm0, en0 = mel_energy(x, lens, hp=hp)
        assert torch.equal(lm, lm0) and torch.equal(en, en0), label
        f0b, st = pitch(x, lens, hp=hp, return_strength=True, **opt)
        assert torch.equal(f0b, f0), label
        frames = sum(n // hop + 1 for n in lens)
        assert f0.shape == st.shape == en.shape == (frames,) and lm.shape == (frames, 80)
        f0, st = f0.cpu().numpy().astype(np.float64), st.cpu().numpy().astype(np.float64)
        assert np.isfinite(f0).all() and np.isfinite(st).all(), label
        n_short = lens[2] // hop + 1
        assert (f0[-n_short:] == 0).all() and (st[-n_short:] == 0).all(), label           # the short waveform: 0 / 0
        o = P.pitch_packed(waves, geom)
        cmp_ = P.compared(o, GAP_MIN, thr)
        share = 1.0 - cmp_.mean()
        voiced = f0 > 0
        both = cmp_ & o.voiced
        rel = np.abs(f0[both] / o.f0[both] - 1.0).max() if both.any() else 0.0
        dp = np.abs(st[cmp_] - o.strength[cmp_]).max()
        print("%s %s: %d frames, excluded %.4f, voiced %d, f0 rel %.3e, strength abs %.3e" % (name, label, frames, share, int(both.sum()), rel, dp))
        assert share <= EXCLUDED_SHARE, (label, share)
        assert (voiced[cmp_] == o.voiced[cmp_]).all(), (label, np.nonzero(cmp_ & (voiced != o.voiced))[0])
        assert rel <= F0_REL[name], (label, rel)
        assert dp <= STRENGTH_ABS, (label, dp)
        worst_f0, worst_p = max(worst_f0, rel), max(worst_p, dp)
        n_cmp, n_voiced = n_cmp + int(cmp_.sum()), n_voiced + int(both.sum())
    assert n_voiced > 1000
    _record("pitch_%s_f0_rel" % name, worst_f0)
    _record("pitch_%s_strength_abs" % name, worst_p)
    _record("pitch_%s_compared_frames" % name, n_cmp)


@pytest.mark.parametrize("geom", P.GEOMS, ids=GEOM_IDS)
def test_batch_invariance_and_repeatability(geom):
    from fastspeech2_amd.vocoder import pitch, wav_features
    _, n_fft, hop, win, sr, opt, _ = geom
    hp = _hp(geom)
    cases = dict(_cases(geom))
    waves = [cases["mixed"][0], cases["glide_200_600"][1], cases["white"][2], cases["const_440_0.05"][0], cases["white"][1]]
    x, lens = _pack(waves)
    lm, en, f0 = wav_features(x, lens, hp=hp, **opt)
    f0b, st = pitch(x, lens, hp=hp, return_strength=True, **opt)
    lm2, en2, f02 = wav_features(x, lens, hp=hp, **opt)
    assert torch.equal(lm, lm2) and torch.equal(en, en2) and torch.equal(f0, f02) and torch.equal(f0, f0b)
    r = 0
    for w in waves:
        n = len(w) // hop + 1
        xa, la = _pack([w])
        lma, ena, f0a = wav_features(xa, la, hp=hp, **opt)
        _, sta = pitch(xa, la, hp=hp, return_strength=True, **opt)
        assert torch.equal(lma, lm[r:r + n]) and torch.equal(ena, en[r:r + n]) and torch.equal(f0a, f0[r:r + n]) and torch.equal(sta, st[r:r + n])
        r += n
    assert r == f0.numel()
    assert (f0[:P.MIXED_SEG - P.margin(n_fft, hop)] == 0).all() and (f0 > 0).any()


def test_non_default_stream():
    from fastspeech2_amd.vocoder import wav_features
    geom = P.GEOMS[2]
    hp = _hp(geom)
    x, lens = _pack(dict(_cases(geom))["mixed"])
    ref = wav_features(x, lens, hp=hp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # the input is produced on this stream right before the call: a call that ran elsewhere would read a half-written input
        x2 = torch.empty_like(x)
        x2.copy_(x * 1.0)
        res = [t.clone() for t in wav_features(x2, lens, hp=hp)]
    s.synchronize()
    for a, b in zip(res, ref):
        assert torch.equal(a, b)


def test_cpu_tensors_and_bad_floor_raise_on_the_gpu_machine_too():
    from fastspeech2_amd.vocoder import pitch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch(torch.zeros(4096), [4096])
    with pytest.raises(ValueError, match=r"110\.25"):
        pitch(torch.zeros(4096, device="cuda"), [4096], hp=_hp(P.GEOMS[3]))
    f0 = pitch(torch.zeros(0, device="cuda"), [])
    assert f0.shape == (0,)


def test_end_to_end_text_to_wav_to_features():
    """inference_batch(packed=True) -> GriffinLim -> wav_features: the three per-frame targets line up with olens."""
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    from fastspeech2_amd.vocoder import GriffinLim, wav_features
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    ilens = [23, 9, 17]
    xs = torch.zeros(3, max(ilens), dtype=torch.int64)
    for b, n in enumerate(ilens):
        xs[b, :n] = torch.randint(1, N_PHONEME_SYMBOLS, (n,), generator=g)
    with torch.no_grad():
        mels, olens = model.inference_batch(xs.cuda(), ilens, packed=True)
    olens = [int(v) for v in olens]
    w = GriffinLim(hp)(mels, olens)
    lm, en, f0 = wav_features(w.wav, w.sample_lens, hp=hp)
    frames = sum(int(n) // 256 + 1 for n in w.sample_lens)
    assert frames == sum(max(L, 1) for L in olens)               # hop (L - 1) samples give L frames back
    assert lm.shape == (frames, hp.audio.num_mels) and en.shape == (frames,) and f0.shape == (frames,)
    assert torch.isfinite(f0).all() and torch.isfinite(en).all() and torch.isfinite(lm).all()
    assert ((f0 == 0) | ((f0 >= 71.0) & (f0 <= 800.0))).all()
