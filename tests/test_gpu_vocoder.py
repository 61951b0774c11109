"""Griffin-Lim vocoder and analysis STFT on the MI355X (fs2_op_griffin_lim / fs2_op_stft) against the float64 oracle
(tests/vocoder_oracle.py, itself checked against the reference's recorded outputs in test_vocoder_host.py)."""
import os

import numpy as np
import pytest
import torch

from tests import vocoder_oracle as O

pytestmark = pytest.mark.gpu


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


@pytest.fixture(scope="module")
def g10(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g10_griffin_lim.npz")))


@pytest.fixture(scope="module")
def gl():
    from fastspeech2_amd.vocoder import GriffinLim
    return GriffinLim()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def test_istft_alone_matches_oracle(gl, g10):
    M, A = g10["magnitudes"], g10["angles"]
    w = gl(_cuda(M), [M.shape[0]], n_iter=0, init_phase=_cuda(A), magnitudes=True)
    got = w.wav.cpu().numpy().astype(np.float64)
    want = O.griffin_lim(M, A, 0)
    err = np.abs(got - want).max() / np.abs(want).max()
    _record("vocoder_istft_rel", err)
    assert got.shape == want.shape and int(w.sample_lens[0]) == want.size
    assert err <= 1e-6, err            # measured 2.2e-7


def test_stft_magnitude_and_logmel_match_oracle(gl, g10):
    from fastspeech2_amd.vocoder import stft_magnitude
    sig = g10["signal"]
    T = [sig.size, 7000, 3000]
    wavs = [sig, sig[:7000] * 0.5, O.harmonic_signal(3000, seed=5)]
    packed = _cuda(np.concatenate(wavs))
    mag = stft_magnitude(packed, T).cpu().numpy().astype(np.float64)
    logmel = stft_magnitude(packed, T, mel=True).cpu().numpy().astype(np.float64)
    want = np.concatenate([np.abs(O.stft(np.asarray(x, np.float64))) for x in wavs])
    assert mag.shape == want.shape == (sum(t // 256 + 1 for t in T), 513)
    err = np.abs(mag - want).max() / np.abs(want).max()
    _record("vocoder_stft_rel", err)
    assert err <= 5e-7, err            # measured 1.0e-7
    # log-mel: compared in the linear domain (near the 1e-5 clamp the log magnifies fp32's absolute error of a tiny |X|), and in
    # the log domain where the mel energy is >= 1 % of the peak
    mel_want = want @ gl._basis_np.T
    merr = np.abs(np.exp(logmel) - np.maximum(mel_want, 1e-5)).max() / mel_want.max()
    _record("vocoder_mel_rel", merr)
    assert merr <= 1e-6, merr
    big = mel_want >= 1e-2 * mel_want.max()
    lerr = np.abs(logmel - np.log(mel_want))[big].max()
    _record("vocoder_logmel_abs_big", lerr)
    assert lerr <= 1e-4, lerr


def test_griffin_lim_30_iterations_matches_oracle(gl, g10):
    M, A = g10["magnitudes"], g10["angles"]
    w = gl(_cuda(M), [M.shape[0]], n_iter=30, init_phase=_cuda(A), magnitudes=True)
    got = w.wav.cpu().numpy().astype(np.float64)
    want = O.griffin_lim(M, A, 30)
    err = np.abs(got - want).max() / np.abs(want).max()
    _record("vocoder_gl30_rel", err)
    sc_got, sc_want = O.spectral_convergence(M, got), O.spectral_convergence(M, want)
    _record("vocoder_gl30_sc_rel_diff", abs(sc_got - sc_want) / sc_want)
    assert abs(sc_got - sc_want) <= 0.01 * sc_want, (sc_got, sc_want)
    assert err <= 1e-3, err
    # the reference's own recording (fp32) of the same run
    assert np.abs(got - g10["wav_iter30"]).max() <= 1e-3 * np.abs(want).max()


def test_momentum_converges_faster(gl):
    sig = O.harmonic_signal(256 * 120, seed=11, noise=0.05)
    M = np.abs(O.stft(sig))
    L = M.shape[0]
    m = _cuda(M)
    scs = []
    for mom in (0.0, 0.99):
        w = gl(m, [L], n_iter=16, momentum=mom, seed=3, magnitudes=True)
        scs.append(O.spectral_convergence(M, w.wav.cpu().numpy().astype(np.float64)))
    _record("vocoder_sc_momentum0", scs[0])
    _record("vocoder_sc_momentum099", scs[1])
    assert scs[1] < scs[0], scs
    # the oracle's momentum run agrees in kind
    from fastspeech2_amd.vocoder import seed_angles
    o = O.griffin_lim(M, seed_angles(3, L), 16, momentum=0.99)
    assert abs(O.spectral_convergence(M, o) - scs[1]) <= 0.02 * O.spectral_convergence(M, o)


def test_seeded_phase_is_the_documented_hash(gl):
    from fastspeech2_amd.vocoder import seed_angles
    sig = O.harmonic_signal(256 * 40, seed=2)
    M = np.abs(O.stft(sig))
    a = gl(_cuda(M), [M.shape[0]], n_iter=2, seed=9, magnitudes=True).wav
    b = gl(_cuda(M), [M.shape[0]], n_iter=2, init_phase=_cuda(seed_angles(9, M.shape[0])), magnitudes=True).wav
    assert torch.equal(a, b)


def test_batch_invariance_and_short_utterances(gl):
    F = 32                                  # frames per workgroup tile (csrc/griffin_lim.h kGlTile)
    lens = [1, 2, 3, 4, 5, F, F + 1, 2 * F + 1, 997, 0, 7]
    g = torch.Generator().manual_seed(0)
    mels = [torch.randn(L, 80, generator=g) * 1.5 - 5.0 for L in lens]
    packed = torch.cat(mels).cuda()
    batch = gl(packed, lens, n_iter=4, seed=5)
    assert batch.sample_lens.tolist() == [256 * max(L - 1, 0) for L in lens]
    parts = batch.split()
    for L, m, got in zip(lens, mels, parts):
        alone = gl(m.cuda(), [L], n_iter=4, seed=5).wav
        assert torch.equal(got, alone), L
        if L < 4:
            assert got.numel() == 256 * max(L - 1, 0) and not got.abs().any()
        else:
            assert torch.isfinite(got).all() and got.abs().max() > 0
    # padded input of the same utterances
    Lmax = max(lens)
    pad = torch.zeros(len(lens), Lmax, 80)
    for b, m in enumerate(mels):
        pad[b, :m.shape[0]] = m
    padded = gl(pad.cuda(), lens, n_iter=4, seed=5)
    assert torch.equal(padded.wav, batch.wav)


def test_non_default_stream_and_cpu_rejected(gl):
    sig = O.harmonic_signal(256 * 300, seed=4)
    M = _cuda(np.abs(O.stft(sig)))
    ref = gl(M, [M.shape[0]], n_iter=8, seed=1, magnitudes=True).wav
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # the input is produced on this stream right before the call: a call that ran elsewhere would read a half-written input
        M2 = torch.empty_like(M)
        M2.copy_(M * 1.0)
        out = gl(M2, [M.shape[0]], n_iter=8, seed=1, magnitudes=True).wav
        res = out.clone()
    s.synchronize()
    assert torch.equal(res, ref)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(M.cpu(), [M.shape[0]], magnitudes=True)


def test_end_to_end_inference_batch_to_wav(gl, tmp_path):
    import wave
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    from fastspeech2_amd.vocoder import save_wav
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
        padded, olens2 = model.inference_batch(xs.cuda(), ilens)
    from fastspeech2_amd.vocoder import GriffinLim
    gl2 = GriffinLim(hp)
    w = gl2(mels, olens)
    olens = [int(x) for x in olens]
    assert w.sample_lens.tolist() == [256 * max(L - 1, 0) for L in olens]
    assert w.wav.numel() == sum(256 * max(L - 1, 0) for L in olens)
    assert torch.isfinite(w.wav).all()
    wp = gl2(padded, olens2)
    assert torch.equal(wp.wav, w.wav)
    p = tmp_path / "tts.wav"
    n = save_wav(p, w.wav, hp.audio.sample_rate)
    with wave.open(str(p), "rb") as f:
        assert (f.getframerate(), f.getsampwidth(), f.getnchannels(), f.getnframes()) == (22050, 2, 1, n)
    assert n == w.wav.numel()
