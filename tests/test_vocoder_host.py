"""Host-side checks of the Griffin-Lim vocoder (no GPU): the float64 oracle against the reference's recorded outputs, the Slaney
mel filterbank, the seeded-phase hash, save_wav and argument validation."""
import math
import os
import wave

import numpy as np
import pytest
import torch

from tests import vocoder_oracle as O


@pytest.fixture(scope="module")
def g10(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g10_griffin_lim.npz")))


@pytest.mark.parametrize("n_iter", [0, 1, 30])
def test_oracle_matches_reference_fixture(g10, n_iter):
    ref = g10["wav_iter%d" % n_iter]
    got = O.griffin_lim(g10["magnitudes"], g10["angles"], n_iter)
    assert got.shape == ref.shape == (256 * (g10["magnitudes"].shape[0] - 1),)
    # the reference runs in fp32 (conv1d / conv_transpose1d with 1026-row bases): measured 3.6e-7 / 1.0e-6 / 5.8e-6 at 0 / 1 / 30
    assert np.abs(got - ref).max() <= 5e-5 * np.abs(ref).max()
    assert abs(O.spectral_convergence(g10["magnitudes"], got) - O.spectral_convergence(g10["magnitudes"], ref)) < 1e-4


def test_oracle_stft_matches_fixture_magnitudes(g10):
    M = np.abs(O.stft(g10["signal"]))
    assert np.abs(M - g10["magnitudes"]).max() <= 1e-5 * np.abs(M).max()


def _mel_basis_restated(sr, n_fft, n_mels, fmin, fmax):
    # independent restatement: scalar loops over the Slaney mel scale (Auditory Toolbox): linear 3 mels per 200 Hz below 1 kHz,
    # then 27 mels per factor 6.4
    def hz2mel(f):
        return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)

    def mel2hz(m):
        return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)
    lo, hi = hz2mel(fmin), hz2mel(fmax)
    edges = [mel2hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    W = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        a, c, b = edges[i], edges[i + 1], edges[i + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            if a < f < b:
                W[i, k] = ((f - a) / (c - a) if f <= c else (b - f) / (b - c)) * 2.0 / (b - a)
    return W, edges


def test_mel_basis_matches_restatement_and_properties():
    from fastspeech2_amd.vocoder import mel_basis
    B = mel_basis()
    assert B.shape == (80, 513)
    W, edges = _mel_basis_restated(22050, 1024, 80, 0.0, 8000.0)
    assert np.abs(B - W).max() <= 1e-9 * np.abs(W).max()
    freqs = np.arange(513) * 22050 / 1024
    for i in range(80):
        # the triangle peaks at the bin nearest its mel-spaced centre, and the unnormalised triangle integrates to (b - a) / 2,
        # so (Slaney area normalisation) sum of the row x bin width ~= 1 where the triangle spans several bins
        k = int(np.argmax(B[i]))
        assert abs(freqs[k] - edges[i + 1]) <= 22050 / 1024
        if edges[i + 2] - edges[i] > 8 * 22050 / 1024:
            assert abs(B[i].sum() * 22050 / 1024 - 1.0) < 0.02
    assert not B[:, freqs > 8000.0].any()          # nothing above fmax
    assert (B >= 0).all()


def test_mel_basis_defaults_from_hp():
    from fastspeech2_amd import default_hparams
    from fastspeech2_amd.vocoder import GriffinLim, mel_basis
    gl = GriffinLim(default_hparams())
    assert gl.params == dict(sample_rate=22050, n_fft=1024, n_mels=80, fmin=0.0, fmax=8000.0)
    assert np.array_equal(gl._basis_np, mel_basis())


def test_seed_angles_formula():
    from fastspeech2_amd.vocoder import seed_angles
    a = seed_angles(7, 5)
    assert a.shape == (5, 513) and a.dtype == np.float32
    assert (a >= -np.float32(math.pi)).all() and (a < np.float32(math.pi)).all()

    def mix(x):          # the kernel's gl_mix32, on Python ints
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
        return x
    for f, k in ((0, 0), (4, 512), (3, 77)):
        h = mix(((k + 513 * f) & 0xFFFFFFFF) ^ mix((7 + 0x9E3779B9) & 0xFFFFFFFF))
        want = np.float32(np.float32(h >> 8) * np.float32(1.0 / 16777216.0)) * np.float32(6.28318548) - np.float32(3.14159274)
        assert a[f, k] == want
    # keyed by the utterance-local frame: a longer utterance starts with the same angles; another seed differs
    assert np.array_equal(seed_angles(7, 9)[:5], a)
    assert not np.array_equal(seed_angles(8, 5), a)
    # roughly uniform
    big = seed_angles(0, 200).ravel()
    assert abs(big.mean()) < 0.02 and abs(big.std() - math.pi / math.sqrt(3)) < 0.02


def test_save_wav_round_trip(tmp_path):
    from fastspeech2_amd.vocoder import save_wav
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -3.0, 1e-3], np.float32)
    p = tmp_path / "a.wav"
    assert save_wav(p, torch.from_numpy(x)) == x.size
    with wave.open(str(p), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 22050, x.size)
        y = np.frombuffer(f.readframes(x.size), "<i2")
    assert y.tolist() == [0, 16384, -16384, 32767, -32767, 32767, -32767, 33]


def test_griffin_lim_argument_validation():
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude
    gl = GriffinLim()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(torch.zeros(10, 80), [10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft_magnitude(torch.zeros(1000), [1000])

    class FakeCuda(torch.Tensor):          # passes the device check; shape checks run before any GPU work
        @property
        def is_cuda(self):
            return True
    z = lambda *s: torch.zeros(*s).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="packed"):
        gl(z(10, 81), [10])
    with pytest.raises(ValueError, match="513"):
        gl(z(10, 80), [10], magnitudes=True)
    with pytest.raises(ValueError, match="sum to"):
        gl(z(10, 80), [4, 5])
    with pytest.raises(ValueError, match=">= 0"):
        gl(z(10, 80), [11, -1])
    with pytest.raises(ValueError, match="entries"):
        gl(z(2, 6, 80), [3])
    with pytest.raises(ValueError, match="exceeds Lmax"):
        gl(z(2, 6, 80), [3, 7])
    with pytest.raises(ValueError, match="n_iter"):
        gl(z(10, 80), [10], n_iter=-1)
    with pytest.raises(ValueError, match="momentum"):
        gl(z(10, 80), [10], momentum=float("nan"))
    with pytest.raises(ValueError, match="init_phase"):
        gl(z(10, 80), [10], init_phase=z(10, 80))


def test_unsupported_transform_sizes():
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    with pytest.raises(ValueError, match="hop"):
        GriffinLim(DotDict({"audio": {"hop_length": 200}}))
    with pytest.raises(ValueError, match="n_fft"):
        GriffinLim(DotDict({"audio": {"n_fft": 800}}))
