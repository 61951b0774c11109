"""Float64 numpy statement of the mel-constrained Griffin-Lim (``GriffinLim(...)(..., constraint="mel")``, csrc/griffin_lim.h:
gl_iterate with PROJ = 1), built on ``vocoder_oracle.Stft`` for any transform geometry.  Everything but the
projection of an iteration is ``Stft.griffin_lim``: the start ``C0 = max(pinv . exp(mel), 0) . exp(i angles)``, the transforms, the
momentum form ``A = X - beta T_prev, T_prev <- X`` and the final ISTFT.  Test infrastructure only."""
import numpy as np

from tests import vocoder_oracle as O

Y_FLOOR, R_CAP = 1e-12, 1e4      # act on degenerate frames only (silence: mel = log 1e-5)


def mel_project(A, mel, basis):
    """A [L, bins] complex, mel [L, n_mels] log-mel, basis [n_mels, bins] non-negative -> g . A: the magnitudes of A rescaled per mel
    band so that basis . |g A| follows exp(mel).  A bin no filter covers goes to zero; a bin with A = 0 stays 0."""
    B = np.asarray(basis, np.float64)
    y = np.abs(A) @ B.T
    r = np.minimum(np.exp(np.asarray(mel, np.float64)) / np.maximum(y, Y_FLOOR), R_CAP)
    w = B.sum(axis=0)
    g = np.where(w > 0, (r @ B) / np.where(w > 0, w, 1.0), 0.0)
    return g * A


def griffin_lim_mel(st, mel, basis, pinv, angles, n_iter=30, momentum=0.0):
    """st: an ``Stft``; mel [L, n_mels]; basis [n_mels, bins]; pinv [bins, n_mels]; angles [L, bins] -> signal [hop (L - 1)].
    L < L_min gives zeros, as the kernels write."""
    mel = np.asarray(mel, np.float64)
    L = mel.shape[0]
    if L < O.l_min(st.n_fft, st.hop):
        return np.zeros(st.hop * max(L - 1, 0))
    C = O.mel_to_mag(mel, pinv) * np.exp(1j * np.asarray(angles, np.float64))
    sig = st.istft(C)
    Tprev = np.zeros_like(C)
    beta = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        X = st.stft(sig)
        A = X - beta * Tprev if momentum else X
        Tprev = X
        sig = st.istft(mel_project(A, mel, basis))
    return sig


def log_mel(st, sig, basis):
    """log(clamp(basis . |STFT(sig)|, 1e-5)) [L, n_mels]: TacotronSTFT.mel_spectrogram in float64."""
    return np.log(np.maximum(np.abs(st.stft(sig)) @ np.asarray(basis, np.float64).T, 1e-5))


def mel_error(st, sig, mel, basis):
    """mean |log-mel(sig) - mel|: how far the waveform's mel lies from the one it was made from."""
    return float(np.abs(log_mel(st, sig, basis) - np.asarray(mel, np.float64)).mean())
