"""Float64 numpy restatement of the Griffin-Lim vocoder (fastspeech2_amd/vocoder.py, csrc/griffin_lim.h) for any transform geometry
(n_fft, hop, win_length): the reference's STFT class (utils/stft.py:41-151) with its bases built literally -- forward basis = [Re; Im]
rows of the n_fft-point DFT times the periodic Hann window of win_length zero-padded to n_fft at the centre (pad_center), inverse
basis = pinv(n_fft / hop . F)^T times the same window, conv-transpose overlap-add, division by the window sum-square where it exceeds
tiny, x n_fft / hop, trim n_fft / 2 at both ends -- and the reference's griffin_lim (dataset/audio_processing.py:171-240).  The
module-level ``stft``, ``istft``, ``griffin_lim``, ``spectral_convergence`` and ``window_sumsquare`` are those of the default transform
(1024 / 256 / 1024).  Test infrastructure only (host tests and GPU tests compare against it)."""
import numpy as np


def hann_padded(n_fft, win):
    """scipy.signal.get_window("hann", win, fftbins=True) zero-padded to n_fft at the centre (librosa.util.pad_center)."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    lp = (n_fft - win) // 2
    return np.pad(w, (lp, n_fft - win - lp))


def l_min(n_fft, hop):
    """Fewest frames L whose hop (L - 1) samples the reference can reflect-pad by n_fft / 2."""
    return n_fft // (2 * hop) + 2


class Stft:
    _cache = {}

    def __init__(self, n_fft=1024, hop=256, win=None):
        self.n_fft, self.hop, self.win = int(n_fft), int(hop), int(win if win is not None else n_fft)
        self.cut = self.n_fft // 2 + 1
        key = (self.n_fft, self.hop, self.win)
        if key not in Stft._cache:
            F = np.fft.fft(np.eye(self.n_fft))
            F = np.vstack([np.real(F[:self.cut, :]), np.imag(F[:self.cut, :])])
            w = hann_padded(self.n_fft, self.win)
            Stft._cache[key] = (F * w[None, :], np.linalg.pinv(float(self.n_fft) / self.hop * F).T * w[None, :], w)
        self.fwd, self.inv, self.window = Stft._cache[key]

    def window_sumsquare(self, n_frames):
        n = self.n_fft + self.hop * (n_frames - 1)
        x = np.zeros(n)
        w2 = self.window ** 2
        for i in range(n_frames):
            s = i * self.hop
            x[s:min(n, s + self.n_fft)] += w2[:max(0, min(self.n_fft, n - s))]
        return x

    def stft(self, sig):
        """sig [T] -> complex X [L, bins], L = T // hop + 1 (reflect padding by n_fft / 2; needs T > n_fft / 2, as torch's pad)."""
        sig = np.asarray(sig, np.float64)
        if sig.size <= self.n_fft // 2:
            raise ValueError("reflect padding by %d needs more than %d samples, got %d" % (self.n_fft // 2, self.n_fft // 2, sig.size))
        x = np.pad(sig, (self.n_fft // 2, self.n_fft // 2), mode="reflect")
        L = (len(x) - self.n_fft) // self.hop + 1
        frames = np.stack([x[self.hop * f:self.hop * f + self.n_fft] for f in range(L)])
        y = frames @ self.fwd.T
        return y[:, :self.cut] + 1j * y[:, self.cut:]

    def istft(self, C):
        """complex C [L, bins] -> signal [hop (L - 1)] (STFT.inverse: conv_transpose1d with the pinv basis, / wss, x n_fft / hop, trim)."""
        L = C.shape[0]
        rec = np.concatenate([C.real, C.imag], axis=1)
        fr = rec @ self.inv
        out = np.zeros(self.n_fft + self.hop * (L - 1))
        for f in range(L):
            out[self.hop * f:self.hop * f + self.n_fft] += fr[f]
        wss = self.window_sumsquare(L)
        nz = wss > np.finfo(np.float32).tiny
        out[nz] /= wss[nz]
        out *= float(self.n_fft) / self.hop
        return out[self.n_fft // 2:len(out) - self.n_fft // 2]

    def griffin_lim(self, M, angles, n_iter=30, momentum=0.0):
        """M [L, bins] magnitudes, angles [L, bins] initial phase -> signal [hop (L - 1)]; L < L_min gives zeros (what the kernels
        write).  momentum: librosa's fast Griffin-Lim."""
        M = np.asarray(M, np.float64)
        L = M.shape[0]
        if L < l_min(self.n_fft, self.hop):
            return np.zeros(self.hop * max(L - 1, 0))
        C = M * np.exp(1j * np.asarray(angles, np.float64))
        sig = self.istft(C)
        Tprev = np.zeros_like(C)
        beta = momentum / (1.0 + momentum)
        for _ in range(n_iter):
            X = self.stft(sig)
            A = X - beta * Tprev if momentum else X
            Tprev = X
            mag = np.abs(A)
            P = np.where(mag > 0, A / np.where(mag > 0, mag, 1.0), 1.0)
            sig = self.istft(M * P)
        return sig

    def energy(self, sig):
        """Per-frame energy of the reference's preprocessing: torch.norm(|X|, dim=0) (nvidia_preprocessing.py)."""
        return np.linalg.norm(np.abs(self.stft(sig)), axis=1)

    def spectral_convergence(self, M, sig):
        """||M - |STFT(sig)||| / ||M||."""
        X = np.abs(self.stft(sig))
        return float(np.linalg.norm(M - X) / np.linalg.norm(M))


# the default transform (configs/default.yaml: n_fft = win_length = 1024, hop 256)
N_FFT, HOP = 1024, 256
_DEFAULT = Stft(N_FFT, HOP, N_FFT)
stft, istft, griffin_lim = _DEFAULT.stft, _DEFAULT.istft, _DEFAULT.griffin_lim
spectral_convergence, window_sumsquare = _DEFAULT.spectral_convergence, _DEFAULT.window_sumsquare


def hann():
    return _DEFAULT.window.copy()       # scipy.signal.get_window("hann", 1024, fftbins=True)


def mel_to_mag(mel, pinv):
    """M = max(pinv . exp(mel), 0); mel [L, n_mels], pinv [bins, n_mels]."""
    return np.maximum(np.exp(np.asarray(mel, np.float64)) @ np.asarray(pinv, np.float64).T, 0.0)


def harmonic_signal(n, seed=0, f0=220.0, sr=22050, noise=0.0):
    """A small test signal: decaying harmonics of f0 with a slow vibrato, plus optional white noise; |x| < 1."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * t + 0.8 * np.sin(2 * np.pi * 5.0 * t)
    x = sum((0.5 / h) * np.sin(h * ph + rs.uniform(0, 2 * np.pi)) for h in range(1, 9))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 1.5 * t))
    x = x + noise * rs.randn(n)
    return 0.8 * x / np.abs(x).max()
