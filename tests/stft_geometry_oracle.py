"""Float64 numpy restatement of the vocoder's transform for any geometry (n_fft, hop, win_length): the reference's STFT class
(utils/stft.py:41-151) with its bases built literally -- forward basis = [Re; Im] rows of the n_fft-point DFT times the periodic Hann
window of win_length zero-padded to n_fft at the centre (pad_center), inverse basis = pinv(n_fft / hop . F)^T times the same window,
conv-transpose overlap-add, division by the window sum-square where it exceeds tiny, x n_fft / hop, trim n_fft / 2 at both ends --
and the reference's griffin_lim (dataset/audio_processing.py:224-240).  At 1024 / 256 / 1024 it is tests/vocoder_oracle.py.
Test infrastructure only."""
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
        """complex C [L, bins] -> signal [hop (L - 1)]."""
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
        """M [L, bins] magnitudes, angles [L, bins] -> signal [hop (L - 1)]; L < L_min gives zeros (what the kernels write)."""
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
        X = np.abs(self.stft(sig))
        return float(np.linalg.norm(M - X) / np.linalg.norm(M))
