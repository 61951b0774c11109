"""Numpy statement of the excitation from F0 and of its STFT phase (fastspeech2_amd/csrc/gl_excite.h, include/fs2.h:
fs2_op_excitation_geom / fs2_op_f0_phase_geom), twice: in float64 (``dtype=np.float64``: the oracle) and in
float32 with the phase theta, the frequency and the harmonic count still in float64 (``dtype=np.float32``: the statement whose own
error against the oracle sets the tolerances of the kernel tests, see ``bars``).  Test infrastructure only.

One utterance: L frames, hop H, sample rate sr, f0[0..L-1] float32 in Hz -> N = H (L - 1) samples; frame t is centred on sample t H.
  voiced frame     f0[t] finite and f0_floor <= f0[t] <= f0_ceil
  voiced segment   t <= L - 2 covers the samples t H .. t H + H - 1; voiced iff frames t and t + 1 are: a = f0[t], d = f0[t+1] - f0[t]
                   (both exact in float64); else a = d = 0
  frequency        n = t H + i: f = a + (d i) / H
  phase in turns   S_t = (H a + d (H - 1) 0.5) / sr; Theta_0 = 0, Theta_{t+1} = frac(Theta_t + S_t) in frame order;
                   theta[n] = frac(Theta_t + ((i + 1) a + (d (i (i + 1))) / (2 H)) / sr); frac(x) = x - floor(x); every operation
                   rounded to float64 on its own, in the order written
  voiced sample    Hn = the largest integer with Hn f < sr / 2 (the product rounded to float64), at least 1;
                   e[n] = sqrt(2 / Hn) sum_{h = 1..Hn} cos(2 pi frac(h theta[n]))                       (unit power)
  unvoiced sample  h = mix32(n ^ mix32(seed + 0x9E3779B9)), u = (h >> 8) / 2^24, e[n] = (u - 0.5) sqrt(12)  (float32, bit-exact)
  phase            atan2(Im, Re) of the STFT of e (reflect padding, periodic Hann of win in n_fft), float32; 0 where both parts are 0;
                   every row 0 where N <= n_fft / 2
"""
import numpy as np

from tests import vocoder_oracle as O

F32, F64 = np.float32, np.float64
DEFAULTS = dict(f0_floor=71.0, f0_ceil=800.0)


def _mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def noise(n_samples, seed):
    """float32 [n_samples]: (u - 0.5) sqrt(12) of the counter hash, one rounding per operation."""
    with np.errstate(over="ignore"):
        s = _mix32(np.uint32((int(seed) + 0x9E3779B9) & 0xFFFFFFFF))
        h = _mix32(np.arange(n_samples, dtype=np.uint32) ^ s)
    u = (h >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)
    return (u - F32(0.5)) * F32(3.46410162)


def voiced_frames(f0, f0_floor=71.0, f0_ceil=800.0):
    f = np.asarray(f0, F32).astype(F64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(f) & (f >= f0_floor) & (f <= f0_ceil)


def segments(f0, f0_floor=71.0, f0_ceil=800.0):
    """(a [L - 1], d [L - 1], voiced [L - 1]) float64 / bool; empty for L <= 1."""
    f = np.asarray(f0, F32).astype(F64)
    v = voiced_frames(f0, f0_floor, f0_ceil)
    if f.size <= 1:
        return np.zeros(0), np.zeros(0), np.zeros(0, bool)
    vs = v[:-1] & v[1:]
    fa, fb = np.where(vs, f[:-1], 0.0), np.where(vs, f[1:], 0.0)
    return fa, fb - fa, vs


def frame_prefix(a, d, hop, sr):
    """Theta [L] (L = len(a) + 1) in turns: the only thing that chains the frames."""
    S = (float(hop) * a + d * float(hop - 1) * 0.5) / float(sr)
    T = np.zeros(a.size + 1)
    for t in range(a.size):
        x = T[t] + S[t]
        T[t + 1] = x - np.floor(x)
    return T


def sample_phase(f0, hop, sr, f0_floor=71.0, f0_ceil=800.0):
    """(theta [N] turns, f [N] Hz, Hn [N] int, voiced [N] bool, Theta [L]) in float64."""
    a, d, vs = segments(f0, f0_floor, f0_ceil)
    T = frame_prefix(a, d, hop, sr)
    i = np.arange(hop, dtype=F64)[None, :]
    A, D = a[:, None], d[:, None]
    x = T[:-1, None] + ((i + 1.0) * A + (D * (i * (i + 1.0))) / float(2 * hop)) / float(sr)
    theta = (x - np.floor(x)).reshape(-1)
    f = (A + (D * i) / float(hop)).reshape(-1)
    voiced = np.repeat(vs, hop)
    half = float(sr) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        Hn = np.where(voiced, np.floor(half / np.where(voiced, f, 1.0)), 1.0)
    for _ in range(2):
        Hn = np.where(voiced & (Hn * f >= half), Hn - 1.0, Hn)
        Hn = np.where(voiced & ((Hn + 1.0) * f < half), Hn + 1.0, Hn)
    Hn = np.maximum(Hn, 1.0)
    return theta, f, Hn.astype(np.int64), voiced, T


def excitation(f0, hop, sr, seed=0, f0_floor=71.0, f0_ceil=800.0, dtype=F64):
    """e [hop (L - 1)]: the sum of cosines in ``dtype`` (float32: every term, the running sum in harmonic order and the scale are
    rounded to float32; theta, frac(h theta) and Hn stay float64), the hashed noise where unvoiced."""
    L = np.asarray(f0).size
    N = hop * max(L - 1, 0)
    if N == 0:
        return np.zeros(0, dtype)
    theta, _, Hn, voiced, _ = sample_phase(f0, hop, sr, f0_floor, f0_ceil)
    e = noise(N, seed).astype(dtype)
    idx = np.nonzero(voiced)[0]
    for lo in range(0, idx.size, 8192):
        k = idx[lo:lo + 8192]
        h = np.arange(1, int(Hn[k].max()) + 1, dtype=F64)[None, :]
        x = h * theta[k, None]
        x = x - np.floor(x)
        on = h <= Hn[k, None]
        if dtype == F64:
            s = np.where(on, np.cos(2.0 * np.pi * x), 0.0).sum(axis=1)
            e[k] = np.sqrt(2.0 / Hn[k]) * s
        else:
            c = np.where(on, np.cos(F32(6.28318548) * x.astype(F32)), F32(0.0)).astype(F32)
            s = np.cumsum(c, axis=1, dtype=F32)[:, -1]          # in harmonic order, one rounding per addition
            e[k] = np.sqrt(F32(2.0) / Hn[k].astype(F32)).astype(F32) * s
    return e


def stft_of(e, n_fft, hop, win, n_frames, dtype=F64):
    """complex X [n_frames, bins] of the excitation as gl_stft cuts its frames; zeros where it is too short for the reflect padding.
    float32: the windowed frames and the transform are float32 (numpy transforms float32 input in float32)."""
    NB = n_fft // 2 + 1
    if e.size <= n_fft // 2:
        return np.zeros((n_frames, NB), np.complex128 if dtype == F64 else np.complex64)
    x = np.pad(np.asarray(e, dtype), (n_fft // 2, n_fft // 2), mode="reflect")
    fr = np.stack([x[hop * f:hop * f + n_fft] for f in range(n_frames)]) * O.hann_padded(n_fft, win).astype(dtype)[None, :]
    X = np.fft.rfft(fr, axis=1)                          # (vocoder_oracle.Stft.stft is the same transform as a matrix product)
    assert X.dtype == (np.complex128 if dtype == F64 else np.complex64)
    return X


def phase_of(X):
    ph = np.arctan2(X.imag, X.real)
    return np.where((X.real == 0) & (X.imag == 0), 0.0, ph).astype(F32)


def f0_phase(f0, n_fft, hop, win, sr, seed=0, f0_floor=71.0, f0_ceil=800.0, dtype=F64, return_stft=False):
    """phase float32 [L, bins] of one utterance (and X with ``return_stft``)."""
    L = np.asarray(f0).size
    e = excitation(f0, hop, sr, seed, f0_floor, f0_ceil, dtype)
    X = stft_of(e, n_fft, hop, win, L, dtype)
    return (phase_of(X), X) if return_stft else phase_of(X)


def batch(fn, f0_rows, starts, lens, width=None):
    """``fn(f0 of one utterance)`` laid into the rows of the batch's source layout ([rows] or [rows, width]), zeros elsewhere."""
    rows = np.asarray(f0_rows).shape[0]
    out = np.zeros((rows, width) if width else rows, F32)
    for s, n in zip(starts, lens):
        if n > 0:
            out[s:s + n] = fn(np.asarray(f0_rows)[s:s + n])
    return out


# ---- the tolerances of the kernel tests: 8 x the float32 statement's own error against the float64 one ----
def phasor_error(ph, X64, ref):
    """max |exp(i ph) - exp(i ref)| over the bins with |X64| >= 1e-3 max_k |X64[t]| (0 without such a bin)."""
    mag = np.abs(X64)
    m = (mag >= 1e-3 * mag.max(axis=1, keepdims=True)) & (mag > 0)
    if not m.any():
        return 0.0
    return float(np.abs(np.exp(1j * ph.astype(F64)) - np.exp(1j * ref.astype(F64)))[m].max())


def bars(f0s, n_fft, hop, win, sr, seed=0, f0_floor=71.0, f0_ceil=800.0):
    """(excitation bar, phase bar) over the utterances ``f0s``: 8 x the float32 statement's largest absolute error of a sample, and 8 x
    its largest phasor error, against the float64 statement.  The factor allows another equally valid float32 evaluation (a closed
    form for the sum, another order of additions, another FFT)."""
    ee, pe = 0.0, 0.0
    for f0 in f0s:
        e64 = excitation(f0, hop, sr, seed, f0_floor, f0_ceil, F64)
        e32 = excitation(f0, hop, sr, seed, f0_floor, f0_ceil, F32)
        if e64.size:
            ee = max(ee, float(np.abs(e32.astype(F64) - e64).max()))
        L = np.asarray(f0).size
        X64 = stft_of(e64, n_fft, hop, win, L, F64)
        pe = max(pe, phasor_error(phase_of(stft_of(e32, n_fft, hop, win, L, F32)), X64, phase_of(X64)))
    return 8.0 * ee, 8.0 * pe


# ---- f0 rows that take every path: voiced glides, unvoiced, NaN / inf / negative, the floor and the ceiling exactly ----
BATCH_LENS = (1, 2, 3, 5, 32, 33, 65, 70)


def f0_rows(L, seed, f0_floor=71.0, f0_ceil=800.0):
    rs = np.random.RandomState(seed)
    t = np.arange(L)
    f = (rs.uniform(90, 300) + rs.uniform(10, 60) * np.sin(0.21 * t + rs.uniform(0, 6))).astype(F32)
    if L >= 5:
        f[1] = F32(f0_floor)                # exactly at the floor and at the ceiling: voiced
        f[2] = F32(f0_ceil)
    if L >= 32:
        f[7:12] = 0.0                       # unvoiced stretch
        f[14] = np.nan
        f[16] = np.inf
        f[18] = -120.0
        f[20] = 0.0; f[22] = 0.0            # frame 21: a voiced island of one frame, no voiced segment
        f[25] = F32(f0_floor) - F32(0.5)
        f[27] = F32(f0_ceil) + F32(1.0)
    return f


def batch_case(lens=BATCH_LENS, padded=False, seed=21):
    """(f0 rows float32 [rows], starts, lens): the utterances packed, or each at b * max(lens) with NaN in the rows no utterance covers."""
    lens = list(lens)
    stride = max(lens) if lens else 0
    starts = [b * stride for b in range(len(lens))] if padded else list(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int))
    rows = stride * len(lens) if padded else int(sum(lens))
    f = np.full(rows, np.nan, F32)
    for b, (s, n) in enumerate(zip(starts, lens)):
        f[s:s + n] = f0_rows(n, seed + b)
    return f, starts, lens


# ---- what the phase is for: one-pass vocoding (host and GPU tests share the cases and the oracle's figures) ----
SR = 22050
VALUE_GEOMS = ((1024, 256, 1024), (2048, 300, 1200))
SIGNALS = ("harmonic", "speech")
LORENTZ = ((1.0, 600.0, 120.0), (0.6, 1500.0, 200.0), (0.3, 2600.0, 250.0), (0.1, 3800.0, 400.0))


def harmonic_case(hop, sr=SR):
    """(signal [63 hop], f0 float32 [64]): vocoder_oracle.harmonic_signal(seed=1, noise=0.01), whose phase 2 pi 220 t + 0.8 sin(2 pi 5 t)
    has the frequency 220 + 4 cos(2 pi 5 t)."""
    sig = O.harmonic_signal(hop * 63, seed=1, noise=0.01, sr=sr)
    tc = np.arange(64) * hop / float(sr)
    return sig, (220.0 + 4.0 * np.cos(2 * np.pi * 5.0 * tc)).astype(F32)


def speech_case(hop, sr=SR):
    """(signal [63 hop], f0 float32 [64], 0 where unvoiced): 59 cosine harmonics of a moving F0 under four formant-like Lorentzians,
    voiced and unvoiced stretches, RandomState(1)."""
    rs = np.random.RandomState(1)
    n = hop * 63
    f0i = lambda t: 140.0 + 40.0 * np.sin(2 * np.pi * 0.9 * t) + 6.0 * np.sin(2 * np.pi * 5.0 * t)
    is_voiced = lambda t: np.sin(2 * np.pi * 1.3 * t + 0.3) > -0.5
    t = np.arange(n) / float(sr)
    f = f0i(t)
    ph = 2 * np.pi * np.cumsum(f / sr)
    x = np.zeros(n)
    for h in range(1, 60):
        w = sum(amp / (1.0 + ((h * f - c) / wd) ** 2) for amp, c, wd in LORENTZ) + 0.01
        x += w * np.cos(h * ph)
    v = is_voiced(t)
    sd = x[v].std()
    x = np.where(v, x, 0.3 * sd * rs.randn(n)) + 0.01 * sd * rs.randn(n)
    tc = np.arange(64) * hop / float(sr)
    return 0.8 * x / np.abs(x).max(), np.where(is_voiced(tc), f0i(tc), 0.0).astype(F32)


_VALUE = {}


def value_case(n_fft, hop, win, signal, mel, iters10=False):
    """dict(M float32 [64, NB] the target magnitudes, mel float32 [64, 80] or None, f0 float32 [64], phase_f0, phase_spsi, sc_f0_0,
    sc_spsi_0, wav_f0_0 the one-pass waveform from the F0 phase (float64 oracle throughout); with ``iters10`` also sc_f0_10, sc_spsi_10,
    sc_seed_5)."""
    key = (n_fft, hop, win, signal, bool(mel))
    if key not in _VALUE:
        from fastspeech2_amd.hparams import DotDict
        from fastspeech2_amd.vocoder import GriffinLim
        from tests import spsi_oracle as S
        st = O.Stft(n_fft, hop, win)
        sig, f0 = harmonic_case(hop) if signal == "harmonic" else speech_case(hop)
        M = np.abs(st.stft(sig))
        lm = None
        if mel:
            gl = GriffinLim(DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "n_mels": 80}}))
            lm = np.log(np.maximum(M @ gl._basis_np.T, 1e-5)).astype(F32)
            M = O.mel_to_mag(lm, gl._pinv_np)
        M = M.astype(F32)
        pf = f0_phase(f0, n_fft, hop, win, SR)
        ps = S.spsi_phase(M, n_fft, hop)
        wav = st.griffin_lim(M, pf, 0)
        sc = lambda w: st.spectral_convergence(M.astype(F64), w)
        _VALUE[key] = dict(M=M, mel=lm, f0=f0, phase_f0=pf, phase_spsi=ps, wav_f0_0=wav, sc_f0_0=sc(wav), sc_spsi_0=sc(st.griffin_lim(M, ps, 0)))
    c = _VALUE[key]
    if iters10 and "sc_f0_10" not in c:
        from fastspeech2_amd.vocoder import seed_angles
        st = O.Stft(n_fft, hop, win)
        sc = lambda angles, n: st.spectral_convergence(c["M"].astype(F64), st.griffin_lim(c["M"], angles, n))
        c.update(sc_f0_10=sc(c["phase_f0"], 10), sc_spsi_10=sc(c["phase_spsi"], 10), sc_seed_5=sc(seed_angles(0, 64, n_fft // 2 + 1), 5))
    return c


def pitch_true(f0_cmd, est_f0, n_fft, hop, f0_floor=71.0, f0_ceil=800.0):
    """(largest relative deviation on the frames that count, share of the interior frames left out because commanded and estimated
    voicing disagree, the deviations): the frames that count are commanded voiced, estimated voiced and pitch_oracle.interior."""
    from tests import pitch_oracle as P
    cmd = np.asarray(f0_cmd, F64)
    est = np.asarray(est_f0, F64)
    inner = P.interior(cmd.size, n_fft, hop)
    v_cmd, v_est = voiced_frames(f0_cmd, f0_floor, f0_ceil), est > 0
    counted = inner & v_cmd & v_est
    dev = np.abs(est[counted] / cmd[counted] - 1.0)
    left_out = (inner & (v_cmd != v_est)).sum() / max(int(inner.sum()), 1)
    return float(dev.max()) if dev.size else 0.0, float(left_out), dev
