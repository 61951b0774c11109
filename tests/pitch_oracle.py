"""Float64 numpy restatement of the autocorrelation F0 estimator of fastspeech2_amd.vocoder.pitch / wav_features (csrc/gl_pitch.h:
gl_features), and the synthetic signals its tests use.  The estimator is Boersma's 1993 autocorrelation method without the path
search, with parabolic peak interpolation; it is NOT the reference's pitch (pyworld's DIO, dataset/audio_processing.py:54-70).

Per frame of the analysis STFT (T // hop + 1 frames, reflect padding by n_fft / 2, periodic Hann of ``win`` samples centred in n_fft):
  r = irfft(|rfft(y)|^2), rw the same of the window, rho[t] = (r[t] / r[0]) / (rw[t] / rw[0]); r[0] <= 1e-12: unvoiced
  candidates: integer lags t in [tmin, tmax] = [floor(sr / f0_ceil), ceil(sr / f0_floor)] with rho[t] > rho[t-1], rho[t] >= rho[t+1],
  rho[t] > 0, refined with a = rho[t-1], c = rho[t], b = rho[t+1]: d = 0.5 (a - b) / (a - 2c + b), t* = t + d, p = c - 0.25 (a - b) d,
  S = p - octave_cost log2(f0_floor t* / sr); the winner is the largest S (ties: the smaller t); voiced iff p >= voicing_threshold;
  f0 = sr / t* where voiced else 0, strength = the winner's p (0 without a candidate).
Test infrastructure only (host tests and GPU tests compare against it)."""
import math
from typing import NamedTuple

import numpy as np

from tests.vocoder_oracle import hann_padded

DEFAULTS = dict(f0_floor=71.0, f0_ceil=800.0, voicing_threshold=0.45, octave_cost=0.02)


def lag_range(sr, win, f0_floor, f0_ceil):
    """(tmin, tmax); ValueError unless 2 <= tmin <= tmax <= win / 2."""
    tmin, tmax = int(math.floor(sr / f0_ceil)), int(math.ceil(sr / f0_floor))
    if tmin < 2 or tmax > win // 2 or tmin > tmax:
        raise ValueError("lags %d .. %d outside 2 .. %d (lowest usable floor %g)" % (tmin, tmax, win // 2, 2.0 * sr / win))
    return tmin, tmax


def frames_of(sig, n_fft, hop, win):
    """Windowed frames [T // hop + 1, n_fft] of ``sig`` as stft_magnitude cuts them; zeros for a signal of <= n_fft / 2 samples."""
    sig = np.asarray(sig, np.float64)
    L = sig.size // hop + 1
    if sig.size <= n_fft // 2:
        return np.zeros((L, n_fft))
    x = np.pad(sig, (n_fft // 2, n_fft // 2), mode="reflect")
    return np.stack([x[hop * f:hop * f + n_fft] for f in range(L)]) * hann_padded(n_fft, win)[None, :]


class Pitch(NamedTuple):
    f0: np.ndarray          # [frames] Hz, 0 = unvoiced
    strength: np.ndarray    # [frames] the winner's p, 0 without a candidate
    gap: np.ndarray         # [frames] best minus second-best S (inf with fewer than two candidates)
    voiced: np.ndarray      # [frames] bool


def pitch(sig, n_fft, hop, win, sr, f0_floor=71.0, f0_ceil=800.0, voicing_threshold=0.45, octave_cost=0.02):
    tmin, tmax = lag_range(sr, win, f0_floor, f0_ceil)
    y = frames_of(sig, n_fft, hop, win)
    L = y.shape[0]
    r = np.fft.irfft(np.abs(np.fft.rfft(y, axis=1)) ** 2, n=n_fft, axis=1)
    w = hann_padded(n_fft, win)
    rw = np.fft.irfft(np.abs(np.fft.rfft(w)) ** 2, n=n_fft)
    live = r[:, 0] > 1e-12
    lags = np.arange(tmin - 1, tmax + 2)
    rho = np.zeros((L, lags.size))
    rho[live] = (r[live][:, lags] / r[live, :1]) / (rw[lags] / rw[0])[None, :]
    a, c, b = rho[:, :-2], rho[:, 1:-1], rho[:, 2:]
    cand = (c > a) & (c >= b) & (c > 0) & live[:, None]
    den = np.where(cand, a - 2 * c + b, -1.0)
    d = 0.5 * (a - b) / den
    ts = lags[1:-1][None, :] + d
    p = c - 0.25 * (a - b) * d
    S = np.where(cand, p - octave_cost * np.log2(np.where(cand, f0_floor * ts / sr, 1.0)), -np.inf)
    best = np.argmax(S, axis=1)                 # the first of equal maxima: the smaller lag
    rows = np.arange(L)
    has = cand.any(axis=1)
    pw = np.where(has, p[rows, best], 0.0)
    voiced = has & (pw >= voicing_threshold)
    f0 = np.where(voiced, sr / ts[rows, best], 0.0)
    Ss = np.sort(S, axis=1)
    with np.errstate(invalid="ignore"):
        gap = np.where(cand.sum(axis=1) >= 2, Ss[:, -1] - Ss[:, -2], np.inf)
    return Pitch(f0, pw, gap, voiced)


# ---- signals with a known F0 ----
def _harmonics(phase, f_inst, sr, rs):
    """sum_{h = 1..8, h f < sr / 2} (0.5 / h) sin(h phase + phi_h), phi_h seeded."""
    x = np.zeros_like(phase)
    for h in range(1, 9):
        phi = rs.uniform(0, 2 * np.pi)
        x += np.where(h * f_inst < sr / 2, (0.5 / h) * np.sin(h * phase + phi), 0.0)
    return x


def const(f0, noise, sr, hop, n_hops=60, seed=0):
    """(signal, truth [frames]): harmonics of a constant f0 plus ``noise`` x white Gaussian noise, peak 0.8."""
    rs = np.random.RandomState(seed)
    n = n_hops * hop
    t = np.arange(n) / sr
    x = _harmonics(2 * np.pi * f0 * t, np.full(n, float(f0)), sr, rs) + noise * rs.randn(n)
    return 0.8 * x / np.abs(x).max(), np.full(n // hop + 1, float(f0))


def glide(fa, fb, sr, hop, n_hops=120, seed=0, noise=0.02):
    """(signal, truth [frames]): the same harmonics on an exponential sweep fa -> fb; truth is the F0 at each frame's centre."""
    rs = np.random.RandomState(seed)
    n = n_hops * hop
    t = np.arange(n) / sr
    dur = n / sr
    k = math.log(fb / fa) / dur
    f = fa * np.exp(k * t)
    phase = 2 * np.pi * fa * (np.exp(k * t) - 1.0) / k
    x = _harmonics(phase, f, sr, rs) + noise * rs.randn(n)
    return 0.8 * x / np.abs(x).max(), fa * np.exp(k * np.arange(n // hop + 1) * hop / sr)


def white(amp, sr, hop, n_hops, seed=0):
    return amp * np.random.RandomState(seed).randn(n_hops * hop)


MIXED_SEG = 40          # hops per segment
MIXED_LABELS = (False, True, False, True, False)


def mixed(sr, hop, seed=0):
    """Five segments of 40 hops: silence, const(180, 0.01), 0.2 x white noise, glide(150, 260), silence."""
    n = MIXED_SEG * hop
    return np.concatenate([np.zeros(n), const(180.0, 0.01, sr, hop, MIXED_SEG, seed)[0], white(0.2, sr, hop, MIXED_SEG, seed + 1),
                           glide(150.0, 260.0, sr, hop, MIXED_SEG, seed + 2)[0], np.zeros(n)])


def margin(n_fft, hop):
    return -(-n_fft // (2 * hop)) + 1


def interior(n_frames, n_fft, hop):
    """bool [frames]: False on margin(n_fft, hop) frames at each end."""
    m = margin(n_fft, hop)
    ok = np.zeros(n_frames, bool)
    ok[m:n_frames - m] = True
    return ok


def mixed_interior(n_fft, hop):
    """(bool [frames] interior, bool [frames] label) of ``mixed``: frames within margin(n_fft, hop) of a segment boundary (the
    waveform's ends included) are not interior."""
    m = margin(n_fft, hop)
    f = np.arange(len(MIXED_LABELS) * MIXED_SEG + 1)
    near = np.minimum(f % MIXED_SEG, MIXED_SEG - f % MIXED_SEG) <= m
    label = np.asarray(MIXED_LABELS)[np.minimum(f // MIXED_SEG, len(MIXED_LABELS) - 1)]
    return ~near, label


# (name, n_fft, hop, win, sample rate, pitch options, lowest F0 of the signals)
GEOMS = [("1024_256_1024", 1024, 256, 1024, 22050, {}, 0.0),
         ("2048_300_1200", 2048, 300, 1200, 24000, {}, 0.0),
         ("1024_200_800", 1024, 200, 800, 22050, {}, 0.0),
         ("512_160_400", 512, 160, 400, 22050, dict(f0_floor=110.4), 130.0)]
CONST_F0 = (80, 95, 110, 155.3, 220, 311.7, 440, 523.3, 620, 700, 790)
CONST_NOISE = (0.0, 0.05)
GLIDES = ((90, 300), (120, 400), (200, 600))


def signals(geom):
    """[(label, signal, truth [frames])] of one geometry: the const and glide cases whose F0 stays at or above the geometry's lowest."""
    _, n_fft, hop, win, sr, opt, lo = geom
    out = []
    for i, f0 in enumerate(CONST_F0):
        if f0 >= lo:
            for nz in CONST_NOISE:
                out.append(("const_%g_%g" % (f0, nz),) + const(f0, nz, sr, hop, seed=17 * i + int(nz * 100) + 1))
    for i, (fa, fb) in enumerate(GLIDES):
        if fa >= lo:
            out.append(("glide_%g_%g" % (fa, fb),) + glide(fa, fb, sr, hop, seed=100 + i))
    return out


def packed_cases(geom):
    """[(label, [three float32 waveforms])] the GPU tests pack per call: every signal of ``signals`` plus 0.3 x white noise (200 hops),
    zeros and ``mixed``; each with a cut of itself that starts and ends off the hop grid and with n_fft / 2 samples of itself (too short
    for the reflect padding).  The seeds of ``signals`` are fixed such that the oracle alone leaves at most 1 % of a case's frames
    with a best-two gap or a distance to the voicing threshold below 1e-4 (tests/test_pitch_host.py checks that here, on the CPU)."""
    _, n_fft, hop, win, sr, _, _ = geom
    sigs = [(label, sig) for label, sig, _ in signals(geom)]
    sigs += [("white", white(0.3, sr, hop, 200, seed=5)), ("zeros", np.zeros(60 * hop)), ("mixed", mixed(sr, hop))]
    out = []
    for i, (label, sig) in enumerate(sigs):
        x = sig.astype(np.float32)
        cut, off = (len(x) // hop * 2 // 3) * hop + 13 + 7 * (i % 5), 3 * hop + 5
        out.append((label, [x, x[off:off + cut].copy(), x[hop:hop + n_fft // 2].copy()]))
    return out


def pitch_packed(waves, geom):
    """The oracle on each waveform of a packed case, concatenated as the kernel packs its frames."""
    _, n_fft, hop, win, sr, opt, _ = geom
    rs = [pitch(w.astype(np.float64), n_fft, hop, win, sr, **opt) for w in waves]
    return Pitch(*[np.concatenate([getattr(r, k) for r in rs]) for k in Pitch._fields])


def compared(o, gap_min=1e-4, threshold=0.45):
    """bool [frames]: frames a float32 implementation is held to -- the oracle's two best candidates, and its winner and the voicing
    threshold, are at least ``gap_min`` apart."""
    return (o.gap >= gap_min) & (np.abs(o.strength - threshold) >= gap_min)
