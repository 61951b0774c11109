"""Numpy statement of the phase-continuity initial phase (SPSI: Beauregard, Harish and Wyse, "Single Pass Spectrogram Inversion", 2015)
as csrc/gl_spsi.h computes it, in float32 with every operation rounded on its own, plus a literal sequential
transcription of the published algorithm to check the closed form against.  Test infrastructure only.

Closed form, per utterance: phases in turns, state acc[NB] = 0 before frame 0.  For the row m of frame t:
  peak j (1 <= j <= NB - 2): m[j] > m[j-1] and m[j] > m[j+1]; a non-peak bin b is rising iff m[b] < m[b+1], falling iff m[b] < m[b-1]
  owner of a non-peak bin: the nearest peak to its right if every bin from it up to that peak is rising, else the nearest peak to its
  left if every bin from it down to that peak is falling, else none; bins 0 and NB - 1 have none; a peak owns itself
  peak: a, b, c = m[j-1], m[j], m[j+1]; den = (a - 2 b) + c; p = den != 0 ? (0.5 (a - c)) / den : 0;
        w = float((hop j) mod n_fft) / n_fft + p float(hop / n_fft); pk = acc[j] + w; pk -= floor(pk); right = c > a
  owned bin k of peak j, d = k - j: new[k] = pk + h, - 1 if >= 1; h = 0.5 if (right and (d == 1 or d < 0)) or (not right and
        (d == -1 or d > 0)), else 0
  unowned: new[k] = acc[k].  acc <- new; phase[t] = acc * 6.28318548f."""
import numpy as np

F32 = np.float32
UNOWNED = -1


def owners(m):
    """(owner [NB] int, UNOWNED where none; half [NB] bool: the bin is shifted by half a turn; right [NB] bool at peaks) of one row."""
    m = np.asarray(m, F32)
    NB = m.size
    own = np.full(NB, UNOWNED, np.int64)
    right = np.zeros(NB, bool)
    peaks = [j for j in range(1, NB - 1) if m[j] > m[j - 1] and m[j] > m[j + 1]]
    for j in peaks:
        own[j] = j
        right[j] = bool(m[j + 1] > m[j - 1])
    for j in peaks:                       # left-owned first, so that the right owner of a shared valley overwrites it
        k = j + 1
        while k <= NB - 2 and own[k] != k and m[k] < m[k - 1]:
            own[k] = j
            k += 1
    for j in peaks:
        k = j - 1
        while k >= 1 and m[k] < m[k + 1]:
            own[k] = j
            k -= 1
    half = np.zeros(NB, bool)
    for k in range(NB):
        j = own[k]
        if j == UNOWNED or j == k:
            continue
        d = k - j
        half[k] = (d == 1 or d < 0) if right[j] else (d == -1 or d > 0)
    return own, half, right


def peak_advance(m, j, n_fft, hop):
    """w of the peak j of row m (float32, one rounding per operation)."""
    a, b, c = F32(m[j - 1]), F32(m[j]), F32(m[j + 1])
    with np.errstate(all="ignore"):
        den = F32(F32(a - F32(F32(2) * b)) + c)
        p = F32(F32(F32(0.5) * F32(a - c)) / den) if den != 0 else F32(0)
        return F32(F32(F32((hop * j) % n_fft) / F32(n_fft)) + F32(p * F32(hop / n_fft)))


def spsi_turns(M, n_fft, hop):
    """acc after every frame [L, NB] float32 (turns) for one utterance's magnitudes M [L, NB]."""
    M = np.asarray(M, F32)
    L, NB = M.shape
    assert NB == n_fft // 2 + 1
    acc = np.zeros(NB, F32)
    out = np.zeros((L, NB), F32)
    for t in range(L):
        m = M[t]
        own, half, _ = owners(m)
        new = acc.copy()
        pk = {}
        for j in np.flatnonzero(own == np.arange(NB)):
            v = F32(acc[j] + peak_advance(m, j, n_fft, hop))
            pk[j] = F32(v - np.floor(v))
        for k in range(NB):
            j = own[k]
            if j == UNOWNED:
                continue
            v = F32(pk[j] + (F32(0.5) if half[k] else F32(0)))
            new[k] = F32(v - F32(1)) if v >= F32(1) else v
        acc = new
        out[t] = acc
    return out


def spsi_phase(M, n_fft, hop):
    """The initial phase [L, NB] float32 in radians, [0, 2 pi)."""
    return (spsi_turns(M, n_fft, hop) * F32(6.28318548)).astype(F32)


def spsi_batch(src, starts, lens, n_fft, hop):
    """Phase in the row layout of src [rows, NB]: utterance b = rows [starts[b], starts[b] + lens[b]); zeros elsewhere."""
    src = np.asarray(src, F32)
    out = np.zeros_like(src)
    for s, n in zip(starts, lens):
        if n > 0:
            out[s:s + n] = spsi_phase(src[s:s + n], n_fft, hop)
    return out


def spsi_published(M, n_fft, hop):
    """The published sequential algorithm (Beauregard et al. 2015, listing 1), float64, in place on one accumulator, radians; returned
    in turns mod 1 [L, NB].  Bins 0 and NB - 1 are whatever the listing's unconditional neighbour writes leave there."""
    M = np.asarray(M, np.float64)
    L, NB = M.shape
    acc = np.zeros(NB)
    out = np.zeros((L, NB))
    for t in range(L):
        mag = M[t]
        for j in range(1, NB - 1):
            if mag[j] > mag[j - 1] and mag[j] > mag[j + 1]:
                alpha, beta, gamma = mag[j - 1], mag[j], mag[j + 1]
                denom = alpha - 2 * beta + gamma
                p = 0.5 * (alpha - gamma) / denom if denom != 0 else 0.0
                acc[j] += hop * 2 * np.pi * (j + p) / n_fft
                peak = acc[j]
                if p > 0:
                    acc[j + 1] = peak + np.pi
                    b = j - 1
                    while b > 0 and mag[b] < mag[b + 1]:
                        acc[b] = peak + np.pi
                        b -= 1
                    b = j + 2
                    while b < NB - 1 and mag[b] < mag[b - 1]:
                        acc[b] = peak
                        b += 1
                else:
                    acc[j - 1] = peak + np.pi
                    b = j + 1
                    while b < NB - 1 and mag[b] < mag[b - 1]:
                        acc[b] = peak + np.pi
                        b += 1
                    b = j - 2
                    while b > 0 and mag[b] < mag[b + 1]:
                        acc[b] = peak
                        b -= 1
        out[t] = np.mod(acc / (2 * np.pi), 1.0)
    return out


def wrapped_diff(a, b):
    """|a - b| on the circle of circumference 1."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 1.0
    return np.minimum(d, 1.0 - d)


# ---- the cases the host, stand-in and GPU tests share ----
def crafted_rows(NB, seed=5):
    """dict name -> row [NB] float32: the rows at which the owner rule can go wrong."""
    rs = np.random.RandomState(seed)
    base = (rs.rand(NB).astype(F32) + F32(0.1))
    rows = {}
    r = np.full(NB, 0.25, F32); r[1] = 2.0; r[0] = 0.5; r[2] = 0.125
    rows["peak_at_bin_1"] = r
    r = np.full(NB, 0.25, F32); r[NB - 2] = 2.0; r[NB - 1] = 0.5; r[NB - 3] = 0.125
    rows["peak_at_bin_NB-2"] = r
    r = np.full(NB, 0.0, F32); r[10:17] = [1, 3, 2, 0.5, 1.5, 4, 1]          # peaks 11 and 15, valley 13
    rows["two_peaks_sharing_a_valley"] = r
    r = base.copy(); r[20:27] = [0.2, 0.2, 0.6, 2.0, 0.7, 0.7, 0.3]           # plateau on each side of the peak 23
    rows["plateau_next_to_a_peak"] = r
    rows["monotone"] = np.linspace(0.0, 1.0, NB).astype(F32)
    rows["all_zero"] = np.zeros(NB, F32)
    r = base.copy(); r[40] = np.nan; r[41] = 0.5; r[50] = np.inf; r[60] = np.nan; r[61] = np.inf
    rows["nan_and_inf"] = r
    return rows


def crafted_utterance(NB, seed=5):
    """[10, NB]: a random row, every crafted row (one of them twice in a row: a row equal to its predecessor), the first row again."""
    rs = np.random.RandomState(seed + 1)
    c = crafted_rows(NB, seed)
    first = rs.rand(NB).astype(F32)
    rows = [first, c["peak_at_bin_1"], c["peak_at_bin_NB-2"], c["two_peaks_sharing_a_valley"], c["two_peaks_sharing_a_valley"],
            c["plateau_next_to_a_peak"], c["monotone"], c["all_zero"], c["nan_and_inf"], first]
    return np.stack(rows).astype(F32)


BATCH_LENS = (1, 2, 3, 4, 5, 31, 32, 33, 65, 0, 7)


def random_rows(L, NB, seed):
    """Spectrum-like random rows: a smooth envelope times noise, so that runs of several rising / falling bins occur."""
    rs = np.random.RandomState(seed)
    x = rs.rand(L, NB + 8)
    sm = sum(x[:, i:i + NB] for i in range(8)) / 8.0
    return (sm * (0.2 + rs.rand(L, NB)) ** 2).astype(F32)


def batch_case(NB, lens=BATCH_LENS, seed=11, padded=False):
    """(src [rows, NB], starts, lens): random utterances with the crafted utterance's rows written over the head of the longest ones.
    padded: utterance b at row b * max(lens), the rows no utterance covers filled with a canary the kernels must not read into a result."""
    lens = list(lens)
    Lmax = max(lens)
    starts = [b * Lmax for b in range(len(lens))] if padded else list(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int))
    rows = Lmax * len(lens) if padded else sum(lens)
    src = np.full((rows, NB), 7.5, F32)
    craft = crafted_utterance(NB)
    for b, (s, n) in enumerate(zip(starts, lens)):
        u = random_rows(n, NB, seed + b)
        if n >= 31:
            u[3:3 + craft.shape[0]] = craft
        elif n > 0:
            u[:min(n, craft.shape[0])] = craft[b % 3:b % 3 + min(n, craft.shape[0])][:n]
        src[s:s + n] = u
    return src, starts, lens


# ---- what the initial phase is for: fewer Griffin-Lim iterations (host and GPU tests share the case and the oracle's figures) ----
_CONV = {}


def convergence_case(n_fft, hop, win, mel):
    """dict(M float32 [L, NB] the target magnitudes, mel float32 [L, 80] or None, phase = spsi_phase(M), sc_spsi10, sc_seed20) for
    harmonic_signal(hop 63, seed=1, noise=0.01): the spectral convergence (tests/vocoder_oracle.py) of 10 iterations from the SPSI
    phase and of 20 from seed_angles(0, L).  mel: M goes through 80 mels and the pseudo-inverse first."""
    key = (n_fft, hop, win, bool(mel))
    if key not in _CONV:
        from fastspeech2_amd.hparams import DotDict
        from fastspeech2_amd.vocoder import GriffinLim, seed_angles
        from tests import vocoder_oracle as O
        st = O.Stft(n_fft, hop, win)
        M = np.abs(st.stft(O.harmonic_signal(hop * 63, seed=1, noise=0.01)))
        lm = None
        if mel:
            gl = GriffinLim(DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "n_mels": 80}}))
            lm = np.log(np.maximum(M @ gl._basis_np.T, 1e-5)).astype(F32)
            M = O.mel_to_mag(lm, gl._pinv_np)
        M = M.astype(F32)
        ph = spsi_phase(M, n_fft, hop)
        sc = lambda angles, n: st.spectral_convergence(M.astype(np.float64), st.griffin_lim(M, angles, n))
        _CONV[key] = dict(M=M, mel=lm, phase=ph, sc_spsi10=sc(ph, 10), sc_seed20=sc(seed_angles(0, M.shape[0], n_fft // 2 + 1), 20))
    return _CONV[key]
