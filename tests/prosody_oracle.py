"""numpy statements of csrc/prosody.h -- the per-phoneme means of a per-frame track (label_means) and the control of the predicted
pitch / energy rows (prosody_apply) -- and the cases both the host stand-in (tests/test_prosody_kernel_host.py) and the device
(tests/test_gpu_prosody.py) are held to.  Both statements perform the kernels' IEEE operations in the kernels' order (a float64 sum in
frame order and one division; a float32 product, then a float32 sum), so the bar is EQUALITY."""
import numpy as np

B = 4
TMAXES = (1, 63, 64, 65, 130)
STRIDES = (1, 7, 300)
GARBAGE = (-1, 10 ** 6)


def label_means(x, labels, lens, n_labels, positive_only=False):
    """-> (mean float32 [B, n_labels], count int32 [B, n_labels])."""
    x, labels = np.asarray(x, np.float32), np.asarray(labels, np.int32)
    nb, S = x.shape
    mean, count = np.zeros((nb, n_labels), np.float32), np.zeros((nb, n_labels), np.int32)
    for b in range(nb):
        n = min(max(int(lens[b]), 0), S)
        lab = labels[b, :n]
        for t in range(n_labels):
            first, last = int(np.searchsorted(lab, t, "left")), int(np.searchsorted(lab, t, "right"))
            s, c = np.float64(0.0), 0
            for j in range(first, last):
                v = x[b, j]
                if not positive_only or v > 0:
                    s = s + np.float64(v)
                    c += 1
            if c:
                mean[b, t] = np.float32(s / np.float64(c))
            count[b, t] = c
    return mean, count


class MeansCase:
    """B = 4 utterances of 0, 1, x_stride and a random number of valid frames.  Utterance 1: one frame; utterance 2: ONE phoneme owns
    every frame; utterance 3: a sorted draw from [0, Tmax), which skips phonemes (count 0) and repeats others.  Behind the valid
    frames: garbage labels (-1, 10^6) and values that must not be read.  The values hold zeros and negatives in every longer run."""

    def __init__(self, Tmax, S, seed=0):
        rng = np.random.default_rng(1000 * Tmax + S + seed)
        self.Tmax, self.S = Tmax, S
        self.lens = np.asarray([0, 1, S, int(rng.integers(0, S + 1))], np.int64)
        self.x = rng.normal(100.0, 80.0, (B, S)).astype(np.float32)
        self.x[rng.random((B, S)) < 0.25] = 0.0
        self.labels = np.empty((B, S), np.int32)
        for b in range(B):
            n = int(self.lens[b])
            if b == 2:
                self.labels[b, :n] = Tmax - 1 if Tmax % 2 else Tmax // 2
            else:
                self.labels[b, :n] = np.sort(rng.integers(0, Tmax, n))
            self.labels[b, n:] = np.resize(np.asarray(GARBAGE, np.int32), S - n)
            self.x[b, n:] = np.float32(1e30)

    def oracle(self, positive_only):
        return label_means(self.x, self.labels, self.lens, self.Tmax, positive_only)


_cases = {}


def means_case(Tmax, S):
    if (Tmax, S) not in _cases:
        c = MeansCase(Tmax, S)
        c.want = {po: c.oracle(po) for po in (False, True)}
        _cases[(Tmax, S)] = c
    return _cases[(Tmax, S)]


def check_means_case(c):
    """What the case is there for, asserted on the oracle's side."""
    mean, count = c.want[False]
    assert count[0].sum() == 0 and not mean[0].any()                                  # lens 0: nothing counted, whatever lies behind
    assert count[1].sum() == 1 and count[2].max() == c.S == count[2].sum()            # lens 1; one phoneme owns every frame
    assert np.array_equal(count.sum(1), c.lens)
    if c.Tmax > 1:
        assert (count[1:] == 0).any()                                                 # skipped phonemes
    voiced = c.want[True][1]
    assert np.all(voiced <= count) and (c.S < 7 or (voiced < count).any())            # zeros / negatives inside a run were left out
    assert np.all(np.abs(mean) < 1e4) and np.all(c.want[True][0] >= 0)                # nothing from behind the valid frames


def apply_control(v, row_pos, row_seq, lri, scale, shift):
    """v [R] float32 -> v' [R]: fl32(fl32(v * scale) + shift) on the rows with row_pos >= 0 and lri >= 0; scale / shift: None or
    float32 [B, cols], cols 1 (per utterance) or Tmax (per phoneme)."""
    out = np.asarray(v, np.float32).copy()
    for row in range(len(out)):
        t, b = int(lri[row]), int(row_seq[row])
        if row_pos[row] < 0 or t < 0:
            continue
        sc = np.float32(1.0) if scale is None else scale[b, 0 if scale.shape[1] == 1 else t]
        sh = np.float32(0.0) if shift is None else shift[b, 0 if shift.shape[1] == 1 else t]
        out[row] = np.float32(np.float32(out[row] * sc) + sh)
    return out


class ApplyCase:
    """A packed row image as fs2_decode builds it: 3 utterances of 300 / 1 / 37 frames from 9 / 1 / 5 phonemes, starts aligned to 32 rows
    with gap rows (row_pos = -1) between and behind them (more than one block of 256 rows), and a few valid rows without a phoneme
    (lri = -1).  The values of the gap rows are NaN patterns that must come back unchanged."""

    def __init__(self, seed=3):
        rng = np.random.default_rng(seed)
        self.B, self.Tmax = 3, 9
        frames, toks = (300, 1, 37), (9, 1, 5)
        self.R = 448
        self.row_pos, self.row_seq, self.lri = (np.full(self.R, -1, np.int32) for _ in range(3))
        start = 0
        for b, (n, T) in enumerate(zip(frames, toks)):
            self.row_pos[start:start + n], self.row_seq[start:start + n] = np.arange(n), b
            self.lri[start:start + n] = np.sort(rng.integers(0, T, n))
            start = (start + n + 8 + 31) // 32 * 32
        assert start <= self.R
        valid = np.flatnonzero(self.row_pos >= 0)
        self.no_phoneme = valid[[5, 299, 301]]
        self.lri[self.no_phoneme] = -1
        self.p = rng.uniform(60, 700, self.R).astype(np.float32)
        self.e = rng.normal(0, 3, self.R).astype(np.float32)
        self.p[self.row_pos < 0] = np.float32(np.nan)
        self.e[self.row_pos < 0] = np.float32(np.nan)
        ctl = lambda cols, lo, hi: rng.uniform(lo, hi, (self.B, cols)).astype(np.float32)
        per_utt, per_tok = 1, self.Tmax
        # name -> (pitch_scale, pitch_shift, energy_scale, energy_shift): cols mixed across the four, and each of the four alone
        self.controls = {
            "mixed_a": (ctl(per_utt, 0.5, 2), ctl(per_tok, -50, 50), ctl(per_tok, 0.5, 2), ctl(per_utt, -1, 1)),
            "mixed_b": (ctl(per_tok, 0.5, 2), ctl(per_utt, -50, 50), ctl(per_utt, 0.5, 2), ctl(per_tok, -1, 1)),
            "pitch_scale": (ctl(per_tok, 0.5, 2), None, None, None),
            "pitch_shift": (None, ctl(per_utt, -50, 50), None, None),
            "energy_scale": (None, None, ctl(per_utt, 0.5, 2), None),
            "energy_shift": (None, None, None, ctl(per_tok, -1, 1)),
        }

    def oracle(self, name):
        ps, ph, es, eh = self.controls[name]
        return (apply_control(self.p, self.row_pos, self.row_seq, self.lri, ps, ph),
                apply_control(self.e, self.row_pos, self.row_seq, self.lri, es, eh))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
