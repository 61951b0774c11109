"""The loss terms of fs2_op_loss_terms (include/fs2.h, csrc/losses.h) restated in numpy float64: the
per-utterance record, the batch record, and what ``LossTerms.report`` / ``LossTerms.evaluate`` make of them.  Every difference is
formed in float64 from the float32 / int64 inputs (exact), and numpy's own summation order is used: the kernels are held to these
numbers at the bar of a reordered double sum (tests/test_losses_kernel_host.py states it).  TEST INFRASTRUCTURE ONLY.

Also the edge batch that the host stand-in and the GPU tests share."""
import numpy as np

TERMS = 20            # include/fs2.h: FS2_LOSS_TERMS
REPORT_NAMES = ("l1_loss", "before_loss", "after_loss", "duration_loss", "energy_loss", "pitch_loss", "loss")
D = np.float64


def record(before, after, ys, d_outs, ds, e_outs, es, p_outs, ps, ilen, olen, Tmax, Lmax, pads=True):
    """The record of one utterance from its rows: before / after / ys [>= Lmax, odim], d_outs / ds [>= Tmax], e / p [>= Lmax]."""
    r = np.zeros(TERMS, D)
    r[:4] = ilen, olen, Tmax - ilen, Lmax - olen

    def sums(f, t):
        dm_b = np.abs(before[f].astype(D) - ys[f].astype(D)).sum()
        dm_a = np.abs(after[f].astype(D) - ys[f].astype(D)).sum()
        dd = d_outs[t].astype(D) - np.log(ds[t].astype(D) + 1.0)
        de = e_outs[f].astype(D) - es[f].astype(D)
        dp = p_outs[f].astype(D) - ps[f].astype(D)
        return dm_b, dm_a, (dd * dd).sum(), (de * de).sum(), (dp * dp).sum(), de, dp

    f, t = slice(0, olen), slice(0, ilen)
    r[4], r[5], r[6], r[7], r[8], de, dp = sums(f, t)
    r[9] = np.abs(d_outs[t].astype(D) - ds[t].astype(D)).sum()        # evaluation.py:31: log-domain output against linear durations
    r[10], r[11] = np.abs(de).sum(), np.abs(dp).sum()
    if pads:
        r[12], r[13], r[14], r[15], r[16], _, _ = sums(slice(olen, Lmax), slice(ilen, Tmax))
    return r


def records(before, after, ys, d_outs, ds, e_outs, es, p_outs, ps, ilens, olens, Tmax=None, Lmax=None, pads=True):
    """[B, 20] records of a padded batch and the batch record (the column sums)."""
    B = len(ilens)
    Tmax = int(max(ilens)) if Tmax is None else Tmax
    Lmax = int(max(olens)) if Lmax is None else Lmax
    rows = np.stack([record(before[b], after[b], ys[b], d_outs[b], ds[b], e_outs[b], es[b], p_outs[b], ps[b], int(ilens[b]), int(olens[b]),
                            Tmax, Lmax, pads) for b in range(B)]) if B else np.zeros((0, TERMS), D)
    return rows, rows.sum(axis=0)


def report(batch, odim, use_masking=True, use_weighted_masking=False):
    """The reference's seven report values (fastspeech.py:280-333) from a batch record, in its order."""
    if use_masking and use_weighted_masking:
        raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got 2)")
    b = np.asarray(batch, D)
    if use_masking:
        frames, tokens = b[1], b[0]
        bl, al, dl, el, pl = b[4] / (frames * odim), b[5] / (frames * odim), b[6] / tokens, b[7] / frames, b[8] / frames
    else:
        frames, tokens = b[1] + b[3], b[0] + b[2]
        bl, al = (b[4] + b[12]) / (frames * odim), (b[5] + b[13]) / (frames * odim)
        dl, el, pl = (b[6] + b[14]) / tokens, (b[7] + b[15]) / frames, (b[8] + b[16]) / frames
    l1 = bl + al
    if use_weighted_masking:
        l1 = l1 / odim          # the weights multiply the already reduced scalar and sum to 1 / odim; duration's sum to 1
    return list(zip(REPORT_NAMES, (l1, bl, al, dl, el, pl, l1 + dl + el + pl)))


def evaluate(rows):
    """evaluation.py:12-41 for the same utterances fed one at a time: (pitch, energy, dur)."""
    rows = np.asarray(rows, D)
    return (float(np.mean(rows[:, 11] / rows[:, 1])), float(np.mean(rows[:, 10] / rows[:, 1])), float(np.mean(rows[:, 9] / rows[:, 0])))


class Edge:
    """The edge batch: tiles of K frames -- olens 1, 2, K - 1, K, K + 1, 3 K + 5, ilens 1 .. 64, target strides wider than the
    predictions', Lmax above max olens, some zero durations, exact zeros in es / ps.  Random float32 data, pads included."""

    def __init__(self, K, odim=80, seed=7):
        rng = np.random.default_rng([seed, K, odim])
        self.K, self.odim = K, odim
        self.olens = np.asarray([1, 2, K - 1, K, K + 1, 3 * K + 5], np.int32)
        self.ilens = np.asarray([1, 2, 7, 16, 33, 64], np.int32)
        self.B = B = 6
        self.Tmax, self.Lmax = 64, 3 * K + 9
        self.psf, self.ysf, self.pst, self.dst, self.tsf = self.Lmax + 1, self.Lmax + 6, 64, 71, self.Lmax + 3
        f = lambda *s: rng.normal(0.0, 1.0, s).astype(np.float32)
        self.before, self.after, self.ys = f(B, self.psf, odim), f(B, self.psf, odim), f(B, self.ysf, odim)
        self.d_outs = f(B, self.pst)
        self.ds = rng.integers(0, 12, (B, self.dst)).astype(np.int64)
        self.ds[:, 3::5] = 0
        self.e_outs, self.p_outs = f(B, self.psf), f(B, self.psf)
        self.es = rng.uniform(0.0, 130.5, (B, self.tsf)).astype(np.float32)
        self.ps = rng.uniform(71.0, 676.0, (B, self.tsf)).astype(np.float32)
        self.ps[rng.uniform(size=self.ps.shape) < 0.3] = 0.0
        self.es[:, 1::7] = 0.0
        self.rows, self.batch = records(*self.tensors(), self.ilens, self.olens, self.Tmax, self.Lmax, pads=True)

    def tensors(self):
        return (self.before, self.after, self.ys, self.d_outs, self.ds, self.e_outs, self.es, self.p_outs, self.ps)

    def largest_n(self):
        """Terms of the largest sum of the batch record (the mel sums over valid plus pad frames are separate sums)."""
        return int(max(self.olens.sum(), self.B * self.Lmax - self.olens.sum()) * self.odim)


def close(got, want, rel=1e-12, floor=1e-300):
    """|got - want| <= rel |want| + floor, elementwise; NaN only where NaN."""
    got, want = np.asarray(got, D), np.asarray(want, D)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= rel * np.abs(want[ok]) + floor))
