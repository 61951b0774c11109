"""Validation losses of the teacher-forced forward on the MI355X (csrc/losses.h, include/fs2.h: fs2_op_loss_terms; DESIGN.md
section 14.5).

The reference reduces the outputs of ``FeedForwardTransformer._forward`` and the targets twice: ``forward()`` to seven batch
scalars (fastspeech.py:280-333: a dozen ``masked_select`` copies, five float32 means, seven ``.item()`` calls), and
``evaluation.py`` to the mean L1 of duration, energy and pitch, one utterance and three ``.item()`` calls at a time.  ``loss_terms``
makes one pass over the same tensors instead and leaves a record of sums per utterance (``FS2_LOSS_TERMS`` doubles) plus their
batch record on the device; ``LossTerms`` turns the records into the reference's numbers on the host, in float64:
``report()`` (the seven values, under any of the reference's masking switches), ``evaluate()`` (evaluation.py's three),
``per_utterance()`` (a breakdown the reference does not have) and ``merge()`` (batches, ranks).

Every difference is formed in double from the float32 / int64 inputs and every sum is carried in double in a fixed order: an
utterance's sums over its own frames and tokens do not depend on the batch it is in, on its place there, on the padding or on a
stride.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._host import _i32, _lens, _require_cuda, _stream

TERMS = _lib.LOSS_TERMS
REPORT_NAMES = ("l1_loss", "before_loss", "after_loss", "duration_loss", "energy_loss", "pitch_loss", "loss")
# index of a record (include/fs2.h)
ILEN, OLEN, PAD_TOKENS, PAD_FRAMES, BEFORE_L1, AFTER_L1, DUR_SQ, ENERGY_SQ, PITCH_SQ, DUR_L1, ENERGY_L1, PITCH_L1 = range(12)
PAD_BEFORE_L1, PAD_AFTER_L1, PAD_DUR_SQ, PAD_ENERGY_SQ, PAD_PITCH_SQ = range(12, 17)


class DeviceRecords:
    """The records of a batched operator, ``terms`` [B, TERMS], and their batch record ``batch`` [TERMS] (float64 numpy): the base of
    :class:`LossTerms`, ``dtw.DtwTerms`` and ``align.Alignment``, which set ``TERMS``.  An operator leaves them on the device as ONE
    tensor ``_device`` [B + 1, TERMS] float64 -- the records, then the batch record -- and the first read of either fetches them with one
    copy, which waits for the stream."""
    TERMS = None

    def __init__(self, terms, batch, _device=None):
        self._terms = None if terms is None else np.asarray(terms, np.float64).reshape(-1, self.TERMS)
        self._batch = None if batch is None else np.asarray(batch, np.float64).reshape(self.TERMS)
        self._device = _device

    @classmethod
    def _on_device(cls, B, dev):
        """-> (an empty ``_device`` tensor for B records, the address of its records -- None for B = 0 --, that of its batch record)"""
        rec = torch.empty(B + 1, cls.TERMS, dtype=torch.float64, device=dev)
        return rec, rec.data_ptr() if B else None, rec[B].data_ptr()

    def _fetch(self):
        if self._device is not None:
            host = self._device.cpu().numpy()
            self._terms, self._batch, self._device = host[:-1], host[-1], None

    @property
    def terms(self):
        self._fetch()
        return self._terms

    @property
    def batch(self):
        self._fetch()
        return self._batch

    def __len__(self):
        return int(self._device.shape[0] - 1 if self._device is not None else self._terms.shape[0])

    def _synced(self, sync):
        if sync:
            self._fetch()
        return self


class LossTerms(DeviceRecords):
    """The per-utterance records ``terms`` [B, 20] and their batch record ``batch`` [20] (float64 numpy; include/fs2.h lists the
    indices).  After ``loss_terms(..., sync=False)`` both are still on the device; the first read of either fetches them with one
    copy, which waits for the stream.  ``pads`` tells whether the pad sums (indices 12 .. 16) were built; ``odim`` is the number of
    mel bins behind the two mel sums."""
    TERMS = TERMS

    def __init__(self, terms, batch, pads, odim, _device=None):
        super().__init__(terms, batch, _device)
        self.pads, self.odim = bool(pads), odim

    def report(self, use_masking=True, use_weighted_masking=False, odim=None):
        """The reference's seven ``(name, value)`` pairs (fastspeech.py:326-334), in its order, in float64 from the batch record.
        Masked: sum / count over the valid frames and tokens.  Unmasked: (valid + pad sum) / (B Lmax odim), (B Tmax) and (B Lmax).
        ``use_weighted_masking`` as the reference actually computes it (fastspeech.py:308-325): the weights multiply the already
        reduced scalars and sum to 1 / odim (l1_loss) and to 1 (duration_loss), so l1_loss becomes (before + after) / odim and
        nothing else changes.  Both switches together raise the reference's IndexError (its ``ys.size(2)`` of the 1-D selection)."""
        if use_masking and use_weighted_masking:
            raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got 2)")
        odim = self.odim if odim is None else odim
        if odim is None:
            raise ValueError("report() needs odim (these terms were merged or built without it)")
        b = self.batch
        with np.errstate(divide="ignore", invalid="ignore"):
            if use_masking:
                frames, tokens = b[OLEN], b[ILEN]
                bl, al = b[BEFORE_L1] / (frames * odim), b[AFTER_L1] / (frames * odim)
                dl, el, pl = b[DUR_SQ] / tokens, b[ENERGY_SQ] / frames, b[PITCH_SQ] / frames
            else:
                if not self.pads:
                    raise ValueError("the unmasked means run over the pad positions: these terms were built with pads=False")
                frames, tokens = b[OLEN] + b[PAD_FRAMES], b[ILEN] + b[PAD_TOKENS]
                bl, al = (b[BEFORE_L1] + b[PAD_BEFORE_L1]) / (frames * odim), (b[AFTER_L1] + b[PAD_AFTER_L1]) / (frames * odim)
                dl, el, pl = (b[DUR_SQ] + b[PAD_DUR_SQ]) / tokens, (b[ENERGY_SQ] + b[PAD_ENERGY_SQ]) / frames, (b[PITCH_SQ] + b[PAD_PITCH_SQ]) / frames
            l1 = bl + al
            if use_weighted_masking:
                l1 = l1 / odim
        return [(n, float(v)) for n, v in zip(REPORT_NAMES, (l1, bl, al, dl, el, pl, l1 + dl + el + pl))]

    def evaluate(self):
        """``(pitch, energy, dur)``: what the reference's evaluation.py returns for these utterances fed one at a time -- the mean
        over the utterances of each one's mean |p_outs - ps|, |e_outs - es| over its frames and |d_outs - ds| over its tokens
        (evaluation.py:31 as written: the log-domain predictor output against the linear durations)."""
        t = self.terms
        with np.errstate(divide="ignore", invalid="ignore"):
            return (float(np.mean(t[:, PITCH_L1] / t[:, OLEN])), float(np.mean(t[:, ENERGY_L1] / t[:, OLEN])),
                    float(np.mean(t[:, DUR_L1] / t[:, ILEN])))

    def per_utterance(self, odim=None):
        """Per-utterance means over each utterance's own frames and tokens, as a dict of float64 arrays [B]: ``before_l1``,
        ``after_l1`` (per mel value), ``duration_mse`` (log domain), ``energy_mse``, ``pitch_mse``, ``duration_l1`` (evaluation.py's),
        ``energy_l1``, ``pitch_l1``, and the counts ``ilen``, ``olen``."""
        odim = self.odim if odim is None else odim
        if odim is None:
            raise ValueError("per_utterance() needs odim (these terms were merged or built without it)")
        t = self.terms
        with np.errstate(divide="ignore", invalid="ignore"):
            return dict(ilen=t[:, ILEN].astype(np.int64), olen=t[:, OLEN].astype(np.int64),
                        before_l1=t[:, BEFORE_L1] / (t[:, OLEN] * odim), after_l1=t[:, AFTER_L1] / (t[:, OLEN] * odim),
                        duration_mse=t[:, DUR_SQ] / t[:, ILEN], energy_mse=t[:, ENERGY_SQ] / t[:, OLEN], pitch_mse=t[:, PITCH_SQ] / t[:, OLEN],
                        duration_l1=t[:, DUR_L1] / t[:, ILEN], energy_l1=t[:, ENERGY_L1] / t[:, OLEN], pitch_l1=t[:, PITCH_L1] / t[:, OLEN])

    def merge(self, other):
        """The terms of two disjoint sets of utterances (batches of a validation set, ranks): the rows one after the other, the
        batch records added (sums and counts are additive).  Raises if one was built with the pad sums and the other without:
        their pad counts (indices 2, 3) would count positions whose sums only one of them holds."""
        if self.pads != other.pads:
            raise ValueError("merge of terms built with pads=%s and pads=%s" % (self.pads, other.pads))
        if self.odim is not None and other.odim is not None and self.odim != other.odim:
            raise ValueError("merge of terms over %d and %d mel bins" % (self.odim, other.odim))
        return LossTerms(np.concatenate([self.terms, other.terms]), self.batch + other.batch, self.pads,
                         self.odim if self.odim is not None else other.odim)

    @staticmethod
    def empty(pads=True, odim=None):
        """The terms of no utterance: the identity of ``merge``."""
        return LossTerms(np.zeros((0, TERMS)), np.zeros(TERMS), pads, odim)


def _rows(t, name, dtype, inner):
    """-> (tensor, stride of the second dimension in rows) of a [B, S] (inner = 0) or [B, S, inner] tensor whose rows lie back to back;
    anything else (a transposed view, a column slice) is copied."""
    _require_cuda(t, name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != (3 if inner else 2) or (inner and t.shape[2] != inner):
        raise ValueError("%s must be [B, S%s], got %s" % (name, ", %d" % inner if inner else "", tuple(t.shape)))
    w = inner if inner else 1
    ok = t.stride(1) == w and t.stride(0) % w == 0 and t.stride(0) // w >= t.shape[1] and (not inner or t.stride(2) == 1)
    if not ok or t.shape[0] * t.shape[1] == 0:
        t = t.contiguous()
        return t, t.shape[1]
    return t, t.stride(0) // w


def loss_terms(before, after, ys, d_outs, ds, e_outs, es, p_outs, ps, ilens, olens, pads=True, sync=True):
    """One pass over the outputs of the teacher-forced forward and the targets -> :class:`LossTerms`.

    before, after [B, >= Lmax, odim], ys [B, >= Lmax, odim], d_outs [B, >= Tmax] (log domain), ds int64 [B, >= Tmax], e_outs, p_outs,
    es, ps [B, >= Lmax]: float32 device tensors, read in place through their strides (the collate's targets are usually wider than
    the model's outputs; no copy is made of a tensor whose rows lie back to back).  A prediction and its target may be None
    together (before and after share ys): its sums are 0.  ``ilens`` / ``olens``: host lengths; Tmax / Lmax are their maxima.
    ``pads=False`` skips the sums over the pad positions (what ``report(use_masking=False)`` needs): nothing outside
    [0, len) of any utterance is then read, so whatever is parked there -- NaN included -- cannot reach a result.
    ``sync=False``: nothing waits for the GPU; the records stay on the device until they are first read."""
    il, ol = _lens(ilens, name="ilens"), _lens(olens, name="olens")
    B = int(il.numel())
    if ol.numel() != B:
        raise ValueError("ilens has %d entries, olens %d" % (B, ol.numel()))
    Tmax, Lmax = (int(il.max()), int(ol.max())) if B else (0, 0)
    if max(Tmax, Lmax) > 2 ** 31 - 1:
        raise ValueError("lengths beyond 2^31 - 1")
    for a, b, na, nb in ((d_outs, ds, "d_outs", "ds"), (e_outs, es, "e_outs", "es"), (p_outs, ps, "p_outs", "ps")):
        if (a is None) != (b is None):
            raise ValueError("%s and %s must be given together" % (na, nb))
    if (before is not None or after is not None) and ys is None:
        raise ValueError("before / after without ys")
    given = [t for t in (before, after, ys, d_outs, ds, e_outs, es, p_outs, ps) if t is not None]
    if not given:
        raise ValueError("no tensor given")
    dev = given[0].device
    odim = next((int(t.shape[2]) for t in (before, after, ys) if t is not None and t.dim() == 3), None)
    f32, i64 = torch.float32, torch.int64

    def group(members, dtype, extent, what):
        """The tensors of one stride group [(tensor or None, name, inner width)] brought to a common row stride -> (tensors, stride)."""
        out = []
        for t, n, inner in members:
            if t is None:
                out.append((None, 0))
                continue
            if t.device != dev:
                raise ValueError("%s is on %s, the other tensors on %s" % (n, t.device, dev))
            if t.shape[0] != B:
                raise ValueError("%s holds %d utterances, ilens %d" % (n, t.shape[0], B))
            if t.shape[1] < extent:
                raise ValueError("%s has %d %s per utterance, the longest utterance %d" % (n, t.shape[1], what, extent))
            out.append(_rows(t, n, dtype, inner))
        if len({s for t, s in out if t is not None}) > 1:          # (e.g. a wider e_outs next to before [B, Lmax, odim]): narrow copies
            out = [(None, 0) if t is None else (t[:, :extent].contiguous(), extent) for t, _ in out]
        return [t for t, _ in out], max([s for t, s in out if t is not None], default=0)

    (before, after, e_outs, p_outs), psf = group(((before, "before", odim), (after, "after", odim), (e_outs, "e_outs", 0), (p_outs, "p_outs", 0)),
                                                 f32, Lmax, "frames")
    (ys,), ysf = group(((ys, "ys", odim),), f32, Lmax, "frames")
    (d_outs,), pst = group(((d_outs, "d_outs", 0),), f32, Tmax, "tokens")
    (ds,), dst = group(((ds, "ds", 0),), i64, Tmax, "tokens")
    (es, ps), tsf = group(((es, "es", 0), (ps, "ps", 0)), f32, Lmax, "frames")
    if max(psf, ysf, pst, dst, tsf) > 2 ** 31 - 1:
        raise ValueError("a row stride beyond 2^31 - 1")

    lib = _lib.lib()
    il_np, il_p = _i32(il.numpy())
    ol_np, ol_p = _i32(ol.numpy())
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        ws_bytes = int(lib.fs2_op_loss_workspace_bytes(B, ol_p)) if B else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if B else None
        rec, terms_p, batch_p = LossTerms._on_device(B, dev)
        args = _lib.OpLossArgs(B, odim or 0, Tmax, Lmax, int(bool(pads)), psf, ysf, pst, dst, tsf,
                               ptr(before), ptr(after), ptr(ys), ptr(d_outs), ptr(ds), ptr(e_outs), ptr(es), ptr(p_outs), ptr(ps),
                               il_p, ol_p, ptr(ws), ws_bytes, terms_p, batch_p)
        _lib.check(lib.fs2_op_loss_terms(_stream(dev), C.byref(args)))
    return LossTerms(None, None, pads, odim, _device=rec)._synced(sync)
