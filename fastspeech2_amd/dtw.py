"""Free-running validation on the MI355X: batched dynamic time warping between synthesized and recorded mel sequences, with the F0
and energy errors over the aligned frame pairs (csrc/dtw.h, include/fs2.h: fs2_op_dtw).

``loss_terms`` compares the teacher-forced outputs with the targets frame by frame, which works because teacher forcing gives
both the same length.  The model's real output -- ``inference_batch``, with the durations it predicts itself -- differs in length
from the recording, and the reference can only plot it (train_fastspeech.py:148-190).  ``mel_dtw`` aligns each pair with the
cheapest monotone path and leaves a record per pair (``FS2_DTW_TERMS`` doubles) plus their batch record on the device; ``DtwTerms``
turns the records into the usual numbers on the host, in float64: the mean distance along the path (log-spectral distance in dB
for mel features, mel-cepstral distortion for ``features="mcep"``), the F0 and energy L1 over the aligned pairs, the voicing
mismatch rate and the length ratio.

Everything is formed in double in a fixed order: a pair's record does not depend on the batch it is in, on its place there, on a
stride or on the workspace.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes as C
import math
import types

import numpy as np
import torch

from . import _lib
from ._host import _i32, _lens, _require_cuda, _stream
from .losses import DeviceRecords, _rows

TERMS = _lib.DTW_TERMS
# index of a record (include/fs2.h)
N_PRED, N_REF, STEPS, COST, ENERGY_L1, PITCH_L1, VOICED, PITCH_L1_VOICED, VUV = range(9)
FEATURES = ("mel", "mcep")


class DtwTerms(DeviceRecords):
    """The per-pair records ``terms`` [B, 12] and their batch record ``batch`` [12] (float64 numpy; include/fs2.h lists the
    indices).  After ``mel_dtw(..., sync=False)`` both are still on the device; the first read of either fetches them with one
    copy, which waits for the stream.  ``features`` ("mel" / "mcep") and ``D`` (the width of the compared vectors) say what the
    cost is a distance of."""
    TERMS = TERMS

    def __init__(self, terms, batch, features, D, _device=None):
        if features not in FEATURES:
            raise ValueError("features must be one of %s, got %r" % (FEATURES, features))
        super().__init__(terms, batch, _device)
        self.features, self.D = features, D

    def per_utterance(self):
        """Per pair, as a dict of float64 arrays [B]: ``n_pred``, ``n_ref``, ``steps`` (counts), ``distance`` = cost / steps,
        ``lsd_db`` = (20 / ln 10) distance / sqrt(D) (mel features: the rms log-spectral difference per aligned pair, for natural-log
        mels) or ``mcd_db`` = (10 sqrt 2 / ln 10) distance (mcep features), ``energy_l1``, ``pitch_l1`` (per aligned pair),
        ``f0_l1_voiced`` (over the pairs voiced on both sides), ``vuv_error`` = voicing mismatches / steps, ``length_ratio`` = N / M."""
        t = self.terms
        with np.errstate(divide="ignore", invalid="ignore"):
            distance = t[:, COST] / t[:, STEPS]
            out = dict(n_pred=t[:, N_PRED].astype(np.int64), n_ref=t[:, N_REF].astype(np.int64), steps=t[:, STEPS].astype(np.int64),
                       distance=distance, energy_l1=t[:, ENERGY_L1] / t[:, STEPS], pitch_l1=t[:, PITCH_L1] / t[:, STEPS],
                       f0_l1_voiced=t[:, PITCH_L1_VOICED] / t[:, VOICED], vuv_error=t[:, VUV] / t[:, STEPS],
                       length_ratio=t[:, N_PRED] / t[:, N_REF])
            if self.features == "mel":
                if self.D is None:
                    raise ValueError("lsd_db needs D (these terms were built without it)")
                out["lsd_db"] = (20.0 / math.log(10.0)) * distance / math.sqrt(self.D)
            else:
                out["mcd_db"] = (10.0 * math.sqrt(2.0) / math.log(10.0)) * distance
        return out

    def evaluate(self):
        """``(pitch_l1, energy_l1, distance)``, each the mean over the pairs of the pair's own mean along its path: the free-running
        counterpart of ``LossTerms.evaluate()``."""
        t = self.terms
        with np.errstate(divide="ignore", invalid="ignore"):
            return (float(np.mean(t[:, PITCH_L1] / t[:, STEPS])), float(np.mean(t[:, ENERGY_L1] / t[:, STEPS])),
                    float(np.mean(t[:, COST] / t[:, STEPS])))

    def merge(self, other):
        """The terms of two disjoint sets of pairs (batches of a validation set, ranks): the rows one after the other, the batch
        records added.  Raises if the two were built from different features or different widths: their costs are distances of
        different things."""
        if self.features != other.features:
            raise ValueError("merge of terms over %s and %s features" % (self.features, other.features))
        if self.D is not None and other.D is not None and self.D != other.D:
            raise ValueError("merge of terms over vectors of width %d and %d" % (self.D, other.D))
        return DtwTerms(np.concatenate([self.terms, other.terms]), self.batch + other.batch, self.features,
                        self.D if self.D is not None else other.D)

    @staticmethod
    def empty(features="mel", D=None):
        """The terms of no pair: the identity of ``merge``."""
        return DtwTerms(np.zeros((0, TERMS)), np.zeros(TERMS), features, D)


def dct_basis(D, n_mcep, device=None):
    """Orthonormal DCT-II, coefficients 1 .. n_mcep of D inputs: [D, n_mcep] float64."""
    if not 1 <= n_mcep < D:
        raise ValueError("n_mcep must be in [1, %d) for %d mel bins, got %d" % (D, D, n_mcep))
    n = torch.arange(D, dtype=torch.float64, device=device)[:, None]
    k = torch.arange(1, n_mcep + 1, dtype=torch.float64, device=device)[None, :]
    return math.sqrt(2.0 / D) * torch.cos(math.pi / D * (n + 0.5) * k)


def mcep(x, n_mcep=13):
    """[..., D] float32 log-mels -> [..., n_mcep] float32: a float64 matmul with the DCT basis, rounded once."""
    return (x.double() @ dct_basis(x.shape[-1], n_mcep, x.device)).float()


def _side(x, lens, name, tracks):
    """One side of the pairs -> (x, row stride in floats, first row of every pair, tracks), the tracks laid out by the same row offsets.
    ``x``: padded [B, S, D] or packed [rows, D]; ``tracks``: [(tensor or None, name)] or [(tensor or None, name, dtype)] (float32
    unless given), padded [B, S'] or packed [rows]."""
    _require_cuda(x, name)
    if x.dtype != torch.float32:
        raise TypeError("%s must be torch.float32, got %s" % (name, x.dtype))
    B = int(lens.numel())
    dtypes = {t[1]: t[2] if len(t) > 2 else torch.float32 for t in tracks}
    tracks = [(t[0], t[1]) for t in tracks]
    for t, n in tracks:
        if t is not None:
            _require_cuda(t, n)
            if t.dtype != dtypes[n]:
                raise TypeError("%s must be %s, got %s" % (n, dtypes[n], t.dtype))
            if t.device != x.device:
                raise ValueError("%s is on %s, %s on %s" % (n, t.device, name, x.device))
            if t.dim() != x.dim() - 1:
                raise ValueError("%s must be %s like %s, got %s" % (n, "[B, S]" if x.dim() == 3 else "[rows]", name, tuple(t.shape)))
    if x.dim() == 3:
        if x.shape[0] != B:
            raise ValueError("%s holds %d sequences, its lengths %d" % (name, x.shape[0], B))
        Lmax = int(lens.max()) if B else 0
        if Lmax > x.shape[1]:
            raise ValueError("%s has %d frames per sequence, its longest length is %d" % (name, x.shape[1], Lmax))
        for t, n in tracks:
            if t is not None and (t.shape[0] != B or t.shape[1] < Lmax):
                raise ValueError("%s is %s, %s needs [%d, >= %d]" % (n, tuple(t.shape), name, B, Lmax))
        x, stride = _rows(x, name, torch.float32, int(x.shape[2]))
        out = [(None, 0) if t is None else _rows(t, n, dtypes[n], 0) for t, n in tracks]
        if any(t is not None and s != stride for t, s in out):      # (e.g. targets wider than the mels): narrow copies, one common stride
            x, stride = x[:, :Lmax].contiguous(), Lmax
            out = [(None, 0) if t is None else (t[:, :Lmax].contiguous(), Lmax) for t, _ in out]
        starts = np.arange(B, dtype=np.int64) * stride
        return x, int(x.shape[2]), starts, [t for t, _ in out]
    if x.dim() != 2:
        raise ValueError("%s must be padded [B, S, D] or packed [rows, D], got %s" % (name, tuple(x.shape)))
    total = int(lens.sum())
    if total > x.shape[0]:
        raise ValueError("%s has %d rows, its lengths add up to %d" % (name, x.shape[0], total))
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    out = []
    for t, n in tracks:
        if t is not None and t.shape[0] < total:
            raise ValueError("%s has %d entries, the lengths of %s add up to %d" % (n, t.shape[0], name, total))
        out.append(None if t is None else t.contiguous())
    starts = np.cumsum(lens.numpy()) - lens.numpy()
    return x, int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1]), starts, out


def _pairs(cls, query, a, a_lens, b, b_lens, a_tracks, b_tracks, features, n_mcep, workspace_cap):
    """What ``mel_dtw`` and ``monotonic_align`` do before their call: the checks of the lengths and the two sides, the mcep projection,
    the layout of each side with its tracks (``_side``), the host int32 arrays ``lens`` = (a_starts, a_lens, b_starts, b_lens) as
    pointers (``keep`` holds their memory), the workspace ``ws`` of ``ws_bytes`` = ``query`` (the name of the operator's
    fs2_op_*_workspace_bytes) and the device records of ``cls`` (``rec``, ``terms_p``, ``batch_p``) -> a namespace of all that."""
    al, bl = _lens(a_lens, name="a_lens"), _lens(b_lens, name="b_lens")
    B = int(al.numel())
    if bl.numel() != B:
        raise ValueError("a_lens has %d entries, b_lens %d" % (B, bl.numel()))
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    if a.device != b.device:
        raise ValueError("a is on %s, b on %s" % (a.device, b.device))
    if a.shape[-1] != b.shape[-1]:
        raise ValueError("a has %d features per frame, b %d" % (a.shape[-1], b.shape[-1]))
    if features == "mcep":
        a, b = mcep(a.float(), n_mcep), mcep(b.float(), n_mcep)
    D = int(a.shape[-1])
    if not 1 <= D <= 128:
        raise ValueError("D = %d outside [1, 128]" % D)
    dev = a.device
    a, a_stride, a_starts, a_tracks = _side(a, al, "a", a_tracks)
    b, b_stride, b_starts, b_tracks = _side(b, bl, "b", b_tracks)
    if B and max(int((a_starts + al.numpy()).max()), int((b_starts + bl.numpy()).max())) > 2 ** 31 - 1:
        raise ValueError("rows beyond 2^31 - 1")
    keep = [_i32(x) for x in (a_starts, al.numpy(), b_starts, bl.numpy())]
    lens = tuple(p for _, p in keep)
    ws_bytes = int(getattr(_lib.lib(), query)(B, lens[1], lens[3], int(workspace_cap))) if B else 0
    if B and not ws_bytes:
        raise ValueError("a pair of more than 2^40 cells")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if B else None
    rec, terms_p, batch_p = cls._on_device(B, dev)
    return types.SimpleNamespace(B=B, D=D, dev=dev, al=al, a=a, b=b, a_stride=a_stride, b_stride=b_stride, a_starts=a_starts, b_starts=b_starts,
                                 a_tracks=a_tracks, b_tracks=b_tracks, keep=keep, lens=lens, ws=ws, ws_bytes=ws_bytes, rec=rec, terms_p=terms_p,
                                 batch_p=batch_p)


def mel_dtw(a, a_lens, b, b_lens, e=None, p=None, features="mel", n_mcep=13, workspace_cap=256 << 20, sync=True):
    """DTW between B pairs of sequences -> :class:`DtwTerms`.

    ``a`` (synthesized) and ``b`` (reference): float32 device tensors, padded [B, S, D] or packed [rows, D] (the sequences back to
    back), read in place through their strides; ``a_lens`` / ``b_lens``: host lengths.  ``e`` / ``p``: ``(pred, ref)`` pairs of
    per-frame energy / pitch tracks ([B, S] or [rows], laid out like their side; pitch 0 = unvoiced), each optional.
    ``features="mcep"`` first projects both sides onto the orthonormal DCT-II coefficients 1 .. ``n_mcep`` (a float64 matmul
    rounded to float32).  ``workspace_cap``: the distance matrices of as many consecutive pairs as fit this many bytes are held at
    once (a single pair larger than that still gets what it needs); the records do not depend on it.  ``sync=False``: nothing
    waits for the GPU; the records stay on the device until they are first read."""
    if features not in FEATURES:
        raise ValueError("features must be one of %s, got %r" % (FEATURES, features))
    for pair, n in ((e, "e"), (p, "p")):
        if pair is not None and (len(pair) != 2 or (pair[0] is None) != (pair[1] is None)):
            raise ValueError("%s must be a (pred, ref) pair: a track is given for both sides or for neither" % n)
    e = None if e is None or e[0] is None else e
    p = None if p is None or p[0] is None else p
    q = _pairs(DtwTerms, "fs2_op_dtw_workspace_bytes", a, a_lens, b, b_lens, ((e[0] if e else None, "e[0]"), (p[0] if p else None, "p[0]")),
               ((e[1] if e else None, "e[1]"), (p[1] if p else None, "p[1]")), features, n_mcep, workspace_cap)
    (e_a, p_a), (e_b, p_b) = q.a_tracks, q.b_tracks
    if e_a is not None and 0 in (e_a.numel(), e_b.numel()):         # a side without a frame: every pair is empty, and an empty tensor has no address
        e_a = e_b = None
    if p_a is not None and 0 in (p_a.numel(), p_b.numel()):
        p_a = p_b = None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(q.dev):
        args = _lib.OpDtwArgs(q.B, q.D, q.a_stride, q.b_stride, ptr(q.a), ptr(q.b), ptr(e_a), ptr(e_b), ptr(p_a), ptr(p_b), *q.lens,
                              ptr(q.ws), q.ws_bytes, q.terms_p, q.batch_p)
        _lib.check(_lib.lib().fs2_op_dtw(_stream(q.dev), C.byref(args)))
    return DtwTerms(None, None, features, q.D, _device=q.rec)._synced(sync)
