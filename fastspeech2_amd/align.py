"""Phoneme durations of a recording on the MI355X: batched forced alignment of recorded frames to synthesized frames
(csrc/align.h, include/fs2.h: fs2_op_align).

The reference's data loader needs a duration per phoneme for every utterance and gets them from an aligner that is not part of it.
``monotonic_align`` assigns every frame of a recording to exactly one frame of a synthesis of the same text (a *state*), monotonically
and with a step of at most ``max_step`` states per frame, at the least total distance; the frames per label (the phoneme a state
belongs to: ``fs2_decode``'s ``lr_index``) are the durations, and they add up to the recording's length by construction.
``FeedForwardTransformer.align_durations`` does the free-running forward and this in one call.

Everything is formed in double in a fixed order: a pair's results do not depend on the batch it is in, on its place there, on a
stride or on the workspace.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._host import _i32, _lens, _stream
from .dtw import FEATURES, _pairs
from .losses import DeviceRecords

TERMS = _lib.ALIGN_TERMS
# index of a record (include/fs2.h)
N_STATES, N_FRAMES, FLAGS, COST, STATES_USED, LONGEST_STAY, EMPTY_LABELS = range(7)


class Alignment(DeviceRecords):
    """``durations``: device int64 [B, T], row b = the frames per label of pair b (zeros beyond its labels; all zeros where no
    alignment was found).  ``state``: device int32 laid out like the rows of ``b`` -- the pair-local index of the state every frame
    was assigned to, -1 at pads and where no alignment was found -- or None.  ``terms`` [B, 8] / ``batch`` [8]: the records (float64
    numpy; include/fs2.h lists the indices); after ``sync=False`` they are still on the device and the first read fetches them with
    one copy, which waits for the stream."""
    TERMS = TERMS

    def __init__(self, durations, state, terms, batch, features, D, _device=None):
        if features not in FEATURES:
            raise ValueError("features must be one of %s, got %r" % (FEATURES, features))
        super().__init__(terms, batch, _device)
        self.durations, self.state = durations, state
        self.features, self.D = features, D

    @property
    def ok(self):
        """bool [B]: an alignment was found (flags 0)."""
        return self.terms[:, FLAGS] == 0

    def __len__(self):
        return int(self.durations.shape[0])

    def per_utterance(self):
        """Per pair, as a dict of arrays [B]: ``n_states``, ``n_frames``, ``flags`` (0 fine, 1 no alignment exists, 2 the cost is
        not finite), ``cost_per_frame`` = cost / M (NaN without an alignment), ``length_ratio`` = N / M, ``states_skipped`` = the
        states that received no frame, ``longest_stay`` = the longest run of frames in one state, ``empty_labels`` = the labels that
        received no frame."""
        t = self.terms
        fine = t[:, FLAGS] == 0
        i64 = lambda x: x.astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return dict(n_states=i64(t[:, N_STATES]), n_frames=i64(t[:, N_FRAMES]), flags=i64(t[:, FLAGS]),
                        cost_per_frame=np.where(fine, t[:, COST] / t[:, N_FRAMES], np.nan), length_ratio=t[:, N_STATES] / t[:, N_FRAMES],
                        states_skipped=i64(np.where(fine, t[:, N_STATES] - t[:, STATES_USED], 0)), longest_stay=i64(t[:, LONGEST_STAY]),
                        empty_labels=i64(t[:, EMPTY_LABELS]))

    def merge(self, other):
        """The alignments of two disjoint sets of pairs: the rows one after the other (the durations padded with zeros to the wider
        of the two), the batch records added.  ``state`` is kept when both have it in the same layout (padded ones are widened with
        -1).  Raises if the two were built from different features or widths."""
        if self.features != other.features:
            raise ValueError("merge of alignments over %s and %s features" % (self.features, other.features))
        if self.D is not None and other.D is not None and self.D != other.D:
            raise ValueError("merge of alignments over vectors of width %d and %d" % (self.D, other.D))

        def wide(x, w, fill):
            return x if x.shape[1] == w else torch.nn.functional.pad(x, (0, w - x.shape[1]), value=fill)
        w = max(self.durations.shape[1], other.durations.shape[1])
        durations = torch.cat([wide(self.durations, w, 0), wide(other.durations.to(self.durations.device), w, 0)])
        state = None
        if self.state is not None and other.state is not None and self.state.dim() == other.state.dim():
            o = other.state.to(self.state.device)
            if o.dim() == 1:
                state = torch.cat([self.state, o])
            else:
                w = max(self.state.shape[1], o.shape[1])
                state = torch.cat([wide(self.state, w, -1), wide(o, w, -1)])
        return Alignment(durations, state, np.concatenate([self.terms, other.terms]), self.batch + other.batch, self.features,
                         self.D if self.D is not None else other.D)


def monotonic_align(a, a_lens, b, b_lens, labels=None, n_labels=None, max_step=2, features="mel", n_mcep=13, workspace_cap=256 << 20,
                    sync=True):
    """Forced alignment of B pairs -> :class:`Alignment`.

    ``a`` (the states: synthesized frames) and ``b`` (the frames of the recording): float32 device tensors, padded [B, S, D] or
    packed [rows, D], read in place through their strides; ``a_lens`` / ``b_lens``: host lengths.  ``labels``: device int32 laid out
    like the rows of ``a`` ([B, S] or [rows]), non-decreasing within a pair, with ``n_labels`` (host [B]) labels per pair; without
    them every state is its own label.  ``max_step``: a frame may advance by at most this many states (1 or 2); a pair has an
    alignment iff N >= 1, M >= 1 and N - 1 <= max_step (M - 1), and a pair without one keeps zeros and ``ok`` False.
    ``features``, ``n_mcep``, ``workspace_cap``, ``sync``: as ``mel_dtw``.  ``durations`` is [B, max n_labels] (without labels:
    [B, max a_lens])."""
    if features not in FEATURES:
        raise ValueError("features must be one of %s, got %r" % (FEATURES, features))
    if max_step not in (1, 2):
        raise ValueError("max_step must be 1 or 2, got %r" % (max_step,))
    if (labels is None) != (n_labels is None):
        raise ValueError("labels and n_labels are given together or not at all")
    q = _pairs(Alignment, "fs2_op_align_workspace_bytes", a, a_lens, b, b_lens, ((labels, "labels", torch.int32),), (), features, n_mcep, workspace_cap)
    B, b, b_starts, dev, (lab,) = q.B, q.b, q.b_starts, q.dev, q.a_tracks
    nl = q.al if labels is None else _lens(n_labels, B, name="n_labels")
    if lab is not None and lab.numel() == 0:                    # no state at all: an empty tensor has no address
        lab = None
    nl_keep, nl_p = _i32(nl.numpy())
    ptr = lambda t: None if t is None else t.data_ptr()
    T = int(nl.max()) if B else 0
    with torch.cuda.device(dev):
        durations = torch.empty(B, T, dtype=torch.int64, device=dev)
        if b.dim() == 3:                # indexed by the rows of b: the view [B, S] of a buffer with b's rows per sequence
            per_seq = int(b_starts[1]) if B > 1 else int(b.shape[1])
            flat = torch.full((max(B - 1, 0) * per_seq + (int(b.shape[1]) if B else 0),), -1, dtype=torch.int32, device=dev)
            state = torch.as_strided(flat, (B, int(b.shape[1])), (per_seq, 1))
        else:                           # (packed: the rows beyond the lengths' sum stay -1 too)
            state = torch.full((int(b.shape[0]),), -1, dtype=torch.int32, device=dev)
            flat = state
        args = _lib.OpAlignArgs(B, q.D, int(max_step), q.a_stride, q.b_stride, T, ptr(q.a), ptr(b), ptr(lab), *q.lens,
                                nl_p if lab is not None else None, ptr(q.ws), q.ws_bytes, durations.data_ptr() if durations.numel() else None,
                                flat.data_ptr() if flat.numel() else None, q.terms_p, q.batch_p)
        _lib.check(_lib.lib().fs2_op_align(_stream(dev), C.byref(args)))
    return Alignment(durations, state, None, None, features, q.D, _device=q.rec)._synced(sync)
