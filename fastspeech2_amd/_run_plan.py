"""The run plan: what one ``FeedForwardTransformer._run`` call consists of, decided once from plain values.

``plan_run`` takes no tensor and touches neither a device nor the library.  It either raises one of the call's refusals -- in the
order of ``REFUSALS`` below, before a handle exists, before anything is allocated or launched -- or returns a ``RunPlan`` that
``_run`` only follows.  What needs more than plain values stays where it was: the device and training refusals in front of the
plan; a control tensor's own shape (``prosody.normalize_controls``), the model's device (``_ensure_ready``), the library's
``Fs2Error`` and the two refusals that read device results (a phoneme id out of range, ``olens`` against the durations) behind it.

REFUSALS, first match wins:
   1  pitch / energy control together with ``compat``
   2  pitch / energy control together with a teacher-forced pass
   3  the number of ``ilens`` entries is not ``B``
   4  ``regime`` holds a value <= 0
   5  ``regime`` together with ``compat``
   6  a teacher-forced pass without ``ds``, ``es`` or ``ps``
   7  durations (``ds``; free-running: ``d_override``) whose shape is not ``(B, Tmax)``
   8  a teacher-forced pass with ``capacity``
   9  a malformed ``packed_out`` (looked at only when ``after_packed`` is wanted with a capacity)
  10  with a capacity: neither ``after`` nor ``after_packed`` wanted
  11  without one: ``after`` not wanted
"""
from collections import namedtuple

import torch

_F32, _I32 = torch.float32, torch.int32


class Output(namedtuple("Output", "key B per_frame tail dtype")):
    """One padded output of fs2_decode: ``shape(L)`` for a frame extent of ``L`` decoder frames."""
    __slots__ = ()

    def shape(self, L):
        return (self.B, L * self.per_frame) + self.tail


# what plan_run is told about ``packed_out`` (None: not given)
PackedOut = namedtuple("PackedOut", "contiguous dtype same_device shape")

RunPlan = namedtuple("RunPlan", (
    "device",            # the device-driven layout (capacity given): no read-back, row capacity and status; else the host layout
    "teacher", "controlled", "masked", "regime_tokens", "regime_utterances",
    "side_encoder",      # fs2_encode runs on the side stream (overlap_encoder)
    "d_log", "d_int", "encoder_out",      # what fs2_encode writes besides olens: two flags, and encoder_out's shape or None
    "outputs",           # the padded outputs in the field order of DecodeIO (before .. dec_out): an Output, or None = not written
    "after_packed",      # whether the pack is written ...
    "packed_per_row",    # ... and its rows per row of the layout (device: x fs2_row_capacity; host: x sum(olens))
    "packed_rows",       # device layout: its rows (rows x reduction_factor); host layout: None, known after the read-back
    "keys"))             # the keys of the result dict, in order


def plan_run(B, Tmax, n_ilens, reduction_factor, odim, adim, ddim, is_inference, compat, want, has_ds=False, has_es=False, has_ps=False,
             has_d_override=False, has_olens=False, durations_shape=None, capacity=None, rows=0, regime=None, controlled=False,
             packed_out=None, device=None, overlap_encoder=False, capturing=False):
    """``durations_shape``: of ``ds`` (teacher-forced) or of ``d_override`` (free-running, if given); ``rows``: fs2_row_capacity of
    ``capacity[0]`` (a pure function of ``B`` and the bound); ``packed_out``: a ``PackedOut`` or None; ``device``: named by refusal 9."""
    teacher = not is_inference
    if controlled:
        if compat:
            raise ValueError("pitch / energy control has per-utterance semantics only (batch_semantics='padded_compat')")
        if teacher:
            raise ValueError("pitch / energy control acts on predictions: the teacher-forced pass quantises the es / ps it is given")
    if n_ilens != B:
        raise ValueError("ilens has %d entries for a batch of %d" % (n_ilens, B))
    rt = ru = 0
    if regime is not None:
        rt, ru = int(regime[0]), int(regime[1])
        if rt <= 0 or ru <= 0:
            raise ValueError("regime=(phonemes, utterances) must both be positive, got %r" % (regime,))
        if compat:
            raise ValueError("regime applies to per-utterance semantics: a padded_compat batch depends on its batch-mates anyway")
    if teacher and not (has_ds and has_es and has_ps):
        raise ValueError("teacher-forced _forward needs ds, es and ps")
    if (teacher or has_d_override) and tuple(durations_shape) != (B, Tmax):
        raise ValueError("ds must be [B, Tmax] = [%d, %d], got %s" % (B, Tmax, tuple(durations_shape)))
    dev_layout = capacity is not None
    r = reduction_factor
    packed, prows = "after_packed" in want, None
    if dev_layout:
        if teacher:
            raise ValueError("the device-driven layout serves free-running synthesis")
        if packed:
            prows = rows * r       # mel frames: r per decoder row
            p = packed_out
            if p is not None and (not p.contiguous or p.dtype != _F32 or not p.same_device or len(p.shape) != 2 or p.shape[1] != odim
                                  or p.shape[0] < prows):
                raise ValueError("packed_out must be a contiguous float32 [>= %d, %d] tensor on %s" % (prows, odim, device))
        elif "after" not in want:
            raise ValueError("'after' or 'after_packed' must be requested")
    elif "after" not in want:
        raise ValueError("'after' must be requested")
    outputs = tuple([Output(key, B, per, tail, dt) if key in want else None for key, per, tail, dt in (
        ("before", r, (odim,), _F32), ("after", r, (odim,), _F32), ("e_outs", 1, (), _F32), ("p_outs", 1, (), _F32),
        ("qe", 1, (), _I32), ("qp", 1, (), _I32), ("lr_index", 1, (), _I32), ("decoder_out", 1, (ddim,), _F32))])
    enc_out = (B, Tmax, adim) if "encoder_out" in want else None
    keys = [o.key for o in outputs if o is not None]
    if packed:
        keys.append("after_packed")
    keys.append("olens")
    if dev_layout:
        keys.append("status")
    keys.append("d_log" if teacher else "d_int")
    if enc_out is not None:
        keys.append("encoder_out")
    return RunPlan(dev_layout, teacher, bool(controlled), int(teacher and has_olens) if compat else 0, rt, ru,
                   dev_layout and bool(overlap_encoder) and not capturing, teacher, not teacher, enc_out, outputs, packed, r, prows, tuple(keys))
