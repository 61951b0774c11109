"""Pitch and energy control at synthesis time, and per-phoneme means of per-frame tracks (csrc/prosody.h, include/fs2.h:
fs2_decode_ctl, fs2_op_label_means).

FastSpeech 2 predicts pitch and energy per frame before it decodes.  ``inference``, ``inference_batch``, ``capture_graph`` and
``predict_prosody`` of ``FeedForwardTransformer`` take ``pitch_scale``, ``pitch_shift``, ``energy_scale`` and ``energy_shift``: each
None (neutral), a number, a ``[B, 1]`` tensor (one value per utterance) or a ``[B, Tmax]`` tensor (one per phoneme).  Every predicted
value ``v`` of a frame becomes ``v * scale + shift`` in float32, the product and the sum rounded one after the other, before it is
quantised; the units are the predictors' own, i.e. those of the training targets (with F0 in Hz, ``pitch_scale=semitones(+2)`` speaks
two semitones higher, and ``pitch_scale=0, pitch_shift=contour`` imposes a contour).  There is no CPU fallback: CPU tensors raise.
"""
from typing import NamedTuple

import torch

from . import _lib
from ._host import _require_cuda, _stream

CONTROLS = ("pitch_scale", "pitch_shift", "energy_scale", "energy_shift")


def semitones(x):
    """The frequency ratio of ``x`` semitones: ``2 ** (x / 12)`` (a ``pitch_scale``)."""
    return 2.0 ** (x / 12.0)


def _control(name, v, B, Tmax, device):
    if v is None:
        return None
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return torch.full((B, 1), float(v), dtype=torch.float32, device=device)
    if not torch.is_tensor(v):
        raise ValueError("%s must be None, a number or a float32 tensor [B, 1] or [B, Tmax], got %s" % (name, type(v).__name__))
    if v.dim() != 2 or v.shape[0] != B or v.shape[1] not in (1, Tmax):
        raise ValueError("%s must be [B, 1] = [%d, 1] (per utterance) or [B, Tmax] = [%d, %d] (per phoneme), got %s"
                         % (name, B, B, Tmax, list(v.shape)))
    if v.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, v.dtype))
    if v.device != device:
        raise ValueError("%s is on %s, the batch on %s (no CPU fallback)" % (name, v.device, device))
    return v.detach().contiguous()


def normalize_controls(B, Tmax, device, pitch_scale=None, pitch_shift=None, energy_scale=None, energy_shift=None):
    """The four controls of a batch of ``B`` utterances of up to ``Tmax`` phonemes on ``device`` -> dict name -> contiguous float32
    tensor ``[B, 1]`` or ``[B, Tmax]`` on ``device``, or None.  Accepted: None, a Python number, a ``[B, 1]`` or a ``[B, Tmax]`` float32
    tensor on ``device``; anything else raises ``ValueError`` naming the argument."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    given = dict(pitch_scale=pitch_scale, pitch_shift=pitch_shift, energy_scale=energy_scale, energy_shift=energy_shift)
    return {k: _control(k, v, int(B), int(Tmax), device) for k, v in given.items()}


def prosody_struct(ctl):
    """``normalize_controls``' dict -> the ``_lib.Prosody`` to hand to fs2_decode_ctl, or None when nothing is controlled."""
    if ctl is None or all(ctl[k] is None for k in CONTROLS):
        return None
    return _lib.Prosody(*[None if ctl[k] is None else ctl[k].data_ptr() for k in CONTROLS],
                        *[1 if ctl[k] is None else int(ctl[k].shape[1]) for k in CONTROLS])


def label_means(x, labels, lens, n_labels, positive_only=False):
    """Per-label means of a per-frame track -> ``(mean float32 [B, n_labels], count int32 [B, n_labels])``.

    ``x``: float32 device ``[B, S]``; ``labels``: int32 device ``[B, S]`` (``lr_index``: the phoneme of every frame, non-decreasing
    over the valid frames); ``lens``: the valid frames per utterance (a device int64 tensor is used as it is: nothing then waits for
    the GPU, and the call may be captured into a graph).  ``count[b, t]`` = the frames of label ``t``, with ``positive_only`` only
    those whose value is > 0 (the voiced frames of an F0 track); ``mean[b, t]`` = their sum, added in frame order in float64, over
    the count, 0 where the count is 0."""
    _require_cuda(x, "x")
    _require_cuda(labels, "labels")
    if x.dim() != 2 or tuple(labels.shape) != tuple(x.shape):
        raise ValueError("x and labels must both be [B, S], got %s and %s" % (list(x.shape), list(labels.shape)))
    if x.dtype != torch.float32 or labels.dtype != torch.int32:
        raise TypeError("x must be float32 and labels int32, got %s and %s" % (x.dtype, labels.dtype))
    if labels.device != x.device:
        raise ValueError("x is on %s, labels on %s" % (x.device, labels.device))
    n_labels = int(n_labels)
    if n_labels < 0:
        raise ValueError("n_labels must be >= 0, got %d" % n_labels)
    dev = x.device
    B, S = int(x.shape[0]), int(x.shape[1])
    x, labels = x.contiguous(), labels.contiguous()
    lens = torch.as_tensor(lens).detach().reshape(-1)
    if lens.numel() != B:
        raise ValueError("lens has %d entries for %d utterances" % (lens.numel(), B))
    lens = lens.to(dev, torch.int64).contiguous()
    mean = torch.empty(B, n_labels, dtype=torch.float32, device=dev)
    count = torch.empty(B, n_labels, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().fs2_op_label_means(_stream(dev), ptr(x), ptr(labels), ptr(lens), B, S, n_labels, int(bool(positive_only)),
                                                 ptr(mean), ptr(count)))
    return mean, count


class ProsodyPrediction(NamedTuple):
    """What ``FeedForwardTransformer.predict_prosody`` returns (device tensors unless noted; ``Lmax`` = the longest utterance's frames).

    ``durations`` int64 [B, Tmax]: the frames each phoneme received (edit and pass as ``d_override``: duration control per phoneme);
    ``olens`` int64 [B] on the host: decoder frames per utterance = ``durations.sum(1)``;
    ``pitch`` / ``energy`` float32 [B, Lmax]: the per-frame values that were quantised (controlled, if control was given), pads 0;
    ``lr_index`` int32 [B, Lmax]: the phoneme of every frame, -1 at pads;
    ``pitch_tok`` / ``energy_tok`` float32 [B, Tmax]: their means per phoneme -- pitch over the frames with a value > 0 only (the
    voiced frames, the reference's convention for F0), 0 where there is none;
    ``voiced_tok`` int32 [B, Tmax]: the frames of each phoneme that entered ``pitch_tok``."""
    durations: torch.Tensor
    olens: torch.Tensor
    pitch: torch.Tensor
    energy: torch.Tensor
    lr_index: torch.Tensor
    pitch_tok: torch.Tensor
    energy_tok: torch.Tensor
    voiced_tok: torch.Tensor
