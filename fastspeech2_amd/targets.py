"""Training targets from the per-frame energy and F0 arrays on the MI355X (csrc/targets.h, include/fs2.h: fs2_op_clean_targets;
DESIGN.md section 14.4).

The reference cleans every energy and pitch array its data loader returns with ``remove_outlier`` (utils/util.py:26-49,
dataset/dataloader.py:56-61): per utterance, every value at or beyond 1.5 interquartile ranges from the 25th / 75th percentile is
replaced by the largest remaining value, and original zeros (unvoiced frames, silence) go back to zero.  Its compute_statistics.py
then takes, over the cleaned arrays of the whole corpus, the minima and maxima its quantiser's bucket boundaries are built from
(``hp.data.e_min / e_max / p_min / p_max``, fastspeech.py:322-327) and the mean and standard deviation of the non-zero values.
``clean_targets`` does both for a packed batch in one call, ``TargetStats.merge`` joins the statistics of batches into those of a
corpus, ``hp_data`` names them as the reference's config does, and ``training_targets`` goes from waveforms to the cleaned targets.

The cleaning equals the reference's under numpy 2.x bit for bit (float32 data; tests/targets_oracle.py states it operation by
operation).  An utterance's result does not depend on the batch it is in, the statistics of a batch are the same bits on every call,
and there is no limit on an utterance's length.  There is no CPU fallback: CPU tensors raise.
"""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._host import _i32, _lens, _require_cuda, _stream
from .vocoder import _audio_config, wav_features

_INF = float("inf")


class TargetStats(NamedTuple):
    """Statistics of cleaned targets over the finite utterances of one or more batches, as Python numbers.  ``clean_targets`` reads
    them back from the device once per call, and that read-back synchronises with the stream.

    n_total: values; n_outliers: values that were flagged; n_nonfinite: utterances with a NaN or an infinity (copied unchanged, left
    out of everything else); n_no_positive: utterances without any cleaned value > 0 (the reference's ``bad_pitch`` list); n, mean,
    std, M2: count, mean, population standard deviation sqrt(M2 / n) and sum of squared deviations of the cleaned values != 0, in
    float64; min, max: over all cleaned values; nonzero_min: over the cleaned values > 0 (+inf: none)."""
    n_total: int
    n_outliers: int
    n_nonfinite: int
    n_no_positive: int
    n: int
    min: float
    nonzero_min: float
    max: float
    mean: float
    std: float
    M2: float

    @staticmethod
    def empty():
        """The statistics of nothing: the identity of ``merge``."""
        return TargetStats(0, 0, 0, 0, 0, _INF, _INF, -_INF, 0.0, 0.0, 0.0)

    @staticmethod
    def merge(a, b):
        """Statistics of the union of two disjoint sets of utterances: sums, min / max, and Chan's update of (n, mean, M2) in
        float64.  A corpus is processed in batches and merged."""
        n = a.n + b.n
        if b.n == 0:
            mean, M2 = a.mean, a.M2
        elif a.n == 0:
            mean, M2 = b.mean, b.M2
        else:
            delta = b.mean - a.mean
            mean = a.mean + delta * (b.n / n)
            M2 = (a.M2 + b.M2) + delta * delta * (a.n * b.n / n)
        return TargetStats(a.n_total + b.n_total, a.n_outliers + b.n_outliers, a.n_nonfinite + b.n_nonfinite,
                           a.n_no_positive + b.n_no_positive, n, min(a.min, b.min), min(a.nonzero_min, b.nonzero_min), max(a.max, b.max),
                           mean, math.sqrt(M2 / n) if n else 0.0, M2)

    @staticmethod
    def from_record(rec):
        """From the double[12] record of fs2_op_clean_targets (include/fs2.h)."""
        r = [float(v) for v in rec]
        return TargetStats(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), r[5], r[6], r[7], r[8], r[9], r[10])


def _checked(x_packed, lens, out):
    """Everything that can be refused is refused here, before the library is loaded or the GPU touched."""
    _require_cuda(x_packed, "x_packed")
    if x_packed.dim() != 1:
        raise ValueError("x_packed must be 1-D, got %s" % (tuple(x_packed.shape),))
    if x_packed.dtype != torch.float32:
        raise TypeError("x_packed must be float32 (the cleaning is defined on float32 values), got %s" % x_packed.dtype)
    L = _lens(lens, name="lens")
    if int(L.sum()) != x_packed.numel():
        raise ValueError("lens sum to %d, x_packed has %d values" % (int(L.sum()), x_packed.numel()))
    if x_packed.numel() > 2 ** 31 - 1:
        raise ValueError("x_packed has %d values, one call takes at most 2^31 - 1" % x_packed.numel())
    if out is not None:
        _require_cuda(out, "out")
        if out.shape != x_packed.shape or out.dtype != torch.float32 or out.device != x_packed.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of x_packed's shape on its device")
    return L


def clean_targets(x_packed, lens, out=None, return_quartiles=False):
    """``remove_outlier`` of every utterance of a packed batch and the statistics of the result, from one call.

    x_packed: float32 [sum lens] on the GPU, utterance b = the next ``lens[b]`` values.  Returns ``(y, TargetStats)``; with
    ``return_quartiles=True`` ``(y, TargetStats, quartiles [B, 2], n_outliers [B])`` (p25 and p75 as np.percentile gives them, and
    the number of flagged values; NaN and 0 for an utterance that is empty or holds a NaN / infinity).  ``out=x_packed`` cleans in
    place.  An utterance whose quartiles coincide comes out all zero (the reference's behaviour); one with a NaN or an infinity is
    copied unchanged and counted in ``n_nonfinite``.  Reading the statistics back synchronises with the stream."""
    L = _checked(x_packed, lens, out)
    dev = x_packed.device
    B = int(L.numel())
    y = out if out is not None else torch.empty_like(x_packed, memory_format=torch.contiguous_format)
    q = torch.full((B, 2), float("nan"), dtype=torch.float32, device=dev) if return_quartiles else None
    no = torch.zeros(B, dtype=torch.int32, device=dev) if return_quartiles else None
    stats = TargetStats.empty()
    if x_packed.numel() > 0:
        x = x_packed.contiguous()
        lib = _lib.lib()
        ln = L.numpy()
        st_np, st_p = _i32(np.concatenate([[0], np.cumsum(ln)[:-1]]))
        ln_np, ln_p = _i32(ln)
        ws_bytes = int(lib.fs2_op_targets_workspace_bytes(B))
        with torch.cuda.device(dev):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            rec = torch.empty(12, dtype=torch.float64, device=dev)
            _lib.check(lib.fs2_op_clean_targets(_stream(dev), x.data_ptr(), B, st_p, ln_p, ws.data_ptr(), ws_bytes, y.data_ptr(),
                                                q.data_ptr() if return_quartiles else None, no.data_ptr() if return_quartiles else None,
                                                rec.data_ptr()))
            stats = TargetStats.from_record(rec.cpu().tolist())
    return (y, stats, q, no) if return_quartiles else (y, stats)


def remove_outlier(x_packed, lens):
    """The reference's ``remove_outlier`` (utils/util.py:34-49) of every utterance of a packed batch: a new tensor."""
    return clean_targets(x_packed, lens)[0]


def hp_data(energy_stats, pitch_stats):
    """The constants of the reference's config that come from compute_statistics.py, from the statistics of a corpus' cleaned energy
    and pitch: ``e_min`` / ``p_min`` are the non-zero minima, ``e_max`` / ``p_max`` the maxima (what FeedForwardTransformer builds
    its energy and pitch bucket boundaries from), ``e_mean``, ``e_std``, ``f0_mean``, ``f0_std`` the moments of the non-zero values.
    Raises ValueError if either has no positive value."""
    for name, s in (("energy", energy_stats), ("pitch", pitch_stats)):
        if not math.isfinite(s.nonzero_min):
            raise ValueError("the %s statistics hold no positive value (nonzero_min = %r over %d values): no bucket boundaries can be "
                             "built from them" % (name, s.nonzero_min, s.n_total))
    return dict(e_min=energy_stats.nonzero_min, e_max=energy_stats.max, p_min=pitch_stats.nonzero_min, p_max=pitch_stats.max,
                e_mean=energy_stats.mean, e_std=energy_stats.std, f0_mean=pitch_stats.mean, f0_std=pitch_stats.std)


class TrainingTargets(NamedTuple):
    logmel: torch.Tensor          # [frames, n_mels]
    energy: torch.Tensor          # [frames], cleaned
    f0: torch.Tensor              # [frames], cleaned
    frame_lens: torch.Tensor      # [B] int64 (CPU): sample_lens // hop + 1
    energy_stats: TargetStats
    pitch_stats: TargetStats


def training_targets(wav_packed, sample_lens, hp=None, f0_method="frame", **pitch_options):
    """Waveforms to the targets the model is taught with: ``wav_features`` (log-mel, energy, F0; the F0 is the autocorrelation
    estimator of :func:`fastspeech2_amd.vocoder.pitch`, not the reference's DIO, or with ``f0_method="path"`` that of
    :func:`fastspeech2_amd.vocoder.pitch_track`, the same candidates joined by a path search), then ``clean_targets`` of the energy
    and of the F0, in place.  ``logmel`` is ``wav_features``' bit for bit; the zeros of unvoiced frames stay zero."""
    lm, en, f0 = wav_features(wav_packed, sample_lens, hp=hp, f0_method=f0_method, **pitch_options)
    frame_lens = _lens(sample_lens, name="sample_lens") // _audio_config(hp)[1].hop + 1
    _, es = clean_targets(en, frame_lens, out=en)
    _, ps = clean_targets(f0, frame_lens, out=f0)
    return TrainingTargets(lm, en, f0, frame_lens, es, ps)
