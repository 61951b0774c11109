"""The vocode plan: what one call of ``GriffinLim`` consists of, decided once from plain values.

``plan_vocode`` takes no tensor and touches neither a device nor the library: a tensor argument reaches it as an ``Arg`` (what the
checks read of it), host frame counts as a tuple of ints.  It either raises one of the call's refusals -- in the order of REFUSALS
below, before anything is allocated or launched -- or returns a ``VocodePlan`` that ``GriffinLim`` only follows: which entry of
``_ENTRIES`` runs (and which one first, for the initial phase), the batch, the source, the iteration group, how the output is sized
and whether anything is launched at all.  What needs a tensor's contents or a device stays with the caller: the conversions
(``.contiguous().float()``, ``.reshape``), the constants, the allocations, the status record and the capture test.

REFUSALS per kind, first match wins (``mels`` stands for the source as the messages name it):

SYNTHESIS (``GriffinLim.__call__``)
   1  ``init`` unknown; ``init="spsi"`` with ``init_phase``; ``f0`` with ``init_phase``; ``init="f0"`` with ``init_phase``, without
      ``f0``, with bad ``f0_floor`` / ``f0_ceil``; ``f0`` without ``init="f0"``
   2  ``constraint`` unknown; ``constraint="mel"`` with ``magnitudes``
   sync:
   3  ``capacity`` / ``padded_out`` given
   sync=False:
   3  ``olens`` beside an AsyncMels
   4  ``olens`` no tensor; not int64; ``capacity`` < 1; ``olens`` not on a GPU
   both:
   5  ``mels`` no tensor (an AsyncMels with sync counts as none); not on a GPU; not [N, W] / [B, Lmax, W]; not on this GriffinLim's
      device; (sync=False) ``olens`` on another device
   6  ``n_iter`` < 0; ``momentum`` negative or not finite
   7  ``init_phase`` no tensor / not on a GPU; not in the layout of ``mels``
   8  ``init="f0"``: ``f0`` no tensor; not on a GPU; not float32; not one value per row; on another device
   sync:
   9  the frame counts: their number (padded), a negative one, their sum (packed) or an entry beyond Lmax (padded)
  10  (after the empty return) frames * bins or the samples reach 2^31
   sync=False:
   9  padded ``mels`` with another number of ``olens``; ``padded_out`` with packed ``mels``; ``capacity`` beyond the packed rows
  10  capacity * bins or the waveform's capacity reach 2^31

SPSI (``GriffinLim.spsi_phase``)
   1  an AsyncMels with sync; ``olens`` beside an AsyncMels
   2  sync=False: ``olens`` no CUDA int64 tensor
   3  as 5 above
   4  sync: the frame counts (as 9 above), then rows * bins reach 2^31;
      sync=False: padded ``src`` with another number of ``olens``, then rows * bins reach 2^31

F0 (``GriffinLim.f0_phase``) and EXCITATION (``GriffinLim.excitation``, which is always sync and takes no AsyncMels)
   1  bad ``f0_floor`` / ``f0_ceil``
   2  an AsyncMels with sync; ``olens`` beside it; an AsyncMels without pitch
   3  sync=False: ``olens`` no CUDA int64 tensor
   4  ``f0`` no tensor; not on a GPU; not float32; not [N] / [B, Lmax]
   5  sync=False: ``olens`` on another device
   6  rows * bins or rows * hop reach 2^31
   7  sync: the frame counts (as 9 above); sync=False: padded ``f0`` with another number of ``olens``
"""
import math
from collections import namedtuple
from itertools import accumulate

import torch

SYNTHESIS, SPSI, F0, EXCITATION = "synthesis", "spsi_phase", "f0_phase", "excitation"
INITS = ("seeded", "spsi", "f0")
CONSTRAINTS = ("magnitude", "mel")
LIMIT = 2 ** 31          # the kernels index with int32: no extent of a call reaches this

# what plan_vocode is told about a tensor argument (None: not given; is_tensor False: something else, of the type ``type_name``)
Arg = namedtuple("Arg", "type_name is_tensor is_cuda dtype shape device")

# (workspace query, call) of include/fs2.h and the groups of csrc/griffin_lim_host.h's GlCall its arguments are, in their order
Entry = namedtuple("Entry", "query call order n_out")      # n_out: the arguments of its output group
_SYN = ("stream", "geometry", "source", "batch", "iteration", "workspace", "output")
_MEL = ("stream", "geometry", "mel_source", "batch", "iteration", "workspace", "output")          # source with the mel basis behind pinv
_PHASE = ("stream", "geometry", "source", "batch", "workspace", "output")
_EXCITE = ("stream", "geometry", "f0_source", "batch", "f0_options", "workspace", "output")      # source: the f0 pointer alone
# by (kind, device batch, mel constraint): the one place a call picks its entry points
_ENTRIES = {
    (SYNTHESIS, False, False): Entry("fs2_op_vocode_workspace_bytes_geom", "fs2_op_griffin_lim_geom", _SYN, 1),
    (SYNTHESIS, False, True): Entry("fs2_op_vocode_mel_workspace_bytes_geom", "fs2_op_griffin_lim_mel_geom", _MEL, 1),
    (SYNTHESIS, True, False): Entry("fs2_op_vocode_workspace_bytes_cap", "fs2_op_griffin_lim_dev", _SYN, 5),
    (SYNTHESIS, True, True): Entry("fs2_op_vocode_mel_workspace_bytes_cap", "fs2_op_griffin_lim_mel_dev", _MEL, 5),
    (SPSI, False, False): Entry("fs2_op_spsi_workspace_bytes_geom", "fs2_op_spsi_phase_geom", _PHASE, 2),
    (SPSI, True, False): Entry("fs2_op_spsi_workspace_bytes_cap", "fs2_op_spsi_phase_dev", _PHASE, 2),
    (F0, False, False): Entry("fs2_op_f0_phase_workspace_bytes_geom", "fs2_op_f0_phase_geom", _EXCITE, 1),
    (F0, True, False): Entry("fs2_op_f0_phase_workspace_bytes_cap", "fs2_op_f0_phase_dev", _EXCITE, 1),
    (EXCITATION, False, False): Entry("fs2_op_f0_phase_workspace_bytes_geom", "fs2_op_excitation_geom", _EXCITE, 1),
}
_INIT_KIND = {"seeded": None, "spsi": SPSI, "f0": F0}

VocodePlan = namedtuple("VocodePlan", (
    "kind", "sync",
    "empty",                       # the call returns its empty result (allocated as below) and launches nothing
    "entry", "init_entry",         # the main stage, and the stage that computes the initial phase first (None: none): rows of _ENTRIES
    "B", "starts", "lens",         # host batch (sync): tuples of ints; else None
    "stride", "cap", "upstream",   # device batch: row stride (0 packed), frame capacity, whether an upstream status is passed
    "rows", "W", "pinv", "basis",  # source: its rows and width; whether pinv / the mel basis are passed
    "n_iter", "momentum", "seed",  # the iteration group as the call takes it (seed: masked to 32 bits; also the F0 stage's)
    "f0_options",                  # (f0_floor, f0_ceil, sample_rate) of an F0 stage, else None
    "out_shapes", "zero_fill",     # float32 outputs to allocate; phase [rows, bins] of the init stage is always zero-filled
    "wav_stride", "wav_cap", "padded",      # device synthesis: what the call takes, and AsyncWaveforms' flag
    "result_shape",                # the shape the (first) outputs are returned in
    "sample_lens"))                # host sample counts of a sync waveform call, else None


def _need_cuda(a, name):
    if a is None or not a.is_tensor:
        raise TypeError("%s must be a torch.Tensor" % name)
    if not a.is_cuda:
        raise RuntimeError("fastspeech2_amd runs on an MI355X only (no CPU fallback): %s is on %s" % (name, a.device))


def _fits(message, count, *extents):
    if any(e >= LIMIT for e in extents):
        raise ValueError(message % count)


def check_constraint(constraint, magnitudes):
    if constraint not in CONSTRAINTS:
        raise ValueError("constraint must be one of %s, got %r" % (CONSTRAINTS, constraint))
    if constraint == "mel" and magnitudes:
        raise ValueError("constraint='mel' needs log-mel frames: with magnitudes=True there is no mel to constrain to")
    return constraint == "mel"


def check_f0_limits(f0_floor, f0_ceil):
    """(f0_floor, f0_ceil) as floats: positive, finite and ordered (csrc/griffin_lim_host.h: f0_phase checks the same)."""
    lo, hi = float(f0_floor), float(f0_ceil)
    if not (lo > 0 and math.isfinite(lo) and math.isfinite(hi) and hi >= lo):
        raise ValueError("need 0 < f0_floor <= f0_ceil, both finite, got %r, %r" % (f0_floor, f0_ceil))
    return lo, hi


def check_init(init, has_init_phase, has_f0, f0_floor=71.0, f0_ceil=800.0):
    if init not in INITS:
        raise ValueError("init must be one of %s, got %r" % (INITS, init))
    if init == "spsi" and has_init_phase:
        raise ValueError("init='spsi' computes the initial phase itself: pass init_phase or init='spsi', not both")
    if has_f0 and has_init_phase:
        raise ValueError("f0 gives the initial phase (init='f0'): pass init_phase or f0, not both")
    if init == "f0":
        if has_init_phase:
            raise ValueError("init='f0' computes the initial phase itself: pass init_phase or init='f0', not both")
        if not has_f0:
            raise ValueError("init='f0' needs f0: one value in Hz per row of mels (or an AsyncMels of inference_batch_pitch)")
        check_f0_limits(f0_floor, f0_ceil)
    elif has_f0:
        raise ValueError("f0 belongs to init='f0', got init=%r" % (init,))


def _check_f0(f0, like, name="mels"):
    """``f0`` has one float32 value per row of ``like`` ([N, W] or [B, Lmax, W]; None: f0 itself is [N] or [B, Lmax]), on its device."""
    if f0 is None or not f0.is_tensor:
        raise TypeError("f0 must be a float32 CUDA tensor, got %s" % ("NoneType" if f0 is None else f0.type_name))
    _need_cuda(f0, "f0")
    if f0.dtype != torch.float32:
        raise TypeError("f0 must be float32 (Hz), got %s" % f0.dtype)
    if like is None:
        if len(f0.shape) not in (1, 2):
            raise ValueError("f0 must be [N] (packed) or [B, Lmax] (padded), got %s" % (f0.shape,))
    else:
        if f0.shape != like.shape[:-1]:
            raise ValueError("f0 must have one value per row of %s, %s, got %s" % (name, like.shape[:-1], f0.shape))
        if f0.device != like.device:
            raise ValueError("f0 on %s, %s on %s" % (f0.device, name, like.device))


def _check_source(src, W, own_device, olens):
    """What every call with mel / magnitude rows checks of them (and of a device ``olens``: that it lives where they do)."""
    _need_cuda(src, "mels")
    if len(src.shape) not in (2, 3) or src.shape[-1] != W:
        raise ValueError("mels must be [N, %d] (packed) or [B, Lmax, %d] (padded), got %s" % (W, W, src.shape))
    if own_device is not None and src.device != own_device:
        raise ValueError("mels on %s, this GriffinLim on %s" % (src.device, own_device))
    if olens is not None and olens.device != src.device:
        raise ValueError("olens on %s, mels on %s" % (olens.device, src.device))


def _device_olens(olens):
    if olens is None or not olens.is_tensor or not olens.is_cuda or olens.dtype != torch.int64:
        raise TypeError("olens must be a CUDA int64 tensor with sync=False (the frame counts stay on the device)")


def _async_source(sync, olens_clash, name, pitch=True):
    if sync:
        raise ValueError("an AsyncMels belongs to sync=False (its frame counts are on the device)")
    if olens_clash:
        raise ValueError("olens is taken from the AsyncMels given as %s; pass one or the other" % name)
    if not pitch:
        raise ValueError("this AsyncMels carries no pitch: call inference_batch_pitch(sync=False)")


def _host_batch(layout, lens, name="mels", have="have"):
    """(L [B], starts [B]) of packed rows (``layout`` (N,)) or padded ones (B, Lmax) with the host frame counts ``lens`` (None: one
    utterance of N rows / every utterance Lmax frames).  ``name``, ``have``: how the messages call the argument."""
    def counts(L, B=None):
        if B is not None and len(L) != B:
            raise ValueError("olens has %d entries for %d utterances" % (len(L), B))
        if any(n < 0 for n in L):
            raise ValueError("olens must be >= 0")
        return L
    if len(layout) == 1:
        N = layout[0]
        L = counts((N,) if lens is None else lens)
        if sum(L) != N:
            raise ValueError("packed %s: olens sum to %d, %s %s %d rows" % (name, sum(L), name, have, N))
        return L, tuple(accumulate(L, initial=0))[:-1]
    Bp, Lmax = layout
    L = counts((Lmax,) * Bp if lens is None else lens, Bp)
    if Bp and max(L) > Lmax:
        raise ValueError("padded %s: an olens entry exceeds Lmax = %d" % (name, Lmax))
    return L, tuple(range(0, Bp * Lmax, Lmax)) if Lmax else (0,) * Bp


def _device_batch(layout, olens):
    """(B, rows, stride, Lcap) of packed (stride 0, Lcap None) or padded (B, Lcap) rows whose frame counts stay on the device."""
    B = math.prod(olens.shape)
    if len(layout) == 1:
        return B, layout[0], 0, None
    if layout[0] != B:
        raise ValueError("olens has %d entries for %d utterances" % (B, layout[0]))
    return B, B * layout[1], layout[1], layout[1]


def plan_vocode(kind, sync, geometry, sample_rate, src, olens=None, lens=None, olens_clash=False, async_src=False, async_pitch=False,
                upstream=False, init_phase=None, f0=None, own_device=None, magnitudes=False, init="seeded", constraint="magnitude", n_iter=0,
                momentum=0.0, seed=0, capacity=None, padded_out=False, f0_floor=71.0, f0_ceil=800.0, return_magnitudes=False):
    """``geometry``: (n_fft, hop, win, n_mels); ``src``, ``olens``, ``init_phase``, ``f0``: ``Arg`` or None (``src`` of F0 / EXCITATION:
    the f0; ``olens``: what a sync=False call reads its counts from, an AsyncMels' own included); ``lens``: the host frame counts of
    a sync call (None: not given); ``olens_clash``: ``olens`` was given beside an AsyncMels; ``async_src`` / ``async_pitch``: the
    source came as an AsyncMels / one with a pitch; ``upstream``: it brought a status; ``own_device``: the GriffinLim's, if it has one."""
    n_fft, hop, _, n_mels = geometry
    NB = n_fft // 2 + 1
    dev_batch, mel, W, opts = not sync, False, None, None
    if kind == SYNTHESIS:
        check_init(init, init_phase is not None, f0 is not None, f0_floor, f0_ceil)
        mel = check_constraint(constraint, magnitudes)
        if sync:
            if capacity is not None or padded_out:
                raise ValueError("capacity / padded_out belong to sync=False (sync=True sizes the waveform from olens)")
        else:
            if olens_clash:
                raise ValueError("olens is taken from the AsyncMels given as mels; pass one or the other")
            if olens is None or not olens.is_tensor:
                raise TypeError("olens must be a CUDA int64 tensor with sync=False (the frame counts stay on the device), got %s"
                                % ("NoneType" if olens is None else olens.type_name))
            if olens.dtype != torch.int64:
                raise TypeError("olens must be int64 with sync=False, got %s" % olens.dtype)
            if capacity is not None and int(capacity) < 1:
                raise ValueError("capacity must be >= 1, got %r" % (capacity,))
            if not olens.is_cuda:
                raise TypeError("olens must be a CUDA int64 tensor with sync=False (the frame counts stay on the device), it is on %s; "
                                "use sync=True for host lengths" % olens.device)
        W = NB if magnitudes else n_mels
        _check_source(None if sync and async_src else src, W, own_device, None if sync else olens)
        n_iter, momentum = int(n_iter), float(momentum)
        if n_iter < 0:
            raise ValueError("n_iter must be >= 0")
        if not (momentum >= 0.0 and math.isfinite(momentum)):
            raise ValueError("momentum must be finite and >= 0")
        if init_phase is not None:
            _need_cuda(init_phase, "init_phase")
            if init_phase.shape[:-1] != src.shape[:-1] or init_phase.shape[-1] != NB:
                raise ValueError("init_phase must have the layout of mels with %d bins, got %s" % (NB, init_phase.shape))
        if init == "f0":
            _check_f0(f0, src)
            opts = check_f0_limits(f0_floor, f0_ceil) + (int(sample_rate),)
        layout, names = src.shape[:-1], ("mels", "have")
    elif kind == SPSI:
        if async_src:
            _async_source(sync, olens_clash, "src")
        if not sync:
            _device_olens(olens)
        W = NB if magnitudes else n_mels
        _check_source(src, W, own_device, None if sync else olens)
        layout, names = src.shape[:-1], ("src", "has")
    else:
        opts = check_f0_limits(f0_floor, f0_ceil) + (int(sample_rate),)
        if async_src:
            _async_source(sync, olens_clash, "f0", async_pitch)
        if not sync:
            _device_olens(olens)
        _check_f0(src, None)
        if not sync and olens.device != src.device:
            raise ValueError("olens on %s, f0 on %s" % (olens.device, src.device))
        layout, names = src.shape, ("f0", "has")
        rows = math.prod(layout)
        _fits("batch too large for one call (%d rows)", rows, rows * NB, rows * hop)

    B = starts = L = sample_lens = Lcap = None
    stride = cap = 0
    if sync:
        L, starts = _host_batch(layout, lens, *names)
        B, rows, frames = len(L), math.prod(layout), sum(L)
    else:
        B, rows, stride, Lcap = _device_batch(layout, olens)
        cap = rows
    entry, init_entry = _ENTRIES[kind, dev_batch, mel], None
    wav_stride = wav_cap = 0
    padded = False
    if kind == SYNTHESIS and sync or kind == EXCITATION:
        sample_lens = tuple([hop * max(n - 1, 0) for n in L])
        total = sum(sample_lens)
        out_shapes = result_shape = ((total,),)
        empty = total == 0 or frames == 0
        if kind == SYNTHESIS and not empty:
            _fits("batch too large for one call (%d frames)", frames, frames * NB, total)
    elif kind == SYNTHESIS:
        if Lcap is None and padded_out:
            raise ValueError("padded_out needs padded mels [B, Lcap, %d] (the waveform's row length is hop * (Lcap - 1))" % W)
        if Lcap is None and capacity is not None and int(capacity) > rows:
            raise ValueError("capacity %d exceeds the %d rows of the packed mels" % (int(capacity), rows))
        cap = rows if capacity is None else min(int(capacity), rows)
        padded = bool(padded_out)
        wav_stride = hop * (Lcap - 1) if padded and Lcap >= 2 else 0
        wav_cap = B * wav_stride if padded else hop * max(cap - 1, 0)        # (padded_out at Lcap < 2: no utterance owns a sample)
        _fits("capacity too large for one call (%d frames)", cap, cap * NB, wav_cap)
        out_shapes, result_shape = ((wav_cap,),), ((B, wav_stride) if padded else (wav_cap,),)
        empty = B == 0 or cap == 0
    else:
        if kind == SPSI:
            _fits("batch too large for one call (%d rows)", rows, rows * NB)
        out_shapes = ((rows, NB),) * (2 if return_magnitudes else 1)
        result_shape = (layout + (NB,),) * len(out_shapes)
        empty = frames == 0 if sync else (B == 0 or rows == 0)
    if kind == SYNTHESIS and _INIT_KIND[init] is not None:
        init_entry = _ENTRIES[_INIT_KIND[init], dev_batch, False]
    return VocodePlan(kind, bool(sync), empty, entry, init_entry, B, starts, L, stride, cap, bool(upstream) and not sync, rows, W,
                      W is not None and not magnitudes, mel, n_iter if kind == SYNTHESIS else None, momentum if kind == SYNTHESIS else None,
                      int(seed) & 0xFFFFFFFF, opts, out_shapes, kind in (SPSI, F0), wav_stride, wav_cap, padded, result_shape, sample_lens)
