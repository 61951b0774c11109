"""Griffin-Lim vocoder: packed mel frames -> waveforms on the MI355X (csrc/griffin_lim.h, include/fs2.h: fs2_op_griffin_lim).

The reference's only self-contained way from a mel to a wav is Griffin-Lim (reference inference.py:195-199,
dataset/audio_processing.py:224-240, utils/stft.py:41-151), with the transform of configs/default.yaml: n_fft = win_length = 1024,
hop 256, periodic Hann window.  As written it feeds the 80-bin mel where the 513-bin magnitude belongs; here the mel is first mapped
back to magnitudes with the pseudo-inverse of the mel filterbank it was made with (``M = max(pinv(B) . exp(mel), 0)``: the inverse of
TacotronSTFT's log(clamp(B . |S|, 1e-5)), stft.py:188-204).  The whole batch is vocoded in one call, every utterance with its own
STFT (reflect padding at its own ends), nothing goes through the host, and an utterance's waveform is bit-identical whether it is
vocoded alone or inside any batch.

``stft_magnitude`` is the analysis direction (TacotronSTFT.mel_spectrogram): waveforms -> |STFT| or log-mel on the GPU;
``mel_energy`` gives the log-mel and the per-frame energy (the reference preprocessing's targets) from one launch; ``wav_features``
adds a per-frame F0 from the same launch and ``pitch`` gives it alone (an autocorrelation estimator, not the reference's DIO);
``pitch_candidates`` / ``pitch_path`` / ``pitch_track`` add the path search across frames (``f0_method="path"``).  Other transform
geometries (n_fft 512 / 1024 / 2048, any hop <= win_length <= n_fft with ceil(n_fft / hop) <= 8, 1 .. 128 mels) come from hp.audio.
There is no CPU fallback: CPU tensors raise.

``GriffinLim(...)(..., sync=False)`` is the device-driven form (fs2_op_griffin_lim_dev): the frame counts stay
on the device (an ``AsyncMels`` of ``inference_batch(sync=False)`` can be passed as it is), the tiles are planned by kernels inside
capacities, nothing waits for the GPU and the call can be captured into a HIP graph; it returns an ``AsyncWaveforms``.
"""
import ctypes as C
import math
import wave
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._host import _i32, _lens, _require_cuda, _stream
from ._vocode_plan import CONSTRAINTS, EXCITATION, F0, INITS, SPSI, SYNTHESIS, Arg, plan_vocode       # noqa: F401  (INITS, CONSTRAINTS: public here)
from .fastspeech import AsyncMels, Fs2CapacityError
from .losses import DeviceRecords

N_FFT, HOP, WIN, N_BINS = 1024, 256, 1024, 513
_AUDIO_DEFAULTS = dict(sample_rate=22050, n_fft=1024, n_mels=80, fmin=0.0, fmax=8000.0)


# ---- Slaney mel filterbank (what librosa.filters.mel computes by default, htk=False, norm="slaney"; reference stft.py:173) ----
def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_basis(sample_rate=22050, n_fft=1024, n_mels=80, fmin=0.0, fmax=8000.0):
    """Slaney mel filterbank [n_mels, 1 + n_fft // 2] (float64): triangles between mel-spaced edges (linear below 1 kHz, logarithmic
    above), each scaled to unit area (2 / (f[i+2] - f[i]))."""
    fftfreqs = np.linspace(0.0, sample_rate / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:n_mels] / fdiff[:n_mels, None]
    upper = ramps[2:n_mels + 2] / fdiff[1:n_mels + 1, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    return weights * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


class Geometry(NamedTuple):
    """The STFT a GriffinLim / stft_magnitude works in (the reference's STFT(filter_length, hop_length, win_length) and TacotronSTFT's
    n_mel_channels).  The window is a periodic Hann of ``win`` samples zero-padded to ``n_fft`` at the centre."""
    n_fft: int = N_FFT
    hop: int = HOP
    win: int = WIN
    n_mels: int = 80

    @property
    def n_bins(self):
        return self.n_fft // 2 + 1

    @property
    def l_min(self):
        """Fewest frames an utterance needs for the reference's reflect padding (hop (L - 1) > n_fft / 2); shorter ones give zeros."""
        return self.n_fft // (2 * self.hop) + 2


SUPPORTED_N_FFT = (512, 1024, 2048)
MAX_MELS = 128


def check_geometry(g):
    """Raise ValueError unless the kernels implement ``g`` (include/fs2.h: fs2_op_griffin_lim_geom)."""
    if g.n_fft not in SUPPORTED_N_FFT:
        raise ValueError("n_fft must be one of %s (radix-2/4/8 transforms only), got %r" % (SUPPORTED_N_FFT, g.n_fft))
    if not (1 <= g.hop <= g.win <= g.n_fft):
        raise ValueError("need hop <= win_length <= n_fft, got hop %r, win_length %r, n_fft %r" % (g.hop, g.win, g.n_fft))
    if -(-g.n_fft // g.hop) > 8:
        raise ValueError("ceil(n_fft / hop) must be <= 8 (a sample lies in at most 8 frames), got n_fft %d, hop %d" % (g.n_fft, g.hop))
    if not 1 <= g.n_mels <= MAX_MELS:
        raise ValueError("n_mels must be 1 .. %d, got %r" % (MAX_MELS, g.n_mels))
    return g


def _audio_config(hp):
    """(mel_basis arguments, Geometry) from hp.audio.  The transform defaults to 1024 / 256 / 1024; any other one must be named in
    full (n_fft, hop_length and win_length together, as the reference's preprocessing reads all three): a partial departure raises
    and names what is missing, the transform is never guessed.  n_mels: hp.audio.n_mels, else hp.audio.num_mels, else 80."""
    p = dict(_AUDIO_DEFAULTS)
    a = getattr(hp, "audio", None) if hp is not None else None
    tr = {}
    if a is not None:
        get = a.get if hasattr(a, "get") else (lambda k, d=None: getattr(a, k, d))
        for k in ("sample_rate", "fmin", "fmax"):
            if get(k, None) is not None:
                p[k] = type(_AUDIO_DEFAULTS[k])(get(k))
        nm = get("n_mels", None)
        nm = get("num_mels", None) if nm is None else nm
        if nm is not None:
            p["n_mels"] = int(nm)
        tr = {k: int(get(k)) for k in ("n_fft", "hop_length", "win_length") if get(k, None) is not None}
    default = dict(n_fft=N_FFT, hop_length=HOP, win_length=WIN)
    if any(tr[k] != default[k] for k in tr) and len(tr) < 3:
        named = ", ".join("%s = %d" % (k, v) for k, v in tr.items())
        missing = ", ".join(k for k in default if k not in tr)
        raise ValueError("hp.audio departs from the default transform (n_fft 1024, hop_length 256, win_length 1024) with %s but does not "
                         "name %s: a transform other than the default must name n_fft, hop_length and win_length together" % (named, missing))
    tr = dict(default, **tr)
    g = check_geometry(Geometry(tr["n_fft"], tr["hop_length"], tr["win_length"], p["n_mels"]))
    p["n_fft"] = g.n_fft
    return p, g


# ---- tile rule of csrc/griffin_lim.h (gl_halo, gl_tail, gl_lmin, gl_sig_max, gl_tile_frames), restated for the host checks ----
LDS_BYTES = 163840


def tile_rule(n_fft, hop):
    """dict(F, halo, tail, lmin, sig_max) of the fused kernel at (n_fft, hop): frames per tile, halo frames each side, the extra frame
    L - tail of a tile at the utterance's end, L_min, and the signal buffer (floats).  F: the largest of 32, 16, ... whose LDS fits."""
    R = -(-n_fft // hop)
    halo, tail, lmin = max(R - 1, 1), n_fft // hop + 1, n_fft // (2 * hop) + 2
    sig = lambda F: hop * (F + 2 * halo - 1) + n_fft
    F = 32
    if not (n_fft == N_FFT and hop == HOP):
        while F > 1 and 28 * n_fft + 4 * sig(F) > LDS_BYTES:
            F //= 2
    return dict(F=F, halo=halo, tail=tail, lmin=lmin, sig_max=sig(F))


def tile_span(n_fft, hop, L, f0, rule=None):
    """Frames [fa, fb] the tile starting at f0 inverse-transforms (its own frames, the halo and the reflection's extra frame)."""
    r = rule or tile_rule(n_fft, hop)
    nf = min(r["F"], L - f0)
    return max(0, min(f0 - r["halo"], L - r["tail"])), min(L - 1, f0 + nf - 1 + r["halo"])


# ---- slot rule of the device-driven planner (csrc/gl_slot_rule.h: gl_tile_count, gl_slot_capacity, gl_slot_tile), restated ----
def slot_capacity(frame_capacity, F, B):
    """Workgroups of a device-driven call: enough for the tiles of any batch of B utterances with sum L <= frame_capacity."""
    return int(frame_capacity) // int(F) + int(B)


def slot_tiles(lens, F, frame_capacity):
    """int array [slots, 2] of (utterance, first frame) the planner gives each slot, (-1, 0) for a slot without a tile: the batch's
    tiles in batch order (``f0 = 0, F, 2F, ..`` per utterance with L >= 2), found as the kernel finds them, by binary search in the
    inclusive prefix sum of the tile counts."""
    L = np.asarray(lens, np.int64).reshape(-1)
    F = int(F)
    counts = np.where(L >= 2, -(-L // F), 0)
    end = np.cumsum(counts)
    slots = np.arange(slot_capacity(frame_capacity, F, L.size), dtype=np.int64)
    b = np.searchsorted(end, slots, side="right")             # first b with end[b] > slot
    out = np.zeros((slots.size, 2), np.int64)
    out[:, 0] = -1
    has = b < L.size
    bb = b[has]
    out[has, 0] = bb
    out[has, 1] = (slots[has] - (end[bb] - counts[bb])) * F
    return out


# ---- seeded initial phase: the formula of csrc/griffin_lim.h (gl_seed_angle), restated ----
def _mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def seed_angles(seed, n_frames, n_bins=N_BINS):
    """Initial angles [n_frames, n_bins] (float32) of an utterance for ``seed``: uniform on [-pi, pi) from a counter-based hash of
    (seed, utterance-local frame, bin) = hash(k + n_bins f), exactly as the kernel computes them."""
    with np.errstate(over="ignore"):
        f = np.arange(n_frames, dtype=np.uint32)[:, None]
        k = np.arange(n_bins, dtype=np.uint32)[None, :]
        s = _mix32(np.uint32((int(seed) + 0x9E3779B9) & 0xFFFFFFFF))
        h = _mix32((k + np.uint32(n_bins) * f) ^ s)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u * np.float32(6.28318548) - np.float32(3.14159274)


class Waveforms(NamedTuple):
    """Packed float32 waveforms (device) and the samples of each utterance (host int64): utterance b starts at sum(sample_lens[:b])."""
    wav: torch.Tensor
    sample_lens: torch.Tensor

    def split(self):
        return split(self.wav, self.sample_lens)


def split(wav, sample_lens):
    """Packed waveform -> list of per-utterance tensors (views)."""
    return list(torch.split(wav, [int(n) for n in sample_lens]))


FS2_OVF_UPSTREAM = 32    # include/fs2.h: the producer of the frames had flagged its own status


class _WavRecord:
    """Status of one sync-free vocoder call, copied to pinned host memory behind its kernels.  The pinned block belongs to a ring:
    the first look after the event has fired moves the flags into the record (a block is resolved before another call gets it)."""
    __slots__ = ("event", "pin", "_status")

    def __init__(self, event, pin):
        self.event, self.pin, self._status = event, pin, None

    def status(self):
        if self._status is None:
            self.event.synchronize()
            self._status = [int(v) for v in self.pin]
            self.pin = None
        return self._status


class AsyncWaveforms(tuple):
    """What ``GriffinLim(...)(..., sync=False)`` returns: unpacks like ``(wav, sample_lens_dev)`` -- ``wav`` float32 [capacity]
    whose first ``sum(sample_lens)`` samples are the utterances back to back and the rest zero, or with ``padded_out=True``
    [B, hop (Lcap - 1)] zero-padded; ``sample_lens_dev`` a DEVICE int64 [B].  ``status`` is the device int32[8] of
    fs2_op_griffin_lim_dev ({frames, tiles, flags, longest utterance, valid samples, ...}).  ``ok()`` waits for THIS call (its own
    event and pinned copy of the status) and tells whether its capacities sufficed and its frame counts were valid; ``check()``
    raises ``Fs2CapacityError`` instead.  On any flag the whole ``wav`` is NaN and ``sample_lens_dev`` zero.  A call made under
    stream capture keeps no host-side record: read ``status`` after the replay."""

    def __new__(cls, wav, sample_lens, status, record, padded=False):
        self = super().__new__(cls, (wav, sample_lens))
        self.status, self._record, self.padded = status, record, padded
        return self

    @property
    def wav(self):
        return self[0]

    @property
    def sample_lens(self):
        return self[1]

    def flags(self):
        """The flag word of this call (waits for it); 0 for a call captured into a graph, which keeps no record."""
        return 0 if self._record is None else self._record.status()[2]

    def ok(self):
        return self.flags() == 0

    def check(self):
        fl = self.flags()
        if fl:
            why = "the mel call that produced the frames had flagged its own status" if fl & FS2_OVF_UPSTREAM else \
                "a capacity was too small or a frame count invalid"
            raise Fs2CapacityError("device-driven vocoder: %s (flags %d); the waveforms of the call are NaN-filled: rerun with "
                                   "sync=True or a larger capacity" % (why, fl))
        return self

    def split(self):
        """List of per-utterance waveforms (views).  WAITS for the call: the sample counts are read back to the host."""
        self.check()
        n = [int(v) for v in self[1].cpu()]
        if self.padded:
            return [self[0][b, :k] for b, k in enumerate(n)]
        return list(torch.split(self[0][:sum(n)], n))


# ---- what plan_vocode (_vocode_plan.py) is told about a call's arguments: plain values, read here ----
def _describe(x):
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        return Arg(type(x).__name__, False, False, None, None, None)
    return Arg(type(x).__name__, True, x.is_cuda, x.dtype, tuple(x.shape), x.device)


def _host_lens(olens):
    """Host frame counts as a tuple of ints (a CUDA ``olens`` is copied back, which waits for the GPU); None stays None."""
    return None if olens is None else tuple(torch.as_tensor(olens).detach().to("cpu", torch.int64).reshape(-1).tolist())


def _async_parts(x, olens):
    """(rows, olens, status, pitch, whether ``x`` is an AsyncMels, whether ``olens`` was given beside one) of a source argument: an
    AsyncMels is taken apart, its own frame counts standing in where none were given; anything else passes through."""
    if not isinstance(x, AsyncMels):
        return x, olens, None, None, False, False
    return x[0], x[1] if olens is None else olens, x.status, getattr(x, "pitch", None), True, olens is not None


class GriffinLim:
    """Griffin-Lim on the GPU, batched.  ``GriffinLim(hp)(mels, olens)`` -> ``Waveforms(wav_packed, sample_lens)``.

    The transform comes from hp.audio (``geometry``; default n_fft = win_length = 1024, hop 256, 80 mel bins).  An utterance of L
    frames gives hop (L - 1) samples (the reference's STFT.inverse trims n_fft / 2 at both ends); L < L_min = n_fft // (2 hop) + 2
    (4 at the default) is too short for the reference's reflect padding and gives hop (L - 1) zeros (none for L <= 1), without
    failing the batch."""

    def __init__(self, hp=None, device=None):
        self.params, self.geometry = _audio_config(hp)
        self.device = torch.device(device) if device is not None else None
        B = mel_basis(**self.params)
        if not (np.isfinite(B).all() and (B >= 0).all()):       # the mel-constrained projection divides by the column sums
            raise ValueError("the mel basis of hp.audio must be finite and non-negative")
        self._basis_np = B
        self._pinv_np = np.linalg.pinv(B)          # [bins, n_mels], float64 on the host
        self._dev = {}
        self._pin_ring, self._pin_next = [], 0     # pinned status blocks of the sync=False calls (_record)

    def constants(self, device):
        """(pinv [bins, n_mels], mel basis [n_mels, bins]) as fp32 tensors on ``device``."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = (torch.tensor(self._pinv_np, dtype=torch.float32, device=device).contiguous(),
                                 torch.tensor(self._basis_np, dtype=torch.float32, device=device).contiguous())
        return self._dev[device]

    def __call__(self, mels, olens=None, n_iter=30, momentum=0.0, seed=0, init_phase=None, magnitudes=False, sync=True, capacity=None,
                 padded_out=False, init="seeded", constraint="magnitude", f0=None, f0_floor=71.0, f0_ceil=800.0):
        """mels: packed [N, n_mels] (``inference_batch(packed=True)``) with ``olens`` [B] summing to N, or padded [B, Lmax, n_mels]
        with ``olens`` [B] <= Lmax (None: every utterance Lmax frames; packed: one utterance).  ``magnitudes=True``: linear magnitudes
        [.., n_fft / 2 + 1] instead (the reference's ``griffin_lim(magnitudes, ...)`` contract).  ``init_phase``: angles in the layout
        of ``mels`` with n_fft / 2 + 1 bins, or None: seeded.  ``init="spsi"``: start from the phase-continuity phase of
        :func:`spsi_phase` instead of the seeded random one (``seed`` is ignored; together with ``init_phase`` it raises): on
        harmonic signals 10 iterations from it beat 20 from the seeded start.  ``momentum`` > 0: fast
        Griffin-Lim (0 = the reference).  Runs on the current stream of the input's device without synchronising.

        ``init="f0"``: start from the phase of an excitation built from ``f0`` (:func:`f0_phase`; float32 Hz, one value per row of
        ``mels``, packed or padded like them; a frame is voiced where ``f0_floor <= f0 <= f0_ceil``; ``seed`` seeds the noise of the
        unvoiced stretches).  With ``n_iter=0`` this is a one-pass source-filter vocoder: the magnitudes filter the excitation and
        the pitch of the waveform is ``f0``.  It is for few iterations and an ``f0`` that matches the
        mel, which the model's own prediction does: an ``AsyncMels`` of ``inference_batch_pitch(sync=False)`` brings
        its pitch along.  Without ``f0``, together with ``init_phase``, or with ``f0`` of another shape, dtype or device it raises.

        ``constraint="magnitude"`` (default) projects every iteration onto the fixed ``M = max(pinv . exp(mel), 0)``.
        ``constraint="mel"`` keeps the magnitudes of the current STFT and rescales them per mel band so that their mel is the
        given one (fs2_op_griffin_lim_mel_geom / _dev): the waveform's log-mel then lies much closer to
        ``mels``.  It needs log-mel frames (with ``magnitudes=True`` it raises) and composes with ``init``, ``init_phase``,
        ``momentum`` and ``sync=False``; ``n_iter=0`` is the same in both.

        ``sync=True`` reads ``olens`` on the host (a CUDA ``olens`` is copied back, which waits for the GPU) and sizes the result
        from it.  ``sync=False``: the frame counts stay on the device -- ``olens`` must be a CUDA int64 tensor, or ``mels`` an
        :class:`AsyncMels` (``inference_batch(sync=False)``), whose mels, ``olens`` and status are taken -- and nothing waits for
        the GPU (include/fs2.h: fs2_op_griffin_lim_dev).  Returns an :class:`AsyncWaveforms`.  ``capacity``: bound on the batch's total
        frames (default: the rows of a packed ``mels``, B * Lcap of a padded one); the tiles are planned on the GPU inside it and the
        waveform is sized from it: packed float32 [hop * (capacity - 1)], or with ``padded_out=True`` (padded ``mels`` only)
        [B, hop (Lcap - 1)].  Frame counts that are negative, sum beyond ``capacity`` or exceed Lcap, and an ``AsyncMels`` whose own
        call overflowed, give a NaN-filled ``wav``, zero ``sample_lens`` and ``ok() == False``.  ``init="spsi"`` / ``init="f0"``
        compute the initial phase on the device from the same frame counts first (fs2_op_spsi_phase_dev, fs2_op_f0_phase_dev),
        equally without a host read; an ``AsyncMels`` with a ``pitch`` brings its own ``f0``."""
        lens = _host_lens(olens) if sync else None
        mels, olens, status, pitch, was_async, clash = _async_parts(mels, olens)
        if f0 is None and init == "f0":
            f0 = pitch
        p = plan_vocode(SYNTHESIS, sync, self.geometry, self.params["sample_rate"], _describe(mels), None if sync else _describe(olens), lens, clash,
                        was_async, pitch is not None, status is not None, _describe(init_phase), _describe(f0), self.device, magnitudes, init,
                        constraint, n_iter, momentum, seed, capacity, padded_out, f0_floor, f0_ceil)
        dev = mels.device
        src = mels.reshape(-1, p.W).contiguous().float()
        if init_phase is not None:
            init_phase = init_phase.reshape(-1, self.geometry.n_bins).contiguous().float()
        if p.f0_options is not None:
            f0 = f0.reshape(-1).contiguous()
        if sync:
            wav = torch.empty(p.out_shapes[0], dtype=torch.float32, device=dev)
            if not p.empty:
                self._run(p, dev, src, f0, None, None, init_phase, (wav.data_ptr(),))
            return Waveforms(wav, torch.tensor(p.sample_lens, dtype=torch.int64))
        olens = olens.reshape(-1).contiguous()
        with torch.cuda.device(dev):
            wav = torch.empty(p.wav_cap, dtype=torch.float32, device=dev)
            shaped = wav.reshape(p.result_shape[0])
            if p.empty:
                return AsyncWaveforms(shaped, torch.zeros(p.B, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                                      None, p.padded)
            sample_lens = torch.empty(p.B, dtype=torch.int64, device=dev)        # both written in full by the planner
            done = torch.empty(8, dtype=torch.int32, device=dev)
            self._run(p, dev, src, f0, olens, status, init_phase,
                      (wav.data_ptr() if p.wav_cap else None, p.wav_stride, p.wav_cap, sample_lens.data_ptr(), done.data_ptr()))
            rec = None if torch.cuda.is_current_stream_capturing() else self._record(done, dev)
        return AsyncWaveforms(shaped, sample_lens, done, rec, p.padded)

    def spsi_phase(self, src, olens=None, magnitudes=False, return_magnitudes=False, sync=True):
        """The phase-continuity initial phase (:func:`spsi_phase`) in this GriffinLim's geometry."""
        lens = _host_lens(olens) if sync else None
        src, olens, status, _, was_async, clash = _async_parts(src, olens)
        p = plan_vocode(SPSI, sync, self.geometry, self.params["sample_rate"], _describe(src), None if sync else _describe(olens), lens, clash,
                        was_async, upstream=status is not None, own_device=self.device, magnitudes=magnitudes, return_magnitudes=return_magnitudes)
        dev = src.device
        outs = [torch.zeros(s, dtype=torch.float32, device=dev) for s in p.out_shapes]
        if not p.empty:
            self._run(p, dev, src.reshape(-1, p.W).contiguous().float(), None, None if sync else olens.reshape(-1).contiguous(), status, None,
                      (outs[0].data_ptr(), outs[1].data_ptr() if return_magnitudes else None))
        outs = [o.reshape(s) for o, s in zip(outs, p.result_shape)]
        return tuple(outs) if return_magnitudes else outs[0]

    def f0_phase(self, f0, olens=None, f0_floor=71.0, f0_ceil=800.0, seed=0, sync=True):
        """The phase of the excitation from F0 (:func:`f0_phase`) in this GriffinLim's geometry and sample rate."""
        lens = _host_lens(olens) if sync else None
        rows, olens, status, pitch, was_async, clash = _async_parts(f0, olens)
        f0 = pitch if was_async else rows
        p = plan_vocode(F0, sync, self.geometry, self.params["sample_rate"], _describe(f0), None if sync else _describe(olens), lens, clash,
                        was_async, pitch is not None, status is not None, seed=seed, f0_floor=f0_floor, f0_ceil=f0_ceil)
        dev = f0.device
        phase = torch.zeros(p.out_shapes[0], dtype=torch.float32, device=dev)
        if not p.empty:
            self._run(p, dev, None, f0.reshape(-1).contiguous(), None if sync else olens.reshape(-1).contiguous(), status, None, (phase.data_ptr(),))
        return phase.reshape(p.result_shape[0])

    def excitation(self, f0, olens=None, seed=0, f0_floor=71.0, f0_ceil=800.0):
        """The excitation from F0 itself (:func:`excitation`) at this GriffinLim's hop and sample rate -> ``Waveforms``."""
        p = plan_vocode(EXCITATION, True, self.geometry, self.params["sample_rate"], _describe(f0), None, _host_lens(olens), seed=seed,
                        f0_floor=f0_floor, f0_ceil=f0_ceil)
        wav = torch.empty(p.out_shapes[0], dtype=torch.float32, device=f0.device)
        if not p.empty:
            self._run(p, f0.device, None, f0.reshape(-1).contiguous(), None, None, None, (wav.data_ptr(),))
        return Waveforms(wav, torch.tensor(p.sample_lens, dtype=torch.int64))

    def _run(self, p, dev, src, f0, olens, status, init_phase, output):
        """Follow the stages of plan ``p`` on converted inputs: the one that computes the initial phase, if it names one, then its
        main one, which writes ``output`` (its output group).  The groups are those of csrc/griffin_lim_host.h's GlCall."""
        if p.sync:
            s_np, s_p = _i32(p.starts)
            l_np, l_p = _i32(p.lens)
            size, groups = (p.B, l_p), dict(batch=(p.B, s_p, l_p))
        else:
            size = (p.B, p.cap)
            groups = dict(batch=(p.B, olens.data_ptr(), p.stride, p.cap, status.data_ptr() if p.upstream else None))
        if p.W is not None:
            pinv, basis = self.constants(dev)
            groups["source"] = (src.data_ptr(), p.W, pinv.data_ptr() if p.pinv else None)
            if p.basis:
                groups["mel_source"] = groups["source"] + (basis.data_ptr(),)
        if p.f0_options is not None:
            groups.update(f0_source=(f0.data_ptr(),), f0_options=p.f0_options + (p.seed,))
        if p.init_entry is not None:
            init_phase = torch.zeros(p.rows, self.geometry.n_bins, dtype=torch.float32, device=dev)      # zeros where no utterance is
            self._launch(p.init_entry, dev, size, groups, (init_phase.data_ptr(),) + (None,) * (p.init_entry.n_out - 1))
        if p.kind == SYNTHESIS:
            groups["iteration"] = (p.n_iter, p.momentum, p.seed, init_phase.data_ptr() if init_phase is not None else None)
        self._launch(p.entry, dev, size, groups, output)

    def _launch(self, entry, dev, size, groups, output):
        """The one launch site.  ``entry``: a row of _vocode_plan._ENTRIES.  Query its workspace (``size``: what the query takes after
        the geometry), allocate it, and make the call with the argument groups in the order the row names."""
        lib, g = _lib.lib(), self.geometry
        ws_bytes = int(getattr(lib, entry.query)(*g, *size))
        with torch.cuda.device(dev):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            groups = dict(groups, stream=(_stream(dev),), geometry=g, workspace=(ws.data_ptr(), ws_bytes), output=output)
            _lib.check(getattr(lib, entry.call)(*[a for name in entry.order for a in groups[name]]))

    _PIN_SLOTS = 16

    def _record(self, status, dev):
        """Queue a pinned copy of a call's status behind its kernels; an event tells when it is there."""
        ring = self._pin_ring
        if len(ring) < self._PIN_SLOTS:
            ring.append([torch.empty(8, dtype=torch.int32).pin_memory(), None])
            slot = ring[-1]
        else:
            slot, self._pin_next = ring[self._pin_next], (self._pin_next + 1) % self._PIN_SLOTS
            if slot[1] is not None:
                slot[1].status()                   # a call still in flight owns the block: wait for it and keep its values
        slot[0].copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        slot[1] = _WavRecord(ev, slot[0])
        return slot[1]


_DEFAULT_GL = None


def _gl_for(hp):
    """The GriffinLim (geometry, mel basis) of ``hp``; the default one is kept."""
    global _DEFAULT_GL
    if hp is not None:
        return GriffinLim(hp)
    if _DEFAULT_GL is None:
        _DEFAULT_GL = GriffinLim()
    return _DEFAULT_GL


def spsi_phase(src, olens=None, hp=None, magnitudes=False, return_magnitudes=False, sync=True):
    """Initial phase for Griffin-Lim from the magnitudes alone: Single Pass Spectrogram Inversion (Beauregard, Harish and Wyse 2015;
    csrc/gl_spsi.h, include/fs2.h: fs2_op_spsi_phase_geom).  Per frame the spectral peaks are found, each
    peak's frequency is refined with a parabola, and its phase advances by hop times that frequency from the phase its bin had in the
    previous frame; the bins around a peak follow it.  ``src``, ``olens`` and ``magnitudes`` as in ``GriffinLim.__call__`` (log-mel
    frames [.., n_mels], or magnitudes [.., n_fft / 2 + 1]), in the geometry of ``hp.audio``.  Returns the angles (radians in
    [0, 2 pi)) in the layout of ``src`` with n_fft / 2 + 1 columns, zeros in the rows no utterance covers: what ``init_phase=`` takes
    (``GriffinLim()(mels, olens, init="spsi")`` does both).  ``return_magnitudes=True``: also the magnitudes the phase was computed
    from, in the same layout.  ``sync=False``: ``olens`` is a CUDA int64 tensor (or ``src`` an ``AsyncMels``) and nothing waits for
    the GPU; invalid frame counts leave the phase zero (the vocoder call that follows reports them).  Every utterance with at least
    one frame is computed; an utterance's phase is bit-identical alone or in any batch.  CPU tensors raise."""
    return _gl_for(hp).spsi_phase(src, olens, magnitudes=magnitudes, return_magnitudes=return_magnitudes, sync=sync)


def f0_phase(f0, olens=None, hp=None, f0_floor=71.0, f0_ceil=800.0, seed=0, sync=True):
    """Initial phase for Griffin-Lim from an F0 contour (csrc/gl_excite.h, include/fs2.h: fs2_op_f0_phase_geom, DESIGN.md section
    14.12): the STFT phase of an excitation -- a band-limited pulse train of the frequency ``f0`` where voiced, hashed noise where not.
    ``f0``: float32 Hz on the GPU, one value per frame, packed [N] with ``olens`` [B] summing to N or padded [B, Lmax] with ``olens``
    <= Lmax, in the geometry and at the sample rate of ``hp.audio``; a frame is voiced where ``f0_floor <= f0 <= f0_ceil`` (NaN,
    infinities, 0 and negative values are unvoiced), a stretch between two frames where both are.  Returns the angles (float32 radians)
    in the layout of ``f0`` with n_fft / 2 + 1 columns, zeros in the rows no utterance covers and in utterances too short for the
    reflect padding: what ``init_phase=`` takes (``GriffinLim()(mels, olens, init="f0", f0=f0)`` does both).  ``seed`` changes the
    unvoiced stretches only.  ``sync=False``: ``olens`` is a CUDA int64 tensor and nothing waits for the GPU; invalid frame counts
    leave the phase zero (the vocoder call that follows reports them).  An utterance's phase is bit-identical alone or in any batch.
    The F0 must match the magnitudes it is used with: with a 3 % error per frame the advantage over ``init="spsi"`` is lost after a
    few iterations.  CPU tensors raise."""
    return _gl_for(hp).f0_phase(f0, olens, f0_floor=f0_floor, f0_ceil=f0_ceil, seed=seed, sync=sync)


def excitation(f0, olens=None, hp=None, seed=0, f0_floor=71.0, f0_ceil=800.0):
    """The excitation :func:`f0_phase` transforms -> ``Waveforms``: hop (L - 1) samples of unit power per utterance of L frames (host
    ``olens``), sum_{h = 1..Hn} cos(h phase) sqrt(2 / Hn) with every harmonic below half the sample rate where voiced, uniform noise
    from a counter hash of (seed, sample) where not (include/fs2.h: fs2_op_excitation_geom).  CPU tensors raise."""
    return _gl_for(hp).excitation(f0, olens, seed=seed, f0_floor=f0_floor, f0_ceil=f0_ceil)


def _analysis(wav_packed, sample_lens, hp, want_mag, want_mel, want_energy, gl=None, pitch=None, n_candidates=0):
    """One analysis launch.  ``pitch``: None (fs2_op_stft_geom), or (f0_floor, f0_ceil, voicing_threshold, octave_cost) as
    ``pitch_lags`` accepted them (fs2_op_stft_pitch_geom); then f0 and strength [frames] follow (mag, mel, energy).  With
    ``n_candidates`` = K > 0 (fs2_op_stft_pitch_cands_geom) these two are cand_f0 and cand_strength [frames, K]."""
    _require_cuda(wav_packed, "wav_packed")
    if wav_packed.dim() != 1:
        raise ValueError("wav_packed must be 1-D, got %s" % (tuple(wav_packed.shape),))
    T = _lens(sample_lens, name="sample_lens")
    if int(T.sum()) != wav_packed.numel():
        raise ValueError("sample_lens sum to %d, wav_packed has %d samples" % (int(T.sum()), wav_packed.numel()))
    gl = gl or _gl_for(hp)
    g = gl.geometry
    dev = wav_packed.device
    frames = int((T // g.hop + 1).sum()) if T.numel() else 0
    mag = torch.empty(frames, g.n_bins, dtype=torch.float32, device=dev) if want_mag else None
    mel = torch.empty(frames, g.n_mels, dtype=torch.float32, device=dev) if want_mel else None
    en = torch.empty(frames, dtype=torch.float32, device=dev) if want_energy else None
    per_frame = (frames, n_candidates) if n_candidates else (frames,)
    f0 = torch.empty(per_frame, dtype=torch.float32, device=dev) if pitch is not None else None
    st = torch.empty(per_frame, dtype=torch.float32, device=dev) if pitch is not None else None
    out = (mag, mel, en) if pitch is None else (mag, mel, en, f0, st)
    if frames == 0:
        return out
    x = wav_packed.contiguous().float()
    lib = _lib.lib()
    st_np, st_p = _i32(np.concatenate([[0], np.cumsum(T.numpy())[:-1]]))
    t_np, t_p = _i32(T.numpy())
    B = len(t_np)
    query = lib.fs2_op_stft_workspace_bytes_geom if pitch is None else lib.fs2_op_stft_pitch_workspace_bytes_geom
    ws_bytes = int(query(*g, B, t_p))
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(dev):
        basis = gl.constants(dev)[1]
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        head = (_stream(dev),) + tuple(g) + (x.data_ptr(), B, st_p, t_p, ws.data_ptr(), ws_bytes, ptr(mag),
                                             basis.data_ptr() if want_mel else None, ptr(mel), ptr(en))
        if pitch is None:
            _lib.check(lib.fs2_op_stft_geom(*head))
        elif n_candidates:
            _lib.check(lib.fs2_op_stft_pitch_cands_geom(*head, int(gl.params["sample_rate"]), *pitch, int(n_candidates), ptr(f0), ptr(st)))
        else:
            _lib.check(lib.fs2_op_stft_pitch_geom(*head, int(gl.params["sample_rate"]), *pitch, ptr(f0), ptr(st)))
    return out


def stft_magnitude(wav_packed, sample_lens, mel=False, hp=None):
    """Analysis STFT (the reference's STFT.transform / TacotronSTFT.mel_spectrogram, stft.py:80-110,188-204) of packed waveforms in
    the geometry of ``hp.audio`` (default 1024 / 256 / 1024, 80 mels): waveform b = ``sample_lens[b]`` samples, giving
    ``sample_lens[b] // hop + 1`` frames (reflect padding at its own ends), packed back to back.  Returns |X| [frames, n_fft / 2 + 1],
    or with ``mel=True`` the log-mel [frames, n_mels] = log(clamp(B . |X|, 1e-5)).  A waveform of <= n_fft / 2 samples cannot be
    reflect-padded: its frames are |X| = 0 (log-mel log(1e-5))."""
    mag, lm, _ = _analysis(wav_packed, sample_lens, hp, not mel, mel, False)
    return lm if mel else mag


def mel_energy(wav_packed, sample_lens, hp=None):
    """(log-mel [frames, n_mels], energy [frames]) of packed waveforms from one launch: the reference preprocessing's mel and energy
    targets (nvidia_preprocessing.py: TacotronSTFT.mel_spectrogram and torch.norm(|X|, dim=0)), without pitch.  Frames as in
    ``stft_magnitude``; a waveform of <= n_fft / 2 samples gives energy 0."""
    _, lm, en = _analysis(wav_packed, sample_lens, hp, False, True, True)
    return lm, en


def pitch_lags(sample_rate, win, f0_floor=71.0, f0_ceil=800.0):
    """(tmin, tmax) = (floor(sr / f0_ceil), ceil(sr / f0_floor)): the integer lags the F0 estimator searches.  It divides the frame's
    autocorrelation by the window's, which is too small to divide by beyond half the window: raises ValueError unless
    2 <= tmin and tmax <= win / 2 (csrc/griffin_lim_host.h: gl_pitch_args checks the same)."""
    sr, lo, hi = float(sample_rate), float(f0_floor), float(f0_ceil)
    if not (sr >= 1 and lo > 0 and hi >= lo and math.isfinite(hi)):
        raise ValueError("need sample_rate >= 1 and 0 < f0_floor <= f0_ceil, got %r, %r, %r" % (sample_rate, f0_floor, f0_ceil))
    tmin, tmax = int(math.floor(sr / hi)), int(math.ceil(sr / lo))
    if tmin < 2 or tmax > win // 2:
        raise ValueError("f0_floor %g .. f0_ceil %g at %g Hz need the lags %d .. %d, the window of %d samples allows 2 .. %d: the lowest "
                         "usable f0_floor is 2 sample_rate / win_length = %g Hz, the highest f0_ceil %g Hz"
                         % (lo, hi, sr, tmin, tmax, win, win // 2, 2.0 * sr / win, sr / 2.0))
    return tmin, tmax


def _pitch_setup(hp, f0_floor, f0_ceil, voicing_threshold, octave_cost):
    """(GriffinLim of hp, the four options as floats), checked before anything touches the GPU."""
    gl = _gl_for(hp)
    opt = (float(f0_floor), float(f0_ceil), float(voicing_threshold), float(octave_cost))
    pitch_lags(gl.params["sample_rate"], gl.geometry.win, opt[0], opt[1])
    if not (math.isfinite(opt[2]) and math.isfinite(opt[3])):
        raise ValueError("voicing_threshold and octave_cost must be finite, got %r, %r" % (voicing_threshold, octave_cost))
    return gl, opt


def pitch(wav_packed, sample_lens, hp=None, f0_floor=71.0, f0_ceil=800.0, voicing_threshold=0.45, octave_cost=0.02, return_strength=False):
    """F0 [frames] in Hz of packed waveforms, one value per frame of ``stft_magnitude`` (the same frame count as the mel by
    construction), 0 where unvoiced; with ``return_strength=True`` also the winner's peak height [frames].

    This is an autocorrelation estimator (Boersma 1993 without the path search), NOT the reference's pitch: the reference calls
    pyworld's DIO (dataset/audio_processing.py:54-70).  Per frame, with y the windowed frame: r = irfft(|rfft(y)|^2), rw the same of
    the window, rho[t] = (r[t] / r[0]) / (rw[t] / rw[0]) (r[0] <= 1e-12: unvoiced).  Candidates are the lags t in
    [floor(sr / f0_ceil), ceil(sr / f0_floor)] with rho[t] > rho[t-1], rho[t] >= rho[t+1], rho[t] > 0, refined by a parabola through
    a, c, b = rho[t-1], rho[t], rho[t+1]: d = 0.5 (a - b) / (a - 2c + b), t* = t + d, p = c - 0.25 (a - b) d, scored
    S = p - octave_cost log2(f0_floor t* / sr).  The largest S wins (ties: the smaller t); the frame is voiced iff the winner's
    p >= voicing_threshold; f0 = sr / t*; strength = p (0 without a candidate).  ``sr`` is hp.audio.sample_rate.  No smoothing or
    path search across frames.  (t* may lie up to half a sample outside the integer lags, and f0 that far outside the floor / ceiling.)  The lags must fit half the window (``pitch_lags``): a floor below 2 sr / win_length raises ValueError.
    A waveform of <= n_fft / 2 samples gives 0 on all its frames.  CPU tensors raise."""
    gl, opt = _pitch_setup(hp, f0_floor, f0_ceil, voicing_threshold, octave_cost)
    _, _, _, f0, st = _analysis(wav_packed, sample_lens, hp, False, False, False, gl, opt)
    return (f0, st) if return_strength else f0


MAX_CANDIDATES = _lib.PITCH_MAX_CANDS
# index of a record of the path search (include/fs2.h)
PATH_FRAMES, PATH_FLAGS, PATH_SCORE, PATH_VOICED, PATH_SWITCHES, PATH_MAX_STEP, PATH_CHANGED = range(7)


def _check_n_candidates(n_candidates):
    if not (isinstance(n_candidates, (int, np.integer)) and 1 <= n_candidates <= MAX_CANDIDATES):
        raise ValueError("n_candidates must be an integer in 1 .. %d, got %r" % (MAX_CANDIDATES, n_candidates))
    return int(n_candidates)


def _check_path_options(time_step, f0_floor, voicing_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost):
    """The six numbers of the path search as floats, checked before anything touches the GPU (csrc/pitch_path.h: pp_pitch_path
    checks the same)."""
    ts, lo = float(time_step), float(f0_floor)
    if not (ts > 0 and math.isfinite(ts) and lo > 0 and math.isfinite(lo)):
        raise ValueError("need time_step > 0 and f0_floor > 0, both finite, got %r, %r" % (time_step, f0_floor))
    vt, oc = float(voicing_threshold), float(octave_cost)
    if not (math.isfinite(vt) and math.isfinite(oc)):
        raise ValueError("voicing_threshold and octave_cost must be finite, got %r, %r" % (voicing_threshold, octave_cost))
    oj, vu = float(octave_jump_cost), float(voiced_unvoiced_cost)
    if not (oj >= 0 and math.isfinite(oj) and vu >= 0 and math.isfinite(vu)):
        raise ValueError("octave_jump_cost and voiced_unvoiced_cost must be finite and not negative, got %r, %r"
                         % (octave_jump_cost, voiced_unvoiced_cost))
    return ts, lo, vt, oc, oj, vu


def pitch_candidates(wav_packed, sample_lens, hp=None, n_candidates=8, f0_floor=71.0, f0_ceil=800.0, octave_cost=0.02):
    """(cand_f0 [frames, n_candidates], cand_strength [frames, n_candidates]) of packed waveforms: per frame of ``pitch`` the first
    ``n_candidates`` (1 .. 8) candidates of its definition in the order "larger S, then smaller lag", as f0 = sr / t* and strength = p;
    empty slots are 0 / 0.  Slot 0 is ``pitch``'s winner bit for bit: its strength everywhere and its f0 wherever ``pitch`` calls
    the frame voiced (csrc/gl_pitch.h: gl_candidates).  What ``pitch_path`` takes.  CPU tensors raise."""
    K = _check_n_candidates(n_candidates)
    gl, opt = _pitch_setup(hp, f0_floor, f0_ceil, 0.45, octave_cost)
    _, _, _, cf, cs = _analysis(wav_packed, sample_lens, hp, False, False, False, gl, opt, K)
    return cf, cs


class PitchTrack(DeviceRecords):
    """The result of the path search.  ``f0`` [frames] float32: the chosen candidate's f0, 0 = unvoiced; ``state`` [frames] int32:
    its slot, -1 = unvoiced; ``strength`` [frames] float32: its strength, 0 = unvoiced (device tensors).  ``terms`` [B, 8] /
    ``batch`` [8]: the records (float64 numpy; include/fs2.h lists the indices)."""
    TERMS = _lib.PITCH_PATH_TERMS

    def __init__(self, f0, state, strength, terms, batch, _device=None):
        super().__init__(terms, batch, _device)
        self.f0, self.state, self.strength = f0, state, strength

    def per_utterance(self):
        """Per utterance, as a dict of arrays [B]: ``voiced_share`` = voiced frames / frames (NaN without frames), ``vuv_switches``
        = changes between voiced and unvoiced, ``max_octave_step`` = the largest |log2| step between consecutive voiced frames,
        ``changed_frames`` = the frames whose choice differs from the frame's own best candidate, ``flags`` (0 fine, 2 a candidate
        value was not finite or was negative: the utterance is all unvoiced)."""
        t = self.terms
        i64 = lambda x: x.astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return dict(voiced_share=t[:, PATH_VOICED] / t[:, PATH_FRAMES], vuv_switches=i64(t[:, PATH_SWITCHES]),
                        max_octave_step=t[:, PATH_MAX_STEP].copy(), changed_frames=i64(t[:, PATH_CHANGED]), flags=i64(t[:, PATH_FLAGS]))


def pitch_path(cand_f0, cand_strength, frame_lens, time_step, f0_floor=71.0, voicing_threshold=0.45, octave_cost=0.02,
               octave_jump_cost=0.35, voiced_unvoiced_cost=0.14):
    """The path search over per-frame candidates (Boersma 1993, the step ``pitch`` leaves out) -> :class:`PitchTrack`
    (csrc/pitch_path.h, include/fs2.h: fs2_op_pitch_path).

    ``cand_f0`` / ``cand_strength``: float32 device tensors [frames, K], K = 1 .. 8, the utterances packed back to back
    (``pitch_candidates``' output, or candidates from any other source; a slot with f0 = 0 is empty); ``frame_lens``: host lengths;
    ``time_step``: seconds per frame (hop / sample_rate).  Per utterance the sequence of states (unvoiced, or one of the frame's
    candidates) with the largest sum of local scores -- ``voicing_threshold`` for unvoiced, p - octave_cost log2(f0_floor / f)
    for a candidate -- minus transition costs: ``voiced_unvoiced_cost`` s for a change of voicing and ``octave_jump_cost`` s
    |log2 (f_a / f_b)| between voiced frames, s = 0.01 / time_step.  Everything is formed in double in a fixed order, so an utterance's
    track does not depend on its batch.  With both costs 0 it is the per-frame best.  CPU tensors raise."""
    opt = _check_path_options(time_step, f0_floor, voicing_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost)
    _require_cuda(cand_f0, "cand_f0")
    _require_cuda(cand_strength, "cand_strength")
    if cand_f0.dim() != 2 or cand_f0.shape != cand_strength.shape or cand_f0.device != cand_strength.device:
        raise ValueError("cand_f0 and cand_strength must be [frames, K] tensors of one shape on one device, got %s and %s"
                         % (tuple(cand_f0.shape), tuple(cand_strength.shape)))
    K = cand_f0.shape[1]
    if not 1 <= K <= MAX_CANDIDATES:
        raise ValueError("the candidates per frame must be 1 .. %d, got %d" % (MAX_CANDIDATES, K))
    L = _lens(frame_lens, name="frame_lens")
    rows = int(cand_f0.shape[0])
    if int(L.sum()) != rows:
        raise ValueError("frame_lens sum to %d, the candidates have %d frames" % (int(L.sum()), rows))
    dev = cand_f0.device
    B = int(L.numel())
    cf, cs = cand_f0.contiguous().float(), cand_strength.contiguous().float()
    lib = _lib.lib()
    st_keep, st_p = _i32(np.concatenate([[0], np.cumsum(L.numpy())[:-1]]) if B else np.zeros(0))
    ln_keep, ln_p = _i32(L.numpy())
    ptr = lambda t: t.data_ptr() if t.numel() else None
    with torch.cuda.device(dev):
        f0 = torch.empty(rows, dtype=torch.float32, device=dev)
        state = torch.empty(rows, dtype=torch.int32, device=dev)
        strength = torch.empty(rows, dtype=torch.float32, device=dev)
        rec, terms_p, batch_p = PitchTrack._on_device(B, dev)
        ws_bytes = int(lib.fs2_op_pitch_path_workspace_bytes(B, ln_p if B else None))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        args = _lib.OpPitchPathArgs(B, K, *opt, ptr(cf), ptr(cs), st_p if B else None, ln_p if B else None, ws.data_ptr(), ws_bytes,
                                    ptr(f0), ptr(state), ptr(strength), terms_p, batch_p)
        _lib.check(lib.fs2_op_pitch_path(_stream(dev), C.byref(args)))
    return PitchTrack(f0, state, strength, None, None, _device=rec)


def pitch_track(wav_packed, sample_lens, hp=None, n_candidates=8, f0_floor=71.0, f0_ceil=800.0, voicing_threshold=0.45, octave_cost=0.02,
                octave_jump_cost=0.35, voiced_unvoiced_cost=0.14):
    """``pitch_candidates`` then ``pitch_path`` -> :class:`PitchTrack`: the F0 of packed waveforms with the path search, one value
    per frame of ``stft_magnitude``, 0 where unvoiced.  ``time_step`` is hop / sample_rate of ``hp.audio``."""
    K = _check_n_candidates(n_candidates)
    gl, opt = _pitch_setup(hp, f0_floor, f0_ceil, voicing_threshold, octave_cost)
    time_step = gl.geometry.hop / float(gl.params["sample_rate"])
    _check_path_options(time_step, f0_floor, voicing_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost)
    return _track(wav_packed, sample_lens, hp, gl, opt, K, octave_jump_cost, voiced_unvoiced_cost, False)[1]


def _track(wav_packed, sample_lens, hp, gl, opt, K, octave_jump_cost, voiced_unvoiced_cost, features):
    """((log-mel, energy) or (None, None), PitchTrack): one candidates call, with the log-mel and the energy when ``features``
    (gl_stft's launch beside gl_candidates'), and the path over it."""
    _, lm, en, cf, cs = _analysis(wav_packed, sample_lens, hp, False, features, features, gl, opt, K)
    frame_lens = _lens(sample_lens, name="sample_lens") // gl.geometry.hop + 1
    time_step = gl.geometry.hop / float(gl.params["sample_rate"])
    return (lm, en), pitch_path(cf, cs, frame_lens, time_step, opt[0], opt[2], opt[3], octave_jump_cost, voiced_unvoiced_cost)


F0_METHODS = ("frame", "path")


def wav_features(wav_packed, sample_lens, hp=None, f0_method="frame", **pitch_options):
    """(log-mel [frames, n_mels], energy [frames], f0 [frames]) of packed waveforms: the three arrays the reference's preprocessing
    saves per utterance (nvidia_preprocessing.py).  ``f0_method="frame"``: the F0 of :func:`pitch` (an autocorrelation estimator,
    not the reference's DIO) with its options (f0_floor, f0_ceil, voicing_threshold, octave_cost), all from one launch.
    ``f0_method="path"``: the F0 of :func:`pitch_track` -- the same candidates joined by a path search across frames -- which also
    takes octave_jump_cost, voiced_unvoiced_cost and n_candidates; ``mel_energy``'s launch, one for the candidates and one for the
    path.  The log-mel and the energy are ``mel_energy``'s bit for bit in both."""
    if "return_strength" in pitch_options:
        raise TypeError("wav_features returns (logmel, energy, f0); use pitch(..., return_strength=True) for the strength")
    if f0_method not in F0_METHODS:
        raise ValueError("f0_method must be one of %s, got %r" % (F0_METHODS, f0_method))
    o = dict(f0_floor=71.0, f0_ceil=800.0, voicing_threshold=0.45, octave_cost=0.02)
    if f0_method == "path":
        o.update(octave_jump_cost=0.35, voiced_unvoiced_cost=0.14, n_candidates=8)
    unknown = sorted(set(pitch_options) - set(o))
    if unknown:
        raise TypeError("unknown pitch option(s) %s" % ", ".join(unknown))
    o.update(pitch_options)
    gl, opt = _pitch_setup(hp, o["f0_floor"], o["f0_ceil"], o["voicing_threshold"], o["octave_cost"])
    if f0_method == "path":
        K = _check_n_candidates(o["n_candidates"])
        _check_path_options(gl.geometry.hop / float(gl.params["sample_rate"]), *opt[:1], *opt[2:], o["octave_jump_cost"], o["voiced_unvoiced_cost"])
        (lm, en), track = _track(wav_packed, sample_lens, hp, gl, opt, K, o["octave_jump_cost"], o["voiced_unvoiced_cost"], True)
        return lm, en, track.f0
    _, lm, en, f0, _ = _analysis(wav_packed, sample_lens, hp, False, True, True, gl, opt)
    return lm, en, f0


def save_wav(path, wav, sample_rate=22050):
    """Write a mono 16-bit PCM wav with the standard library: samples clipped to [-1, 1] and scaled by 32767.  (The reference writes
    ``wav.astype("int16")`` of the float waveform, inference.py:201, which truncates [-1, 1] to near-silence; this scales first.)"""
    x = wav.detach().float().cpu().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav, np.float32)
    pcm = np.round(np.clip(x.reshape(-1), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())
    return pcm.size
