"""Griffin-Lim vocoder: packed mel frames -> waveforms on the MI355X (csrc/griffin_lim.h, include/fs2.h: fs2_op_griffin_lim).

The reference's only self-contained way from a mel to a wav is Griffin-Lim (reference inference.py:195-199,
dataset/audio_processing.py:224-240, utils/stft.py:41-151), with the transform of configs/default.yaml: n_fft = win_length = 1024,
hop 256, periodic Hann window.  As written it feeds the 80-bin mel where the 513-bin magnitude belongs; here the mel is first mapped
back to magnitudes with the pseudo-inverse of the mel filterbank it was made with (``M = max(pinv(B) . exp(mel), 0)``: the inverse of
TacotronSTFT's log(clamp(B . |S|, 1e-5)), stft.py:188-204).  The whole batch is vocoded in one call, every utterance with its own
STFT (reflect padding at its own ends), nothing goes through the host, and an utterance's waveform is bit-identical whether it is
vocoded alone or inside any batch.

``stft_magnitude`` is the analysis direction (TacotronSTFT.mel_spectrogram): waveforms -> |STFT| or log-mel on the GPU.
There is no CPU fallback: CPU tensors raise.
"""
import ctypes as C
import math
import wave
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

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


def _audio_params(hp):
    """mel_basis arguments from hp.audio where the keys exist; the transform itself must be the kernels' 1024 / 256 / 1024."""
    p = dict(_AUDIO_DEFAULTS)
    a = getattr(hp, "audio", None) if hp is not None else None
    if a is not None:
        get = a.get if hasattr(a, "get") else (lambda k, d=None: getattr(a, k, d))
        for k, hk in (("sample_rate", "sample_rate"), ("n_fft", "n_fft"), ("n_mels", "n_mels"), ("fmin", "fmin"), ("fmax", "fmax")):
            if get(hk, None) is not None:
                p[k] = type(_AUDIO_DEFAULTS[k])(get(hk))
        for k, want in (("n_fft", N_FFT), ("hop_length", HOP), ("win_length", WIN)):
            if get(k, None) is not None and int(get(k)) != want:
                raise ValueError("the Griffin-Lim kernels implement n_fft = win_length = 1024, hop 256 only; hp.audio.%s = %s" % (k, get(k)))
    if p["n_fft"] != N_FFT:
        raise ValueError("n_fft must be 1024, got %r" % p["n_fft"])
    if p["n_mels"] != 80:
        raise ValueError("the Griffin-Lim kernels take 80 mel bins, got %r" % p["n_mels"])
    return p


# ---- seeded initial phase: the formula of csrc/griffin_lim.h (gl_seed_angle), restated ----
def _mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def seed_angles(seed, n_frames):
    """Initial angles [n_frames, 513] (float32) of an utterance for ``seed``: uniform on [-pi, pi) from a counter-based hash of
    (seed, utterance-local frame, bin), exactly as the kernel computes them."""
    with np.errstate(over="ignore"):
        f = np.arange(n_frames, dtype=np.uint32)[:, None]
        k = np.arange(N_BINS, dtype=np.uint32)[None, :]
        s = _mix32(np.uint32((int(seed) + 0x9E3779B9) & 0xFFFFFFFF))
        h = _mix32((k + np.uint32(513) * f) ^ s)
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


def _require_cuda(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not x.is_cuda:
        raise RuntimeError("fastspeech2_amd runs on an MI355X only (no CPU fallback): %s is on %s" % (name, x.device))


def _lens(olens, B=None, name="olens"):
    L = torch.as_tensor(olens).detach().to("cpu", torch.int64).reshape(-1)
    if B is not None and L.numel() != B:
        raise ValueError("%s has %d entries for %d utterances" % (name, L.numel(), B))
    if (L < 0).any():
        raise ValueError("%s must be >= 0" % name)
    return L


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


class GriffinLim:
    """Griffin-Lim on the GPU, batched.  ``GriffinLim(hp)(mels, olens)`` -> ``Waveforms(wav_packed, sample_lens)``.

    An utterance of L frames gives 256 (L - 1) samples (the reference's STFT.inverse trims n_fft / 2 at both ends); L < 4 is too
    short for the reference's reflect padding and gives 256 (L - 1) zeros (none for L <= 1), without failing the batch."""

    def __init__(self, hp=None, device=None):
        self.params = _audio_params(hp)
        self.device = torch.device(device) if device is not None else None
        B = mel_basis(**self.params)
        self._basis_np = B
        self._pinv_np = np.linalg.pinv(B)          # [513, 80], float64 on the host
        self._dev = {}

    def constants(self, device):
        """(pinv [513, 80], mel basis [80, 513]) as fp32 tensors on ``device``."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = (torch.tensor(self._pinv_np, dtype=torch.float32, device=device).contiguous(),
                                 torch.tensor(self._basis_np, dtype=torch.float32, device=device).contiguous())
        return self._dev[device]

    def __call__(self, mels, olens=None, n_iter=30, momentum=0.0, seed=0, init_phase=None, magnitudes=False):
        """mels: packed [N, 80] (``inference_batch(packed=True)``) with ``olens`` [B] summing to N, or padded [B, Lmax, 80] with
        ``olens`` [B] <= Lmax (None: every utterance Lmax frames; packed: one utterance).  ``magnitudes=True``: linear magnitudes
        [.., 513] instead (the reference's ``griffin_lim(magnitudes, ...)`` contract).  ``init_phase``: angles in the layout of
        ``mels`` with 513 bins, or None: seeded.  ``momentum`` > 0: fast Griffin-Lim (0 = the reference).  Runs on the current
        stream of the input's device without synchronising."""
        _require_cuda(mels, "mels")
        W = N_BINS if magnitudes else 80
        if mels.dim() not in (2, 3) or mels.shape[-1] != W:
            raise ValueError("mels must be [N, %d] (packed) or [B, Lmax, %d] (padded), got %s" % (W, W, tuple(mels.shape)))
        if self.device is not None and mels.device != self.device:
            raise ValueError("mels on %s, this GriffinLim on %s" % (mels.device, self.device))
        n_iter, momentum = int(n_iter), float(momentum)
        if n_iter < 0:
            raise ValueError("n_iter must be >= 0")
        if not (momentum >= 0.0 and math.isfinite(momentum)):
            raise ValueError("momentum must be finite and >= 0")
        if mels.dim() == 2:
            N = mels.shape[0]
            L = _lens([N] if olens is None else olens)
            if int(L.sum()) != N:
                raise ValueError("packed mels: olens sum to %d, mels have %d rows" % (int(L.sum()), N))
            starts = np.concatenate([[0], np.cumsum(L.numpy())[:-1]]).astype(np.int64)
            src = mels
        else:
            Bp, Lmax = mels.shape[0], mels.shape[1]
            L = _lens([Lmax] * Bp if olens is None else olens, Bp)
            if Bp and int(L.max()) > Lmax:
                raise ValueError("padded mels: an olens entry exceeds Lmax = %d" % Lmax)
            starts = np.arange(Bp, dtype=np.int64) * Lmax
            src = mels.reshape(Bp * Lmax, W)
        if init_phase is not None:
            _require_cuda(init_phase, "init_phase")
            if tuple(init_phase.shape[:-1]) != tuple(mels.shape[:-1]) or init_phase.shape[-1] != N_BINS:
                raise ValueError("init_phase must have the layout of mels with 513 bins, got %s" % (tuple(init_phase.shape),))
            init_phase = init_phase.reshape(-1, N_BINS).contiguous().float()
        src = src.contiguous().float()
        dev = mels.device
        sample_lens = HOP * torch.clamp(L - 1, min=0)
        wav = torch.empty(int(sample_lens.sum()), dtype=torch.float32, device=dev)
        if wav.numel() == 0:
            return Waveforms(wav, sample_lens)
        if int(L.sum()) * N_BINS >= 2 ** 31 or wav.numel() >= 2 ** 31:
            raise ValueError("batch too large for one call (%d frames)" % int(L.sum()))
        lib = _lib.lib()
        s_np, s_p = _i32(starts)
        l_np, l_p = _i32(L.numpy())
        B = len(l_np)
        ws_bytes = int(lib.fs2_op_vocode_workspace_bytes(B, l_p))
        with torch.cuda.device(dev):
            pinv = self.constants(dev)[0] if not magnitudes else None
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.fs2_op_griffin_lim(_stream(dev), src.data_ptr(), W, pinv.data_ptr() if pinv is not None else None, B, s_p, l_p,
                                              n_iter, momentum, int(seed) & 0xFFFFFFFF,
                                              init_phase.data_ptr() if init_phase is not None else None, ws.data_ptr(), ws_bytes,
                                              wav.data_ptr()))
        return Waveforms(wav, sample_lens)


_DEFAULT_GL = None


def stft_magnitude(wav_packed, sample_lens, mel=False, hp=None):
    """Analysis STFT (the reference's STFT.transform / TacotronSTFT.mel_spectrogram, stft.py:80-110,188-204) of packed waveforms:
    waveform b = ``sample_lens[b]`` samples, giving ``sample_lens[b] // 256 + 1`` frames (reflect padding at its own ends), packed back
    to back.  Returns |X| [frames, 513], or with ``mel=True`` the log-mel [frames, 80] = log(clamp(B . |X|, 1e-5)).  A waveform of
    <= 512 samples cannot be reflect-padded: its frames are |X| = 0 (log-mel log(1e-5))."""
    global _DEFAULT_GL
    _require_cuda(wav_packed, "wav_packed")
    if wav_packed.dim() != 1:
        raise ValueError("wav_packed must be 1-D, got %s" % (tuple(wav_packed.shape),))
    T = _lens(sample_lens, name="sample_lens")
    if int(T.sum()) != wav_packed.numel():
        raise ValueError("sample_lens sum to %d, wav_packed has %d samples" % (int(T.sum()), wav_packed.numel()))
    gl = GriffinLim(hp) if hp is not None else (_DEFAULT_GL or GriffinLim())
    if hp is None:
        _DEFAULT_GL = gl
    dev = wav_packed.device
    frames = int((T // HOP + 1).sum()) if T.numel() else 0
    out = torch.empty(frames, 80 if mel else N_BINS, dtype=torch.float32, device=dev)
    if frames == 0:
        return out
    x = wav_packed.contiguous().float()
    lib = _lib.lib()
    st_np, st_p = _i32(np.concatenate([[0], np.cumsum(T.numpy())[:-1]]))
    t_np, t_p = _i32(T.numpy())
    B = len(t_np)
    ws_bytes = int(lib.fs2_op_stft_workspace_bytes(B, t_p))
    with torch.cuda.device(dev):
        basis = gl.constants(dev)[1]
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.fs2_op_stft(_stream(dev), x.data_ptr(), B, st_p, t_p, ws.data_ptr(), ws_bytes, None if mel else out.data_ptr(),
                                   basis.data_ptr() if mel else None, out.data_ptr() if mel else None))
    return out


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
