"""Griffin-Lim at c3 on one MI355X: the HIP vocoder (fs2_op_griffin_lim) against the same 30-iteration loop written with
torch.stft / torch.istft (rocFFT) on the same GPU.  Prints one JSON line.

Mels: the default model's free-running output on the c3 batch (64 LJSpeech-shaped utterances; what bench.py times), packed as
inference_batch(packed=True) returns it.  Times are host clocks around device-synchronised loops after a warm-up, over >= --min-s
seconds of work.  Bytes and FLOP per iteration come from shapes (csrc/griffin_lim.h header); kernel times: run this under
rocprofv3 --kernel-trace --stats separately.

Usage:  python tools/vocoder_bench.py [--n-iter 30] [--min-s 0.5] [--workload c3]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_TFLOPS = 157.3          # MI355X dense fp32 vector peak (MI355X_MICROARCH chip table)
PEAK_HBM_TBS = 8.0                # HBM3E peak


def c3_mels(workload):
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, ljspeech_durations, make_batch
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(ljspeech_durations(portable_state_dict(model.state_dict(), seed=0)))
    model = model.cuda()
    b = make_batch(workload)
    with torch.no_grad():
        mels, olens = model.inference_batch(b["xs"].cuda(), b["ilens"], packed=True)
    torch.cuda.synchronize()
    return hp, mels, [int(x) for x in olens]


def timed(fn, min_s):
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if el >= min_s and n >= 3:
            return el / n * 1e3, n


class TorchGL:
    """The reference's griffin_lim with torch.stft / torch.istft (center=True, reflect padding, periodic Hann, wss normalisation:
    the same transform), batched over padded utterances, lengths honoured by istft(length=)."""

    def __init__(self, device):
        self.win = torch.hann_window(1024, periodic=True, device=device)

    def __call__(self, M, lens, n_iter, angles):
        # M [B, 513, Lmax] (zero past each utterance's frames), angles same shape
        C = M * torch.exp(1j * angles)
        length = 256 * (M.shape[-1] - 1)
        sig = torch.istft(C, 1024, 256, 1024, self.win, center=True, length=length)
        for _ in range(n_iter):
            X = torch.stft(sig, 1024, 256, 1024, self.win, center=True, pad_mode="reflect", return_complex=True)
            C = M * torch.exp(1j * torch.angle(X))
            sig = torch.istft(C, 1024, 256, 1024, self.win, center=True, length=length)
        return sig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-iter", type=int, default=30)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vocoder_bench needs a GPU"
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude
    hp, mels, olens = c3_mels(args.workload)
    N, B = mels.shape[0], len(olens)
    gl = GriffinLim(hp)
    run = lambda n: gl(mels, olens, n_iter=n, seed=0)
    ms_call, reps = timed(lambda: run(args.n_iter), args.min_s)
    ms_zero, _ = timed(lambda: run(0), args.min_s)
    ms_iter = (ms_call - ms_zero) / max(args.n_iter, 1)
    out = run(args.n_iter)
    samples = int(out.wav.numel())
    audio_s = samples / float(hp.audio.sample_rate)
    # spectral convergence of the HIP output against its target magnitudes, per utterance, summed in quadrature
    pinv, basis = gl.constants(mels.device)
    Mt = torch.clamp(torch.exp(mels) @ pinv.T, min=0)                                       # [N, 513]
    Xh = stft_magnitude(out.wav, out.sample_lens)
    num = float(torch.linalg.norm(Mt - Xh)) if Xh.shape == Mt.shape else float("nan")
    sc_hip = num / float(torch.linalg.norm(Mt))
    # traffic / FLOP per iteration from shapes: C of (F + 6) / F frames in, M in, C out (+ halo), 2.4 real 1024-FFTs per frame
    F = 32
    tiles = sum(math.ceil(L / F) for L in olens if L >= 4)
    halo_frames = sum(min(L, F) + 6 for L in olens if L >= 4 for _ in range(math.ceil(L / F)))
    bytes_iter = halo_frames * 513 * 8 + N * 513 * 4 + N * 513 * 8
    fft_flop = 2.5 * 1024 * 10                                                              # one 1024-point real FFT
    flop_iter = (halo_frames + N) * fft_flop + N * 513 * 12
    t_bytes = bytes_iter / (PEAK_HBM_TBS * 1e12) * 1e3
    t_flop = flop_iter / (PEAK_FP32_TFLOPS * 1e12) * 1e3
    rec = dict(workload=args.workload, utterances=B, frames=N, tiles=tiles, n_iter=args.n_iter, samples=samples,
               audio_seconds=round(audio_s, 3), hip_ms_per_call=round(ms_call, 3), hip_ms_call_n_iter0=round(ms_zero, 3),
               hip_ms_per_iter=round(ms_iter, 4), hip_reps=reps, real_time_factor=round(audio_s / (ms_call / 1e3), 1),
               bytes_per_iter=bytes_iter, flop_per_iter=flop_iter,
               bound_ms_bytes=round(t_bytes, 4), bound_ms_flop=round(t_flop, 4),
               share_of_larger_bound=round(max(t_bytes, t_flop) / ms_iter, 3) if ms_iter > 0 else None,
               larger_bound="bytes" if t_bytes >= t_flop else "flop", sc_hip=round(sc_hip, 5))
    if not args.no_torch:
        Lmax = max(olens)
        Mp = torch.zeros(B, 513, Lmax, device=mels.device)
        o = 0
        for b, L in enumerate(olens):
            Mp[b, :, :L] = Mt[o:o + L].T
            o += L
        ang = (torch.rand(B, 513, Lmax, device=mels.device, generator=torch.Generator(device=mels.device).manual_seed(0)) * 2 - 1) * math.pi
        tg = TorchGL(mels.device)
        ms_torch, treps = timed(lambda: tg(Mp, olens, args.n_iter, ang), args.min_s)
        sig = tg(Mp, olens, args.n_iter, ang)
        parts = [sig[b, :256 * (L - 1)] for b, L in enumerate(olens)]
        Xt = stft_magnitude(torch.cat(parts).contiguous(), [256 * (L - 1) for L in olens])
        sc_torch = float(torch.linalg.norm(Mt - Xt)) / float(torch.linalg.norm(Mt)) if Xt.shape == Mt.shape else float("nan")
        rec.update(torch_ms_per_call=round(ms_torch, 3), torch_reps=treps, speedup_vs_torch=round(ms_torch / ms_call, 2),
                   sc_torch=round(sc_torch, 5))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
