"""Griffin-Lim at c3 on one MI355X: the HIP vocoder (fs2_op_griffin_lim) against the same 30-iteration loop written with
torch.stft / torch.istft (rocFFT) on the same GPU.  Prints one JSON line.

Mels: the default model's free-running output on the c3 batch (64 LJSpeech-shaped utterances; what bench.py times), packed as
inference_batch(packed=True) returns it.  Times are host clocks around device-synchronised loops after a warm-up, over >= --min-s
seconds of work.  Bytes and FLOP per iteration come from shapes (csrc/griffin_lim.h header); kernel times: run this under
rocprofv3 --kernel-trace --stats separately.

Usage:  python tools/vocoder_bench.py [--n-iter 30] [--min-s 0.5] [--workload c3]

--geometry N,H,W [--sample-rate SR] [--repeats K]: another transform (n_fft, hop, win_length).  The workload is then the c3
utterances' audio durations (olens x 256 / 22050 s) at SR, as synthetic harmonic waveforms whose magnitudes come from
stft_magnitude at that geometry; 30 iterations of the HIP path and of TorchGL at the same geometry are each timed K times
(median and max - min spread reported).  With neither flag the run is the default one above.

--pipeline [--steps K] [--repeats R] [--precision P] [--pipeline-workloads c3,c1]: text -> waveform end to end at c3 and at c1 (one utterance), per step, in three
forms timed alternately (R rounds of K steps each per form; median and max - min spread over the rounds):
  (a) sync      synchronous inference_batch(packed=True), then the host-driven GriffinLim(mels, olens)
  (b) async     both halves sync=False (AsyncMels -> AsyncWaveforms), three steps in flight on StepStreams(3)
  (c) graph     c1 only: capture_graph(vocoder=gl), one graph launch per step
Every region is K steps between two device synchronisations; (b) and (c) are checked for flags afterwards.

--init seeded|spsi: the initial phase of every Griffin-Lim call of the runs above (default seeded; --n-iter as before).

--constraint magnitude|mel: the projection of every Griffin-Lim iteration of the default run and of --pipeline (default magnitude;
DESIGN.md section 14.10).  The default run also reports logmel_err = mean |log-mel(wav) - mels| over the batch (stft_magnitude on the GPU).

--compare-constraint [--repeats R]: the vocoder call in both constraints on the same mels, at --n-iter and at 0 iterations, all four timed
alternately over R rounds (median and max - min spread); per-iteration times, their ratio mel / magnitude, and logmel_err of both.

--compare-init [--n-iter 10] [--repeats R] [--steps K] [--pipeline-workloads c3,c1]: the SPSI initial phase against the seeded one, per
workload, every pair timed alternately over R rounds (median and max - min spread): (i) spsi_phase alone, (ii) the vocoder call
(seeded, 30) against (spsi, --n-iter), (iii) the text -> wav step, synchronous and sync-free on three streams, for the same two
settings, (iv) the spectral convergence of both settings on the same mels (stft_magnitude on the GPU).  The mels are those of a
randomly initialised model: they are not speech.
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
    """The reference's griffin_lim with torch.stft / torch.istft (center=True, reflect padding, periodic Hann of win_length padded
    to n_fft at the centre, wss normalisation: the same transform), batched over padded utterances, lengths honoured by
    istft(length=)."""

    def __init__(self, device, n_fft=1024, hop=256, win=1024):
        self.n_fft, self.hop, self.wl = n_fft, hop, win
        self.win = torch.hann_window(win, periodic=True, device=device)

    def __call__(self, M, lens, n_iter, angles):
        # M [B, bins, Lmax] (zero past each utterance's frames), angles same shape
        n, h, w = self.n_fft, self.hop, self.wl
        C = M * torch.exp(1j * angles)
        length = h * (M.shape[-1] - 1)
        sig = torch.istft(C, n, h, w, self.win, center=True, length=length)
        for _ in range(n_iter):
            X = torch.stft(sig, n, h, w, self.win, center=True, pad_mode="reflect", return_complex=True)
            C = M * torch.exp(1j * torch.angle(X))
            sig = torch.istft(C, n, h, w, self.win, center=True, length=length)
        return sig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-iter", type=int, default=30)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--geometry", default=None, help="n_fft,hop,win_length (default: the 1024,256,1024 run)")
    ap.add_argument("--sample-rate", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5, help="timings per path in the --geometry run")
    ap.add_argument("--pipeline", action="store_true", help="time text -> wav end to end (see the module docstring)")
    ap.add_argument("--pipeline-workloads", default="c3,c1", help="workloads of the --pipeline run (the graph form runs at c1 only)")
    ap.add_argument("--steps", type=int, default=20, help="steps per timed region of the --pipeline run")
    ap.add_argument("--precision", default="mix_mx4", help="the model's arithmetic mode in the --pipeline run (bench.py's default)")
    ap.add_argument("--init", default="seeded", choices=("seeded", "spsi"), help="initial phase of the Griffin-Lim calls")
    ap.add_argument("--constraint", default="magnitude", choices=("magnitude", "mel"), help="projection of a Griffin-Lim iteration")
    ap.add_argument("--compare-init", action="store_true", help="(seeded, 30) against (spsi, --n-iter) (see the module docstring)")
    ap.add_argument("--compare-constraint", action="store_true", help="both constraints alternately (see the module docstring)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vocoder_bench needs a GPU"
    if args.constraint != "magnitude" and (args.compare_init or args.geometry is not None or args.sample_rate is not None):
        ap.error("--constraint belongs to the default run and to --pipeline (the --geometry run vocodes magnitudes)")
    if args.compare_init:
        return compare_init_main(args)
    if args.compare_constraint:
        return compare_constraint_main(args)
    if args.pipeline:
        return pipeline_main(args)
    if args.geometry is not None or args.sample_rate is not None:
        return geometry_main(args)
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude
    hp, mels, olens = c3_mels(args.workload)
    N, B = mels.shape[0], len(olens)
    gl = GriffinLim(hp)
    run = lambda n: gl(mels, olens, n_iter=n, seed=0, init=args.init, constraint=args.constraint)
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
    lm = stft_magnitude(out.wav, out.sample_lens, mel=True, hp=hp)
    logmel_err = float((lm - mels).abs().mean()) if lm.shape == mels.shape else float("nan")
    # traffic / FLOP per iteration from shapes: C of (F + 6) / F frames in, M in, C out (+ halo), 2.4 real 1024-FFTs per frame
    F = 32
    tiles = sum(math.ceil(L / F) for L in olens if L >= 4)
    halo_frames = sum(min(L, F) + 6 for L in olens if L >= 4 for _ in range(math.ceil(L / F)))
    bytes_iter = halo_frames * 513 * 8 + N * 513 * 4 + N * 513 * 8
    fft_flop = 2.5 * 1024 * 10                                                              # one 1024-point real FFT
    flop_iter = (halo_frames + N) * fft_flop + N * 513 * 12
    t_bytes = bytes_iter / (PEAK_HBM_TBS * 1e12) * 1e3
    t_flop = flop_iter / (PEAK_FP32_TFLOPS * 1e12) * 1e3
    rec = dict(workload=args.workload, utterances=B, frames=N, tiles=tiles, n_iter=args.n_iter, init=args.init, constraint=args.constraint,
               samples=samples, logmel_err=round(logmel_err, 5),
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


def pipeline_main(args):
    from fastspeech2_amd import FeedForwardTransformer, StepStreams, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, ljspeech_durations, make_batch
    from fastspeech2_amd.vocoder import GriffinLim
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(ljspeech_durations(portable_state_dict(model.state_dict(), seed=0)))
    model = model.cuda()
    model.precision = args.precision
    gl = GriffinLim(hp)
    K, n_iter, init, con = args.steps, args.n_iter, args.init, args.constraint
    rec = dict(mode="pipeline", precision=args.precision, n_iter=n_iter, init=init, constraint=con, steps_per_region=K, rounds=args.repeats, workloads={})

    def region(step, finish=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            step()
        if finish is not None:
            finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / K * 1e3

    with torch.no_grad():
        for workload in args.pipeline_workloads.split(","):
            b = make_batch(workload)
            xs, il = b["xs"].cuda(), b["ilens"]
            mels, olens = model.inference_batch(xs, il, packed=True)          # (first call: synchronous, learns the capacities)
            ref = gl(mels, olens, n_iter=n_iter, init=init, constraint=con)

            def step_sync():
                m, ol = model.inference_batch(xs, il, packed=True)
                return gl(m, ol, n_iter=n_iter, init=init, constraint=con)

            rot = StepStreams(3)
            keep = []

            def step_async():
                with rot.next():
                    am = model.inference_batch(xs, il, packed=True, sync=False)
                    keep.append((am, gl(am, n_iter=n_iter, sync=False, init=init, constraint=con)))
                del keep[:-3]                                                   # (three steps in flight own their buffers)

            forms = {"sync": (step_sync, None), "async": (step_async, rot.join)}
            if workload == "c1":
                run = model.capture_graph(xs, il, vocoder=gl, n_iter=n_iter, init=init, constraint=con)
                forms["graph"] = (lambda: run(xs), None)
            for step, finish in forms.values():                                # warm-up of every form
                region(step, finish)
            ms = {k: [] for k in forms}
            for _ in range(args.repeats):                                       # alternating: one region of each form per round
                for k, (step, finish) in forms.items():
                    ms[k].append(region(step, finish))
            # validity, and that the three forms computed the same waveform
            am, w = keep[-1]
            ok = bool(model.async_ok() and am.ok() and w.ok())
            n = int(ref.wav.numel())
            same = bool(torch.equal(w[0][:n], ref.wav))
            out = dict(utterances=int(il.numel()), frames=int(sum(int(x) for x in olens)), samples=n, async_ok=ok, async_equals_sync=same)
            if "graph" in forms:
                wav, sl, status = run(xs)
                out["graph_flags"] = int(status.cpu()[2])
                out["graph_equals_sync"] = bool(torch.equal(torch.cat([wav[i, :int(k)] for i, k in enumerate(sl.cpu())]), ref.wav))
            for k, v in ms.items():
                out[k + "_ms_per_step"] = round(float(np.median(v)), 4)
                out[k + "_ms_spread"] = round(max(v) - min(v), 4)
                out[k + "_ms_runs"] = [round(x, 4) for x in v]
            out["async_over_sync"] = round(out["async_ms_per_step"] / out["sync_ms_per_step"], 4)
            if "graph" in forms:
                out["graph_over_sync"] = round(out["graph_ms_per_step"] / out["sync_ms_per_step"], 4)
            rec["workloads"][workload] = out
    print(json.dumps(rec))


def compare_constraint_main(args):
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude
    hp, mels, olens = c3_mels(args.workload)
    gl = GriffinLim(hp)
    rec = dict(mode="compare_constraint", workload=args.workload, utterances=len(olens), frames=int(mels.shape[0]), n_iter=args.n_iter, init=args.init,
               rounds=args.repeats, min_s=args.min_s, note="mels of a randomly initialised model: not speech")
    stat = lambda v: dict(median=round(float(np.median(v)), 4), spread=round(max(v) - min(v), 4), runs=[round(x, 4) for x in v])
    ms = {(c, n): [] for c in ("magnitude", "mel") for n in (args.n_iter, 0)}
    for _ in range(args.repeats):                                                # alternating: every setting once per round
        for (c, n), v in ms.items():
            v.append(timed(lambda: gl(mels, olens, n_iter=n, seed=0, init=args.init, constraint=c), args.min_s)[0])
    per_iter = {}
    for c in ("magnitude", "mel"):
        rec[c + "_ms_per_call"], rec[c + "_ms_call_n_iter0"] = stat(ms[(c, args.n_iter)]), stat(ms[(c, 0)])
        per_iter[c] = (rec[c + "_ms_per_call"]["median"] - rec[c + "_ms_call_n_iter0"]["median"]) / max(args.n_iter, 1)
        rec[c + "_ms_per_iter"] = round(per_iter[c], 4)
        w = gl(mels, olens, n_iter=args.n_iter, seed=0, init=args.init, constraint=c)
        lm = stft_magnitude(w.wav, w.sample_lens, mel=True, hp=hp)
        rec[c + "_logmel_err"] = round(float((lm - mels).abs().mean()), 5) if lm.shape == mels.shape else None
    rec["mel_over_magnitude_per_iter"] = round(per_iter["mel"] / per_iter["magnitude"], 4)
    print(json.dumps(rec))


def compare_init_main(args):
    from fastspeech2_amd import FeedForwardTransformer, StepStreams, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, ljspeech_durations, make_batch
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(ljspeech_durations(portable_state_dict(model.state_dict(), seed=0)))
    model = model.cuda()
    model.precision = args.precision
    gl = GriffinLim(hp)
    K, R = args.steps, args.repeats
    settings = {"seeded30": dict(n_iter=30, init="seeded"), "spsi%d" % args.n_iter: dict(n_iter=args.n_iter, init="spsi")}
    a, b = list(settings)
    rec = dict(mode="compare_init", precision=args.precision, settings=settings, steps_per_region=K, rounds=R, min_s=args.min_s,
               note="mels of a randomly initialised model: not speech", workloads={})
    stat = lambda v: dict(median=round(float(np.median(v)), 4), spread=round(max(v) - min(v), 4), runs=[round(x, 4) for x in v])

    def region(step, finish=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            step()
        if finish is not None:
            finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / K * 1e3

    with torch.no_grad():
        for workload in args.pipeline_workloads.split(","):
            bt = make_batch(workload)
            xs, il = bt["xs"].cuda(), bt["ilens"]
            mels, olens = model.inference_batch(xs, il, packed=True)
            olens = [int(x) for x in olens]
            out = dict(utterances=len(olens), frames=sum(olens), longest=max(olens))
            # (i), (ii): the calls alone, alternately
            calls = {"spsi_phase": lambda: gl.spsi_phase(mels, olens)}
            for k, kw in settings.items():
                calls["vocoder_" + k] = (lambda kw: lambda: gl(mels, olens, seed=0, **kw))(kw)
            ms = {k: [] for k in calls}
            for _ in range(R):
                for k, fn in calls.items():
                    ms[k].append(timed(fn, args.min_s)[0])
            for k, v in ms.items():
                out[k + "_ms"] = stat(v)
            d = out["vocoder_" + a + "_ms"]["median"] - out["vocoder_" + b + "_ms"]["median"]
            out["vocoder_ms_saved"] = round(d, 4)
            out["saved_more_than_spread"] = bool(d > max(out["vocoder_" + a + "_ms"]["spread"], out["vocoder_" + b + "_ms"]["spread"]))
            # (iv): spectral convergence of both settings on the same mels
            Mt = torch.clamp(torch.exp(mels) @ gl.constants(mels.device)[0].T, min=0)
            for k, kw in settings.items():
                w = gl(mels, olens, seed=0, **kw)
                X = stft_magnitude(w.wav, w.sample_lens)
                keep_rows = torch.cat([torch.full((L,), L >= 4, dtype=torch.bool) for L in olens]).to(mels.device)
                out["sc_" + k] = round(float(torch.linalg.norm((Mt - X)[keep_rows])) / float(torch.linalg.norm(Mt[keep_rows])), 5) \
                    if X.shape == Mt.shape else None
            # (iii): text -> wav per step
            rot = StepStreams(3)
            keep = []

            def sync_step(kw):
                def step():
                    m, ol = model.inference_batch(xs, il, packed=True)
                    return gl(m, ol, **kw)
                return step

            def async_step(kw):
                def step():
                    with rot.next():
                        am = model.inference_batch(xs, il, packed=True, sync=False)
                        keep.append((am, gl(am, sync=False, **kw)))
                    del keep[:-3]
                return step

            forms = {}
            for k, kw in settings.items():
                forms["sync_" + k] = (sync_step(kw), None)
                forms["async_" + k] = (async_step(kw), rot.join)
            for step, finish in forms.values():
                region(step, finish)
            pm = {k: [] for k in forms}
            for _ in range(R):
                for k, (step, finish) in forms.items():
                    pm[k].append(region(step, finish))
            am, w = keep[-1]
            out["async_ok"] = bool(model.async_ok() and am.ok() and w.ok())
            for k, v in pm.items():
                out["step_" + k + "_ms"] = stat(v)
            rec["workloads"][workload] = out
    print(json.dumps(rec))


def geometry_main(args):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude, tile_rule
    from tests.vocoder_oracle import harmonic_signal
    n_fft, hop, win = (int(x) for x in (args.geometry or "1024,256,1024").split(","))
    sr = args.sample_rate or 22050
    hp = DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "sample_rate": sr, "n_mels": 80}})
    gl = GriffinLim(hp)
    _, _, c3_olens = c3_mels(args.workload)
    T = [int(round(L * 256 / 22050.0 * sr)) for L in c3_olens]                   # the c3 utterances' durations at this rate
    dev = torch.device("cuda")
    wav = torch.from_numpy(np.concatenate([harmonic_signal(t, seed=b, f0=110.0 + 3 * (b % 40), sr=sr, noise=0.01) for b, t in enumerate(T)])
                           .astype(np.float32)).to(dev)
    M = stft_magnitude(wav, T, hp=hp)                                              # [N, bins]
    olens = [t // hop + 1 for t in T]
    N, B, NB = M.shape[0], len(olens), n_fft // 2 + 1
    run = lambda n: gl(M, olens, n_iter=n, seed=0, magnitudes=True, init=args.init)
    med = lambda xs: float(np.median(xs))
    hip = [timed(lambda: run(args.n_iter), args.min_s)[0] for _ in range(args.repeats)]
    ms_zero = med([timed(lambda: run(0), args.min_s)[0] for _ in range(max(1, args.repeats // 2))])
    ms_call = med(hip)
    ms_iter = (ms_call - ms_zero) / max(args.n_iter, 1)
    out = run(args.n_iter)
    Xh = stft_magnitude(out.wav, out.sample_lens, hp=hp)
    sc_hip = float(torch.linalg.norm(M - Xh)) / float(torch.linalg.norm(M))
    r = tile_rule(n_fft, hop)
    F, halo = r["F"], r["halo"]
    tiles = [(L, f0) for L in olens if L >= r["lmin"] for f0 in range(0, L, F)]
    span = sum(min(L - 1, f0 + min(F, L - f0) - 1 + halo) - max(0, min(f0 - halo, L - r["tail"])) + 1 for L, f0 in tiles)
    bytes_iter = span * NB * 8 + N * NB * 4 + N * NB * 8
    fft_flop = 2.5 * n_fft * math.log2(n_fft)
    flop_iter = (span + N) * fft_flop + N * NB * 12
    t_bytes = bytes_iter / (PEAK_HBM_TBS * 1e12) * 1e3
    t_flop = flop_iter / (PEAK_FP32_TFLOPS * 1e12) * 1e3
    rec = dict(workload=args.workload, geometry=[n_fft, hop, win], sample_rate=sr, tile_frames=F, halo=halo, utterances=B, frames=N,
               tiles=len(tiles), n_iter=args.n_iter, samples=int(out.wav.numel()), audio_seconds=round(sum(T) / sr, 3),
               hip_ms_runs=[round(x, 3) for x in hip], hip_ms_per_call=round(ms_call, 3), hip_ms_spread=round(max(hip) - min(hip), 3),
               hip_ms_call_n_iter0=round(ms_zero, 3), hip_ms_per_iter=round(ms_iter, 4), bytes_per_iter=bytes_iter, flop_per_iter=flop_iter,
               bound_ms_bytes=round(t_bytes, 4), bound_ms_flop=round(t_flop, 4),
               share_of_larger_bound=round(max(t_bytes, t_flop) / ms_iter, 3) if ms_iter > 0 else None,
               larger_bound="bytes" if t_bytes >= t_flop else "flop", sc_hip=round(sc_hip, 5))
    if not args.no_torch:
        Lmax = max(olens)
        Mp = torch.zeros(B, NB, Lmax, device=dev)
        o = 0
        for b, L in enumerate(olens):
            Mp[b, :, :L] = M[o:o + L].T
            o += L
        ang = (torch.rand(B, NB, Lmax, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 2 - 1) * math.pi
        tg = TorchGL(dev, n_fft, hop, win)
        tt = [timed(lambda: tg(Mp, olens, args.n_iter, ang), args.min_s)[0] for _ in range(args.repeats)]
        sig = tg(Mp, olens, args.n_iter, ang)
        parts = [sig[b, :hop * (L - 1)] for b, L in enumerate(olens)]
        Xt = stft_magnitude(torch.cat(parts).contiguous(), [hop * (L - 1) for L in olens], hp=hp)
        sc_torch = float(torch.linalg.norm(M - Xt)) / float(torch.linalg.norm(M))
        rec.update(torch_ms_runs=[round(x, 3) for x in tt], torch_ms_per_call=round(med(tt), 3), torch_ms_spread=round(max(tt) - min(tt), 3),
                   speedup_vs_torch=round(med(tt) / ms_call, 2), sc_torch=round(sc_torch, 5),
                   hip_beats_torch_by_more_than_spread=bool(med(tt) - ms_call > max(tt) - min(tt)),
                   sc_hip_within_1pct_of_torch=bool(sc_hip <= 1.01 * sc_torch))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
