"""wav -> (log-mel, energy, f0) at c3 on one MI355X: wav_features (one gl_features launch, csrc/gl_pitch.h) against mel_energy (the
launch without pitch) and against a torch composition of the same definition on the same GPU (torch.fft.rfft / irfft plus tensor
ops, float32, every frame of the batch in one [frames, n_fft] tensor).  Prints one JSON line.

Workload: the c3 utterances (64, about 35.6 k frames) as synthetic harmonic waveforms of hop (L - 1) samples each, default geometry.
The three forms are timed in alternating rounds within one process (--rounds rounds, each form --calls calls between two device
synchronisations per round, after a warm-up round); medians and max - min spreads over the rounds are reported, and the gate
``wav_features_beats_torch``: wav_features' slowest round is faster than the torch composition's median.  The torch composition's
f0 is compared with wav_features' (same voicing decision, relative difference where both are voiced) so that the two are known to
compute the same thing.

Usage:  python tools/time_pitch.py [--rounds 7] [--calls 20] [--workload c3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


class TorchFeatures:
    """The definition of fastspeech2_amd.vocoder.wav_features in torch ops (float32, any device): frames by reflect padding and
    unfold per waveform, everything after that on all frames at once."""

    def __init__(self, device, n_fft, hop, win, sr, basis, f0_floor=71.0, f0_ceil=800.0, voicing_threshold=0.45, octave_cost=0.02):
        self.n_fft, self.hop, self.sr = n_fft, hop, float(sr)
        w = torch.zeros(n_fft, dtype=torch.float64)
        lp = (n_fft - win) // 2
        w[lp:lp + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
        rw = torch.fft.irfft(torch.fft.rfft(w).abs() ** 2, n=n_fft)
        self.tmin, self.tmax = int(math.floor(sr / f0_ceil)), int(math.ceil(sr / f0_floor))
        lags = torch.arange(self.tmin - 1, self.tmax + 2)
        self.lag0 = self.tmin - 1
        self.norm = (rw[0] / rw[lags]).float().to(device)                  # [lags]
        self.win = w.float().to(device)
        self.basis = basis.to(device)                                       # [n_mels, bins]
        self.tau = torch.arange(self.tmin, self.tmax + 1, dtype=torch.float32, device=device)
        self.floor, self.thr, self.oc = float(f0_floor), float(voicing_threshold), float(octave_cost)

    def __call__(self, wav_packed, lens):
        n, h = self.n_fft, self.hop
        frames, o = [], 0
        for T in lens:
            x = wav_packed[o:o + T]
            o += T
            if T > n // 2:
                frames.append(torch.nn.functional.pad(x[None, None], (n // 2, n // 2), mode="reflect")[0, 0].unfold(0, n, h))
            else:
                frames.append(wav_packed.new_zeros(T // h + 1, n))
        y = torch.cat(frames) * self.win
        mag = torch.fft.rfft(y).abs()
        logmel = torch.log(torch.clamp(mag @ self.basis.T, min=1e-5))
        energy = torch.linalg.norm(mag, dim=1)
        r = torch.fft.irfft(mag * mag, n=n)
        r0 = r[:, :1]
        live = r0 > 1e-12
        rho = r[:, self.lag0:self.lag0 + self.norm.numel()] / torch.where(live, r0, torch.ones_like(r0)) * self.norm
        a, c, b = rho[:, :-2], rho[:, 1:-1], rho[:, 2:]
        cand = (c > a) & (c >= b) & (c > 0) & live
        d = 0.5 * (a - b) / torch.where(cand, (a - c) + (b - c), -torch.ones_like(a))
        ts = self.tau + d
        p = c - 0.25 * (a - b) * d
        S = torch.where(cand, p - self.oc * torch.log2(torch.where(cand, self.floor / self.sr * ts, torch.ones_like(ts))),
                        torch.full_like(p, -float("inf")))
        best = S.argmax(dim=1, keepdim=True)
        pw = torch.where(cand.any(dim=1), p.gather(1, best)[:, 0], torch.zeros_like(p[:, 0]))
        voiced = cand.any(dim=1) & (pw >= self.thr)
        f0 = torch.where(voiced, self.sr / ts.gather(1, best)[:, 0], torch.zeros_like(pw))
        return logmel, energy, f0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--workload", default="c3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_pitch needs a GPU"
    from vocoder_bench import c3_mels
    from fastspeech2_amd.vocoder import GriffinLim, mel_energy, wav_features
    from tests.vocoder_oracle import harmonic_signal
    hp, _, olens = c3_mels(args.workload)
    gl = GriffinLim(hp)
    g, sr = gl.geometry, gl.params["sample_rate"]
    assert tuple(g) == (1024, 256, 1024, 80) and sr == 22050, "the timing is that of the default geometry"
    lens = [g.hop * max(L - 1, 0) for L in olens]
    dev = torch.device("cuda")
    wav = torch.from_numpy(np.concatenate([harmonic_signal(t, seed=b, f0=110.0 + 3 * (b % 40), sr=sr, noise=0.01) for b, t in enumerate(lens)])
                           .astype(np.float32)).to(dev)
    tf = TorchFeatures(dev, g.n_fft, g.hop, g.win, sr, gl.constants(dev)[1])
    # hp=None: the default geometry's GriffinLim (mel basis on the device) is built once and kept; a given hp builds one per call
    forms = {"mel_energy": lambda: mel_energy(wav, lens), "wav_features": lambda: wav_features(wav, lens), "torch": lambda: tf(wav, lens)}

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls * 1e3

    for fn in forms.values():
        region(fn)
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            ms[k].append(region(fn))
    lm, en, f0 = forms["wav_features"]()
    lt, et, ft = forms["torch"]()
    both = (f0 > 0) & (ft > 0)
    rec = dict(workload=args.workload, utterances=len(lens), frames=int(f0.numel()), samples=int(wav.numel()), geometry=list(g[:3]),
               rounds=args.rounds, calls_per_round=args.calls)
    for k, v in ms.items():
        rec[k + "_ms"] = round(float(np.median(v)), 4)
        rec[k + "_ms_spread"] = round(max(v) - min(v), 4)
        rec[k + "_ms_runs"] = [round(x, 4) for x in v]
    rec.update(pitch_cost_ms=round(rec["wav_features_ms"] - rec["mel_energy_ms"], 4),
               wav_features_over_mel_energy=round(rec["wav_features_ms"] / rec["mel_energy_ms"], 3),
               torch_over_wav_features=round(rec["torch_ms"] / rec["wav_features_ms"], 2),
               wav_features_beats_torch=bool(max(ms["wav_features"]) < rec["torch_ms"]),
               voiced_frames=int(both.sum()), voicing_disagreements=int(((f0 > 0) != (ft > 0)).sum()),
               f0_rel_vs_torch=float((f0[both] / ft[both] - 1).abs().max()) if both.any() else 0.0,
               logmel_maxabs_vs_torch=float((lm - lt).abs().max()), energy_rel_vs_torch=float(((en - et).abs() / et.clamp(min=1e-6)).max()))
    print(json.dumps(rec))
    return 0 if rec["wav_features_beats_torch"] else 1


if __name__ == "__main__":
    sys.exit(main())
