"""wav -> (log-mel, energy, f0) at c3 on one MI355X with and without the pitch path search: wav_features(f0_method="frame") (one
gl_features launch) against wav_features(f0_method="path") (one gl_candidates launch, then pitch_path and records_combine<8, 1, 5>;
csrc/gl_pitch.h, csrc/pitch_path.h), and the pitch_path call alone on the candidates of the same batch.
Prints one JSON line.

Workload: the c3 utterances (64, about 35.6 k frames) as synthetic harmonic waveforms of hop (L - 1) samples each with noise 0.3,
default geometry.  The forms are timed with device events around --calls calls, in alternating rounds after a warm-up round;
medians and max - min spreads over the rounds are reported.  The walk back is part of the pitch_path launch, so it has no time of
its own here.  ``path_share`` is the pitch_path call's time over wav_features(f0_method="path")'s.

Usage:  python tools/time_pitch_path.py [--rounds 7] [--calls 20] [--workload c3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--workload", default="c3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_pitch_path needs a GPU"
    from vocoder_bench import c3_mels
    from fastspeech2_amd.vocoder import GriffinLim, mel_energy, pitch_candidates, pitch_path, wav_features
    from tests.vocoder_oracle import harmonic_signal
    hp, _, olens = c3_mels(args.workload)
    gl = GriffinLim(hp)
    g, sr = gl.geometry, gl.params["sample_rate"]
    assert tuple(g) == (1024, 256, 1024, 80) and sr == 22050, "the timing is that of the default geometry"
    lens = [g.hop * max(L - 1, 0) for L in olens]
    frame_lens = [n // g.hop + 1 for n in lens]
    dev = torch.device("cuda")
    wav = torch.from_numpy(np.concatenate([harmonic_signal(t, seed=b, f0=110.0 + 3 * (b % 40), sr=sr, noise=0.3) for b, t in enumerate(lens)])
                           .astype(np.float32)).to(dev)
    cf, cs = pitch_candidates(wav, lens)
    time_step = g.hop / float(sr)
    # hp=None: the default geometry's GriffinLim (mel basis on the device) is built once and kept; a given hp builds one per call
    forms = {"mel_energy": lambda: mel_energy(wav, lens), "frame": lambda: wav_features(wav, lens, f0_method="frame"),
             "path": lambda: wav_features(wav, lens, f0_method="path"), "candidates": lambda: pitch_candidates(wav, lens),
             "pitch_path": lambda: pitch_path(cf, cs, frame_lens, time_step)}

    def region(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(args.calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / args.calls

    for fn in forms.values():
        region(fn)
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            ms[k].append(region(fn))
    f_frame, track = forms["frame"]()[2], forms["pitch_path"]()
    f_path = forms["path"]()[2]
    rec = dict(workload=args.workload, utterances=len(lens), frames=int(f_frame.numel()), longest_utterance_frames=max(frame_lens), samples=int(wav.numel()),
               geometry=list(g[:3]), rounds=args.rounds, calls_per_round=args.calls)
    for k, v in ms.items():
        rec[k + "_ms"] = round(float(np.median(v)), 4)
        rec[k + "_ms_spread"] = round(max(v) - min(v), 4)
        rec[k + "_ms_runs"] = [round(x, 4) for x in v]
    pu = track.per_utterance()
    rec.update(path_over_frame=round(rec["path_ms"] / rec["frame_ms"], 3), path_share=round(rec["pitch_path_ms"] / rec["path_ms"], 3),
               candidates_over_frame=round(rec["candidates_ms"] / rec["frame_ms"], 3), same_track=bool(torch.equal(f_path, track.f0)),
               voiced_frames_frame=int((f_frame > 0).sum()), voiced_frames_path=int((f_path > 0).sum()),
               changed_frames=int(pu["changed_frames"].sum()), flagged=int((pu["flags"] != 0).sum()))
    print(json.dumps(rec))
    return 0 if rec["same_track"] and rec["flagged"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
