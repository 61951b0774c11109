"""What pitch / energy control costs on one MI355X: ``inference_batch`` of the c3 batch in mix_mx4 with and without a per-phoneme pitch
shift plus an energy scale (fs2_decode_ctl: one launch of prosody_apply over the packed frame rows, csrc/prosody.h).  Prints one
JSON line.

Forms: ``plain`` / ``control`` are the synchronous call (the frame counts are read back between encoder and decoder), ``plain_async``
/ ``control_async`` the sync-free one (``sync=False``).  Each is timed with device events around --calls calls, in alternating rounds
after a warm-up round; medians and max - min spreads over the rounds are reported, and the time of the var.control launch itself
from the library's per-launch profile.

``--root DIR`` measures the package of another checkout instead (the parent commit's, built there: the uncontrolled call must not
have moved); a checkout without control is timed on the plain forms only.

Usage:  python tools/time_prosody.py [--rounds 5] [--calls 10] [--precision mix_mx4] [--root DIR]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--precision", default="mix_mx4")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    assert torch.cuda.is_available(), "time_prosody needs a GPU"
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import ljspeech_durations, make_batch, portable_state_dict
    dev = torch.device("cuda:0")
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(ljspeech_durations(portable_state_dict(model.state_dict(), seed=0)))
    model = model.to(dev)
    model.precision = args.precision
    b = make_batch("c3")
    xs, il = b["xs"].to(dev), b["ilens"]
    B, T = xs.shape
    has_control = "pitch_shift" in inspect.signature(model.inference_batch).parameters
    g = torch.Generator().manual_seed(0)
    ctl = dict(pitch_shift=(80.0 * torch.rand((B, T), generator=g) - 40.0).to(dev), energy_scale=1.1) if has_control else {}
    forms = {"plain": lambda: model.inference_batch(xs, il), "plain_async": lambda: model.inference_batch(xs, il, sync=False)}
    if has_control:
        forms["control"] = lambda: model.inference_batch(xs, il, **ctl)
        forms["control_async"] = lambda: model.inference_batch(xs, il, sync=False, **ctl)

    def region(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    with torch.no_grad():
        mel, ol = model.inference_batch(xs, il)
        for fn in forms.values():
            region(fn, 2)
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                ms[k].append(region(fn, args.calls))
        ok = model.async_ok()
        out = dict(workload="c3 (64 utterances), free-running, seed-0 weights with LJSpeech-like durations", precision=args.precision, utterances=B,
                   phonemes=int(il.sum()), frames=int(ol.sum()), rounds=args.rounds, calls_per_round=args.calls, has_control=has_control, async_ok=bool(ok))
        if has_control:
            mel_c, ol_c = model.inference_batch(xs, il, **ctl)
            out["control_changes_the_mel"] = bool(torch.equal(ol_c, ol) and not torch.equal(mel_c, mel))
            model.set_profiling(True, only="var.control")
            for _ in range(args.calls):
                model.inference_batch(xs, il, **ctl)
            prof = [r[1] for r in model.get_profile()]
            model.set_profiling(False)
            out["var_control_launches_per_call"] = len(prof) / args.calls
            out["var_control_us"] = round(1e3 * float(np.median(prof)), 2)
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_spread"] = round(max(v) - min(v), 4)
        out[k + "_ms_runs"] = [round(t, 4) for t in v]
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
