"""Times of the excitation from F0, on the GPU, at the c3 shape of bench.py:

    python tools/time_excitation.py [--out FILE]

f0_phase beside spsi_phase, excitation alone, the vocoder call and text -> wav with init="f0", n_iter=0 beside the default 30 seeded
iterations (and beside init="spsi", n_iter=0).  The calls are timed alternately over R rounds, each for at least MIN_S seconds of
work that ends in a device synchronise; median and max - min spread per call.  The model is randomly initialised: its pitch is made
a known contour with pitch_scale=0 and a per-phoneme pitch_shift.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS  # noqa: E402
from fastspeech2_amd.synthetic import portable_state_dict, ljspeech_durations, make_batch  # noqa: E402
from fastspeech2_amd.vocoder import GriffinLim  # noqa: E402

R, MIN_S = 7, 0.4


def timed(fn):
    fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= MIN_S:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_excitation.py needs a GPU"
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(ljspeech_durations(portable_state_dict(model.state_dict(), seed=0)))
    model = model.cuda()
    gl = GriffinLim(hp)
    bt = make_batch("c3")
    xs, il = bt["xs"].cuda(), bt["ilens"]
    contour = (150.0 + 60.0 * torch.sin(0.35 * torch.arange(xs.shape[1], dtype=torch.float32))).repeat(xs.shape[0], 1).cuda()
    ctl = dict(pitch_scale=0.0, pitch_shift=contour)
    with torch.no_grad():
        mels, olens, f0 = model.inference_batch_pitch(xs, il, packed=True, **ctl)
        olens = [int(x) for x in olens]
        out = dict(workload="c3", utterances=len(olens), frames=sum(olens), longest=max(olens), rounds=R, min_s=MIN_S,
                   note="mels of a randomly initialised model with a commanded F0 contour: not speech")

        def text_to_wav(**kw):
            def step():
                m, ol, f = model.inference_batch_pitch(xs, il, packed=True, **ctl)
                gl(m, ol, f0=f if kw.get("init") == "f0" else None, **kw)
            return step
        calls = {"spsi_phase": lambda: gl.spsi_phase(mels, olens), "f0_phase": lambda: gl.f0_phase(f0, olens),
                 "excitation": lambda: gl.excitation(f0, olens),
                 "vocoder_seeded30": lambda: gl(mels, olens, n_iter=30), "vocoder_f0_0": lambda: gl(mels, olens, n_iter=0, init="f0", f0=f0),
                 "vocoder_spsi_0": lambda: gl(mels, olens, n_iter=0, init="spsi"),
                 "text_to_wav_seeded30": text_to_wav(n_iter=30), "text_to_wav_f0_0": text_to_wav(n_iter=0, init="f0")}
        ms = {k: [] for k in calls}
        for _ in range(R):
            for k, fn in calls.items():
                ms[k].append(timed(fn))
        for k, v in ms.items():
            out[k + "_ms"] = dict(median=round(float(np.median(v)), 4), spread=round(max(v) - min(v), 4), runs=[round(x, 4) for x in v])
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
