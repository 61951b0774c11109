"""Cleaning of energy / F0 targets on one MI355X: fastspeech2_amd.targets.clean_targets (csrc/targets.h: tg_clean + tg_combine) against
the numpy oracle of the same definition (tests/targets_oracle.py: the reference's remove_outlier restated with vectorised numpy, so
already far faster than the reference's Python loop over every frame, which does not exist on the GPU machine).  Prints one JSON line.

Workloads: "c3" -- the frame counts of the c3 batch (64 utterances, about 35.6 k frames); "corpus" -- 13,100 utterances with
LJSpeech-like lengths (log-normal around 6.6 s at hop 256 / 22.05 kHz, 1.1 .. 10.1 s), about 7.7 M frames in one call.  Values are
F0-like (zeros and spikes) for the odd utterances and energy-like for the even ones.

Two GPU forms are timed in alternating rounds within one process (--rounds rounds, each form --calls calls between two device
synchronisations per round, after a warm-up round): "clean_targets", the Python entry point as a user calls it (allocation, the
launches, and the read-back of the statistics, which synchronises every call), and "launches", fs2_op_clean_targets alone on buffers
allocated once (what a caller that keeps the statistics on the device pays).  Medians and max - min spreads over the rounds are
reported.  The numpy oracle (clean of every utterance plus the float64 statistics) runs in this one process --oracle-runs times;
its output is compared with the GPU's (equality of the cleaned values) so that the two are known to compute the same thing.

Usage:  python tools/time_targets.py [--rounds 7] [--calls 20] [--oracle-runs 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def corpus_lens(n=13100, seed=0):
    rng = np.random.default_rng(seed)
    sec = np.clip(rng.lognormal(np.log(6.6), 0.45, n), 1.1, 10.1)
    return (sec * 22050 / 256).astype(np.int64) + 1


def make(lens, seed):
    from tests import targets_oracle as O
    rng = np.random.default_rng(seed)
    return [(O.f0_like if b % 2 else O.energy_like)(rng, int(n)) for b, n in enumerate(lens)]


def measure(name, utts, args):
    from fastspeech2_amd import _lib
    from fastspeech2_amd.targets import clean_targets
    from tests import targets_oracle as O
    lens = [u.size for u in utts]
    dev = torch.device("cuda")
    x = torch.from_numpy(np.concatenate(utts)).to(dev)
    lib = _lib.lib()
    B = len(lens)
    ln = np.ascontiguousarray(lens, np.int32)
    st = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)[:-1]]), np.int32)
    i32p = C.POINTER(C.c_int32)
    nb = int(lib.fs2_op_targets_workspace_bytes(B))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    rec = torch.empty(12, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launches():
        _lib.check(lib.fs2_op_clean_targets(stream, x.data_ptr(), B, st.ctypes.data_as(i32p), ln.ctypes.data_as(i32p), ws.data_ptr(), nb,
                                            y.data_ptr(), None, None, rec.data_ptr()))

    forms = {"clean_targets": lambda: clean_targets(x, lens), "launches": launches}

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
    oracle_ms = []
    for _ in range(args.oracle_runs):
        t0 = time.perf_counter()
        cleaned, ostats = O.clean_batch(utts)
        oracle_ms.append((time.perf_counter() - t0) * 1e3)
    yg, sg = clean_targets(x, lens)
    out = dict(workload=name, utterances=B, frames=int(x.numel()), rounds=args.rounds, calls_per_round=args.calls)
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_spread"] = round(max(v) - min(v), 4)
        out[k + "_ms_runs"] = [round(t, 4) for t in v]
    out.update(oracle_ms=round(float(np.median(oracle_ms)), 2), oracle_ms_runs=[round(t, 2) for t in oracle_ms],
               oracle_over_clean_targets=round(float(np.median(oracle_ms)) / out["clean_targets_ms"], 1),
               frames_per_second_launches=round(x.numel() / (out["launches_ms"] * 1e-3)),
               equals_oracle=bool(np.array_equal(yg.cpu().numpy(), np.concatenate([c.y for c in cleaned]))),
               counts_equal_oracle=bool(tuple(sg[:8]) == tuple(ostats[:8])),
               mean_rel_vs_oracle=abs(sg.mean / ostats.mean - 1.0), std_rel_vs_oracle=abs(sg.std / ostats.std - 1.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--oracle-runs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_targets needs a GPU"
    from vocoder_bench import c3_mels
    _, _, olens = c3_mels("c3")
    res = dict(c3=measure("c3", make([int(v) for v in olens], 1), args), corpus=measure("corpus", make(corpus_lens(), 2), args),
               threads=torch.get_num_threads())
    print(json.dumps(res))
    return 0 if res["c3"]["equals_oracle"] and res["corpus"]["equals_oracle"] else 1


if __name__ == "__main__":
    sys.exit(main())
