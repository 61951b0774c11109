"""The forced alignment on one MI355X: fs2_op_align (csrc/align.h: dtw_dist on the swapped sides + align_sweep with its walk back +
records_combine<8, 2, -1>) beside fs2_op_dtw on the SAME 64 pairs.  Prints one JSON line.

Workload: 64 pairs of 80-dimensional frames; M = the c3 batch's recorded lengths, N = M scaled by a factor in [0.85, 1.15] (what a
free-running synthesis of the same text gives); b is a time-warped noisy copy of a, so every pair has an alignment.  Both ops are
timed with device events around --calls calls, in alternating rounds after a warm-up round; medians and max - min spreads over the
rounds are reported.  The walk back is part of the align_sweep launch, so it has no time of its own here.  ``--root DIR`` measures the
package of another checkout instead (the parent commit's, built there).

Usage:  python tools/time_align.py [--rounds 5] [--calls 10] [--max-step 2] [--root DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--max-step", type=int, default=2)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    assert torch.cuda.is_available(), "time_align needs a GPU"
    from fastspeech2_amd import _lib
    from fastspeech2_amd.synthetic import make_batch
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    bl = make_batch("c3")["olens"].numpy().astype(np.int32)
    B, D = len(bl), 80
    al = np.maximum(1, np.rint(bl * rng.uniform(0.85, 1.15, B))).astype(np.int32)
    a_np = rng.normal(-5, 2, (int(al.sum()), D)).astype(np.float32)
    as_np, bs_np = (np.cumsum(al) - al).astype(np.int32), (np.cumsum(bl) - bl).astype(np.int32)
    b_np = np.concatenate([a_np[as_np[n] + np.sort(rng.integers(0, al[n], bl[n]))] for n in range(B)])
    b_np = (b_np + 0.1 * rng.normal(0, 1, b_np.shape)).astype(np.float32)
    a, b = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)

    lib = _lib.lib()
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec_d = torch.empty(B + 1, _lib.DTW_TERMS, dtype=torch.float64, device=dev)
    rec_a = torch.empty(B + 1, _lib.ALIGN_TERMS, dtype=torch.float64, device=dev)
    T = int(al.max())
    dur = torch.empty(B, T, dtype=torch.int64, device=dev)
    state = torch.empty(int(bl.sum()), dtype=torch.int32, device=dev)
    nb_d = int(lib.fs2_op_dtw_workspace_bytes(B, p32(al), p32(bl), 1 << 44))
    nb_a = int(lib.fs2_op_align_workspace_bytes(B, p32(al), p32(bl), 1 << 44))
    ws = torch.empty(max(nb_d, nb_a), dtype=torch.uint8, device=dev)
    xd = _lib.OpDtwArgs(B, D, D, D, a.data_ptr(), b.data_ptr(), None, None, None, None, p32(as_np), p32(al), p32(bs_np), p32(bl),
                        ws.data_ptr(), nb_d, rec_d.data_ptr(), rec_d[B].data_ptr())
    xa = _lib.OpAlignArgs(B, D, args.max_step, D, D, T, a.data_ptr(), b.data_ptr(), None, p32(as_np), p32(al), p32(bs_np), p32(bl), None,
                          ws.data_ptr(), nb_a, dur.data_ptr(), state.data_ptr(), rec_a.data_ptr(), rec_a[B].data_ptr())
    forms = {"align": lambda: _lib.check(lib.fs2_op_align(stream, C.byref(xa))), "dtw": lambda: _lib.check(lib.fs2_op_dtw(stream, C.byref(xd)))}

    def region(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    for fn in forms.values():
        region(fn, 2)
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            ms[k].append(region(fn, args.calls))
    forms["align"]()
    torch.cuda.synchronize()
    rows, d = rec_a.cpu().numpy()[:-1], dur.cpu().numpy()
    ok = bool(np.all(rows[:, 2] == 0) and np.array_equal(d.sum(1), bl.astype(np.int64)))
    out = dict(workload="64 pairs, c3 recorded lengths, N / M in [0.85, 1.15]", pairs=B, D=D, max_step=args.max_step,
               cells=int((al.astype(np.int64) * bl).sum()), median_pair=[int(np.median(al)), int(np.median(bl))], longest_pair=[int(al.max()), int(bl.max())],
               workspace_bytes_align=nb_a, workspace_bytes_dtw=nb_d, rounds=args.rounds, calls_per_round=args.calls, all_aligned_and_sums_match=ok,
               mean_cost_per_frame=float(np.mean(rows[:, 3] / rows[:, 1])), mean_longest_stay=float(np.mean(rows[:, 5])))
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_spread"] = round(max(v) - min(v), 4)
        out[k + "_ms_runs"] = [round(t, 4) for t in v]
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
