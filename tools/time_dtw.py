"""The DTW of the free-running validation on one MI355X: fs2_op_dtw (csrc/dtw.h: dtw_dist + dtw_sweep + records_combine<12, -1, -1>) on the c3-shaped
validation batch, beside (a) the free-running forward that produces its input and (b) what a user would write today -- torch.cdist
plus one torch step per anti-diagonal -- for ONE pair of median length.  Prints one JSON line.

Workload: the c3 batch (64 utterances): a = the mels, e_outs and p_outs of the model's free-running forward (seed-0 weights with
LJSpeech-like durations), b = random mel targets of the batch's own recorded lengths with its es / ps.  About 20 M cells of
80-dimensional distances.

Forms, timed in alternating rounds within one process (--rounds rounds, each form --calls calls between two device
synchronisations per round, after a warm-up round): "dtw", fs2_op_dtw alone on resident buffers with everything held at once;
"dtw_cap", the same through a workspace of --cap-mb MB (groups of pairs); "forward", model.inference_batch of the same batch
(synchronous: it reads the frame counts back); "torch_one_pair", the torch loop for the pair of median cell count (--torch-calls
calls per round: it is slow).  Medians and max - min spreads over the rounds are reported.  The kernels' own durations come from a
run of their own: rocprofv3 --kernel-trace --stats -- python tools/time_dtw.py --only-op.  ``--root DIR`` measures the package of
another checkout instead (the parent commit's, built there).

Usage:  python tools/time_dtw.py [--rounds 5] [--calls 10] [--torch-calls 1] [--cap-mb 32] [--only-op] [--root DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch


def torch_dtw_cost(a, b):
    """C(N-1, M-1) with torch alone: cdist in double, then one step per anti-diagonal (cost only: no records are carried)."""
    d = torch.cdist(a.double(), b.double())
    N, M = d.shape
    Cm = torch.full((N + 1, M + 1), float("inf"), dtype=torch.float64, device=a.device)
    Cm[0, 0] = 0.0
    for k in range(N + M - 1):
        i = torch.arange(max(0, k - M + 1), min(N - 1, k) + 1, device=a.device)
        j = k - i
        Cm[i + 1, j + 1] = d[i, j] + torch.minimum(torch.minimum(Cm[i, j], Cm[i, j + 1]), Cm[i + 1, j])
    return Cm[N, M]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--cap-mb", type=int, default=32)
    ap.add_argument("--only-op", action="store_true", help="time fs2_op_dtw only (for a kernel-trace run)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    assert torch.cuda.is_available(), "time_dtw needs a GPU"
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS, _lib
    from fastspeech2_amd.synthetic import ljspeech_durations, portable_state_dict, make_batch
    dev = torch.device("cuda")
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(ljspeech_durations(portable_state_dict(model.state_dict(), seed=0)))
    model = model.to(dev)
    b = make_batch("c3")
    xs, il = b["xs"].to(dev), b["ilens"].long()
    with torch.no_grad():
        r = model._run(xs, il, is_inference=True, want=("after", "e_outs", "p_outs"))
    a, e_a, p_a, al = r["after"], r["e_outs"], r["p_outs"], r["olens"]
    B, Sa, D = a.shape
    bl = b["olens"].long()
    Sb = int(bl.max())
    gen = torch.Generator(device="cpu").manual_seed(0)
    ys = (torch.randn(B, Sb, D, generator=gen) * 2 - 5).to(dev)
    e_b, p_b = b["es"].to(dev), b["ps"].to(dev)
    assert e_b.shape[1] == Sb and e_a.shape[1] == Sa
    torch.cuda.synchronize()

    lib = _lib.lib()
    i32p = C.POINTER(C.c_int32)
    i32 = lambda x: np.ascontiguousarray(np.asarray(x), np.int32)
    al_np, bl_np = i32(al.numpy()), i32(bl.numpy())
    as_np, bs_np = i32(np.arange(B) * Sa), i32(np.arange(B) * Sb)
    p32 = lambda x: x.ctypes.data_as(i32p)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = torch.empty(B + 1, _lib.DTW_TERMS, dtype=torch.float64, device=dev)

    def op(cap):
        nb = int(lib.fs2_op_dtw_workspace_bytes(B, p32(al_np), p32(bl_np), cap))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        x = _lib.OpDtwArgs(B, D, D, D, a.data_ptr(), ys.data_ptr(), e_a.data_ptr(), e_b.data_ptr(), p_a.data_ptr(), p_b.data_ptr(),
                           p32(as_np), p32(al_np), p32(bs_np), p32(bl_np), ws.data_ptr(), nb, rec.data_ptr(), rec[B].data_ptr())
        return (lambda: _lib.check(lib.fs2_op_dtw(stream, C.byref(x)))), nb, (ws, x)

    dtw_all, bytes_all, keep1 = op(1 << 44)
    dtw_cap, bytes_cap, keep2 = op(args.cap_mb << 20)
    cells = al_np.astype(np.int64) * bl_np.astype(np.int64)
    mid = int(np.argsort(cells)[B // 2])
    a1, b1 = a[mid, : al_np[mid]], ys[mid, : bl_np[mid]]
    forms = {"dtw": (dtw_all, args.calls), "dtw_cap": (dtw_cap, args.calls)}
    if not args.only_op:
        forms["forward"] = (lambda: model.inference_batch(xs, il), args.calls)
        forms["torch_one_pair"] = (lambda: torch_dtw_cost(a1, b1), args.torch_calls)

    def region(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    with torch.no_grad():
        for fn, calls in forms.values():
            region(fn, 1)
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, (fn, calls) in forms.items():
                ms[k].append(region(fn, calls))
        dtw_all()
        all_at_once = rec.cpu().numpy().copy()
        dtw_cap()
        grouped = rec.cpu().numpy().copy()
        theirs = None if args.only_op else float(torch_dtw_cost(a1, b1))
    steps_sweep = int(sum((-(-int(m) // 256)) * (int(n) + 300) for n, m in zip(al_np, bl_np)))
    out = dict(workload="c3 free-running against recorded lengths", pairs=B, D=D, cells=int(cells.sum()), frames_pred=int(al_np.sum()),
               frames_ref=int(bl_np.sum()), median_pair=[int(al_np[mid]), int(bl_np[mid])], workspace_bytes=bytes_all,
               workspace_bytes_cap=bytes_cap, rounds=args.rounds, calls_per_round=args.calls, sweep_steps_upper=steps_sweep,
               grouped_equals_all_at_once=bool(np.array_equal(all_at_once.view(np.uint64), grouped.view(np.uint64))),
               mean_distance=float(np.mean(all_at_once[:-1, 3] / all_at_once[:-1, 2])))
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_spread"] = round(max(v) - min(v), 4)
        out[k + "_ms_runs"] = [round(t, 4) for t in v]
    ok = out["grouped_equals_all_at_once"]
    if theirs is not None:
        out["cost_rel_vs_torch_one_pair"] = abs(float(all_at_once[mid, 3]) / theirs - 1.0)
        out["dtw_over_forward"] = round(out["dtw_ms"] / out["forward_ms"], 3)
        out["torch_one_pair_over_dtw_batch"] = round(out["torch_one_pair_ms"] / out["dtw_ms"], 1)
        ok = ok and out["cost_rel_vs_torch_one_pair"] <= 1e-9
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
