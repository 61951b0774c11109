"""The loss terms of the teacher-forced forward on one MI355X: fs2_op_loss_terms (csrc/losses.h: lt_terms + lt_combine) against the
PyTorch loss algebra of FeedForwardTransformer.forward() on the same device tensors.  Prints one JSON line.

Workload: the c3 batch (64 utterances, about 35.6 k frames, odim 80): the outputs of the teacher-forced forward (padded_compat, so
the pad positions hold what forward() sees there), random mel targets, the batch's own ds / es / ps.

Three forms are timed in alternating rounds within one process (--rounds rounds, each form --calls calls between two device
synchronisations per round, after a warm-up round): "op_masked", fs2_op_loss_terms alone with pads = 0 on buffers allocated once
(what use_masking = True needs: about 34 MB read); "op_pads", the same with pads = 1 (every padded position read as well: what
use_masking = False needs); and "torch_algebra", the masked_select / l1_loss / mse_loss / .item() sequence of forward() (restated
below from fastspeech.py, use_masking = True) including its seven .item() calls, each of which synchronises.  Medians and
max - min spreads over the rounds are reported, the op's achieved bytes / s, and the agreement of the two results.

Usage:  python tools/time_losses.py [--rounds 7] [--calls 50]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12      # bytes / s of a float4 copy kernel on the MI355X (the microarchitecture guide's measured ceiling)


def torch_algebra(before, after, ys, d_outs, ds_t, e_outs, es, p_outs, ps, il, ol):
    """forward()'s loss algebra under use_masking = True, use_weighted_masking = False, with its seven .item() calls."""
    dev = before.device
    ar_t = torch.arange(d_outs.shape[1], device=dev).unsqueeze(0)
    ar_l = torch.arange(before.shape[1], device=dev).unsqueeze(0)
    in_masks = ar_t < il.to(dev).unsqueeze(1)
    mel_masks = ar_l < ol.to(dev).unsqueeze(1)
    out_masks = mel_masks.unsqueeze(-1)
    es, ps = es[:, : before.shape[1]], ps[:, : before.shape[1]]
    d_outs, ds_t = d_outs.masked_select(in_masks), ds_t.masked_select(in_masks)
    before, after = before.masked_select(out_masks), after.masked_select(out_masks)
    es, ps = es.masked_select(mel_masks), ps.masked_select(mel_masks)
    e_outs, p_outs = e_outs.masked_select(mel_masks), p_outs.masked_select(mel_masks)
    ys = ys.masked_select(out_masks)
    before_loss = F.l1_loss(before, ys)
    after_loss = F.l1_loss(after, ys)
    l1_loss = before_loss + after_loss
    duration_loss = F.mse_loss(d_outs, torch.log(ds_t.float() + 1.0))
    energy_loss = F.mse_loss(e_outs, es)
    pitch_loss = F.mse_loss(p_outs, ps)
    loss = l1_loss + duration_loss + energy_loss + pitch_loss
    return [l1_loss.item(), before_loss.item(), after_loss.item(), duration_loss.item(), energy_loss.item(), pitch_loss.item(), loss.item()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_losses needs a GPU"
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS, _lib
    from fastspeech2_amd.losses import LossTerms
    from fastspeech2_amd.synthetic import portable_state_dict, make_batch
    dev = torch.device("cuda")
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.to(dev)
    b = make_batch("c3")
    il, ol = b["ilens"].long(), b["olens"].long()
    ds, es, ps = b["ds"].to(dev), b["es"].to(dev), b["ps"].to(dev)
    with torch.no_grad():
        r = model._run(b["xs"].to(dev), il, ol, ds, es, ps, is_inference=False, compat=True, want=("before", "after", "e_outs", "p_outs"))
    before, after, d_outs, e_outs, p_outs = r["before"], r["after"], r["d_log"], r["e_outs"], r["p_outs"]
    B, Lmax, odim = before.shape
    Tmax = d_outs.shape[1]
    gen = torch.Generator(device="cpu").manual_seed(0)
    ys = torch.randn(B, Lmax, odim, generator=gen).to(dev) * (torch.arange(Lmax).unsqueeze(0) < ol.unsqueeze(1)).unsqueeze(-1).to(dev)
    torch.cuda.synchronize()

    lib = _lib.lib()
    i32p = C.POINTER(C.c_int32)
    il_np, ol_np = np.ascontiguousarray(il.numpy(), np.int32), np.ascontiguousarray(ol.numpy(), np.int32)
    nb = int(lib.fs2_op_loss_workspace_bytes(B, ol_np.ctypes.data_as(i32p)))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    rec = torch.empty(B + 1, 20, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def op(pads):
        a = _lib.OpLossArgs(B, odim, Tmax, Lmax, pads, Lmax, Lmax, Tmax, ds.shape[1], es.shape[1],
                            before.data_ptr(), after.data_ptr(), ys.data_ptr(), d_outs.data_ptr(), ds.data_ptr(), e_outs.data_ptr(), es.data_ptr(),
                            p_outs.data_ptr(), ps.data_ptr(), il_np.ctypes.data_as(i32p), ol_np.ctypes.data_as(i32p), ws.data_ptr(), nb,
                            rec.data_ptr(), rec[B].data_ptr())
        return lambda: _lib.check(lib.fs2_op_loss_terms(stream, C.byref(a)))

    forms = {"op_masked": op(0), "op_pads": op(1),
             "torch_algebra": lambda: torch_algebra(before, after, ys, d_outs, ds, e_outs, es, p_outs, ps, il, ol)}

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls * 1e3

    with torch.no_grad():
        for fn in forms.values():
            region(fn)
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                ms[k].append(region(fn))
        forms["op_masked"]()
        host = rec.cpu().numpy()
        ours = [v for _, v in LossTerms(host[:-1], host[-1], False, odim).report()]
        theirs = torch_algebra(before, after, ys, d_outs, ds, e_outs, es, p_outs, ps, il, ol)
    frames, tokens = int(ol.sum()), int(il.sum())
    per_frame, per_token = 3 * odim * 4 + 4 * 4, 4 + 8
    bytes_masked = frames * per_frame + tokens * per_token
    bytes_pads = B * Lmax * per_frame + B * Tmax * per_token
    out = dict(workload="c3", utterances=B, frames=frames, Lmax=Lmax, tiles=int(sum(max(1, -(-int(v) // 32)) for v in ol_np)),
               rounds=args.rounds, calls_per_round=args.calls, bytes_masked=bytes_masked, bytes_pads=bytes_pads)
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 5)
        out[k + "_ms_spread"] = round(max(v) - min(v), 5)
        out[k + "_ms_runs"] = [round(t, 5) for t in v]
    out.update(op_masked_bytes_per_s=round(bytes_masked / (out["op_masked_ms"] * 1e-3)), op_pads_bytes_per_s=round(bytes_pads / (out["op_pads_ms"] * 1e-3)),
               torch_over_op_masked=round(out["torch_algebra_ms"] / out["op_masked_ms"], 1),
               report_rel_vs_torch=float(np.max(np.abs(np.asarray(ours) / np.asarray(theirs) - 1.0))))
    out["op_masked_fraction_of_copy_ceiling"] = round(out["op_masked_bytes_per_s"] / COPY_CEILING, 4)
    print(json.dumps(out))
    return 0 if out["report_rel_vs_torch"] <= 1e-5 else 1


if __name__ == "__main__":
    sys.exit(main())
