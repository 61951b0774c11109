"""Wall time of fs2_load_weights for the default model (on an MI355X): one JSON line per process.

    python tools/time_weight_load.py [--root TREE] [--loads N]

The handle is created and loaded once by a small forward (that load also pays for the first use of every repack kernel); then fs2_load_weights is called N times on
the same handle with the same tensors and each call is timed on the host -- the call returns after its own stream synchronisation.  --root runs another checkout's
package (built there): run parent and tree alternating, one fresh process each (profiles/weight_plan_time.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package runs (default: this one)")
    ap.add_argument("--loads", type=int, default=9)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import fastspeech2_amd
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS, _lib
    from fastspeech2_amd.synthetic import portable_state_dict, make_batch
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.to("cuda:0")
    b = make_batch("c1")
    with torch.no_grad():
        t0 = time.perf_counter()
        model.inference(b["xs"][0, : int(b["ilens"][0])].cuda())
        torch.cuda.synchronize()
        first_call_ms = (time.perf_counter() - t0) * 1e3
    tensors = [(n, t.detach().contiguous()) for n, t in model.state_dict().items() if t.dtype == torch.float32]
    descs = [_lib.TensorDesc(n.encode(), t.data_ptr(), t.dim(), (C.c_int64 * 4)(*(list(t.shape) + [0] * (4 - t.dim())))) for n, t in tensors]
    arr = (_lib.TensorDesc * len(descs))(*descs)
    L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = []
    for _ in range(args.loads):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.fs2_load_weights(model._handle, arr, len(descs), stream), model._handle)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms_sorted = sorted(ms)
    print(json.dumps({"package": os.path.dirname(os.path.abspath(fastspeech2_amd.__file__)), "loads": args.loads, "load_ms": [round(m, 3) for m in ms],
                      "load_ms_median": round(ms_sorted[len(ms) // 2], 3), "first_inference_ms": round(first_call_ms, 1)}))


if __name__ == "__main__":
    main()
