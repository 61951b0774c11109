"""What the three workspace queries answer for a few batches: a refactor of the layout or of the workspace carving must leave every number alone.

    python tools/layout_workspace_sizes.py [--root TREE] [--out FILE.json]

For the default model and the one with reduction_factor = 2, and three batches (1, 3 and 64 utterances), prints {config: {batch: [fs2_token_workspace_bytes,
fs2_frame_workspace_bytes, fs2_row_capacity, fs2_frame_workspace_bytes_cap]}} as JSON.  The queries need a handle (fs2_create needs a device) but launch nothing.
--root runs another checkout's package (built there): profiles/layout_workspace_parent.json was recorded that way from the commit before csrc/layout_rule.h
existed; tests/test_gpu_parity.py compares sizes() of the tree under test with it."""
import argparse
import ctypes as C
import json
import os
import sys

CONFIGS = ("default", "reduction_factor_2")


def batches():
    """{name: (phonemes per utterance, frames per utterance)}: around the 128-frame attention block, equal counts, one long utterance."""
    import numpy as np
    rs = np.random.RandomState(17)
    il = rs.randint(1, 60, size=64)
    ol = il * rs.randint(3, 12, size=64)
    ol[:4] = [127, 128, 129, 129]
    ol[-1] = 1900
    return {"b1": ([23], [181]), "b3": ([5, 17, 33], [40, 131, 260]), "b64": (il.tolist(), ol.tolist())}


def make_model(config):
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    hp = default_hparams()
    if config == "reduction_factor_2":
        hp.model.reduction_factor = 2
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=3))
    return model.to("cuda:0")


def sizes():
    import torch
    from fastspeech2_amd import _lib
    out = {}
    for config in CONFIGS:
        model = make_model(config)
        out[config] = {}
        for name, (il, ol) in batches().items():
            B, Tmax = len(il), max(il)
            L = model._ensure_ready(torch.device("cuda:0"), Tmax, max(ol))
            h = model._handle
            batch = _lib.Batch(B, Tmax, (C.c_int64 * B)(*il), 0, _lib.PRECISIONS["bf16x3"])
            rows = int(L.fs2_row_capacity(C.byref(batch), sum(ol) + 100))
            out[config][name] = [int(L.fs2_token_workspace_bytes(h, C.byref(batch))), int(L.fs2_frame_workspace_bytes(h, C.byref(batch), (C.c_int64 * B)(*ol))), rows,
                                 int(L.fs2_frame_workspace_bytes_cap(h, C.byref(batch), rows, max(ol) + 32))]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package runs (default: this one)")
    ap.add_argument("--out", help="write the JSON here as well")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import fastspeech2_amd
    print("# package:", os.path.dirname(os.path.abspath(fastspeech2_amd.__file__)), file=sys.stderr)
    text = json.dumps(sizes(), indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
