"""Digest of one small forward per launch-forming case: what a change of the host code that forms the model's launches must leave alone.

For every case -- the default FFT block and the pre-LN + concat_after one, in fp32 / bf16x3 / mix_mx / mix_mx4, with the kernel choice automatic and with the
row-complete kernels forced (FS2_ROW8 = 1: the planes-only regime at this size), plus the device-driven layout of the default block -- one teacher-forced
forward of 3 utterances (5, 17 and 33 phonemes, synthetic weights):

    python tools/forward_digest.py [--root TREE] [--names FILE.json] [--call-names FILE.json]

prints `<case> <sha256 over before, after, d, e, p>`; --names also writes the ordered profile names of each case's launches.  CALL_CASES adds, on the same
utterances and the default block, the cases the per-call decisions of csrc/call_plan.h depend on and the ones above do not reach (every FS2_TOKPROJ value,
FS2_FUSE_VAR = 0, a free-running forward, per-phoneme pitch control, reduction_factor = 2, the device-driven layout with the packed output): `<case> <sha256
over the outputs it asks for>`, their names to --call-names (profiles/call_plan_names_parent.json, profiles/call_plan_digest.txt).  --root runs another checkout's
package (built there) with this file's cases: run it on the parent commit twice and on the tree under test, on one machine; where the parent equals itself the
tree must equal the parent (profiles/model_launches_digest.txt).  LOAD_CASES adds, on the same utterances, the configurations that reach the branches of the weight
loader (csrc/weight_plan.h) the cases above do not -- a Linear FFN, no BatchNorm, a 3-tap FFN, padded heads, concat_after on padded heads, a 256-wide decoder -- in fp32,
bf16x3 and mix_mx4, and the default block after a second fs2_load_weights on the same handle (profiles/weight_plan_digest.txt).  tests/test_gpu_parity.py compares launch_names() with the names recorded from the parent
(profiles/model_launches_names_parent.json)."""
import argparse
import hashlib
import json
import os
import sys

BLOCKS = {"default": {}, "pre_ln_concat": dict(encoder_normalize_before=True, decoder_normalize_before=True, encoder_concat_after=True, decoder_concat_after=True)}
MODES = ("fp32", "bf16x3", "mix_mx", "mix_mx4")
TLENS = [5, 17, 33]


def case_id(block, precision, row8):
    return "%s/%s/%s" % (block, precision, "row8" if row8 else "auto")


def make_model(block):
    import torch  # noqa: F401
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    hp = default_hparams()
    for k, v in BLOCKS[block].items():
        hp.model[k] = v
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=3))
    return model.to("cuda:0")


def make_inputs():
    from fastspeech2_amd.synthetic import make_batch
    b = make_batch("c2", seed=11, B=len(TLENS), tlens=TLENS)      # (durations from the synthetic Gamma fit: about 8 frames per phoneme)
    return {k: (v.cuda() if k in ("xs", "ds", "es", "ps") else v) for k, v in b.items()}


def forward(model, b, precision, row8, profile=False):
    """One teacher-forced forward -> (dict of outputs, ordered profile names or None).  FS2_ROW8 is restored to automatic afterwards."""
    import torch
    from fastspeech2_amd import _lib
    want = ("before", "after", "e_outs", "p_outs")
    model.precision = precision
    _lib.set_option("FS2_ROW8", 1 if row8 else -1)
    try:
        with torch.no_grad():
            r = model._run(b["xs"], b["ilens"], b["olens"], b["ds"], b["es"], b["ps"], is_inference=False, want=want)      # (creates the handle on first use)
            names = None
            if profile:
                model.set_profiling(True)
                try:
                    r = model._run(b["xs"], b["ilens"], b["olens"], b["ds"], b["es"], b["ps"], is_inference=False, want=want)
                    torch.cuda.synchronize()
                    names = [n for n, *_ in model.get_profile()]
                finally:
                    model.set_profiling(False)
        return {k: r[k] for k in want + ("d_log",)}, names
    finally:
        _lib.set_option("FS2_ROW8", -1)
        model.precision = "fp32"


def launch_names(model, b, precision, row8):
    return forward(model, b, precision, row8, profile=True)[1]


# ---- the cases of the call plan: id -> (model, precision, options, kind of forward).  tests/test_call_plan_host.py maps every id to the probe's case.
CALL_CASES = {}
for _prec in ("bf16x3", "mix_mx4"):
    for _v in (0, 1, 2):
        CALL_CASES["default/%s/tokproj%d" % (_prec, _v)] = ("default", _prec, {"FS2_TOKPROJ": _v}, "teacher")
CALL_CASES["default/bf16x3/fuse_var0"] = ("default", "bf16x3", {"FS2_FUSE_VAR": 0}, "teacher")
CALL_CASES["default/bf16x3/free_running"] = ("default", "bf16x3", {}, "free")
CALL_CASES["default/bf16x3/pitch_control"] = ("default", "bf16x3", {}, "control")
CALL_CASES["rf2/fp32/teacher"] = ("rf2", "fp32", {}, "teacher")
CALL_CASES["rf2/bf16x3/teacher"] = ("rf2", "bf16x3", {}, "teacher")
CALL_CASES["default/bf16x3/device_packed"] = ("default", "bf16x3", {}, "device_packed")
OPTION_DEFAULTS = {"FS2_TOKPROJ": 3, "FS2_FUSE_VAR": 1}


def make_rf2_model():
    """reduction_factor = 2, built as tests/test_oracle_golden.py's reduction_setup builds it (fixture G8)."""
    import math
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, bias_durations
    hp = default_hparams()
    hp.model.reduction_factor = 2
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(bias_durations(portable_state_dict(model.state_dict(), seed=23), math.log(1 + 3.0)))
    return model.to("cuda:0")


def device_capacity(b):
    """The capacities the device_packed case names: the frames of the batch and of its longest utterance (fs2_row_capacity makes rows of the first)."""
    return int(b["olens"].sum()), int(b["olens"].max())


def call_forward(model, b, case, profile=False):
    """One forward of a CALL_CASES entry -> (list of output tensors, ordered profile names or None).  The durations are always the batch's, so the frame counts
    are make_inputs()'s in every case; the options are restored afterwards."""
    import torch
    from fastspeech2_amd import _lib
    _, precision, options, kind = CALL_CASES[case]
    model.precision = precision
    for k, v in options.items():
        _lib.set_option(k, v)

    def run():
        if kind == "teacher":
            r = model._run(b["xs"], b["ilens"], b["olens"], b["ds"], b["es"], b["ps"], is_inference=False, want=("before", "after", "e_outs", "p_outs"))
            return [r[k] for k in ("before", "after", "d_log", "e_outs", "p_outs")]
        if kind in ("free", "control"):
            pro = None
            if kind == "control":      # one factor per phoneme, the same ramp for every utterance
                T = b["xs"].shape[1]
                pro = {"pitch_scale": torch.linspace(0.8, 1.25, T, device=b["xs"].device).repeat(b["xs"].shape[0], 1).contiguous()}
            r = model._run(b["xs"], b["ilens"], is_inference=True, compat=False, want=("before", "after", "e_outs", "p_outs"), d_override=b["ds"], prosody=pro)
            return [r[k] for k in ("before", "after", "e_outs", "p_outs")]
        res = model.inference_batch(b["xs"], b["ilens"], d_override=b["ds"], packed=True, sync=False, capacity=device_capacity(b))
        assert res.ok(), "capacity overflow"
        return [res[0][: int(res[1].sum())], res[1]]

    try:
        with torch.no_grad():
            out, names = run(), None
            if profile:
                model.set_profiling(True)
                try:
                    out = run()
                    torch.cuda.synchronize()
                    names = [n for n, *_ in model.get_profile()]
                finally:
                    model.set_profiling(False)
        return out, names
    finally:
        for k in options:
            _lib.set_option(k, OPTION_DEFAULTS[k])
        model.precision = "fp32"


def call_launch_names(model, b, case):
    return call_forward(model, b, case, profile=True)[1]


# ---- the cases of the weight loader: id -> (configuration, precision, second load).  The configurations are tests/test_gpu_parity.py's VARIANTS of the same names
# (tests/test_weight_plan_host.py holds the two together).
LOAD_VARIANTS = {
    "linear_ffn": dict(positionwise_layer_type="linear", positionwise_conv_kernel_size=1),
    "no_batchnorm": dict(use_batch_norm=False),
    "conv_k3_ffn": dict(positionwise_conv_kernel_size=3, duration_predictor_layers=3),
    "aheads8": dict(aheads=8),
    "aheads4_pre_ln_concat": dict(aheads=4, decoder_normalize_before=True, decoder_concat_after=True),
    "ddim256_arch": dict(ddim=256, dunits=1024, elayers=2, dlayers=3, postnet_layers=3),
}
LOAD_MODES = ("fp32", "bf16x3", "mix_mx4")
LOAD_CASES = {"%s/%s/load" % (v, m): (v, m, False) for v in LOAD_VARIANTS for m in LOAD_MODES}
LOAD_CASES.update({"default/%s/reload" % m: ("default", m, True) for m in LOAD_MODES})


def make_load_model(variant):
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    hp = default_hparams()
    for k, v in LOAD_VARIANTS.get(variant, {}).items():
        hp.model[k] = v
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=3))
    return model.to("cuda:0")


def load_forward(model, b, case):
    """One teacher-forced forward of a LOAD_CASES entry -> list of output tensors; a reload case runs one forward, has the weights loaded again and runs the next."""
    _, precision, reload = LOAD_CASES[case]
    out, _ = forward(model, b, precision, 0)
    if reload:
        generation = model._weights_generation
        model.refresh_weights()
        out, _ = forward(model, b, precision, 0)
        assert model._weights_generation == generation + 1, "no second fs2_load_weights"
    return [out[k] for k in ("before", "after", "d_log", "e_outs", "p_outs")]


def digest(tensors):
    import torch
    h = hashlib.sha256()
    for t in tensors:
        torch.cuda.synchronize()
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package runs (default: this one)")
    ap.add_argument("--names", help="write {case: [profile names]} here")
    ap.add_argument("--call-names", help="write {case: [profile names]} of CALL_CASES here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import fastspeech2_amd
    print("# package:", os.path.dirname(os.path.abspath(fastspeech2_amd.__file__)))
    b = make_inputs()
    names = {}
    for block in BLOCKS:
        model = make_model(block)
        for precision in MODES:
            for row8 in (0, 1):
                out, names[case_id(block, precision, row8)] = forward(model, b, precision, row8, profile=bool(args.names))
                print(case_id(block, precision, row8), digest([out[k] for k in ("before", "after", "d_log", "e_outs", "p_outs")]), flush=True)
            if block == "default":      # the device-driven layout (no host read-back between encode and decode): free-running decisions, given durations
                model.precision = precision
                with torch.no_grad():
                    model.inference_batch(b["xs"], b["ilens"], d_override=b["ds"])
                    res = model.inference_batch(b["xs"], b["ilens"], d_override=b["ds"], sync=False)
                    ok = res.ok()
                model.precision = "fp32"
                print("%s/%s/device_layout" % (block, precision), digest([res[0], res[1]]) if ok else "capacity overflow", flush=True)
    call_names, models = {}, {"default": make_model("default"), "rf2": make_rf2_model()}
    for case in CALL_CASES:
        out, call_names[case] = call_forward(models[CALL_CASES[case][0]], b, case, profile=bool(args.call_names))
        print(case, digest(out), flush=True)
    load_models = {}
    for case in LOAD_CASES:
        variant = LOAD_CASES[case][0]
        if variant not in load_models:
            load_models = {variant: make_load_model(variant)}      # (one model at a time on the device)
        try:
            print(case, digest(load_forward(load_models[variant], b, case)), flush=True)
        except fastspeech2_amd._lib.Fs2LibraryError as e:      # (a refusal of the library is an answer too: the same one from both trees)
            print(case, "refused: %s" % e, flush=True)
    for path, what in ((args.names, names), (args.call_names, call_names)):
        if path:
            with open(path, "w") as f:
                json.dump(what, f, indent=0, sort_keys=True)
                f.write("\n")


if __name__ == "__main__":
    main()
