"""Multiply before expanding (FS2_TOKPROJ): the variance predictors' first convolution and the decoder input layer computed from token-level
products (tok.proj in fs2_encode; var.gather0 / dec.in.gather in fs2_decode) instead of once per frame on the length regulator's copies.

Option 3 (the default) against option 0 (the frame-level launches) and against the CPU oracle in float64, at the smallest shapes at which the gather
can go wrong: zero-duration tokens at both edges and next to each other, a one-frame utterance, frame rows that cross a 128-row tile, the gap rows
between two utterances, both frame layouts, teacher forcing.  Tolerances: the predictor outputs within tests/test_gpu_ops.py's GEMM_TOL["bf16x3"]
(5 x the measured error of the split-bf16 GEMMs) times max |reference|; the mel within the end-to-end bar MEL_TOL."""
import numpy as np
import pytest
import torch

from tests.test_gpu_ops import GEMM_TOL
from tests.test_gpu_parity import MEL_TOL

pytestmark = pytest.mark.gpu
PRED_TOL = GEMM_TOL["bf16x3"]
WANT = ("after", "e_outs", "p_outs", "qe", "qp", "lr_index")


@pytest.fixture(scope="module")
def env():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    from oracle import fs2_oracle as O
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    sd = portable_state_dict(model.state_dict(), seed=0)
    model.load_state_dict(sd)
    model = model.to("cuda:0")
    cfg = O.config_from_hp(hp, N_PHONEME_SYMBOLS, hp.audio.num_mels)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return model, sd64, cfg, O


_ORACLE = {}      # case name -> the float64 oracle's outputs: computed once, shared by the precisions


def _oracle(name, fn):
    if name not in _ORACLE:
        _ORACLE[name] = fn()
    return _ORACLE[name]


def _batch(rs, tlens, durations):
    """xs / ilens / ds of utterances with the given token counts and forced durations."""
    B, T = len(tlens), max(tlens)
    xs = torch.zeros(B, T, dtype=torch.long)
    ds = torch.zeros(B, T, dtype=torch.long)
    for b, t in enumerate(tlens):
        xs[b, :t] = torch.from_numpy(rs.randint(1, 68, size=t))
        ds[b, :t] = torch.as_tensor(durations[b], dtype=torch.long)
    return xs, torch.as_tensor(tlens, dtype=torch.long), ds


def _scaled(ds, alpha):
    """The length regulator's speed control on forced durations: round_half_even(float32(d) * alpha)."""
    if alpha == 1.0:
        return ds
    return torch.round(ds.float() * torch.tensor(alpha, dtype=torch.float32)).long()


def _both_options(fs2_option, run):
    """run() with FS2_TOKPROJ = 3 and = 0 (the fixture restores the default afterwards)."""
    out = {}
    for opt in (3, 0):
        fs2_option("FS2_TOKPROJ", opt)
        with torch.no_grad():
            out[opt] = run()
    fs2_option("FS2_TOKPROJ", 3)
    return out[3], out[0]


def _compare(tag, new, old, o, olens):
    """Integer outputs of option 3 equal option 0's; predictor outputs and mel of both against the float64 oracle."""
    ol = torch.as_tensor(olens).cpu()
    assert torch.equal(torch.as_tensor(new["olens"]).cpu(), torch.as_tensor(old["olens"]).cpu()) and torch.equal(torch.as_tensor(new["olens"]).cpu(), o["olens"])
    if "d_int" in new:
        assert torch.equal(new["d_int"], old["d_int"])
    for k in ("lr_index", "qe", "qp"):
        for i in range(len(ol)):
            L = int(ol[i])
            assert torch.equal(new[k][i, :L], old[k][i, :L]), (tag, k, i)
            assert bool((new[k][i, L:] == old[k][i, L:]).all()), (tag, k, i)
    for i in range(len(ol)):
        L = int(ol[i])
        assert torch.equal(new["lr_index"][i, :L].cpu().long(), o["lr_index"][i]), (tag, i)
    for r, which in ((new, "option 3"), (old, "option 0")):
        for k, tol in (("e_outs", PRED_TOL), ("p_outs", PRED_TOL), ("after", None)):
            worst, scale = 0.0, float(o[k].abs().max())
            for i in range(len(ol)):
                L = int(ol[i])
                worst = max(worst, float((r[k][i, :L].cpu().double() - o[k][i, :L]).abs().max()))
            bound = MEL_TOL if tol is None else tol * scale
            print("%s [%s] %s: max-abs vs float64 oracle %.2e (max |ref| %.2f, bound %.2e)" % (tag, which, k, worst, scale, bound))
            assert worst <= bound, (tag, which, k, worst, bound)


# ---- 1. edges: zero-duration tokens first, last and side by side; an utterance whose only non-zero token lasts one frame; a single-token utterance
EDGE_T = (1, 7, 19)
EDGE_D = ([3], [0, 0, 0, 1, 0, 0, 0], [0, 3, 1, 2, 0, 0, 9, 1, 1, 2, 3, 0, 9, 2, 1, 0, 3, 2, 0])


def _edge_batch():
    return _batch(np.random.RandomState(11), EDGE_T, EDGE_D)


@pytest.mark.parametrize("alpha", [1.0, 1.3])
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx"])
def test_edges_zero_durations_and_one_frame_utterances(env, fs2_option, precision, alpha):
    model, sd64, cfg, O = env
    xs, il, ds = _edge_batch()
    o = _oracle("edges%g" % alpha, lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=_scaled(ds, alpha)))
    model.precision = precision
    try:
        new, old = _both_options(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), alpha=alpha, want=WANT))
    finally:
        model.precision = "fp32"
    assert torch.equal(new["olens"], _scaled(ds, alpha).sum(1))
    _compare("edges alpha=%g %s" % (alpha, precision), new, old, o, new["olens"])


@pytest.mark.parametrize("opt", [1, 2])
def test_each_half_alone(env, fs2_option, opt):
    """FS2_TOKPROJ = 1 (the predictors' first layer only: the expanded rows are still built for the input layer) and = 2 (the input layer only:
    tok.proj sliced to its 384 columns) on the edge batch."""
    model, sd64, cfg, O = env
    xs, il, ds = _edge_batch()
    o = _oracle("edges1", lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=ds))
    model.precision = "bf16x3"
    try:
        out = {}
        for v in (opt, 0):
            fs2_option("FS2_TOKPROJ", v)
            with torch.no_grad():
                out[v] = model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT)
        fs2_option("FS2_TOKPROJ", 3)
    finally:
        model.precision = "fp32"
    _compare("edges FS2_TOKPROJ=%d" % opt, out[opt], out[0], o, out[opt]["olens"])
    same = "after" if opt == 1 else "e_outs"      # the half that is switched off is computed as with option 0 (equal buckets -> equal decoder input)
    assert torch.equal(out[opt][same], out[0][same])


# ---- 2. 130 + 33 frames: rows cross a 128-row tile, a gap sits between the utterances; both frame layouts
TILE_T = (20, 9)
TILE_D = ([7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6, 7, 6], [4, 3, 4, 3, 4, 4, 3, 4, 4])
TILE_D_OTHER = ([1, 0, 2, 9, 3, 0, 0, 1, 2, 3, 9, 9, 1, 1, 2, 0, 3, 3, 2, 1], TILE_D[1])


@pytest.mark.parametrize("layout", ["host", "device"])
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx"])
def test_tile_crossing_rows_and_gap_rows_in_both_layouts(env, fs2_option, precision, layout):
    model, sd64, cfg, O = env
    rs = np.random.RandomState(12)
    xs, il, ds = _batch(rs, TILE_T, TILE_D)
    _, _, ds2 = _batch(np.random.RandomState(12), TILE_T, TILE_D_OTHER)
    assert ds.sum(1).tolist() == [130, 33]
    o = _oracle("tile", lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=ds))
    cap = dict(capacity=(200, 144)) if layout == "device" else {}
    model.precision = precision
    try:
        new, old = _both_options(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT, **cap))
        with torch.no_grad():
            other = model._run(xs.cuda(), il, is_inference=True, d_override=ds2.cuda(), want=WANT, **cap)
    finally:
        model.precision = "fp32"
    if layout == "device":
        assert int(new["status"].cpu()[2]) == 0 and int(old["status"].cpu()[2]) == 0 and int(other["status"].cpu()[2]) == 0
    assert torch.as_tensor(new["olens"]).cpu().tolist() == [130, 33]
    _compare("tile %s %s" % (layout, precision), new, old, o, [130, 33])
    # the second utterance does not see the first one's durations
    for k in WANT:
        assert torch.equal(other[k][1, :33], new[k][1, :33]), k


# ---- 3. teacher-forced: ds, es and ps given; the bucket indices come from the targets
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx"])
def test_teacher_forced(env, fs2_option, precision):
    model, sd64, cfg, O = env
    from fastspeech2_amd.synthetic import make_batch
    b = make_batch("c2", B=2, tlens=[5, 11])
    o = _oracle("teacher", lambda: O.per_utterance_forward(sd64, cfg, b["xs"], b["ilens"], b["ds"], b["es"].double(), b["ps"].double()))
    model.precision = precision
    try:
        new, old = _both_options(fs2_option, lambda: model._run(b["xs"].cuda(), b["ilens"], b["olens"], b["ds"].cuda(), b["es"].cuda(), b["ps"].cuda(),
                                                                is_inference=False, want=WANT))
    finally:
        model.precision = "fp32"
    _compare("teacher %s" % precision, new, old, o, b["olens"])
    for i in range(2):
        L = int(b["olens"][i])
        assert torch.equal(new["qe"][i, :L].cpu().long(), o["qe"][i, :L]) and torch.equal(new["qp"][i, :L].cpu().long(), o["qp"][i, :L])


# ---- 4. inert where it must be: the fp32 mode, and a model without the decoder input layer
def test_fp32_never_takes_the_token_level_path(env, fs2_option):
    model, sd64, cfg, O = env
    xs, il, ds = _edge_batch()
    assert model.precision == "fp32"
    new, old = _both_options(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT + ("before",)))
    for k in WANT + ("before",):
        assert torch.equal(new[k], old[k]), k


def test_model_without_decoder_input_layer_runs_unchanged(fs2_option):
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    twin = FeedForwardTransformer(N_PHONEME_SYMBOLS, 80, default_hparams(), _script_twin=True).eval()
    twin.load_state_dict(portable_state_dict(twin.state_dict(), seed=5))
    twin = twin.to("cuda:0")
    twin.precision = "bf16x3"
    xs, il, ds = _edge_batch()
    new, old = _both_options(fs2_option, lambda: twin._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT))
    for k in WANT:
        assert torch.equal(new[k], old[k]), k
    assert torch.isfinite(new["after"]).all()


# ---- 5. launch sites
NEW_SITES = {"tok.proj", "var.gather0", "dec.in.gather", "lr.index"}
# The frame-level first layer of the fused predictors is the two launches energy.conv0 / pitch.conv0 in the row-complete regime (what c3 runs; forced here with
# FS2_ROW8 = 1) and one stacked launch, var.conv0, below it (FS2_ROW8 = 0: what this shape would pick by itself).
OLD_CONV0 = {1: {"energy.conv0", "pitch.conv0"}, 0: {"var.conv0"}}
OLD_SITES = {"var.embed", "dec.in", "lr.expand"}


@pytest.mark.parametrize("row8", [1, 0])
def test_launch_sites(env, fs2_option, row8):
    model, sd64, cfg, O = env
    xs, il, ds = _edge_batch()
    fs2_option("FS2_ROW8", row8)
    model.precision = "bf16x3"
    try:
        names, outs = {}, {}
        for opt in (3, 0):
            fs2_option("FS2_TOKPROJ", opt)
            with torch.no_grad():
                model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT)      # (creates the handle on first use)
                model.set_profiling(True)
                try:
                    outs[opt] = model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT)
                    torch.cuda.synchronize()
                    names[opt] = {n for n, *_ in model.get_profile()}
                finally:
                    model.set_profiling(False)
        fs2_option("FS2_TOKPROJ", 3)
    finally:
        model.precision = "fp32"
    every_conv0 = OLD_CONV0[0] | OLD_CONV0[1]
    assert NEW_SITES <= names[3] and not (names[3] & (OLD_SITES | every_conv0)), sorted(names[3])
    assert (OLD_SITES | OLD_CONV0[row8]) <= names[0] and not (names[0] & NEW_SITES), sorted(names[0])
    # the replacement of the regime's own kernels computes the same thing
    o = _oracle("edges1", lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=ds))
    _compare("sites row8=%d" % row8, outs[3], outs[0], o, outs[3]["olens"])


# ---- 6. padded-batch semantics: the frames behind an utterance's end are stored rows (row_pos >= 0) without a token (lr_index -1); both gathers
#         then add nothing for them, as the zero rows of the expanded tensor did
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx"])
def test_padded_batch_semantics_rows_without_a_token(env, fs2_option, precision):
    model, sd64, cfg, O = env
    xs, il, ds = _batch(np.random.RandomState(13), (4, 9), ([2, 0, 1, 3], [3, 1, 0, 2, 9, 1, 2, 0, 3]))
    assert ds.sum(1).tolist() == [6, 21]
    o = _oracle("padded", lambda: O.padded_forward(sd64, cfg, xs, il, is_inference=True, d_override=ds))
    model.precision = precision
    try:
        new, old = _both_options(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, compat=True, d_override=ds.cuda(), want=WANT))
    finally:
        model.precision = "fp32"
    assert new["olens"].tolist() == [6, 21] and old["olens"].tolist() == [6, 21]
    for k in ("qe", "qp", "lr_index"):
        assert torch.equal(new[k], old[k]), k
    assert new["lr_index"][0, 6:].tolist() == [-1] * 15
    for r, which in ((new, "option 3"), (old, "option 0")):
        for k in ("e_outs", "p_outs", "after"):      # every stored row, the 15 token-less ones of the first utterance included
            worst, scale = float((r[k].cpu().double() - o[k]).abs().max()), float(o[k].abs().max())
            bound = MEL_TOL if k == "after" else PRED_TOL * scale
            print("padded %s [%s] %s: max-abs vs float64 oracle %.2e (max |ref| %.2f, bound %.2e)" % (precision, which, k, worst, scale, bound))
            assert worst <= bound, (which, k, worst, bound)
