"""Variance predictors on at most five frames per phoneme (FS2_VARSHORT): the fused pitch / energy predictors, the prosody control and the bucket
search of the predictions run on the SHORT rows -- min(d, 5) frames of every phoneme (csrc/layout_rule.h: vs_*; tests/test_varshort_host.py) --
and every frame reads its values through the frame-to-short map.

Option 1 (the default) against option 0 (the frame-level launches) and against the CPU oracle in float64, in the style of tests/test_gpu_tokproj.py,
whose tolerances these are (PRED_TOL x max |reference| on the predictor outputs, MEL_TOL on the mel).  With FS2_ROW8 = 1 the same gemm_row8c_bf16
serves var.conv1 at both row counts and every row sees the same values in the same order: the outputs are then equal bit for bit.  Shapes: the
smallest at which the map can go wrong -- durations 0 .. 7, 12 and 40, zero-duration phonemes first, last and between two long ones, a one-token
utterance, one of all ones, one of all long phonemes; short rows that cross a 128-row tile with gap rows behind them; both frame layouts."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import MEL_TOL
from tests.test_gpu_tokproj import PRED_TOL, _batch, _compare, _scaled

pytestmark = pytest.mark.gpu
WANT = ("after", "e_outs", "p_outs", "qe", "qp", "lr_index")
EQUAL = WANT + ("olens",)
K = 5


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


_ORACLE = {}      # case name -> the float64 oracle's outputs: computed once, shared by precisions and layouts


def _oracle(name, fn):
    if name not in _ORACLE:
        _ORACLE[name] = fn()
    return _ORACLE[name]


def _row_kernels(fs2_option, precision):
    """The row-complete kernels at these small sizes: gemm_row8c_bf16 then serves var.conv1 whatever the row count (and the fp4 conv of mix_mx4 runs)."""
    fs2_option("FS2_ROW8", 1)
    if precision == "mix_mx4":
        fs2_option("FS2_QKV8", 1)


def _both(fs2_option, run):
    """run() with FS2_VARSHORT = 1 and = 0 (the fixture restores the default afterwards)."""
    out = {}
    for opt in (1, 0):
        fs2_option("FS2_VARSHORT", opt)
        with torch.no_grad():
            out[opt] = run()
    fs2_option("FS2_VARSHORT", 1)
    return out[1], out[0]


def _assert_equal(tag, new, old, keys=EQUAL):
    for k in keys:
        assert torch.equal(torch.as_tensor(new[k]).cpu(), torch.as_tensor(old[k]).cpu()), (tag, k)


# ---- 1. the edges of the map.  0 first, last and between two long phonemes (12, 0, 40); every duration 0 .. 7, 12, 40
EDGE_T = (1, 9, 5, 16)
EDGE_D = ([6], [1] * 9, [12, 40, 7, 6, 12], [0, 12, 0, 40, 1, 2, 3, 4, 5, 6, 7, 0, 0, 9, 3, 0])


def _edge_batch():
    return _batch(np.random.RandomState(21), EDGE_T, EDGE_D)


@pytest.mark.parametrize("alpha", [1.0, 1.3])
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx4"])
def test_forced_durations_at_the_edges_of_the_map(env, fs2_option, precision, alpha):
    model, sd64, cfg, O = env
    xs, il, ds = _edge_batch()
    o = _oracle("edges%g" % alpha, lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=_scaled(ds, alpha)))
    _row_kernels(fs2_option, precision)
    model.precision = precision
    try:
        new, old = _both(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), alpha=alpha, want=WANT))
    finally:
        model.precision = "fp32"
    assert torch.equal(new["olens"], _scaled(ds, alpha).sum(1))
    _assert_equal("edges alpha=%g %s" % (alpha, precision), new, old)
    _compare("varshort edges alpha=%g %s" % (alpha, precision), new, old, o, new["olens"])


# ---- 2. tiling: 30 phonemes x 5 short frames = 150 short rows cross a 128-row tile (236 frames cross one too); a second utterance behind the gap rows
TILE_T = (30, 9)
TILE_D = ([6, 7, 12, 9, 8, 6, 7, 6, 9, 8] * 3, [4, 3, 9, 3, 4, 7, 3, 4, 6])


@pytest.mark.parametrize("layout", ["host", "device"])
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx4"])
def test_short_rows_cross_a_tile_and_gap_rows_in_both_layouts(env, fs2_option, precision, layout):
    model, sd64, cfg, O = env
    xs, il, ds = _batch(np.random.RandomState(22), TILE_T, TILE_D)
    frames = ds.sum(1).tolist()
    assert frames == [234, 43] and sum(min(d, K) for d in TILE_D[0]) == 150 > 128
    o = _oracle("tile", lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=ds))
    cap = dict(capacity=(320, 256)) if layout == "device" else {}
    _row_kernels(fs2_option, precision)
    model.precision = precision
    try:
        new, old = _both(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT, **cap))
    finally:
        model.precision = "fp32"
    if layout == "device":
        assert int(new["status"].cpu()[2]) == 0 and int(old["status"].cpu()[2]) == 0
    assert torch.as_tensor(new["olens"]).cpu().tolist() == frames
    for k in EQUAL:      # (the device-driven outputs are padded to the capacity: compared over the valid frames and behind them)
        assert torch.equal(torch.as_tensor(new[k]).cpu(), torch.as_tensor(old[k]).cpu()), (layout, precision, k)
    _compare("varshort tile %s %s" % (layout, precision), new, old, o, frames)


# ---- 3. different kernels for the two row counts: the regime of a batch of 2500 phonemes in 8 utterances puts the frame rows (8 per phoneme: 158 tiles)
#         on gemm_row8c_bf16 and the short rows (5 per phoneme: 99 tiles) on the tile kernel + ln_rows -- each against the oracle
def test_different_kernels_for_the_two_row_counts(env, fs2_option):
    model, sd64, cfg, O = env
    xs, il, ds = _edge_batch()
    o = _oracle("edges1", lambda: O.per_utterance_forward(sd64, cfg, xs, il, is_inference=True, d_override=ds))
    model.precision = "bf16x3"
    try:
        sites = {}

        def run(opt):
            def go():
                model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT, regime=(2500, 8))
                model.set_profiling(True)
                try:
                    r = model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT, regime=(2500, 8))
                    torch.cuda.synchronize()
                    sites[opt] = [n for n, *_ in model.get_profile()]
                finally:
                    model.set_profiling(False)
                return r
            return go
        out = {}
        for opt in (1, 0):
            fs2_option("FS2_VARSHORT", opt)
            with torch.no_grad():
                out[opt] = run(opt)()
        fs2_option("FS2_VARSHORT", 1)
    finally:
        model.precision = "fp32"
    # (launch_gemm names the row pass of a tile-kernel launch "<name>.rows": the row-complete kernel has none)
    assert "var.conv1.rows" in sites[1] and "var.conv1.rows" not in sites[0] and "var.conv1" in sites[0], (sites[1], sites[0])
    _compare("varshort other kernel", out[1], out[0], o, out[1]["olens"])
    for k, q in (("e_outs", "qe"), ("p_outs", "qp")):      # equal predictions -> equal integer outputs
        same = out[1][k] == out[0][k]
        assert torch.equal(out[1][q][same], out[0][q][same]), q


# ---- 4. teacher forcing: the buckets come from the given values, per frame; the predictions still come back for every frame
@pytest.mark.parametrize("precision", ["bf16x3", "mix_mx4"])
def test_teacher_forced(env, fs2_option, precision):
    model, sd64, cfg, O = env
    from fastspeech2_amd.synthetic import make_batch
    b = make_batch("c2", B=2, tlens=[5, 11])
    o = _oracle("teacher", lambda: O.per_utterance_forward(sd64, cfg, b["xs"], b["ilens"], b["ds"], b["es"].double(), b["ps"].double()))
    _row_kernels(fs2_option, precision)
    model.precision = precision
    try:
        new, old = _both(fs2_option, lambda: model._run(b["xs"].cuda(), b["ilens"], b["olens"], b["ds"].cuda(), b["es"].cuda(), b["ps"].cuda(),
                                                        is_inference=False, want=WANT))
    finally:
        model.precision = "fp32"
    _assert_equal("teacher %s" % precision, new, old, WANT)
    _compare("varshort teacher %s" % precision, new, old, o, b["olens"])
    for i in range(2):
        L = int(b["olens"][i])
        assert torch.equal(new["qe"][i, :L].cpu().long(), o["qe"][i, :L]) and torch.equal(new["qp"][i, :L].cpu().long(), o["qp"][i, :L])


# ---- 5. control, per utterance and per phoneme: applied on the short rows, it is what it is per frame
@pytest.mark.parametrize("per", ["utterance", "phoneme"])
def test_prosody_control(env, fs2_option, per):
    model, _, _, _ = env
    xs, il, ds = _edge_batch()
    B, T = xs.shape
    rs = np.random.RandomState(23)
    cols = 1 if per == "utterance" else T
    pro = {"pitch_scale": torch.from_numpy(rs.uniform(0.7, 1.4, size=(B, cols)).astype(np.float32)).cuda(),
           "energy_shift": torch.from_numpy(rs.uniform(-0.5, 0.5, size=(B, cols)).astype(np.float32)).cuda()}
    _row_kernels(fs2_option, "bf16x3")
    model.precision = "bf16x3"
    try:
        new, old = _both(fs2_option, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT, prosody=pro))
        with torch.no_grad():
            plain = model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=WANT)
    finally:
        model.precision = "fp32"
    _assert_equal("control per %s" % per, new, old)
    assert not torch.equal(new["p_outs"], plain["p_outs"]) and not torch.equal(new["e_outs"], plain["e_outs"])      # the control acted


# ---- 6. launch sites
def _profile(model, run):
    with torch.no_grad():
        run()      # (creates the handle on first use)
        model.set_profiling(True)
        try:
            run()
            torch.cuda.synchronize()
            return model.get_profile()
        finally:
            model.set_profiling(False)


def _up(x, a):
    return -(-x // a) * a


def test_launch_sites_run_on_the_short_row_count(env, fs2_option):
    """var.gather0 and var.conv1 work on the short rows' bound (their flops / bytes are proportional to the rows), the list of launch sites is the
    frame-level one -- nothing is expanded when only `after` is wanted -- and the other sites keep their rows."""
    model, _, _, _ = env
    xs, il, ds = _batch(np.random.RandomState(22), TILE_T, TILE_D)
    _row_kernels(fs2_option, "bf16x3")
    model.precision = "bf16x3"
    try:
        prof = {}
        for opt in (1, 0):
            fs2_option("FS2_VARSHORT", opt)
            prof[opt] = _profile(model, lambda: model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=("after",)))
        fs2_option("FS2_VARSHORT", 1)
    finally:
        model.precision = "fp32"
    assert [n for n, *_ in prof[1]] == [n for n, *_ in prof[0]]
    # the rule restated: frame rows R of the gapped layout (gap 4: the 9-tap FFN), short rows min(row_bound(min(R, 5 x phonemes), B), R)
    frames, row = [sum(d) for d in TILE_D], 4
    for f in frames:
        row = _up(row, 8) + f + 4
    R = row + 8
    Rs = min(min(R, K * sum(TILE_T)) + 16 * len(TILE_T) + 8, R)
    assert Rs < R
    site = {opt: {n: (fl, by) for n, _, fl, by in prof[opt]} for opt in (1, 0)}
    assert site[0]["lr.index"][1] == 4.0 * R
    assert site[1]["var.conv1"][0] * R == site[0]["var.conv1"][0] * Rs and site[1]["var.gather0"][1] * R == site[0]["var.gather0"][1] * Rs
    for n in ("dec.in.gather", "dec.qkv", "feat_out"):
        assert site[1][n] == site[0][n], n


@pytest.mark.parametrize("case", ["compat_padded", "fp32", "unfused"])
def test_paths_that_keep_the_frame_level_sites(env, fs2_option, case):
    """Padded-batch semantics, fp32 and the unfused predictors: the option changes no launch, no row count and no output."""
    model, _, _, _ = env
    xs, il, ds = _edge_batch()
    if case == "unfused":
        fs2_option("FS2_FUSE_VAR", 0)
    model.precision = "fp32" if case == "fp32" else "bf16x3"
    try:
        prof, out = {}, {}
        for opt in (1, 0):
            fs2_option("FS2_VARSHORT", opt)
            run = lambda: model._run(xs.cuda(), il, is_inference=True, compat=(case == "compat_padded"), d_override=ds.cuda(), want=WANT)      # noqa: E731
            prof[opt] = [(n, fl, by) for n, _, fl, by in _profile(model, lambda: out.__setitem__(opt, run()))]
        fs2_option("FS2_VARSHORT", 1)
    finally:
        model.precision = "fp32"
    assert prof[1] == prof[0]
    names = {n for n, *_ in prof[1]}
    assert ("energy.conv1" in names) == (case != "compat_padded") and ("var.conv1" in names) == (case == "compat_padded")
    _assert_equal(case, out[1], out[0], WANT)


# ---- 7. graph capture: one replay equals the eager call
def test_graph_replay_equals_the_eager_call(env):
    model, _, _, _ = env
    xs, il, ds = _edge_batch()
    model.precision = "bf16x3"
    try:
        run = model.capture_graph(xs.cuda(), il, d_override=ds.cuda())
        after, olens_dev, status = run(xs.cuda())
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = model._run(xs.cuda(), il, is_inference=True, d_override=ds.cuda(), want=("after",))
    finally:
        model.precision = "fp32"
    assert int(status.cpu()[2]) == 0 and torch.equal(olens_dev.cpu().long(), eager["olens"].cpu().long())
    for i, L in enumerate(eager["olens"].tolist()):
        assert torch.equal(after[i, :L], eager["after"][i, :L]), i
    assert float(eager["after"].abs().max()) > 0 and MEL_TOL > 0 and PRED_TOL > 0
