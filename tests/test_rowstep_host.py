"""CPU checks of tests/rowstep_raw.py, the helper of the kernel-level tests of the row steps (tests/test_gpu_rowstep_kernels.py): all of them must pass before a launch
is sent to a GPU.

(a) the ctypes mirrors of TokGatherArgs, ShortLayoutArgs and RowStepArgs against csrc/row_step_args.h as the host compiler lays them out (tests/rowstep_raw_probe.cpp),
    the step names against the FS2_ROW_STEP_* enumerators; the hook's refusals, which launch nothing and so need no GPU;
(b) the numpy references against oracle/fs2_oracle.py wherever it states the same operation (integers equal, floats to 1e-12);
(c) the gather formulation is the model's: var_gather0's reference equals a 3-tap convolution over the expanded rows, dec_in_gather's a Linear over
    expanded + Tp[qp] + Te[qe], in float64 to 1e-10;
(d) the CPU figures behind the bars (recorded >= computed, <= 1.25 x computed) and the condition that the bars sit at or below a tenth of the model-level bar;
(e) DISCRIMINATION: every mutant at 8 bars or more from the reference on at least one case;
(f) the NaN plants and the trap behind R are there and reach no output of a reference; every gap row carries the index -1."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib
from oracle import fs2_oracle as O
from tests import rowstep_raw as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rowstep_raw") / "probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "rowstep_raw_probe.cpp"), "-o", exe], check=True)
    return lambda *args: [l.split() for l in subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip().split("\n")]


@pytest.mark.parametrize("mode,mirror", [("tok", W.TokGatherArgs), ("short", W.ShortLayoutArgs), ("flat", W.RowStepArgs)])
def test_argument_block_mirrors_match_the_compiled_header(probe, mode, mirror):
    lines = probe(mode)
    assert lines[0] == ["sizeof", str(ctypes.sizeof(mirror))]
    assert [l[0] for l in lines[1:]] == [f[0] for f in mirror._fields_]
    for name, off in lines[1:]:
        assert getattr(mirror, name).offset == int(off), name
    last = mirror._fields_[-1][0]
    assert ctypes.sizeof(mirror) - getattr(mirror, last).offset - getattr(mirror, last).size < 8


def test_step_names_follow_the_enumerators(probe):
    lines = probe("steps")
    assert [(int(v), n) for v, n in lines[:-1]] == list(enumerate(W.STEPS)) and lines[-1] == ["count", str(len(W.STEPS))]
    assert tuple(_lib.ROW_STEPS) == W.STEPS


def test_hook_refuses_before_anything_is_launched():
    """A NULL block, an unknown step and a size that is not the step's block's return FS2_ERR_ARG; nothing is launched (no GPU is needed to see it)."""
    _lib.build()
    L = _lib.lib()
    hook = L.fs2_op_launch_row_step
    for i, step in enumerate(W.STEPS):
        blk = W.BLOCK_OF.get(step, W.RowStepArgs)()
        n = ctypes.sizeof(blk)
        assert hook(None, i, None, n) == -1 and b"null" in L.fs2_last_error(None)
        for size in (n - 8, n + 8, 0):
            assert hook(None, i, ctypes.byref(blk), size) == -1 and b"bytes" in L.fs2_last_error(None), (step, size)
    blk = W.RowStepArgs()
    for step in (-1, len(W.STEPS), 1000):
        assert hook(None, step, ctypes.byref(blk), ctypes.sizeof(blk)) == -1 and b"unknown step" in L.fs2_last_error(None)
    assert len({ctypes.sizeof(b) for b in (W.TokGatherArgs, W.ShortLayoutArgs, W.RowStepArgs)}) == 3      # (a block of another step never has the right size)


# ------------------------------------------------------------------ (b) the pin to the oracle
def test_references_agree_with_the_oracle():
    bt = W.batch()
    ds = torch.from_numpy(bt.ds)
    for b, T in enumerate(bt.ilens):
        rows = slice(bt.start[b], bt.start[b] + bt.vlen[b])
        assert bt.lri[rows].tolist() == O.lr_indices(ds[b, :T]).tolist(), b
    hs = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, size=(bt.B, bt.Tmax, 8)))
    packed = np.zeros((bt.Rtok, 8))
    for b, T in enumerate(bt.ilens):
        packed[bt.tok_start[b]:bt.tok_start[b] + T] = hs[b, :T].numpy()
    out, olens, _ = O.length_regulate(hs, ds, torch.tensor(bt.ilens))
    mine = W.ref_lr_expand(bt, packed)
    assert olens.tolist() == bt.vlen
    for b in range(bt.B):
        assert np.array_equal(mine[bt.start[b]:bt.start[b] + bt.vlen[b]], out[b, :bt.vlen[b]].numpy())
    ops = W.operands(*W.WIDTHS[0])
    for vals, bins in ((ops.se, ops.ebins), (ops.sp, ops.pbins)):
        v = vals[bt.short["srow_pos"] >= 0]
        assert [W.bucket(x, bins) for x in v] == O.bucketize(torch.from_numpy(v), torch.from_numpy(bins)).tolist()
    du = W.DurOperands()
    for b in range(du.B):
        assert du.d_int[b, :du.ilens[b]].tolist() == O.duration_from_log(torch.from_numpy(du.y[b]).double()).tolist()
    # embed: E[xs] + alpha pe (use_scaled_pos_enc) and E[xs] sqrt(D) + pe, through the oracle's _add_pos on float64 rows
    D, idim = 16, 11
    rs = np.random.RandomState(2)
    E, xs = rs.uniform(-1, 1, size=(idim, D)).astype(np.float32), rs.randint(0, idim, size=(bt.B, bt.Tmax)).astype(np.int64)
    pe = O.positional_table(bt.Tmax, D).numpy()
    x = torch.from_numpy(E.astype(np.float64))[torch.from_numpy(xs)]
    for scaled, xsc, alpha in ((True, 1.0, 0.75), (False, float(np.sqrt(D)), 1.0)):
        want = O._add_pos({"p.alpha": torch.tensor([alpha], dtype=torch.float64)}, "p", x, dict(use_scaled_pos_enc=scaled)).numpy()
        got, _ = W.ref_embed(bt, xs, E, pe, idim, x_scale=xsc, alpha=alpha)
        for b, T in enumerate(bt.ilens):
            assert np.abs(got[bt.tok_start[b]:bt.tok_start[b] + T] - want[b, :T]).max() <= 1e-12


# ------------------------------------------------------------------ (c) the second route
def _layer_norm(y, g, b, eps):
    m = y.mean(-1, keepdims=True)
    return (y - m) / np.sqrt(((y - m) ** 2).mean(-1, keepdims=True) + eps) * g + b


@pytest.mark.parametrize("chans,D", W.WIDTHS[:2])
def test_gather_formulation_is_the_models(chans, D):
    """P = H W^T per tap and for the input layer, TP = Tp W^T + b, TE = Te W^T in float64: the references on these products equal the frame-level convolution and
    Linear over the expanded rows."""
    ops, bt = copy.copy(W.operands(chans, D)), W.batch()
    rs, A, N = np.random.RandomState(chans), 16, chans
    H = rs.uniform(-1, 1, size=(bt.Rtok, A))
    Wc, Wd, bd = rs.uniform(-1, 1, size=(3, 2 * N, A)), rs.uniform(-1, 1, size=(D, A)), rs.uniform(-1, 1, size=D)
    Te, Tp = rs.uniform(-1, 1, size=(W.NB + 1, A)), rs.uniform(-1, 1, size=(W.NB + 1, A))
    P = np.concatenate([H @ Wc[d].T for d in range(3)] + [H @ Wd.T], axis=1)
    P[bt.dead_tok] = W.NAN
    ops.P, ops.TP, ops.TE = P, Tp @ Wd.T + bd, Te @ Wd.T
    X = np.zeros((bt.R + 2, A))                                        # the expanded rows, one zero row on either side
    live = bt.row_pos[:bt.R] >= 0
    for row in range(bt.R):
        if bt.lri[row] >= 0:
            X[row + 1] = H[bt.tok_start[bt.row_seq[row]] + bt.lri[row]]
    bias, g, b = (t.astype(np.float64) for t in (ops.bias, ops.ln_g, ops.ln_b))
    y = np.maximum(sum(X[d:d + bt.R] @ Wc[d].T for d in range(3)) + bias, 0.0)
    conv = np.concatenate([_layer_norm(y[:, k * N:(k + 1) * N], g[k * N:(k + 1) * N], b[k * N:(k + 1) * N], W.EPS_VAR) for k in range(2)], axis=1)
    conv[~live] = 0.0
    assert np.abs(W.ref_var_gather0(ops) - conv).max() <= 1e-10
    got, qe, qp = W.ref_dec_in_gather(ops)
    lin = (X[1:-1] + Tp[np.maximum(qp, 0)] + Te[np.maximum(qe, 0)]) @ Wd.T + bd
    x = np.maximum(_layer_norm(lin, ops.ln_g2.astype(np.float64), ops.ln_b2.astype(np.float64), W.EPS_DEC), 0.0) * W.X_SCALE
    x = x + W.PE_ALPHA * ops.pe.astype(np.float64)[np.maximum(bt.row_pos[:bt.R], 0)]
    x[~live] = 0.0
    assert np.abs(got - x).max() <= 1e-10


# ------------------------------------------------------------------ (d) the figures and the bars
_refs = {}


def _ref(step, chans, D, route="rows"):
    key = (step, chans, D, route)
    if key not in _refs:
        ops = W.operands(chans, D)
        _refs[key] = W.ref_var_gather0(ops) if step == "var_gather0" else W.ref_dec_in_gather(ops, route)[0]
    return _refs[key]


@pytest.mark.parametrize("chans,D", W.WIDTHS)
def test_cpu_figures_are_reproduced_and_the_bars_see_more_than_the_model_tests(chans, D):
    ops = W.operands(chans, D)
    fig = {("var_gather0", chans): float(np.abs(W.var_gather0_fp32(ops) - _ref("var_gather0", chans, D)).max()),
           ("dec_in_gather", D): max(float(np.abs(W.dec_in_gather_fp32(ops, r) - _ref("dec_in_gather", chans, D, r)).max()) for r in ("rows", "teacher"))}
    for key, computed in fig.items():
        print(key, "computed %.4e recorded %.4e" % (computed, W.CPU_FIGURE[key]))
        assert computed <= W.CPU_FIGURE[key] <= 1.25 * computed, (key, computed)
        ref = _ref(key[0], chans, D)
        assert W.BAR[key] == 8 * W.CPU_FIGURE[key] and W.BAR[key] <= 0.1 * W.PRED_TOL * float(np.abs(ref).max()), key


# ------------------------------------------------------------------ (e) discrimination
def _bars_cleared(step, key, ref, mut, planes):
    bar = W.planes_bar(key, ref) if planes else np.full(ref.shape, W.BAR[key])
    err = np.abs(mut - ref)
    err[np.isnan(err)] = np.inf                                          # a mutant that read a planted NaN is as wrong as can be
    return float((err / bar).max())


@pytest.mark.parametrize("step,mutant", [(s, m) for s in ("var_gather0", "dec_in_gather") for m in W.MUTANTS[s]])
def test_every_mutant_clears_its_bar_by_8(step, mutant):
    """var_gather0 leaves planes only, so its bar carries the planes' rounding; dec_in_gather is held on its fp32 rows, the dropped lo plane on its planes."""
    best = {}
    for chans, D in W.WIDTHS:
        ops = W.operands(chans, D)
        key = (step, chans if step == "var_gather0" else D)
        mut = W.ref_var_gather0(ops, mutant) if step == "var_gather0" else W.ref_dec_in_gather(ops, "rows", mutant)[0]
        best[key] = _bars_cleared(step, key, _ref(step, chans, D), mut, planes=step == "var_gather0" or mutant == "lo_plane_dropped")
    print(step, mutant, {k: "%.3g" % v for k, v in best.items()})
    assert max(best.values()) >= 8, best


def test_ln_bias_exactly_where_the_relu_kills_the_row():
    bt = W.batch()
    for chans, D in W.WIDTHS:
        ops, ref = W.operands(chans, D), _ref("var_gather0", chans, D)
        rows = slice(bt.start[W.Batch.KILLED], bt.start[W.Batch.KILLED] + bt.len[W.Batch.KILLED])
        assert np.array_equal(ref[rows], np.broadcast_to(ops.ln_b.astype(np.float64), ref[rows].shape))
        assert np.array_equal(W.var_gather0_fp32(ops)[rows], ref[rows])


# ------------------------------------------------------------------ (f) plants, trap, gaps
def test_plants_are_there_and_reach_no_reference_output():
    bt = W.batch()
    assert bt.R % 4 and 200 <= sum(bt.len) <= 400
    gaps = bt.row_pos[:bt.R] < 0
    assert gaps[:bt.start[0]].all() and all(gaps[bt.start[b] + bt.len[b]:bt.start[b + 1]].all() and bt.start[b + 1] - bt.start[b] - bt.len[b] >= W.GAP for b in range(bt.B - 1))
    assert (bt.lri[gaps] == -1).all() and (bt.short["f2s"][gaps] == -1).all()          # neighbour_across_gap: the reference index carries -1 on every gap row
    extra = slice(bt.start[0] + bt.vlen[0], bt.start[0] + bt.len[0])
    assert (bt.row_pos[extra] >= 0).all() and (bt.lri[extra] == -1).all()               # frame rows with no token
    assert bt.row_pos[bt.R] >= 0 and bt.lri_in[bt.R] >= 0 and bt.dead_tok[bt.tok_start[bt.row_seq[bt.R]] + bt.lri_in[bt.R]]      # the trap
    for chans, D in W.WIDTHS:
        ops = W.operands(chans, D)
        assert np.isnan(ops.P[bt.dead_tok]).all() and bt.dead_tok.sum() > 20 and np.isnan(ops.P[bt.tok_start[1] + 2]).all()
        assert np.isnan(ops.pe[bt.Lmax:]).all() and np.isnan(ops.e_rows[:bt.R][gaps]).all() and np.isnan(ops.p_rows[bt.R:]).all()
        assert np.isnan(ops.es[bt.B * ops.es_stride:]).all() and np.isnan(ops.es[bt.len[0]:ops.es_stride]).all() and np.isnan(ops.ps[bt.B * ops.ps_stride:]).all()
        assert np.isnan(ops.TE[10]).all() and np.isnan(ops.TP[12]).all()
        assert ops.f2s[ops.forced] == -1 and bt.short["f2s"][ops.forced] >= 0 and bt.row_pos[ops.forced] >= 0
        qe, qp = ops.q["rows"]
        assert W.NB in qe and W.NB in qp and 0 in qe and 0 in qp                        # NaN / above the last bin, below the first
        qr = ops.search(ops.e_rows, ops.p_rows, right=True)
        assert (qr[0] != qe).sum() >= 3 and (qr[1] != qp).sum() >= 3                    # values exactly on an edge
        assert any(bt.row_pos[r] >= ops.es_stride for r in range(bt.R))                 # teacher forcing reads 0 behind the stride
        for route in ("rows", "teacher"):
            assert np.isfinite(_ref("dec_in_gather", chans, D, route)).all()
        assert np.isfinite(_ref("var_gather0", chans, D)).all()
        # variance of the quiet utterance's pre-LayerNorm rows: about 1e-2
        row = bt.start[W.Batch.QUIET] + 5
        y = (ops.P[bt.tok_start[W.Batch.QUIET] + bt.lri[row], ops.col0:].astype(np.float64) + ops.TP[qp[row]]) + ops.TE[qe[row]]
        assert 2e-3 < y.var() < 3e-2


def test_duration_operands_cover_the_cases_of_the_scan():
    du = W.DurOperands()
    assert du.ilens[:5] == [1, 255, 256, 257, 300] and du.Tmax == 300
    for alpha in du.ALPHAS:
        e = du.expected(du.ds, alpha)
        assert e["olens"][8] == e["olens"][9] == -1 and e["olens"][6] == 7 and e["used"][6] == [1] * 7
        assert all(e["so"][b] == sum(min(d, W.K_SHORT) for d in e["used"][b]) for b in range(du.B))
    half = [np.float32(d) * np.float32(0.5) for d in du.ds[1, :255] if d > 0]
    assert any(h % 1 == 0.5 and int(np.rint(h)) % 2 == 0 for h in half) and W.scaled_duration(5, 0.5) == 2 and W.scaled_duration(3, 0.5) == 2 and W.scaled_duration(1, 0.5) == 0
    assert du.expected(du.ds, 1.0)["used"][7][3] == 0 and du.ds[7, 3] < 0
    # exp(y) - 1 stays at least 1e-3 from a half-integer (here: 0.19), in float64 and with an fp32 exponential's error
    for y in du.y:
        v = np.exp(y.astype(np.float64)) - 1.0
        assert (np.abs(v - np.floor(v) - 0.5) > 0.19).all()
