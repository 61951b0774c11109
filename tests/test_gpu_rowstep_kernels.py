"""Kernel-level tests of the row steps between the GEMMs: embed_pe, dur_finalize + dur_scan, lr_index_only, lr_index_short, lr_expand, var_gather0, bucket_embed,
var_bucket_short + dec_in_gather, to_planes and planes_to_rows, each launched on the library itself through fs2_op_launch_row_step -- the function the model launches
the step with -- on the operands of tests/rowstep_raw.py: exact values, NaN wherever nothing may be read, live-looking entries behind R that point at NaN rows.

Every output buffer is preset to the sentinel 0xFF and carries a guard region.  For every step: finite values in the rows < R (no planted value was read), gap rows
exactly zero (-1 for the index outputs), nothing written behind the buffer.  Integer outputs are held bit for bit against numpy; rows a kernel only moves against the
source; planes against the split of the fp32 rows written with them; the routes of one step against each other.  embed_pe and bucket_embed are held to derived bars
(one or two fp32 roundings of exact operands), var_gather0 and dec_in_gather to 8 x the error of their arithmetic stated in fp32 on the CPU (rowstep_raw.BAR), measured
against the float64 reference; tests/test_rowstep_host.py holds every mutant at 8 bars or more."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_raw as G
from tests import rowstep_raw as W

pytestmark = pytest.mark.gpu

_state = {}


def _dev():
    """The device side of the module, once: the batch's integer arrays uploaded."""
    if "dev" not in _state:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        d, bt = W.Dev(), W.batch()
        i32 = lambda a: d.up(np.asarray(a, np.int32))
        m = dict(row_pos=i32(bt.row_pos), row_seq=i32(bt.row_seq), vlen=i32(bt.vlen), tok_start=i32(bt.tok_start), ilen=i32(bt.ilens), cum=i32(bt.cum_padded(bt.cum)),
                 scum=i32(bt.cum_padded(bt.scum)), so32=i32(bt.so), lri=i32(bt.lri_in), tok_pos=i32(bt.tok_pos), tok_seq=i32(bt.tok_seq),
                 srow_pos=i32(bt.short["srow_pos"]), alpha=d.up(np.array([W.PE_ALPHA], np.float32)))
        _state["dev"], _state["meta"] = d, m
    return _state["dev"], _state["meta"], W.batch()


def _ok(rc):
    from fastspeech2_amd import _lib
    _lib.check(rc)


def _ints(buf, n):
    return W.view(buf, torch.int32, n)


def _rows(buf, R, D):
    return W.view(buf, torch.float32, R * D).reshape(R, D)


def _plane_bits(buf, R, Cc):
    hi, lo = G.decode_planes(buf.cpu(), R, Cc)
    return hi.contiguous().view(torch.int16).numpy(), lo.contiguous().view(torch.int16).numpy()


def _plane_values(buf, R, Cc):
    return G.pair_value(*G.decode_planes(buf.cpu(), R, Cc)).numpy()


def _assert_rows(v, live, nbytes, buf, who):
    """finite in every row < R, exactly zero in the rows that are no frame, nothing behind the buffer"""
    assert np.isfinite(v).all(), "%s: a planted NaN was read, or a row < R was never written" % who
    assert not v[~live].any(), "%s: a gap row is not exactly zero" % who
    assert G.untouched(buf.cpu(), nbytes), "%s wrote behind its buffer" % who


def _assert_planes_are_split_of(pbuf, rows32, who):
    hi, lo = _plane_bits(pbuf, *rows32.shape)
    want_hi, want_lo = W.split_planes(rows32)
    assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo), "%s: the planes are not the split of the fp32 rows" % who


# ------------------------------------------------------------------ the index writers
def _index_results():
    if "index" not in _state:
        d, m, bt = _dev()
        sh, R = bt.short, bt.R
        out = {}
        a = W.RowStepArgs(row_pos=W.ptr(m["row_pos"]), row_seq=W.ptr(m["row_seq"]), R=R, vlen=W.ptr(m["vlen"]), B=bt.B, Tmax=bt.Tmax, D=128, cum_in=W.ptr(m["cum"]),
                          ilen=W.ptr(m["ilen"]), tok_start=W.ptr(m["tok_start"]))
        lri = d.out(4 * R)
        a.index_rows = W.ptr(lri)
        _ok(d.launch("lr_index", a))
        out["only"] = lri.cpu()
        names = dict(lri=R, f2s=R, sstart=bt.B, slen=bt.B, sdims=16, srow_pos=sh["Rs_pad"], srow_seq=sh["Rs_pad"], slri=sh["Rs_pad"])
        bufs = {k: d.out(4 * n) for k, n in names.items()}
        s = W.ShortLayoutArgs(cum=W.ptr(m["cum"]), scum=W.ptr(m["scum"]), Tmax=bt.Tmax, ilen=W.ptr(m["ilen"]), so32=W.ptr(m["so32"]), row_pos=W.ptr(m["row_pos"]),
                              row_seq=W.ptr(m["row_seq"]), vlen=W.ptr(m["vlen"]), R=R, ovf=None, B=bt.B, gap=W.GAP, K=W.K_SHORT, Rs=sh["Rs"], Rs_pad=sh["Rs_pad"],
                              **{k: W.ptr(b) for k, b in bufs.items()})
        _ok(d.launch("lr_index_short", s))
        out["short"] = {k: b.cpu() for k, b in bufs.items()}
        out["short_n"] = names
        _state["index"] = out
    return _state["index"]


def test_index_writers_agree_with_numpy_and_put_minus_one_on_every_gap_row():
    """lr_index_only and lr_index_short against the reference index (lr_expand's: test_lr_expand); the short layout against layout_rule.h's rule as
    tests/test_varshort_host.py states it.  var_gather0 takes a neighbour's token from lri[row +- 1]: every gap row must carry -1."""
    _, _, bt = _dev()
    res, sh, R = _index_results(), bt.short, bt.R
    gaps = bt.row_pos[:R] < 0
    for who, buf in (("lr_index_only", res["only"]), ("lr_index_short", res["short"]["lri"])):
        got = _ints(buf, R)
        assert np.array_equal(got, bt.lri), "%s: rows %s" % (who, np.nonzero(got != bt.lri)[0][:8])
        assert (got[gaps] == -1).all() and G.untouched(buf, 4 * R), who
    s, n = res["short"], res["short_n"]
    want = dict(f2s=sh["f2s"], sstart=sh["sstart"], slen=sh["slen"], srow_pos=sh["srow_pos"], srow_seq=sh["srow_seq"], slri=sh["slri"])
    for k, w in want.items():
        got = _ints(s[k], n[k])
        assert np.array_equal(got, np.asarray(w, np.int32)), "%s: entries %s" % (k, np.nonzero(got != np.asarray(w))[0][:8])
        assert G.untouched(s[k], 4 * n[k]), k
    assert _ints(s["sdims"], 1)[0] == sh["rows"] and G.untouched(s["sdims"], 4)
    assert (_ints(s["f2s"], R)[gaps] == -1).all()


@pytest.mark.parametrize("D", W.D_WIDTHS)
def test_lr_expand_moves_the_source_rows_bit_for_bit(D):
    d, m, bt = _dev()
    R = bt.R
    hs = W._u(np.random.RandomState(D), bt.Rtok, D)
    hs[bt.dead_tok] = W.NAN
    hsd = d.up(hs)
    runs = {}
    for planes in (False, True):
        rows, idx, pl = d.out(4 * R * D), d.out(4 * R), (d.out(4 * R * D) if planes else None)
        a = W.RowStepArgs(row_pos=W.ptr(m["row_pos"]), row_seq=W.ptr(m["row_seq"]), R=R, vlen=W.ptr(m["vlen"]), B=bt.B, Tmax=bt.Tmax, D=D, cum_in=W.ptr(m["cum"]),
                          ilen=W.ptr(m["ilen"]), tok_start=W.ptr(m["tok_start"]), src_rows=W.ptr(hsd), rows=W.ptr(rows), planes=W.ptr(pl), index_rows=W.ptr(idx))
        _ok(d.launch("lr_expand", a))
        runs[planes] = (rows, idx, pl)
    want = W.ref_lr_expand(bt, hs)
    for planes, (rows, idx, pl) in runs.items():
        v = _rows(rows, R, D)
        _assert_rows(v, bt.lri >= 0, 4 * R * D, rows, "lr_expand rows")
        assert np.array_equal(v.view(np.int32), want.view(np.int32)), "lr_expand: rows differ from the gathered source"
        got = _ints(idx, R)
        assert np.array_equal(got, bt.lri) and np.array_equal(got, _ints(_index_results()["only"], R)) and G.untouched(idx.cpu(), 4 * R)
        if planes:
            _assert_planes_are_split_of(pl, v, "lr_expand")
            assert G.untouched(pl.cpu(), 4 * R * D)


# ------------------------------------------------------------------ dur.post
def _dur_run(du, ds, alpha):
    d, _, _ = _dev()
    B, T = du.B, du.Tmax
    if "dur_in" not in _state:
        i32 = lambda a: d.up(np.asarray(a, np.int32))
        _state["dur_in"] = dict(start=i32(du.start), vlen=i32(du.ilens), dlog=d.up(du.dlog_rows), xs=d.up(du.xs))
    k = _state["dur_in"]
    sizes = dict(d_log=4 * B * T, d_int=8 * B * T, d_int2=8 * B * T, cum=4 * B * T, scum=4 * B * T, olens=8 * B, olens32=4 * B, so32=4 * B)
    out = {n: d.out(s) for n, s in sizes.items()}
    dsd = d.up(ds) if ds is not None else None
    a = W.RowStepArgs(start=W.ptr(k["start"]), vlen=W.ptr(k["vlen"]), B=B, Tmax=T, xs=W.ptr(k["xs"]), idim=du.idim, dlog_rows=W.ptr(k["dlog"]), ds=W.ptr(dsd), alpha=alpha,
                      K=W.K_SHORT, **{n: W.ptr(b) for n, b in out.items()})
    _ok(d.launch("dur_post", a))
    return {n: b.cpu() for n, b in out.items()}, sizes


def _assert_scan(du, got, sizes, want, who):
    B, T = du.B, du.Tmax
    for name in ("cum", "scum"):
        v = _ints(got[name], B * T).reshape(B, T)
        for b, n in enumerate(du.ilens):
            assert v[b, :n].tolist() == want[name][b], "%s: %s of utterance %d (%d tokens)" % (who, name, b, n)
            assert (v[b, n:] == -1).all(), "%s: %s written behind the %d tokens of utterance %d" % (who, name, n, b)
    assert W.view(got["olens"], torch.int64, B).tolist() == want["olens"], who
    assert _ints(got["olens32"], B).tolist() == want["olens"] and _ints(got["so32"], B).tolist() == want["so"], who
    for name, nbytes in sizes.items():
        assert G.untouched(got[name], nbytes), "%s wrote behind %s" % (who, name)


def test_dur_post_finalize_then_scan_of_its_own_durations():
    """ds == nullptr: the scan takes the durations dur_finalize just wrote.  Token counts 1, 255, 256, 257, 300 of Tmax = 300: the carry between the 256-token passes."""
    du = W.DurOperands()
    got, sizes = _dur_run(du, None, 1.0)
    B, T = du.B, du.Tmax
    assert np.array_equal(W.view(got["d_log"], torch.float32, B * T).view(np.int32), du.d_log.reshape(-1).view(np.int32)), "d_log is not the packed rows, zero behind"
    for name in ("d_int", "d_int2"):
        assert np.array_equal(W.view(got[name], torch.int64, B * T), du.d_int.reshape(-1)), name
    _assert_scan(du, got, sizes, du.expected(du.d_int, 1.0), "scan of d_int")


@pytest.mark.parametrize("alpha", W.DurOperands.ALPHAS)
def test_dur_scan_edges(alpha):
    """Teacher-forced durations: zeros at both edges and adjacent, an all-zero utterance (all ones), a negative duration, alpha 0.5 (ties to even) and 1.3, a bad id
    inside an utterance and one in the padding only (frame count -1), the K = 5 short sums; the finalize outputs are those of the log-durations all the same."""
    du = W.DurOperands()
    got, sizes = _dur_run(du, du.ds, alpha)
    _assert_scan(du, got, sizes, du.expected(du.ds, alpha), "alpha %g" % alpha)
    assert np.array_equal(W.view(got["d_int"], torch.int64, du.B * du.Tmax), du.d_int.reshape(-1))


HUGE = (2 ** 32 + 5, 2 ** 63 - 1, 2 ** 31, 2 ** 40)


@pytest.mark.parametrize("alpha", (1.0, 0.5))
def test_one_huge_duration_is_never_a_small_frame_count(alpha):
    """One duration beyond the int range beside ordinary ones: 2^32 + 5 (narrowed: 5), INT64_MAX (what duration_from_log saturates to; narrowed: -1), 2^31, 2^40.  The
    frame count of such an utterance is INT32_MAX in olens and olens32 -- which fs2_decode refuses (no positional table holds it) or flags (FS2_OVF_LMAX / _PE) --, never
    a wrapped count; so is the count of an utterance whose ordinary-looking durations sum beyond the range; the other utterances are untouched.  (scaled_duration
    used to narrow with a plain (int) and dur_scan to sum in int: 2^32 + 5 counted as 5 frames and INT64_MAX as -1, beside the d_int that told the caller otherwise.)"""
    du = W.DurOperands()
    ds = du.ds.copy()
    for b, huge in zip((1, 2, 3, 4), HUGE):
        ds[b, 7] = huge
    ds[5, :40] = 2 ** 27                                               # 40 x 2^27 = 5 x 2^30: every duration fits, the sum does not
    got, sizes = _dur_run(du, ds, alpha)
    want = du.expected(ds, alpha)
    B = du.B
    olens, o32 = W.view(got["olens"], torch.int64, B).tolist(), _ints(got["olens32"], B).tolist()
    assert olens == want["olens"] and o32 == want["olens"], (olens, o32)
    assert all(olens[b] == W.DUR_MAX for b in (1, 2, 4, 5)) and olens[3] == (W.DUR_MAX if alpha == 1.0 else 2 ** 30 + sum(want["used"][3]) - want["used"][3][7]) and 0 < olens[7] < 1000
    cum = _ints(got["cum"], B * du.Tmax).reshape(B, du.Tmax)
    for b in (0, 6, 7):
        assert cum[b, :du.ilens[b]].tolist() == want["cum"][b]
    for name, nbytes in sizes.items():
        assert G.untouched(got[name], nbytes), name


def test_a_saturated_log_duration_reaches_the_caller_as_such():
    """dur_finalize on y = 50 and +inf gives INT64_MAX (duration_from_log saturates); the scan of these durations gives the frame count INT32_MAX."""
    d, _, _ = _dev()
    du = W.DurOperands()
    dlog = du.dlog_rows.copy()
    dlog[du.start[5] + 3], dlog[du.start[7] + 1] = 50.0, np.inf
    keep = _state.pop("dur_in", None)
    try:
        _dur_run(du, None, 1.0)                                        # (fills the module's inputs)
        _state["dur_in"]["dlog"] = d.up(dlog)
        got, _ = _dur_run(du, None, 1.0)
    finally:
        _state.pop("dur_in", None)
        if keep is not None:
            _state["dur_in"] = keep
    d_int = W.view(got["d_int"], torch.int64, du.B * du.Tmax).reshape(du.B, du.Tmax)
    assert d_int[5, 3] == 2 ** 63 - 1 and d_int[7, 1] == 2 ** 63 - 1
    olens = W.view(got["olens"], torch.int64, du.B).tolist()
    assert olens[5] == olens[7] == W.DUR_MAX and _ints(got["olens32"], du.B).tolist() == olens


# ------------------------------------------------------------------ embed_pe, bucket_embed, planes
@pytest.mark.parametrize("D", W.D_WIDTHS)
def test_embed_pe(D):
    from tests.conftest import record_measurement
    from oracle import fs2_oracle as O
    d, m, bt = _dev()
    rs, idim, Rt = np.random.RandomState(100 + D), 12, bt.Rtok
    E = W._u(rs, idim, D)
    xs = rs.randint(0, idim - 2, size=(bt.B, bt.Tmax)).astype(np.int64)
    E[idim - 2:] = W.NAN                                               # table rows no id selects
    xs[1, 4], xs[3, 0] = idim + 5, -3                                  # ids outside [0, idim): row 0 is read
    for b, n in enumerate(bt.ilens):
        xs[b, n:] = idim - 1                                           # the padding names a NaN row: never embedded
    n_pe = max(bt.ilens)
    pe = np.full((n_pe + 8, D), W.NAN, np.float32)
    pe[:n_pe] = O.positional_table(n_pe, D).numpy()
    Ed, xsd, ped = d.up(E), d.up(xs), d.up(pe)
    ref, mag = W.ref_embed(bt, xs, E, pe, idim)
    live = bt.tok_pos[:Rt] >= 0
    runs = {}
    for planes in (False, True):
        rows, pl = d.out(4 * Rt * D), (d.out(4 * Rt * D) if planes else None)
        a = W.RowStepArgs(row_pos=W.ptr(m["tok_pos"]), row_seq=W.ptr(m["tok_seq"]), R=Rt, B=bt.B, Tmax=bt.Tmax, D=D, rows=W.ptr(rows), planes=W.ptr(pl), xs=W.ptr(xsd),
                          E=W.ptr(Ed), idim=idim, pe=W.ptr(ped), pe_alpha=W.ptr(m["alpha"]), x_scale=W.X_SCALE)
        _ok(d.launch("embed", a))
        runs[planes] = (rows, pl)
    v = _rows(runs[True][0], Rt, D)
    _assert_rows(v, live, 4 * Rt * D, runs[True][0], "embed_pe")
    bar = 3 * W.U24 * mag
    err = np.abs(v - ref)
    assert (err[live] <= bar[live]).all(), "embed_pe: %d elements beyond 3 x 2^-24 (|E x_scale| + |alpha pe|), worst %.3g bars" % ((err > bar).sum(), (err[live] / bar[live]).max())
    record_measurement("rowstep_embed_pe_D%d_error_to_bar" % D, float((err[live] / bar[live]).max()))
    assert torch.equal(runs[False][0].cpu(), runs[True][0].cpu()), "embed_pe: the rows written alone differ from the rows written with planes"
    _assert_planes_are_split_of(runs[True][1], v, "embed_pe")
    assert G.untouched(runs[True][1].cpu(), 4 * Rt * D)


@pytest.mark.parametrize("D", W.D_WIDTHS)
def test_bucket_embed(D):
    from tests.conftest import record_measurement
    d, m, bt = _dev()
    ops = W.operands(dict((dd, c) for c, dd in W.WIDTHS)[D], D)
    R = bt.R
    live = bt.row_pos[:R] >= 0
    h = W._u(np.random.RandomState(200 + D), R, D)
    h[bt.lri < 0] = 0.0                                                # as lr_expand leaves them
    dv = {k: d.up(getattr(ops, k)) for k in ("e_rows", "p_rows", "es", "ps", "ebins", "pbins", "TE", "TP")}
    worst = 0.0
    for route in ("rows", "teacher"):
        ref, mag, qe, qp = W.ref_bucket_embed(ops, h, ops.TE, ops.TP, route)
        runs = {}
        for planes in (False, True):
            rows, pl, qeb, qpb = d.out(4 * R * D), (d.out(4 * R * D) if planes else None), d.out(4 * R), d.out(4 * R)
            rows[:4 * R * D] = torch.from_numpy(h).view(torch.uint8).reshape(-1).to(rows.device)
            a = W.RowStepArgs(row_pos=W.ptr(m["row_pos"]), row_seq=W.ptr(m["row_seq"]), R=R, D=D, rows=W.ptr(rows), planes=W.ptr(pl), e_rows=W.ptr(dv["e_rows"]),
                              p_rows=W.ptr(dv["p_rows"]), ebins=W.ptr(dv["ebins"]), pbins=W.ptr(dv["pbins"]), nb=W.NB, Te=W.ptr(dv["TE"]), Tp=W.ptr(dv["TP"]),
                              qe_rows=W.ptr(qeb), qp_rows=W.ptr(qpb))
            if route == "teacher":
                a.es, a.ps, a.es_stride, a.ps_stride, a.e_rows, a.p_rows = W.ptr(dv["es"]), W.ptr(dv["ps"]), ops.es_stride, ops.ps_stride, None, None
            _ok(d.launch("var_embed", a))
            runs[planes] = (rows, pl, qeb, qpb)
        rows, pl, qeb, qpb = runs[True]
        v = _rows(rows, R, D)
        _assert_rows(v, live, 4 * R * D, rows, "bucket_embed " + route)
        for name, got, want in (("qe", qeb, qe), ("qp", qpb, qp)):
            assert np.array_equal(_ints(got, R), want) and G.untouched(got.cpu(), 4 * R), "bucket_embed %s: %s" % (route, name)
        bar, err = 3 * W.U24 * mag, np.abs(v - ref)
        assert (err[live] <= bar[live]).all(), "bucket_embed %s: %d elements beyond 3 x 2^-24 (|h| + |Tp| + |Te|)" % (route, (err > bar).sum())
        worst = max(worst, float((err[live] / np.maximum(bar[live], 1e-300)).max()))
        assert torch.equal(runs[False][0].cpu(), rows.cpu())
        _assert_planes_are_split_of(pl, v, "bucket_embed " + route)
        assert G.untouched(pl.cpu(), 4 * R * D)
    record_measurement("rowstep_bucket_embed_D%d_error_to_bar" % D, worst)


@pytest.mark.parametrize("D", W.D_WIDTHS)
def test_to_planes_then_planes_to_rows_is_hi_plus_lo(D):
    d, _, bt = _dev()
    R = bt.R
    x = W._u(np.random.RandomState(300 + D), R, D, scale=3.0)
    x[5, :6] = [0.0, -0.0, 1.0, -1.0, 1e-30, -7.0]
    xd, pl, back = d.up(x), d.out(4 * R * D), d.out(4 * R * D)
    _ok(d.launch("to_planes", W.RowStepArgs(R=R, D=D, rows=W.ptr(xd), planes=W.ptr(pl))))
    _ok(d.launch("planes_to_rows", W.RowStepArgs(R=R, D=D, rows=W.ptr(back), planes=W.ptr(pl))))
    _assert_planes_are_split_of(pl, x, "to_planes")
    hi, lo = G.split_bf16(torch.from_numpy(x))
    want = (hi.float() + lo.float()).numpy()
    got = _rows(back, R, D)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "planes_to_rows is not hi + lo formed in fp32"
    assert G.untouched(pl.cpu(), 4 * R * D) and G.untouched(back.cpu(), 4 * R * D)


# ------------------------------------------------------------------ the two LayerNorm kernels
def _gather_block(d, m, bt, ops, dv):
    return W.TokGatherArgs(P=W.ptr(dv["P"]), ldp=ops.ldp, tok_start=W.ptr(m["tok_start"]), lri=W.ptr(m["lri"]), row_pos=W.ptr(m["row_pos"]), row_seq=W.ptr(m["row_seq"]), R=bt.R,
                           chans=ops.chans, bias=W.ptr(dv["bias"]), ln_g=W.ptr(dv["ln_g"]), ln_b=W.ptr(dv["ln_b"]), col0=ops.col0, D=ops.D, ebins=W.ptr(dv["ebins"]),
                           pbins=W.ptr(dv["pbins"]), nb=W.NB, TE=W.ptr(dv["TE"]), TP=W.ptr(dv["TP"]), ln_g2=W.ptr(dv["ln_g2"]), ln_b2=W.ptr(dv["ln_b2"]), pe=W.ptr(dv["pe"]),
                           pe_alpha=W.ptr(m["alpha"]), x_scale=W.X_SCALE)


def _uploads(chans, D):
    key = ("ops", chans, D)
    if key not in _state:
        d, _, _ = _dev()
        ops = W.operands(chans, D)
        names = ("P", "bias", "ln_g", "ln_b", "ln_g2", "ln_b2", "ebins", "pbins", "TE", "TP", "pe", "e_rows", "p_rows", "es", "ps", "se", "sp", "f2s")
        _state[key] = (ops, {k: d.up(getattr(ops, k)) for k in names})
    return _state[key]


@pytest.mark.parametrize("chans,D", W.WIDTHS)
def test_var_gather0_against_float64(chans, D):
    """Planes only, at the column offset of the predictor; half a wave idle in the first pass (128), the shipped width (256), the last element of the four-pass
    register array (1024).  The rows the ReLU kills completely give ln_b exactly."""
    from tests.conftest import record_measurement
    d, m, bt = _dev()
    ops, dv = _uploads(chans, D)
    R, N2 = bt.R, 2 * chans
    vp = d.out(4 * R * N2)
    a = _gather_block(d, m, bt, ops, dv)
    a.vp = W.ptr(vp)
    _ok(d.launch("var_gather0", a))
    live = bt.row_pos[:R] >= 0
    v = _plane_values(vp, R, N2)
    _assert_rows(v, live, 4 * R * N2, vp, "var_gather0 %d" % chans)
    ref = W.ref_var_gather0(ops)
    key = ("var_gather0", chans)
    err, bar = np.abs(v - ref), W.planes_bar(key, ref)
    ratio = float((err / bar).max())
    print("var_gather0 %d: max-abs %.3e, bar %.3e (+ planes), worst error / bar %.3f, error / fp32 bar alone %.3f" % (chans, err.max(), W.BAR[key], ratio, err.max() / W.BAR[key]))
    record_measurement("rowstep_var_gather0_c%d_error_to_bar" % chans, ratio)
    rows = np.nonzero((err > bar).any(axis=1))[0]
    assert len(rows) == 0, "var_gather0 %d: rows %s beyond the bar (worst %.3g bars)" % (chans, rows[:8], ratio)
    k0 = bt.start[W.Batch.KILLED]
    killed = v[k0:k0 + bt.len[W.Batch.KILLED]]
    hi, lo = G.split_bf16(torch.from_numpy(ops.ln_b))
    assert np.array_equal(killed, np.broadcast_to(G.pair_value(hi, lo).numpy(), killed.shape)), "a row the ReLU kills is not ln_b exactly"


ROUTES = ("rows", "planes", "teacher", "short", "short_per_frame")


def _dec_in_results(chans, D):
    key = ("dec", chans, D)
    if key not in _state:
        d, m, bt = _dev()
        ops, dv = _uploads(chans, D)
        R, sh = bt.R, bt.short
        runs = {}
        for route in ROUTES:
            x0, x0p, qe, qp = (None if route == "planes" else d.out(4 * R * D)), d.out(4 * R * D), d.out(4 * R), d.out(4 * R)
            a = _gather_block(d, m, bt, ops, dv)
            a.x0, a.x0p, a.qe_rows, a.qp_rows = W.ptr(x0), W.ptr(x0p), W.ptr(qe), W.ptr(qp)
            a.e_rows, a.p_rows = W.ptr(dv["e_rows"]), W.ptr(dv["p_rows"])
            sq = None
            if route == "teacher":
                a.es, a.ps, a.es_stride, a.ps_stride, a.e_rows, a.p_rows = W.ptr(dv["es"]), W.ptr(dv["ps"]), ops.es_stride, ops.ps_stride, None, None
            elif route == "short":          # the predictions per short row: var_bucket_short searches them, the frames read the indices through f2s
                sq = (d.out(4 * sh["Rs"]), d.out(4 * sh["Rs"]))
                a.e_rows, a.p_rows, a.f2s, a.sqe, a.sqp, a.srow_pos, a.Rs = W.ptr(dv["se"]), W.ptr(dv["sp"]), W.ptr(dv["f2s"]), W.ptr(sq[0]), W.ptr(sq[1]), W.ptr(m["srow_pos"]), sh["Rs"]
            elif route == "short_per_frame":      # the map is given, the indices are not: searched per frame from the same values
                a.f2s, a.srow_pos, a.Rs = W.ptr(dv["f2s"]), W.ptr(m["srow_pos"]), sh["Rs"]
            _ok(d.launch("dec_in_gather", a))
            runs[route] = dict(x0=x0.cpu() if x0 is not None else None, x0p=x0p.cpu(), qe=qe.cpu(), qp=qp.cpu(), sq=tuple(t.cpu() for t in sq) if sq else None)
        _state[key] = runs
    return _state[key]


@pytest.mark.parametrize("chans,D", W.WIDTHS)
def test_dec_in_gather_against_float64(chans, D):
    from tests.conftest import record_measurement
    _, _, bt = _dev()
    ops, runs = W.operands(chans, D), _dec_in_results(chans, D)
    R, key = bt.R, ("dec_in_gather", D)
    live = bt.row_pos[:R] >= 0
    worst = 0.0
    for route, out in runs.items():
        ref, qe, qp = W.ref_dec_in_gather(ops, "teacher" if route == "teacher" else "rows")
        for name, got, want in (("qe", out["qe"], qe), ("qp", out["qp"], qp)):
            assert np.array_equal(_ints(got, R), want) and G.untouched(got, 4 * R), "dec_in_gather %s: %s" % (route, name)
        forms = [("planes", _plane_values(out["x0p"], R, D), W.planes_bar(key, ref), out["x0p"])]
        if out["x0"] is not None:
            forms.append(("rows", _rows(out["x0"], R, D).astype(np.float64), np.full(ref.shape, W.BAR[key]), out["x0"]))
        for form, v, bar, buf in forms:
            who = "dec_in_gather %d %s %s" % (D, route, form)
            _assert_rows(v, live, 4 * R * D, buf, who)
            err = np.abs(v - ref)
            ratio = float((err / bar).max())
            print("%s: max-abs %.3e, bar %.3e, worst error / bar %.3f" % (who, err.max(), W.BAR[key], ratio))
            worst = max(worst, ratio)
            rows = np.nonzero((err > bar).any(axis=1))[0]
            assert len(rows) == 0, "%s: rows %s beyond the bar (worst %.3g bars)" % (who, rows[:8], ratio)
    record_measurement("rowstep_dec_in_gather_D%d_error_to_bar" % D, worst)


@pytest.mark.parametrize("chans,D", W.WIDTHS)
def test_dec_in_gather_routes_and_forms_agree_bit_for_bit(chans, D):
    """The planes are the split of the rows written with them; without rows (x0 == nullptr) the planes hold the same bytes; through f2s / sqe / sqp the bytes and the
    indices are those of the per-frame search of the same values, also where the map is given and the indices are not; var_bucket_short's indices are numpy's."""
    _, _, bt = _dev()
    ops, runs = W.operands(chans, D), _dec_in_results(chans, D)
    R, sh = bt.R, bt.short
    base = runs["rows"]
    _assert_planes_are_split_of(base["x0p"], _rows(base["x0"], R, D), "dec_in_gather")
    t = runs["teacher"]
    _assert_planes_are_split_of(t["x0p"], _rows(t["x0"], R, D), "dec_in_gather teacher")
    assert torch.equal(runs["planes"]["x0p"], base["x0p"]), "the planes written alone differ from the planes written with rows"
    for route in ("planes", "short", "short_per_frame"):
        for k in ("x0", "x0p", "qe", "qp"):
            if runs[route][k] is not None:
                assert torch.equal(runs[route][k], base[k]), "dec_in_gather %s: %s differs from the per-frame search's" % (route, k)
    sqe, sqp = ops.short_search()
    for name, got, want in (("sqe", runs["short"]["sq"][0], sqe), ("sqp", runs["short"]["sq"][1], sqp)):
        assert np.array_equal(_ints(got, sh["Rs"]), want) and G.untouched(got, 4 * sh["Rs"]), name
    assert ops.f2s[ops.forced] == -1 and _ints(base["qe"], R)[ops.forced] == W.bucket(0.0, ops.ebins)      # the frame without a short row reads 0


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    d, m, bt = _dev()
    R = bt.R
    lri = d.out(4 * R)
    a = W.RowStepArgs(row_pos=W.ptr(m["row_pos"]), row_seq=W.ptr(m["row_seq"]), R=R, vlen=W.ptr(m["vlen"]), B=bt.B, Tmax=bt.Tmax, D=128, cum_in=W.ptr(m["cum"]),
                      ilen=W.ptr(m["ilen"]), tok_start=W.ptr(m["tok_start"]), index_rows=W.ptr(lri))
    n = ctypes.sizeof(a)
    assert d.launch("lr_index", a, size=n - 8) == -1 and d.launch("lr_index", a, size=ctypes.sizeof(W.TokGatherArgs)) == -1
    assert d.launch("lr_index", None, size=n) == -1
    assert d.launch(-1, a) == -1 and d.launch(len(W.STEPS), a) == -1
    assert d.launch("var_gather0", a) == -1 and d.launch("lr_index_short", a) == -1      # another step's block
    assert G.untouched(lri.cpu(), 0), "a refused call launched"
    _ok(d.launch("lr_index", a))
    assert np.array_equal(_ints(lri, R), bt.lri)
