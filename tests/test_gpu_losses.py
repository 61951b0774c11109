"""Loss terms on the MI355X (fs2_op_loss_terms: fastspeech2_amd.losses, csrc/losses.h) against the numpy float64 oracle of the same
definition (tests/losses_oracle.py, itself held to the reference's recordings in tests/test_losses_host.py).

Bars.  The lengths and pad counts (indices 0 .. 3) are exact.  Every sum is within 1e-12 relative of the oracle (floor 1e-300): both
sides add the same non-negative float64 terms in different orders, a reordered double sum of n such terms moves by at most
n 2^-53 relative (3.8e-12 for the largest sum here, n = 34,400; expected sqrt(n) 2^-53 = 2e-14) -- tests/test_losses_kernel_host.py
carries the derivation.  Batch invariance, the NaN cases, graph replay and sync=False are held with EQUALITY of bits.  The
reference's recorded report values are float32 means of <= 11,280 terms: 1e-6 relative, as in tests/test_losses_host.py; forward()'s
own float32 reductions of the same device outputs: 1e-5 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import losses_oracle as O

pytestmark = pytest.mark.gpu

K = 32                # csrc/losses.h: kLtFrames, the frames of a tile (tests/test_losses_kernel_host.py checks that the two agree)
ERR_ARG, ERR_WORKSPACE = -1, -5      # include/fs2.h
DEV = "cuda:0"


def _dev(arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def raw(arrays, ilens, olens, Tmax, Lmax, pads, odim=None, ws_short=0, struct_size_off=0):
    """fs2_op_loss_terms through the bare binding, with Tmax / Lmax of the caller's choice: contiguous numpy arrays (or device
    tensors) in, (rows [B, 20], batch [20]) out; the strides are the arrays' widths."""
    from fastspeech2_amd import _lib
    lib = _lib.lib()
    t = tuple(a if isinstance(a, torch.Tensor) or a is None else _dev([a])[0] for a in arrays)
    before, after, ys, d_outs, ds, e_outs, es, p_outs, ps = t
    B = len(ilens)
    il = np.ascontiguousarray(ilens, np.int32)
    ol = np.ascontiguousarray(olens, np.int32)
    i32p = C.POINTER(C.c_int32)
    ws_bytes = int(lib.fs2_op_loss_workspace_bytes(B, ol.ctypes.data_as(i32p))) if B else 0
    assert ws_bytes > 0 or B == 0
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    rec = torch.full((B + 1, O.TERMS), -777.0, dtype=torch.float64, device=DEV)
    w = lambda x, d=1: 0 if x is None else int(x.shape[d])
    ptr = lambda x: None if x is None else x.data_ptr()
    odim = odim if odim is not None else next(int(x.shape[2]) for x in (before, after, ys) if x is not None)
    a = _lib.OpLossArgs(B, odim, Tmax, Lmax, pads, max(w(before), w(after), w(e_outs), w(p_outs)), w(ys), w(d_outs), w(ds), max(w(es), w(ps)),
                        ptr(before), ptr(after), ptr(ys), ptr(d_outs), ptr(ds), ptr(e_outs), ptr(es), ptr(p_outs), ptr(ps),
                        il.ctypes.data_as(i32p), ol.ctypes.data_as(i32p), ws.data_ptr() if B else None, ws_bytes - ws_short,
                        rec.data_ptr() if B else None, rec[B].data_ptr())
    a.struct_size += struct_size_off
    rc = lib.fs2_op_loss_terms(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a))
    if rc:
        return rc
    host = rec.cpu().numpy()
    return host[:-1], host[-1]


@pytest.fixture(scope="module")
def edge():
    e = O.Edge(K)
    e.dev = _dev(e.tensors())
    e.got = raw(e.dev, e.ilens, e.olens, e.Tmax, e.Lmax, 1)
    return e


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_edge_batch_equals_the_oracle(edge):
    rows, batch = edge.got
    assert np.array_equal(rows[:, :4], edge.rows[:, :4]) and np.array_equal(batch[:4], edge.batch[:4])          # integers: exactly
    rel = np.abs(rows[:, 4:17] - edge.rows[:, 4:17]) / np.maximum(np.abs(edge.rows[:, 4:17]), 1e-300)
    print("worst relative difference of a sum: %.3g (valid), %.3g (pads)" % (rel[:, :8].max(), rel[:, 8:].max()))
    assert O.close(rows, edge.rows) and O.close(batch, edge.batch)
    assert np.all(rows[:, 17:] == 0) and np.all(batch[17:] == 0)
    assert np.all(edge.rows[:, [12, 13, 15, 16]] > 0) and np.all(edge.rows[:5, 14] > 0)      # (the pad sums are a real check: the pads hold data)


def test_python_operator_reads_through_the_strides(edge):
    """loss_terms on the same device tensors: strides from the tensors (the targets are wider), Tmax / Lmax from the lengths."""
    from fastspeech2_amd import loss_terms
    lt = loss_terms(*edge.dev, edge.ilens, edge.olens)
    want_rows, want_batch = O.records(*edge.tensors(), edge.ilens, edge.olens)
    assert lt.pads and lt.odim == 80 and len(lt) == edge.B
    assert np.array_equal(lt.terms[:, :4], want_rows[:, :4])
    assert O.close(lt.terms, want_rows) and O.close(lt.batch, want_batch)
    assert _bits(lt.terms[:, 4:12], edge.got[0][:, 4:12])                 # another Lmax: the same sums over [0, len)
    want = O.report(want_batch, 80, False, True)
    assert np.allclose([v for _, v in lt.report(use_masking=False, use_weighted_masking=True)], [v for _, v in want], rtol=1e-12, atol=0)
    assert np.allclose(lt.evaluate(), O.evaluate(want_rows), rtol=1e-12, atol=0)
    column_slice = loss_terms(edge.dev[0][:, :, :40], None, edge.dev[2][:, :, :40], *([None] * 6), edge.ilens, edge.olens)      # copied
    r40, _ = O.records(*[a[:, :, :40] if i in (0, 1, 2) else a for i, a in enumerate(edge.tensors())], edge.ilens, edge.olens)
    assert column_slice.odim == 40 and O.close(column_slice.terms[:, [4, 12]], r40[:, [4, 12]])
    assert np.all(column_slice.terms[:, 5:12] == 0) and np.all(column_slice.terms[:, 13:] == 0)


def test_batch_invariance_bit_for_bit(edge):
    """Alone (Tmax = ilen, Lmax = olen), at another place in another batch, with other strides: the sums over [0, len) are the
    same bits as in the edge batch."""
    rows = edge.got[0]
    for b in range(edge.B):
        il, ol = int(edge.ilens[b]), int(edge.olens[b])
        alone, _ = raw([t[b:b + 1] for t in edge.dev], [il], [ol], il, ol, 1)
        assert _bits(alone[0, 4:12], rows[b, 4:12]), b
    order = [5, 0, 3, 1, 4, 2]
    moved, _ = raw([t[order].contiguous() for t in edge.dev], edge.ilens[order], edge.olens[order], edge.Tmax, edge.Lmax, 0)
    assert _bits(moved[:, 4:12], rows[order, 4:12])
    Lm, Tm = int(edge.olens.max()), int(edge.ilens.max())
    widths = (Lm, Lm, Lm + 1, Tm, Tm, Lm, Lm + 2, Lm, Lm + 2)            # (d_outs / ds [B, 64]: 8-byte rows; ys: 4 (Lm + 1) 80 bytes)
    narrow, _ = raw([t[:, :w].contiguous() for t, w in zip(edge.dev, widths)], edge.ilens, edge.olens, Tm, Lm, 1)
    assert _bits(narrow[:, 4:12], rows[:, 4:12])
    one_off = [torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape).copy_(t) for t in edge.dev]      # 4 bytes off: the 4-byte loads
    assert one_off[0].data_ptr() % 16 == 4
    shifted, _ = raw(one_off, edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 1)
    assert _bits(shifted, rows)


def _nan_pads(edge):
    out = []
    for i, a in enumerate(edge.tensors()):
        a = a.copy()
        ext = edge.ilens if i in (3, 4) else edge.olens
        for b in range(edge.B):
            a[b, ext[b]:] = -5 if i == 4 else np.nan                    # (ds is int64: -5 makes log(ds + 1) a NaN)
        out.append(a)
    return out


def test_pads_0_reads_nothing_outside_the_utterances(edge):
    clean = raw(edge.dev, edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 0)
    dirty = raw(_nan_pads(edge), edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 0)
    assert np.all(np.isfinite(dirty[0])) and np.all(np.isfinite(dirty[1]))
    assert _bits(dirty[0], clean[0]) and _bits(dirty[1], clean[1])
    assert _bits(clean[0][:, :12], edge.got[0][:, :12]) and np.all(clean[0][:, 12:] == 0) and np.all(clean[1][12:] == 0)
    with_pads = raw(_nan_pads(edge), edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 1)          # (and the pad sums do read them)
    assert np.all(np.isnan(with_pads[0][:, [12, 13, 15, 16]])) and np.all(np.isnan(with_pads[0][:5, 14])) and with_pads[0][5, 14] == 0      # (utterance 5 has Tmax tokens)
    assert _bits(with_pads[0][:, :12], clean[0][:, :12])


def test_nan_in_a_valid_frame_stays_in_its_sums(edge):
    t = [a.copy() for a in edge.tensors()]
    t[0][4, K, 3] = np.nan            # before, utterance 4, its second tile
    t[5][2, 0] = np.nan               # e_outs, utterance 2
    t[3][5, 63] = np.nan              # d_outs, utterance 5, its last token
    rows, batch = raw(t, edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 1)
    want_nan = np.zeros_like(rows, bool)
    want_nan[4, 4] = want_nan[2, 7] = want_nan[2, 10] = want_nan[5, 6] = want_nan[5, 9] = True
    assert np.array_equal(np.isnan(rows), want_nan)
    assert _bits(rows[~want_nan], edge.got[0][~want_nan])
    assert np.array_equal(np.isnan(batch), want_nan.any(axis=0))


@pytest.mark.parametrize("odim", [1, 3, 128])
def test_other_mel_widths(odim):
    rng = np.random.default_rng(odim)
    il, ol, Tm, Lm = [5, 9], [K + 3, 2 * K + 1], 9, 2 * K + 2
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    t = (f(2, Lm, odim), f(2, Lm, odim), f(2, Lm + 1, odim), f(2, Tm), rng.integers(0, 9, (2, Tm)).astype(np.int64), f(2, Lm), f(2, Lm + 3), f(2, Lm), f(2, Lm + 3))
    rows, batch = raw(t, il, ol, Tm, Lm, 1)
    want_rows, want_batch = O.records(*t, il, ol, Tm, Lm)
    assert np.array_equal(rows[:, :4], want_rows[:, :4])
    assert O.close(rows, want_rows) and O.close(batch, want_batch)


def test_many_utterances_and_none():
    B = 257                           # beyond the 256 threads of lt_combine and the 250 records of one upload launch
    rng = np.random.default_rng(257)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    t = (f(B, 1, 80), f(B, 1, 80), f(B, 1, 80), f(B, 1), rng.integers(0, 9, (B, 1)).astype(np.int64), f(B, 1), f(B, 1), f(B, 1), f(B, 1))
    rows, batch = raw(t, [1] * B, [1] * B, 1, 1, 1)
    want_rows, want_batch = O.records(*t, [1] * B, [1] * B)
    assert O.close(rows, want_rows) and O.close(batch, want_batch) and batch[0] == B == batch[1]
    rows0, batch0 = raw(t, [], [], 0, 0, 1)
    assert rows0.shape == (0, O.TERMS) and np.all(batch0 == 0)
    from fastspeech2_amd import loss_terms
    none = loss_terms(*[x[:0] for x in _dev(t)], [], [])
    assert len(none) == 0 and np.all(none.batch == 0)


def test_reference_recordings_through_the_operator(golden_dir):
    from fastspeech2_amd import loss_terms
    g2, g9 = np.load(golden_dir + "/g2_teacher_padded_b3.npz"), np.load(golden_dir + "/g9_weighted_masking_b3.npz")
    lt = loss_terms(*_dev([g2[k] for k in ("before", "after", "ys", "d_outs", "ds", "e_outs", "es", "p_outs", "ps")]), g2["ilens"], g2["olens"])
    assert [n for n, _ in lt.report()] == g2["report_names"].tolist()
    masked = np.asarray([v for _, v in lt.report()])
    weighted = np.asarray([v for _, v in lt.report(use_masking=False, use_weighted_masking=True)])
    w2, w9 = np.max(np.abs(masked / g2["report_values"] - 1)), np.max(np.abs(weighted / g9["report_values"] - 1))
    print("worst relative difference: G2 masked %.3g, G9 unmasked + weighted %.3g" % (w2, w9))
    assert w2 <= 1e-6 and w9 <= 1e-6
    with pytest.raises(IndexError):
        lt.report(use_masking=True, use_weighted_masking=True)


@pytest.fixture(scope="module")
def model():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    hp = default_hparams()
    m = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    m.load_state_dict(portable_state_dict(m.state_dict(), seed=0))
    m = m.to(DEV)
    assert m.precision == "fp32"
    return m


def test_evaluate_batch(model, golden_dir):
    g = np.load(golden_dir + "/g2_teacher_padded_b3.npz")
    a = {k: torch.from_numpy(g[k]).to(DEV) for k in ("xs", "ilens", "ys", "olens", "ds", "es", "ps")}
    args = lambda s=slice(None): [a[k][s] for k in ("xs", "ilens", "ys", "olens", "ds", "es", "ps")]
    with torch.no_grad():
        _, rep = model(*args())                                         # forward(): float32 reductions of the same device outputs
        lt = model.evaluate_batch(*args(), semantics="padded_compat")
        assert [n for n, _ in lt.report()] == [list(x)[0] for x in rep]
        got, want = np.asarray([v for _, v in lt.report()]), np.asarray([list(x.values())[0] for x in rep])
        print("evaluate_batch(padded_compat).report() against forward(): worst relative %.3g" % np.max(np.abs(got / want - 1)))
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (got, want)
        model.use_masking, model.use_weighted_masking = False, True
        try:
            _, rep = model(*args())
        finally:
            model.use_masking, model.use_weighted_masking = True, False
        got, want = np.asarray([v for _, v in lt.report(False, True)]), np.asarray([list(x.values())[0] for x in rep])
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (got, want)
        # per-utterance semantics: an utterance's numbers do not depend on the batch it is in
        whole = model.evaluate_batch(*args())
        assert not whole.pads
        singles = [model.evaluate_batch(*args(slice(b, b + 1))) for b in range(3)]
        assert all(_bits(s.terms[0, 4:12], whole.terms[b, 4:12]) for b, s in enumerate(singles))
        mean = tuple(float(np.mean([s.evaluate()[i] for s in singles])) for i in range(3))
        assert _bits(whole.evaluate(), mean)
        with pytest.raises(ValueError, match="pads=False"):
            whole.report(use_masking=False)
        with pytest.raises(ValueError, match="semantics"):
            model.evaluate_batch(*args(), semantics="padded")
        model.reduction_factor = 2
        try:
            with pytest.raises(NotImplementedError):
                model.evaluate_batch(*args())
        finally:
            model.reduction_factor = 1


def test_sync_false_and_graph_replay(edge):
    from fastspeech2_amd import loss_terms
    eager = loss_terms(*edge.dev, edge.ilens, edge.olens)
    later = loss_terms(*edge.dev, edge.ilens, edge.olens, sync=False)
    assert later._device is not None and later._terms is None           # nothing was read back
    assert _bits(later.terms, eager.terms) and _bits(later.batch, eager.batch) and later._device is None
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = loss_terms(*edge.dev, edge.ilens, edge.olens, sync=False)
        captured._device.fill_(float("nan"))                            # whatever the capture left: only a replay's numbers count
        graph.replay()
    side.synchronize()
    assert _bits(captured.terms, eager.terms) and _bits(captured.batch, eager.batch)


def test_refusals(edge):
    assert raw(edge.dev, edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 1, ws_short=1) == ERR_WORKSPACE
    assert raw(edge.dev, edge.ilens, edge.olens, edge.Tmax, edge.Lmax, 1, struct_size_off=8) == ERR_ARG
    assert raw(edge.dev, edge.ilens, edge.olens, edge.Tmax, int(edge.olens.max()) - 1, 1) == ERR_ARG          # olen > Lmax
    from fastspeech2_amd import _lib
    assert "Lmax" in _lib.lib().fs2_last_error(None).decode()
