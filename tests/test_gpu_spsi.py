"""The SPSI initial phase on the MI355X (fs2_op_spsi_phase_geom / _dev, fastspeech2_amd.spsi_phase, GriffinLim(init="spsi")) against
the numpy statement of tests/spsi_oracle.py: equality of bits for the phase, in every layout and in both forms of the call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spsi_oracle as S
from tests import vocoder_oracle as O

pytestmark = pytest.mark.gpu

GEOMS = {513: (1024, 256, 1024), 257: (512, 128, 512), 1025: (2048, 300, 1200)}


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


def _hp(geom, n_mels=80):
    from fastspeech2_amd.hparams import DotDict
    return DotDict({"audio": {"n_fft": geom[0], "hop_length": geom[1], "win_length": geom[2], "n_mels": n_mels}})


def _cuda(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()


_GL = {}


def _gl(NB=513):
    from fastspeech2_amd.vocoder import GriffinLim
    if NB not in _GL:
        _GL[NB] = GriffinLim(_hp(GEOMS[NB]))
    return _GL[NB]


_CASES = {}


def case(NB, padded=False):
    """(src, starts, lens, the oracle's phase) of the shared batch, computed once."""
    if (NB, padded) not in _CASES:
        src, starts, lens = S.batch_case(NB, padded=padded)
        want = S.spsi_batch(src, starts, lens, *GEOMS[NB][:2])
        for a in (src, want):
            a.setflags(write=False)
        _CASES[(NB, padded)] = (src, starts, lens, want)
    return _CASES[(NB, padded)]


def _same_bits(t, a):
    return torch.equal(t.cpu().view(torch.int32), torch.from_numpy(np.array(a, np.float32)).view(torch.int32))


# ---- 1. bits against the oracle, magnitude mode ----
def test_packed_batch_equals_the_oracle_bit_for_bit():
    src, starts, lens, want = case(513)
    got = _gl().spsi_phase(_cuda(src), lens, magnitudes=True)
    assert got.shape == (sum(lens), 513) and got.dtype == torch.float32
    assert _same_bits(got, want)
    assert float(got.min()) >= 0.0 and float(got.max()) < 6.2832


def test_padded_batch_equals_the_oracle_bit_for_bit():
    src, starts, lens, want = case(513, padded=True)
    B, Lmax = len(lens), max(lens)
    got = _gl().spsi_phase(_cuda(src).reshape(B, Lmax, 513), lens, magnitudes=True)
    assert got.shape == (B, Lmax, 513)
    assert _same_bits(got.reshape(-1, 513), want)                  # zeros in the rows no utterance covers, as the oracle's


@pytest.mark.parametrize("NB", [257, 1025])
def test_one_utterance_of_each_length_at_the_other_geometries(NB):
    gl = _gl(NB)
    for L in S.BATCH_LENS:
        if L == 0:
            continue
        src, starts, lens = S.batch_case(NB, lens=(L,), seed=40 + L)
        if L >= 10:
            src[:10] = S.crafted_utterance(NB)
        got = gl.spsi_phase(_cuda(src), [L], magnitudes=True)
        assert _same_bits(got, S.spsi_batch(src, starts, lens, *GEOMS[NB][:2])), L


# ---- 2. mel mode ----
@pytest.mark.parametrize("NB", [513, 257])
def test_mel_mode(NB):
    gl = _gl(NB)
    rs = np.random.RandomState(21)
    lens = [33, 1, 0, 18]
    mel = (rs.randn(sum(lens), 80) * 1.5 - 3.0).astype(np.float32)
    m = _cuda(mel)
    phase, mag = gl.spsi_phase(m, lens, return_magnitudes=True)
    assert torch.equal(phase, gl.spsi_phase(mag, lens, magnitudes=True))
    pinv32 = gl.constants(m.device)[0].cpu().numpy().astype(np.float64)
    e = np.exp(mel.astype(np.float64))
    want, bound = O.mel_to_mag(mel, pinv32), 1e-5 * (e @ np.abs(pinv32).T)
    err = np.abs(mag.cpu().numpy().astype(np.float64) - want)
    _record("spsi_mel_to_mag_err_over_bound_%d" % NB, float((err[bound > 0] / bound[bound > 0]).max()))      # (bins above fmax: 0 <= 0)
    assert np.all(err <= bound)
    assert _same_bits(phase, S.spsi_batch(mag.cpu().numpy(), np.concatenate([[0], np.cumsum(lens)[:-1]]), lens, *GEOMS[NB][:2]))


# ---- 3. invariance ----
def test_each_utterance_alone_equals_it_inside_the_batch_and_packed_equals_padded():
    src, starts, lens, _ = case(513)
    gl = _gl()
    batch = gl.spsi_phase(_cuda(src), lens, magnitudes=True)
    for s, n in zip(starts, lens):
        if n:
            alone = gl.spsi_phase(_cuda(src[s:s + n]), [n], magnitudes=True)
            assert torch.equal(alone, batch[s:s + n]), n
    psrc, pstarts, _, _ = case(513, padded=True)
    B, Lmax = len(lens), max(lens)
    padded = gl.spsi_phase(_cuda(psrc).reshape(B, Lmax, 513), lens, magnitudes=True)
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert torch.equal(padded[b, :n], batch[s:s + n]), b
        assert not padded[b, n:].any()


def test_host_form_equals_device_form():
    gl = _gl()
    src, starts, lens, _ = case(513)
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    assert torch.equal(gl.spsi_phase(_cuda(src), ol, magnitudes=True, sync=False), gl.spsi_phase(_cuda(src), lens, magnitudes=True))
    psrc, _, _, _ = case(513, padded=True)
    p = _cuda(psrc).reshape(len(lens), max(lens), 513)
    assert torch.equal(gl.spsi_phase(p, ol, magnitudes=True, sync=False), gl.spsi_phase(p, lens, magnitudes=True))
    rs = np.random.RandomState(5)
    mel = _cuda(rs.randn(sum(lens), 80) - 3.0)
    a, am = gl.spsi_phase(mel, ol, sync=False, return_magnitudes=True)
    b, bm = gl.spsi_phase(mel, lens, return_magnitudes=True)
    assert torch.equal(a, b) and torch.equal(am, bm)


@pytest.mark.parametrize("lens,stride", [((4, -1, 3), 0), ((9, 9), 0), ((3, 7), 6)], ids=["negative", "sum_overflows", "longer_than_stride"])
def test_invalid_device_lengths_write_nothing_and_the_vocoder_reports_them(lens, stride):
    from fastspeech2_amd import _lib
    gl = _gl()
    g = gl.geometry
    rows = 17 if not stride else stride * len(lens)
    src = _cuda(S.random_rows(rows, 513, 2))
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    lib = _lib.lib()
    phase = torch.full((rows, 513), -7.25, dtype=torch.float32, device="cuda")
    mag = torch.full((rows, 513), -7.25, dtype=torch.float32, device="cuda")
    n = int(lib.fs2_op_spsi_workspace_bytes_cap(*g, len(lens), rows))
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(lib.fs2_op_spsi_phase_dev(C.c_void_p(torch.cuda.current_stream().cuda_stream), *g, src.data_ptr(), 513, None, len(lens), ol.data_ptr(),
                                         stride, rows, None, ws.data_ptr(), n, phase.data_ptr(), mag.data_ptr()))
    torch.cuda.synchronize()
    assert bool((phase == -7.25).all()) and bool((mag == -7.25).all())
    m = src if not stride else src.reshape(len(lens), stride, 513)
    w = gl(m, ol, n_iter=1, magnitudes=True, sync=False, init="spsi")
    assert not w.ok() and bool(torch.isnan(w.wav).all())


# ---- 4. wiring ----
@pytest.mark.parametrize("k", [0, 3])
def test_init_spsi_is_init_phase_of_spsi_phase(k):
    gl = _gl()
    lens = [5, 40, 1, 0, 9, 3]
    M = _cuda(S.random_rows(sum(lens), 513, 9))
    ph = gl.spsi_phase(M, lens, magnitudes=True)
    a = gl(M, lens, n_iter=k, magnitudes=True, init="spsi")
    b = gl(M, lens, n_iter=k, magnitudes=True, init_phase=ph)
    assert torch.equal(a.wav, b.wav) and a.wav.numel() > 0 and bool(torch.isfinite(a.wav).all())
    c = gl(M, lens, n_iter=k, magnitudes=True, init="spsi", seed=77)                      # the seed is ignored
    assert torch.equal(a.wav, c.wav)
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    d = gl(M, ol, n_iter=k, magnitudes=True, init="spsi", sync=False)
    e = gl(M, ol, n_iter=k, magnitudes=True, init_phase=gl.spsi_phase(M, ol, magnitudes=True, sync=False), sync=False)
    assert d.ok() and e.ok() and torch.equal(d.wav, e.wav)
    assert torch.equal(d.wav[:a.wav.numel()], a.wav)
    mel = _cuda(np.random.RandomState(4).randn(sum(lens), 80) - 3.0)
    assert torch.equal(gl(mel, lens, n_iter=k, init="spsi").wav, gl(mel, lens, n_iter=k, init_phase=gl.spsi_phase(mel, lens)).wav)


def test_capture_graph_with_init_spsi_replays_the_eager_pair():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, make_batch
    from fastspeech2_amd.vocoder import GriffinLim
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.cuda()
    b = make_batch("c3", B=2)
    xs, il, ds = b["xs"].cuda(), b["ilens"], b["ds"].cuda()
    gl = GriffinLim()
    with torch.no_grad():
        run = model.capture_graph(xs, il, d_override=ds, vocoder=gl, init="spsi", n_iter=2)
        wav, sl, status = run(xs)
        assert int(status.cpu()[2]) == 0
        am = model.inference_batch(xs, il, d_override=ds, sync=False)
        w = gl(am, n_iter=2, sync=False, padded_out=True, init="spsi")
        assert am.ok() and w.ok() and torch.equal(sl, w[1]) and int(sl.sum()) > 0
        n = min(wav.shape[1], w[0].shape[1])                        # (the two capacities differ: compare the common columns, zeros beyond)
        assert int(sl.max()) <= n
        assert torch.equal(wav[:, :n], w[0][:, :n]) and not wav[:, n:].any() and not w[0][:, n:].any()
        seeded = gl(am, n_iter=2, sync=False, padded_out=True)
        assert not torch.equal(seeded[0][:, :n], w[0][:, :n])       # the initial phase reached the kernels
    with pytest.raises(ValueError, match="init must be one of"):
        model.capture_graph(xs, il, d_override=ds, vocoder=gl, init="bogus")


# ---- 5. it does what it is for ----
@pytest.mark.parametrize("mel", [False, True], ids=["magnitudes", "mel_round_trip"])
@pytest.mark.parametrize("geom", [(1024, 256, 1024), (2048, 300, 1200)], ids=lambda g: "%d_%d_%d" % g)
def test_ten_iterations_from_spsi_beat_twenty_from_the_seeded_phase(geom, mel):
    c = S.convergence_case(*geom, mel)
    gl = _gl(geom[0] // 2 + 1)
    st = O.Stft(*geom)
    M = c["M"].astype(np.float64)
    L = M.shape[0]
    src = _cuda(c["mel"] if mel else c["M"])
    spsi = gl(src, [L], n_iter=10, init="spsi", magnitudes=not mel)
    seeded = gl(src, [L], n_iter=20, seed=0, magnitudes=not mel)
    sc_spsi = st.spectral_convergence(M, spsi.wav.cpu().numpy().astype(np.float64))
    sc_seed = st.spectral_convergence(M, seeded.wav.cpu().numpy().astype(np.float64))
    tag = "%d_%d_%d_%s" % (geom + ("mel" if mel else "mag",))
    _record("spsi_sc_spsi10_" + tag, sc_spsi)
    _record("spsi_sc_seeded20_" + tag, sc_seed)
    print("sc spsi+10 %.4f (oracle %.4f) seeded+20 %.4f (oracle %.4f)" % (sc_spsi, c["sc_spsi10"], sc_seed, c["sc_seed20"]))
    assert sc_spsi < sc_seed, (sc_spsi, sc_seed)
    assert abs(sc_spsi - c["sc_spsi10"]) <= 0.02 * c["sc_spsi10"], (sc_spsi, c["sc_spsi10"])


# ---- 6. defaults unchanged ----
def test_init_seeded_is_the_default():
    gl = _gl()
    lens = [6, 21]
    M = _cuda(S.random_rows(sum(lens), 513, 3))
    a = gl(M, lens, seed=3, n_iter=4, magnitudes=True)
    b = gl(M, lens, seed=3, n_iter=4, magnitudes=True, init="seeded")
    assert torch.equal(a.wav, b.wav) and a.wav.numel() == 256 * (5 + 20)
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    assert torch.equal(gl(M, ol, seed=3, n_iter=4, magnitudes=True, sync=False).wav, gl(M, ol, seed=3, n_iter=4, magnitudes=True, sync=False, init="seeded").wav)
