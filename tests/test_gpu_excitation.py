"""The excitation from F0 and its phase on the MI355X (fs2_op_excitation_* / fs2_op_f0_phase_*, fastspeech2_amd.f0_phase / excitation,
GriffinLim(init="f0"), inference_batch_pitch) against the numpy statement of tests/excitation_oracle.py.  The bars are the
oracle's (excitation_oracle.bars: 8 x the error of its own float32 statement against the float64 one), equality of bits between the
forms of the call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import excitation_oracle as E
from tests import vocoder_oracle as O

pytestmark = pytest.mark.gpu

GEOMS = [(1024, 256, 1024), (2048, 300, 1200), (512, 128, 512)]
SR = E.SR


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


_GL = {}


def _gl(geom=GEOMS[0]):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    if geom not in _GL:
        _GL[geom] = GriffinLim(DotDict({"audio": {"n_fft": geom[0], "hop_length": geom[1], "win_length": geom[2], "n_mels": 80, "sample_rate": SR}}))
    return _GL[geom]


def _cuda(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()


_CASES = {}


def case(padded=False):
    if padded not in _CASES:
        f0, starts, lens = E.batch_case(padded=padded)
        f0.setflags(write=False)
        _CASES[padded] = (f0, starts, lens)
    return _CASES[padded]


# ---- 1. against the oracle ----
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d_%d_%d" % g)
def test_excitation_and_phase_against_the_oracle(geom):
    f0, starts, lens = case()
    gl = _gl(geom)
    hop = geom[1]
    utts = [f0[s:s + n] for s, n in zip(starts, lens)]
    ebar, pbar = E.bars(utts, *geom, SR)
    w = gl.excitation(_cuda(f0), lens)
    assert w.sample_lens.tolist() == [hop * (n - 1) for n in lens]
    got = w.wav.cpu().numpy()
    phase = gl.f0_phase(_cuda(f0), lens).cpu().numpy()
    assert phase.shape == (sum(lens), geom[0] // 2 + 1) and np.all(np.isfinite(phase))
    at, we, wp = 0, 0.0, 0.0
    for u, s, n in zip(utts, starts, lens):
        want = E.excitation(u, hop, SR)
        e = got[at:at + want.size]
        at += want.size
        if want.size:
            v = E.sample_phase(u, hop, SR)[3]
            assert np.array_equal(e[~v].view(np.uint32), want[~v].astype(np.float32).view(np.uint32))    # the hashed noise: the same bits
            we = max(we, float(np.abs(e - want).max()))
        ph, X = E.f0_phase(u, *geom, SR, return_stft=True)
        if n < geom[0] // (2 * hop) + 2:
            assert not phase[s:s + n].any()
        wp = max(wp, E.phasor_error(phase[s:s + n], X, ph))
    tag = "%d_%d_%d" % geom
    _record("excitation_err_" + tag, we)
    _record("f0_phase_phasor_err_" + tag, wp)
    print("excitation error %.3g (bar %.3g), phasor error %.3g (bar %.3g)" % (we, ebar, wp, pbar))
    assert we <= ebar, (we, ebar)
    assert wp <= pbar, (wp, pbar)


# ---- 2. invariance: equality of bits ----
@pytest.mark.parametrize("geom", GEOMS[:2], ids=lambda g: "%d_%d_%d" % g)
def test_alone_batch_packed_padded_host_device_and_twice(geom):
    f0, starts, lens = case()
    gl = _gl(geom)
    hop = geom[1]
    f = _cuda(f0)
    batch, wav = gl.f0_phase(f, lens), gl.excitation(f, lens)
    assert torch.equal(batch, gl.f0_phase(f, lens)) and torch.equal(wav.wav, gl.excitation(f, lens).wav)            # two calls in a row
    parts = wav.split()
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert torch.equal(gl.f0_phase(f[s:s + n], [n]), batch[s:s + n]), n
        assert torch.equal(gl.excitation(f[s:s + n], [n]).wav, parts[b]), n
    pf0, pstarts, _ = case(padded=True)
    B, Lmax = len(lens), max(lens)
    p = _cuda(pf0).reshape(B, Lmax)
    padded = gl.f0_phase(p, lens)
    assert padded.shape == (B, Lmax, geom[0] // 2 + 1)
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert torch.equal(padded[b, :n], batch[s:s + n]), b
        assert not padded[b, n:].any()
    assert torch.equal(gl.excitation(p, lens).wav, wav.wav)
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    assert torch.equal(gl.f0_phase(f, ol, sync=False), batch)
    assert torch.equal(gl.f0_phase(p, ol, sync=False), padded)
    assert not torch.equal(gl.excitation(f, lens, seed=1).wav, wav.wav)


def _dev_call(name, gl, f0, ol, stride, cap, out, extra=(), upstream=None):
    from fastspeech2_amd import _lib
    lib = _lib.lib()
    g = gl.geometry
    n = int(lib.fs2_op_f0_phase_workspace_bytes_cap(*g, ol.numel(), cap))
    assert n > 0
    ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    _lib.check(getattr(lib, name)(C.c_void_p(torch.cuda.current_stream().cuda_stream), *g, f0.data_ptr(), ol.numel(), ol.data_ptr(), stride, cap,
                                  upstream.data_ptr() if upstream is not None else None, 71.0, 800.0, SR, 0, ws.data_ptr(), n, out.data_ptr(), *extra))
    torch.cuda.synchronize()
    return ws[:16].view(torch.int32).cpu().tolist()


def test_device_form_of_the_excitation_equals_the_host_form():
    f0, starts, lens = case()
    gl = _gl()
    f = _cuda(f0)
    want = gl.excitation(f, lens).wav
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    out = torch.full((want.numel() + 5,), -7.25, dtype=torch.float32, device="cuda")
    hdr = _dev_call("fs2_op_excitation_dev", gl, f, ol, 0, f.numel(), out, (0, out.numel()))
    assert hdr[:3] == [sum(lens), 0, want.numel()]
    assert torch.equal(out[:want.numel()], want) and bool((out[want.numel():] == -7.25).all())


@pytest.mark.parametrize("lens,stride,upstream,flag", [((4, -1, 3), 0, False, 64), ((9, 9), 0, False, 1), ((3, 7), 6, False, 2), ((4, 5), 0, True, 32)],
                         ids=["negative", "sum_overflows", "longer_than_stride", "upstream"])
def test_invalid_device_lengths_write_nothing(lens, stride, upstream, flag):
    gl = _gl()
    rows = 17 if not stride else stride * len(lens)
    f = torch.full((rows,), 200.0, dtype=torch.float32, device="cuda")
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    up = torch.tensor([0, 0, 4, 0, 0, 0, 0, 0], dtype=torch.int32, device="cuda") if upstream else None
    phase = torch.full((rows, 513), -7.25, dtype=torch.float32, device="cuda")
    hdr = _dev_call("fs2_op_f0_phase_dev", gl, f, ol, stride, rows, phase, upstream=up)
    assert hdr[0] == 0 and hdr[1] & flag and bool((phase == -7.25).all())
    wav = torch.full((256 * rows,), -7.25, dtype=torch.float32, device="cuda")
    hdr = _dev_call("fs2_op_excitation_dev", gl, f, ol, stride, rows, wav, (0, wav.numel()), upstream=up)
    assert hdr[0] == 0 and hdr[1] & flag and bool((wav == -7.25).all())


# ---- 3. wiring ----
@pytest.mark.parametrize("kw", [dict(n_iter=0), dict(n_iter=3), dict(n_iter=3, momentum=0.99), dict(n_iter=3, constraint="mel")],
                         ids=["it0", "it3", "momentum", "mel"])
def test_init_f0_is_init_phase_of_f0_phase(kw):
    gl = _gl()
    f0, starts, lens = case()
    f = _cuda(f0)
    mel = _cuda(np.random.RandomState(4).randn(sum(lens), 80) - 3.0)
    a = gl(mel, lens, init="f0", f0=f, **kw)
    b = gl(mel, lens, init_phase=gl.f0_phase(f, lens), **kw)
    assert torch.equal(a.wav, b.wav) and a.wav.numel() > 0 and bool(torch.isfinite(a.wav).all())
    assert not torch.equal(a.wav, gl(mel, lens, **kw).wav)                                   # the phase reached the kernels
    ol = torch.tensor(lens, dtype=torch.int64, device="cuda")
    d = gl(mel, ol, init="f0", f0=f, sync=False, **kw)
    e = gl(mel, ol, init_phase=gl.f0_phase(f, ol, sync=False), sync=False, **kw)
    assert d.ok() and e.ok() and torch.equal(d.wav, e.wav)
    assert torch.equal(d.wav[:a.wav.numel()], a.wav)


def test_refusals_before_the_gpu_is_touched():
    gl = _gl()
    mel, f = torch.zeros(4, 80, device="cuda"), torch.full((4,), 200.0, device="cuda")
    with pytest.raises(ValueError, match="needs f0"):
        gl(mel, [4], init="f0")
    with pytest.raises(ValueError, match="not both"):
        gl(mel, [4], init="f0", f0=f, init_phase=torch.zeros(4, 513, device="cuda"))
    with pytest.raises(ValueError, match="one value per row"):
        gl(mel, [4], init="f0", f0=f[:3])
    with pytest.raises(TypeError, match="float32"):
        gl(mel, [4], init="f0", f0=f.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(mel, [4], init="f0", f0=f.cpu())
    for lo, hi in ((0.0, 800.0), (-1.0, 800.0), (71.0, float("inf")), (900.0, 800.0), (float("nan"), 800.0)):
        with pytest.raises(ValueError, match="f0_floor"):
            gl(mel, [4], init="f0", f0=f, f0_floor=lo, f0_ceil=hi)
        with pytest.raises(ValueError, match="f0_floor"):
            gl.f0_phase(f, [4], f0_floor=lo, f0_ceil=hi)


# ---- 4. it does what it is for ----
@pytest.mark.parametrize("signal", E.SIGNALS)
@pytest.mark.parametrize("geom", E.VALUE_GEOMS, ids=lambda g: "%d_%d_%d" % g)
def test_one_pass_through_mels_matches_the_oracle_and_keeps_the_pitch(geom, signal):
    from fastspeech2_amd.vocoder import pitch
    c = E.value_case(*geom, signal, True)
    gl = _gl(geom)
    st = O.Stft(*geom)
    w = gl(_cuda(c["mel"]), [64], n_iter=0, init="f0", f0=_cuda(c["f0"]))
    sc = st.spectral_convergence(c["M"].astype(np.float64), w.wav.cpu().numpy().astype(np.float64))
    tag = "%d_%d_%d_%s" % (geom + (signal,))
    _record("f0_one_pass_sc_" + tag, sc)
    print("one pass from the F0 phase: sc %.4f (oracle %.4f; SPSI %.4f)" % (sc, c["sc_f0_0"], c["sc_spsi_0"]))
    assert abs(sc - c["sc_f0_0"]) <= 0.02 * c["sc_f0_0"], (sc, c["sc_f0_0"])
    assert sc < c["sc_spsi_0"]
    if signal == "speech":
        est = pitch(w.wav, w.sample_lens, hp=_hp_of(geom)).cpu().numpy()
        worst, left_out, dev = E.pitch_true(c["f0"], est, geom[0], geom[1])
        _record("f0_one_pass_pitch_dev_" + tag, worst)
        print("pitch of the one-pass waveform: worst %.4f, median %.4f of %d frames, left out %.3f" % (worst, float(np.median(dev)), dev.size, left_out))
        assert worst <= 0.03 and left_out <= 0.10 and dev.size > 0


def _hp_of(geom):
    from fastspeech2_amd.hparams import DotDict
    return DotDict({"audio": {"n_fft": geom[0], "hop_length": geom[1], "win_length": geom[2], "n_mels": 80, "sample_rate": SR}})


# ---- 5. the model's own pitch ----
def test_model_pitch_to_waveform_eager_async_and_graph():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, make_batch
    from fastspeech2_amd.vocoder import GriffinLim
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.cuda()
    b = make_batch("c3", B=2)
    xs, il, ds = b["xs"].cuda(), b["ilens"], b["ds"].cuda()
    # a random-init model predicts no usable F0: scale 0 and a per-phoneme shift make p_outs a known contour in Hz
    contour = (150.0 + 60.0 * torch.sin(0.35 * torch.arange(xs.shape[1], dtype=torch.float32))).repeat(xs.shape[0], 1).cuda()
    ctl = dict(pitch_scale=0.0, pitch_shift=contour)
    gl = GriffinLim()
    with torch.no_grad():
        mels, ol, f0 = model.inference_batch_pitch(xs, il, d_override=ds, **ctl)
        assert f0.shape == mels.shape[:2] and f0.dtype == torch.float32
        pp = model.predict_prosody(xs, il, d_override=ds, **ctl)
        for i, L in enumerate(ol.tolist()):
            assert torch.equal(f0[i, :L], pp.pitch[i, :L]) and float(f0[i, :L].min()) >= 90.0 - 1e-3
        a = gl(mels, ol, n_iter=2, init="f0", f0=f0)
        m2 = gl(mels, ol, n_iter=2, init_phase=gl.f0_phase(f0, ol))                        # the manual two-step path
        assert torch.equal(a.wav, m2.wav) and a.wav.numel() > 0
        pm, pol, pf0 = model.inference_batch_pitch(xs, il, d_override=ds, packed=True, **ctl)
        assert torch.equal(gl(pm, pol, n_iter=2, init="f0", f0=pf0).wav, a.wav)
        am = model.inference_batch_pitch(xs, il, d_override=ds, sync=False, **ctl)
        w = gl(am, n_iter=2, sync=False, padded_out=True, init="f0")
        assert am.ok() and w.ok() and torch.equal(w[1].cpu(), a.sample_lens)
        for i, piece in enumerate(a.split()):
            assert torch.equal(w[0][i, :piece.numel()], piece), i
        run = model.capture_graph(xs, il, d_override=ds, vocoder=gl, init="f0", n_iter=2, **ctl)
        wav, sl, status = run(xs)
        assert int(status.cpu()[2]) == 0 and torch.equal(sl.cpu(), a.sample_lens)
        for i, piece in enumerate(a.split()):
            assert torch.equal(wav[i, :piece.numel()], piece), i
