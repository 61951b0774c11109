"""CPU: the semantics of the excitation from F0 and of its phase as tests/excitation_oracle.py states them --
a case done by hand, the closed-form phase against a running sum, the edge rows -- what the feature is for (one pass from the F0 phase
beats one pass from SPSI; the waveform has the commanded pitch), and what needs no GPU of the interface: the exported symbols, the
workspace queries, the refusals of the entry points that end before a launch, the argument errors of the Python layer."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import excitation_oracle as E
from tests import pitch_oracle as P

PTR = C.c_void_p(0x1000)          # a non-null pointer nothing dereferences: every call here ends before a launch
G = (1024, 256, 1024, 80)
FS2_OK, FS2_ERR_ARG, FS2_ERR_WORKSPACE, FS2_ERR_UNSUPPORTED = 0, -1, -5, -6          # include/fs2.h


@pytest.fixture(scope="module")
def lib():
    from fastspeech2_amd import _lib
    _lib.build()
    return _lib.lib()


def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


# ---- 1. by hand: H = 4, sr = 1000, five frames, one switch to unvoiced and one back ----
def test_a_case_done_by_hand():
    H, sr = 4, 1000
    f0 = np.array([100, 120, 0, 200, 200], np.float32)
    a, d, vs = E.segments(f0)
    assert vs.tolist() == [True, False, False, True]
    assert a.tolist() == [100.0, 0.0, 0.0, 200.0] and d.tolist() == [20.0, 0.0, 0.0, 0.0]
    theta, f, Hn, voiced, Theta = E.sample_phase(f0, H, sr)
    # S_0 = (4 . 100 + 20 . 3 / 2) / 1000 = 0.43, S_1 = S_2 = 0, S_3 = 0.8
    assert np.allclose(Theta, [0.0, 0.43, 0.43, 0.43, 0.23], atol=1e-15)
    # segment 0: ((i + 1) 100 + 20 i (i + 1) / 8) / 1000; its last sample lands on Theta_1.  segment 3: 0.43 + 0.2 (i + 1)
    assert np.allclose(theta[:4], [0.1, 0.205, 0.315, 0.43], atol=1e-15)
    assert np.allclose(theta[12:], [0.63, 0.83, 0.03, 0.23], atol=1e-15)
    assert f[:4].tolist() == [100.0, 105.0, 110.0, 115.0] and f[12:].tolist() == [200.0] * 4
    assert Hn[:4].tolist() == [4, 4, 4, 4] and Hn[12:].tolist() == [2, 2, 2, 2]            # 4 . 115 < 500 <= 5 . 100; 2 . 200 < 500 <= 3 . 200
    assert voiced.tolist() == [True] * 4 + [False] * 8 + [True] * 4
    e = E.excitation(f0, H, sr, seed=3)
    for n, (th, hn) in enumerate(zip(theta, Hn)):
        if voiced[n]:
            want = math.sqrt(2.0 / hn) * sum(math.cos(2 * math.pi * h * th) for h in range(1, hn + 1))
            assert abs(e[n] - want) <= 1e-12
        else:
            u = np.float32(_mix32(n ^ _mix32(3 + 0x9E3779B9)) >> 8) * np.float32(2.0 ** -24)
            assert e[n] == np.float64((u - np.float32(0.5)) * np.float32(3.46410162))
    e32 = E.excitation(f0, H, sr, seed=3, dtype=np.float32)
    assert e32.dtype == np.float32 and np.array_equal(e32[~voiced], e[~voiced].astype(np.float32)) and np.abs(e32 - e).max() < 1e-5


def test_the_closed_form_phase_is_the_running_sum_of_the_frequency():
    rs = np.random.RandomState(0)
    for hop, sr in ((256, 22050), (300, 22050), (128, 16000)):
        f0 = (rs.uniform(80, 400, 40)).astype(np.float32)
        f0[10:13] = 0.0
        f0[20] = np.nan
        theta, f, _, voiced, _ = E.sample_phase(f0, hop, sr)
        run = np.cumsum(np.where(voiced, f, 0.0) / sr)
        diff = theta - run
        diff -= np.round(diff)
        assert np.abs(diff[voiced]).max() <= 1e-12
        e = E.excitation(f0, hop, sr)
        assert abs(np.mean(e[voiced] ** 2) - 1.0) < 0.1 and abs(np.mean(e[~voiced] ** 2) - 1.0) < 0.1      # unit power, both kinds


# ---- 2. edge rows ----
def test_which_frames_and_segments_are_voiced():
    f0 = np.array([np.nan, np.inf, -np.inf, -100.0, 0.0, 70.99, 71.0, 800.0, 800.1, 200.0], np.float32)
    assert E.voiced_frames(f0).tolist() == [False] * 6 + [True, True, False, True]
    assert E.segments(f0)[2].tolist() == [False] * 6 + [True, False, False]
    island = np.array([0, 0, 200, 0, 0], np.float32)                   # one voiced frame: no voiced segment
    assert not E.segments(island)[2].any()
    assert np.array_equal(E.excitation(island, 8, 22050, seed=5), E.noise(32, 5).astype(np.float64))
    assert np.array_equal(E.excitation(np.full(6, np.nan, np.float32), 8, 22050, seed=5), E.noise(40, 5).astype(np.float64))
    allv = np.full(6, 150.0, np.float32)
    assert E.sample_phase(allv, 8, 22050)[3].all()
    assert np.array_equal(E.excitation(allv, 8, 22050, seed=1), E.excitation(allv, 8, 22050, seed=2))       # the seed: unvoiced samples only
    assert not np.array_equal(E.excitation(island, 8, 22050, seed=1), E.excitation(island, 8, 22050, seed=2))
    # the limits are inclusive and the caller's
    assert E.voiced_frames(np.array([60.0, 900.0], np.float32), 60.0, 900.0).all()


@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_the_shortest_utterances(L):
    f0 = np.full(L, 200.0, np.float32)
    e = E.excitation(f0, 256, 22050)
    assert e.size == 256 * max(L - 1, 0)
    ph = E.f0_phase(f0, 1024, 256, 1024, 22050)
    assert ph.shape == (L, 513) and ph.dtype == np.float32
    assert not ph.any() if L < 4 else ph.any()                         # N <= n_fft / 2: every row 0
    assert E.f0_phase(np.full(4, 200.0, np.float32), 1024, 256, 1024, 22050).any()


def test_the_bars_come_from_the_float32_statement():
    f0s = [E.f0_rows(L, 21 + b) for b, L in enumerate(E.BATCH_LENS)]
    for g in ((1024, 256, 1024), (512, 128, 512)):
        ebar, pbar = E.bars(f0s, *g, E.SR)
        print("%s: excitation bar %.3g, phase bar %.3g" % (g, ebar, pbar))
        assert 1e-6 < ebar < 1e-3 and 1e-5 < pbar < 0.1


# ---- 3. what it is for ----
@pytest.mark.parametrize("mel", [False, True], ids=["magnitudes", "through_80_mels"])
@pytest.mark.parametrize("signal", E.SIGNALS)
@pytest.mark.parametrize("geom", E.VALUE_GEOMS, ids=lambda g: "%d_%d_%d" % g)
def test_one_pass_from_the_f0_phase_beats_one_pass_from_spsi(geom, signal, mel):
    c = E.value_case(*geom, signal, mel, iters10=True)
    print("sc after 0 / 10 iterations: F0 %.3f / %.3f, SPSI %.3f / %.3f; seeded after 5: %.3f"
          % (c["sc_f0_0"], c["sc_f0_10"], c["sc_spsi_0"], c["sc_spsi_10"], c["sc_seed_5"]))
    assert c["sc_f0_0"] < c["sc_spsi_0"]


@pytest.mark.parametrize("geom", E.VALUE_GEOMS, ids=lambda g: "%d_%d_%d" % g)
def test_the_one_pass_waveform_has_the_commanded_pitch(geom):
    c = E.value_case(*geom, "speech", True)
    est = P.pitch(c["wav_f0_0"], *geom, E.SR).f0
    worst, left_out, dev = E.pitch_true(c["f0"], est, geom[0], geom[1])
    print("worst deviation %.4f, median %.4f over %d frames; left out %.3f" % (worst, float(np.median(dev)), dev.size, left_out))
    assert dev.size > 0 and worst <= 0.03 and left_out <= 0.10


# ---- 4. the interface, without a GPU ----
NAMES = ("fs2_op_f0_phase_workspace_bytes_geom", "fs2_op_f0_phase_workspace_bytes_cap", "fs2_op_f0_phase_geom", "fs2_op_f0_phase_dev",
         "fs2_op_excitation_geom", "fs2_op_excitation_dev")


def test_symbols_and_abi_version(lib):
    from fastspeech2_amd import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.fs2_abi_version() == 4
    import fastspeech2_amd as fs
    from fastspeech2_amd import vocoder as V
    assert "f0" in V.INITS and callable(fs.f0_phase) and callable(fs.excitation)


def _i32s(v):
    return (C.c_int32 * len(v))(*v)


def test_workspace_queries(lib):
    q, qc = lib.fs2_op_f0_phase_workspace_bytes_geom, lib.fs2_op_f0_phase_workspace_bytes_cap
    a = q(*G, 2, _i32s((10, 5)))
    assert a > 0 and a % 256 == 0 and a == qc(*G, 2, 15)               # a host plan and the capacities it fills: the same layout
    assert a >= 15 * 256 * 4 + 15 * 8 + 1024 * 12                      # the excitation, Theta, the tables
    assert q(*G, 3, _i32s((10, 0, 5))) > a - 256 and q(*G, 0, None) > 0
    assert q(1000, 256, 1000, 80, 2, _i32s((10, 5))) == 0 and q(*G, 2, _i32s((10, -1))) == 0 and q(*G, 2, None) == 0
    assert qc(*G, 0, 15) == 0 and qc(*G, 2, 0) == 0 and qc(*G, 2, 2 ** 31 // 513 + 1) == 0
    assert qc(2048, 2048, 2048, 80, 2, 2 ** 31 // 2048 + 1) == 0       # hop * frame_capacity must index with an int


def _host(name, g=G, f0=PTR, lens=(10, 5), floor=71.0, ceil=800.0, sr=22050, ws=PTR, ws_bytes=0, out=PTR, B=None):
    starts = None if lens is None else _i32s(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist())
    return name, (None,) + tuple(g) + (f0, len(lens) if B is None else B, starts, None if lens is None else _i32s(lens), floor, ceil, sr, 0, ws, ws_bytes, out)


def _dev(name, g=G, f0=PTR, B=2, lens_dev=PTR, stride=0, cap=15, floor=71.0, ceil=800.0, sr=22050, ws=PTR, ws_bytes=0, out=PTR, wav=(0, 15 * 256)):
    tail = wav if name.startswith("fs2_op_excitation") else ()
    return name, (None,) + tuple(g) + (f0, B, lens_dev, stride, cap, None, floor, ceil, sr, 0, ws, ws_bytes, out) + tuple(tail)


@pytest.mark.parametrize("kind", ["f0_phase", "excitation"])
def test_refusals_of_the_entry_points(lib, kind):
    h = lambda **kw: _host("fs2_op_%s_geom" % kind, **kw)
    d = lambda **kw: _dev("fs2_op_%s_dev" % kind, **kw)
    need = int(lib.fs2_op_f0_phase_workspace_bytes_geom(*G, 2, _i32s((10, 5))))
    cases = []
    for c in (h, d):
        cases += [(c(sr=0), FS2_ERR_ARG, "sample_rate"), (c(floor=0.0), FS2_ERR_ARG, "f0_floor"), (c(floor=-5.0), FS2_ERR_ARG, "f0_floor"),
                  (c(floor=900.0), FS2_ERR_ARG, "f0_ceil"), (c(ceil=float("inf")), FS2_ERR_ARG, "f0_ceil"), (c(floor=float("nan")), FS2_ERR_ARG, "f0_floor"),
                  (c(g=(1000, 256, 1000, 80)), FS2_ERR_UNSUPPORTED, "n_fft"), (c(f0=None), FS2_ERR_ARG, "null pointer"),
                  (c(out=None), FS2_ERR_ARG, "null pointer"), (c(ws=None), FS2_ERR_ARG, "null pointer"),
                  (c(ws_bytes=need - 1), FS2_ERR_WORKSPACE, "workspace")]
    cases += [(h(lens=None, B=2), FS2_ERR_ARG, "null starts / lens"), (h(lens=(10, -1)), FS2_ERR_ARG, "negative length"),
              (h(lens=(0, 0), f0=None, out=None, ws=None), FS2_OK, None), (h(lens=(), f0=None, out=None, ws=None), FS2_OK, None),
              (d(B=0), FS2_ERR_ARG, "B 0"), (d(cap=0), FS2_ERR_ARG, "frame_capacity 0"), (d(stride=-1), FS2_ERR_ARG, "src_stride -1"),
              (d(lens_dev=None), FS2_ERR_ARG, "null pointer"), (d(cap=2 ** 31 // 513 + 1), FS2_ERR_ARG, "frame_capacity")]
    if kind == "excitation":
        cases += [(d(wav=(-1, 100)), FS2_ERR_ARG, "wav_stride -1"), (d(wav=(0, -1)), FS2_ERR_ARG, "wav_capacity"), (d(wav=(4096, 4096)), FS2_ERR_ARG, "wav_stride")]
    for (name, args), rc, text in cases:
        got = getattr(lib, name)(*args)
        msg = lib.fs2_last_error(None).decode() if got != FS2_OK else ""
        assert got == rc, (name, args[5:], got, msg)
        assert text is None or (text in msg and name in msg), (name, text, msg)


def test_argument_errors_of_the_python_layer():
    import torch
    from fastspeech2_amd import vocoder as V
    gl = V.GriffinLim()
    mel, f = torch.zeros(4, 80), torch.full((4,), 200.0)
    with pytest.raises(ValueError, match="init must be one of"):
        gl(mel, [4], init="pitch")
    with pytest.raises(ValueError, match="needs f0"):
        gl(mel, [4], init="f0")
    with pytest.raises(ValueError, match="needs f0"):
        gl(mel, torch.tensor([4]), init="f0", sync=False)
    with pytest.raises(ValueError, match="not both"):
        gl(mel, [4], init="f0", f0=f, init_phase=torch.zeros(4, 513))
    with pytest.raises(ValueError, match="not both"):
        gl(mel, [4], f0=f, init_phase=torch.zeros(4, 513))
    with pytest.raises(ValueError, match="belongs to init='f0'"):
        gl(mel, [4], init="spsi", f0=f)
    for lo, hi in ((0.0, 800.0), (-1.0, 800.0), (71.0, float("inf")), (900.0, 800.0), (float("nan"), 800.0)):
        with pytest.raises(ValueError, match="f0_floor"):
            gl(mel, [4], init="f0", f0=f, f0_floor=lo, f0_ceil=hi)
        with pytest.raises(ValueError, match="f0_floor"):
            V.f0_phase(f, [4], f0_floor=lo, f0_ceil=hi)
        with pytest.raises(ValueError, match="f0_floor"):
            V.excitation(f, [4], f0_floor=lo, f0_ceil=hi)
    for call in (lambda: gl(mel, [4], init="f0", f0=f), lambda: V.f0_phase(f, [4]), lambda: V.excitation(f, [4])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="float32 CUDA tensor"):
        V.f0_phase([200.0] * 4, [4])


def test_the_pitch_forms_are_refused_with_a_reduction_factor():
    import torch
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    hp = default_hparams()
    hp.model.reduction_factor = 2
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    if model.reduction_factor != 2:
        pytest.fail("the hyper-parameters did not set reduction_factor")
    with pytest.raises(ValueError, match="reduction_factor > 1"):
        model.inference_batch_pitch(torch.zeros(1, 3, dtype=torch.long), [3])
    with pytest.raises(ValueError, match="reduction_factor > 1"):
        model.capture_graph(torch.zeros(1, 3, dtype=torch.long), [3], vocoder=object(), init="f0")
