"""Mel-constrained Griffin-Lim without a GPU: the float64 oracle (tests/mel_gl_oracle.py) and what the
method gains in it, and the host side of fs2_op_griffin_lim_mel_geom / _dev -- exported names, workspace queries and the calls refused
before any launch (fake pointers, as in test_vocoder_async_host.py: no call below gets as far as using one)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mel_gl_oracle as MO
from tests import vocoder_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = [(1024, 256, 1024), (2048, 300, 1200), (512, 160, 400), (1024, 200, 800)]
NEW = ("fs2_op_vocode_mel_workspace_bytes_geom", "fs2_op_griffin_lim_mel_geom", "fs2_op_vocode_mel_workspace_bytes_cap",
       "fs2_op_griffin_lim_mel_dev")


@pytest.fixture(scope="module")
def lib():
    from fastspeech2_amd import _lib
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def default():
    """(Stft, basis, pinv) of the default transform, and per f0 the log-mel of a 61-frame harmonic signal with noise."""
    from fastspeech2_amd.vocoder import mel_basis
    st = O.Stft()
    B = mel_basis()
    mels = {f0: MO.log_mel(st, O.harmonic_signal(256 * 60, seed=k, f0=f0, noise=0.05), B) for k, f0 in enumerate((120.0, 220.0, 330.0))}
    return st, B, np.linalg.pinv(B), mels


def test_zero_iterations_is_the_plain_oracle(default):
    from fastspeech2_amd.vocoder import seed_angles
    st, B, pinv, mels = default
    mel = mels[220.0]
    ang = seed_angles(4, mel.shape[0])
    assert np.array_equal(MO.griffin_lim_mel(st, mel, B, pinv, ang, 0), st.griffin_lim(O.mel_to_mag(mel, pinv), ang, 0))
    short = mel[:3]
    assert np.array_equal(MO.griffin_lim_mel(st, short, B, pinv, ang[:3], 5), np.zeros(512))


def test_projection_gives_the_mel_it_was_given(default):
    """One projection of a spectrum whose bands are all alive reproduces exp(mel) wherever a band's bins belong to it alone, and moves
    every band towards it; the bins above fmax, which no filter covers, go to zero."""
    st, B, pinv, mels = default
    rng = np.random.default_rng(0)
    A = rng.standard_normal((5, 513)) + 1j * rng.standard_normal((5, 513))
    mel = mels[120.0][:5]
    P = MO.mel_project(A, mel, B)
    assert np.array_equal(P[:, B.sum(axis=0) == 0], np.zeros((5, int((B.sum(axis=0) == 0).sum()))))
    assert (B.sum(axis=0) == 0).sum() > 100                                   # fmax 8000 of 11025 Hz
    before, after = np.abs(np.log(np.abs(A) @ B.T) - mel).mean(), np.abs(np.log(np.abs(P) @ B.T) - mel).mean()
    assert after < 0.2 * before, (before, after)
    assert np.allclose(np.angle(P[np.abs(P) > 0]), np.angle(A[np.abs(P) > 0]))


def test_mel_error_is_three_quarters_of_the_plain_loops_or_less(default):
    from fastspeech2_amd.vocoder import seed_angles
    st, B, pinv, mels = default
    for f0, mel in mels.items():
        ang = seed_angles(0, mel.shape[0])
        plain = st.griffin_lim(O.mel_to_mag(mel, pinv), ang, 30)
        con = MO.griffin_lim_mel(st, mel, B, pinv, ang, 30)
        e0, e1 = MO.mel_error(st, plain, mel, B), MO.mel_error(st, con, mel, B)
        print("f0 %g: mean |log-mel error| plain %.4f, mel-constrained %.4f, ratio %.3f" % (f0, e0, e1, e1 / e0))
        assert e1 <= 0.75 * e0, (f0, e0, e1)


def test_silent_frames_stay_finite_and_near_zero(default):
    from fastspeech2_amd.vocoder import seed_angles
    st, B, pinv, mels = default
    mel = mels[220.0][:20].copy()
    mel[5:12] = np.log(1e-5)
    silent = np.full((12, 80), np.log(1e-5))
    for m, mom in ((mel, 0.0), (mel, 0.99), (silent, 0.0)):
        sig = MO.griffin_lim_mel(st, m, B, pinv, seed_angles(1, m.shape[0]), 8, momentum=mom)
        assert np.isfinite(sig).all()
    # all-silent input: a band of a Slaney basis sums to 1 / (bin width in Hz) = 1024 / 22050, so a band energy of 1e-5 is a magnitude
    # of about 2.2e-4 per bin, and 373 such bins bound a sample by 2 . 373 . 2.2e-4 / 1024 = 1.6e-4
    assert np.abs(sig).max() <= 1e-3, np.abs(sig).max()
    # a spectrum that is exactly zero stays zero (no division by |A|), and the cap bounds the gain of a dead band
    Z = MO.mel_project(np.zeros((2, 513), complex), mel[:2], B)
    assert not Z.any()
    tiny = MO.mel_project(np.full((1, 513), 1e-30 + 0j), mel[:1], B)
    assert np.isfinite(tiny).all() and np.abs(tiny).max() <= MO.R_CAP * 1e-30 * (1 + 1e-12)


def test_names_are_declared_exported_and_bound(lib):
    from fastspeech2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fs2.h")).read()
    declared = set(re.findall(r"\b(fs2_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define FS2_ABI_VERSION (\d+)", hdr).group(1)) == 4 == _lib.ABI_VERSION


def _band_bytes(n_fft):
    # row ranges (int2 x 128), bin ranges (int2 x bins), 1 / w (float x bins), the shifted transposed basis (float x bins x 128)
    return 128 * 8 + (n_fft // 2 + 1) * (12 + 128 * 4)


def test_workspace_is_the_plain_one_plus_the_band_tables(lib):
    """The band tables are one 256-aligned region at the end of the plain layout (whose own end is 256-aligned), in both forms."""
    up = lambda n: -(-n // 256) * 256
    rng = np.random.default_rng(5)
    n = 0
    for n_fft, hop, win in GEOMS:
        g = (n_fft, hop, win, 80)
        for B in (1, 3, 64):
            for hi in (4, 70, 400):
                L = rng.integers(0, hi, size=B)
                Lc = (C.c_int32 * B)(*L.tolist())
                plain = int(lib.fs2_op_vocode_workspace_bytes_geom(*g, B, Lc))
                assert int(lib.fs2_op_vocode_mel_workspace_bytes_geom(*g, B, Lc)) == plain + up(_band_bytes(n_fft)) and plain % 256 == 0
                cap = int(L.sum())
                plain = int(lib.fs2_op_vocode_workspace_bytes_cap(*g, B, cap))
                assert int(lib.fs2_op_vocode_mel_workspace_bytes_cap(*g, B, cap)) == (plain + up(_band_bytes(n_fft)) if plain else 0)
                n += 2
    assert n == 72
    q, qc = lib.fs2_op_vocode_mel_workspace_bytes_geom, lib.fs2_op_vocode_mel_workspace_bytes_cap
    for bad in ((1000, 256, 1000, 80), (1024, 100, 1024, 80), (1024, 512, 256, 80), (1024, 256, 2048, 80), (1024, 256, 1024, 129)):
        assert q(*bad, 1, (C.c_int32 * 1)(10)) == 0 and qc(*bad, 1, 10) == 0
    assert q(1024, 256, 1024, 80, 1, (C.c_int32 * 1)(-1)) == 0 and qc(1024, 256, 1024, 80, -1, 10) == 0
    assert qc(1024, 256, 1024, 80, 4, 2 ** 31 // 513 + 1) == 0


OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -5, -6      # include/fs2.h
PTR = 0x1000
DEFAULT_G = (1024, 256, 1024, 80)


def _i32s(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def _host_call(g=DEFAULT_G, src=PTR, width=80, pinv=PTR, basis=PTR, B=None, lens=(10, 5), n_iter=2, momentum=0.0, ws=PTR, ws_bytes=0, wav=PTR):
    B = (0 if lens is None else len(lens)) if B is None else B
    starts = None if lens is None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    return "fs2_op_griffin_lim_mel_geom", (None,) + tuple(g) + (src, width, pinv, basis, B, _i32s(starts), _i32s(lens), n_iter, momentum, 0, None,
                                                               ws, ws_bytes, wav)


def _dev_call(g=DEFAULT_G, src=PTR, width=80, pinv=PTR, basis=PTR, B=2, lens_dev=PTR, src_stride=0, frame_capacity=15, n_iter=2, momentum=0.0,
              ws=PTR, ws_bytes=0, wav=PTR, wav_stride=0, wav_capacity=256 * 14, sample_lens=PTR, status=PTR):
    return "fs2_op_griffin_lim_mel_dev", (None,) + tuple(g) + (src, width, pinv, basis, B, lens_dev, src_stride, frame_capacity, None, n_iter, momentum,
                                                              0, None, ws, ws_bytes, wav, wav_stride, wav_capacity, sample_lens, status)


def _calls(lib):
    """(label, function, arguments, code).  Every call passes a workspace below what it needs, the last thing either path checks: one
    that passed the check it is here for would still end with FS2_ERR_WORKSPACE and launch nothing."""
    h, d = _host_call, _dev_call
    need = int(lib.fs2_op_vocode_mel_workspace_bytes_geom(*DEFAULT_G, 2, _i32s((10, 5))))
    need_d = int(lib.fs2_op_vocode_mel_workspace_bytes_cap(*DEFAULT_G, 2, 15))
    plain = int(lib.fs2_op_vocode_workspace_bytes_geom(*DEFAULT_G, 2, _i32s((10, 5))))
    for e, c, nd in (("host", h, need), ("dev", d, need_d)):
        yield ("magnitude source", e) + c(width=513) + (ERR_ARG,)
        yield ("magnitude source without pinv", e) + c(width=513, pinv=None) + (ERR_ARG,)
        yield ("null basis", e) + c(basis=None) + (ERR_ARG,)
        yield ("src_width", e) + c(width=100) + (ERR_UNSUPPORTED,)
        yield ("mel without pinv", e) + c(pinv=None) + (ERR_ARG,)
        yield ("n_iter < 0", e) + c(n_iter=-1) + (ERR_ARG,)
        yield ("momentum nan", e) + c(momentum=float("nan")) + (ERR_ARG,)
        yield ("null src", e) + c(src=None) + (ERR_ARG,)
        yield ("null wav", e) + c(wav=None) + (ERR_ARG,)
        yield ("null workspace", e) + c(ws=None) + (ERR_ARG,)
        yield ("workspace one byte short", e) + c(ws_bytes=nd - 1) + (ERR_WORKSPACE,)
        yield ("geometry", e) + c(g=(1000, 256, 1000, 80), src=None, basis=None) + (ERR_UNSUPPORTED,)
    yield ("the plain call's workspace is too small", "host") + h(ws_bytes=plain) + (ERR_WORKSPACE,)
    yield ("null starts / lens", "host") + h(lens=None, B=2) + (ERR_ARG,)
    yield ("negative length", "host") + h(lens=(10, -1)) + (ERR_ARG,)
    yield ("B = 0", "host") + h(lens=None, src=None, wav=None, ws=None) + (OK,)
    yield ("nobody owns a sample", "host") + h(lens=(1, 0, 1), src=None, wav=None, ws=None) + (OK,)
    yield ("B = 0", "dev") + d(B=0) + (ERR_ARG,)
    yield ("frame_capacity 0", "dev") + d(frame_capacity=0) + (ERR_ARG,)
    yield ("null lens_dev", "dev") + d(lens_dev=None) + (ERR_ARG,)
    yield ("null status", "dev") + d(status=None) + (ERR_ARG,)
    yield ("padded output beyond wav", "dev") + d(wav_stride=256 * 7 + 1) + (ERR_ARG,)


def test_calls_refused_before_a_launch(lib):
    n = 0
    for label, where, fn, args, want in _calls(lib):
        got = int(getattr(lib, fn)(*args))
        assert got == want, (label, where, fn, got, want)
        if want != OK:
            assert lib.fs2_last_error(None), (label, where)
        n += 1
    assert n >= 34


def test_python_argument_checks_need_no_gpu():
    from fastspeech2_amd.vocoder import CONSTRAINTS, GriffinLim
    assert CONSTRAINTS == ("magnitude", "mel")
    gl = GriffinLim()
    assert (gl._basis_np >= 0).all()
    with pytest.raises(ValueError, match="no mel to constrain to"):
        gl(torch.zeros(10, 513), [10], magnitudes=True, constraint="mel")
    with pytest.raises(ValueError, match="no mel to constrain to"):
        gl(torch.zeros(10, 513), torch.tensor([10]), magnitudes=True, constraint="mel", sync=False)
    with pytest.raises(ValueError, match="constraint must be one of"):
        gl(torch.zeros(10, 80), [10], constraint="linear")
    # the constraint changes no other check: a CPU tensor is refused as before
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(torch.zeros(10, 80), [10], constraint="mel")
    with pytest.raises(TypeError, match="olens must be a CUDA int64 tensor"):
        gl(torch.zeros(10, 80), [10], constraint="mel", sync=False)
