"""GriffinLim makes every library call from one place (GriffinLim._launch, from the plan of fastspeech2_amd/_vocode_plan.py).  Here each of
the calls it can make is made once through the Python API and once directly through ctypes, with every argument written out longhand
(nothing is taken from the entry table or from a plan), and every output must agree bit for bit: the waveform or phase, the magnitudes
where asked for, ``sample_lens`` and ``status`` of the device forms.  A swapped stride and capacity, a dropped seed mask, a basis in the
place of pinv or a permuted geometry shows here.

Shapes: lens (6, 1, 4) -- at the default geometry one utterance above L_min = 4, one below, one at it -- packed, and padded at Lmax 7 (a
stride that equals no length); the default geometry and (512, 160, 400, 80), four different numbers; n_iter 2, momentum 0.99, a seed with
the top bit set; f0 of 0 on some frames and 120 .. 220 Hz on others; an upstream status once absent and once a zeroed int32[8]."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMS = [(1024, 256, 1024, 80), (512, 160, 400, 80)]
LENS, LMAX = (6, 1, 4), 7
N_ITER, MOMENTUM, SEED, SR = 2, 0.99, 0x9E3779B9, 22050
FLOOR, CEIL = 71.0, 800.0

_GL, _INPUTS = {}, {}


def gl_of(g):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    if g not in _GL:
        _GL[g] = GriffinLim(DotDict({"audio": {"n_fft": g[0], "hop_length": g[1], "win_length": g[2], "n_mels": g[3], "sample_rate": SR}}))
    return _GL[g]


def pad(x):
    out = torch.zeros((len(LENS), LMAX) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    row = 0
    for b, n in enumerate(LENS):
        out[b, :n] = x[row:row + n]
        row += n
    return out


def inputs(g, padded):
    """mels, magnitudes and f0 of the batch, packed [11, ..] or padded [3, 7, ..]; made once and never written."""
    if (g, padded) not in _INPUTS:
        gen = torch.Generator().manual_seed(17)
        N, NB = sum(LENS), g[0] // 2 + 1
        mels = torch.randn(N, g[3], generator=gen) - 3.0
        mags = torch.randn(N, NB, generator=gen).abs()
        f0 = 120.0 + 100.0 * torch.rand(N, generator=gen)
        f0[[1, 2, 6, 9]] = 0.0
        t = [x.cuda() for x in (mels, mags, f0)]
        _INPUTS[g, padded] = tuple(pad(x) for x in t) if padded else tuple(t)
    return _INPUTS[g, padded]


def i32(v):
    return (C.c_int32 * len(v))(*v)


def host_batch(padded):
    return i32([0, 7, 14] if padded else [0, 6, 7]), i32(LENS)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(n):
    return torch.empty(int(n), dtype=torch.uint8, device="cuda")


def f32(*shape, zero=False):
    return (torch.zeros if zero else torch.empty)(*shape, dtype=torch.float32, device="cuda")


def same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
        bits = torch.int32 if a.dtype == torch.float32 else a.dtype
        assert torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def lib_and_check():
    from fastspeech2_amd import _lib
    return _lib.lib(), _lib.check


def olens_dev():
    return torch.tensor(LENS, dtype=torch.int64, device="cuda")


def async_mels(mels, pitch=None):
    from fastspeech2_amd.fastspeech import AsyncMels
    return AsyncMels(mels, olens_dev(), torch.zeros(8, dtype=torch.int32, device="cuda"), None, pitch)


# ---- the two phase stages longhand (also the first half of the two-stage calls below) ----
def spsi_host_longhand(g, src, width, pinv, padded, want_mag):
    lib, check = lib_and_check()
    n_fft, hop, win, n_mels = g
    starts, lens = host_batch(padded)
    rows = 21 if padded else 11
    phase, mag = f32(rows, n_fft // 2 + 1, zero=True), f32(rows, n_fft // 2 + 1, zero=True) if want_mag else None
    ws = workspace(lib.fs2_op_spsi_workspace_bytes_geom(n_fft, hop, win, n_mels, 3, lens))
    check(lib.fs2_op_spsi_phase_geom(stream(), n_fft, hop, win, n_mels, src.data_ptr(), width, pinv.data_ptr() if pinv is not None else None, 3, starts,
                                     lens, ws.data_ptr(), ws.numel(), phase.data_ptr(), mag.data_ptr() if want_mag else None))
    return phase, mag


def spsi_dev_longhand(g, src, width, pinv, padded, upstream, want_mag, cap=None):
    lib, check = lib_and_check()
    n_fft, hop, win, n_mels = g
    rows = 21 if padded else 11
    cap = rows if cap is None else cap
    ol = olens_dev()
    phase, mag = f32(rows, n_fft // 2 + 1, zero=True), f32(rows, n_fft // 2 + 1, zero=True) if want_mag else None
    ws = workspace(lib.fs2_op_spsi_workspace_bytes_cap(n_fft, hop, win, n_mels, 3, cap))
    check(lib.fs2_op_spsi_phase_dev(stream(), n_fft, hop, win, n_mels, src.data_ptr(), width, pinv.data_ptr() if pinv is not None else None, 3,
                                    ol.data_ptr(), 7 if padded else 0, cap, upstream.data_ptr() if upstream is not None else None, ws.data_ptr(),
                                    ws.numel(), phase.data_ptr(), mag.data_ptr() if want_mag else None))
    return phase, mag


def f0_host_longhand(g, f0, padded, excitation=False):
    lib, check = lib_and_check()
    n_fft, hop, win, n_mels = g
    starts, lens = host_batch(padded)
    out = f32(hop * (5 + 0 + 3)) if excitation else f32(21 if padded else 11, n_fft // 2 + 1, zero=True)
    ws = workspace(lib.fs2_op_f0_phase_workspace_bytes_geom(n_fft, hop, win, n_mels, 3, lens))
    call = lib.fs2_op_excitation_geom if excitation else lib.fs2_op_f0_phase_geom
    check(call(stream(), n_fft, hop, win, n_mels, f0.data_ptr(), 3, starts, lens, FLOOR, CEIL, SR, SEED, ws.data_ptr(), ws.numel(), out.data_ptr()))
    return out


def f0_dev_longhand(g, f0, padded, upstream, cap=None):
    lib, check = lib_and_check()
    n_fft, hop, win, n_mels = g
    rows = 21 if padded else 11
    cap = rows if cap is None else cap
    ol = olens_dev()
    phase = f32(rows, n_fft // 2 + 1, zero=True)
    ws = workspace(lib.fs2_op_f0_phase_workspace_bytes_cap(n_fft, hop, win, n_mels, 3, cap))
    check(lib.fs2_op_f0_phase_dev(stream(), n_fft, hop, win, n_mels, f0.data_ptr(), 3, ol.data_ptr(), 7 if padded else 0, cap,
                                  upstream.data_ptr() if upstream is not None else None, FLOOR, CEIL, SR, SEED, ws.data_ptr(), ws.numel(),
                                  phase.data_ptr()))
    return phase


# ---- the four synthesis calls longhand ----
def synth_host_longhand(g, src, width, pinv, basis, padded, init_phase=None):
    """fs2_op_griffin_lim_geom, or with ``basis`` fs2_op_griffin_lim_mel_geom"""
    lib, check = lib_and_check()
    n_fft, hop, win, n_mels = g
    starts, lens = host_batch(padded)
    wav = f32(hop * (5 + 0 + 3))
    ip = init_phase.data_ptr() if init_phase is not None else None
    if basis is None:
        ws = workspace(lib.fs2_op_vocode_workspace_bytes_geom(n_fft, hop, win, n_mels, 3, lens))
        check(lib.fs2_op_griffin_lim_geom(stream(), n_fft, hop, win, n_mels, src.data_ptr(), width, pinv.data_ptr() if pinv is not None else None, 3,
                                          starts, lens, N_ITER, MOMENTUM, SEED, ip, ws.data_ptr(), ws.numel(), wav.data_ptr()))
    else:
        ws = workspace(lib.fs2_op_vocode_mel_workspace_bytes_geom(n_fft, hop, win, n_mels, 3, lens))
        check(lib.fs2_op_griffin_lim_mel_geom(stream(), n_fft, hop, win, n_mels, src.data_ptr(), width, pinv.data_ptr(), basis.data_ptr(), 3, starts, lens,
                                              N_ITER, MOMENTUM, SEED, ip, ws.data_ptr(), ws.numel(), wav.data_ptr()))
    return (wav,)


def synth_dev_longhand(g, src, width, pinv, basis, padded, upstream, init_phase=None, padded_out=False, cap=None):
    """fs2_op_griffin_lim_dev, or with ``basis`` fs2_op_griffin_lim_mel_dev -> (wav, sample_lens, status)"""
    lib, check = lib_and_check()
    n_fft, hop, win, n_mels = g
    cap = (21 if padded else 11) if cap is None else cap
    wav_stride = hop * 6 if padded_out else 0
    wav_cap = 3 * hop * 6 if padded_out else hop * (cap - 1)
    ol = olens_dev()
    wav, sample_lens, status = f32(wav_cap), torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda")
    ip = init_phase.data_ptr() if init_phase is not None else None
    up = upstream.data_ptr() if upstream is not None else None
    if basis is None:
        ws = workspace(lib.fs2_op_vocode_workspace_bytes_cap(n_fft, hop, win, n_mels, 3, cap))
        check(lib.fs2_op_griffin_lim_dev(stream(), n_fft, hop, win, n_mels, src.data_ptr(), width, pinv.data_ptr() if pinv is not None else None, 3,
                                         ol.data_ptr(), 7 if padded else 0, cap, up, N_ITER, MOMENTUM, SEED, ip, ws.data_ptr(), ws.numel(), wav.data_ptr(),
                                         wav_stride, wav_cap, sample_lens.data_ptr(), status.data_ptr()))
    else:
        ws = workspace(lib.fs2_op_vocode_mel_workspace_bytes_cap(n_fft, hop, win, n_mels, 3, cap))
        check(lib.fs2_op_griffin_lim_mel_dev(stream(), n_fft, hop, win, n_mels, src.data_ptr(), width, pinv.data_ptr(), basis.data_ptr(), 3, ol.data_ptr(),
                                             7 if padded else 0, cap, up, N_ITER, MOMENTUM, SEED, ip, ws.data_ptr(), ws.numel(), wav.data_ptr(),
                                             wav_stride, wav_cap, sample_lens.data_ptr(), status.data_ptr()))
    return (wav.reshape(3, wav_stride) if padded_out else wav), sample_lens, status


KW = dict(n_iter=N_ITER, momentum=MOMENTUM, seed=SEED)
FORMS = [(GEOMS[0], False), (GEOMS[0], True), (GEOMS[1], False)]
form_ids = ["default_packed", "default_padded", "512_160_400_packed"]


@pytest.mark.parametrize("g,padded", FORMS, ids=form_ids)
@pytest.mark.parametrize("mel", (False, True), ids=("magnitude", "mel"))
def test_host_synthesis(g, padded, mel):
    """fs2_op_griffin_lim_geom and fs2_op_griffin_lim_mel_geom"""
    gl = gl_of(g)
    mels, mags, _ = inputs(g, padded)
    pinv, basis = gl.constants(mels.device)
    w = gl(mels, list(LENS), constraint="mel" if mel else "magnitude", **KW)
    assert w.sample_lens.tolist() == [g[1] * 5, 0, g[1] * 3]
    same((w.wav,), synth_host_longhand(g, mels, g[3], pinv, basis if mel else None, padded))
    if not mel:      # a magnitude source: 513 (257) columns and no pinv
        w = gl(mags, list(LENS), magnitudes=True, **KW)
        same((w.wav,), synth_host_longhand(g, mags, g[0] // 2 + 1, None, None, padded))


@pytest.mark.parametrize("g,padded", FORMS, ids=form_ids)
@pytest.mark.parametrize("mel", (False, True), ids=("magnitude", "mel"))
@pytest.mark.parametrize("upstream", (False, True), ids=("no_upstream", "upstream"))
def test_device_synthesis(g, padded, mel, upstream):
    """fs2_op_griffin_lim_dev and fs2_op_griffin_lim_mel_dev"""
    gl = gl_of(g)
    mels, _, _ = inputs(g, padded)
    pinv, basis = gl.constants(mels.device)
    con = "mel" if mel else "magnitude"
    a = async_mels(mels) if upstream else None
    w = gl(a, sync=False, constraint=con, **KW) if upstream else gl(mels, olens_dev(), sync=False, constraint=con, **KW)
    want = synth_dev_longhand(g, mels, g[3], pinv, basis if mel else None, padded, a.status if upstream else None)
    same((w.wav, w.sample_lens, w.status), want)
    assert w.sample_lens.tolist() == [g[1] * 5, 0, g[1] * 3] and w.ok()
    # an explicit capacity (padded: 12, below the 21 rows and above the 11 frames), and the padded output
    cap = 12 if padded else 11
    w = gl(mels, olens_dev(), sync=False, constraint=con, capacity=cap, **KW)
    same((w.wav, w.sample_lens, w.status), synth_dev_longhand(g, mels, g[3], pinv, basis if mel else None, padded, None, cap=cap))
    if padded:
        w = gl(mels, olens_dev(), sync=False, constraint=con, padded_out=True, **KW)
        same((w.wav, w.sample_lens, w.status), synth_dev_longhand(g, mels, g[3], pinv, basis if mel else None, padded, None, padded_out=True))
        assert w.wav.shape == (3, g[1] * 6) and w.padded


@pytest.mark.parametrize("g,padded", FORMS, ids=form_ids)
def test_spsi_phase_both_forms(g, padded):
    """fs2_op_spsi_phase_geom and fs2_op_spsi_phase_dev"""
    gl = gl_of(g)
    mels, mags, _ = inputs(g, padded)
    pinv = gl.constants(mels.device)[0]
    NB = g[0] // 2 + 1
    shape = ((3, 7) if padded else (11,)) + (NB,)
    reshaped = lambda outs: [o.reshape(shape) for o in outs if o is not None]
    same(gl.spsi_phase(mels, list(LENS), return_magnitudes=True), reshaped(spsi_host_longhand(g, mels, g[3], pinv, padded, True)))
    same([gl.spsi_phase(mags, list(LENS), magnitudes=True)], reshaped(spsi_host_longhand(g, mags, NB, None, padded, False)))
    same(gl.spsi_phase(mels, olens_dev(), return_magnitudes=True, sync=False), reshaped(spsi_dev_longhand(g, mels, g[3], pinv, padded, None, True)))
    a = async_mels(mels)
    same([gl.spsi_phase(a, sync=False)], reshaped(spsi_dev_longhand(g, mels, g[3], pinv, padded, a.status, False)))
    same([gl.spsi_phase(mags, olens_dev(), magnitudes=True, sync=False)], reshaped(spsi_dev_longhand(g, mags, NB, None, padded, None, False)))


@pytest.mark.parametrize("g,padded", FORMS, ids=form_ids)
def test_f0_phase_both_forms_and_the_excitation(g, padded):
    """fs2_op_f0_phase_geom, fs2_op_f0_phase_dev and fs2_op_excitation_geom"""
    gl = gl_of(g)
    mels, _, f0 = inputs(g, padded)
    NB = g[0] // 2 + 1
    shape = ((3, 7) if padded else (11,)) + (NB,)
    opt = dict(f0_floor=FLOOR, f0_ceil=CEIL, seed=SEED)
    same([gl.f0_phase(f0, list(LENS), **opt)], [f0_host_longhand(g, f0, padded).reshape(shape)])
    same([gl.f0_phase(f0, olens_dev(), sync=False, **opt)], [f0_dev_longhand(g, f0, padded, None).reshape(shape)])
    a = async_mels(mels, f0)
    same([gl.f0_phase(a, sync=False, **opt)], [f0_dev_longhand(g, f0, padded, a.status).reshape(shape)])
    w = gl.excitation(f0, list(LENS), **opt)
    assert w.sample_lens.tolist() == [g[1] * 5, 0, g[1] * 3]
    same([w.wav], [f0_host_longhand(g, f0, padded, excitation=True)])
    assert float(w.wav.abs().max()) > 0


@pytest.mark.parametrize("g,padded", FORMS, ids=form_ids)
@pytest.mark.parametrize("mel", (False, True), ids=("magnitude", "mel"))
def test_the_two_stage_calls_are_the_two_calls_in_sequence(g, padded, mel):
    """init="spsi" and init="f0", host-planned and device-driven: the phase stage longhand, then the synthesis longhand from its phase"""
    gl = gl_of(g)
    mels, _, f0 = inputs(g, padded)
    pinv, basis = gl.constants(mels.device)
    b = basis if mel else None
    con = "mel" if mel else "magnitude"
    w = gl(mels, list(LENS), init="spsi", constraint=con, **KW)
    same((w.wav,), synth_host_longhand(g, mels, g[3], pinv, b, padded, spsi_host_longhand(g, mels, g[3], pinv, padded, False)[0]))
    w = gl(mels, list(LENS), init="f0", f0=f0, f0_floor=FLOOR, f0_ceil=CEIL, constraint=con, **KW)
    same((w.wav,), synth_host_longhand(g, mels, g[3], pinv, b, padded, f0_host_longhand(g, f0, padded)))
    cap = 12 if padded else 11
    w = gl(mels, olens_dev(), sync=False, init="spsi", capacity=cap, constraint=con, **KW)
    phase = spsi_dev_longhand(g, mels, g[3], pinv, padded, None, False, cap=cap)[0]
    same((w.wav, w.sample_lens, w.status), synth_dev_longhand(g, mels, g[3], pinv, b, padded, None, phase, cap=cap))
    a = async_mels(mels, f0)
    w = gl(a, sync=False, init="f0", f0_floor=FLOOR, f0_ceil=CEIL, constraint=con, **KW)
    phase = f0_dev_longhand(g, f0, padded, a.status)
    same((w.wav, w.sample_lens, w.status), synth_dev_longhand(g, mels, g[3], pinv, b, padded, a.status, phase))
    assert w.ok()
