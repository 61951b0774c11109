"""Griffin-Lim and the analysis STFT at other transform geometries on the MI355X (fs2_op_griffin_lim_geom / fs2_op_stft_geom)
against the generic float64 oracle (tests/vocoder_oracle.py) and the reference's recordings (tests/golden/g11_stft_geometries.npz;
g10_griffin_lim.npz at the default geometry, run here through the new entry points).  The bars are those of test_gpu_vocoder.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import vocoder_oracle as O

pytestmark = pytest.mark.gpu

FIXTURE = [(1024, 256, 1024), (2048, 300, 1200), (512, 160, 400), (1024, 200, 800)]
ALL = FIXTURE + [(512, 128, 512), (2048, 512, 2048)]
SR = {(2048, 300, 1200): 24000}


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


def _tag(geom):
    return "%d_%d_%d" % geom


def _hp(geom, n_mels=80):
    from fastspeech2_amd.hparams import DotDict
    n_fft, hop, win = geom
    return DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "n_mels": n_mels,
                              "sample_rate": SR.get(geom, 22050)}})


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    """geometry -> dict(signal, magnitudes, angles, wav_iter0/1/30, energy) recorded from the reference."""
    g11 = dict(np.load(os.path.join(golden_dir, "g11_stft_geometries.npz")))
    out = {}
    for geom in FIXTURE[1:]:
        k = _tag(geom) + "/"
        out[geom] = {a[len(k):]: b for a, b in g11.items() if a.startswith(k)}
    g10 = dict(np.load(os.path.join(golden_dir, "g10_griffin_lim.npz")))
    g10["energy"] = torch.norm(torch.from_numpy(g10["magnitudes"]).T, dim=0).numpy()     # the reference's torch.norm(mag, dim=0)
    out[FIXTURE[0]] = g10
    return out


def _fixture_or_synthetic(fixtures, geom):
    if geom in fixtures:
        return fixtures[geom]
    from fastspeech2_amd.vocoder import seed_angles
    n_fft, hop, win = geom
    sig = O.harmonic_signal(43 * hop, seed=3, noise=0.01, sr=SR.get(geom, 22050))
    M = np.abs(O.Stft(*geom).stft(sig)).astype(np.float32)
    return dict(signal=sig.astype(np.float32), magnitudes=M, angles=seed_angles(4, M.shape[0], n_fft // 2 + 1))


@pytest.mark.parametrize("geom", ALL, ids=_tag)
def test_istft_alone_matches_oracle(fixtures, geom):
    from fastspeech2_amd.vocoder import GriffinLim
    gl = GriffinLim(_hp(geom))
    d = _fixture_or_synthetic(fixtures, geom)
    M, A = d["magnitudes"], d["angles"]
    w = gl(_cuda(M), [M.shape[0]], n_iter=0, init_phase=_cuda(A), magnitudes=True)
    got = w.wav.cpu().numpy().astype(np.float64)
    want = O.Stft(*geom).griffin_lim(M, A, 0)
    err = np.abs(got - want).max() / np.abs(want).max()
    _record("vocoder_geom_%s_istft_rel" % _tag(geom), err)
    assert got.shape == want.shape and int(w.sample_lens[0]) == want.size == geom[1] * (M.shape[0] - 1)
    assert err <= 1e-6, err


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("geom", ALL, ids=_tag)
def test_stft_magnitude_logmel_energy_match_oracle(fixtures, geom, n_mels):
    from fastspeech2_amd.vocoder import GriffinLim, mel_energy, stft_magnitude
    n_fft, hop, win = geom
    hp = _hp(geom, n_mels)
    o = O.Stft(*geom)
    sig = _fixture_or_synthetic(fixtures, geom)["signal"]
    wavs = [sig, sig[:int(0.6 * sig.size)] * 0.5, O.harmonic_signal(2 * n_fft + 37, seed=5)]
    T = [x.size for x in wavs]
    packed = _cuda(np.concatenate(wavs))
    mag = stft_magnitude(packed, T, hp=hp)
    logmel = stft_magnitude(packed, T, mel=True, hp=hp)
    lm2, en = mel_energy(packed, T, hp=hp)
    assert torch.equal(lm2, logmel)
    mag, logmel, en = (t.cpu().numpy().astype(np.float64) for t in (mag, logmel, en))
    want = np.concatenate([np.abs(o.stft(np.asarray(x, np.float64))) for x in wavs])
    assert mag.shape == want.shape == (sum(t // hop + 1 for t in T), n_fft // 2 + 1)
    assert logmel.shape == (want.shape[0], n_mels) and en.shape == (want.shape[0],)
    err = np.abs(mag - want).max() / np.abs(want).max()
    _record("vocoder_geom_%s_stft_rel" % _tag(geom), err)
    assert err <= 5e-7, err
    basis = GriffinLim(hp)._basis_np
    mel_want = want @ basis.T
    merr = np.abs(np.exp(logmel) - np.maximum(mel_want, 1e-5)).max() / mel_want.max()
    _record("vocoder_geom_%s_mel%d_rel" % (_tag(geom), n_mels), merr)
    assert merr <= 1e-6, merr
    big = mel_want >= 1e-2 * mel_want.max()
    lerr = np.abs(logmel - np.log(mel_want))[big].max()
    _record("vocoder_geom_%s_logmel%d_abs_big" % (_tag(geom), n_mels), lerr)
    assert lerr <= 1e-4, lerr
    # energy: the norm of the kernel's own |X| (same launch), and the oracle within 2x the reference's own fp32 distance to it
    assert np.abs(en - np.linalg.norm(mag, axis=1)).max() <= 1e-6 * en.max()
    d = fixtures.get(geom)
    if d is not None:
        e_or = o.energy(np.asarray(d["signal"], np.float64))
        lm_f, en_f = mel_energy(_cuda(d["signal"]), [d["signal"].size], hp=hp)
        e_gpu = en_f.cpu().numpy().astype(np.float64)
        ref_err = np.abs(d["energy"].astype(np.float64) - e_or).max() / e_or.max()
        gpu_err = np.abs(e_gpu - e_or).max() / e_or.max()
        _record("vocoder_geom_%s_energy_rel" % _tag(geom), gpu_err)
        _record("vocoder_geom_%s_energy_ref_rel" % _tag(geom), ref_err)
        assert gpu_err <= 2 * ref_err, (gpu_err, ref_err)


def test_short_waveforms_give_zero_frames():
    from fastspeech2_amd.vocoder import mel_energy, stft_magnitude
    geom = (2048, 300, 1200)
    hp = _hp(geom)
    T = [1024, 0, 3000, 700]
    packed = _cuda(np.concatenate([O.harmonic_signal(t, seed=1) if t else np.zeros(0) for t in T]))
    mag = stft_magnitude(packed, T, hp=hp)
    lm, en = mel_energy(packed, T, hp=hp)
    rows = [t // 300 + 1 for t in T]
    assert mag.shape == (sum(rows), 1025)
    o = 0
    for t, r in zip(T, rows):
        if t <= 1024:
            assert not mag[o:o + r].any() and not en[o:o + r].any()
            assert (lm[o:o + r] - float(np.log(1e-5))).abs().max() <= 1e-5
        else:
            assert mag[o:o + r].abs().max() > 0 and (en[o:o + r] > 0).all()
        o += r


@pytest.mark.parametrize("geom", ALL, ids=_tag)
def test_griffin_lim_30_iterations_matches_oracle_and_reference(fixtures, geom):
    """Against the oracle at every geometry; against the reference's own recording where the fixtures hold one."""
    from fastspeech2_amd.vocoder import GriffinLim
    gl = GriffinLim(_hp(geom))
    d = _fixture_or_synthetic(fixtures, geom)
    M, A = d["magnitudes"], d["angles"]
    o = O.Stft(*geom)
    w = gl(_cuda(M), [M.shape[0]], n_iter=30, init_phase=_cuda(A), magnitudes=True)
    got = w.wav.cpu().numpy().astype(np.float64)
    want = o.griffin_lim(M, A, 30)
    err = np.abs(got - want).max() / np.abs(want).max()
    _record("vocoder_geom_%s_gl30_rel" % _tag(geom), err)
    sc_got, sc_want = o.spectral_convergence(M, got), o.spectral_convergence(M, want)
    _record("vocoder_geom_%s_gl30_sc_rel_diff" % _tag(geom), abs(sc_got - sc_want) / sc_want)
    assert abs(sc_got - sc_want) <= 0.01 * sc_want, (sc_got, sc_want)
    assert err <= 1e-3, err
    if "wav_iter30" in d:
        ref_err = np.abs(got - d["wav_iter30"]).max() / np.abs(want).max()
        _record("vocoder_geom_%s_gl30_vs_reference_rel" % _tag(geom), ref_err)
        assert ref_err <= 1e-3, ref_err


# (geometry, n_mels, sample rate).  57 is not a multiple of 4 (no aligned float4 rows).  512 / 160 / 400 runs at 16 kHz: at
# 22.05 kHz its 257 bins leave some of 80 or 100 mel triangles without a bin, pinv(B) is then ill-conditioned (cond ~ 1e17) and
# fp32 arithmetic on it moves the waveform by 1e-5 to 4e-3 of its peak against float64, whatever computes it.
MEL_CASES = [((1024, 256, 1024), 128, 22050), ((1024, 256, 1024), 100, 22050), ((1024, 256, 1024), 57, 22050),
             ((2048, 300, 1200), 128, 24000), ((2048, 300, 1200), 100, 24000), ((2048, 300, 1200), 57, 24000),
             ((512, 160, 400), 57, 16000)]


@pytest.mark.parametrize("geom,n_mels,sr", MEL_CASES, ids=lambda v: _tag(v) if isinstance(v, tuple) else str(v))
def test_mel_input_other_widths_matches_oracle(geom, n_mels, sr):
    """Log-mel input of n_mels != 80 (the prologue's run-time mel width): M = max(pinv(B) . exp(mel), 0) in the oracle with the
    float64 pinv of the same Slaney basis, then the ISTFT alone and 30 iterations from the same initial phase."""
    from fastspeech2_amd.vocoder import GriffinLim, seed_angles
    hp = _hp(geom, n_mels)
    hp.audio.sample_rate = sr
    gl = GriffinLim(hp)
    assert gl.geometry.n_mels == n_mels and gl.params["sample_rate"] == sr
    o = O.Stft(*geom)
    B = gl._basis_np
    lens = [97, 40]
    mels = []
    for b, L in enumerate(lens):      # the log-mels of real signals, as TacotronSTFT.mel_spectrogram makes them
        sig = O.harmonic_signal(geom[1] * (L - 1), seed=6 + b, noise=0.01, sr=sr)
        mels.append(np.log(np.maximum(np.abs(o.stft(sig)) @ B.T, 1e-5)).astype(np.float32))
    NB = geom[0] // 2 + 1
    angles = [seed_angles(4 + b, L, NB) for b, L in enumerate(lens)]
    packed, ang = _cuda(np.concatenate(mels)), _cuda(np.concatenate(angles))
    for n_iter, bar in ((0, 1e-6), (30, 1e-3)):
        w = gl(packed, lens, n_iter=n_iter, init_phase=ang)
        parts = [p.cpu().numpy().astype(np.float64) for p in w.split()]
        for b, (mel, A, got) in enumerate(zip(mels, angles, parts)):
            M = O.mel_to_mag(mel, gl._pinv_np)
            want = o.griffin_lim(M, A, n_iter)
            assert got.shape == want.shape
            err = np.abs(got - want).max() / np.abs(want).max()
            _record("vocoder_geom_%s_mel%d_in_iter%d_rel" % (_tag(geom), n_mels, n_iter), err)
            assert err <= bar, (b, n_iter, err)
            if n_iter:
                sc_got, sc_want = o.spectral_convergence(M, got), o.spectral_convergence(M, want)
                assert abs(sc_got - sc_want) <= 0.01 * sc_want, (b, sc_got, sc_want)
    # the same utterances padded [B, Lmax, n_mels] give the same waveforms
    pad = np.zeros((len(lens), max(lens), n_mels), np.float32)
    for b, m in enumerate(mels):
        pad[b, :m.shape[0]] = m
    assert torch.equal(gl(_cuda(pad), lens, n_iter=2, seed=3).wav, gl(packed, lens, n_iter=2, seed=3).wav)


@pytest.mark.parametrize("geom", ALL, ids=_tag)
def test_batch_invariance_and_short_utterances(geom):
    from fastspeech2_amd.vocoder import GriffinLim, tile_rule
    n_fft, hop, win = geom
    gl = GriffinLim(_hp(geom))
    F, lmin = tile_rule(n_fft, hop)["F"], gl.geometry.l_min
    lens = [0, 1, lmin - 1, lmin, F, F + 1, 2 * F + 1, 997]
    g = torch.Generator().manual_seed(0)
    mels = [torch.randn(L, 80, generator=g) * 1.5 - 5.0 for L in lens]
    batch = gl(torch.cat(mels).cuda(), lens, n_iter=4, seed=5)
    assert batch.sample_lens.tolist() == [hop * max(L - 1, 0) for L in lens]
    for L, m, got in zip(lens, mels, batch.split()):
        alone = gl(m.cuda(), [L], n_iter=4, seed=5).wav
        assert torch.equal(got, alone), L
        if L < lmin:
            assert got.numel() == hop * max(L - 1, 0) and not got.abs().any()
        else:
            assert torch.isfinite(got).all() and got.abs().max() > 0
    pad = torch.zeros(len(lens), max(lens), 80)
    for b, m in enumerate(mels):
        pad[b, :m.shape[0]] = m
    assert torch.equal(gl(pad.cuda(), lens, n_iter=4, seed=5).wav, batch.wav)


def test_seeded_phase_uses_n_bins():
    from fastspeech2_amd.vocoder import GriffinLim, seed_angles
    geom = (2048, 300, 1200)
    gl = GriffinLim(_hp(geom))
    M = np.abs(O.Stft(*geom).stft(O.harmonic_signal(300 * 40, seed=2)))
    a = gl(_cuda(M), [M.shape[0]], n_iter=2, seed=9, magnitudes=True).wav
    b = gl(_cuda(M), [M.shape[0]], n_iter=2, init_phase=_cuda(seed_angles(9, M.shape[0], n_bins=1025)), magnitudes=True).wav
    assert torch.equal(a, b)


def test_new_entry_points_equal_the_old_ones_at_the_default():
    from fastspeech2_amd import _lib
    from fastspeech2_amd.vocoder import GriffinLim, stft_magnitude
    lib = _lib.lib()
    gl = GriffinLim()
    assert tuple(gl.geometry) == (1024, 256, 1024, 80)
    g = torch.Generator().manual_seed(3)
    lens = [1, 4, 37, 200]
    mels = (torch.randn(sum(lens), 80, generator=g) * 1.5 - 5.0).cuda()
    for mom in (0.0, 0.5):
        new = gl(mels, lens, n_iter=5, seed=2, momentum=mom).wav       # GriffinLim calls fs2_op_griffin_lim_geom
        L = np.asarray(lens, np.int32)
        st = np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        ws = torch.empty(int(lib.fs2_op_vocode_workspace_bytes(len(L), ip(L))), dtype=torch.uint8, device="cuda")
        assert ws.numel() == int(lib.fs2_op_vocode_workspace_bytes_geom(1024, 256, 1024, 80, len(L), ip(L)))
        old = torch.empty_like(new)
        pinv = gl.constants(mels.device)[0]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.fs2_op_griffin_lim(stream, mels.data_ptr(), 80, pinv.data_ptr(), len(L), ip(st), ip(L), 5, mom, 2, None,
                                          ws.data_ptr(), ws.numel(), old.data_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(new, old), mom
    # analysis
    x = _cuda(O.harmonic_signal(9000, seed=7))
    T = np.asarray([9000], np.int32)
    st = np.zeros(1, np.int32)
    new_mag = stft_magnitude(x, [9000])
    new_mel = stft_magnitude(x, [9000], mel=True)
    ws = torch.empty(int(lib.fs2_op_stft_workspace_bytes(1, ip(T))), dtype=torch.uint8, device="cuda")
    old_mag, old_mel = torch.empty_like(new_mag), torch.empty_like(new_mel)
    basis = gl.constants(x.device)[1]
    _lib.check(lib.fs2_op_stft(stream, x.data_ptr(), 1, ip(st), ip(T), ws.data_ptr(), ws.numel(), old_mag.data_ptr(), basis.data_ptr(),
                               old_mel.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(new_mag, old_mag) and torch.equal(new_mel, old_mel)


def test_unsupported_geometry_is_refused_by_the_library():
    from fastspeech2_amd import _lib
    lib = _lib.lib()
    L = np.asarray([10], np.int32)
    p = L.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.fs2_op_vocode_workspace_bytes_geom(800, 200, 800, 80, 1, p) == 0
    assert lib.fs2_op_vocode_workspace_bytes_geom(2048, 200, 2048, 80, 1, p) == 0
    assert lib.fs2_op_stft_workspace_bytes_geom(1024, 256, 1024, 129, 1, p) == 0
    assert lib.fs2_op_griffin_lim_geom(None, 1024, 300, 256, 80, None, 80, None, 1, p, p, 1, 0.0, 0, None, None, 0, None) == -6


@pytest.mark.parametrize("geom", ALL, ids=_tag)
def test_non_default_stream(geom):
    from fastspeech2_amd.vocoder import GriffinLim
    gl = GriffinLim(_hp(geom))
    M = _cuda(np.abs(O.Stft(*geom).stft(O.harmonic_signal(geom[1] * 300, seed=4, sr=SR.get(geom, 22050)))))
    ref = gl(M, [M.shape[0]], n_iter=8, seed=1, magnitudes=True).wav
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # the input is produced on this stream right before the call: a call that ran elsewhere would read a half-written input
        M2 = torch.empty_like(M)
        M2.copy_(M * 1.0)
        res = gl(M2, [M.shape[0]], n_iter=8, seed=1, magnitudes=True).wav.clone()
    s.synchronize()
    assert torch.equal(res, ref)


def test_end_to_end_inference_batch_to_24khz_wav(tmp_path):
    import wave
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    from fastspeech2_amd.vocoder import GriffinLim, save_wav
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.cuda()
    g = torch.Generator().manual_seed(1)
    ilens = [23, 9, 17]
    xs = torch.zeros(3, max(ilens), dtype=torch.int64)
    for b, n in enumerate(ilens):
        xs[b, :n] = torch.randint(1, N_PHONEME_SYMBOLS, (n,), generator=g)
    with torch.no_grad():
        mels, olens = model.inference_batch(xs.cuda(), ilens, packed=True)
    vhp = _hp((2048, 300, 1200))
    gl = GriffinLim(vhp)
    w = gl(mels, olens)
    olens = [int(x) for x in olens]
    assert w.sample_lens.tolist() == [300 * max(L - 1, 0) for L in olens]
    assert torch.isfinite(w.wav).all()
    p = tmp_path / "tts24k.wav"
    n = save_wav(p, w.wav, vhp.audio.sample_rate)
    with wave.open(str(p), "rb") as f:
        assert (f.getframerate(), f.getsampwidth(), f.getnchannels(), f.getnframes()) == (24000, 2, 1, n)
    assert n == w.wav.numel()
