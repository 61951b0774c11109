"""Mel-constrained Griffin-Lim on the MI355X (``GriffinLim(...)(..., constraint="mel")``, fs2_op_griffin_lim_mel_geom / _dev; DESIGN.md
section 14.10) against the float64 oracle (tests/mel_gl_oracle.py), and its bit-identity across batches, layouts and call forms."""
import numpy as np
import pytest
import torch

from tests import mel_gl_oracle as MO
from tests import vocoder_oracle as O

pytestmark = pytest.mark.gpu

# (n_fft, hop, win), sample rate, n_mels, frame counts: the default with a full 32-frame tile plus a 5-frame tile with both halos, an
# utterance just above L_min and one below it; 2048 / 300 / 1200; 512 with the smallest hop (halo 7, L_min 6) and fewer mels than lanes
CASES = [((1024, 256, 1024), 22050, 80, [37, 5, 3]), ((2048, 300, 1200), 24000, 80, [12]), ((512, 64, 512), 16000, 40, [40, 6, 5])]
_tag = lambda c: "%d_%d_%d" % c[0]           # noqa: E731


def _record(name, value):
    from tests.conftest import record_measurement
    record_measurement(name, value)


def _gl(geom=(1024, 256, 1024), sr=22050, n_mels=80):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    n_fft, hop, win = geom
    return GriffinLim(DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "n_mels": n_mels, "sample_rate": sr}}))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _harmonic_mels(st, basis, lens, sr):
    """Per utterance the float32 log-mel of a harmonic signal with noise (an utterance too short to analyse borrows rows of the first)."""
    lmin = O.l_min(st.n_fft, st.hop)
    out = []
    for b, L in enumerate(lens):
        if L >= lmin:
            sig = O.harmonic_signal(st.hop * (L - 1), seed=b, f0=120.0 + 100.0 * b, sr=sr, noise=0.05)
            out.append(MO.log_mel(st, sig, basis).astype(np.float32))
        else:
            out.append(out[0][:L].copy())
        assert out[-1].shape[0] == L
    return out


def _rel_errors(st, gl, mels, lens, parts, angles, n_iter, momentum):
    errs = []
    for mel, L, got, ang in zip(mels, lens, parts, angles):
        want = MO.griffin_lim_mel(st, mel, gl._basis_np, gl._pinv_np, ang, n_iter, momentum)
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape == (st.hop * (L - 1),)
        if L < O.l_min(st.n_fft, st.hop):
            assert not got.any() and not want.any()           # documented zeros
        else:
            assert np.abs(want).max() > 0
            errs.append(np.abs(got - want).max() / np.abs(want).max())
    return errs


@pytest.mark.parametrize("case", CASES, ids=_tag)
def test_matches_the_float64_oracle(case):
    from fastspeech2_amd.vocoder import seed_angles
    geom, sr, n_mels, lens = case
    gl, st = _gl(geom, sr, n_mels), O.Stft(*geom)
    NB = geom[0] // 2 + 1
    mels = _harmonic_mels(st, gl._basis_np, lens, sr)
    packed = _cuda(np.concatenate(mels))
    rng = np.random.default_rng(1)
    given = [rng.uniform(-np.pi, np.pi, size=(L, NB)).astype(np.float32) for L in lens]
    worst = 0.0
    for momentum in (0.0, 0.99):
        w = gl(packed, lens, n_iter=4, momentum=momentum, seed=7, constraint="mel")
        assert w.sample_lens.tolist() == [geom[1] * (L - 1) for L in lens]
        errs = _rel_errors(st, gl, mels, lens, w.split(), [seed_angles(7, L, NB) for L in lens], 4, momentum)
        w = gl(packed, lens, n_iter=4, momentum=momentum, init_phase=_cuda(np.concatenate(given)), constraint="mel")
        errs += _rel_errors(st, gl, mels, lens, w.split(), given, 4, momentum)
        print("%s momentum %g: max |wav - oracle| / peak per utterance and phase source: %s" % (_tag(case), momentum, ["%.2e" % e for e in errs]))
        worst = max(worst, max(errs))
    _record("vocoder_mel_gl4_rel_" + _tag(case), worst)
    assert worst <= 1e-3, worst
    # no iteration: the plain call, bit for bit
    assert torch.equal(gl(packed, lens, n_iter=0, seed=7, constraint="mel").wav, gl(packed, lens, n_iter=0, seed=7).wav)
    # and the constraint does change an iteration
    assert not torch.equal(gl(packed, lens, n_iter=1, seed=7, constraint="mel").wav, gl(packed, lens, n_iter=1, seed=7).wav)


def _random_mels(lens, n_mels=80, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(L, n_mels, generator=g) * 1.5 - 5.0 for L in lens]


def test_batch_invariance_layouts_and_short_utterances():
    gl = _gl()
    F = 32
    lens = [1, 2, 3, 4, 5, F, F + 1, 2 * F + 1, 70, 0, 7]
    mels = _random_mels(lens)
    for momentum in (0.0, 0.99):
        batch = gl(torch.cat(mels).cuda(), lens, n_iter=4, momentum=momentum, seed=5, constraint="mel")
        assert batch.sample_lens.tolist() == [256 * max(L - 1, 0) for L in lens]
        for L, m, got in zip(lens, mels, batch.split()):
            alone = gl(m.cuda(), [L], n_iter=4, momentum=momentum, seed=5, constraint="mel").wav
            assert torch.equal(got, alone), L
            if L < 4:
                assert got.numel() == 256 * max(L - 1, 0) and not got.abs().any()
            else:
                assert torch.isfinite(got).all() and got.abs().max() > 0
        pad = torch.zeros(len(lens), max(lens), 80)
        for b, m in enumerate(mels):
            pad[b, :m.shape[0]] = m
        padded = gl(pad.cuda(), lens, n_iter=4, momentum=momentum, seed=5, constraint="mel")
        assert torch.equal(padded.wav, batch.wav)


def _nan_packed(mels, rows):
    out = torch.full((rows, mels[0].shape[1]), float("nan"))
    cat = torch.cat(mels)
    out[:cat.shape[0]] = cat
    return out.cuda()


@pytest.mark.parametrize("geom", [(1024, 256, 1024), (512, 160, 400)], ids=lambda g: "%d_%d_%d" % g)
def test_device_driven_and_captured_calls_equal_the_eager_one(geom):
    gl = _gl(geom)
    hop = geom[1]
    lens = [40, 3, 70, 0, 9]
    mels = _random_mels(lens, seed=2)
    total = sum(lens)
    dev_lens = torch.tensor(lens, dtype=torch.int64).cuda()
    for momentum in (0.0, 0.99):
        ref = gl(torch.cat(mels).cuda(), lens, n_iter=4, momentum=momentum, seed=3, constraint="mel")
        n = ref.wav.numel()
        assert n == hop * sum(max(L - 1, 0) for L in lens) and ref.wav.abs().max() > 0
        w = gl(_nan_packed(mels, total + 13), dev_lens, n_iter=4, momentum=momentum, seed=3, sync=False, constraint="mel")
        assert w.ok() and torch.equal(w[1].cpu(), ref.sample_lens)
        assert torch.equal(w[0][:n], ref.wav) and not w[0][n:].any()
        pad = torch.full((len(lens), max(lens) + 2, 80), float("nan"))
        for b, m in enumerate(mels):
            pad[b, :m.shape[0]] = m
        wp = gl(pad.cuda(), dev_lens, n_iter=4, momentum=momentum, seed=3, sync=False, padded_out=True, constraint="mel")
        assert wp.ok() and all(torch.equal(a, b) for a, b in zip(wp.split(), ref.split()))
    # captured and replayed with other lengths: the eager call above did the one-time host work of this geometry and constraint
    static_mels, static_lens = _nan_packed(mels, 200), dev_lens.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gl(static_mels, static_lens, n_iter=4, momentum=0.99, seed=3, sync=False, constraint="mel")
    for k, new in enumerate([lens, [100, 2, 31, 60, 7]]):
        m2 = _random_mels(new, seed=20 + k)
        static_mels.copy_(_nan_packed(m2, 200))
        static_lens.copy_(torch.tensor(new, dtype=torch.int64).cuda())
        graph.replay()
        torch.cuda.synchronize()
        ref = gl(torch.cat(m2).cuda(), new, n_iter=4, momentum=0.99, seed=3, constraint="mel")
        n = ref.wav.numel()
        assert int(out.status.cpu()[2]) == 0 and torch.equal(out[1].cpu(), ref.sample_lens)
        assert torch.equal(out[0][:n], ref.wav) and not out[0][n:].any(), new


def test_capture_graph_takes_the_constraint():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import make_batch, portable_state_dict
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=0))
    model = model.to("cuda:0")
    gl = _gl()
    b = make_batch("c3", B=2)
    xs, il, ds = b["xs"].cuda(), b["ilens"], b["ds"].cuda()
    with torch.no_grad():
        run = model.capture_graph(xs, il, d_override=ds, vocoder=gl, n_iter=4, constraint="mel")
        wav, sl, status = run(xs)
        assert int(status.cpu()[2]) == 0 and int(sl.sum()) > 0
        mels, ol = model.inference_batch(xs, il, d_override=ds)
        ref = gl(mels, ol, n_iter=4, constraint="mel").split()
        plain = gl(mels, ol, n_iter=4).split()
    for i, p in enumerate(ref):
        assert int(sl[i]) == p.numel() and torch.equal(wav[i, :p.numel()], p) and not wav[i, p.numel():].any()
        assert not torch.equal(p, plain[i])


def test_a_dense_basis_and_the_spsi_start():
    """Any non-negative basis: a dense random one (8 mels, 512-point) has full ranges in the band tables and still matches the oracle.
    ``init="spsi"`` composes with the constraint."""
    from fastspeech2_amd.vocoder import seed_angles
    geom = (512, 128, 512)
    gl, st = _gl(geom, 16000, 8), O.Stft(*geom)
    rng = np.random.default_rng(3)
    gl._basis_np = rng.uniform(0.0, 1.0, size=(8, 257)) / 257.0
    gl._basis_np[:, 200:] = 0.0                                # bins no filter covers
    gl._basis_np[2, 50:60] = 0.0                               # a zero inside a row's support
    gl._pinv_np = np.linalg.pinv(gl._basis_np)
    gl._dev.clear()
    lens = [19, 9]
    mels = _harmonic_mels(st, gl._basis_np, lens, 16000)
    w = gl(_cuda(np.concatenate(mels)), lens, n_iter=4, momentum=0.99, seed=2, constraint="mel")
    errs = _rel_errors(st, gl, mels, lens, w.split(), [seed_angles(2, L, 257) for L in lens], 4, 0.99)
    _record("vocoder_mel_gl4_rel_dense_basis", max(errs))
    assert max(errs) <= 1e-3, errs
    gd = _gl()
    m = _cuda(_harmonic_mels(O.Stft(), gd._basis_np, [40], 22050)[0])
    a = gd(m, [40], n_iter=6, init="spsi", constraint="mel").wav
    assert torch.isfinite(a).all() and a.abs().max() > 0
    assert not torch.equal(a, gd(m, [40], n_iter=6, init="spsi").wav)
    with pytest.raises(ValueError, match="no mel to constrain to"):
        gd(torch.zeros(10, 513).cuda(), [10], magnitudes=True, constraint="mel")


def test_the_waveforms_mel_is_closer_to_the_given_one():
    """61 frames, 30 iterations, both constraints from the same seed; the log-mel of each output is taken by the float64 oracle's
    STFT on the host.  Float64 prototype of the same run: ratio 0.55 (tests/test_mel_gl_host.py)."""
    gl, st = _gl(), O.Stft()
    mel = MO.log_mel(st, O.harmonic_signal(256 * 60, seed=1, f0=220.0, noise=0.05), gl._basis_np)
    m = _cuda(mel)
    err = {}
    for c in ("magnitude", "mel"):
        wav = gl(m, [61], n_iter=30, seed=0, constraint=c).wav.cpu().numpy().astype(np.float64)
        err[c] = MO.mel_error(st, wav, mel, gl._basis_np)
        _record("vocoder_mel_error_30_" + c, err[c])
    print("mean |log-mel(wav) - mel| after 30 iterations: magnitude %.4f, mel %.4f, ratio %.3f" % (err["magnitude"], err["mel"], err["mel"] / err["magnitude"]))
    assert err["mel"] <= 0.75 * err["magnitude"], err
