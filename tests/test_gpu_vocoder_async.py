"""Device-driven Griffin-Lim on the MI355X (``GriffinLim(...)(..., sync=False)``, fs2_op_griffin_lim_dev).

The yardstick of every waveform is the host-driven path (``GriffinLim(hp)(mels, olens)`` with host ``olens``), which
tests/test_gpu_vocoder*.py tie to the float64 oracles and the reference's recordings.  The tile kernels are the same and see the same
tile records, so every comparison here is ``torch.equal``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMS = [(1024, 256, 1024), (2048, 300, 1200), (512, 160, 400)]
_tag = lambda g: "%d_%d_%d" % g           # noqa: E731


def _gl(geom):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    n_fft, hop, win = geom
    return GriffinLim(DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "n_mels": 80}}))


def _mels(lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(L, 80, generator=g) * 1.5 - 5.0 for L in lens]


def _packed(mels, rows):
    """The utterances back to back in ``rows`` rows; the surplus rows are NaN (no valid result may depend on them)."""
    out = torch.full((rows, 80), float("nan"))
    cat = torch.cat(mels)
    out[:cat.shape[0]] = cat
    return out.cuda()


def _padded(mels, Lcap):
    out = torch.full((len(mels), Lcap, 80), float("nan"))
    for b, m in enumerate(mels):
        out[b, :m.shape[0]] = m
    return out.cuda()


def _dev(lens):
    return torch.tensor(lens, dtype=torch.int64).cuda()


def _assert_packed_equal(w, ref, hop, lens):
    wav, sl = w
    assert w.ok()
    total = ref.wav.numel()
    assert sl.dtype == torch.int64 and sl.is_cuda and torch.equal(sl.cpu(), ref.sample_lens)
    assert ref.sample_lens.tolist() == [hop * max(L - 1, 0) for L in lens]
    assert wav.numel() >= total and torch.equal(wav[:total], ref.wav)
    assert not wav[total:].any()                                    # zeros, not NaN, beyond the valid samples
    st = w.status.cpu().tolist()
    assert st[0] == sum(lens) and st[2] == 0 and st[3] == max(lens) and st[4] == total and st[5:] == [0, 0, 0]


@pytest.mark.parametrize("geom", GEOMS, ids=_tag)
def test_device_driven_equals_host_driven(geom):
    from fastspeech2_amd.vocoder import tile_rule
    gl = _gl(geom)
    hop = geom[1]
    F = tile_rule(geom[0], hop)["F"]
    lens = [1, 2, 3, 4, 5, F, F + 1, 2 * F + 1, 997, 0, 7]
    mels = _mels(lens)
    total, Lmax = sum(lens), max(lens)
    for momentum in (0.0, 0.99):
        ref = gl(torch.cat(mels).cuda(), lens, n_iter=4, momentum=momentum, seed=5)
        parts = ref.split()
        assert st_tiles(lens, F) > 0 and ref.wav.abs().max() > 0
        for cap in (total, 2 * total):
            w = gl(_packed(mels, cap), _dev(lens), n_iter=4, momentum=momentum, seed=5, sync=False)          # capacity = the rows
            _assert_packed_equal(w, ref, hop, lens)
            assert w.status.cpu()[1] == st_tiles(lens, F)
            w = gl(_packed(mels, 2 * total), _dev(lens), n_iter=4, momentum=momentum, seed=5, sync=False, capacity=cap)
            _assert_packed_equal(w, ref, hop, lens)
            for Lcap in (Lmax, Lmax + 13):
                pad = _padded(mels, Lcap)
                w = gl(pad, _dev(lens), n_iter=4, momentum=momentum, seed=5, sync=False, capacity=cap)
                _assert_packed_equal(w, ref, hop, lens)
                wp = gl(pad, _dev(lens), n_iter=4, momentum=momentum, seed=5, sync=False, capacity=cap, padded_out=True)
                assert wp.ok() and wp[0].shape == (len(lens), hop * (Lcap - 1)) and torch.equal(wp[1].cpu(), ref.sample_lens)
                for b, p in enumerate(parts):
                    assert torch.equal(wp[0][b, :p.numel()], p) and not wp[0][b, p.numel():].any(), b
                got = wp.split()
                assert all(torch.equal(a, b) for a, b in zip(got, parts))
        assert all(torch.equal(a, b) for a, b in zip(w.split(), parts))


def test_a_batch_of_thousands_of_utterances():
    """B = 3000: every thread of the planner's scan owns several utterances, and the tile prefix is searched over thousands of entries."""
    gl = _gl(GEOMS[0])
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 13, size=3000).tolist()
    lens[17], lens[2999] = 150, 70
    mels = _mels(lens, seed=4)
    ref = gl(torch.cat(mels).cuda(), lens, n_iter=2, seed=8)
    for rows in (sum(lens), sum(lens) + 999):
        w = gl(_packed(mels, rows), _dev(lens), n_iter=2, seed=8, sync=False)
        _assert_packed_equal(w, ref, 256, lens)
        assert int(w.status.cpu()[1]) == st_tiles(lens, 32)


def st_tiles(lens, F):
    return sum(-(-L // F) for L in lens if L >= 2)


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=_tag)
def test_the_call_is_captured_and_replayed_with_other_lengths(geom):
    """The frame counts are read by kernels only: a graph captured with one ``olens`` vocodes whatever lengths the static tensor
    holds at replay.  A host read of the counts would fail the capture or replay the captured lengths."""
    gl = _gl(geom)
    B, cap = 5, 600
    first = [100, 40, 0, 3, 57]
    static_mels = _packed(_mels(first, seed=1), cap)
    static_olens = _dev(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gl(static_mels, static_olens, n_iter=4, seed=3, sync=False)          # eager warm-up: one-time host work stays outside the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gl(static_mels, static_olens, n_iter=4, seed=3, sync=False)
    assert out.ok()                                                            # no host-side record under capture
    seen = []
    for k, lens in enumerate([first, [7, 250, 90, 1, 200], [590, 2, 2, 2, 4]]):
        assert len(lens) == B and sum(lens) <= cap
        mels = _mels(lens, seed=10 + k)
        static_mels.copy_(_packed(mels, cap))
        static_olens.copy_(_dev(lens))
        graph.replay()
        torch.cuda.synchronize()
        ref = gl(torch.cat(mels).cuda(), lens, n_iter=4, seed=3)
        total = ref.wav.numel()
        assert int(out.status.cpu()[2]) == 0
        assert torch.equal(out[1].cpu(), ref.sample_lens), lens
        assert torch.equal(out[0][:total], ref.wav) and not out[0][total:].any(), lens
        seen.append(out[0][:2000].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def _assert_refused(w, B):
    from fastspeech2_amd.fastspeech import Fs2CapacityError
    assert not w.ok()
    with pytest.raises(Fs2CapacityError):
        w.check()
    assert w[0].numel() > 0 and torch.isnan(w[0]).all()
    assert w[1].numel() == B and not w[1].any()
    st = w.status.cpu().tolist()
    assert st[1] == 0 and st[2] != 0 and st[4] == 0
    return st[2]


def test_invalid_lengths_and_capacities_are_refused_by_the_planner():
    """Lengths one past a bound, a negative one and a flagged producer: the planner emits no tile, says so in the flags and NaN-fills
    the waveform; the next call on the same stream is unaffected."""
    from fastspeech2_amd.fastspeech import AsyncMels
    gl = _gl(GEOMS[0])
    lens = [40, 3, 100, 0, 65]
    B, total, Lmax = len(lens), sum(lens), max(lens)
    mels = _mels(lens, seed=2)
    ref = gl(torch.cat(mels).cuda(), lens, n_iter=4, seed=1)

    def good():
        w = gl(_packed(mels, total), _dev(lens), n_iter=4, seed=1, sync=False)
        _assert_packed_equal(w, ref, 256, lens)

    good()
    # sum L = frame_capacity + 1
    fl = _assert_refused(gl(_packed(mels, total), _dev(lens), n_iter=4, seed=1, sync=False, capacity=total - 1), B)
    assert fl == 1                                        # FS2_OVF_ROWS
    good()
    # one negative entry
    neg = list(lens)
    neg[1] = -1
    fl = _assert_refused(gl(_packed(mels, total), _dev(neg), n_iter=4, seed=1, sync=False), B)
    assert fl == 64                                       # FS2_OVF_NEG_LEN
    good()
    # a padded source with one L_b = Lcap + 1
    long = list(lens)
    long[2] = Lmax + 1
    for padded_out in (False, True):
        fl = _assert_refused(gl(_padded(mels, Lmax), _dev(long), n_iter=4, seed=1, sync=False, padded_out=padded_out), B)
        assert fl == 2                                    # FS2_OVF_LMAX
    good()
    # the producer of the frames had flagged its own status
    up = torch.zeros(8, dtype=torch.int32)
    up[2] = 1
    am = AsyncMels(_packed(mels, total), _dev(lens), up.cuda(), None)
    fl = _assert_refused(gl(am, n_iter=4, seed=1, sync=False), B)
    assert fl == 32 | 1                                   # FS2_OVF_UPSTREAM and the producer's own flags
    good()
    # a clean producer status changes nothing
    am = AsyncMels(_packed(mels, total), _dev(lens), torch.zeros(8, dtype=torch.int32).cuda(), None)
    _assert_packed_equal(gl(am, n_iter=4, seed=1, sync=False), ref, 256, lens)


@pytest.fixture(scope="module")
def model():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    hp = default_hparams()
    m = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    m.load_state_dict(portable_state_dict(m.state_dict(), seed=0))
    return m.to("cuda:0")


def _text_to_wav_matches(model, gl, xs, il, **kw):
    am = model.inference_batch(xs, il, packed=True, sync=False, **kw)
    w = gl(am, n_iter=4, seed=2, sync=False)
    assert am.ok() and w.ok()
    mels, ol_dev = am
    ol = ol_dev.cpu()
    ref = gl(mels[:int(ol.sum())], ol, n_iter=4, seed=2)             # the host-driven vocoder on this call's own mels
    assert ref.wav.numel() > 0 and torch.isfinite(ref.wav).all() and ref.wav.abs().max() > 0
    assert torch.equal(w[1].cpu(), ref.sample_lens)
    assert torch.equal(w[0][:ref.wav.numel()], ref.wav) and not w[0][ref.wav.numel():].any()
    return ol


def test_text_to_waveform_without_a_host_sync(model):
    from fastspeech2_amd.synthetic import make_batch
    gl = _gl(GEOMS[0])
    b = make_batch("c3", B=6)
    xs, il, ds = b["xs"].cuda(), b["ilens"], b["ds"].cuda()
    with torch.no_grad():
        _, ol_sync = model.inference_batch(xs, il, d_override=ds)          # (the first call of a model is synchronous: learns the capacities)
        ol = _text_to_wav_matches(model, gl, xs, il, d_override=ds)
        assert torch.equal(ol, ol_sync)
        # padded mels, padded waveforms
        am = model.inference_batch(xs, il, d_override=ds, sync=False)
        wp = gl(am, n_iter=4, seed=2, sync=False, padded_out=True)
        ref = gl(am[0], ol, n_iter=4, seed=2).split()
        assert wp.ok() and wp[0].shape == (6, 256 * (am[0].shape[1] - 1))
        for i, p in enumerate(ref):
            assert torch.equal(wp[0][i, :p.numel()], p) and not wp[0][i, p.numel():].any()


def test_text_to_waveform_with_reduction_factor_2():
    from tests.test_oracle_golden import reduction_setup
    from fastspeech2_amd.synthetic import make_batch
    hp, m, sd, cfg = reduction_setup()
    m.load_state_dict(sd)
    m = m.cuda()
    gl = _gl(GEOMS[0])
    b = make_batch("c2", B=3)
    xs, il = b["xs"].cuda(), b["ilens"]
    with torch.no_grad():
        _, ol_sync = m.inference_batch(xs, il)
        ol = _text_to_wav_matches(m, gl, xs, il)
    assert torch.equal(ol, ol_sync) and (ol % 2 == 0).all()                 # the lengths are MEL frames: 2 per decoder frame


def test_three_batches_in_flight(model):
    from fastspeech2_amd import StepStreams
    from fastspeech2_amd.synthetic import make_batch
    gl = _gl(GEOMS[0])
    batches = []
    for k in range(3):
        b = make_batch("c3", B=4 + k)
        batches.append((b["xs"].cuda(), b["ilens"], b["ds"].cuda()))
    with torch.no_grad():
        for xs, il, ds in batches:
            model.inference_batch(xs, il, d_override=ds)
        one_by_one = []
        for xs, il, ds in batches:
            am = model.inference_batch(xs, il, d_override=ds, packed=True, sync=False)
            w = gl(am, n_iter=4, seed=9, sync=False)
            torch.cuda.synchronize()
            one_by_one.append((w[0].clone(), w[1].clone()))
        rot = StepStreams(3)
        flight = []
        for xs, il, ds in batches:
            with rot.next():
                am = model.inference_batch(xs, il, d_override=ds, packed=True, sync=False)
                flight.append((am, gl(am, n_iter=4, seed=9, sync=False)))
        rot.join()
        assert model.async_ok()
        for (am, w), (wav, sl) in zip(flight, one_by_one):
            assert am.ok() and w.ok()
            n = int(sl.sum())                       # (the predicted capacities, so the lengths of the two buffers, may differ between the runs)
            assert torch.equal(w[1], sl) and n > 0, (w[1].tolist(), sl.tolist())
            assert torch.equal(w[0][:n], wav[:n]) and not w[0][n:].any() and not wav[n:].any(), (w[0].shape, wav.shape)


def test_capture_graph_with_a_vocoder(model):
    from fastspeech2_amd.synthetic import make_batch
    gl = _gl(GEOMS[0])
    b = make_batch("c3", B=3)
    xs, il, ds = b["xs"].cuda(), b["ilens"], b["ds"].cuda()
    with torch.no_grad():
        run = model.capture_graph(xs, il, d_override=ds, vocoder=gl, n_iter=4)
        xs2 = xs.clone()
        for i in range(xs.shape[0]):
            T = int(il[i])
            xs2[i, :T] = xs[i, :T].flip(0)
        outs = []
        for x in (xs, xs2):
            wav, sl, status = run(x)
            assert int(status.cpu()[2]) == 0
            am = model.inference_batch(x, il, d_override=ds, sync=False)
            w = gl(am, n_iter=4, sync=False, padded_out=True)
            assert am.ok() and w.ok() and torch.equal(sl, w[1]) and int(sl.sum()) > 0
            n = min(wav.shape[1], w[0].shape[1])                        # (the two capacities differ: compare the common columns, zeros beyond)
            assert int(sl.max()) <= n
            assert torch.equal(wav[:, :n], w[0][:, :n]) and not wav[:, n:].any() and not w[0][:, n:].any()
            outs.append(wav.clone())
        assert not torch.equal(outs[0], outs[1])
        with pytest.raises(TypeError, match="vocoder"):
            model.capture_graph(xs, il, d_override=ds, n_iter=4)
        model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        model.inference_batch(xs, il, d_override=ds)
        with pytest.raises(RuntimeError, match="capture"):
            run(xs)
