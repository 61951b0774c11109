"""Pitch and energy control on the MI355X (fs2_decode_ctl, fs2_op_label_means: fastspeech2_amd.prosody, csrc/prosody.h).

Every comparison is EXACT.  The control is one float32 product and one float32 sum per value, rounded one after the other, which torch
restates bit for bit; everything behind it is the code the uncontrolled and the teacher-forced paths run, so a controlled run is held
to (1) the uncontrolled run under neutral control, (2) the definition applied to the uncontrolled run's own outputs, (3) the
teacher-forced run that is GIVEN the controlled values, (4) torch.bucketize of an imposed contour, and (5) itself through every
other entry point.  There is nothing to tolerate.

Both routes of the predictor outputs to the decoder are covered: fp32 quantises in bucket_embed, mix_mx in dec_in_gather."""
import numpy as np
import pytest
import torch

from tests import prosody_oracle as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WANT = ("after", "qe", "qp", "e_outs", "p_outs", "lr_index")
PRECISIONS = ["fp32", "mix_mx"]
BATCHES = ["b3", "b1"]


@pytest.fixture(scope="module")
def model():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import ljspeech_durations, portable_state_dict
    hp = default_hparams()
    m = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    m.load_state_dict(ljspeech_durations(portable_state_dict(m.state_dict(), seed=0)))
    return m.to(DEV)


_batches, _base = {}, {}


def batch(name):
    if name not in _batches:
        from fastspeech2_amd.synthetic import make_batch
        b = make_batch("c2", B=3, tlens=[9, 1, 5], seed=11) if name == "b3" else make_batch("c2", B=1, tlens=[1], seed=11)
        _batches[name] = (b["xs"].to(DEV), b["ilens"])
    return _batches[name]


def run(model, prec, name, **controls):
    model.precision = prec
    xs, il = batch(name)
    with torch.no_grad():
        return model._run(xs, il, is_inference=True, want=WANT, prosody=controls or None)


def base(model, prec, name):
    """The uncontrolled run, computed once and left unchanged."""
    if (prec, name) not in _base:
        _base[(prec, name)] = run(model, prec, name)
    return _base[(prec, name)]


def draw(name, seed):
    """Random controls of a batch: [B, 1] scales in [0.5, 2], a [B, Tmax] pitch shift, a [B, 1] energy shift."""
    xs, _ = batch(name)
    B, T = xs.shape
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: (lo + (hi - lo) * torch.rand(shape, generator=g)).to(DEV)
    return dict(pitch_scale=u((B, 1), 0.5, 2.0), pitch_shift=u((B, T), -40.0, 40.0), energy_scale=u((B, 1), 0.5, 2.0), energy_shift=u((B, 1), -1.0, 1.0))


def per_frame(v, lri):
    """A [B, 1] or [B, Tmax] control at every frame, through lr_index (anything at pads)."""
    return v.expand(-1, 1) if v.shape[1] == 1 else v.gather(1, lri.clamp(min=0).long())


def names(model):
    return [r[0] for r in model.get_profile()]


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_neutral_control_is_no_control(model, prec, name):
    r0 = base(model, prec, name)
    xs, _ = batch(name)
    ones, zeros = torch.ones(xs.shape, device=DEV), torch.zeros(xs.shape, device=DEV)
    for ctl in (dict(pitch_scale=1.0, pitch_shift=0.0, energy_scale=1.0, energy_shift=0.0),
                dict(pitch_scale=ones, pitch_shift=zeros, energy_scale=ones, energy_shift=zeros)):
        r = run(model, prec, name, **ctl)
        for k in ("after", "qe", "qp", "e_outs", "p_outs", "lr_index"):
            assert torch.equal(r[k], r0[k]), k
        assert torch.equal(r["olens"], r0["olens"])
    model.set_profiling(True)
    try:
        run(model, prec, name)
        assert names(model).count("var.control") == 0 and len(names(model)) > 10
        model.set_profiling(True)                                          # (clears the records)
        run(model, prec, name, pitch_scale=1.0)
        assert names(model).count("var.control") == 1
        model.set_profiling(True)
        run(model, prec, name, **draw(name, 1))                            # pitch and energy: still one launch
        assert names(model).count("var.control") == 1
    finally:
        model.set_profiling(False)


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_the_values_are_the_definition(model, prec, name):
    r0, ctl = base(model, prec, name), draw(name, 2)
    r = run(model, prec, name, **ctl)
    lri = r0["lr_index"]
    assert torch.equal(r["lr_index"], lri) and torch.equal(r["olens"], r0["olens"])
    valid = lri >= 0
    assert int(valid.sum()) == int(r0["olens"].sum())
    for track, out in (("pitch", "p_outs"), ("energy", "e_outs")):
        scaled = r0[out] * per_frame(ctl[track + "_scale"], lri)           # float32, rounded
        want = torch.where(valid, scaled + per_frame(ctl[track + "_shift"], lri), torch.zeros_like(scaled))      # rounded again; pads stay 0
        assert torch.equal(r[out], want), out
        assert not torch.equal(r[out], r0[out])
        assert not r[out][~valid].any()


def _used_durations(r, il):
    used = r["d_int"].cpu().clone()
    for n in range(used.shape[0]):
        used[n, int(il[n]):] = 0
        if int(used[n].sum()) == 0:                                         # the length regulator's rule for a row of zeros: one frame per token
            used[n, :int(il[n])] = 1
    assert torch.equal(used.sum(1), r["olens"])
    return used


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_the_mel_is_the_one_those_values_give(model, prec, name):
    """The teacher-forced, per-utterance run that is handed the durations used and the controlled values quantises and decodes them
    to the same bits: the feature is tied to the reference's own teacher-forced path."""
    r = run(model, prec, name, **draw(name, 3))
    xs, il = batch(name)
    with torch.no_grad():
        t = model._run(xs, il, ds=_used_durations(r, il).to(DEV), es=r["e_outs"], ps=r["p_outs"], is_inference=False, compat=False, want=WANT)
    assert torch.equal(t["olens"], r["olens"]) and torch.equal(t["lr_index"], r["lr_index"])
    assert torch.equal(t["qe"], r["qe"]) and torch.equal(t["qp"], r["qp"])
    assert torch.equal(t["after"], r["after"])


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_a_contour_can_be_imposed(model, prec, name):
    r0 = base(model, prec, name)
    xs, il = batch(name)
    B, T = xs.shape
    bins = model.pitch_predictor.pitch_bins
    hz = (60.0 + 640.0 * torch.rand((B, T), generator=torch.Generator().manual_seed(4))).float()
    assert not torch.isin(hz, bins.cpu()).any()                             # no drawn value on a bin edge
    hz = hz.to(DEV)
    r = run(model, prec, name, pitch_scale=0.0, pitch_shift=hz)
    lri = r["lr_index"]
    valid = lri >= 0
    gathered = per_frame(hz, lri)
    assert torch.equal(r["p_outs"], torch.where(valid, gathered, torch.zeros_like(gathered)))
    want_q = torch.where(valid, torch.bucketize(gathered, bins).to(torch.int32), torch.full_like(lri, -1))
    assert torch.equal(r["qp"], want_q)
    assert torch.equal(r["qe"], r0["qe"]) and torch.equal(r["e_outs"], r0["e_outs"])      # energy was not touched
    assert not torch.equal(r["after"], r0["after"])                         # control reaches the decoder
    if name == "b3":
        print("distinct pitch buckets: uncontrolled %d, imposed %d" % (r0["qp"][valid].unique().numel(), r["qp"][valid].unique().numel()))
        assert r["qp"][valid].unique().numel() >= 10
    with torch.no_grad():
        p = model.predict_prosody(xs, il, pitch_scale=0.0, pitch_shift=hz)
    assert torch.equal(p.durations.sum(1).cpu(), p.olens) and torch.equal(p.olens, r["olens"])
    assert p.durations.dtype == torch.int64 and p.durations.shape == (B, T) and p.voiced_tok.dtype == torch.int32
    assert torch.equal(p.durations, _used_durations(r, il).to(DEV))
    has = p.durations > 0
    assert torch.equal(p.pitch_tok[has], hz[has]) and not p.pitch_tok[~has].any()
    assert torch.equal(p.voiced_tok.long(), p.durations)                   # every imposed value is > 0: every frame is voiced
    assert torch.equal(p.pitch, r["p_outs"]) and torch.equal(p.energy, r["e_outs"]) and torch.equal(p.lr_index, lri)
    e_np, lri_np = r["e_outs"].cpu().numpy(), lri.cpu().numpy()
    want_e, want_n = P.label_means(e_np, lri_np, r["olens"].numpy(), T)
    assert P.same_bits(p.energy_tok.cpu().numpy(), want_e) and np.array_equal(p.durations.cpu().numpy(), want_n)


def _frames(mels, olens):
    return [mels[n, :int(olens[n])] for n in range(len(olens))]


def _same_frames(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_every_path_agrees(model, prec, name):
    model.precision = prec
    xs, il = batch(name)
    B, T = xs.shape
    ctl = dict(draw(name, 5), energy_scale=1.25)
    with torch.no_grad():
        mel, ol = model.inference_batch(xs, il, **ctl)
        want = _frames(mel, ol)
        assert not _same_frames(want, _frames(*model.inference_batch(xs, il)))      # (the control does something)
        # sync=False: the device-driven layout
        res = model.inference_batch(xs, il, sync=False, **ctl)
        assert type(res).__name__ == "AsyncMels"
        res.check()
        assert torch.equal(res[1].cpu(), ol) and _same_frames(_frames(res[0], ol), want)
        # packed
        packed, ol_p = model.inference_batch(xs, il, packed=True, **ctl)
        assert torch.equal(ol_p, ol) and _same_frames(list(packed.split(ol.tolist())), want)
        # inference() on one utterance against the synchronous padded call on that utterance
        for n in range(B):
            t = int(il[n])
            one = {k: (v[n:n + 1, :t] if torch.is_tensor(v) else v) for k, v in ctl.items()}
            m1, o1 = model.inference_batch(xs[n:n + 1, :t], il[n:n + 1], **one)
            assert torch.equal(model.inference(xs[n, :t], **one), m1[0, :int(o1[0])])
        # two shards, the controls cut as ShardedSynthesizer cuts tensor keywords
        if B > 1:
            for mine in ([0, 2], [1]):
                sel = torch.as_tensor(mine)
                il_loc = il[sel]
                xs_loc = xs[sel.to(DEV)][:, :int(il_loc.max())]
                kw = {k: (v[sel.to(v.device)][:, :xs_loc.shape[1]] if torch.is_tensor(v) else v) for k, v in ctl.items()}
                m_loc, o_loc = model.inference_batch(xs_loc, il_loc, regime=(int(il.sum()), B), **kw)
                assert torch.equal(o_loc, ol[sel]) and _same_frames(_frames(m_loc, o_loc), [want[n] for n in mine])
        # a captured graph, replayed twice with other controls copied in
        run_graph = model.capture_graph(xs, il, **ctl)
        for seed in (6, 7):
            new = dict(draw(name, seed), energy_scale=0.75 if seed == 6 else torch.full((B, 1), 1.5, device=DEV))
            after, olens_dev, status = run_graph(xs, **new)
            torch.cuda.synchronize()
            assert int(status[2]) == 0
            m_e, o_e = model.inference_batch(xs, il, **new)
            assert torch.equal(olens_dev.cpu(), o_e) and _same_frames(_frames(after, o_e), _frames(m_e, o_e))
            assert not _same_frames(_frames(after, o_e), want)
        with pytest.raises(ValueError, match="captured shape"):
            run_graph(xs, pitch_shift=torch.zeros(B, T + 1, device=DEV))
        plain = model.capture_graph(xs, il)
        with pytest.raises(ValueError, match="pitch_scale"):
            plain(xs, pitch_scale=1.1)


def test_errors_are_raised_before_any_launch(model, monkeypatch):
    from fastspeech2_amd import _lib
    from fastspeech2_amd import fastspeech as F
    model.precision = "fp32"
    xs, il = batch("b3")
    B, T = xs.shape
    r = base(model, "fp32", "b3")
    model.set_profiling(True)
    try:
        model.batch_semantics = "padded_compat"
        try:
            with pytest.raises(ValueError, match="per-utterance"):
                model.inference_batch(xs, il, pitch_scale=1.1)
        finally:
            model.batch_semantics = "per_utterance"
        with torch.no_grad():
            with pytest.raises(ValueError, match="per-utterance"):
                model._run(xs, il, is_inference=True, compat=True, prosody=dict(pitch_scale=1.1))
            with pytest.raises(ValueError, match="pitch_shift"):
                model.inference_batch(xs, il, pitch_shift=torch.zeros(B, device=DEV))
            with pytest.raises(ValueError, match="energy_scale"):
                model.inference_batch(xs, il, energy_scale=torch.ones(B, T + 1, device=DEV))
            with pytest.raises(ValueError, match="energy_shift"):
                model.inference_batch(xs, il, energy_shift=torch.zeros(B, 1))
            with pytest.raises(ValueError, match="predictions"):
                model._run(xs, il, ds=_used_durations(r, il).to(DEV), es=r["e_outs"], ps=r["p_outs"], is_inference=False, prosody=dict(pitch_scale=1.1))
        assert names(model) == []                                           # nothing was launched by any of them
        # the library's own checks (a binding that skips the Python ones): refused by fs2_decode_ctl before ITS first launch
        real = F._prosody.prosody_struct

        def wrong_cols(ctl):
            s = real(ctl)
            s.pitch_scale_cols = T + 1
            return s

        def wrong_size(ctl):
            s = real(ctl)
            s.struct_size += 8
            return s
        for fake, msg in ((wrong_cols, "pitch_scale_cols"), (wrong_size, "struct_size")):
            monkeypatch.setattr(F._prosody, "prosody_struct", fake)
            model.set_profiling(True)
            with torch.no_grad():
                with pytest.raises(_lib.Fs2Error, match=msg) as e:
                    model._run(xs, il, is_inference=True, prosody=dict(pitch_scale=1.1))
            assert e.value.code == -1
            got = names(model)
            assert got and not any(n.startswith(("lr.", "var.", "dec.", "energy", "pitch", "postnet", "feat_out", "unpack")) for n in got), got
        monkeypatch.setattr(F._prosody, "prosody_struct", real)
    finally:
        model.set_profiling(False)
    r2 = run(model, "fp32", "b3")                                           # and the handle is as good as before
    assert torch.equal(r2["after"], r["after"])


def _dev_means(c, positive_only, **kw):
    from fastspeech2_amd import label_means
    return label_means(torch.from_numpy(c.x).to(DEV), torch.from_numpy(c.labels).to(DEV), kw.get("lens", torch.from_numpy(c.lens).to(DEV)), c.Tmax,
                       positive_only=positive_only)


@pytest.mark.parametrize("S", P.STRIDES)
@pytest.mark.parametrize("Tmax", P.TMAXES)
def test_label_means_on_the_device_equal_the_oracle(Tmax, S):
    c = P.means_case(Tmax, S)
    for positive_only in (False, True):
        mean, count = _dev_means(c, positive_only)
        want_mean, want_count = c.want[positive_only]
        assert mean.dtype == torch.float32 and count.dtype == torch.int32 and mean.shape == count.shape == (P.B, Tmax)
        assert np.array_equal(count.cpu().numpy(), want_count)
        assert P.same_bits(mean.cpu().numpy(), want_mean)
    mean, _ = _dev_means(c, False, lens=c.lens.tolist())                   # host lengths are accepted too
    assert P.same_bits(mean.cpu().numpy(), c.want[False][0])


def test_label_means_under_stream_capture_and_empty_batches():
    from fastspeech2_amd import label_means
    c = P.means_case(130, 300)
    x, lab, lens = (torch.from_numpy(a).to(DEV) for a in (c.x, c.labels, c.lens))
    eager = label_means(x, lab, lens, c.Tmax, positive_only=True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            mean, count = label_means(x, lab, lens, c.Tmax, positive_only=True)
        mean.fill_(float("nan"))                                            # whatever the capture left: only a replay's numbers count
        count.fill_(-5)
        graph.replay()
    side.synchronize()
    assert P.same_bits(mean.cpu().numpy(), eager[0].cpu().numpy()) and torch.equal(count, eager[1])
    assert P.same_bits(mean.cpu().numpy(), c.want[True][0])
    none = label_means(torch.zeros(0, 5, device=DEV), torch.zeros(0, 5, dtype=torch.int32, device=DEV), [], 3)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)
    wide = label_means(torch.zeros(2, 0, device=DEV), torch.zeros(2, 0, dtype=torch.int32, device=DEV), [0, 0], 3)
    assert not wide[0].any() and not wide[1].any() and wide[0].shape == (2, 3)
    with pytest.raises(TypeError, match="int32"):
        label_means(x, lab.long(), lens, c.Tmax)
    with pytest.raises(ValueError, match="lens"):
        label_means(x, lab, lens[:2], c.Tmax)
