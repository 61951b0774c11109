"""CPU: the oracle restatement replayed against the golden vectors captured from the real reference
(oracle/gen_golden.py).  This is what pins the oracle on machines where /root/reference is absent."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def env():
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    from oracle import fs2_oracle as O
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp)
    sd = portable_state_dict(model.state_dict(), seed=0)
    return sd, O.config_from_hp(hp, N_PHONEME_SYMBOLS, hp.audio.num_mels), O


def _t(a):
    return torch.from_numpy(np.asarray(a))


TOL = 2e-5   # same torch ops on a possibly different CPU/BLAS build: summation-order noise only


def test_g1(env, golden_dir):
    sd, cfg, O = env
    g = np.load(golden_dir + "/g1_teacher_b1.npz")
    o = O.padded_forward(sd, cfg, _t(g["xs"]), _t(g["ilens"]), _t(g["olens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]))
    for k in ("before", "after", "d_outs", "e_outs", "p_outs", "encoder_out"):
        assert float((o[k] - _t(g[k])).abs().max()) <= TOL, k
    assert o["lr_index"][0].tolist() == g["lr_index"].tolist()
    assert o["qe"].tolist() == g["qe"].tolist() and o["qp"].tolist() == g["qp"].tolist()
    rows = _t(g["decoder_rows"])
    assert float((o["decoder_out"][0][rows] - _t(g["decoder_out_rows"])).abs().max()) <= TOL


def test_g2_and_losses(env, golden_dir):
    sd, cfg, O = env
    g = np.load(golden_dir + "/g2_teacher_padded_b3.npz")
    o = O.padded_forward(sd, cfg, _t(g["xs"]), _t(g["ilens"]), _t(g["olens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]))
    for k in ("before", "after", "d_outs", "e_outs", "p_outs"):
        assert float((o[k] - _t(g[k])).abs().max()) <= TOL, k
    loss, rep = O.loss_report(o, _t(g["ys"]), _t(g["ilens"]), _t(g["olens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]))
    assert [list(d.keys())[0] for d in rep] == g["report_names"].tolist()
    assert np.allclose([list(d.values())[0] for d in rep], g["report_values"], rtol=1e-5)


def test_g9_weighted_masking_losses(env, golden_dir):
    """hp.model.use_weighted_masking (reference fastspeech.py:308-333; runs only with use_masking = False): the oracle's loss algebra
    against the real reference's loss and 7 report values."""
    sd, cfg, O = env
    g = np.load(golden_dir + "/g9_weighted_masking_b3.npz")
    o = O.padded_forward(sd, cfg, _t(g["xs"]), _t(g["ilens"]), _t(g["olens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]))
    loss, rep = O.loss_report(o, _t(g["ys"]), _t(g["ilens"]), _t(g["olens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]),
                              use_masking=False, use_weighted_masking=True)
    assert [list(d.keys())[0] for d in rep] == g["report_names"].tolist()
    assert np.allclose([list(d.values())[0] for d in rep], g["report_values"], rtol=1e-5)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))


def test_g6_per_utterance(env, golden_dir):
    sd, cfg, O = env
    g2 = np.load(golden_dir + "/g2_teacher_padded_b3.npz")
    g6 = np.load(golden_dir + "/g6_teacher_per_utt_b3.npz")
    o = O.per_utterance_forward(sd, cfg, _t(g2["xs"]), _t(g2["ilens"]), _t(g2["ds"]), _t(g2["es"]), _t(g2["ps"]))
    for b in range(3):
        L = int(g2["olens"][b])
        assert float((o["after"][b, :L] - _t(g6["after_%d" % b])).abs().max()) <= TOL
        assert float(o["after"][b, L:].abs().max() if L < o["after"].shape[1] else 0) == 0


def test_g3_inference(env, golden_dir):
    sd, cfg, O = env
    from fastspeech2_amd.synthetic import bias_durations
    g = np.load(golden_dir + "/g3_inference_t24.npz")
    o = O.padded_forward(bias_durations(sd, 4.0), cfg, _t(g["x"]).unsqueeze(0), torch.tensor([24]), is_inference=True)
    assert o["d_outs"][0].tolist() == g["d_outs"][0].tolist()
    assert float((o["after"][0] - _t(g["mel"])).abs().max()) <= TOL


def test_g4_known_answers(env, golden_dir):
    sd, cfg, O = env
    g = np.load(golden_dir + "/g4_known_answers.npz")
    assert O.bucketize(_t(g["xe"]), _t(g["energy_bins"])).tolist() == g["qe"].tolist()
    assert O.bucketize(_t(g["xp"]), _t(g["pitch_bins"])).tolist() == g["qp"].tolist()
    assert g["qe"][0] == 0 and g["qe"][5] == 255 and g["qe"][6] == 255          # below range, above range, NaN
    assert O.duration_from_log(_t(g["dur_log"])).tolist() == g["dur_int"].tolist()
    assert g["dur_int"].tolist()[:6] == [0, 0, 0, 2, 2, 4]                     # round half to even: .5->0, 1.5->2, 2.5->2, 3.5->4
    out, olens, idx = O.length_regulate(_t(g["lr_hs"]), _t(g["lr_ds"]), _t(g["lr_ilens"]))
    assert torch.equal(out, _t(g["lr_out"])) and olens.tolist() == [7, 4, 2]
    assert torch.equal(~O._len_mask([5, 3, 2], 5), _t(g["pad_mask_5_3_2"]).bool())
    # the positional tables: float32 exp / sin / cos on the CPU run MKL's vector math, whose last bits depend on the code path MKL takes on
    # this host (at t = 4999 one ulp of a frequency is ~1e-4 in the table).  G4 holds the reference's table on MKL's AVX-512 path, G4b the
    # same on each of its x86 paths (AVX-512, AVX2, the compatible path it takes on AMD CPUs): the oracle must equal the reference's table
    # on one of them.
    rows = g["pe_rows"].tolist()
    pe = np.load(golden_dir + "/g4b_positional_mkl_paths.npz")
    assert pe["pe_rows"].tolist() == rows
    for d in (256, 384):
        assert np.array_equal(pe["pe%d_avx512" % d], g["pe%d" % d])
        got = O.positional_table(5000, d)[rows]
        diffs = {k: float((got - _t(pe[k])).abs().max()) for k in pe.files if k.startswith("pe%d_" % d)}
        assert min(diffs.values()) <= 1e-6, diffs
    valid = O._len_mask([6, 3], 6)
    att = O._mha(sd, "encoder.encoders_.0.self_attn", _t(g["attn_x"]), valid.unsqueeze(-2) & valid.unsqueeze(-1), 2)
    assert float((att - _t(g["attn_out"])).abs().max()) <= TOL
    # fully masked query rows -> linear_out.bias   
    bo = sd["encoder.encoders_.0.self_attn.linear_out.bias"]
    assert float((att[1, 3:] - bo).abs().max()) <= 1e-6


def test_g5_script_twin(golden_dir):
    """The TorchScript twin of the reference (utils/fastspeech2_script.py): oracle with the twin architecture."""
    from fastspeech2_amd import default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.fastspeech2_script import FeedForwardTransformer as Twin
    from fastspeech2_amd.synthetic import portable_state_dict, bias_durations
    from oracle import fs2_oracle as O
    g = np.load(golden_dir + "/g5_script_twin_t30.npz")
    hp = default_hparams()
    twin = Twin(N_PHONEME_SYMBOLS, 80, hp)
    sd_t = twin.state_dict()
    assert sorted(sd_t.keys()) == g["keys"].tolist()                        # reference twin's state-dict layout
    assert [str(tuple(sd_t[k].shape)) for k in sorted(sd_t)] == g["shapes"].tolist()
    assert sum(p.numel() for p in twin.parameters()) == 26691573
    sd = bias_durations(portable_state_dict(sd_t, seed=5), 4.0)
    o = O.padded_forward(sd, O.config_from_hp(hp, N_PHONEME_SYMBOLS, 80, script_twin=True), _t(g["x"]).unsqueeze(0),
                         torch.tensor([30]), is_inference=True)
    assert float((o["after"][0] - _t(g["mel"])).abs().max()) <= TOL


BLOCK_VARIANTS = {      # as in oracle/gen_golden.py (the generating script): hp.model overrides of fixture G7
    "pre_ln": dict(encoder_normalize_before=True, decoder_normalize_before=True),
    "concat_after": dict(encoder_concat_after=True, decoder_concat_after=True),
    "pre_ln_concat": dict(encoder_normalize_before=True, decoder_normalize_before=True, encoder_concat_after=True, decoder_concat_after=True),
    "enc_pre_ln_dec_concat": dict(encoder_normalize_before=True, decoder_concat_after=True),
}


def variant_setup(name):
    """hp, portable weights (seed 21) and oracle config of one G7 block variant."""
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict
    from oracle import fs2_oracle as O
    hp = default_hparams()
    for k, v in BLOCK_VARIANTS[name].items():
        hp.model[k] = v
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    sd = portable_state_dict(model.state_dict(), seed=21)
    return hp, model, sd, O.config_from_hp(hp, N_PHONEME_SYMBOLS, hp.audio.num_mels)


@pytest.mark.parametrize("name", sorted(BLOCK_VARIANTS))
def test_g7_block_variants(name, golden_dir):
    """normalize_before / concat_after FFT blocks (reference core/encoder.py:53-71,201-202): oracle vs the real reference's outputs."""
    from oracle import fs2_oracle as O
    g = np.load(golden_dir + "/g7_block_variants_b2.npz")
    assert name in g["names"].tolist()
    hp, model, sd, cfg = variant_setup(name)
    o = O.per_utterance_forward(sd, cfg, _t(g["xs"]), _t(g["ilens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]))
    for i in range(2):
        L = int(g["olens"][i])
        assert float((o["after"][i, :L] - _t(g["%s_after_%d" % (name, i)])).abs().max()) <= TOL
        assert float((o["before"][i, :L] - _t(g["%s_before_%d" % (name, i)])).abs().max()) <= TOL


def reduction_setup():
    """hp, model, portable weights (seed 23, duration bias ln(1 + 1.386...)) and oracle config of fixture G8 (reduction_factor = 2)."""
    import math
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, bias_durations
    from oracle import fs2_oracle as O
    hp = default_hparams()
    hp.model.reduction_factor = 2
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    sd = bias_durations(portable_state_dict(model.state_dict(), seed=23), math.log(1 + 3.0))
    return hp, model, sd, O.config_from_hp(hp, N_PHONEME_SYMBOLS, hp.audio.num_mels)


def test_g8_reduction_factor(golden_dir):
    """reduction_factor = 2 (reference fastspeech.py:153,228-230): oracle vs the real reference, teacher-forced and free-running."""
    from oracle import fs2_oracle as O
    g = np.load(golden_dir + "/g8_reduction_factor2_b2.npz")
    hp, model, sd, cfg = reduction_setup()
    assert cfg["reduction_factor"] == 2
    o = O.per_utterance_forward(sd, cfg, _t(g["xs"]), _t(g["ilens"]), _t(g["ds"]), _t(g["es"]), _t(g["ps"]))
    f = O.per_utterance_forward(sd, cfg, _t(g["xs"]), _t(g["ilens"]), is_inference=True)
    for i in range(2):
        L = 2 * int(g["olens"][i])
        assert float((o["after"][i, :L] - _t(g["tf_after_%d" % i])).abs().max()) <= TOL
        assert float((o["before"][i, :L] - _t(g["tf_before_%d" % i])).abs().max()) <= TOL
        y = _t(g["free_after_%d" % i])
        assert y.shape[0] == 2 * int(f["olens"][i])
        assert float((f["after"][i, : y.shape[0]] - y).abs().max()) <= TOL
