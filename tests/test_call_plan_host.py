"""Host-side checks of the call plan (no GPU): csrc/call_plan.h -- what fs2_encode / fs2_decode refuse and which launches a call consists of -- compiled with the
host compiler (tests/gemm_plan_probe.cpp, the driver of tests/test_gemm_plan_host.py, whose encode() / decode() branch on the plan fields fs2_runtime.hip branches on).

(a) names: the ordered profile names of one teacher-forced forward of tools/forward_digest.py's three utterances, sub-launches included, equal the lists recorded
    on a GPU from the parent commit -- its 16 cases (profiles/model_launches_names_parent.json) and the cases of the call plan
    (profiles/call_plan_names_parent.json).  The token and frame counts are make_inputs()'s, the row counts csrc/layout_rule.h's: none is typed in here;
(b) decisions: every field of EncodePlan / DecodePlan over precision x FS2_TOKPROJ x FS2_FUSE_VAR x FS2_ROW8 x input layer x reduction_factor x postnet_layers x
    tok.proj buffer x es / ps given x e_out / p_out asked x layout, and the output decisions over the layout, the outputs given, their alignment, the batch
    semantics and the control.  The expected values are the expressions of fs2_encode / fs2_decode_ctl of commit a429589 (the parent of the call plan), quoted
    at expected_encode / expected_decode / expected_out below and restated in Python; nothing is read back from the tree;
(c) refusals: every refusal of check_encode / check_decode with its FS2_ERR_* code and text, and for each pair of conditions the parent tests in sequence one
    case (`a+b`) in which both hold: the first one answers."""
import importlib.util
import json
import os
import re

import pytest

from tests.test_gemm_plan_host import ERR_ARG, ERR_STATE, MODES, REGIMES, ROOT, probe  # noqa: F401  (probe: the fixture)


# ------------------------------------------------------------------ (a) names
def _forward_digest():
    spec = importlib.util.spec_from_file_location("forward_digest", os.path.join(ROOT, "tools", "forward_digest.py"))
    fd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fd)
    return fd


@pytest.fixture(scope="module")
def utterances():
    """tokens,frames of forward_digest's three utterances, from its make_inputs() (the synthetic batch; no GPU: only the lengths are looked at)."""
    from fastspeech2_amd.synthetic import make_batch
    fd = _forward_digest()
    b = make_batch("c2", seed=11, B=len(fd.TLENS), tlens=fd.TLENS)
    assert [int(t) for t in b["ilens"]] == fd.TLENS
    return ["%d,%d" % (int(t), int(f)) for t, f in zip(b["ilens"], b["olens"])]


def _recorded(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return json.load(f)


PARENT_CASES = sorted("%s/%s/%s" % (b, m, r) for b in ("default", "pre_ln_concat") for m in MODES for r in ("auto", "row8"))


@pytest.mark.parametrize("case", PARENT_CASES)
def test_names_are_the_parents(probe, utterances, case):
    block, mode, row8 = case.split("/")
    got = probe("names", block, mode, "row8=1" if row8 == "row8" else "-", *utterances)
    want = _recorded("model_launches_names_parent.json")[case]
    assert len(want) > 40
    assert got == want


# forward_digest's CALL_CASES -> the probe's (block, case): what each forward gives and asks for (tools/forward_digest.py: call_forward)
_FREE = "es=0,ps=0"
CALL_CASES = {
    "default/bf16x3/tokproj0": "tokproj=0", "default/bf16x3/tokproj1": "tokproj=1", "default/bf16x3/tokproj2": "tokproj=2",
    "default/mix_mx4/tokproj0": "tokproj=0", "default/mix_mx4/tokproj1": "tokproj=1", "default/mix_mx4/tokproj2": "tokproj=2",
    "default/bf16x3/fuse_var0": "fuse_var=0",
    "default/bf16x3/free_running": _FREE,
    "default/bf16x3/pitch_control": _FREE + ",ctl=1",
    "rf2/fp32/teacher": "rf=2", "rf2/bf16x3/teacher": "rf=2",
    "default/bf16x3/device_packed": _FREE + ",e_out=0,p_out=0,after=0,before=0,packed=1,devlay=1",
}


def test_call_cases_are_forward_digests():
    assert set(CALL_CASES) == set(_forward_digest().CALL_CASES) == set(_recorded("call_plan_names_parent.json"))


@pytest.mark.parametrize("case", sorted(CALL_CASES))
def test_call_case_names_are_the_parents(probe, utterances, case):
    got = probe("names", "default", case.split("/")[1], CALL_CASES[case], *utterances)
    want = _recorded("call_plan_names_parent.json")[case]
    assert len(want) > 40
    assert got == want


def test_default_walk_is_the_default_call(probe):
    """With the default options the probe's model walk is the call the runtime makes: tok.proj in the bf16 modes and neither var.conv0 nor dec.in."""
    launches = {}
    for line in probe("model", *REGIMES["c1"], "-"):
        f = line.split()
        launches.setdefault(f[0], set()).add(f[1])
    for mode in MODES:
        if mode == "fp32":
            assert {"energy.conv0", "pitch.conv0", "dec.in"} <= launches[mode] and "tok.proj" not in launches[mode]
        else:
            assert "tok.proj" in launches[mode] and not {"var.conv0", "dec.in", "energy.conv0"} & launches[mode] and "var.conv1" in launches[mode]


# ------------------------------------------------------------------ (b) decisions
FP32, BF16X3 = 0, 1                                                     # include/fs2.h: FS2_PREC_FP32, FS2_PREC_BF16X3 (the base precision of every mixed mode)
FFN_TERMS = {"fp32": 0, "bf16x3": 0, "mix_mx": 9, "mix_mx4": 10}      # model_launches.h: ffn_f16_terms
VAR_CHANS, WIDTH = 256, 384                                             # the probe's model in `decisions`: adim = ddim = 384, so adim % 32 == 0 and var2.ok


def _fields(text):
    return {k: int(v) for k, v in (kv.split("=") for kv in text.split())}


def expected_encode(mode, c):
    """fs2_encode at a429589:
        const int prec = base_precision(b.precision), ffn_terms = ffn_f16_terms(b.precision);
        const bool enc_pl = prec != FS2_PREC_FP32;
        embed_pe(..., enc_pl && c.adim % 32 == 0 ? sb.x0p : nullptr);
        if (enc_pl && h->tokw.N && t.tokp && opts().tokproj) {
            const bool conv = (opts().tokproj & 1) && opts().fuse_var;
            const int n0 = conv ? 0 : 6 * c.var_chans;
            launch_gemm(h, s, "tok.proj", a, opts().tokproj_f32 ? FS2_PREC_FP32 : prec)
    with t.tokp = (tok_proj_cols(c) && b.precision != FS2_PREC_FP32) ? ... : nullptr and tokw loaded where the model has an input layer."""
    pl = mode != "fp32"
    tok_proj = pl and c["in"] and c["tokp"] and c["tokproj"] != 0
    conv = tok_proj and (c["tokproj"] & 1) and c["fuse"]
    return dict(prec=BF16X3 if pl else FP32, ffn_terms=FFN_TERMS[mode], planes=pl, embed_planes=pl, tok_proj=tok_proj, tok_conv=conv,
                tok_n0=(0 if conv else 6 * VAR_CHANS) if tok_proj else 0, tok_prec=BF16X3 if pl else FP32)


def expected_decode(mode, c, enc):
    """fs2_decode_ctl at a429589:
        const bool devlay = io->olens == nullptr && io->row_capacity > 0;
        void* hfr_planes = (prec != FS2_PREC_FP32 && c.adim % 32 == 0) ? f.sb.x1p : nullptr;
        const bool need_e = (io->es == nullptr) || io->e_out, need_p = (io->ps == nullptr) || io->p_out;
        const bool fused_var = need_e && need_p && prec != FS2_PREC_FP32 && h->var2.ok && hfr_planes && opts().fuse_var;
        const int tokproj = (prec != FS2_PREC_FP32 && h->tokP && c.decoder_input_layer) ? (opts().tokproj & ((fused_var && h->tokP_conv) ? 3 : 2)) : 0;
        const bool dec_pl = prec != FS2_PREC_FP32;
        const bool po = dec_pl && planes_only(dec_in, h->dec, c.ddim, rows, f.sb, prec, ffn_terms, opts());
        const int rf = std::max(c.reduction_factor, 1);
        const bool post_pl = dec_pl && c.postnet_layers > 1 && rf == 1;
    planes_only at 896 rows of a 384-wide default block: where FS2_ROW8 = 1 forces the row-complete kernels (test_planes_only_agrees_with_the_old_predicate)."""
    pl = mode != "fp32"
    need_e, need_p = (not c["es"]) or c["e_out"], (not c["ps"]) or c["p_out"]
    fused = need_e and need_p and pl and c["fuse"]
    tokproj = (c["tokproj"] & (3 if fused and enc["tok_conv"] else 2)) if pl and enc["tok_proj"] and c["in"] else 0
    return dict(prec=BF16X3 if pl else FP32, ffn_terms=FFN_TERMS[mode], devlay=c["devlay"], planes=pl, hfr_planes=pl, need_e=need_e, need_p=need_p, fused_var=fused,
                tokproj=tokproj, control=0, po=pl and c["row8"] == 1, mask_q=0, rf=c["rf"], post_pl=pl and c["post"] > 1 and c["rf"] == 1, ep_stored=0)


def expected_out(c):
    """fs2_decode_ctl at a429589:
        if (ctl_pitch || ctl_energy) { ... "var.control"
        const int mask_q = (b.compat_padded && io->masked) ? 1 : 0;
        const int* lim_msk = (b.compat_padded && !io->masked) ? dl.len : dl.vlen;          (e_out / p_out)
        pack_rows(..., (devlay && R == io->row_capacity) ? ovf : nullptr, rf);  packed_done = devlay && R == io->row_capacity;
        const bool need_poison = devlay && ((io->after && !after_done) || (io->before && !before_done) || (io->after_packed && !packed_done));
        poison_on_overflow(..., (io->after && !after_done) ? n : 0, ..., (io->after_packed && !packed_done) ? n : 0, ..., (io->before && !before_done) ? n : 0)
    after_done / before_done: unpack took unpack_rows4 (W % 4 == 0 && fill == 0.f && both pointers 16-byte aligned), which looks at the flags itself."""
    dev = c["devlay"]
    packed_ovf = dev and c["rows_are_capacity"]
    out = dict(control=c["ctl_pitch"] or c["ctl_energy"], mask_q=c["compat"] and c["masked"], ep_stored=c["compat"] and not c["masked"], packed_ovf=packed_ovf,
               poison_after=dev and c["after"] and not c["after_vec"], poison_before=dev and c["before"] and not c["before_vec"],
               poison_packed=dev and c["packed"] and not packed_ovf)
    out["poison"] = out["poison_after"] or out["poison_before"] or out["poison_packed"]
    return out


@pytest.fixture(scope="module")
def decisions(probe):
    out = {"enc": [], "dec": [], "out": []}
    for line in probe("decisions"):
        coords, fields = line.split(" | ")
        kind, *rest = coords.split()
        mode = rest.pop(0) if kind != "out" else None
        out[kind].append((mode, _fields(" ".join(rest)), _fields(fields)))
    return out


def _same(got, want):
    return got == {k: int(v) for k, v in want.items()}


def test_decisions_are_the_parents_expressions(decisions):
    n_model = len(MODES) * 4 * 2 * 2 * 2 * 2 * 3 * 2      # mode x tokproj x fuse_var x row8 x input layer x rf x postnet layers x tok.proj buffer
    assert len(decisions["enc"]) == n_model and len(decisions["dec"]) == n_model * 4 * 4 * 2 and len(decisions["out"]) == 1 << 11
    enc_of = {}
    for mode, c, got in decisions["enc"]:
        want = expected_encode(mode, c)
        assert _same(got, want), (mode, c, got, want)
        enc_of[(mode,) + tuple(sorted(c.items()))] = want
    for mode, c, got in decisions["dec"]:
        key = {k: v for k, v in c.items() if k not in ("es", "ps", "e_out", "p_out", "devlay")}
        want = expected_decode(mode, c, enc_of[(mode,) + tuple(sorted(key.items()))])
        assert _same(got, want), (mode, c, got, want)
    for _, c, got in decisions["out"]:
        assert _same(got, expected_out(c)), (c, got, expected_out(c))


def _dec(decisions, mode, **coords):
    base = dict(tokproj=3, fuse=1, row8=-1, rf=1, post=5, tokp=1, es=1, ps=1, e_out=1, p_out=1, devlay=0)
    base["in"] = 1
    base.update(coords)
    (hit,) = [got for m, c, got in decisions["dec"] if m == mode and c == base]
    return hit


def test_decisions_the_issue_names(decisions):
    """The cases the sweep must hold, one by one (default options: tokproj 3, fused predictors, an input layer, 5 Postnet layers, teacher-forced with e_out / p_out)."""
    d = _dec(decisions, "bf16x3")
    assert d["tokproj"] == 3 and d["fused_var"] == 1                      # -> lr.index runs, var.embed does not (decode() / fs2_decode_ctl branch on tokproj alone)
    d = _dec(decisions, "bf16x3", e_out=0)                               # es given and e_out not asked: only the pitch is predicted
    assert (d["need_e"], d["need_p"], d["fused_var"], d["tokproj"]) == (0, 1, 0, 2)
    assert _dec(decisions, "bf16x3", p_out=0)["tokproj"] == 2
    assert _dec(decisions, "bf16x3", es=0, e_out=0)["tokproj"] == 3      # nothing given: predicted whether asked for or not
    assert _dec(decisions, "fp32")["tokproj"] == 0
    assert _dec(decisions, "bf16x3", **{"in": 0})["tokproj"] == 0
    assert _dec(decisions, "bf16x3", tokp=0)["tokproj"] == 0
    assert _dec(decisions, "bf16x3", fuse=0)["tokproj"] == 2 and _dec(decisions, "bf16x3", tokproj=1, fuse=0)["tokproj"] == 0
    for mode in ("bf16x3", "mix_mx", "mix_mx4"):
        assert _dec(decisions, mode)["post_pl"] == 1
        assert _dec(decisions, mode, rf=2)["post_pl"] == 0 and _dec(decisions, mode, post=1)["post_pl"] == 0 and _dec(decisions, mode, post=0)["post_pl"] == 0
        assert _dec(decisions, mode, row8=1)["po"] == 1 and _dec(decisions, mode)["po"] == 0
    assert _dec(decisions, "fp32", row8=1)["po"] == 0 and _dec(decisions, "fp32")["post_pl"] == 0


def test_poison_decision(decisions):
    """Device-driven layout: poison_on_overflow is needed for exactly the outputs whose writer does not look at the overflow flags itself."""
    def out(**coords):
        base = dict(devlay=1, after=1, before=0, packed=0, after_vec=1, before_vec=1, compat=0, masked=0, ctl_pitch=0, ctl_energy=0, rows_are_capacity=1)
        base.update(coords)
        (hit,) = [got for _, c, got in decisions["out"] if c == base]
        return hit
    assert out()["poison"] == 0
    assert out(after_vec=0)["poison_after"] == 1 and out(after_vec=0)["poison"] == 1                      # an output the unpack_rows4 fast path does not take
    assert out(before=1, before_vec=0)["poison_before"] == 1 and out(before=1, before_vec=0)["poison_after"] == 0
    assert out(before=0, before_vec=0)["poison"] == 0                                                     # not given: nothing to poison
    assert out(packed=1)["poison"] == 0 and out(packed=1)["packed_ovf"] == 1
    d = out(packed=1, rows_are_capacity=0)                                                                # after_packed with R != row_capacity
    assert (d["packed_ovf"], d["poison_packed"], d["poison_after"], d["poison"]) == (0, 1, 0, 1)
    assert out(devlay=0, after_vec=0, before=1, before_vec=0, packed=1, rows_are_capacity=0)["poison"] == 0      # the host layout has no overflow


# ------------------------------------------------------------------ (c) refusals
_BATCH = "batch: B=%d Tmax=%d ilens=%s"
_TOGETHER = "batch: regime_tokens=%d / regime_utterances=%d must be given together (0 / 0 = this call's own batch)"
_COLS = "fs2_decode_ctl: %s_cols = %d is neither 1 (per utterance) nor Tmax = 33 (per phoneme)"
_PAIRING = "fs2_decode: batch does not match the preceding fs2_encode"
_GIVEN = "fs2_decode: olens (or row_capacity) / workspace / after (or after_packed) must be given"
_ENC_GIVEN = "fs2_encode: xs/olens/workspace must be given"
CALL_REFUSALS = {
    "enc.accepted": (0, ""),
    "enc.batch_empty": (ERR_ARG, _BATCH % (0, 33, "PTR")),
    "enc.batch_tmax": (ERR_ARG, _BATCH % (3, 0, "PTR")),
    "enc.batch_ilens+precision": (ERR_ARG, _BATCH % (3, 33, "(nil)")),
    "enc.ilens_zero": (ERR_ARG, "ilens[1]=0 outside [1,33]"),
    "enc.ilens_long+precision": (ERR_ARG, "ilens[2]=34 outside [1,33]"),
    "enc.precision_low": (ERR_ARG, "unknown precision mode -1"),
    "enc.precision+regime": (ERR_ARG, "unknown precision mode 7"),
    "enc.regime_tokens_alone+xs": (ERR_ARG, _TOGETHER % (5, 0)),
    "enc.regime_utterances_alone": (ERR_ARG, _TOGETHER % (0, 2)),
    "enc.regime_negative": (ERR_ARG, _TOGETHER % (-1, -1)),
    "enc.regime_accepted": (0, ""),
    "enc.xs+alpha": (ERR_ARG, _ENC_GIVEN),
    "enc.olens": (ERR_ARG, _ENC_GIVEN),
    "enc.workspace": (ERR_ARG, _ENC_GIVEN),
    "enc.alpha+pe": (ERR_ARG, "fs2_encode: duration_alpha -0.5 must be > 0 (0 = 1.0)"),
    "enc.pe": (ERR_ARG, "sequence longer than the positional table (32 rows): extend `pe` and reload"),
    "enc.pe_exact": (0, ""),
    "enc.pe_padded_batch": (ERR_ARG, "sequence longer than the positional table (39 rows): extend `pe` and reload"),
    "dec.accepted": (0, ""),
    "dec.devlay_accepted": (0, ""),
    "dec.ctl_accepted": (0, ""),
    "dec.ctl_per_phoneme_accepted": (0, ""),
    "dec.ctl_neutral_cols_ignored": (0, ""),
    "dec.ctl_pitch_scale_cols+ps": (ERR_ARG, _COLS % ("pitch_scale", 2)),
    "dec.ctl_pitch_shift_cols+energy_scale_cols": (ERR_ARG, _COLS % ("pitch_shift", 0)),
    "dec.ctl_energy_scale_cols": (ERR_ARG, _COLS % ("energy_scale", 34)),
    "dec.ctl_energy_shift_cols+es": (ERR_ARG, _COLS % ("energy_shift", 3)),
    "dec.ctl_ps+es": (ERR_ARG, "fs2_decode_ctl: pitch control together with given pitches (io->ps): control acts on predictions"),
    "dec.ctl_pitch_with_es_accepted": (0, ""),
    "dec.ctl_es+compat": (ERR_ARG, "fs2_decode_ctl: energy control together with given energies (io->es): control acts on predictions"),
    "dec.ctl_compat+no_encode": (ERR_ARG, "fs2_decode_ctl: control has per-utterance semantics only (batch.compat_padded must be 0)"),
    "dec.no_encode+batch": (ERR_STATE, "fs2_decode called without a preceding fs2_encode"),
    "dec.batch_empty": (ERR_ARG, _BATCH % (0, 33, "PTR")),
    "dec.precision+pairing": (ERR_ARG, "unknown precision mode 99"),
    "dec.pairing_B": (ERR_STATE, _PAIRING),
    "dec.pairing_Tmax": (ERR_STATE, _PAIRING),
    "dec.pairing_compat": (ERR_STATE, _PAIRING),
    "dec.pairing_workspace+workspace": (ERR_STATE, _PAIRING),
    "dec.olens": (ERR_ARG, _GIVEN),
    "dec.workspace": (ERR_ARG, _GIVEN),
    "dec.after": (ERR_ARG, _GIVEN),
    "dec.after_packed_accepted": (0, ""),
    "dec.after+status": (ERR_ARG, _GIVEN),
    "dec.status+Lmax": (ERR_ARG, "fs2_decode: the device-driven layout needs a status buffer"),
    "dec.devlay_Lmax": (ERR_ARG, "row_capacity 1024 / Lmax 0"),
    "dec.row_capacity": (ERR_ARG, "row_capacity 2147483392 / Lmax 264"),
    "dec.row_capacity_accepted": (0, ""),
    "dec.bad_id+empty": (ERR_ARG, "utterance 1 holds a phoneme id outside [0, 68) (fs2_encode marks it with the frame count -1)"),
    "dec.empty+Lmax": (ERR_ARG, "olens[1]=0"),
    "dec.negative": (ERR_ARG, "olens[1]=-2"),
    "dec.Lmax+pe": (ERR_ARG, "Lmax 263 < longest utterance 264"),
    "dec.pe": (ERR_ARG, "utterance of 264 frames exceeds the positional table (263 rows): extend `pe` and reload"),
    "dec.pe_exact": (0, ""),
}


def test_call_refusals_keep_their_codes_and_order(probe):
    got = {}
    for line in probe("call_refusals"):
        what, err, msg = line.split("|")
        got[what] = (int(err), re.sub(r"0x[0-9a-f]+", "PTR", msg))
    assert got == CALL_REFUSALS
