// Host-compiled driver of csrc/gemm_plan.h, csrc/attn_plan.h, csrc/model_launches.h, csrc/call_plan.h and csrc/weight_plan.h for tests/test_gemm_plan_host.py,
// tests/test_attn_plan_host.py, tests/test_call_plan_host.py and tests/test_weight_plan_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe model <Rtok> <regime_tok> <Rfr> <regime_fr> <case>   the plan of every GEMM and attention launch of a teacher-forced forward of the default model, in the four tested precisions
//   probe names <block> <mode> <case> <tokens,frames>..    the ordered profile names of one forward (rows: layout_rule.h), sub-launches (.planes, .rows, .split) included
//   probe decisions                                        every field of EncodePlan / DecodePlan over the inputs they are functions of
//   probe call_refusals                                    one argument set per refusal of check_encode / check_decode, and one per pair the entry points test in sequence
//   probe variants <Rtok> <regime_tok> <Rfr> <regime_fr>   every step of the pre-LN / concat_after block variants, and whether its GEMMs plan
//   probe sweep                                            the planes-only decision: the predicate fs2_decode used to restate against the plan's answer
//   probe refusals                                         one argument set per refusal of plan_gemm
//   probe attn_sweep                                       plan_attention over the regime threshold, the switch, the plane distances, the grid and the scales
//   probe attn_refusals                                    the refusals of plan_attention
//   probe weights <model>                                  every layer of a model as the loader asks for it, with the plan's answer: the byte size of every image
//   probe weight_sweep                                     plan_weight over the asks: `coordinates | fields`
// <case>: key=value,... (or -): the options tokproj, tokproj_f32, fuse_var, row8; the model's rf (reduction_factor), post (postnet_layers), in (decoder input layer); the call's
// es, ps, e_out, p_out, dec_out, after, before, packed, ctl, devlay (0 / 1), tokp (the token workspace has tok.proj's buffer).  Default: the default options, a teacher-forced forward.
// The launches are the ones model_launches.h forms and call_plan.h decides on, the headers fs2_runtime.hip executes: encode() and decode() below are its two entry points
// without the kernels, branching on the same plan fields.  This file holds only data: a model described as the loader leaves it -- the asks of weight_plan.h's
// constructors, a marker pointer wherever plan_weight gives an image bytes or the workspace has a buffer -- and the walk over the headers' step lists.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "attn_plan.h"
#include "call_plan.h"
#include "weight_plan.h"

using namespace fs2;

namespace {

float kMarkStorage[2];
float* const M = kMarkStorage;      // a non-null pointer nobody follows
unsigned char* const MB = reinterpret_cast<unsigned char*>(kMarkStorage);
constexpr int kFp32 = kPlanFp32, kBf16x3 = kPlanBf16x3, kBf16 = 2;

int round_up(int x, int a) { return (x + a - 1) / a * a; }

// a layer as the loader leaves it: an image wherever the plan gives it bytes
Gemm gemm(const WeightAsk& ask) {
    const WeightPlan p = plan_weight(ask);
    Gemm g;
    g.C = ask.C; g.Cpad = p.Cpad; g.ktaps = ask.ktaps; g.N = p.N;
    if (p.has(kImgW)) g.w = M;
    if (p.has(kImgWb)) g.wb = M;
    if (p.has(kImgWf)) g.wf = M;
    if (p.has(kImgWm)) g.wm = M;
    if (p.has(kImgWm4)) g.wm4 = M;
    if (p.has(kImgWs4)) g.ws4 = MB;
    if (p.has(kImgBias)) g.bias = M;
    return g;
}
GemmArgs base(int C, int ktaps, int N, int R, bool y) {      // (the refusal cases start from it: a plain layer without a bias)
    return gemm_args(gemm(ask_of(1, N, C, ktaps, ktaps == 1, false)), M, C, R, nullptr, y ? M : nullptr, N);
}

// hp.model as far as the launches and the weights depend on it; the defaults are default_hparams()'
struct Model { int adim = 256, ddim = 384, heads = 2, eunits = 1024, dunits = 1024, kffn = 9, odim = 80, post_layers = 5, post_chans = 256, post_k = 5,
               dur_chans = 256, dur_k = 3, dur_layers = 2, var_chans = 256, var_k = 3, elayers = 4, dlayers = 4, rf = 1, input_layer = 1;
               bool enc_pre_ln = false, enc_concat = false, dec_pre_ln = false, dec_concat = false, use_batch_norm = true, linear_ffn = false; };

// The model's layers in the loader's order (fs2_load_weights), each with the ask the loader forms for it.
struct NamedAsk { std::string name; WeightAsk ask; };
std::vector<NamedAsk> model_asks(const Model& m) {
    std::vector<NamedAsk> out;
    auto stack = [&](const char* tag, int D, int units, int layers, bool concat) {
        const int Dp = att_width(D, m.heads);
        const WeightAsk w1 = ask_ffn_w1(D, units, m.kffn, m.linear_ffn);
        for (int i = 0; i < layers; ++i) {
            const std::string p = std::string(tag) + "." + std::to_string(i) + ".";
            out.push_back({p + "qkv", ask_qkv(D, Dp)}); out.push_back({p + "out", ask_attn_out(D, Dp)});
            out.push_back({p + "w1", w1}); out.push_back({p + "w2", ask_ffn_w2(w1, m.linear_ffn)});
            if (concat) { out.push_back({p + "cat_x", ask_concat_half(D, 0)}); out.push_back({p + "cat_a", ask_concat_half(D, 1)}); }
        }
    };
    auto predictor = [&](const char* tag, int layers, int chans, int k) {
        for (int l = 0; l < layers; ++l) out.push_back({std::string(tag) + ".conv" + std::to_string(l), ask_predictor_conv(l ? chans : m.adim, chans, k)});
    };
    stack("enc", m.adim, m.eunits, m.elayers, m.enc_concat);
    stack("dec", m.ddim, m.dunits, m.dlayers, m.dec_concat);
    predictor("dur", m.dur_layers, m.dur_chans, m.dur_k); predictor("energy", 2, m.var_chans, m.var_k); predictor("pitch", 2, m.var_chans, m.var_k);
    const bool fused = m.var_chans % 128 == 0 && m.adim % 32 == 0;      // (FusedPredictors: two layers)
    if (fused) { out.push_back({"var.c0", ask_fused_predictor_conv(m.adim, m.var_chans, m.var_k)}); out.push_back({"var.c1", ask_fused_predictor_conv(m.var_chans, m.var_chans, m.var_k)}); }
    if (m.input_layer) out.push_back({"dec_in", ask_dec_in(m.adim, m.ddim)});
    if (m.input_layer && fused && m.var_k == 3 && m.ddim % 32 == 0) out.push_back({"tokw", ask_tok_proj(m.adim, 6 * m.var_chans + m.ddim)});      // (tok_proj_cols)
    out.push_back({"feat", ask_feat_out(m.ddim, m.odim * m.rf)});
    for (int l = 0; l < m.post_layers; ++l)
        out.push_back({"post." + std::to_string(l), ask_postnet(l ? m.post_chans : m.odim, l == m.post_layers - 1 ? m.odim : m.post_chans, m.post_k, m.use_batch_norm)});
    return out;
}

Stack stack(int D, int heads, int units, int k, int layers, bool pre_ln, bool concat, bool linear_ffn) {
    Stack st;
    st.dk = D / heads; st.Dp = att_width(D, heads); st.pre_ln = pre_ln; st.concat = concat; st.pe = M; st.after_g = st.after_b = M;
    Layer ly;
    const WeightAsk w1 = ask_ffn_w1(D, units, k, linear_ffn);
    ly.qkv = gemm(ask_qkv(D, st.Dp)); ly.out = gemm(ask_attn_out(D, st.Dp)); ly.w1 = gemm(w1); ly.w2 = gemm(ask_ffn_w2(w1, linear_ffn));
    if (concat) { ly.cat_x = gemm(ask_concat_half(D, 0)); ly.cat_a = gemm(ask_concat_half(D, 1)); }
    ly.ln1g = ly.ln1b = ly.ln2g = ly.ln2b = M;
    st.layers.assign(layers, ly);
    return st;
}
Predictor predictor(int cin, int chans, int k) {
    Predictor p;
    p.conv = {gemm(ask_predictor_conv(cin, chans, k)), gemm(ask_predictor_conv(chans, chans, k))};
    p.lng = p.lnb = {M, M}; p.lin_w = p.lin_b = M;
    return p;
}
struct Built {
    Stack enc, dec; Predictor dur, energy, pitch; FusedPredictors var2; Gemm dec_in, feat, tokw; std::vector<Gemm> post; fs2_config cfg;
    explicit Built(const Model& m)
        : enc(stack(m.adim, m.heads, m.eunits, m.kffn, m.elayers, m.enc_pre_ln, m.enc_concat, m.linear_ffn)),
          dec(stack(m.ddim, m.heads, m.dunits, m.kffn, m.dlayers, m.dec_pre_ln, m.dec_concat, m.linear_ffn)),
          dur(predictor(m.adim, m.dur_chans, m.dur_k)), energy(predictor(m.adim, m.var_chans, m.var_k)), pitch(energy), dec_in(gemm(ask_dec_in(m.adim, m.ddim))),
          feat(gemm(ask_feat_out(m.ddim, m.odim * m.rf))), cfg() {
        var2.ok = m.var_chans % 128 == 0;
        var2.c0 = gemm(ask_fused_predictor_conv(m.adim, m.var_chans, m.var_k)); var2.c1 = gemm(ask_fused_predictor_conv(m.var_chans, m.var_chans, m.var_k));
        var2.ln0g = var2.ln0b = var2.ln1g = var2.ln1b = var2.lin_w = var2.lin_b = M;
        for (int l = 0; l < m.post_layers; ++l)
            post.push_back(gemm(ask_postnet(l ? m.post_chans : m.odim, l == m.post_layers - 1 ? m.odim : m.post_chans, m.post_k, m.use_batch_norm)));
        if (m.input_layer && var2.ok) tokw = gemm(ask_tok_proj(m.adim, 6 * m.var_chans + m.ddim));      // (load_tok_proj)
        cfg.idim = 68; cfg.odim = m.odim; cfg.adim = m.adim; cfg.ddim = m.ddim; cfg.aheads = m.heads; cfg.var_chans = m.var_chans; cfg.postnet_layers = m.post_layers;
        cfg.reduction_factor = m.rf; cfg.decoder_input_layer = m.input_layer; cfg.use_scaled_pos_enc = 1;
    }
    DecIn in() const { return cfg.decoder_input_layer ? DecIn{&dec_in, M, M, 1.f} : DecIn(); }
};
const StackBufs kTokBufs{M, M, M, M, M, M, M, M, M, M, M, M, nullptr}, kFrameBufs{M, M, M, M, M, M, M, M, M, M, M, M, MB};      // (carve_tokens / carve_frames: only the frames have xs4)

const char* kernel_name(GemmKernel k) {
    switch (k) {
    case GemmKernel::None: return "none";
    case GemmKernel::RowsF32: return "rows_f32";
    case GemmKernel::TileF32: return "tile_f32";
    case GemmKernel::TileRowsF32: return "tile_rows_f32";
    case GemmKernel::PlBf16: return "pl_bf16";
    case GemmKernel::PlF16: return "pl_f16";
    case GemmKernel::PlMx: return "pl_mx";
    case GemmKernel::PlMx4: return "pl_mx4";
    case GemmKernel::Row8: return "row8";
    case GemmKernel::Row8c: return "row8c";
    case GemmKernel::Row8cGrouped: return "row8c_grouped";
    case GemmKernel::Row8cTwoLn: return "row8c_two_ln";
    case GemmKernel::Row4: return "row4";
    case GemmKernel::Qkv8: return "qkv8";
    case GemmKernel::Qkv4: return "qkv4";
    }
    return "?";
}

const char* attn_name(AttnKernel k) {
    switch (k) {
    case AttnKernel::None: return "none";
    case AttnKernel::F32: return "attn_f32";
    case AttnKernel::B16: return "attn_bf16";
    case AttnKernel::W32: return "attn_w32";
    }
    return "?";
}

struct Call {      // one fs2_encode / fs2_decode: prints a line per GEMM launch, or collects the plans into `all` (capacity test)
    int prec, terms;
    Rows r;
    const char* tag;
    Options o;
    std::string* all = nullptr;
    int nwork = -1;          // the attention work list's items (-1: att_blocks(R), one utterance's)
    int gemm_prec = -1;      // the precision of the next emit() where it is not the call's (tok.proj under FS2_TOKPROJ_F32)
    bool steps = false;      // print every step with its kind and the plan's refusal code instead
    bool names = false;      // print the profile names instead: every launch's, the sub-launches launch_gemm / launch_attention / run_stack add included
    void mark(const char* name) const { if (names) printf("%s\n", name); }      // a launch that is no step of model_launches.h
    void emit(const char* stack, const Step& st) const {
        const std::string name = std::string(stack ? stack : "") + (stack ? "." : "") + st.name;
        if (names && st.kind == StepKind::LayerNorm) printf("%s\n", name.c_str());
        if (steps && st.kind != StepKind::Gemm) printf("%s %s %s 0\n", tag, name.c_str(), st.kind == StepKind::Attention ? "attention" : "layernorm");
        if (st.kind != StepKind::Gemm) return;
        GemmArgs a = st.a;
        call_defaults(a, M, kpart_floats(r.Rpad), r.regime_rows);      // the call's split-K scratch (carve_tokens / carve_frames) and regime
        const GemmPlan p = plan_gemm(a, gemm_prec >= 0 ? gemm_prec : prec, o);
        char line[256];
        if (names) {      // launch_gemm's scopes
            if (p.build_planes) printf("%s.planes\n", name.c_str());
            printf("%s\n", name.c_str());
            if (p.rows_pass) printf("%s.rows\n", name.c_str());
        } else if (all) {
            snprintf(line, sizeof line, "%s %s ns%d nb%d bm%d mt%d k1%d ap%d epi%d ar%d res%d ks%d y%d bp%d rp%d err%d\n", name.c_str(), kernel_name(p.kernel), p.nsplit, p.nb, p.bm, p.mt,
                     (int)p.k1, p.apart, p.epi, p.arith, p.res, p.ksplit, (int)p.y, (int)p.build_planes, (int)p.rows_pass, p.err);
            *all += line;
        } else if (steps) {
            printf("%s %s gemm %d\n", tag, name.c_str(), p.err);
        } else {
            printf("%s %s %s %d %d %d\n", tag, name.c_str(), kernel_name(p.kernel), p.tile_rows(), p.ksplit, (int)p.rows_pass);
        }
    }
    // the attention launch of a block as run_stack asks for it: the stack's width, heads and head dim, the call's rows and regime; the operands' lo planes lie
    // one plane behind their hi planes (carve_tokens / carve_frames)
    AttnCall attn_call(const Stack& st, const Step& s) const {
        AttnCall c{st.Dp, st.Dp / padded_head_dim(st.dk), st.dk, prec, r.R, r.Rpad, r.regime_rows, nwork >= 0 ? nwork : att_blocks(r.R)};
        c.qkv_rows = s.a.X != nullptr;
        c.qk_lo_dist = 4LL * r.Rpad * st.Dp; c.vt_lo_dist = 2LL * r.Rpad * st.Dp;
        return c;
    }
    // run_stack: the blocks' steps, the planes of the stack's input where its producer left none, after_norm behind a pre-LN stack
    void stack(const char* name, const Stack& st, int D, const StackBufs& b, bool po, bool x0p_ready = true) const {
        if (names && prec != kFp32 && !st.pre_ln && !x0p_ready) printf("%s.in.planes\n", name);
        for (const Layer& ly : st.layers)
            for (const Step& s : block_steps(st, ly, D, r, b, prec, terms, po, o)) {
                emit(name, s);
                if (s.kind != StepKind::Attention || steps) continue;
                const AttnPlan p = plan_attention(attn_call(st, s), o);
                char line[96];
                snprintf(line, sizeof line, "%s.%s %s %d %d %d\n", name, s.name, attn_name(p.kernel), p.dk, p.nsplit, (int)p.split_pass);
                if (names) {      // launch_attention's scopes
                    if (p.kernel != AttnKernel::None && p.split_pass) printf("%s.%s.split\n", name, s.name);
                    if (p.kernel != AttnKernel::None) printf("%s.%s\n", name, s.name);
                } else if (all) *all += line;
                else printf("%s %s", tag, line);
            }
        if (names && st.pre_ln) printf("%s.after_norm\n", name);
    }
    void predictor(const char* name, const Predictor& p, const void* Xp) const {
        for (size_t l = 0; l < p.conv.size(); ++l) emit(name, predictor_step(p, l, M, p.conv[0].C, r, M, M, M, prec, Xp, M));
    }
};

// fs2_encode without the kernels
void encode(const Built& m, Call c, const EncodePlan& p) {
    c.prec = p.prec; c.terms = p.ffn_terms;
    c.mark("enc.embed");
    c.stack("enc", m.enc, m.cfg.adim, kTokBufs, false, p.embed_planes);
    c.predictor("dur", m.dur, p.planes ? M : nullptr);
    c.mark("dur.post");
    if (p.tok_proj) {
        c.gemm_prec = p.tok_prec;
        c.emit(nullptr, tok_proj_step(m.tokw, p.tok_n0, M, m.cfg.adim, c.r, M, M, M, M));
    }
}

// fs2_decode without the kernels
void decode(const Built& m, Call c, const DecodePlan& p, const DecodeAsk& ask) {
    c.prec = p.prec; c.terms = p.ffn_terms;
    const int D = m.cfg.ddim;
    const void* hfr_planes = p.hfr_planes ? M : nullptr;
    c.mark(p.tokproj == 3 ? "lr.index" : "lr.expand");
    if (p.fused_var) {
        if (p.tokproj & 1) c.mark("var.gather0");
        for (const Step& s : fused_predictor_steps(m.var2, m.energy, m.pitch, !(p.tokproj & 1), M, m.cfg.adim, c.r, hfr_planes, M, M, M, M, M, c.o)) c.emit(nullptr, s);
    } else {
        if (p.need_e) c.predictor("energy", m.energy, hfr_planes);
        if (p.need_p) c.predictor("pitch", m.pitch, hfr_planes);
    }
    if (p.control) c.mark("var.control");
    if (!(p.tokproj & 2)) c.mark("var.embed");
    if (p.tokproj & 2) c.mark("dec.in.gather");
    else if (m.cfg.decoder_input_layer) c.emit(nullptr, dec_in_step(m.in(), m.dec, M, m.cfg.adim, hfr_planes, c.r, kFrameBufs, p.prec, p.po));
    else c.mark("dec.in.pe");
    c.stack("dec", m.dec, D, kFrameBufs, p.po, p.planes);
    if (p.po && ask.dec_out) c.mark("dec.out.rows");
    c.emit(nullptr, feat_out_step(m.feat, c.r, kFrameBufs, M, p.prec, p.post_pl));
    const Rows r2{c.r.R * p.rf, c.r.Rpad * p.rf, nullptr, nullptr, 0};
    for (int l = 0; l < (int)m.post.size(); ++l) c.emit(nullptr, postnet_step(m.post, l, m.cfg.odim, r2, PostBufs{M, M, M, M, M}, kFrameBufs, p.post_pl, p.ffn_terms, c.o));
    c.mark("unpack");
}

Rows rows_of(int R, int regime) { return Rows{R, round_up(R, 128), nullptr, nullptr, regime}; }

const struct { const char* name; int prec, terms; } kModes[] = {{"fp32", kFp32, 0}, {"bf16x3", kBf16x3, 0}, {"mix_mx", kBf16x3, kFfnMx}, {"mix_mx4", kBf16x3, kFfnMx4}};

int mode_precision(const char* name) {      // include/fs2.h's value of a tested mode (-1: none of them)
    const struct { const char* name; int precision; } k[] = {{"fp32", FS2_PREC_FP32}, {"bf16x3", FS2_PREC_BF16X3}, {"mix_mx", FS2_PREC_MIX_MX}, {"mix_mx4", FS2_PREC_MIX_MX4}};
    for (const auto& m : k) if (!strcmp(m.name, name)) return m.precision;
    return -1;
}

// A case: the options, the model's variations and what the call gives and asks for (see the head of this file).  Default: a teacher-forced forward that asks
// for before, after, e_out and p_out (tools/forward_digest.py).
struct Case {
    Options o; Model m; DecodeAsk ask; bool tokp = true;
    Case() { ask.es = ask.ps = ask.e_out = ask.p_out = ask.after = ask.before = true; }
    bool model_key(const std::string& key, int v) {      // hp.model's other settings (probe weights)
        const struct { const char* key; int* at; } ints[] = {{"adim", &m.adim}, {"ddim", &m.ddim}, {"aheads", &m.heads}, {"eunits", &m.eunits}, {"dunits", &m.dunits}, {"kffn", &m.kffn},
            {"elayers", &m.elayers}, {"dlayers", &m.dlayers}, {"dur_layers", &m.dur_layers}, {"post_chans", &m.post_chans}, {"var_chans", &m.var_chans}};
        const struct { const char* key; bool* at; } bools[] = {{"linear_ffn", &m.linear_ffn}, {"bn", &m.use_batch_norm}, {"enc_pre_ln", &m.enc_pre_ln}, {"enc_concat", &m.enc_concat},
            {"dec_pre_ln", &m.dec_pre_ln}, {"dec_concat", &m.dec_concat}};
        for (const auto& k : ints) if (key == k.key) { *k.at = v; return true; }
        for (const auto& k : bools) if (key == k.key) { *k.at = v != 0; return true; }
        return false;
    }
    bool parse(const char* text) {
        if (!strcmp(text, "-")) return true;
        std::string t(text);
        for (size_t at = 0; at < t.size();) {
            const size_t end = std::min(t.find(',', at), t.size()), eq = t.find('=', at);
            if (eq == std::string::npos || eq > end) return false;
            const std::string key = t.substr(at, eq - at);
            const int v = atoi(t.substr(eq + 1, end - eq - 1).c_str());
            if (key == "tokproj") o.tokproj = v; else if (key == "tokproj_f32") o.tokproj_f32 = v; else if (key == "fuse_var") o.fuse_var = v; else if (key == "row8") o.row8 = v;
            else if (key == "rf") m.rf = v; else if (key == "post") m.post_layers = v;
            else if (key == "in") { m.input_layer = v; if (!v) m.adim = m.ddim; }      // (no input layer: the decoder runs at the encoder's width)
            else if (key == "es") ask.es = v; else if (key == "ps") ask.ps = v; else if (key == "e_out") ask.e_out = v; else if (key == "p_out") ask.p_out = v;
            else if (key == "dec_out") ask.dec_out = v; else if (key == "after") ask.after = v; else if (key == "before") ask.before = v; else if (key == "packed") ask.after_packed = v;
            else if (key == "ctl") ask.ctl_pitch = v; else if (key == "devlay") ask.devlay = v; else if (key == "tokp") tokp = v;
            else if (!model_key(key, v)) return false;
            at = end + 1;
        }
        return true;
    }
};

// what the encode of a case leaves behind, as far as plan_decode reads it
Encoded left_by(const EncodePlan& p) {
    Encoded e;
    e.valid = true; e.tokP = p.tok_proj ? M : nullptr; e.tokP_conv = p.tok_conv;
    return e;
}

// one forward: fs2_encode on the token rows, fs2_decode on the frame rows (the outputs unpack_rows4 can take are given aligned; a capacity is the rows)
void forward(const Built& m, const Case& k, int precision, Call c, const Rows& tok, const Rows& fr, int nwork_tok = -1, int nwork_fr = -1) {
    const EncodePlan ep = plan_encode(m.cfg, k.o, precision, m.tokw.N, k.tokp && precision != FS2_PREC_FP32);
    c.r = tok; c.nwork = nwork_tok;
    if (!c.all) encode(m, c, ep);
    DecodeAsk ask = k.ask;
    ask.R = fr.R; ask.row_capacity = fr.R; ask.after_vec = ask.before_vec = true;
    const DecodePlan dp = plan_decode(m.cfg, k.o, precision, ask, left_by(ep), m.var2.ok, m.in(), m.dec, fr, kFrameBufs);
    c.r = fr; c.nwork = nwork_fr;
    decode(m, c, dp, ask);
}

int model(int Rtok, int reg_tok, int Rfr, int reg_fr, const char* text) {
    Case k;
    if (!k.parse(text)) return 2;
    const Built m{k.m};
    for (const auto& md : kModes) {
        const Call c{md.prec, md.terms, Rows(), md.name, k.o};
        forward(m, k, mode_precision(md.name), c, rows_of(Rtok, reg_tok), rows_of(Rfr, reg_fr));
        // the plan does not depend on the row capacity (device-driven layout: 15-25 % above the rows in use)
        std::string plans[3];
        const double caps[3] = {1.0, 1.15, 1.25};
        for (int i = 0; i < 3; ++i) {
            Call q = c;
            q.all = &plans[i];
            forward(m, k, mode_precision(md.name), q, Rows(), rows_of((int)(reg_fr * caps[i]), reg_fr));
        }
        printf("%s capacity_independent %d\n", md.name, (int)(plans[0] == plans[1] && plans[0] == plans[2] && !plans[0].empty()));
    }
    return 0;
}

// ---- the rows of a batch: layout_rule.h's walk and dealing, as layout.h's build_layout applies them on the host (per-utterance semantics)
struct BatchRows { int R = 0, Rpad = 0, nwork = 0; };
BatchRows rows_of_batch(const std::vector<int64_t>& len, int gap) {
    int row = gap;
    for (int64_t l : len) row = row_after(row_start(row), (int)l, gap);
    BatchRows out;
    out.R = rows_used(row); out.Rpad = rows_padded(out.R);
    std::vector<int> order(len.size());
    for (size_t i = 0; i < len.size(); ++i) order[i] = (int)i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return dealt_before((int)len[x], x, (int)len[y], y); });
    Dealer deal;
    for (int b : order) deal.place(att_blocks((int)len[b]));
    out.nwork = deal.items();
    return out;
}

// the ordered profile names of one forward of the utterances given as tokens,frames
int names(const char* block, const char* mode, const char* text, int n, char** utts) {
    Case k;
    const int precision = mode_precision(mode);
    if (!k.parse(text) || precision < 0 || n < 1) return 2;
    if (!strcmp(block, "pre_ln_concat")) k.m.enc_pre_ln = k.m.enc_concat = k.m.dec_pre_ln = k.m.dec_concat = true;
    else if (strcmp(block, "default")) return 2;
    const Built m{k.m};
    std::vector<int64_t> tokens, frames;
    int64_t total = 0, longest = 0;
    for (int i = 0; i < n; ++i) {
        long long t = 0, f = 0;
        if (sscanf(utts[i], "%lld,%lld", &t, &f) != 2) return 2;
        tokens.push_back(t); frames.push_back(f); total += f; longest = std::max<int64_t>(longest, f);
    }
    fs2_batch b{};
    b.B = n; b.ilens = tokens.data(); b.precision = precision;
    for (int64_t t : tokens) b.Tmax = std::max(b.Tmax, (int)t);
    int p = std::max(std::max(k.m.kffn, k.m.dur_k), k.m.var_k);      // fs2_create: the zero rows between utterances are the largest conv halo of the model
    if (k.m.post_layers > 0) p = std::max(p, k.m.post_k);
    const int gap = std::min(kGap, std::max(kMinGap, (p - 1) / 2));
    const BatchRows tok = rows_of_batch(tokens, gap);
    BatchRows fr = rows_of_batch(frames, gap);
    if (k.ask.devlay) {      // the capacities of `total` frames, the longest utterance's as the per-utterance one (fs2_row_capacity, capacity_layout)
        fr.R = fr.Rpad = rows_padded(row_bound(total, n));
        fr.nwork = work_capacity(fr.R, n, (int)longest);
    }
    Call c{0, 0, Rows(), "", k.o};
    c.names = true;
    forward(m, k, precision, c, Rows{tok.R, tok.Rpad, nullptr, nullptr, regime_rows_of(b, true)}, Rows{fr.R, fr.Rpad, nullptr, nullptr, regime_rows_of(b, false)}, tok.nwork, fr.nwork);
    return 0;
}

// ---- every field of the two plans over the inputs they are functions of: `coordinates | fields`
int decisions() {
    const char* modes[] = {"fp32", "bf16x3", "mix_mx", "mix_mx4"};
    const Rows fr = rows_of(896, 664);      // one utterance: the planes-only regime is there only when FS2_ROW8 forces it
    for (const char* mode : modes)
        for (int tokproj = 0; tokproj <= 3; ++tokproj)
            for (int fuse = 0; fuse <= 1; ++fuse)
                for (int row8 : {-1, 1})
                    for (int in = 0; in <= 1; ++in)
                        for (int rf = 1; rf <= 2; ++rf)
                            for (int post : {0, 1, 5})
                                for (int tokp = 0; tokp <= 1; ++tokp) {
                                    Case k;
                                    k.o.tokproj = tokproj; k.o.fuse_var = fuse; k.o.row8 = row8; k.m.rf = rf; k.m.post_layers = post; k.m.input_layer = in; k.tokp = tokp;
                                    k.m.adim = k.m.ddim;      // (one width, so that a model without an input layer is the same model otherwise)
                                    const Built m{k.m};
                                    const int precision = mode_precision(mode);
                                    const EncodePlan e = plan_encode(m.cfg, k.o, precision, m.tokw.N, tokp && precision != FS2_PREC_FP32);
                                    printf("enc %s tokproj=%d fuse=%d row8=%d in=%d rf=%d post=%d tokp=%d | prec=%d ffn_terms=%d planes=%d embed_planes=%d tok_proj=%d tok_conv=%d tok_n0=%d tok_prec=%d\n",
                                           mode, tokproj, fuse, row8, in, rf, post, tokp, e.prec, e.ffn_terms, (int)e.planes, (int)e.embed_planes, (int)e.tok_proj, (int)e.tok_conv, e.tok_n0, e.tok_prec);
                                    for (int given = 0; given < 4; ++given)
                                        for (int asked = 0; asked < 4; ++asked)
                                            for (int devlay = 0; devlay <= 1; ++devlay) {
                                                DecodeAsk a;
                                                a.es = given & 1; a.ps = given & 2; a.e_out = asked & 1; a.p_out = asked & 2; a.after = true; a.devlay = devlay;
                                                a.R = a.row_capacity = fr.R; a.after_vec = true;
                                                const DecodePlan d = plan_decode(m.cfg, k.o, precision, a, left_by(e), m.var2.ok, m.in(), m.dec, fr, kFrameBufs);
                                                printf("dec %s tokproj=%d fuse=%d row8=%d in=%d rf=%d post=%d tokp=%d es=%d ps=%d e_out=%d p_out=%d devlay=%d | prec=%d ffn_terms=%d devlay=%d planes=%d "
                                                       "hfr_planes=%d need_e=%d need_p=%d fused_var=%d tokproj=%d control=%d po=%d mask_q=%d rf=%d post_pl=%d ep_stored=%d\n",
                                                       mode, tokproj, fuse, row8, in, rf, post, tokp, (int)a.es, (int)a.ps, (int)a.e_out, (int)a.p_out, devlay, d.prec, d.ffn_terms, (int)d.devlay,
                                                       (int)d.planes, (int)d.hfr_planes, (int)d.need_e, (int)d.need_p, (int)d.fused_var, d.tokproj, (int)d.control, (int)d.po, d.mask_q, d.rf,
                                                       (int)d.post_pl, (int)d.ep_stored);
                                            }
                                }
    // what the batch semantics, the control and the outputs decide: nothing above depends on them, nor they on anything above but the layout
    const Built m{Model()};
    for (int bits = 0; bits < 1 << 11; ++bits) {
        DecodeAsk a;
        a.devlay = bits & 1; a.after = bits & 2; a.before = bits & 4; a.after_packed = bits & 8; a.after_vec = bits & 16; a.before_vec = bits & 32;
        a.compat = (bits >> 6) & 1; a.masked = (bits >> 7) & 1; a.ctl_pitch = bits & 256; a.ctl_energy = bits & 512;
        a.row_capacity = 1024; a.R = (bits & 1024) ? 1024 : 896;
        const DecodePlan d = plan_decode(m.cfg, Options(), FS2_PREC_BF16X3, a, Encoded(), m.var2.ok, m.in(), m.dec, fr, kFrameBufs);
        printf("out devlay=%d after=%d before=%d packed=%d after_vec=%d before_vec=%d compat=%d masked=%d ctl_pitch=%d ctl_energy=%d rows_are_capacity=%d | control=%d mask_q=%d ep_stored=%d "
               "packed_ovf=%d poison_after=%d poison_before=%d poison_packed=%d poison=%d\n", (int)a.devlay, (int)a.after, (int)a.before, (int)a.after_packed, (int)a.after_vec, (int)a.before_vec,
               a.compat, a.masked, (int)a.ctl_pitch, (int)a.ctl_energy, (int)(a.R == a.row_capacity), (int)d.control, d.mask_q, (int)d.ep_stored, (int)d.packed_ovf, (int)d.poison_after,
               (int)d.poison_before, (int)d.poison_packed, (int)d.poison());
    }
    return 0;
}

// ---- the refusals of the two entry points: what|err|message.  `a+b`: both conditions hold and the one the entry point tests first answers.
constexpr int kPe = 512;      // rows of both positional tables in the cases below
int call_refusals() {
    static const int64_t ilens[3] = {5, 17, 33}, olens[3] = {40, 136, 264};
    auto batch = [&] { fs2_batch b{}; b.B = 3; b.Tmax = 33; b.ilens = ilens; b.precision = FS2_PREC_BF16X3; return b; };
    auto show = [](const char* what, const Refusal& r) { printf("%s|%d|%s\n", what, r.err, r.msg); };
    {
        auto io = [&] { fs2_encode_io e{}; e.batch = batch(); e.xs = reinterpret_cast<const int64_t*>(M); e.olens = reinterpret_cast<int64_t*>(M); e.workspace = M; return e; };
        auto enc = [&](const char* what, const fs2_encode_io& e, int pe = kPe) { show(what, check_encode(e, pe)); };
        static const int64_t zero_len[3] = {5, 0, 33}, long_len[3] = {5, 17, 34};
        fs2_encode_io e = io(); enc("enc.accepted", e);
        e = io(); e.batch.B = 0; enc("enc.batch_empty", e);
        e = io(); e.batch.Tmax = 0; enc("enc.batch_tmax", e);
        e = io(); e.batch.ilens = nullptr; e.batch.precision = 99; enc("enc.batch_ilens+precision", e);
        e = io(); e.batch.ilens = zero_len; enc("enc.ilens_zero", e);
        e = io(); e.batch.ilens = long_len; e.batch.precision = 99; enc("enc.ilens_long+precision", e);
        e = io(); e.batch.precision = -1; enc("enc.precision_low", e);
        e = io(); e.batch.precision = 7; e.batch.regime_tokens = 5; enc("enc.precision+regime", e);
        e = io(); e.batch.regime_tokens = 5; e.xs = nullptr; enc("enc.regime_tokens_alone+xs", e);
        e = io(); e.batch.regime_utterances = 2; enc("enc.regime_utterances_alone", e);
        e = io(); e.batch.regime_tokens = -1; e.batch.regime_utterances = -1; enc("enc.regime_negative", e);
        e = io(); e.batch.regime_tokens = 4528; e.batch.regime_utterances = 64; enc("enc.regime_accepted", e);
        e = io(); e.xs = nullptr; e.duration_alpha = -1.f; enc("enc.xs+alpha", e);
        e = io(); e.olens = nullptr; enc("enc.olens", e);
        e = io(); e.workspace = nullptr; enc("enc.workspace", e);
        e = io(); e.duration_alpha = -0.5f; enc("enc.alpha+pe", e, 32);
        e = io(); enc("enc.pe", e, 32);
        e = io(); enc("enc.pe_exact", e, 33);
        e = io(); e.batch.Tmax = 40; e.batch.compat_padded = 1; enc("enc.pe_padded_batch", e, 39);      // every utterance is stored at Tmax rows
    }
    auto left = [&] { Encoded e; e.valid = true; e.B = 3; e.Tmax = 33; e.ws = M; return e; };
    auto io = [&] { fs2_decode_io d{}; d.batch = batch(); d.olens = olens; d.Lmax = 264; d.token_workspace = M; d.workspace = M; d.after = M; return d; };
    auto dev = [&] { fs2_decode_io d = io(); d.olens = nullptr; d.row_capacity = 1024; d.status = reinterpret_cast<int32_t*>(M); return d; };
    auto ctl = [&] { fs2_prosody p{}; p.pitch_scale = M; p.pitch_scale_cols = 1; return p; };
    auto dec = [&](const char* what, const fs2_decode_io& d, const fs2_prosody* p = nullptr, const Encoded* e = nullptr, int pe = kPe) {
        const Encoded dflt = left();
        show(what, check_decode(d, p, e ? *e : dflt, 68, pe));
    };
    static const int64_t bad_id[3] = {40, -1, 0}, empty[3] = {40, 0, 264}, negative[3] = {40, -2, 264};
    const Encoded none;
    fs2_decode_io d = io(); dec("dec.accepted", d);
    d = dev(); dec("dec.devlay_accepted", d);
    fs2_prosody p = ctl(); d = io(); dec("dec.ctl_accepted", d, &p);
    p = ctl(); p.pitch_scale_cols = 33; d = io(); dec("dec.ctl_per_phoneme_accepted", d, &p);
    p = fs2_prosody{}; p.pitch_scale_cols = 7; d = io(); dec("dec.ctl_neutral_cols_ignored", d, &p);
    p = ctl(); p.pitch_scale_cols = 2; d = io(); d.ps = M; dec("dec.ctl_pitch_scale_cols+ps", d, &p);
    p = ctl(); p.pitch_shift = M; p.pitch_shift_cols = 0; p.energy_scale = M; p.energy_scale_cols = 5; d = io(); dec("dec.ctl_pitch_shift_cols+energy_scale_cols", d, &p);
    p = fs2_prosody{}; p.energy_scale = M; p.energy_scale_cols = 34; d = io(); dec("dec.ctl_energy_scale_cols", d, &p);
    p = fs2_prosody{}; p.energy_shift = M; p.energy_shift_cols = 3; d = io(); d.es = M; dec("dec.ctl_energy_shift_cols+es", d, &p);
    p = ctl(); p.energy_shift = M; p.energy_shift_cols = 1; d = io(); d.ps = M; d.es = M; dec("dec.ctl_ps+es", d, &p);
    p = ctl(); d = io(); d.es = M; dec("dec.ctl_pitch_with_es_accepted", d, &p);
    p = fs2_prosody{}; p.energy_shift = M; p.energy_shift_cols = 1; d = io(); d.es = M; d.batch.compat_padded = 1; dec("dec.ctl_es+compat", d, &p);
    p = ctl(); d = io(); d.batch.compat_padded = 1; dec("dec.ctl_compat+no_encode", d, &p, &none);
    d = io(); d.batch.B = 0; dec("dec.no_encode+batch", d, nullptr, &none);
    d = io(); d.batch.B = 0; dec("dec.batch_empty", d);
    d = io(); d.batch.precision = 99; d.batch.Tmax = 34; dec("dec.precision+pairing", d);
    d = io(); d.batch.B = 2; dec("dec.pairing_B", d);
    d = io(); d.batch.Tmax = 34; dec("dec.pairing_Tmax", d);
    { Encoded e = left(); e.compat = 1; d = io(); dec("dec.pairing_compat", d, nullptr, &e); }
    d = io(); d.token_workspace = MB + 4; d.workspace = nullptr; dec("dec.pairing_workspace+workspace", d);
    d = io(); d.olens = nullptr; dec("dec.olens", d);
    d = io(); d.workspace = nullptr; dec("dec.workspace", d);
    d = io(); d.after = nullptr; dec("dec.after", d);
    d = io(); d.after = nullptr; d.after_packed = M; dec("dec.after_packed_accepted", d);
    d = dev(); d.status = nullptr; d.after = nullptr; dec("dec.after+status", d);
    d = dev(); d.status = nullptr; d.Lmax = 0; dec("dec.status+Lmax", d);
    d = dev(); d.Lmax = 0; dec("dec.devlay_Lmax", d);
    d = dev(); d.row_capacity = (long long)INT32_MAX - 255; dec("dec.row_capacity", d);
    d = dev(); d.row_capacity = (long long)INT32_MAX - 256; dec("dec.row_capacity_accepted", d);
    d = io(); d.olens = bad_id; dec("dec.bad_id+empty", d);
    d = io(); d.olens = empty; d.Lmax = 10; dec("dec.empty+Lmax", d);
    d = io(); d.olens = negative; dec("dec.negative", d);
    d = io(); d.Lmax = 263; dec("dec.Lmax+pe", d, nullptr, nullptr, 200);
    d = io(); dec("dec.pe", d, nullptr, nullptr, 263);
    d = io(); dec("dec.pe_exact", d, nullptr, nullptr, 264);
    return 0;
}

// the block variants of tests/test_oracle_golden.py: one layer per stack, every step
int variants(int Rtok, int reg_tok, int Rfr, int reg_fr) {
    const struct { const char* name; bool enc_pre_ln, enc_concat, dec_pre_ln, dec_concat; } kVariants[] = {
        {"pre_ln", true, false, true, false}, {"concat_after", false, true, false, true}, {"pre_ln_concat", true, true, true, true}, {"enc_pre_ln_dec_concat", true, false, false, true}};
    for (const auto& v : kVariants)
        for (const auto& md : kModes) {
            Model mm; mm.elayers = mm.dlayers = 1; mm.enc_pre_ln = v.enc_pre_ln; mm.enc_concat = v.enc_concat; mm.dec_pre_ln = v.dec_pre_ln; mm.dec_concat = v.dec_concat;
            const Built m{mm};
            const std::string tag = std::string(v.name) + " " + md.name;
            Call c{md.prec, md.terms, rows_of(Rtok, reg_tok), tag.c_str(), Options()};
            c.steps = true;
            c.stack("enc", m.enc, mm.adim, kTokBufs, false);
            c.r = rows_of(Rfr, reg_fr);
            c.stack("dec", m.dec, mm.ddim, kFrameBufs, plan_decode(m.cfg, c.o, mode_precision(md.name), DecodeAsk(), Encoded(), m.var2.ok, m.in(), m.dec, c.r, kFrameBufs).po);
        }
    return 0;
}

// ---- fs2_runtime.hip's planes_only_regime as it stood before the plan existed (verbatim but for the arguments: the reference of the sweep)
struct OldConfig { int ddim, dunits, adim; };
struct OldStack { bool pre_ln, concat; };
bool old_planes_only_regime(const OldConfig& c, const OldStack& st, int prec, long regime_rows, const Options& o) {
    if (prec != kBf16x3 || o.row4 == 0 || c.ddim != 384 || st.pre_ln || st.concat || c.dunits % 64 != 0 || c.adim % 64 != 0) return false;
    if (o.row8 >= 0) return o.row8 != 0;
    return (regime_rows + 127) / 128 >= 128;
}

int sweep() {
    const int regimes[] = {1, 800, 16256, 16257, 36600, 78000};
    for (int regime : regimes)
        for (int row8 = -1; row8 <= 1; ++row8)
            for (int row4 = -1; row4 <= 0; ++row4)
                for (int prec : {kBf16, kBf16x3})
                    for (int ddim : {256, 384})
                        for (int terms : {0, kFfnMx, kFfnMx4}) {
                            Model mm; mm.ddim = ddim;
                            const Built m{mm};
                            Options o; o.row8 = row8; o.row4 = row4;
                            const bool was = old_planes_only_regime({mm.ddim, mm.dunits, mm.adim}, {false, false}, prec, regime, o);
                            const bool now = planes_only(m.in(), m.dec, ddim, rows_of(regime, regime), kFrameBufs, prec, terms, o);
                            const bool at_cap = planes_only(m.in(), m.dec, ddim, rows_of((int)(regime * 1.25) + 1, regime), kFrameBufs, prec, terms, o);
                            printf("%d %d %d %s %d %d %d %d %d\n", regime, row8, row4, prec == kBf16 ? "bf16" : "bf16x3", ddim, (int)was, (int)now, (int)at_cap, terms);
                        }
    return 0;
}

int refusals() {
    const Options o;
    auto show = [&](const char* what, const GemmArgs& a, int prec, const Options& opt) {
        const GemmPlan p = plan_gemm(a, prec, opt);
        char msg[512] = "";
        if (p.err) snprintf(msg, sizeof msg, p.msg, "x", p.m0, p.m1);
        printf("%s|%d|%s\n", what, p.err, msg);
    };
    auto conv = [&] { GemmArgs a = base(256, 9, 1024, 1000, false); a.Xp = M; a.Yp = M; a.yp_chunks = 32; return a; };      // a plain FFN convolution, planes in and out
    auto big_ln = [&] { GemmArgs a = base(384, 1, 384, 40000, false); a.Xp = M; a.Yp = M; a.yp_chunks = 12; a.ln_g = M; a.regime_rows = 36600; return a; };
    GemmArgs a = conv(); a.ktaps = 18; show("kernel_size", a, kBf16x3, o);
    a = conv(); a.C = 258; show("channels", a, kBf16x3, o);
    a = conv(); a.Wb = nullptr; show("weight_image", a, kBf16x3, o);
    a = conv(); a.C = a.ldx = 260; show("bf16_shape", a, kBf16x3, o);
    a = conv(); a.Xp = nullptr; show("no_planes", a, kBf16x3, o);
    a = conv(); a.ldy = 1022; show("row_stride", a, kBf16x3, o);
    a = big_ln(); a.residp = M; a.residp_chunks = 12; show("planes_only_off_row4", a, kBf16, o);
    a = conv(); a.yp_col_off = 256; show("col_off", a, kBf16x3, o);
    a = conv(); a.yp_chunks = 64; show("plane_slice", a, kBf16x3, o);      // (the slice at offset 0 of a wider plane row)
    a = conv(); a.Yp = nullptr; show("no_output", a, kBf16x3, o);
    a = base(256, 1, 600, 1000, false); a.Xp = M; a.qk_hi = M; a.att_D = 200; a.Rvt = 1024; show("qkv_split", a, kBf16x3, o);
    a = base(256, 1, 1024, 1000, false); a.Xp = M; a.Yp = M; a.yp_chunks = 32; a.f16_terms = 2; show("f16_non_conv", a, kBf16x3, o);
    a = base(256, 3, 192, 1000, false); a.Xp = M; a.Yp = M; a.yp_chunks = 6; a.mx = 1; show("mx_shape", a, kBf16x3, o);
    a = conv(); a.mx = 2; show("mx4_row_scales", a, kBf16x3, o);
    a = conv(); a.mx = 2; a.x_rowscale = a.w_rowscale = reinterpret_cast<unsigned char*>(M); show("mx4_width", a, kBf16x3, o);
    a = big_ln(); a.residp = M; a.residp_chunks = 12; a.mx = 1; a.C = a.ldx = a.Cpad = 1024; show("row4_mx_residual", a, kBf16x3, o);
    a = base(256, 1, 100, 1000, true); a.ln_g = M; show("f32_rows_width", a, kFp32, o);
    a = conv(); show("accepted", a, kBf16x3, o);
    return 0;
}

// ---- the attention plan (csrc/attn_plan.h) away from the model's shapes
void show_attn(const char* what, const AttnCall& c, const Options& o) {
    const AttnPlan p = plan_attention(c, o);
    char msg[256] = "";
    if (p.err) snprintf(msg, sizeof msg, p.msg, p.m0);
    unsigned scale_bits;
    memcpy(&scale_bits, &p.softmax_scale, 4);
    printf("%s|%s|%d|%d|%u|%u|%d|%08x|%d|%s\n", what, attn_name(p.kernel), p.dk, p.nsplit, p.grid_x, p.grid_y, (int)p.split_pass, scale_bits, p.err, msg);
}
AttnCall attn_base(int prec, int dk, int heads = 2) {
    AttnCall c{heads * dk, heads, 0, prec, 1024, 1024, 0, 8};
    c.qk_lo_dist = c.vt_lo_dist = 1 << 20;
    return c;
}

// what|kernel|dk|nsplit|grid_x|grid_y|split_pass|softmax_scale bits|err|message, `what` = the case's coordinates
int attn_sweep() {
    char what[128];
    const struct { const char* name; int prec; } precs[] = {{"fp32", kFp32}, {"bf16x3", kBf16x3}, {"bf16", kBf16}};
    // the threshold: regime rows x switch x precision x head dim, the regime given (R = 1 row) or left to R
    for (int rows : {1, 8064, 8065, 8191, 8192, 8193, 37256})
        for (int w32 = -1; w32 <= 1; ++w32)
            for (const auto& pr : precs)
                for (int dk : {64, 128, 192, 256})
                    for (int by_R = 0; by_R <= 1; ++by_R) {
                        AttnCall c = attn_base(pr.prec, dk);
                        c.R = by_R ? rows : 1; c.regime_rows = by_R ? 0 : rows;
                        Options o; o.w32 = w32;
                        snprintf(what, sizeof what, "regime %d %d %s %d %d", rows, w32, pr.name, dk, by_R);
                        show_attn(what, c, o);
                    }
    // the lo planes' distance: where everything else chooses attn_w32
    for (long long d : {0LL, -256LL, (1LL << 31) - 1, 1LL << 31})
        for (int which = 0; which <= 1; ++which) {
            AttnCall c = attn_base(kBf16x3, 128);
            (which ? c.vt_lo_dist : c.qk_lo_dist) = d;
            Options o; o.w32 = 1;
            snprintf(what, sizeof what, "dist %lld %d", d, which);
            show_attn(what, c, o);
        }
    // the grid
    for (int n = 0; n <= 33; ++n)
        for (int k = 0; k < 3; ++k) {
            AttnCall c = attn_base(k == 0 ? kFp32 : kBf16x3, 128);
            c.nwork = n; c.qkv_rows = k != 2;      // (a split pass too has nothing to do without work)
            Options o; o.w32 = k == 2;
            snprintf(what, sizeof what, "grid %d %s", n, k == 0 ? "f32" : (k == 1 ? "b16" : "w32"));
            show_attn(what, c, o);
        }
    // the scales: the model's head dim under a padded one
    for (int dk_true : {64, 96, 128, 192})
        for (const auto& pr : precs) {
            AttnCall c = attn_base(pr.prec, padded_head_dim(dk_true));
            c.dk_true = dk_true; c.qkv_rows = true;
            snprintf(what, sizeof what, "scale %d %s", dk_true, pr.name);
            show_attn(what, c, Options());
        }
    return 0;
}

int attn_refusals() {
    const Options o;
    AttnCall c = attn_base(kFp32, 96); c.qkv_rows = true; show_attn("head_dim_fp32", c, o);
    c = attn_base(kBf16x3, 96); show_attn("head_dim_bf16x3", c, o);
    c = attn_base(kBf16x3, 96); c.nwork = 0; show_attn("head_dim_no_work", c, o);
    c = attn_base(kBf16x3, 264, 4); c.qkv_rows = true; show_attn("wide_split", c, o);                 // D = 1056: the refusal comes before the head dim's
    c = attn_base(kBf16x3, 264, 4); show_attn("wide_operands_given", c, o);                           // ... and only the head dim's is left without a split pass
    c = attn_base(kBf16x3, 192, 6); show_attn("wide_accepted", c, o);                                 // D = 1152, operands given
    c = attn_base(kFp32, 192, 6); c.qkv_rows = true; show_attn("wide_fp32", c, o);
    return 0;
}

// ---- the weight plan (csrc/weight_plan.h)
void show_plan(const WeightPlan& p) {
    printf("N=%d Npad=%d Cpad=%d nchunks=%d w=%zu wb=%zu wf=%zu wm=%zu wm4=%zu ws4=%zu bias=%zu mx_src=%s shape=%d:%lld,%lld,%lld vec=%lld\n", p.N, p.Npad, p.Cpad, p.nchunks,
           p.bytes[kImgW], p.bytes[kImgWb], p.bytes[kImgWf], p.bytes[kImgWm], p.bytes[kImgWm4], p.bytes[kImgWs4], p.bytes[kImgBias],
           p.mx_src == MxSource::None ? "none" : (p.mx_src == MxSource::Tensor ? "tensor" : "folded"), p.w_ndim, (long long)p.w_shape[0], (long long)p.w_shape[1],
           (long long)p.w_shape[2], (long long)p.vec_len);
}

// every layer of a model in the loader's order: `name parts Neach C ktaps | plan`, then the bytes of all images together
int weights(const char* text) {
    Case k;
    if (!k.parse(text)) return 2;
    size_t total = 0;
    for (const NamedAsk& l : model_asks(k.m)) {
        printf("%s parts=%d Neach=%d C=%d k=%d | ", l.name.c_str(), l.ask.parts, l.ask.Neach, l.ask.C, l.ask.ktaps);
        const WeightPlan p = plan_weight(l.ask);
        show_plan(p);
        total += p.total_bytes();
    }
    printf("total %zu\n", total);
    return 0;
}

int weight_sweep() {
    const struct { bool f16, mx_conv, mx4, mx_k1; } roles[] = {{false, false, false, false}, {true, false, false, false}, {false, true, false, false}, {false, false, true, false},
                                                             {false, false, false, true}, {false, true, true, false}, {true, true, true, false}, {true, true, true, true}};
    for (int parts : {1, 3})
        for (int N : {31, 32, 33, 127, 128, 129, 256})
            for (int C : {31, 32, 33, 127, 128, 129, 256, 384})
                for (int ktaps : {1, 3, 9})
                    for (int linear = 0; linear <= 1; ++linear)
                        for (int bn = 0; bn <= 1; ++bn)
                            for (int slice = 0; slice <= 1; ++slice)
                                for (int bias = 0; bias <= 1; ++bias)
                                    for (const auto& r : roles) {
                                        WeightAsk a = ask_of(parts, N, C, ktaps, linear, bias);
                                        a.bn = bn; a.f16 = r.f16; a.mx_conv = r.mx_conv; a.mx4 = r.mx4; a.mx_k1 = r.mx_k1;
                                        if (slice) { a.col_off = C; a.src_cols = 2 * C; }
                                        printf("parts=%d Neach=%d C=%d k=%d linear=%d bn=%d col_off=%d src_cols=%d bias=%d f16=%d mx_conv=%d mx4=%d mx_k1=%d | ", parts, N, C, ktaps, linear, bn,
                                               a.col_off, a.src_cols, bias, (int)r.f16, (int)r.mx_conv, (int)r.mx4, (int)r.mx_k1);
                                        show_plan(plan_weight(a));
                                    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "model")) return model(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6]);
    if (argc >= 6 && !strcmp(argv[1], "names")) return names(argv[2], argv[3], argv[4], argc - 5, argv + 5);
    if (argc == 2 && !strcmp(argv[1], "decisions")) return decisions();
    if (argc == 2 && !strcmp(argv[1], "call_refusals")) return call_refusals();
    if (argc == 6 && !strcmp(argv[1], "variants")) return variants(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !strcmp(argv[1], "refusals")) return refusals();
    if (argc == 2 && !strcmp(argv[1], "attn_sweep")) return attn_sweep();
    if (argc == 2 && !strcmp(argv[1], "attn_refusals")) return attn_refusals();
    if (argc == 3 && !strcmp(argv[1], "weights")) return weights(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "weight_sweep")) return weight_sweep();
    fprintf(stderr, "usage: probe model Rtok regime_tok Rfr regime_fr case | variants Rtok regime_tok Rfr regime_fr | names block mode case tokens,frames.. | decisions | call_refusals | "
                    "sweep | refusals | attn_sweep | attn_refusals | weights case | weight_sweep\n");
    return 2;
}
