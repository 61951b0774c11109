// Host-compiled driver of csrc/gemm_plan.h, csrc/attn_plan.h and csrc/model_launches.h for tests/test_gemm_plan_host.py and tests/test_attn_plan_host.py
// (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe model <Rtok> <regime_tok> <Rfr> <regime_fr>      the plan of every named launch of the default model, attention included, in the four tested precisions
//   probe variants <Rtok> <regime_tok> <Rfr> <regime_fr>   every step of the pre-LN / concat_after block variants, and whether its GEMMs plan
//   probe sweep                                            the planes-only decision: the predicate fs2_decode used to restate against the plan's answer
//   probe refusals                                         one argument set per refusal of plan_gemm
//   probe attn_sweep                                       plan_attention over the regime threshold, the switch, the plane distances, the grid and the scales
//   probe attn_refusals                                    the refusals of plan_attention
// The launches are the ones model_launches.h forms, the header fs2_runtime.hip executes.  This file holds only data: a model described as the loader would leave it
// (a marker pointer wherever it builds an image or the workspace has a buffer) and the walk over the header's step lists.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "attn_plan.h"
#include "model_launches.h"

using namespace fs2;

namespace {

float kMarkStorage[2];
float* const M = kMarkStorage;      // a non-null pointer nobody follows
unsigned char* const MB = reinterpret_cast<unsigned char*>(kMarkStorage);
constexpr int kFp32 = kPlanFp32, kBf16x3 = kPlanBf16x3, kBf16 = 2;

int round_up(int x, int a) { return (x + a - 1) / a * a; }

// a layer as the Loader leaves it: the split-bf16 image always, the others by its rules (mx: the layer is one the mx image is built for when the shape allows)
Gemm gemm(int C, int ktaps, int N, bool mx = false, bool f16 = false) {
    Gemm g;
    g.w = M; g.wb = M; g.C = C; g.Cpad = round_up(C, 32); g.ktaps = ktaps; g.N = N;
    if (f16) g.wf = M;
    if (mx && C % 128 == 0 && N % 128 == 0) { g.wm = M; if (ktaps > 1 && f16) { g.wm4 = M; g.ws4 = MB; } }
    return g;
}
GemmArgs base(int C, int ktaps, int N, int R, bool y) { return gemm_args(gemm(C, ktaps, N), M, C, R, nullptr, y ? M : nullptr, N); }      // (the refusal cases start from it)

struct Model { int adim = 256, ddim = 384, heads = 2, eunits = 1024, dunits = 1024, kffn = 9, odim = 80, post_layers = 5, post_chans = 256, post_k = 5,
               dur_chans = 256, dur_k = 3, var_chans = 256, var_k = 3, layers = 4;
               bool enc_pre_ln = false, enc_concat = false, dec_pre_ln = false, dec_concat = false; };

Stack stack(int D, int heads, int units, int k, int layers, bool pre_ln, bool concat) {
    Stack st;
    st.dk = D / heads; st.Dp = att_width(D, heads); st.pre_ln = pre_ln; st.concat = concat; st.pe = M; st.after_g = st.after_b = M;
    Layer ly;
    ly.qkv = gemm(D, 1, 3 * st.Dp); ly.out = gemm(st.Dp, 1, D); ly.w1 = gemm(D, k, units, k > 1, k > 1); ly.w2 = gemm(units, 1, D, k > 1 && D == 384);
    if (concat) ly.cat_x = ly.cat_a = gemm(D, 1, D);
    ly.ln1g = ly.ln1b = ly.ln2g = ly.ln2b = M;
    st.layers.assign(layers, ly);
    return st;
}
Predictor predictor(int cin, int chans, int k) {
    Predictor p;
    p.conv = {gemm(cin, k, chans), gemm(chans, k, chans)};
    p.lng = p.lnb = {M, M}; p.lin_w = p.lin_b = M;
    return p;
}
struct Built {
    Stack enc, dec; Predictor dur, energy, pitch; FusedPredictors var2; Gemm dec_in, feat; std::vector<Gemm> post;
    explicit Built(const Model& m)
        : enc(stack(m.adim, m.heads, m.eunits, m.kffn, m.layers, m.enc_pre_ln, m.enc_concat)), dec(stack(m.ddim, m.heads, m.dunits, m.kffn, m.layers, m.dec_pre_ln, m.dec_concat)),
          dur(predictor(m.adim, m.dur_chans, m.dur_k)), energy(predictor(m.adim, m.var_chans, m.var_k)), pitch(energy), dec_in(gemm(m.adim, 1, m.ddim)), feat(gemm(m.ddim, 1, m.odim)) {
        var2.ok = m.var_chans % 128 == 0;
        var2.c0 = gemm(m.adim, m.var_k, 2 * m.var_chans); var2.c1 = gemm(m.var_chans, m.var_k, 2 * m.var_chans);
        var2.ln0g = var2.ln0b = var2.ln1g = var2.ln1b = var2.lin_w = var2.lin_b = M;
        for (int l = 0; l < m.post_layers; ++l) post.push_back(gemm(l ? m.post_chans : m.odim, m.post_k, l == m.post_layers - 1 ? m.odim : m.post_chans, true));
    }
    DecIn in() const { return DecIn{&dec_in, M, M, 1.f}; }
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
    bool steps = false;      // print every step with its kind and the plan's refusal code instead
    void emit(const char* stack, const Step& st) const {
        const std::string name = std::string(stack ? stack : "") + (stack ? "." : "") + st.name;
        if (steps && st.kind != StepKind::Gemm) printf("%s %s %s 0\n", tag, name.c_str(), st.kind == StepKind::Attention ? "attention" : "layernorm");
        if (st.kind != StepKind::Gemm) return;
        GemmArgs a = st.a;
        call_defaults(a, M, (size_t)4 * std::min(r.Rpad, kSplitRows) * 1024, r.regime_rows);      // the call's split-K scratch (carve_tokens / carve_frames: 4 slabs) and regime
        const GemmPlan p = plan_gemm(a, prec, o);
        char line[256];
        if (all) {
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
        AttnCall c{st.Dp, st.Dp / padded_head_dim(st.dk), st.dk, prec, r.R, r.Rpad, r.regime_rows, att_blocks(r.R)};
        c.qkv_rows = s.a.X != nullptr;
        c.qk_lo_dist = 4LL * r.Rpad * st.Dp; c.vt_lo_dist = 2LL * r.Rpad * st.Dp;
        return c;
    }
    void stack(const char* name, const Stack& st, int D, const StackBufs& b, bool po) const {
        for (const Layer& ly : st.layers)
            for (const Step& s : block_steps(st, ly, D, r, b, prec, terms, po, o)) {
                emit(name, s);
                if (s.kind != StepKind::Attention || steps) continue;
                const AttnPlan p = plan_attention(attn_call(st, s), o);
                char line[96];
                snprintf(line, sizeof line, "%s.%s %s %d %d %d\n", name, s.name, attn_name(p.kernel), p.dk, p.nsplit, (int)p.split_pass);
                if (all) *all += line; else printf("%s %s", tag, line);
            }
    }
    void predictor(const char* name, const Predictor& p, const void* Xp) const {
        for (size_t l = 0; l < p.conv.size(); ++l) emit(name, predictor_step(p, l, M, p.conv[0].C, r, M, M, M, prec, Xp, M));
    }
};

void encode(const Built& m, const Call& c) {
    c.stack("enc", m.enc, m.enc.layers[0].out.N, kTokBufs, false);
    c.predictor("dur", m.dur, c.prec != kFp32 ? M : nullptr);
}

void decode(const Built& m, const Call& c) {
    const bool pl = c.prec != kFp32;
    const int D = m.dec_in.N;
    if (pl && m.var2.ok && c.o.fuse_var) { for (const Step& s : fused_predictor_steps(m.var2, m.energy, m.pitch, true, M, m.dec_in.C, c.r, M, M, M, M, M, M, c.o)) c.emit(nullptr, s); }
    else { c.predictor("energy", m.energy, pl ? M : nullptr); c.predictor("pitch", m.pitch, pl ? M : nullptr); }
    const bool po = pl && planes_only(m.in(), m.dec, D, c.r, kFrameBufs, c.prec, c.terms, c.o);
    c.emit(nullptr, dec_in_step(m.in(), m.dec, M, m.dec_in.C, pl ? M : nullptr, c.r, kFrameBufs, c.prec, po));
    c.stack("dec", m.dec, D, kFrameBufs, po);
    const bool post_pl = pl && m.post.size() > 1;
    c.emit(nullptr, feat_out_step(m.feat, c.r, kFrameBufs, M, c.prec, post_pl));
    Rows r2 = c.r; r2.regime_rows = 0;
    for (int l = 0; l < (int)m.post.size(); ++l) c.emit(nullptr, postnet_step(m.post, l, m.feat.N, r2, PostBufs{M, M, M, M, M}, kFrameBufs, post_pl, c.terms, c.o));
}

Rows rows_of(int R, int regime) { return Rows{R, round_up(R, 128), nullptr, nullptr, regime}; }

const struct { const char* name; int prec, terms; } kModes[] = {{"fp32", kFp32, 0}, {"bf16x3", kBf16x3, 0}, {"mix_mx", kBf16x3, kFfnMx}, {"mix_mx4", kBf16x3, kFfnMx4}};

int model(int Rtok, int reg_tok, int Rfr, int reg_fr) {
    const Built m{Model()};
    for (const auto& md : kModes) {
        Call c{md.prec, md.terms, rows_of(Rtok, reg_tok), md.name, Options()};
        encode(m, c);
        c.r = rows_of(Rfr, reg_fr);
        decode(m, c);
        // the plan does not depend on the row capacity (device-driven layout: 15-25 % above the rows in use)
        std::string plans[3];
        const double caps[3] = {1.0, 1.15, 1.25};
        for (int i = 0; i < 3; ++i) {
            Call k = c;
            k.r = rows_of((int)(reg_fr * caps[i]), reg_fr); k.all = &plans[i];
            decode(m, k);
        }
        printf("%s capacity_independent %d\n", md.name, (int)(plans[0] == plans[1] && plans[0] == plans[2] && !plans[0].empty()));
    }
    return 0;
}

// the block variants of tests/test_oracle_golden.py: one layer per stack, every step
int variants(int Rtok, int reg_tok, int Rfr, int reg_fr) {
    const struct { const char* name; bool enc_pre_ln, enc_concat, dec_pre_ln, dec_concat; } kVariants[] = {
        {"pre_ln", true, false, true, false}, {"concat_after", false, true, false, true}, {"pre_ln_concat", true, true, true, true}, {"enc_pre_ln_dec_concat", true, false, false, true}};
    for (const auto& v : kVariants)
        for (const auto& md : kModes) {
            Model mm; mm.layers = 1; mm.enc_pre_ln = v.enc_pre_ln; mm.enc_concat = v.enc_concat; mm.dec_pre_ln = v.dec_pre_ln; mm.dec_concat = v.dec_concat;
            const Built m{mm};
            const std::string tag = std::string(v.name) + " " + md.name;
            Call c{md.prec, md.terms, rows_of(Rtok, reg_tok), tag.c_str(), Options()};
            c.steps = true;
            c.stack("enc", m.enc, mm.adim, kTokBufs, false);
            c.r = rows_of(Rfr, reg_fr);
            c.stack("dec", m.dec, mm.ddim, kFrameBufs, c.prec != kFp32 && planes_only(m.in(), m.dec, mm.ddim, c.r, kFrameBufs, c.prec, c.terms, c.o));
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

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "model")) return model(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 6 && !strcmp(argv[1], "variants")) return variants(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !strcmp(argv[1], "refusals")) return refusals();
    if (argc == 2 && !strcmp(argv[1], "attn_sweep")) return attn_sweep();
    if (argc == 2 && !strcmp(argv[1], "attn_refusals")) return attn_refusals();
    fprintf(stderr, "usage: probe model|variants Rtok regime_tok Rfr regime_fr | sweep | refusals | attn_sweep | attn_refusals\n");
    return 2;
}
