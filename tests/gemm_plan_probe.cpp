// Host-compiled driver of csrc/gemm_plan.h for tests/test_gemm_plan_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe model <Rtok> <regime_tok> <Rfr> <regime_fr>   the plan of every named launch of the default model, in the four tested precisions
//   probe sweep                                         the planes-only decision: the predicate fs2_decode used to restate against the plan's answer
//   probe refusals                                      one argument set per refusal of plan_gemm
// The launches are formed the way fs2_runtime.hip forms them (run_stack, run_predictor, run_predictors_fused, fs2_decode), shapes and the null-ness of
// pointers only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "gemm_plan.h"

using namespace fs2;

namespace {

const float kMarkStorage = 0.f;
float* const M = const_cast<float*>(&kMarkStorage);      // a non-null pointer nobody follows
constexpr int kFp32 = 0, kBf16x3 = 1, kBf16 = 2;         // FS2_PREC_*
constexpr int kFfnMx = 9, kFfnMx4 = 10;                  // fs2_runtime.hip: ffn_f16_terms

struct Model { int adim = 256, ddim = 384, heads = 2, eunits = 1024, dunits = 1024, kffn = 9, odim = 80, post_layers = 5, post_chans = 256, post_k = 5,
               dur_chans = 256, dur_k = 3, var_chans = 256, var_k = 3; };

int round_up(int x, int a) { return (x + a - 1) / a * a; }

GemmArgs base(int C, int ktaps, int N, int R, bool y) {      // fs2_runtime.hip: gemm_args
    GemmArgs a = GemmArgs();
    a.X = M; a.ldx = C; a.C = C; a.W = M; a.Cpad = round_up(C, 32); a.ktaps = ktaps; a.N = N; a.R = R;
    a.Y = y ? M : nullptr; a.ldy = N; a.x_scale = 1.f; a.Wb = M;
    return a;
}

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

// what launch_gemm does before it asks: the handle's split-K scratch (carve_tokens / carve_frames: 4 slabs) and regime
GemmPlan plan_in_call(GemmArgs a, int prec, int Rpad, int cur_regime, const Options& o) {
    if (!a.kpart) { a.kpart = M; a.kpart_cap = (size_t)4 * std::min(Rpad, kSplitRows) * 1024; a.ksplit = 3; }
    if (!a.regime_rows) a.regime_rows = cur_regime;
    return plan_gemm(a, prec, o);
}

struct Call {      // one fs2_encode / fs2_decode: prints a line per launch, or collects the plans into `all` (capacity test)
    int prec, terms, R, Rpad, regime;
    const char* tag;
    Options o;
    std::string* all = nullptr;
    void emit(const char* name, const GemmArgs& a) const {
        const GemmPlan p = plan_in_call(a, prec, Rpad, regime, o);
        char line[256];
        if (all) {
            snprintf(line, sizeof line, "%s %s ns%d nb%d bm%d mt%d k1%d ap%d epi%d ar%d res%d ks%d y%d bp%d rp%d err%d\n", name, kernel_name(p.kernel), p.nsplit, p.nb, p.bm, p.mt,
                     (int)p.k1, p.apart, p.epi, p.arith, p.res, p.ksplit, (int)p.y, (int)p.build_planes, (int)p.rows_pass, p.err);
            *all += line;
        } else {
            printf("%s %s %s %d %d %d\n", tag, name, kernel_name(p.kernel), p.tile_rows(), p.ksplit, (int)p.rows_pass);
        }
    }
};

bool ffn2_on_row4_mx(GemmArgs a, const Options& o) { a.mx = 1; const GemmPlan p = plan_gemm(a, kBf16x3, o); return p.kernel == GemmKernel::Row4 && p.arith == 2; }

void run_stack(const Call& c, const char* tag, int D, int heads, int units, int kffn, bool po) {
    const bool pl = c.prec != kFp32;
    const int dk = D / heads, Dp = heads * (dk <= 64 ? 64 : (dk <= 128 ? 128 : (dk <= 192 ? 192 : 256)));
    std::string n = tag;
    GemmArgs a = base(D, 1, 3 * Dp, c.R, true);
    a.regime_rows = c.regime;
    if (pl) a.Xp = M;
    if (pl && Dp % 128 == 0) { a.Y = nullptr; a.qk_hi = M; a.att_D = Dp; a.Rvt = c.Rpad; }
    c.emit((n + ".qkv").c_str(), a);
    a = base(Dp, 1, D, c.R, !po);
    a.regime_rows = c.regime; a.ln_g = M;
    if (po) { a.residp = M; a.residp_chunks = D / 32; } else { a.resid = M; a.ldr = D; }
    const bool mx4l = po && c.terms == kFfnMx4 && D == 384;
    const bool mxl = pl && (c.terms == kFfnMx || c.terms == kFfnMx4);
    if (pl) { a.Xp = M; a.Yp = M; a.yp_chunks = D / 32; a.yp_f16 = mx4l ? 3 : (mxl ? 2 : 0); }
    if (mx4l) a.yp_rowscale = reinterpret_cast<unsigned char*>(M);
    c.emit((n + ".out_ln").c_str(), a);
    GemmArgs a2 = base(units, 1, D, c.R, !po);
    a2.regime_rows = c.regime; a2.ln_g = M;
    if (po) { a2.residp = M; a2.residp_chunks = D / 32; a2.residp_mx = mx4l ? 2 : (mxl ? 1 : 0); } else { a2.resid = M; a2.ldr = D; }
    if (pl) { a2.Xp = M; a2.Yp = M; a2.yp_chunks = D / 32; }
    const bool mx2 = mxl && c.o.ffn2_mx && c.prec == kBf16x3 && ffn2_on_row4_mx(a2, c.o);
    if (mx2) a2.mx = 1;
    a = base(D, kffn, units, c.R, !pl);
    a.act_post = 1;
    if (pl) { a.Xp = M; a.Yp = M; a.yp_chunks = units / 32; }
    if (mx2) a.yp_f16 = 2;
    if (mx4l) { a.mx = 2; a.x_rowscale = a.w_rowscale = reinterpret_cast<unsigned char*>(M); }
    else if (mxl) a.mx = 1;
    c.emit((n + ".ffn1").c_str(), a);
    c.emit((n + ".ffn2_ln").c_str(), a2);
}

void run_predictor(const Call& c, const char* tag, int cin, int chans, int k, bool planes_in) {
    for (int l = 0; l < 2; ++l) {
        const bool last = l == 1;
        GemmArgs a = base(l ? chans : cin, k, chans, c.R, !(last || c.prec != kFp32));
        a.relu_pre = 1; a.ln_g = M; a.scratch = M; a.xp_scratch = M;
        if (last) a.dot_w = M;
        a.Xp = (l || planes_in) ? M : nullptr;
        if (!last) { a.Yp = M; a.yp_chunks = chans / 32; }
        c.emit((std::string(tag) + ".conv" + (l ? "1" : "0")).c_str(), a);
    }
}

void run_predictors_fused(const Call& c, int cin, int chans, int k) {
    if (row_regime(c.regime, c.o.row8) && (chans == 256 || chans == 384)) {
        for (int g = 0; g < 2; ++g) {
            GemmArgs a = base(cin, k, chans, c.R, false);
            a.relu_pre = 1; a.ln_g = M; a.Xp = M; a.xp_scratch = M; a.Yp = M; a.yp_chunks = 2 * chans / 32; a.yp_col_off = g * chans; a.scratch = M;
            c.emit(g ? "pitch.conv0" : "energy.conv0", a);
        }
    } else {
        GemmArgs a = base(cin, k, 2 * chans, c.R, false);
        a.relu_pre = 1; a.ln_g = M; a.ln_groups = 2; a.Xp = M; a.xp_scratch = M; a.Yp = M; a.yp_chunks = 2 * chans / 32; a.scratch = M;
        c.emit("var.conv0", a);
    }
    GemmArgs a = base(chans, k, 2 * chans, c.R, false);
    a.ldx = 2 * chans; a.X = nullptr;
    a.relu_pre = 1; a.ln_g = M; a.ln_groups = 2; a.k_groups = 2; a.Xp = M; a.xp_row_chunks = 2 * chans / 32; a.scratch = M; a.dot_w = M;
    c.emit("var.conv1", a);
}

// the decision of fs2_decode: gemm_plan.h's planes_only_plan on the model's shapes, as fs2_runtime.hip's planes_only_regime calls it, + the ffn_terms condition
// of the call site
bool planes_only(const Model& m, int prec, int terms, int R, int regime, const Options& o) {
    const int dk = m.ddim / m.heads, Dp = m.heads * (dk <= 64 ? 64 : (dk <= 128 ? 128 : (dk <= 192 ? 192 : 256)));
    return prec != kFp32 && (terms == 0 || terms == kFfnMx || terms == kFfnMx4) &&
           planes_only_plan({m.adim, round_up(m.adim, 32)}, {Dp, round_up(Dp, 32)}, {m.dunits, round_up(m.dunits, 32)}, m.ddim, R, regime, prec, o);
}

void encode(const Model& m, const Call& c) {
    run_stack(c, "enc", m.adim, m.heads, m.eunits, m.kffn, false);
    run_predictor(c, "dur", m.adim, m.dur_chans, m.dur_k, c.prec != kFp32);
}

void decode(const Model& m, const Call& c) {
    const bool pl = c.prec != kFp32;
    if (pl && m.var_chans % 128 == 0 && c.o.fuse_var) run_predictors_fused(c, m.adim, m.var_chans, m.var_k);
    else { run_predictor(c, "energy", m.adim, m.var_chans, m.var_k, pl); run_predictor(c, "pitch", m.adim, m.var_chans, m.var_k, pl); }
    const bool po = planes_only(m, c.prec, c.terms, c.R, c.regime, c.o);
    GemmArgs a = base(m.adim, 1, m.ddim, c.R, !po);
    a.regime_rows = c.regime; a.ln_g = M; a.act_post = 1; a.pe = M; a.Xp = pl ? M : nullptr; a.xp_scratch = M;
    if (pl) { a.Yp = M; a.yp_chunks = m.ddim / 32; }
    c.emit("dec.in", a);
    run_stack(c, "dec", m.ddim, m.heads, m.dunits, m.kffn, po);
    a = base(m.ddim, 1, m.odim, c.R, true);
    if (pl) { a.Xp = M; a.Yp = M; a.yp_chunks = round_up(m.odim, 32) / 32; }
    c.emit("feat_out", a);
    auto has_mx = [&](int l) { const int C = l ? m.post_chans : m.odim, N = l == m.post_layers - 1 ? m.odim : m.post_chans; return C % 128 == 0 && N % 128 == 0; };
    for (int l = 0; l < m.post_layers; ++l) {
        const bool last = l == m.post_layers - 1;
        a = base(l ? m.post_chans : m.odim, m.post_k, last ? m.odim : m.post_chans, c.R, true);
        if (!last) a.act_post = 2; else { a.resid = M; a.ldr = m.odim; }
        if (pl) {
            a.Xp = M;
            if (!last) { a.Y = nullptr; a.Yp = M; a.yp_chunks = round_up(a.N, 32) / 32; }
            const bool post_mx = (c.terms == kFfnMx || c.terms == kFfnMx4) && c.o.post_mx;
            if (post_mx && !last && has_mx(l + 1)) a.yp_f16 = 2;
            if (post_mx && l > 0 && has_mx(l)) a.mx = 1;
        } else a.xp_scratch = M;
        c.emit(("postnet." + std::to_string(l)).c_str(), a);
    }
}

const struct { const char* name; int prec, terms; } kModes[] = {{"fp32", kFp32, 0}, {"bf16x3", kBf16x3, 0}, {"mix_mx", kBf16x3, kFfnMx}, {"mix_mx4", kBf16x3, kFfnMx4}};

int model(int Rtok, int reg_tok, int Rfr, int reg_fr) {
    const Model m;
    for (const auto& md : kModes) {
        Call c{md.prec, md.terms, Rtok, round_up(Rtok, 128), reg_tok, md.name, Options()};
        encode(m, c);
        c.R = Rfr; c.Rpad = round_up(Rfr, 128); c.regime = reg_fr;
        decode(m, c);
        // the plan does not depend on the row capacity (device-driven layout: 15-25 % above the rows in use)
        std::string plans[3];
        const double caps[3] = {1.0, 1.15, 1.25};
        for (int i = 0; i < 3; ++i) {
            Call k = c;
            k.R = (int)(reg_fr * caps[i]); k.Rpad = round_up(k.R, 128); k.all = &plans[i];
            decode(m, k);
        }
        printf("%s capacity_independent %d\n", md.name, (int)(plans[0] == plans[1] && plans[0] == plans[2] && !plans[0].empty()));
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
                    for (int ddim : {256, 384}) {
                        Model m; m.ddim = ddim;
                        Options o; o.row8 = row8; o.row4 = row4;
                        const bool was = old_planes_only_regime({m.ddim, m.dunits, m.adim}, {false, false}, prec, regime, o);
                        const bool now = planes_only(m, prec, 0, regime, regime, o), at_cap = planes_only(m, prec, 0, (int)(regime * 1.25) + 1, regime, o);
                        printf("%d %d %d %s %d %d %d %d\n", regime, row8, row4, prec == kBf16 ? "bf16" : "bf16x3", ddim, (int)was, (int)now, (int)at_cap);
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

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "model")) return model(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !strcmp(argv[1], "refusals")) return refusals();
    fprintf(stderr, "usage: probe model Rtok regime_tok Rfr regime_fr | sweep | refusals\n");
    return 2;
}
