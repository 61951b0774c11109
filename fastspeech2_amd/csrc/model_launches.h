// The model's GEMM launches, stated once: the weight descriptors, and for every named launch of the model the arguments it is made with, as short lists of steps.
// fs2_runtime.hip executes the lists (run_stack, run_predictor, run_predictors_fused, tok.proj and the tail of fs2_decode), tests/gemm_plan_probe.cpp walks them on
// the CPU.  Who decides what: this header HOW a launch is made (its arguments; gemm_plan.h / attn_plan.h then choose the kernel), call_plan.h WHICH launches a call
// consists of -- the booleans the functions here take (po, post_pl, layer0, the tok.proj slice) are fields of its plans, and plan_decode asks planes_only below for po.
// HIP-free like gemm_plan.h: integers and pointers nobody follows here (DESIGN.md sections 7.1 and 7.3).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gemm_args.h"
#include "gemm_plan.h"

namespace fs2 {

// The mixed precisions of include/fs2.h (fs2_runtime.hip static_asserts that they agree; kPlanFp32 / kPlanBf16x3 are gemm_plan.h's).
constexpr int kPrecMixF16x2 = 3, kPrecMixF16x1 = 4, kPrecMixMx = 5, kPrecMixMx4 = 6;

struct Gemm {          // one repacked Linear / Conv1d; which images it holds: weight_plan.h
    float* w = nullptr;      // [Npad][ktaps][Cpad]
    void* wb = nullptr;      // split-bf16 image [Npad][ktaps][Cpad/32][hi 32 | lo 32]
    void* wf = nullptr;      // the same image in fp16 (FFN w_1 only): operand of the two- / one-term arithmetic modes
    void* wm = nullptr;      // weight image of the "mx" mode (gemm_mx.h; FFN w_1 convolutions with C % 128 == 0 and N % 128 == 0) ...
    int kw = 0;              // ... and the exponent of its static scale: |w| 2^kw <= 448
    void* wm4 = nullptr;     // weight image of the "mx4" mode (gemm_planes.h ARITH = 3: both cross terms in e2m1) ...
    unsigned char* ws4 = nullptr;      // ... and its scale image: one E8M0 byte per 16-channel block of every weight row (weight_plan.h: mx4_scale_image_bytes)
    float* bias = nullptr;   // [N] or null
    int N = 0, C = 0, Cpad = 0, ktaps = 1;
};
// Output rows [n0, N) of a repacked layer as a layer of its own (n0 a multiple of 128: whole column tiles).  The one place besides the repack kernels that knows the
// row strides of their images: fp32 [Npad][ktaps][Cpad] (elementwise.h: repack_weight), split-bf16 [Npad][Cpad / 32][ktaps][64] (gemm_bf16.h: repack_weight_bf16).
// The fp16 / mx images are not carried over.
inline Gemm gemm_rows_from(const Gemm& g, int n0) {
    Gemm r;
    r.N = g.N - n0; r.C = g.C; r.Cpad = g.Cpad; r.ktaps = g.ktaps;
    r.w = g.w + (size_t)n0 * g.ktaps * g.Cpad;
    r.wb = reinterpret_cast<uint16_t*>(g.wb) + (size_t)n0 * (g.Cpad / 32) * g.ktaps * 64;
    r.bias = g.bias ? g.bias + n0 : nullptr;
    return r;
}
struct Layer {
    Gemm qkv, out, w1, w2;
    Gemm cat_x, cat_a;       // concat_after: concat_linear [D, 2D] split into its x half (carries the bias) and its attention half
    float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
    int ka = 0;              // "mx" mode: exponent of the static scale of the FFN input (the LN1 output): |x| 2^ka <= 448 from the bound
                             // |LN(x)_c| <= sqrt(D) |gamma_c| + |beta_c|
    int kh = 0;              // ... and of the FFN hidden layer (w_2's input in the mx arithmetic, gemm_row4.h ARITH = 2): |h| 2^kh <= 448 from the bound
                             // |h_n| <= sum_{c,tap} |w_1[n,c,tap]| xmax + |b_1[n]|, xmax = the LayerNorm bound above (w2.wm != nullptr: the mode exists)
};
struct Predictor {
    std::vector<Gemm> conv;
    std::vector<float*> lng, lnb;
    float *lin_w = nullptr, *lin_b = nullptr;
};
// The energy and the pitch predictor read the same input (reference fastspeech.py:194-196,214-217): in the bf16 modes they run as ONE launch per
// layer.  Layer 0: the two convolutions stacked along N (2 x chans outputs over one A tile).  Layer 1: a grouped convolution (group g
// contracts the channels of predictor g's hidden layer) with both scalar heads.  Parameters stacked along N in the order energy | pitch.
struct FusedPredictors {
    bool ok = false;
    Gemm c0, c1;
    float *ln0g = nullptr, *ln0b = nullptr, *ln1g = nullptr, *ln1b = nullptr, *lin_w = nullptr, *lin_b = nullptr;
};
struct Stack {
    std::vector<Layer> layers;
    float* pe = nullptr; int pe_rows = 0;
    float* alpha = nullptr;
    int dk = 0, Dp = 0;                             // true head dim; attention width heads x padded head dim (= D when dk is a kernel size)
    bool pre_ln = false, concat = false;            // encoder.py:53-71: normalize_before / concat_after
    float *after_g = nullptr, *after_b = nullptr;   // after_norm (applied only when pre_ln, encoder.py:201-202)
};
// The buffers of an FFT-block stack.  x0p / x1p: split-bf16 planes of x0 / x1 (gemm_planes.h); xps: planes scratch for activations produced without planes.
// In the bf16 modes the attention context and the FFN hidden layer exist ONLY as planes, in the ctx / hid storage.  qkh .. vtl: the attention's bf16 operands.
struct StackBufs { float *x0, *x1, *qkv, *ctx, *hid; void *qkh, *qkl, *vth, *vtl; void *x0p, *x1p, *xps; unsigned char* xs4 = nullptr; };      // xs4: row-scale bytes of x1p in the mx4 format
// The rows of a call: R of them (Rpad: the attention operands'), their metadata, and the row count the kernel choice is based on (gemm_args.h: regime_rows).
struct Rows { int R = 0, Rpad = 0; const int* row_pos = nullptr; const int* Rp = nullptr; int regime_rows = 0; };

// The attention kernels exist for head dims 64 / 128 / 192 / 256.  Any other adim / aheads the reference accepts (core/attention.py:18-20)
// runs with the head dim zero-padded to the next of these: the Q / K / V projection weights get zero rows, the output projection zero
// columns, at load time, so scores and context are unchanged (the softmax scale keeps the true d_k); the attention buffers are
// heads x padded wide.  0: unsupported (d_k > 256).
inline int padded_head_dim(int dk) { return dk <= 64 ? 64 : (dk <= 128 ? 128 : (dk <= 192 ? 192 : (dk <= 256 ? 256 : 0))); }
inline int att_width(int D, int heads) { return heads * padded_head_dim(D / heads); }

// Mixed modes: everything as bf16x3 except the FFN convolution w_1, which runs on fp16 operands with 2 or 1 MFMA per fragment pair.
inline int base_precision(int p) { return (p == kPrecMixF16x2 || p == kPrecMixF16x1 || p == kPrecMixMx || p == kPrecMixMx4) ? kPlanBf16x3 : p; }
constexpr int kFfnMx = 9;      // value of "ffn_terms" that selects the fp16 + block-scaled-fp8 arithmetic (gemm_mx.h)
constexpr int kPostKa = 8;     // static scale exponent of the Postnet's mx operands: tanh outputs, |x| <= 1 -> 2^8 = 256 <= 448
constexpr int kFfnMx4 = 10;    // ... the fp16 + block-scaled-fp4 arithmetic where the planes-only regime offers it (gemm_planes.h ARITH = 3), kFfnMx's elsewhere
inline int ffn_f16_terms(int p) { return p == kPrecMixF16x2 ? 2 : (p == kPrecMixF16x1 ? 1 : (p == kPrecMixMx ? kFfnMx : (p == kPrecMixMx4 ? kFfnMx4 : 0))); }
inline bool ffn_is_mx(int ffn_terms) { return ffn_terms == kFfnMx || ffn_terms == kFfnMx4; }
inline int scale_byte4(int e) { const int b = std::min(std::max(e, 1), 254); return b * 0x01010101; }

inline GemmArgs gemm_args(const Gemm& g, const float* X, int ldx, int R, const int* row_pos, float* Y, int ldy) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.X = X; a.ldx = ldx; a.C = g.C; a.W = g.w; a.Cpad = g.Cpad; a.ktaps = g.ktaps; a.N = g.N; a.R = R;
    a.row_pos = row_pos; a.bias = g.bias; a.Y = Y; a.ldy = ldy; a.x_scale = 1.f; a.ln_eps = 1e-5f; a.Wb = g.wb;
    return a;
}
// a stand-alone LayerNorm over rows (ln_rows, out of place): src [R, ld] -> Y [R, N] fp32 and / or planes
inline GemmArgs ln_args(const float* src, int ld, const Rows& r, int N, const float* g, const float* bta, float* Y, void* Yp) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.N = N; a.R = r.R; a.row_pos = r.row_pos; a.Y = Y; a.ldy = N; a.Ysrc = src; a.ldsrc = ld; a.ln_g = g; a.ln_b = bta; a.ln_eps = 1e-5f;
    a.x_scale = 1.f; a.ksplit = 1; a.Yp = Yp; a.yp_chunks = (N + 31) / 32;
    return a;
}
// What a launch inherits from the call it is part of, before it is planned: the call's split-K scratch (a.ksplit: how many partial buffers the plan may use)
// and its regime.
inline void call_defaults(GemmArgs& a, float* kpart, size_t kpart_cap, int regime_rows) {
    if (!a.kpart && kpart) { a.kpart = kpart; a.kpart_cap = kpart_cap; a.ksplit = 3; }
    if (!a.regime_rows) a.regime_rows = regime_rows;
}
// Does FFN2 + LN2 run in gemm_row4_bf16's mx arithmetic if it is offered mx planes?  (block_steps asks before it decides the format FFN1 leaves the hidden layer in.)
inline bool ffn2_on_row4_mx(GemmArgs a, const Options& o) { a.mx = 1; const GemmPlan p = plan_gemm(a, kPlanBf16x3, o); return p.kernel == GemmKernel::Row4 && p.arith == 2; }

// ------------------------------------------------------------------ steps
// A launch of the model: the suffix of its profile name, what runs it, its arguments.  Gemm: launch_gemm.  Attention: a.X = the fp32 QKV rows (nullptr: the
// projection has left the bf16 operands), a.Y / a.Yp = the context as fp32 rows / as planes.  LayerNorm: ln_args.
enum class StepKind { Gemm, Attention, LayerNorm };
struct Step { char name[16]; StepKind kind; GemmArgs a; };
inline Step make_step(StepKind kind, const GemmArgs& a, const char* name, int index = -1) {
    Step s;
    if (index >= 0) snprintf(s.name, sizeof s.name, "%s%d", name, index); else snprintf(s.name, sizeof s.name, "%s", name);
    s.kind = kind; s.a = a;
    return s;
}
template <int N>
struct Steps {      // a list of at most N steps, in launch order (no heap: formed once per layer and call)
    Step s[N]; int n = 0;
    void add(StepKind kind, const GemmArgs& a, const char* name) { s[n++] = make_step(kind, a, name); }
    const Step* begin() const { return s; }
    const Step* end() const { return s + n; }
    const Step* find(const char* name) const { for (const Step& t : *this) if (!strcmp(t.name, name)) return &t; return nullptr; }
};

// ------------------------------------------------------------------ one FFT block
// Every variant of the block (reference core/encoder.py:53-71): the default post-LN block, whose out-projection and second FFN GEMM end in the LayerNorm
// (out_ln, ffn2_ln), normalize_before (ln1 / ln2 in front of the sub-layers; the stack's runner applies after_norm) and / or concat_after
// (x + concat_linear(cat(x, a)) as x . Wc[:, :D]^T + a . Wc[:, D:]^T: cat_x, cat_a chained through the residual input).  x0 holds the block's input and its output.
// Scratch of the variants: ln1's output -> hid / xps, the attention output a -> qkv / qkh (both free once the attention kernel has run), ln2's -> qkv / xps.
// po: the planes-only residual stream (gemm_row4.h: RES; planes_only decides): the LayerNorm-fused launches write no fp32 rows and take their residual from the
// planes of the producing launch -- x0 / x1 are then never written: the output is b.x0p.  Default block only, like the mixed forms of the FFN.
inline Steps<9> block_steps(const Stack& st, const Layer& ly, int D, const Rows& r, const StackBufs& b, int prec, int ffn_terms, bool po, const Options& o) {
    Steps<9> out;
    const bool pl = prec != kPlanFp32, pre = st.pre_ln, cat = st.concat;      // pl: activations travel between the GEMMs as split-bf16 planes
    const int Dp = st.Dp, terms = (pre || cat) ? 0 : ffn_terms;
    void* ctxp = pl ? (void*)b.ctx : nullptr;
    void* hidp = pl ? (void*)b.hid : nullptr;
    auto gemm = [&](const Gemm& g, const float* X, int ldx, const void* Xp, float* Y, int ldy) {
        GemmArgs a = gemm_args(g, X, ldx, r.R, r.row_pos, Y, ldy);
        a.Rp = r.Rp; a.regime_rows = r.regime_rows; a.Xp = Xp;
        return a;
    };
    const float* qin = b.x0; const void* qinp = pl ? b.x0p : nullptr;
    if (pre) {
        out.add(StepKind::LayerNorm, ln_args(b.x0, D, r, D, ly.ln1g, ly.ln1b, pl ? nullptr : b.hid, pl ? b.xps : nullptr), "ln1");
        qin = b.hid; qinp = pl ? b.xps : nullptr;
    }
    GemmArgs a = gemm(ly.qkv, qin, D, qinp, b.qkv, 3 * Dp);
    const bool fused_split = pl && Dp % kPlanBN == 0;
    if (fused_split) {   // bf16 attention operands straight from the GEMM epilogue (no fp32 QKV round trip)
        a.Y = nullptr; a.qk_hi = b.qkh; a.qk_lo = b.qkl; a.vt_hi = b.vth; a.vt_lo = b.vtl; a.att_D = Dp; a.Rvt = r.Rpad;
        a.q_scale = 1.4426950408889634f / sqrtf((float)st.dk);
    }
    out.add(StepKind::Gemm, a, "qkv");
    GemmArgs at;
    memset(&at, 0, sizeof at);
    at.X = fused_split ? nullptr : b.qkv; at.Y = pl ? nullptr : b.ctx; at.Yp = ctxp;
    out.add(StepKind::Attention, at, "attn");

    const bool mx4l = po && terms == kFfnMx4 && ly.w1.wm4 && b.xs4 && D == 384;      // this layer's FFN conv in the mx4 arithmetic (fp4 cross terms; planes-only regime)?
    const bool mxl = pl && ffn_is_mx(terms) && ly.w1.wm;                            // ... in the mx arithmetic (also the fallback of mix_mx4 wherever mx4 does not apply)?
    const int f16t = (pl && terms && !ffn_is_mx(terms) && ly.w1.ktaps > 1 && ly.w1.wf) ? terms : 0;      // ... or on fp16 operands?
    // the sub-layer's output x1 (+ LN1 when post-LN): planes in the format the FFN conv wants, which alone reads them
    auto x1_out = [&](GemmArgs& g) {
        if (pre) return;
        g.ln_g = ly.ln1g; g.ln_b = ly.ln1b;
        if (pl) { g.Yp = b.x1p; g.yp_chunks = D / 32; }
        if (pl && !cat) { g.yp_f16 = mx4l ? 3 : (mxl ? 2 : (f16t ? 1 : 0)); g.yp_scale = mxl ? exp2f((float)ly.ka) : 1.f; }
        if (mx4l) g.yp_rowscale = b.xs4;
    };
    if (cat) {
        float* att = b.qkv; void* attp = pl ? b.qkh : nullptr;
        a = gemm(ly.out, b.ctx, Dp, ctxp, pl ? nullptr : att, D);
        if (pl) { a.Yp = attp; a.yp_chunks = D / 32; }
        out.add(StepKind::Gemm, a, "out");
        a = gemm(ly.cat_x, qin, D, qinp, b.x1, D);
        a.resid = b.x0; a.ldr = D;
        out.add(StepKind::Gemm, a, "cat_x");
        a = gemm(ly.cat_a, att, D, attp, b.x1, D);
        a.resid = b.x1; a.ldr = D;      // in place: every element is read, then written, by one lane
        x1_out(a);
        out.add(StepKind::Gemm, a, "cat_a");
    } else {
        a = gemm(ly.out, b.ctx, Dp, ctxp, po ? nullptr : b.x1, D);
        if (po) { a.residp = b.x0p; a.residp_chunks = D / 32; }      // (x0p: split-bf16 planes, from the input layer or the previous block's FFN2 + LN2)
        else { a.resid = b.x0; a.ldr = D; }
        x1_out(a);
        out.add(StepKind::Gemm, a, pre ? "out" : "out_ln");
    }
    const float* fin = b.x1; const void* finp = pl ? b.x1p : nullptr;
    if (pre) {
        out.add(StepKind::LayerNorm, ln_args(b.x1, D, r, D, ly.ln2g, ly.ln2b, pl ? nullptr : b.qkv, pl ? b.xps : nullptr), "ln2");
        fin = b.qkv; finp = pl ? b.xps : nullptr;
    }
    // the second FFN GEMM: formed first, because WHERE it will run decides the format the hidden layer leaves FFN1 in (mx planes for gemm_row4_bf16's
    // mx form, split-bf16 planes for everything else)
    GemmArgs a2 = gemm(ly.w2, b.hid, ly.w1.N, hidp, po ? nullptr : b.x0, D);
    if (po) { a2.residp = b.x1p; a2.residp_chunks = D / 32; a2.residp_mx = mx4l ? 2 : (mxl ? 1 : 0); a2.residp_scale = mxl ? exp2f(-(float)(ly.ka + 11)) : 1.f; }      // (x1p: LN1's output in the format the FFN conv wants)
    else { a2.resid = b.x1; a2.ldr = D; }
    if (!pre) { a2.ln_g = ly.ln2g; a2.ln_b = ly.ln2b; if (pl) { a2.Yp = b.x0p; a2.yp_chunks = D / 32; } }
    const bool mx2 = mxl && ly.w2.wm && o.ffn2_mx && prec == kPlanBf16x3 && ffn2_on_row4_mx(a2, o);
    if (mx2) { a2.mx = 1; a2.Wb = ly.w2.wm; a2.mx_scale = scale_byte4(127 - ly.kh - 11); a2.mx_scale_b = scale_byte4(127 - ly.w2.kw); }
    a = gemm(ly.w1, fin, D, finp, pl ? nullptr : b.hid, ly.w1.N);
    a.act_post = 1;
    if (pl) { a.Yp = hidp; a.yp_chunks = (ly.w1.N + 31) / 32; }
    if (mx2) { a.yp_f16 = 2; a.yp_scale = exp2f((float)ly.kh); }
    if (f16t) { a.f16_terms = f16t; a.Wb = ly.w1.wf; }
    if (mx4l) { a.mx = 2; a.Wb = ly.w1.wm4; a.x_rowscale = b.xs4; a.w_rowscale = ly.w1.ws4; }
    else if (mxl) { a.mx = 1; a.Wb = ly.w1.wm; a.mx_scale = scale_byte4(127 - ly.ka - 11); a.mx_scale_b = scale_byte4(127 - ly.w1.kw); }
    out.add(StepKind::Gemm, a, "ffn1");
    out.add(StepKind::Gemm, a2, (pre || cat) ? "ffn2" : "ffn2_ln");
    return out;
}

// ------------------------------------------------------------------ the predictors
// Layer l of a conv stack + scalar head (reference variance_predictor.py:46-51 / duration_predictor.py:70-75); tmp0 / tmp1: [R, chans] scratch, out_rows: [R].
// Planes: the first layer's input from the caller (Xp; or built in xps), later layers' from the row kernel of the previous one (it runs after the GEMM that
// read xps, so the buffer is reused in place).
inline Step predictor_step(const Predictor& p, size_t l, const float* X, int ldx, const Rows& r, float* tmp0, float* tmp1, float* out_rows, int prec, const void* Xp, void* xps) {
    const bool last = l + 1 == p.conv.size();
    float* const bufs[2] = {tmp0, tmp1};
    float* out = bufs[l & 1];
    // bf16 modes: the next layer consumes the planes; the fp32 copy is written only where a kernel pair needs it as scratch
    GemmArgs a = gemm_args(p.conv[l], l ? bufs[(l - 1) & 1] : X, l ? p.conv[l - 1].N : ldx, r.R, r.row_pos, (last || (xps && prec != kPlanFp32)) ? nullptr : out, p.conv[l].N);
    a.Rp = r.Rp;
    a.relu_pre = 1; a.ln_g = p.lng[l]; a.ln_b = p.lnb[l]; a.ln_eps = 1e-12f;
    if (last) { a.dot_w = p.lin_w; a.dot_b = p.lin_b; a.dot_out = out_rows; }
    a.scratch = out;
    a.Xp = l ? xps : Xp; a.xp_scratch = xps;
    if (xps && !last) { a.Yp = xps; a.yp_chunks = (p.conv[l].N + 31) / 32; }
    return make_step(StepKind::Gemm, a, "conv", (int)l);
}

// The pitch and the energy predictor of the bf16 modes as one launch per layer (FusedPredictors).  Every output column is accumulated in the
// order of the separate launches; the LayerNorm of a 256-column group may be summed in another order than the two-wave form (1e-7).
// layer0 = false: the caller has computed layer 0 from the token-level products (var.gather0).  vp / vs: planes / fp32 scratch of the stacked hidden layer.
inline Steps<3> fused_predictor_steps(const FusedPredictors& v, const Predictor& energy, const Predictor& pitch, bool layer0, const float* X, int ldx, const Rows& r,
                                      const void* Xp, void* xps, float* vp, float* vs, float* e_rows, float* p_rows, const Options& o) {
    Steps<3> out;
    const int chans = v.c0.N / 2;
    auto conv = [&](const Gemm& g, const float* in, int ld, const float* lng, const float* lnb) {
        GemmArgs a = gemm_args(g, in, ld, r.R, r.row_pos, nullptr, g.N);
        a.Rp = r.Rp; a.relu_pre = 1; a.ln_g = lng; a.ln_b = lnb; a.ln_eps = 1e-12f; a.scratch = vs;
        a.regime_rows = r.regime_rows;      // (the rows' own: the short rows of FS2_VARSHORT are not the call's frame rows)
        return a;
    };
    if (layer0 && row_regime(r.regime_rows ? r.regime_rows : r.R, o.row8) && (chans == 256 || chans == 384)) {
        // big grids: layer 0 as two row-complete launches (the stacked 512-column form exists at 128-row tiles only -- 128 accumulator
        // registers -- and pays a nearly empty second round where the 192-row form does not: c3 0.169 ms against 2 x 0.07), each filling its half
        // of the stacked plane rows
        const Predictor* ps[2] = {&energy, &pitch};
        for (int g = 0; g < 2; ++g) {
            GemmArgs a = conv(ps[g]->conv[0], X, ldx, ps[g]->lng[0], ps[g]->lnb[0]);
            a.Xp = Xp; a.xp_scratch = xps; a.Yp = vp; a.yp_chunks = v.c0.N / 32; a.yp_col_off = g * chans;
            out.add(StepKind::Gemm, a, g ? "pitch.conv0" : "energy.conv0");
        }
    } else if (layer0) {
        GemmArgs a = conv(v.c0, X, ldx, v.ln0g, v.ln0b);
        a.ln_groups = 2; a.Xp = Xp; a.xp_scratch = xps; a.Yp = vp; a.yp_chunks = v.c0.N / 32;
        out.add(StepKind::Gemm, a, "var.conv0");
    }
    GemmArgs a = conv(v.c1, nullptr, v.c0.N, v.ln1g, v.ln1b);
    a.ln_groups = 2; a.k_groups = 2; a.Xp = vp; a.xp_row_chunks = v.c0.N / 32;
    a.dot_w = v.lin_w; a.dot_b = v.lin_b; a.dot_out = e_rows; a.dot_gstride = (int)(p_rows - e_rows);
    out.add(StepKind::Gemm, a, "var.conv1");
    return out;
}

// tok.proj (fs2_encode; call_plan.h: EncodePlan): the encoder rows X / Xp times the columns [n0, N) of the stacked k = 1 weight, into the same columns of P [R, tokw.N].
// kpart without ksplit: the launch names the call's scratch but allows no partial buffers -- never split-K: one kernel whatever the batch or the slice.
inline Step tok_proj_step(const Gemm& tokw, int n0, const float* X, int ldx, const Rows& r, const void* Xp, void* xps, float* P, float* kpart) {
    GemmArgs a = gemm_args(gemm_rows_from(tokw, n0), X, ldx, r.R, r.row_pos, P + n0, tokw.N);
    a.Xp = Xp; a.xp_scratch = xps;
    a.kpart = kpart; a.kpart_cap = 0;
    return make_step(StepKind::Gemm, a, "tok.proj");
}

// ------------------------------------------------------------------ the decoder's input layer and tail
// The decoder input layer (where the model has one and it is not gathered from token-level products): Linear -> LN -> ReLU -> + alpha * pe
// (reference encoder.py:118-125).  X / Xp: the length-regulator rows (+ embeddings) and their planes (nullptr: built in b.xps).
struct DecIn { const Gemm* g = nullptr; const float *ln_g = nullptr, *ln_b = nullptr; float x_scale = 1.f; };      // g == nullptr: the model has no input layer
inline Step dec_in_step(const DecIn& in, const Stack& dec, const float* X, int ldx, const void* Xp, const Rows& r, const StackBufs& b, int prec, bool po) {
    const int D = in.g->N;
    GemmArgs a = gemm_args(*in.g, X, ldx, r.R, r.row_pos, po ? nullptr : b.x0, D);
    a.Rp = r.Rp; a.regime_rows = r.regime_rows;
    a.ln_g = in.ln_g; a.ln_b = in.ln_b; a.act_post = 1;
    a.pe = dec.pe; a.pe_ld = D; a.pe_alpha = dec.alpha; a.x_scale = in.x_scale;
    a.Xp = Xp; a.xp_scratch = b.xps;
    if (prec != kPlanFp32) { a.Yp = b.x0p; a.yp_chunks = D / 32; }
    return make_step(StepKind::Gemm, a, "dec.in");
}

// Will the decoder's LayerNorm-fused k = 1 launches (the input layer, out-proj + LN1, FFN2 + LN2) run on gemm_row4_bf16 -- i.e. do its activations travel
// as planes ONLY (0.9 GB per c3 step, 11 GB per c4 step of HBM writes less)?  Asked of the plan, once per fs2_decode, for these launches in their planes-only
// form; anything the plan would not put there leaves the decoder on the fp32-rows form, as do the block variants, which have no such form, and the fp16 two- /
// one-term modes (their LN1 output is a fp16 hi + lo pair, a format the residual reader does not have).
inline bool planes_only(const DecIn& in, const Stack& dec, int D, const Rows& r, const StackBufs& b, int prec, int ffn_terms, const Options& o) {
    if (dec.pre_ln || dec.concat || dec.layers.empty() || !(ffn_terms == 0 || ffn_is_mx(ffn_terms))) return false;
    auto on_row4 = [&](const GemmArgs& a) { return plan_gemm(a, prec, o).kernel == GemmKernel::Row4; };
    const Steps<9> blk = block_steps(dec, dec.layers[0], D, r, b, prec, ffn_terms, /*po=*/true, o);
    return (!in.g || on_row4(dec_in_step(in, dec, nullptr, in.g->C, b.x1p, r, b, prec, true).a)) && on_row4(blk.find("out_ln")->a) && on_row4(blk.find("ffn2_ln")->a);
}

// feat_out: the decoder rows -> rf mel frames per row (`before`, fp32) and, where the Postnet takes planes (post_pl), the planes of them
inline Step feat_out_step(const Gemm& feat, const Rows& r, const StackBufs& b, float* before, int prec, bool post_pl) {
    GemmArgs a = gemm_args(feat, b.x0, feat.C, r.R, r.row_pos, before, feat.N);
    a.Rp = r.Rp;
    if (prec != kPlanFp32) a.Xp = b.x0p;
    if (post_pl) { a.Yp = b.xps; a.yp_chunks = (feat.N + 31) / 32; }
    return make_step(StepKind::Gemm, a, "feat_out");
}
// Layer l of the Postnet: before -> pa -> pb -> pa .. -> after (+ before).  post_pl: the layers hand planes on, feat_out's in b.xps, then x0p / x1p in turn;
// else each builds its input planes in xps.  r: the Postnet's rows (reduction_factor per decoder row).
struct PostBufs { float *before, *after, *pa, *pb; void* xps; };
inline Step postnet_step(const std::vector<Gemm>& post, int l, int odim, const Rows& r, const PostBufs& t, const StackBufs& b, bool post_pl, int ffn_terms, const Options& o) {
    const bool last = l + 1 == (int)post.size();
    float* out = last ? t.after : ((l & 1) ? t.pb : t.pa);
    const float* in = l == 0 ? t.before : ((l & 1) ? t.pa : t.pb);
    GemmArgs a = gemm_args(post[l], in, l ? post[l - 1].N : odim, r.R, r.row_pos, out, post[l].N);
    a.Rp = r.Rp;
    if (!last) a.act_post = 2; else { a.resid = t.before; a.ldr = odim; }
    if (post_pl) {
        a.Xp = (l == 0) ? b.xps : ((l & 1) ? b.x0p : b.x1p);
        if (!last) { a.Y = nullptr; a.Yp = (l & 1) ? b.x1p : b.x0p; a.yp_chunks = (post[l].N + 31) / 32; }
        // the 512 -> 512 layers in the mx arithmetic of the mixed modes (fp16 main term + e4m3 cross terms, 2 MFMA-equivalents instead of 3; simulated:
        // mel +6e-6, tools/arith_sim_postnet.py): a layer whose image exists takes mx planes, so the layer in front of it writes them (tanh output: static scale 2^8)
        const bool post_mx = ffn_is_mx(ffn_terms) && o.post_mx;
        if (post_mx && !last && post[l + 1].wm) { a.yp_f16 = 2; a.yp_scale = exp2f((float)kPostKa); }
        if (post_mx && l > 0 && post[l].wm) { a.mx = 1; a.Wb = post[l].wm; a.mx_scale = scale_byte4(127 - kPostKa - 11); a.mx_scale_b = scale_byte4(127 - post[l].kw); }
    } else {
        a.xp_scratch = t.xps;
    }
    return make_step(StepKind::Gemm, a, "postnet.", l);
}

}  // namespace fs2
