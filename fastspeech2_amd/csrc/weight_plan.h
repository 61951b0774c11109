// The weight plan: which images a Linear / Conv1d weight gets at load time, decided once.  A call site states a WeightAsk -- the shape,
// the form of the source and what the layer's role asks for -- and plan_weight answers with the padded sizes, the byte size of every image (0: not built), where
// the mx image comes from and the shape every source tensor must have.  fs2_runtime.hip only executes the answer (build_weight: the loader, fs2_op_conv_gemm and
// fs2_op_repack_weight), tests/gemm_plan_probe.cpp marks a layer's images from it.  The asks of the model's layers are formed below, one function per kind of
// layer, for the loader and the probe alike.  The arithmetic modes rest on the answer: model_launches.h chooses the arithmetic of a launch by the images present.
// A new image, or a new condition for an existing one, is decided here and nowhere else.
// HIP-free like gemm_plan.h: integers and sizes only.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define WP_HD __host__ __device__
#else
#define WP_HD
#endif

namespace fs2 {

// ---- the sizes of the images (Npad: N rounded up to 128 rows, Cpad: C rounded up to 32 channels)
// fp32 [Npad][ktaps][Cpad] (elementwise.h: repack_weight)
inline size_t f32_image_bytes(int Npad, int Cpad, int ktaps) { return (size_t)Npad * ktaps * Cpad * sizeof(float); }
// split-bf16 / fp16 [Npad][Cpad / 32][ktaps][hi 32 | lo 32] of 2-byte words (gemm_bf16.h: repack_weight_bf16)
inline size_t bf16_image_bytes(int Npad, int Cpad, int ktaps) { return (size_t)Npad * ktaps * (Cpad / 32) * 64 * 2; }
// mx: Npad rows x (C / 32 units) x ktaps x 128 B  (= the split-bf16 image's size; gemm_mx.h: repack_weight_mx)
WP_HD inline size_t mx_image_bytes(int Npad, int C, int ktaps) { return (size_t)Npad * (C / 32) * ktaps * 128; }
// mx4: units per (n, tap): C/64 of fp16 channels, then C/128 cross units (layout: gemm_planes.h; gemm_mx.h: repack_weight_mx4)
WP_HD inline size_t mx4_image_bytes(int Npad, int C, int ktaps) { return (size_t)Npad * (C / 64 + C / 128) * ktaps * 128; }
// the mx4 weight scale image: per (N tile of 128 output channels, cross unit, tap) 1 KB = [g = 0 .. 3][n = 0 .. 127][2]: byte 0 = the E8M0 scale of the
// 16-byte slot g of that weight row (16 channels, both terms: the block lane (n, g) hands the first scaled MFMA of a cross-unit step), byte 1 = of slot 4 + g
// (the second MFMA's).  One LDS-DMA piece per step; a lane's four output channels are eight contiguous bytes.
WP_HD inline size_t mx4_scale_image_bytes(int Npad, int C, int ktaps) { return (size_t)(Npad / 128) * (C / 128) * ktaps * 1024; }

// ---- the question
struct WeightAsk {
    int parts = 1;               // weights stacked along N (q|k|v, the fused predictors), Neach rows each
    int Neach = 0, C = 0, ktaps = 1;
    bool linear = false;         // the source is a Linear weight [Neach, C]; otherwise a Conv1d weight [Neach, C, ktaps]
    int col_off = 0, src_cols = 0;      // a concat half: columns [col_off, col_off + C) of a Linear weight stored [Neach, src_cols]
    bool bias = false;           // the layer has bias tensors [Neach], one per part
    bool bn = false;             // BatchNorm [Neach] folded into the weights; its shift is the bias when the layer has none
    // the extra images the layer's role asks for, built where the shape allows:
    bool f16 = false;            // the fp16 twin of the split-bf16 image
    bool mx_conv = false;        // the mx image of a convolution ...
    bool mx4 = false;            // ... and with it the mx4 image and its scale image
    bool mx_k1 = false;          // the mx image of a k = 1 layer
};

// ---- the answer
enum WeightImage { kImgW, kImgWb, kImgWm, kImgWm4, kImgWs4, kImgWf, kImgBias, kWeightImages };      // Gemm::w, wb, wm, wm4, ws4, wf, bias: the order they are allocated in
enum class MxSource { None, Tensor, Folded };      // the mx image is made from the caller's tensor, or from the library's own (BatchNorm-folded) fp32 image

struct WeightPlan {
    int N = 0, Npad = 0, Cpad = 0, nchunks = 0;
    size_t bytes[kWeightImages] = {};      // 0: the image is not built
    MxSource mx_src = MxSource::None;
    int w_ndim = 0; int64_t w_shape[3] = {};      // the shape of every part's weight tensor; its bias and BatchNorm tensors are [vec_len]
    int64_t vec_len = 0;
    bool has(WeightImage i) const { return bytes[i] != 0; }
    size_t total_bytes() const { size_t t = 0; for (size_t b : bytes) t += b; return t; }
};

inline int wp_round_up(int x, int a) { return (x + a - 1) / a * a; }

// the sizes every plan starts from
inline WeightPlan plan_sizes(int N, int C) {
    WeightPlan p;
    p.N = N; p.Npad = wp_round_up(N, 128); p.Cpad = wp_round_up(C, 32); p.nchunks = p.Cpad / 32;
    return p;
}

inline WeightPlan plan_weight(const WeightAsk& a) {
    WeightPlan p = plan_sizes(a.Neach * a.parts, a.C);
    p.bytes[kImgW] = f32_image_bytes(p.Npad, p.Cpad, a.ktaps);
    p.bytes[kImgWb] = bf16_image_bytes(p.Npad, p.Cpad, a.ktaps);
    if (a.f16) p.bytes[kImgWf] = bf16_image_bytes(p.Npad, p.Cpad, a.ktaps);
    // the mx kernels take one unstacked weight with whole 128-wide tiles in both directions
    const bool mx_shape = a.parts == 1 && p.N % 128 == 0 && a.C % 128 == 0;
    const bool of_conv = a.mx_conv && a.ktaps > 1 && !a.linear, of_k1 = a.mx_k1 && a.ktaps == 1 && !a.src_cols;
    if (mx_shape && !a.bn && (of_conv || of_k1)) p.mx_src = MxSource::Tensor;
    if (mx_shape && a.bn && a.ktaps > 1) p.mx_src = MxSource::Folded;      // the Postnet's inner convolutions: their operand is a tanh output
    if (p.mx_src != MxSource::None) p.bytes[kImgWm] = mx_image_bytes(p.Npad, a.C, a.ktaps);
    if (p.mx_src == MxSource::Tensor && a.mx4 && a.ktaps > 1) {
        p.bytes[kImgWm4] = mx4_image_bytes(p.Npad, a.C, a.ktaps);
        p.bytes[kImgWs4] = mx4_scale_image_bytes(p.Npad, a.C, a.ktaps);
    }
    if (a.bias || a.bn) p.bytes[kImgBias] = (size_t)(p.N > 1 ? p.N : 1) * sizeof(float);
    p.w_ndim = (a.src_cols || a.linear) ? 2 : 3;
    p.w_shape[0] = a.Neach; p.w_shape[1] = a.src_cols ? a.src_cols : a.C; p.w_shape[2] = p.w_ndim == 3 ? a.ktaps : 0;
    p.vec_len = a.Neach;
    return p;
}

// One mx / mx4 image of a Conv1d weight [N, C, ktaps] alone, whatever the loader's roles say (the repack hook fs2_op_repack_weight: N % 128 == 0, C % 128 == 0).
inline WeightPlan plan_image_alone(int N, int C, int ktaps, bool mx4) {
    WeightPlan p = plan_sizes(N, C);
    p.mx_src = MxSource::Tensor;
    if (mx4) { p.bytes[kImgWm4] = mx4_image_bytes(p.Npad, C, ktaps); p.bytes[kImgWs4] = mx4_scale_image_bytes(p.Npad, C, ktaps); }
    else p.bytes[kImgWm] = mx_image_bytes(p.Npad, C, ktaps);
    p.w_ndim = 3; p.w_shape[0] = N; p.w_shape[1] = C; p.w_shape[2] = ktaps; p.vec_len = N;
    return p;
}

// ---- the asks of the model's layers, one function per kind of layer
inline WeightAsk ask_of(int parts, int Neach, int C, int ktaps, bool linear, bool bias) {
    WeightAsk a;
    a.parts = parts; a.Neach = Neach; a.C = C; a.ktaps = ktaps; a.linear = linear; a.bias = bias;
    return a;
}
// attention, D wide with Dp = heads x padded head dim (= D when the head dim is a kernel size; otherwise the loader hands in head-padded copies)
inline WeightAsk ask_qkv(int D, int Dp) { return ask_of(3, Dp, D, 1, true, true); }
inline WeightAsk ask_attn_out(int D, int Dp) { return ask_of(1, D, Dp, 1, true, true); }
// FFN w_1 (linear: positionwise_layer_type "linear", a 2-d tensor): a convolution runs in the fp16 / mx / mx4 arithmetic too
inline WeightAsk ask_ffn_w1(int D, int units, int k, bool linear) {
    WeightAsk a = ask_of(1, units, D, k, linear, true);
    a.f16 = a.mx_conv = a.mx4 = k > 1;
    return a;
}
// FFN w_2 behind `w1`: in the mx arithmetic exactly when w_1 is and the row kernel exists for the width (gemm_row4.h is instantiated for N = 384)
inline WeightAsk ask_ffn_w2(const WeightAsk& w1, bool linear) {
    WeightAsk a = ask_of(1, w1.C, w1.Neach, 1, linear, true);
    a.mx_k1 = plan_weight(w1).has(kImgWm) && w1.C == 384;
    return a;
}
// concat_linear [D, 2 D]: half 0 meets x and carries the bias, half 1 meets the attention output
inline WeightAsk ask_concat_half(int D, int half) {
    WeightAsk a = ask_of(1, D, D, 1, true, half == 0);
    a.col_off = half * D; a.src_cols = 2 * D;
    return a;
}
inline WeightAsk ask_predictor_conv(int cin, int chans, int k) { return ask_of(1, chans, cin, k, false, true); }
inline WeightAsk ask_fused_predictor_conv(int cin, int chans, int k) { return ask_of(2, chans, cin, k, false, true); }      // energy | pitch stacked along N
inline WeightAsk ask_dec_in(int adim, int ddim) { return ask_of(1, ddim, adim, 1, true, true); }
inline WeightAsk ask_tok_proj(int adim, int cols) { return ask_of(1, cols, adim, 1, true, false); }      // the stacked weight of "multiply before expanding"
inline WeightAsk ask_feat_out(int ddim, int odim_r) { return ask_of(1, odim_r, ddim, 1, true, true); }
inline WeightAsk ask_postnet(int cin, int cout, int k, bool batch_norm) {
    WeightAsk a = ask_of(1, cout, cin, k, false, false);
    a.bn = batch_norm;
    return a;
}
// fs2_op_conv_gemm: a Conv1d weight [N, C, ktaps] whose bias stays the caller's; mx: the operator runs in the mx arithmetic
inline WeightAsk ask_conv_op(int N, int C, int ktaps, bool mx) {
    WeightAsk a = ask_of(1, N, C, ktaps, false, false);
    a.mx_conv = mx;
    return a;
}

}  // namespace fs2
