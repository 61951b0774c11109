// The argument block of the conv-as-GEMM kernels: plain data, no HIP types, so that the host-side kernel choice (gemm_plan.h) and the CPU test
// that compiles it see the same struct as the kernels (common.h includes this file).
#pragma once
#include <stddef.h>

namespace fs2 {

// Arguments of the conv-as-GEMM kernels (gemm_f32.h).  Y = epilogue(sum_taps X[row+tap-P] . W[tap]).
struct GemmArgs {
    const float* X; int ldx; int C;        // input [R, ldx], C channels contracted per tap (C % 4 == 0)
    const float* W; int Cpad; int ktaps;   // repacked weights [Npad][ktaps][Cpad], zero padded
    int N; int R;
    const int* row_pos;                    // [>= R] or nullptr (all rows valid)
    const float* bias;                     // [N] or nullptr
    const float* resid; int ldr;           // [R, ldr] or nullptr
    int relu_pre;                          // ReLU before the LayerNorm
    const float* ln_g; const float* ln_b; float ln_eps;   // LayerNorm over the N outputs if ln_g
    int act_post;                          // 0 none, 1 relu, 2 tanh
    const float* pe; int pe_ld; const float* pe_alpha; float x_scale;  // v = v*x_scale + alpha*pe[pos] if pe
    const float* dot_w; const float* dot_b; float* dot_out;            // dot_out[row] = v . dot_w + dot_b
    float* Y; int ldy;                     // output [R, ldy] or nullptr
    const float* Ysrc; int ldsrc;          // ln_rows only: read the rows from here instead of Y (out-of-place LayerNorm)
    const void* Wb;                        // split-bf16 weight image (gemm_bf16.h) or nullptr
    // fused QKV epilogue (bf16 attention operands, attn_bf16.h): when qk_hi != nullptr the tile is not written to Y
    // but split into bf16 hi/lo planes: columns [0,2D) -> qk_hi/lo [Rvt][2D] (Q scaled by q_scale), [2D,3D) -> V^T [D][Rvt]
    void *qk_hi, *qk_lo, *vt_hi, *vt_lo; int att_D; int Rvt; float q_scale;
    float* scratch;                        // [R, N] scratch for two-pass epilogues when Y == nullptr
    // split-bf16 activation planes (gemm_planes.h): [rows][Cpad/32][hi 32 | lo 32] bf16, 128 B per (row, chunk), the
    // exact LDS row image of the MFMA kernels.  Xp: input planes (same rows as X); xp_scratch: where launch_gemm may
    // build them from X when the producer did not; Yp: output planes (yp_chunks 32-channel chunks per row), written
    // by the epilogue next to / instead of Y.
    const void* Xp; void* xp_scratch; void* Yp; int yp_chunks;
    // fp16 variant of the planes / weight image (same layout, [hi 32 | lo 32] _Float16): the two- and one-term arithmetic of the FFN
    // convolution.  yp_f16: write Yp as fp16 planes; f16_terms: 0 = bf16 arithmetic, else Xp / W are fp16 images and
    // the kernel issues f16_terms MFMAs per fragment pair (3: lo*hi + hi*lo + hi*hi, 2: lo*hi + hi*hi = weights rounded once, 1: hi*hi)
    int yp_f16; int f16_terms;
    // "mx" arithmetic of the FFN convolution (gemm_mx.h): yp_f16 == 2 writes Yp as mx planes with the static scale yp_scale = 2^ka;
    // mx != 0: Xp are mx planes, W the mx weight image (same unit order), mx_scale / mx_scale_b the E8M0 bytes (x 0x01010101) of the
    // A / B side of the scaled MFMA (127 - ka - 11 and 127 - kw)
    float yp_scale; int mx; int mx_scale, mx_scale_b;
    // deterministic split-K (small grids with a long K: the loop is a serial chain of k-steps): workgroup z of grid.z accumulates the
    // 32-channel chunks [z, z+1) * Cpad/32/ksplit (all taps of them); split 0 (which also adds bias + residual) writes Y, split z > 0
    // writes kpart + (z-1) * kpart_stride; the row kernel that follows (ln_rows) adds the partials in a fixed order and applies the
    // whole epilogue (ReLU, LayerNorm, activation, planes)
    int ksplit; float* kpart; size_t kpart_stride;
    size_t kpart_cap;                      // floats available at kpart (launch_gemm picks a split that fits)
    int regime_rows;                       // row count the kernel-variant choice is based on (0: R).  Frame-level launches pass an estimate derived from
                                           // the PHONEME count, which the host knows in both layout modes, so that the host- and the device-driven
                                           // layout of one batch always pick the same variants (-> bit-identical results); see fs2_decode
    // grouped operands (the pitch and the energy predictor as ONE launch per layer, fs2_runtime.hip: run_predictors_fused):
    //   xp_row_chunks: 32-channel chunks per row of the A planes when the GEMM contracts only a slice of them (0: Cpad / 32);
    //   k_groups G > 1: the N outputs form G groups, group g contracts the chunks [g Cpad/32, (g+1) Cpad/32) of the plane row (a grouped conv);
    //   ln_groups G > 1: ReLU / LayerNorm / scalar head apply to each of the G column groups of a row separately (their parameters are
    //   stacked along N); the scalar head of group g goes to dot_out + g dot_gstride and uses dot_b[g]
    int xp_row_chunks, k_groups, ln_groups, dot_gstride;
    int yp_col_off;                        // column offset of this launch's outputs inside the rows of Yp (a layer that fills one group of a stacked plane buffer)
    const int* Rp;                         // device-driven layout: rows actually used (tiles at or beyond round_up(*Rp, 128) exit at once); nullptr: R
    // planes-only residual stream (gemm_row4.h: RES): the residual as the PLANES the producing launch wrote (residp_chunks 32-channel chunks per row;
    // residp_mx != 0: mx planes, whose e4m3 residual words carry the scale 1 / residp_scale = 2^(ka+11)), instead of fp32 rows (resid must then be
    // nullptr); a launch with Y == nullptr and Yp != nullptr writes planes only.  Only gemm_row4_bf16 implements both: launch_gemm refuses otherwise.
    const void* residp; int residp_chunks; int residp_mx; float residp_scale;      // residp_mx: 1 = mx planes (e4m3 residual at byte 2 C + c of the row), 2 = mx4 planes (at 3 C + c)
    // mx4 (gemm_planes.h: ARITH = 3; yp_f16 == 3 / mx == 2): one E8M0 scale byte per ROW of the activation planes (2^-11 folded in) -- written by the
    // producing LayerNorm epilogue (yp_rowscale), read by the conv (x_rowscale) -- and one per output channel of the weight image (w_rowscale)
    unsigned char* yp_rowscale; const unsigned char* x_rowscale; const unsigned char* w_rowscale;
};

}  // namespace fs2
