// Which kernel runs a self-attention launch: the whole decision of fs2_runtime.hip's launch_attention as one pure function, plan_attention().
// HIP-free like gemm_plan.h (whose Options and error codes it uses; layout_rule.h has the work list's block size): tests/test_attn_plan_host.py compiles it with
// the host compiler.  The plan reads integers and the null-ness of pointers, never what they point to; run_attn_plan executes it.
#pragma once
#include <cmath>

#include "gemm_plan.h"
#include "layout_rule.h"

namespace fs2 {

// attn_w32 (32 queries per wave, one wave per SIMD, 128-query workgroups) serves the split-bf16 launches whose grid fills the chip:
// below kW32MinBlocks 128-query blocks per head a 128-query workgroup per CU leaves CUs idle and doubles the serial chain of an
// utterance's key tiles per wave; the 64-query kernel keeps those (token-level launches, single utterances).  The choice is a
// function of the regime row count (fs2_decode: derived from the phoneme count), like every other kernel-variant choice.
constexpr int kW32MinBlocks = 64;

// The question: what the decision reads of a launch.
struct AttnCall {
    int D = 0, heads = 1;        // D = heads x padded head dim
    int dk_true = 0;             // the model's head dim, for the softmax scale (0: the padded one)
    int precision = kPlanFp32;
    int R = 0, Rvt = 0;          // rows; rows of the V^T planes (Rvt % 32 == 0: qkv_split's grid)
    int regime_rows = 0;         // of the call in progress (0: use R): derived from the phoneme count, the same in the host- and the device-driven layout, whose R differ
    int nwork = 0;               // work-list items (device-driven layout: their capacity)
    bool qkv_rows = false;       // fp32 QKV rows are given: the bf16 kernels need the split pass first (else the projection has left the operands)
    long long qk_lo_dist = 0, vt_lo_dist = 0;      // signed byte distance from the hi plane to the lo plane of Q|K and of V^T
};

// The answer.
enum class AttnKernel { None, F32, B16, W32 };      // attn_f32<dk>, attn_bf16<dk, nsplit>, attn_w32<dk>
struct AttnPlan {
    AttnKernel kernel = AttnKernel::None;      // None without err: nothing to launch
    int dk = 0, nsplit = 0;                    // padded head dim; MFMA terms (B16 only: 3 split-bf16, 1 bf16)
    unsigned grid_x = 0, grid_y = 0;
    bool split_pass = false;                   // qkv_split runs first
    float softmax_scale = 0.f;                 // of the kernel that will run: 1/sqrt(d_k) (F32), log2(e)/sqrt(d_k) (the others: softmax in base 2, applied where Q is split)
    int err = 0; const char* msg = nullptr; int m0 = 0;      // err != 0: refused -- an FS2_ERR_* code and the printf format of its message (argument: m0)
};

inline bool att_head_dim(int dk) { return dk == 128 || dk == 192 || dk == 64 || dk == 256; }
// the lo planes must sit within 2 GB behind the hi planes (attn_w32: 32-bit DMA offsets)
inline bool w32_reaches(long long lo_dist) { return lo_dist > 0 && lo_dist < (1LL << 31); }

inline AttnPlan plan_attention(const AttnCall& c, const Options& o) {
    AttnPlan p;
    if (c.nwork == 0) return p;
    auto refused = [&](const char* msg, int m0) { p.err = kPlanErrUnsupported; p.msg = msg; p.m0 = m0; return p; };
    const bool f32 = c.precision == kPlanFp32, x3 = c.precision == kPlanBf16x3;
    const int dk = c.D / c.heads;
    if (!f32 && c.qkv_rows && c.D > 1024) return refused("attention dim %d > 1024", c.D);      // (qkv_split transposes a [32][D + 1] fp32 tile through LDS)
    if (!att_head_dim(dk)) return refused("attention head dim %d not in {64,128,192,256} (the model path pads other head dims)", dk);
    p.dk = dk; p.grid_y = (unsigned)c.heads; p.split_pass = !f32 && c.qkv_rows;
    p.softmax_scale = (f32 ? 1.0f : 1.4426950408889634f) / sqrtf((float)(c.dk_true ? c.dk_true : dk));
    if (f32) {
        p.kernel = AttnKernel::F32;
    } else if (x3 && (dk == 128 || dk == 192) && w32_reaches(c.qk_lo_dist) && w32_reaches(c.vt_lo_dist) &&
               (o.w32 >= 0 ? o.w32 != 0 : att_blocks(c.regime_rows > 0 ? c.regime_rows : c.R) >= kW32MinBlocks)) {
        p.kernel = AttnKernel::W32;
    } else {
        p.kernel = AttnKernel::B16; p.nsplit = x3 ? 3 : 1;
    }
    p.grid_x = p.kernel == AttnKernel::W32 ? (unsigned)c.nwork : att_grid64(c.nwork);      // one 128-query workgroup / two 64-query workgroups per work item
    return p;
}

}  // namespace fs2
