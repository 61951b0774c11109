// Which kernel runs a dense layer: the whole decision of fs2_runtime.hip's launch_gemm as one pure function, plan_gemm(), and the rules it is made of.
// HIP-free (gemm_args.h + the standard library): tests/test_gemm_plan_host.py compiles this file with the host compiler.  The plan reads integers and the
// null-ness of pointers, never what they point to; launch_gemm executes it.
#pragma once
#include <algorithm>

#include "gemm_args.h"

namespace fs2 {

// Values of include/fs2.h and of the kernel headers that the plan needs (fs2_runtime.hip static_asserts that they agree).
constexpr int kPlanErrArg = -1, kPlanErrHip = -2, kPlanErrState = -3, kPlanErrUnsupported = -6;
constexpr int kPlanFp32 = 0, kPlanBf16x3 = 1;      // FS2_PREC_FP32 / FS2_PREC_BF16X3 (every other precision reaching the plan is plain bf16)
constexpr int kPlanMaxHalo = 16;                   // kMaxHalo
constexpr int kPlanBN = 128;                       // kB16BN: columns of a gemm_pl_bf16 tile

// A/B switches of the kernel choice.  Read from the environment ONCE, when the library is first used, and
// changed afterwards only through fs2_set_option(): the launch path never touches the environment.  -1 = automatic choice.
struct Options {
    int bm = -1;         // FS2_BM       tile height of gemm_pl_bf16 (64 | 128 | 256)
    int bal = 0;         // FS2_BAL      tall conv tiles: 0 = always 256 rows (default: interleaved A/B, profiles/r03_ab_conv_tile_balance.txt), 1 = height balanced over
                         //              whole rounds of the rows in use, 2 = of the row capacity
    int row8 = -1;       // FS2_ROW8     force (1) / forbid (0) the row-complete LayerNorm-fused k = 1 GEMM
    int qkv8 = -1;       // FS2_QKV8     force / forbid the 8-wave fused QKV projection
    int nosplitk = 0;    // FS2_NOSPLITK no split-K of the token-level k = 1 GEMMs
    int f32_rows = 0;    // FS2_F32_ROWS row-complete fp32 GEMM for LayerNorm-terminated ops
    int fuse_var = 1;    // FS2_FUSE_VAR the pitch and the energy predictor as one launch per layer (0: separate launches)
    int mt8 = -1;        // FS2_MT8      m-tiles per wave of the 8-wave row-complete kernels (2 | 3: 128 / 192-row workgroups)
    int op_att_planes = 0;   // FS2_OP_ATT_PLANES  fs2_op_attention (split-bf16 modes) takes the context from the kernels as planes, the model's form, and converts (tests)
    int qkv_split = -1;  // FS2_QKV_SPLIT  the Q, K and V passes of gemm_qkv8_bf16 as three workgroups per row tile (-1: by the round count)
    int w32 = -1;        // FS2_ATTN_W32 split-bf16 attention with 32 queries per wave (attn_w32.h): 0 never, 1 whenever the head dim allows, -1 by regime
    int row4 = -1;       // FS2_ROW4     the one-wave-per-SIMD row-complete kernel (gemm_row4.h) wherever gemm_row8_bf16 would run and it has the epilogue: 0 never, else yes
    int mt4 = -1;        // FS2_MT4      its m-tiles per wave (4 | 5: 128 / 160-row workgroups; -1: by the round count)
    int qkv4 = -1;       // FS2_QKV4     the fused QKV projection's passes on gemm_row4_bf16 (EPI 3) wherever gemm_qkv8_bf16 would run at D = 384: 0 never, else yes
    int ffn2_mx = 1;     // FS2_FFN2_MX  mix_mx mode: the second FFN GEMM in the mx arithmetic too, wherever gemm_row4_bf16 runs it (0: split-bf16 as in round 4)
    int post_mx = 1;     // FS2_POST_MX  mixed modes: the Postnet's 512 -> 512 convolutions in the mx arithmetic (0: split-bf16 as until round 5)
    int tokproj = 3;     // FS2_TOKPROJ  multiply before expanding (non-fp32 precisions): bit 0 = the predictors' first convolution (where the fused predictors run), bit 1 = the
                         //              decoder input layer from token-level products (tok.proj + var.gather0 / dec.in.gather); 0 = the frame-level launches.  Never a function of the batch.
    int tokproj_f32 = 0; // FS2_TOKPROJ_F32  tok.proj on the exact fp32 GEMM instead of the precision's own arithmetic
    int varshort = 1;    // FS2_VARSHORT  the fused variance predictors on at most K frames per phoneme (layout_rule.h; where FS2_TOKPROJ = 3 holds and the batch
                         //               has per-utterance semantics): 0 = on every frame.  Never a function of the batch.
};

// ------------------------------------------------------------------ the rules
// Split-K serves small batches (regime_rows <= kSplitRegime: beyond, the grids fill the chip anyway).  Its scratch holds up to 4 slabs of
// kSplitRows x 1024 floats, enough for every launch with R <= kSplitRows, so that the decision is a function of regime_rows alone (the same
// in the host- and the device-driven layout) as long as the row capacity stays below twice the estimate.
constexpr int kSplitRegime = 8192, kSplitRows = 16384;
constexpr int kCus = 256;

// The row kernels (one workgroup per CU) need about a CU's worth of 128-row tiles to pay; forced: the FS2_ROW8 / FS2_QKV8 switch (-1: by the row count).
inline bool row_regime(long regime_rows, int forced) { return forced >= 0 ? forced != 0 : (regime_rows + 127) / 128 >= 128; }

// Rows a launch will really touch: in the device-driven layout a.R is a capacity (15-25 % above the rows in use, the surplus tiles exit at once);
// the regime estimate (8 frames per phoneme + alignment rows, the same number in both layout modes) is the better basis for balancing rounds.
inline long rows_in_use(const GemmArgs& a, long rows) { return a.regime_rows > 0 ? std::min<long>(rows, a.regime_rows) : rows; }

// Tile height of the 8-wave row-complete kernels (one workgroup per CU): 64 MT rows, MT = 2 or 3.  A launch of T tiles takes ceil(T / #CUs)
// rounds, and a nearly empty second round costs as much as a full one (c3 at 7.87 frames per phoneme: 286 tiles of 128 rows = 256 + 30).
// Same-box A/B: a 192-row tile costs 1.55-1.9 x a 128-row one (its epilogue spills), so it pays exactly when it turns two rounds into one
// (c3: dec.ffn2_ln 0.174 -> 0.134 ms, step 5.68 -> 5.34 ms; c4, 15 rounds against 10: 68.0 -> 70.8 ms, so not there).  Results do not depend on MT.
// wgs: workgroups per row tile (the grouped convolution's grid.y).  The rule above counts tiles; a grouped launch whose tiles fit one round while its workgroups do
// not is in the same position one step earlier -- the fused predictors' second layer on the short rows of FS2_VARSHORT at c3: 175 tiles x 2 groups = 350 workgroups of 128
// rows against 117 x 2 = 234 of 192 rows; same-box, one stream: 0.092 against 0.070 ms -- and takes the taller tile too.
inline int row8_mt(long rows, int wgs = 1) {
    const long t128 = (rows + 127) / 128, t192 = (rows + 191) / 192;
    if (t128 > kCus && t192 <= kCus) return 3;
    return (wgs > 1 && t128 * wgs > kCus && t192 * wgs <= kCus) ? 3 : 2;
}

// gemm_row4_bf16 (gemm_row4.h): one wave per SIMD, 128- or 160-row workgroups, one per CU.  The tile height that minimises rounds x height
// (ties: the taller tile -- fewer weight bytes per row): c3 (36.6 k rows) 160 rows = 229 workgroups in one round, the c5 shard (78 k rows) 160 rows =
// 2 rounds instead of 3, c4 either.  Results do not depend on the height (nor on the kernel: bit-identical to gemm_row8_bf16).
inline int row4_mt(long rows) {
    const long r4 = ((rows + 127) / 128 + kCus - 1) / kCus * 128, r5 = ((rows + 159) / 160 + kCus - 1) / kCus * 160;
    return r5 <= r4 ? 5 : 4;
}
// the epilogues it has (gemm_row4.h: EPI); -1: none, the launch stays on gemm_row8_bf16.  Since round 6 the kernel serves the PLANES-ONLY form of
// these launches only (gemm_row4.h: RES): no fp32 rows out (Y == nullptr, Yp given), the residual -- where there is one -- as the producing launch's
// planes (residp; resid == nullptr).  model_launches.h forms the decoder's launches in that form exactly when the plans of its
// LayerNorm-fused launches land here (planes_only); a launch in the other form stays on gemm_row8_bf16.
inline int row4_epi(const GemmArgs& a) {
    if (a.ktaps != 1 || a.N != 384 || !a.ln_g || a.Y || !a.Yp || a.resid || a.relu_pre || a.dot_w || a.k_groups > 1 || a.ln_groups > 1 || a.qk_hi || a.yp_col_off) return -1;
    if (a.Cpad % 64 != 0 || a.yp_chunks * 32 != a.N) return -1;      // an even number of k-steps; planes exactly N wide
    if (a.residp && a.residp_chunks * 32 != a.N) return -1;
    if (a.pe) return (a.act_post == 1 && a.yp_f16 == 0 && !a.residp) ? 2 : -1;
    if (a.act_post != 0 || !a.residp) return -1;
    if (a.yp_f16 == 2) return a.residp_mx ? -1 : 1;      // out-proj + LN1 of mix_mx: residual = split-bf16 planes of the block input, result = mx planes
    if (a.yp_f16 == 3) return (a.residp_mx || !a.yp_rowscale) ? -1 : 4;      // ... of mix_mx4: result = mx4 planes + one scale byte per row
    return a.yp_f16 == 0 ? 0 : -1;
}

// The Q, K and V passes of a row tile are independent (each re-streams the A tile): as three workgroups per tile (grid.y = 3) the
// unit of work is a third of a tile and the last, partly filled round of a launch costs a third.  Rounds in units of a 128-row
// tile's three passes, a 192-row tile at 1.7 (row8_mt): c3, 286 tiles of 128 rows: whole tiles 2.0 (128) / 1.7 (192, one round
// on 191 of 256 CUs: what ran until round 4), passes apart 4/3 (128) / 1.7 (192).  Never more rounds than whole tiles of the
// same height.  Results do not depend on either choice.
inline void qkv8_plan(long rows, const Options& o, int& mt, int& apart) {
    double best = 1e30;
    for (int m = 2; m <= 3; ++m)
        for (int ap = 0; ap <= 1; ++ap) {
            if (o.mt8 > 0 && m != std::min(std::max(o.mt8, 2), 3)) continue;
            if (o.qkv_split >= 0 && ap != (o.qkv_split != 0)) continue;
            const long tiles = (rows + 64 * m - 1) / (64 * m), units = ap ? 3 * tiles : tiles;
            const double cost = (double)((units + kCus - 1) / kCus) / (ap ? 3.0 : 1.0) * (m == 3 ? 1.7 : 1.0);
            if (cost < best - 1e-9) { best = cost; mt = m; apart = ap; }
        }
}

// The fused QKV projection's passes on the one-wave-per-SIMD structure (gemm_row4.h, EPI 3): always one workgroup per (row tile, pass); the tile height that
// minimises rounds x height of the 3 T pass-workgroups (c3: 160 rows = 687 units = 2.7 rounds against 858 = 3.4 rounds of 128 rows).  Bit-identical to gemm_qkv8_bf16.
inline int qkv4_mt(long rows) {
    const long r4 = (3 * ((rows + 127) / 128) + kCus - 1) / kCus * 128, r5 = (3 * ((rows + 159) / 160) + kCus - 1) / kCus * 160;
    return r5 <= r4 ? 5 : 4;
}

// Fused QKV projection on the 8-wave structure when there is about a CU's worth of 128-row tiles (FS2_QKV8=0|1 forces the choice)
inline bool use_qkv8(const GemmArgs& a, const Options& o) {
    if (!a.qk_hi || a.ktaps != 1 || (a.att_D != 256 && a.att_D != 384) || a.N != 3 * a.att_D) return false;
    return row_regime(a.regime_rows ? a.regime_rows : a.Rvt, o.qkv8);
}

// Row-complete LN-fused kernel (gemm_row8_bf16) for k = 1 GEMMs that end in a row epilogue: one workgroup per CU, so it
// needs about a CU's worth of 128-row tiles to pay (FS2_ROW8=0|1 forces the choice).
inline bool use_row8(const GemmArgs& a, const Options& o) {
    const int Ng = a.k_groups > 1 ? a.N / a.k_groups : a.N;      // (grouped conv: one workgroup row per group, gemm_row8c_bf16's grid.y)
    const bool two_ln_groups = a.ln_groups == 2 && a.k_groups <= 1 && a.N == 512 && a.ktaps > 1;      // two stacked 256-channel layers over one input
    if (a.qk_hi || (!two_ln_groups && Ng != 256 && Ng != 384)) return false;
    if (a.ln_groups > 1 && !two_ln_groups && a.ln_groups != a.k_groups) return false;
    if (a.ktaps > 1) {      // conv form (gemm_row8c_bf16): LayerNorm-terminated convolutions, optionally with the scalar head; no PE
        if (!a.ln_g || a.pe || a.f16_terms) return false;
    } else if (a.dot_w || !(a.ln_g || a.pe) || a.k_groups > 1 || a.ln_groups > 1) return false;
    return row_regime(a.regime_rows ? a.regime_rows : a.R, o.row8);
}

// In the 256-row regime the conv kernel runs two workgroups per CU: a launch of T y-tiles per N tile takes ceil(T nN / 512) rounds, and a nearly
// empty last round costs as much as a full one (c3 at 7.87 frames per phoneme: 143 x 8 tiles = 2.2 rounds -> 3).  The smallest tile height (a
// multiple of 32 rows, 160 .. 256) that keeps that number of rounds spreads the rows evenly instead (191 tiles of 192 rows: 3 full rounds of
// tiles that are a quarter shorter).  Results do not depend on the tile height.
inline int conv_bm_balanced(long rows, long nN) {
    const long ypr = std::max<long>(1, 2 * kCus / nN);
    const long rounds = std::max<long>(1, (rows + 256 * ypr - 1) / (256 * ypr));
    const long h = (rows + rounds * ypr - 1) / (rounds * ypr);
    return (int)std::min<long>(256, std::max<long>(160, (h + 31) / 32 * 32));
}
// Tile height of a convolution on gemm_pl_bf16: FS2_BM if set, else by how many tiles the launch has; snapped to the heights the arithmetic is built at.
// arith (gemm_planes.h: ARITH) 0 = split-bf16 (NSPLIT 3: the four tall heights, balanced under FS2_BAL unless split-K runs; NSPLIT 1: 256), 1 = fp16 terms
// (64 | 128 | 256, never balanced), 2 = mx (the four tall heights, balanced under FS2_BAL).
inline int conv_bm(const GemmArgs& a, int arith, int nsplit, int ksplit, const Options& o) {
    const int force = o.bm > 0 ? o.bm : 0;
    const long rows = a.R, nN = (a.N + kPlanBN - 1) / kPlanBN;
    int bm = force ? force : (nN * ((rows + 255) / 256) >= 512 ? 256 : (nN * ((rows + 127) / 128) >= 400 ? 128 : 64));
    if (arith == 1) return bm == 256 ? 256 : (bm == 128 ? 128 : 64);
    if (bm <= 128) return bm == 128 ? 128 : 64;
    if (arith == 0 && nsplit != 3) return 256;
    if (!force && o.bal && (arith == 2 || ksplit <= 1)) bm = conv_bm_balanced(o.bal == 2 ? rows : rows_in_use(a, rows), nN);
    return bm <= 160 ? 160 : (bm <= 192 ? 192 : (bm <= 224 ? 224 : 256));
}

// split-K: on a grid that leaves most CUs idle the kernel is a serial chain of k-steps (one utterance: 108 steps of the FFN
// conv on 88 workgroups); 2-4 workgroups share the chunks and ln_rows adds their partial sums in a fixed order
// (deterministic, unlike atomics) and applies the epilogue.  The choice depends on regime_rows (the same number in the host-
// and the device-driven layout), never on the capacity.  own_y: the split-0 rows have a buffer of their own (row stride ld), else they take a slab of kpart too.
inline int pick_ksplit(const GemmArgs& a, long rr, int max_extra_splits, bool own_y, size_t ld) {
    const int nchunks = a.Cpad / 32;
    const long wgs = (long)((a.N + kPlanBN - 1) / kPlanBN) * ((rr + 63) / 64);
    for (int cand = 4; cand >= 2; --cand)
        if (nchunks % cand == 0 && (nchunks / cand) * a.ktaps >= 4 && wgs * cand <= 1024 && cand - 1 <= max_extra_splits &&
            (size_t)(cand - (own_y ? 1 : 0)) * a.R * ld <= a.kpart_cap) return cand;
    return 1;
}

inline bool rows_supported(int N) { return N == 80 || N == 256 || N == 384; }

// ------------------------------------------------------------------ the plan
enum class GemmKernel {
    None,
    RowsF32,          // gemm_rows_f32<nb>: fp32 row-complete (epilogue in the kernel)
    TileF32,          // gemm_tile_f32
    TileRowsF32,      // gemm_tile_f32 + ln_rows
    PlBf16,           // gemm_pl_bf16<nsplit, bm, k1, 0>: split-bf16 (nsplit 3) / bf16 (1) tiles
    PlF16,            // gemm_pl_bf16<nsplit, bm, false, 1>: fp16 operands, nsplit terms
    PlMx,             // gemm_pl_bf16<1, bm, false, 2>: fp16 + block-scaled fp8
    PlMx4,            // gemm_pl_bf16<1, 256, false, 3>: fp16 + block-scaled fp4
    Row8,             // gemm_row8_bf16<nsplit, nb, mt>
    Row8c,            // gemm_row8c_bf16<nsplit, nb, mt>: LayerNorm-terminated convolution
    Row8cGrouped,     // ... grouped: one workgroup row per group (grid.y), launched with N = one group's outputs
    Row8cTwoLn,       // gemm_row8c_bf16<nsplit, 4, 2, 2>: two stacked 256-channel layers over one input
    Row4,             // gemm_row4_bf16<3, 3, mt, epi, 2, arith, res>
    Qkv8,             // gemm_qkv8_bf16<nsplit, nb, mt, apart>
    Qkv4,             // gemm_row4_bf16<3, 3, mt, 3, 2, 0>: the QKV passes
};
enum class RowsOut { None, Y, Scratch, KpartSlab };      // where the launch's fp32 rows go: nowhere, the caller's Y, a.scratch, the first slab of a.kpart

struct GemmPlan {
    GemmKernel kernel = GemmKernel::None;
    int nsplit = 0, nb = 0;      // MFMA terms; N-tiles per wave of the row kernels (gemm_rows_f32: its NT)
    int bm = 0, mt = 0;          // tile height: rows of gemm_pl_bf16 / m-tiles per wave of the row kernels (64 mt rows on 8 waves, 32 mt on gemm_row4_bf16)
    bool k1 = false;             // gemm_pl_bf16's k = 1 form
    int apart = 0, epi = -1, arith = 0, res = 0;
    int ksplit = 1;
    RowsOut y = RowsOut::None;
    bool build_planes = false;   // the A operand is converted into a.xp_scratch first (to_planes)
    bool rows_pass = false;      // ln_rows follows: adds the split-K partials and / or applies the row epilogue and writes the planes
    int err = 0;                 // != 0: refused -- an FS2_ERR_* code and the printf format of its message (arguments: the launch's name, m0, m1)
    const char* msg = nullptr;
    int m0 = 0, m1 = 0;
    int tile_rows() const { return bm ? bm : (kernel == GemmKernel::Row4 || kernel == GemmKernel::Qkv4 ? 32 : 64) * mt; }
};
inline GemmPlan refused(int err, const char* msg, int m0 = 0, int m1 = 0) {
    GemmPlan p;
    p.err = err; p.msg = msg; p.m0 = m0; p.m1 = m1;
    return p;
}

// Picks the kernel.  fp32: row-complete tiles when the epilogue needs whole rows and N is small, 128x128 tiles (+ ln_rows) otherwise.
// bf16 / bf16x3 (activation planes in, gemm_planes.h): the row-complete LayerNorm-fused kernel for big k = 1 GEMMs that end in
// a row epilogue, else the BM x 128 tile kernel followed by ln_rows when a row epilogue is needed.
// a: the launch as the caller formed it, the handle's defaults applied; a.ksplit = how many split-K partial buffers the caller allows.
inline GemmPlan plan_gemm(const GemmArgs& a, int precision, const Options& o) {
    if (a.ktaps - 1 > kPlanMaxHalo) return refused(kPlanErrUnsupported, "%s: kernel size %d > %d", a.ktaps, kPlanMaxHalo + 1);
    if (a.C % 4 != 0 || a.ldx % 4 != 0) return refused(kPlanErrUnsupported, "%s: channels %d / ld %d must be multiples of 4", a.C, a.ldx);
    const bool need_rows = a.ln_g || a.dot_w || a.pe;
    GemmPlan p;
    if (precision == kPlanFp32) {
        if (need_rows && a.N >= 128 && a.N <= 1024 && a.N % 4 == 0 && (a.Y || a.scratch) && !o.f32_rows) {
            // fp32, LayerNorm-terminated: 128x128 MFMA tiles + the HBM-bound row kernel (2x faster than the row-complete
            // GEMM, whose 16-rows-per-wave shape re-stages the whole weight matrix for every 64 rows)
            p.kernel = GemmKernel::TileRowsF32; p.rows_pass = true;
            p.y = a.Y ? RowsOut::Y : RowsOut::Scratch;
        } else if (need_rows || (a.N < 128 && rows_supported(a.N))) {
            if (!rows_supported(a.N)) return refused(kPlanErrUnsupported, "%s: row-epilogue GEMM needs N in {80,256,384}, got %d", a.N);
            p.kernel = GemmKernel::RowsF32; p.nb = a.N == 80 ? 5 : (a.N == 256 ? 16 : 24);
            p.y = a.Y ? RowsOut::Y : RowsOut::None;
        } else {
            p.kernel = GemmKernel::TileF32; p.y = RowsOut::Y;
        }
        return p;
    }
    if (!a.Wb) return refused(kPlanErrState, "%s: no bf16 weight image");
    if (a.C % 8 != 0 || a.N % 4 != 0 || (need_rows && a.N > 1024)) return refused(kPlanErrUnsupported, "%s: bf16 path needs C %% 8 == 0, N %% 4 == 0 (N <= 1024 with a row epilogue)");
    // the A operand must exist as split-bf16 planes (Xp) or be convertible into xp_scratch (gemm_planes.h)
    if (!a.Xp && !a.xp_scratch) return refused(kPlanErrState, "%s: no activation planes and no scratch to build them");
    if (a.ldy % 4 != 0 || (a.resid && a.ldr % 4 != 0)) return refused(kPlanErrUnsupported, "%s: bf16 path needs row strides that are multiples of 4");
    const bool x3 = precision == kPlanBf16x3;
    const bool row8 = use_row8(a, o);
    const int epi = (row8 && x3 && o.row4 != 0) ? row4_epi(a) : -1;      // >= 0: this launch belongs to gemm_row4_bf16
    if ((a.residp || (need_rows && !a.Y && a.Yp && !a.dot_w && a.ktaps == 1 && !a.scratch)) && epi < 0)
        return refused(kPlanErrState, "%s: a planes-only launch (residual as planes / no fp32 rows) exists on gemm_row4_bf16 only and this one would not run there");
    if (a.yp_col_off && !(row8 && a.ktaps > 1)) return refused(kPlanErrUnsupported, "%s: a plane column offset exists in the row-complete conv kernel only");
    // (the slice at offset 0 of such a buffer carries no offset to tell it by: every other kernel zero-pads the plane rows to yp_chunks chunks and would wipe the slices behind it)
    if (a.Yp && a.yp_chunks * 32 >= a.N + 32 && !(row8 && a.ktaps > 1))
        return refused(kPlanErrUnsupported, "%s: planes %d columns wide from a launch of %d: filling a slice of a plane row exists in the row-complete conv kernel only", a.yp_chunks * 32, a.N);
    const bool y_needed = (need_rows && !row8) || (!a.Yp && !a.qk_hi && !(row8 && a.dot_w));      // (row-complete + scalar head: nothing but dot_out leaves)
    p.y = a.Y ? RowsOut::Y : ((y_needed && a.scratch) ? RowsOut::Scratch : RowsOut::None);
    if (y_needed && p.y == RowsOut::None) return refused(kPlanErrArg, "%s: no output or scratch buffer");
    if (a.qk_hi && (a.ktaps != 1 || a.att_D % kPlanBN != 0 || a.N != 3 * a.att_D)) return refused(kPlanErrUnsupported, "%s: fused QKV split needs D %% 128 == 0");
    const long rr = a.regime_rows ? a.regime_rows : a.R;
    if (!row8 && !a.qk_hi && a.kpart && !o.nosplitk && a.N <= 1024 && rr <= kSplitRegime && a.R <= kSplitRows && a.mx != 2) {      // (the mx4 conv walks 9 units per row, not Cpad / 32: it exists unsplit -- its regime never splits unless the row kernels are forced on a small batch)
        const bool own_y = p.y != RowsOut::None;
        p.ksplit = pick_ksplit(a, rr, a.ksplit, own_y, p.y == RowsOut::Y ? (size_t)a.ldy : (size_t)a.N);
        if (p.ksplit > 1 && !own_y) p.y = RowsOut::KpartSlab;
    }
    p.rows_pass = (need_rows && !row8) || p.ksplit > 1;
    const bool mx_row4 = a.mx && a.ktaps == 1 && epi == 0 && a.Cpad % 128 == 0 && a.Xp;      // FFN2 + LN2 in the mx arithmetic (gemm_row4.h)
    if ((a.f16_terms || a.mx) && !mx_row4 && (a.ktaps == 1 || need_rows || a.qk_hi)) return refused(kPlanErrUnsupported, "%s: the fp16 arithmetic exists for plain convolutions only");
    if (a.mx && !mx_row4 && (a.ktaps < 3 || a.C % 128 != 0 || a.N % 128 != 0)) return refused(kPlanErrUnsupported, "%s: the mx arithmetic needs a convolution with C %% 128 == 0 and N %% 128 == 0");
    if (a.mx == 2 && (!a.x_rowscale || !a.w_rowscale || !a.Xp || p.ksplit > 1)) return refused(kPlanErrState, "%s: the mx4 arithmetic needs mx4 planes with their row scales and the weight image's channel scales");
    p.build_planes = !a.Xp;
    p.nsplit = x3 ? 3 : 1;
    const int mt8 = (o.mt8 > 0 ? o.mt8 : row8_mt(rows_in_use(a, a.R), a.k_groups > 1 ? a.k_groups : 1)) >= 3 ? 3 : 2;
    const bool force_mt4 = o.mt4 == 4 || o.mt4 == 5;
    if (mx_row4 || epi >= 0) {
        // The instantiations the library holds (fastspeech2_amd/_audit.py: EXPECTED_KERNELS counts them): EPI 0 x {split-bf16 arithmetic with the residual from
        // split-bf16 or from mx planes, mx arithmetic with the residual from mx planes}, EPI 1 and EPI 4 (residual from split-bf16 planes), EPI 2 (no residual),
        // each at two tile heights, + the QKV passes.
        // (This refusal and the mx4 one below were launchers returning hipErrorInvalidValue, which launch_gemm reported as FS2_ERR_HIP with hipGetErrorString's
        //  text.  They keep that code and text, written out here because this header has no HIP: if the runtime's wording for that error changes, these two
        //  messages keep the old one.  to_planes is no longer launched before them.)
        if (a.mx && !a.residp_mx) return refused(kPlanErrHip, "%s launch: invalid argument");      // (FFN2 in the mx arithmetic exists in mix_mx only, where LN1's output is mx planes)
        p.kernel = GemmKernel::Row4; p.epi = epi; p.arith = a.mx ? 2 : 0;
        p.res = epi == 2 ? 3 : ((epi == 0 && a.residp_mx) ? 2 : 1);
        p.mt = force_mt4 ? o.mt4 : row4_mt(rows_in_use(a, a.R));
    } else if (a.mx == 2) {
        // fp16 + block-scaled-fp4 form of the conv (gemm_planes.h ARITH = 3): 256-row tiles only -- it runs where the planes-only regime holds (>= 16 k rows: the
        // tile-height rule picks 256 there for every N >= 1024)
        if (a.Cpad != 384) return refused(kPlanErrHip, "%s launch: invalid argument");      // (the LDS stride of the row scales is a compile-time constant: 8 bytes x 3 cross units; block_steps offers mx4 at D = 384 only)
        p.kernel = GemmKernel::PlMx4; p.nsplit = 1; p.arith = 3; p.bm = 256;
    } else if (a.mx) {      // fp16 + block-scaled-fp8 form of the conv (gemm_mx.h): the planes kernel on mx planes / the mx weight image
        p.kernel = GemmKernel::PlMx; p.nsplit = 1; p.arith = 2; p.bm = conv_bm(a, 2, 1, p.ksplit, o);
    } else if (a.f16_terms) {      // fp16-operand form of the conv kernel (FFN w_1 in the mixed modes): nsplit MFMAs per fragment pair
        p.kernel = GemmKernel::PlF16; p.nsplit = a.f16_terms == 3 ? 3 : (a.f16_terms == 2 ? 2 : 1); p.arith = 1; p.bm = conv_bm(a, 1, p.nsplit, p.ksplit, o);
    } else if (use_qkv8(a, o)) {
        if (x3 && o.qkv4 != 0 && o.row4 != 0 && a.att_D == 384 && a.Cpad % 64 == 0) {
            p.kernel = GemmKernel::Qkv4; p.epi = 3; p.mt = force_mt4 ? o.mt4 : qkv4_mt(rows_in_use(a, a.Rvt));
        } else {
            p.kernel = GemmKernel::Qkv8; p.nb = a.att_D == 384 ? 3 : 2; p.mt = 2;
            qkv8_plan(rows_in_use(a, a.Rvt), o, p.mt, p.apart);
        }
    } else if (row8 && a.ktaps > 1 && a.ln_groups == 2 && a.k_groups <= 1) {      // two stacked layers over one input: N = 512, LayerNorm per N-wave
        p.kernel = GemmKernel::Row8cTwoLn; p.nb = 4; p.mt = 2;
    } else if (row8 && a.ktaps > 1) {
        p.kernel = a.k_groups > 1 ? GemmKernel::Row8cGrouped : GemmKernel::Row8c;
        p.nb = (a.k_groups > 1 ? a.N / a.k_groups : a.N) == 384 ? 3 : 2; p.mt = mt8;
    } else if (row8) {
        p.kernel = GemmKernel::Row8; p.nb = a.N == 384 ? 3 : 2; p.mt = mt8;
    } else {
        p.kernel = GemmKernel::PlBf16; p.k1 = a.ktaps == 1;
        p.bm = p.k1 ? (o.bm == 128 ? 128 : 64)      // measured (c3): 64-row tiles win for every k = 1 GEMM (3 workgroups/CU hide the DMA round trips)
                    : conv_bm(a, 0, p.nsplit, p.ksplit, o);
    }
    return p;
}

}  // namespace fs2
