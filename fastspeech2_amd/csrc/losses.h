// The loss terms of the teacher-forced forward, per utterance: what the reference's FeedForwardTransformer.forward() (fastspeech.py:280-333)
// and its evaluation.py (12-41) reduce the model's outputs and the targets to, behind fs2_op_loss_terms (include/fs2.h; DESIGN.md section
// 14.5; tests/losses_oracle.py states the same in numpy).  Not a header of its own: fs2_runtime.hip includes it inside its unnamed namespace,
// after targets.h (tg_wave_sum), fail() and align_up().  Plain HIP C++, restricted to what tests/kernel_standin/hip_standin.h provides.
//
// The definition: every difference is formed in double from the float32 / int64 inputs (so it is exact), |.|, the square and
// log((double)ds + 1.0) are taken in double (nothing is contracted into a fused multiply-add), and the sums are carried in double and
// reduced in a fixed order -- no floating-point atomics.  Per utterance a record of FS2_LOSS_TERMS doubles (include/fs2.h lists it).
//
// lt_terms: one workgroup of 256 threads per TILE of kLtFrames frames of one utterance; an utterance of olen frames has
// max(1, ceil(olen / kLtFrames)) tiles (uploaded with its record by record_op.h's upload_recs: kernel arguments, no copy).  The
// rows of an utterance lie back to back, so a tile's part of before / after / ys is one run of floats each, read once:
//   thread t takes the quads t, t + 256, ... of the run (a quad's four values in order; 16-byte loads where the run starts on a 16-byte
//   boundary, four 4-byte loads otherwise -- the same values in the same order, so the path changes no bit), then thread t < n % 4 takes
//   tail value t; the xor butterfly of tg_wave_sum; the four waves in order.
// The tile that owns frames [f0, f1) also owns those entries of e / p (thread t: frames f0 + t, + 256, ...); tile 0 owns the tokens.
// Nothing in that order depends on B, on the utterance's place in the batch, on a stride or on Lmax: the sums over [0, len) are a
// function of the utterance's own values.  With pads != 0 the pad frames [olen, Lmax) are shared out in equal runs over the utterance's
// tiles (tile 0 also takes the pad tokens [ilen, Tmax)) and summed apart from the valid ones; with pads == 0 nothing outside [0, len) is
// read.  lt_combine (one workgroup) folds the tiles of each utterance in index order into its record and the B records into the batch
// record: thread t takes utterances t, t + 256, ... in order, then lane l takes lane l + o for o = 32 .. 1, then the four waves in order.

#include "record_op.h"
constexpr int kLtThreads = 256;
constexpr int kLtFrames = 32;             // frames of a tile (odim = 80: 10 KB of each of before / after / ys)
constexpr int kLtRecsPerChunk = 250;      // records per upload launch (kernel-argument bytes: 250 * 16 + 8 < 4 KB)
constexpr int kLtTerms = FS2_LOSS_TERMS;  // doubles of a record
constexpr int kLtSums = 13;               // sums of a tile: the record's indices 4 .. 16
constexpr int kLtValidSums = 8;           // ... of which the first 8 (indices 4 .. 11) run over [0, len)
constexpr int kLtPartial = 16;            // doubles of a tile's partial (128 bytes)
static_assert(FS2_LOSS_TERMS == 20 && 4 + kLtSums <= FS2_LOSS_TERMS, "record layout of include/fs2.h");

// s[j] of a tile is index 4 + j of the record
enum { kLtBefore = 0, kLtAfter, kLtDurSq, kLtEnergySq, kLtPitchSq, kLtDurAbs, kLtEnergyAbs, kLtPitchAbs,
       kLtPadBefore, kLtPadAfter, kLtPadDurSq, kLtPadEnergySq, kLtPadPitchSq };

struct LtRec { int ilen, olen, tile0, ntiles; };

struct LtArgs {
    const float *before, *after, *ys, *d_outs;
    const int64_t* ds;
    const float *e_outs, *es, *p_outs, *ps;
    int64_t pred_stride_f, y_stride_f, pred_stride_t, ds_stride_t, tgt_stride_f;
    int odim, B, Tmax, Lmax, pads;
};

struct alignas(16) LtQuad { float x, y, z, w; };

__device__ inline bool lt_aligned16(const float* p) { return ((uintptr_t)p & 15) == 0; }
__device__ inline LtQuad lt_load_quad(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const LtQuad*>(p);
    return LtQuad{p[0], p[1], p[2], p[3]};
}
__device__ inline int64_t lt_min(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ inline double lt_abs_diff(float a, float b) { return fabs((double)a - (double)b); }

// sum |pred - y| over n consecutive floats, for the two predictions that share y (either may be NULL: its sum stays as it is)
__device__ inline void lt_mel_run(const float* before, const float* after, const float* y, int64_t n, int tid, double& sb, double& sa) {
    const bool vy = lt_aligned16(y), vb = before && lt_aligned16(before), va = after && lt_aligned16(after);
    const int64_t nq = n >> 2;
    for (int64_t q = tid; q < nq; q += kLtThreads) {
        const LtQuad t = lt_load_quad(y + 4 * q, vy);
        if (before) {
            const LtQuad v = lt_load_quad(before + 4 * q, vb);
            sb += lt_abs_diff(v.x, t.x); sb += lt_abs_diff(v.y, t.y); sb += lt_abs_diff(v.z, t.z); sb += lt_abs_diff(v.w, t.w);
        }
        if (after) {
            const LtQuad v = lt_load_quad(after + 4 * q, va);
            sa += lt_abs_diff(v.x, t.x); sa += lt_abs_diff(v.y, t.y); sa += lt_abs_diff(v.z, t.z); sa += lt_abs_diff(v.w, t.w);
        }
    }
    const int64_t i = 4 * nq + tid;
    if (i < n) {
        if (before) sb += lt_abs_diff(before[i], y[i]);
        if (after) sa += lt_abs_diff(after[i], y[i]);
    }
}

// sum (pred - target)^2 and sum |pred - target| over n consecutive frames of a predictor's output
__device__ inline void lt_frame_run(const float* pred, const float* tgt, int64_t n, int tid, double& sq, double& ab) {
#pragma clang fp contract(off)
    for (int64_t i = tid; i < n; i += kLtThreads) {
        const double d = (double)pred[i] - (double)tgt[i];
        const double dd = d * d;
        sq += dd;
        ab += fabs(d);
    }
}

// tokens: sum (d_outs - log(ds + 1))^2, and sum |d_outs - ds| as evaluation.py:31 writes it (log-domain output against linear durations)
__device__ inline void lt_token_run(const float* d_outs, const int64_t* ds, int64_t n, int tid, double& sq, double& ab) {
#pragma clang fp contract(off)
    for (int64_t i = tid; i < n; i += kLtThreads) {
        const double o = (double)d_outs[i], t = (double)ds[i];
        const double d = o - log(t + 1.0);
        const double dd = d * d;
        sq += dd;
        ab += fabs(o - t);
    }
}

__global__ __launch_bounds__(kLtThreads) void lt_terms(const LtRec* recs, LtArgs a, double* partials) {
    __shared__ double red[4][kLtPartial];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int g = blockIdx.x;
    int lo = 0, hi = a.B - 1;                  // the utterance whose tiles hold g: the last one with tile0 <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].tile0 <= g) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const LtRec rec = recs[b];
    const int t = g - rec.tile0;
    double s[kLtSums];
#pragma unroll
    for (int j = 0; j < kLtSums; ++j) s[j] = 0.0;
    double unused = 0.0;
    const float* before = a.before ? a.before + (int64_t)b * a.pred_stride_f * a.odim : nullptr;
    const float* after = a.after ? a.after + (int64_t)b * a.pred_stride_f * a.odim : nullptr;
    const float* ys = a.ys ? a.ys + (int64_t)b * a.y_stride_f * a.odim : nullptr;
    const float* e_outs = a.e_outs ? a.e_outs + (int64_t)b * a.pred_stride_f : nullptr;
    const float* p_outs = a.p_outs ? a.p_outs + (int64_t)b * a.pred_stride_f : nullptr;
    const float* es = a.es ? a.es + (int64_t)b * a.tgt_stride_f : nullptr;
    const float* ps = a.ps ? a.ps + (int64_t)b * a.tgt_stride_f : nullptr;
    const float* d_outs = a.d_outs ? a.d_outs + (int64_t)b * a.pred_stride_t : nullptr;
    const int64_t* ds = a.ds ? a.ds + (int64_t)b * a.ds_stride_t : nullptr;

    // ---- the tile's own frames [f0, f1) of [0, olen), and the tokens [0, ilen) in tile 0 ----
    const int64_t f0 = (int64_t)t * kLtFrames, f1 = lt_min(f0 + kLtFrames, rec.olen);
    if (f1 > f0) {
        const int64_t o = f0 * a.odim;
        if (ys) lt_mel_run(before ? before + o : nullptr, after ? after + o : nullptr, ys + o, (f1 - f0) * a.odim, tid, s[kLtBefore], s[kLtAfter]);
        if (e_outs) lt_frame_run(e_outs + f0, es + f0, f1 - f0, tid, s[kLtEnergySq], s[kLtEnergyAbs]);
        if (p_outs) lt_frame_run(p_outs + f0, ps + f0, f1 - f0, tid, s[kLtPitchSq], s[kLtPitchAbs]);
    }
    if (t == 0 && d_outs) lt_token_run(d_outs, ds, rec.ilen, tid, s[kLtDurSq], s[kLtDurAbs]);

    // ---- pads: this tile's share of the frames [olen, Lmax), and the tokens [ilen, Tmax) in tile 0 ----
    if (a.pads) {
        const int64_t npad = (int64_t)a.Lmax - rec.olen, share = (npad + rec.ntiles - 1) / rec.ntiles;
        const int64_t p0 = rec.olen + lt_min((int64_t)t * share, npad), p1 = rec.olen + lt_min((int64_t)(t + 1) * share, npad);
        if (p1 > p0) {
            const int64_t o = p0 * a.odim;
            if (ys) lt_mel_run(before ? before + o : nullptr, after ? after + o : nullptr, ys + o, (p1 - p0) * a.odim, tid, s[kLtPadBefore], s[kLtPadAfter]);
            if (e_outs) lt_frame_run(e_outs + p0, es + p0, p1 - p0, tid, s[kLtPadEnergySq], unused);
            if (p_outs) lt_frame_run(p_outs + p0, ps + p0, p1 - p0, tid, s[kLtPadPitchSq], unused);
        }
        if (t == 0 && d_outs) lt_token_run(d_outs + rec.ilen, ds + rec.ilen, (int64_t)a.Tmax - rec.ilen, tid, s[kLtPadDurSq], unused);
    }

    const int ns = a.pads ? kLtSums : kLtValidSums;
#pragma unroll
    for (int j = 0; j < kLtSums; ++j) {
        if (j < ns) {             // (the same for every thread of the grid)
            const double v = tg_wave_sum(s[j]);
            if (lane == 0) red[wv][j] = v;
        }
    }
    __syncthreads();
    if (tid < kLtPartial) partials[(size_t)g * kLtPartial + tid] = tid < ns ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
}

__global__ __launch_bounds__(kLtThreads) void lt_combine(const LtRec* recs, const double* partials, int B, int Tmax, int Lmax, double* terms, double* batch) {
    __shared__ double red[4][kLtTerms];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    double acc[kLtTerms];
#pragma unroll
    for (int j = 0; j < kLtTerms; ++j) acc[j] = 0.0;
    for (int b = tid; b < B; b += kLtThreads) {
        const LtRec rec = recs[b];
        double r[kLtTerms];
#pragma unroll
        for (int j = 0; j < kLtTerms; ++j) r[j] = 0.0;
        r[0] = (double)rec.ilen; r[1] = (double)rec.olen; r[2] = (double)(Tmax - rec.ilen); r[3] = (double)(Lmax - rec.olen);
        for (int t = 0; t < rec.ntiles; ++t) {
            const double* p = partials + (size_t)(rec.tile0 + t) * kLtPartial;
#pragma unroll
            for (int j = 0; j < kLtSums; ++j) r[4 + j] += p[j];
        }
        if (terms) {
#pragma unroll
            for (int j = 0; j < kLtTerms; ++j) terms[(size_t)b * kLtTerms + j] = r[j];
        }
#pragma unroll
        for (int j = 0; j < kLtTerms; ++j) acc[j] += r[j];
    }
    if (!batch) return;           // (every thread alike)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int j = 0; j < kLtTerms; ++j) acc[j] += __shfl_down(acc[j], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kLtTerms; ++j) red[wv][j] = acc[j];
    }
    __syncthreads();
    if (tid < kLtTerms) batch[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---- host side: workspace = the records, then one partial per tile ----
struct LtRegions { LtRec* recs; double* partials; size_t bytes; int64_t tiles; };

inline int64_t lt_tiles(int32_t olen) { return std::max<int64_t>(1, ((int64_t)olen + kLtFrames - 1) / kLtFrames); }

// false: a negative length, or more tiles than a grid holds
bool lt_regions(int32_t B, const int32_t* olens, void* ws, LtRegions& r) {
    int64_t tiles = 0;
    for (int b = 0; b < B; ++b) {
        if (olens[b] < 0) return false;
        tiles += lt_tiles(olens[b]);
    }
    if (tiles > INT32_MAX) return false;
    Carve c{(char*)ws};
    r = LtRegions{c.take<LtRec>(B), c.take<double>(tiles, kLtPartial), 0, tiles};
    r.bytes = c.off;
    return true;
}

size_t lt_workspace_bytes(int32_t B, const int32_t* olens) {
    LtRegions r;
    if (B < 0 || (B > 0 && !olens) || !lt_regions(B, olens, nullptr, r)) return 0;
    return r.bytes;
}

int lt_loss_terms(void* stream, const fs2_op_loss_args* a) {
    const char* who = "fs2_op_loss_terms";
    if (const int rc = rec_check_struct(who, "fs2_op_loss_args", a)) return rc;
    const int32_t B = a->B;
    if (B < 0 || (B > 0 && (!a->ilens || !a->olens))) return fail(nullptr, FS2_ERR_ARG, "%s: bad batch (B = %d) or null ilens / olens", who, B);
    if (a->Tmax < 0 || a->Lmax < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative Tmax %d / Lmax %d", who, a->Tmax, a->Lmax);
    for (int b = 0; b < B; ++b) {
        if (a->ilens[b] < 0 || a->olens[b] < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative length of utterance %d", who, b);
        if (a->ilens[b] > a->Tmax) return fail(nullptr, FS2_ERR_ARG, "%s: ilens[%d] = %d > Tmax %d", who, b, a->ilens[b], a->Tmax);
        if (a->olens[b] > a->Lmax) return fail(nullptr, FS2_ERR_ARG, "%s: olens[%d] = %d > Lmax %d", who, b, a->olens[b], a->Lmax);
    }
    // a group is a prediction and its target: given together or not at all (before and after share ys)
    if ((a->before || a->after) && !a->ys) return fail(nullptr, FS2_ERR_ARG, "%s: before / after without ys", who);
    if (!a->d_outs != !a->ds) return fail(nullptr, FS2_ERR_ARG, "%s: d_outs and ds must be given together", who);
    if (!a->e_outs != !a->es) return fail(nullptr, FS2_ERR_ARG, "%s: e_outs and es must be given together", who);
    if (!a->p_outs != !a->ps) return fail(nullptr, FS2_ERR_ARG, "%s: p_outs and ps must be given together", who);
    const bool mel = a->before || a->after, frames_pred = mel || a->e_outs || a->p_outs, frames_tgt = a->es || a->ps;
    if (mel && a->odim <= 0) return fail(nullptr, FS2_ERR_ARG, "%s: odim %d", who, a->odim);
    if (frames_pred && a->Lmax > a->pred_stride_f) return fail(nullptr, FS2_ERR_ARG, "%s: Lmax %d > pred_stride_f %d", who, a->Lmax, a->pred_stride_f);
    if (mel && a->Lmax > a->y_stride_f) return fail(nullptr, FS2_ERR_ARG, "%s: Lmax %d > y_stride_f %d", who, a->Lmax, a->y_stride_f);
    if (frames_tgt && a->Lmax > a->tgt_stride_f) return fail(nullptr, FS2_ERR_ARG, "%s: Lmax %d > tgt_stride_f %d", who, a->Lmax, a->tgt_stride_f);
    if (a->d_outs && a->Tmax > a->pred_stride_t) return fail(nullptr, FS2_ERR_ARG, "%s: Tmax %d > pred_stride_t %d", who, a->Tmax, a->pred_stride_t);
    if (a->d_outs && a->Tmax > a->ds_stride_t) return fail(nullptr, FS2_ERR_ARG, "%s: Tmax %d > ds_stride_t %d", who, a->Tmax, a->ds_stride_t);
    if (!a->terms && !a->batch) return FS2_OK;
    LtRegions at;                                       // (B = 0: no workspace, and lt_combine reads neither region)
    if (!lt_regions(B, a->olens, a->workspace, at)) return fail(nullptr, FS2_ERR_ARG, "%s: more tiles than one launch holds", who);
    if (const int rc = rec_check_workspace(who, B, a->workspace, a->workspace_bytes, at.bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    auto up = rec_uploader<LtRec, kLtRecsPerChunk>(B, at.recs, s);
    int64_t tile0 = 0;
    for (int b = 0; b < B; ++b) {
        const int nt = (int)lt_tiles(a->olens[b]);
        up.put(b, LtRec{a->ilens[b], a->olens[b], (int)tile0, nt});
        tile0 += nt;
    }
    if (B > 0) {
        LtArgs k{a->before, a->after, a->ys, a->d_outs, a->ds, a->e_outs, a->es, a->p_outs, a->ps,
                 a->pred_stride_f, a->y_stride_f, a->pred_stride_t, a->ds_stride_t, a->tgt_stride_f, a->odim, B, a->Tmax, a->Lmax, a->pads != 0};
        hipLaunchKernelGGL(lt_terms, dim3((unsigned)at.tiles), dim3(kLtThreads), 0, s, at.recs, k, at.partials);
    }
    hipLaunchKernelGGL(lt_combine, dim3(1), dim3(kLtThreads), 0, s, at.recs, at.partials, B, a->Tmax, a->Lmax, a->terms, a->batch);
    return rec_finish(who);
}
