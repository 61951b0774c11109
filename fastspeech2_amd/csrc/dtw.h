// Dynamic time warping between pairs of feature sequences of different lengths, with the F0 and energy errors over the aligned frame
// pairs: the numbers of the FREE-RUNNING validation, behind fs2_op_dtw (include/fs2.h; tests/dtw_oracle.py
// states the same in numpy).  Not a header of its own: fs2_runtime.hip includes it inside its unnamed namespace, after losses.h (fail(),
// align_up()); it includes pair_plan.h, the host side it shares with align.h (DtwPair, the layout, the checks, the groups).  Plain HIP C++, restricted to what tests/kernel_standin/hip_standin.h provides (the stand-in moves a cell's record
// between lanes in one exchange, hip_standin_record.h beside it, where the device shuffles it field by field).
//
// The definition.  d(i, j) = sqrt(sum_k ((double)a[i, k] - (double)b[j, k])^2), k in increasing order, one multiply and one add per
// term (nothing is contracted into a fused multiply-add), the square root in double.  C(i, j) = d(i, j) + min over the predecessors
// (i-1, j-1), (i-1, j), (i, j-1), chosen in that order with a strict "<" (a tie keeps the earlier one; a predecessor outside the
// matrix counts as +inf; (0, 0) starts from the empty path).  Each cell carries the record of its path -- copied from the chosen
// predecessor and extended by its own pair (i, j) -- so no back-pointer matrix exists and nothing is traced back.
//
// dtw_dist: one workgroup of 256 threads per kDtwTile x kDtwTile tile of one pair's matrix (the tile is found by bisection over the
// uploaded tile offsets, as lt_terms finds its utterance).  The feature dimension is staged through LDS kDtwKc columns at a time
// (rows padded to kDtwKc + 1 floats: the 16 rows a wave reads at one k lie on 16 different banks); thread (ty, tx) holds the 4 x 4
// patch of rows ty + 16 r and columns tx + 16 c in double.
//
// dtw_sweep: one workgroup of kDtwCols threads per pair.  The matrix is swept in blocks of kDtwCols columns; thread t owns column
// j0 + t and walks down its rows skewed against its neighbour: at step s it handles row s - t - wave (kDtwLag - 1).  Inside a wave
// the record of (i, j - 1) is the lower lane's record of the previous step (one shuffle per field) and that of (i - 1, j - 1) is what
// that shuffle returned one step earlier.  Across the three wave boundaries the records travel through a ring in LDS: a wave runs
// kDtwLag steps behind its lower neighbour, so the workgroup meets at a barrier once per kDtwLag steps, not once per step.  The same
// ring carries the left edge of a column block in (staged from the workspace one chunk ahead) and its right edge out (flushed one
// chunk behind); the two edge buffers of a pair alternate between column blocks.  The d values and the a-side tracks of the next
// chunk are loaded while the current one is computed.  No floating-point atomics, nothing waits on another workgroup.
//
// records_combine<12, -1, -1> (record_op.h; one workgroup): copies the records out and adds the batch record, term by term, over the
// pairs in index order.

#include "pair_plan.h"
constexpr int kDtwCols = 256;             // threads of dtw_sweep = columns of a column block
constexpr int kDtwLag = 16;               // steps between two barriers of dtw_sweep (= steps a wave runs behind its lower neighbour)
constexpr int kDtwTile = 64;              // rows and columns of a dtw_dist tile
constexpr int kDtwKc = 32;                // feature columns staged per pass of dtw_dist
constexpr int kDtwTerms = FS2_DTW_TERMS;  // doubles of a record
static_assert(FS2_DTW_TERMS == 12, "record layout of include/fs2.h");
static_assert(kDtwCols == 256 && kDtwTile * kDtwTile == 16 * kDtwCols, "dtw_dist: 256 threads, a 4 x 4 patch each");

// the record a cell carries (include/fs2.h: indices 2 .. 8 of a pair's record)
struct DtwCell {
    double cost, se, sp, spv;
    int steps, nv, mis, pad;
};
static_assert(sizeof(DtwCell) == kDtwCellBytes && kDtwCols == kPairCols && kDtwTile == kPairTile, "pair_plan.h sizes the matrices and edge buffers");

__global__ __launch_bounds__(256) void dtw_dist(const DtwPair* recs, int npairs, const float* a, const float* b, int64_t a_stride,
                                                int64_t b_stride, int D, char* ws) {
#pragma clang fp contract(off)
    constexpr int P = kDtwKc + 1;
    __shared__ float sa[kDtwTile * P], sb[kDtwTile * P];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int g = blockIdx.x;
    int lo = 0, hi = npairs - 1;               // the pair whose tiles hold g: the last one with tile0 <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].tile0 <= g) lo = mid; else hi = mid - 1;
    }
    const DtwPair rec = recs[lo];
    const int t = g - rec.tile0, i0 = (t / rec.tcols) * kDtwTile, j0 = (t % rec.tcols) * kDtwTile;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int kc = 0; kc < D; kc += kDtwKc) {
        const int kw = min(kDtwKc, D - kc);
        for (int idx = tid; idx < kDtwTile * kw; idx += 256) {          // rows outside the matrix are never read: 0 in their place
            const int r = idx / kw, k = idx - r * kw;
            sa[r * P + k] = i0 + r < rec.n ? a[(int64_t)(rec.a0 + i0 + r) * a_stride + kc + k] : 0.f;
            sb[r * P + k] = j0 + r < rec.m ? b[(int64_t)(rec.b0 + j0 + r) * b_stride + kc + k] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < kw; ++k) {
            float av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { av[r] = sa[(ty + 16 * r) * P + k]; bv[r] = sb[(tx + 16 * r) * P + k]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double df = (double)av[r] - (double)bv[c];
                    const double sq = df * df;
                    acc[r][c] += sq;
                }
        }
        __syncthreads();
    }
    double* d = (double*)(ws + rec.d_off);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < rec.n && j < rec.m) d[(int64_t)i * rec.m + j] = sqrt(acc[r][c]);
        }
}

__device__ inline DtwCell dtw_cell(double cost) { return DtwCell{cost, 0.0, 0.0, 0.0, 0, 0, 0, 0}; }
__device__ inline DtwCell dtw_shfl_up(const DtwCell& c) {      // the record of the lane below (lane 0: its own)
#ifdef FS2_STANDIN_SHFL_UP_RECORD      // (tests/kernel_standin/hip_standin_record.h: the host stand-in's one exchange for the whole record)
    return FS2_STANDIN_SHFL_UP_RECORD(c);
#else
    DtwCell r;
    r.cost = __shfl_up(c.cost, 1); r.se = __shfl_up(c.se, 1); r.sp = __shfl_up(c.sp, 1); r.spv = __shfl_up(c.spv, 1);
    r.steps = __shfl_up(c.steps, 1); r.nv = __shfl_up(c.nv, 1); r.mis = __shfl_up(c.mis, 1); r.pad = 0;
    return r;
#endif
}

__global__ __launch_bounds__(kDtwCols) void dtw_sweep(const DtwPair* recs, const float* e_a, const float* e_b, const float* p_a,
                                                      const float* p_b, char* ws, double* terms) {
#pragma clang fp contract(off)
    constexpr int K = kDtwLag, kLast = kDtwCols - 1, kLastOff = kLast + (kLast >> 6) * (K - 1);
    __shared__ DtwCell ring[5][2 * K];         // ring[w]: what wave w's lane 0 reads (0: the left edge); ring[w + 1]: what its lane 63 writes
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const DtwPair rec = recs[blockIdx.x];
    double* out = terms + (size_t)blockIdx.x * kDtwTerms;
    const int N = rec.n, M = rec.m;
    if (N == 0 || M == 0) {                    // (every thread alike)
        if (tid < kDtwTerms) out[tid] = tid == 0 ? (double)N : tid == 1 ? (double)M : 0.0;
        return;
    }
    const double inf = __builtin_huge_val();
    const double* d = (const double*)(ws + rec.d_off);
    DtwCell* edges = (DtwCell*)(ws + rec.aux);
    const int off = tid + wv * (K - 1);        // this thread handles row s - off at step s
    DtwCell mine = dtw_cell(inf);
    int cb = 0;
    for (int j0 = 0; j0 < M; j0 += kDtwCols, ++cb) {
        const int j = j0 + tid;
        const bool col = j < M, more = j0 + kDtwCols < M, first = j0 == 0;
        const int tl = min(kLast, M - 1 - j0);                          // the thread of the block's last column
        const int nsteps = N + tl + (tl >> 6) * (K - 1), nchunks = (nsteps + K - 1) / K;
        const DtwCell* edge_in = edges + (size_t)((cb + 1) & 1) * N;    // written by the previous column block
        DtwCell* edge_out = edges + (size_t)(cb & 1) * N;
        const float eb = e_b && col ? e_b[rec.b0 + j] : 0.f, pb = p_b && col ? p_b[rec.b0 + j] : 0.f;
        const bool stager = !first && tid < K;
        mine = dtw_cell(inf);
        DtwCell diag = dtw_cell(inf);
        double dc[K], dn[K];
        float eac[K], ean[K], pac[K], pan[K];
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const int i = u - off;
            const bool on = col && i >= 0 && i < N;
            dc[u] = on ? d[(int64_t)i * M + j] : 0.0;
            eac[u] = on && e_a ? e_a[rec.a0 + i] : 0.f;
            pac[u] = on && p_a ? p_a[rec.a0 + i] : 0.f;
        }
        if (stager) ring[0][tid] = tid < N ? edge_in[tid] : dtw_cell(inf);
        __syncthreads();
        for (int c = 0; c < nchunks; ++c) {
            const int h = (c & 1) * K, hp = K - h;                     // this chunk's half of every ring, and the other one
#pragma unroll
            for (int u = 0; u < K; ++u) {                               // the next chunk's inputs
                const int i = (c + 1) * K + u - off;
                const bool on = col && i >= 0 && i < N;
                dn[u] = on ? d[(int64_t)i * M + j] : 0.0;
                ean[u] = on && e_a ? e_a[rec.a0 + i] : 0.f;
                pan[u] = on && p_a ? p_a[rec.a0 + i] : 0.f;
            }
            DtwCell staged = dtw_cell(inf);
            if (stager) {
                const int row = (c + 1) * K + tid;
                if (row < N) staged = edge_in[row];
            }
            if (more && c > 0 && tid < K) {                             // the right edge of the previous chunk
                const int row = (c - 1) * K + tid - kLastOff;
                if (row >= 0 && row < N) edge_out[row] = ring[4][hp + tid];
            }
#pragma unroll
            for (int u = 0; u < K; ++u) {
                const int i = c * K + u - off;
                DtwCell left = dtw_shfl_up(mine);
                if (lane == 0) {
                    if (tid == 0) left = first ? dtw_cell(inf) : ring[0][h + u];
                    else left = c > 0 ? ring[wv][hp + u] : dtw_cell(inf);
                }
                if (col && i >= 0 && i < N) {
                    DtwCell best = diag;
                    if (mine.cost < best.cost) best = mine;             // (i - 1, j)
                    if (left.cost < best.cost) best = left;             // (i, j - 1)
                    if (i == 0 && j == 0) best = dtw_cell(0.0);
                    best.cost = dc[u] + best.cost;
                    best.steps += 1;
                    if (e_a) best.se += fabs((double)eac[u] - (double)eb);
                    if (p_a) {
                        const double dp = fabs((double)pac[u] - (double)pb);
                        const bool va = pac[u] != 0.f, vb = pb != 0.f;
                        best.sp += dp;
                        if (va && vb) { best.nv += 1; best.spv += dp; }
                        else if (va != vb) best.mis += 1;
                    }
                    mine = best;
                }
                diag = left;
                if (lane == 63) ring[wv + 1][h + u] = mine;
            }
            if (stager) ring[0][hp + tid] = staged;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < K; ++u) { dc[u] = dn[u]; eac[u] = ean[u]; pac[u] = pan[u]; }
        }
        if (more && tid < K) {
            const int row = (nchunks - 1) * K + tid - kLastOff;
            if (row >= 0 && row < N) edge_out[row] = ring[4][((nchunks - 1) & 1) * K + tid];
        }
        __syncthreads();
    }
    if (tid == (M - 1) % kDtwCols) {
        out[0] = (double)N; out[1] = (double)M; out[2] = (double)mine.steps; out[3] = mine.cost; out[4] = mine.se; out[5] = mine.sp;
        out[6] = (double)mine.nv; out[7] = mine.spv; out[8] = (double)mine.mis; out[9] = 0.0; out[10] = 0.0; out[11] = 0.0;
    }
}

// ---- host side: pair_plan.h's plan, then per group dtw_dist and dtw_sweep ----
// the pair records travel as kernel arguments: no host copy, no synchronisation
inline void dtw_upload(const PairPlan& p, hipStream_t s) { pair_chunks(p, upload_launch<DtwPair, kDtwRecsPerChunk>(p.at.recs, s)); }
inline void dtw_launch_dist(const PairPlan& p, const PairGroup& g, const DtwPair* recs, char* ws, hipStream_t s) {
    if (g.tiles > 0)
        hipLaunchKernelGGL(dtw_dist, dim3((unsigned)g.tiles), dim3(256), 0, s, recs + g.first, g.count, p.a, p.b, p.a_stride, p.b_stride, p.D, ws);
}

size_t dtw_workspace_bytes(int32_t B, const int32_t* a_lens, const int32_t* b_lens, size_t cap) { return pair_workspace_bytes(kDtwOp, B, a_lens, b_lens, cap); }

int dt_dtw(void* stream, const fs2_op_dtw_args* a) {
    const char* who = kDtwOp.who;
    if (const int rc = pair_check_args(kDtwOp, a)) return rc;
    if (!a->e_a != !a->e_b) return fail(nullptr, FS2_ERR_ARG, "%s: e_a and e_b must be given together", who);
    if (!a->p_a != !a->p_b) return fail(nullptr, FS2_ERR_ARG, "%s: p_a and p_b must be given together", who);
    if (!a->terms && !a->batch) return FS2_OK;
    PairPlan p;
    if (const int rc = pair_plan(kDtwOp, a, nullptr, p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)a->workspace;
    DtwPair* recs = p.at.recs;
    double* recs_out = p.at.terms;
    dtw_upload(p, s);
    // one dtw_dist and one dtw_sweep per group, in stream order: a group's matrices are dead when the next group's are written
    pair_groups(p, [&](const PairGroup& g) {
        dtw_launch_dist(p, g, recs, ws, s);
        hipLaunchKernelGGL(dtw_sweep, dim3((unsigned)g.count), dim3(kDtwCols), 0, s, recs + g.first, a->e_a, a->e_b, a->p_a, a->p_b, ws,
                           recs_out + (size_t)g.first * kDtwTerms);
    });
    hipLaunchKernelGGL((records_combine<kDtwTerms, -1, -1>), dim3(1), dim3(256), 0, s, recs_out, a->B, a->terms, a->batch);
    return rec_finish(who);
}
