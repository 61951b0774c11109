// Variance predictors on at most K frames per phoneme (FS2_VARSHORT; rule: layout_rule.h): the device side.  The short layout -- the gapped
// packed rows of layout_rule.h over the SHORT durations -- is always built on the device, because the host never knows per-token durations
// without a sync; it is built by the launch that wrote the length regulator's index anyway (lr.index), so the call has no launch more for it.
#pragma once
#include "elementwise.h"
#include "layout_rule.h"

namespace fs2 {

// (the argument block: row_step_args.h: ShortLayoutArgs)

// One thread per row of the longer of the two row ranges.  Every workgroup walks the utterances itself (row_start / row_after / rows_used over the
// short lengths: B steps on one thread, operands staged in LDS), which is cheaper than a launch of its own in front of this one.
constexpr int kShortStage = 2048;      // utterances staged in LDS (beyond: the global arrays, which every workgroup fills with the same values)
__global__ __launch_bounds__(256) void lr_index_short(ShortLayoutArgs a) {
    __shared__ int s_start[kShortStage], s_len[kShortStage];
    __shared__ int s_rows;
    const int tid = threadIdx.x;
    const bool staged = a.B <= kShortStage;
    int* st = staged ? s_start : a.sstart;
    int* ln = staged ? s_len : a.slen;
    const bool dead = a.ovf != nullptr && *a.ovf != 0;
    for (int b = tid; b < a.B; b += 256) ln[b] = dead ? 0 : max(a.so32[b], 0);
    __syncthreads();
    if (tid == 0) {
        int row = a.gap;
        for (int b = 0; b < a.B; ++b) {
            row = row_start(row);
            st[b] = row;
            row = row_after(row, ln[b], a.gap);
        }
        s_rows = rows_used(row);
    }
    __syncthreads();
    // (cannot happen where the frame layout is the one of these durations: every short length is at most the frame length, so no short start
    //  lies behind the frame start; the check keeps a caller's inconsistent frame counts from indexing out of range)
    const bool empty = dead || s_rows > a.Rs;
    if (blockIdx.x == 0) {
        if (staged)
            for (int b = tid; b < a.B; b += 256) { a.sstart[b] = st[b]; a.slen[b] = empty ? 0 : ln[b]; }
        if (tid == 0) a.sdims[0] = empty ? 0 : s_rows;
    }
    const int row = blockIdx.x * 256 + tid;
    if (row < a.Rs_pad) {
        int lo = 0, hi = a.B;   // first b with start[b] > row
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (st[mid] <= row) lo = mid + 1; else hi = mid;
        }
        const int b = lo - 1;
        int pos = -1, seq = -1, tk = -1;
        if (!empty && b >= 0 && row - st[b] < ln[b]) {
            pos = row - st[b]; seq = b;
            const int* c = a.scum + (size_t)b * a.Tmax;
            int l2 = 0, h2 = a.ilen[b];   // first i with scum[b, i] > pos
            while (l2 < h2) {
                const int mid = (l2 + h2) >> 1;
                if (c[mid] <= pos) l2 = mid + 1; else h2 = mid;
            }
            tk = l2;
        }
        a.srow_pos[row] = pos; a.srow_seq[row] = seq; a.slri[row] = tk;
    }
    if (row < a.R) {
        const int b = a.row_seq[row], j = a.row_pos[row];
        const int tk = lr_token_index(b, j, a.cum, a.Tmax, a.ilen, a.vlen);
        a.lri[row] = tk;
        int s = -1;
        if (!empty && tk >= 0 && tk < a.ilen[b]) {
            const int* c = a.cum + (size_t)b * a.Tmax;
            const int* sc = a.scum + (size_t)b * a.Tmax;
            const int c0 = tk ? c[tk - 1] : 0, s0 = tk ? sc[tk - 1] : 0;
            s = st[b] + s0 + vs_short_offset(j - c0, c[tk] - c0, a.K);
        }
        a.f2s[row] = s;
    }
}

// torch.bucketize of the predictions, once per short row (dec_in_gather reads the indices through f2s).  e / p == nullptr: that value is given per
// frame (teacher forcing) and searched there.
__global__ void var_bucket_short(const float* e, const float* p, const int* srow_pos, int Rs, const float* ebins, const float* pbins, int nb, int* sqe, int* sqp) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= Rs) return;
    const bool live = srow_pos[row] >= 0;
    if (e) sqe[row] = live ? bucket_index(e[row], ebins, nb) : -1;
    if (p) sqp[row] = live ? bucket_index(p[row], pbins, nb) : -1;
}

// e_out / p_out from the short rows: dst[b, j] = src[f2s[start[b] + j]] for j < limit[b], else 0 (unpack_rows through the frame-to-short map)
__global__ void unpack_short(const float* src, const int* f2s, const int* start, const int* limit, int B, int Lout, float* dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * Lout) return;
    const int j = (int)(i % Lout), b = (int)(i / Lout);
    float v = 0.f;
    if (j < limit[b]) {
        const int s = f2s[start[b] + j];
        if (s >= 0) v = src[s];
    }
    dst[i] = v;
}

}  // namespace fs2
