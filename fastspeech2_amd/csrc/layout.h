// The gapped packed-row layout built from layout_rule.h: on the host (build_layout and the layouts of a batch) and on the device
// (frame_layout_dev, from the frame counts the duration scan left there; build_row_meta and scale_layout derive the per-row arrays).
// Plain HIP C++ restricted to what tests/kernel_standin/hip_standin.h provides (tests/kernel_standin/layout_main.cpp runs the kernels
// on the host against build_layout); the includer has included include/fs2.h (fs2_batch), <vector> and <algorithm>.
#pragma once
#include "layout_rule.h"

namespace fs2 {

constexpr int kLayoutThreads = 1024;      // frame_layout_dev's one workgroup

// row_pos / row_seq for a gapped packed layout (start[] ascending).
__global__ void build_row_meta(const int* start, const int* len, int B, int rpad, int* row_pos, int* row_seq) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rpad) return;
    int lo = 0, hi = B;   // first b with start[b] > row
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= row) lo = mid + 1; else hi = mid;
    }
    const int b = lo - 1;
    int pos = -1, seq = -1;
    if (b >= 0 && row - start[b] < len[b]) { pos = row - start[b]; seq = b; }
    row_pos[row] = pos;
    row_seq[row] = seq;
}

// Frame-side layout built on the device (device-driven mode of fs2_decode: no host read-back).  One workgroup; every rule it applies
// is layout_rule.h's, the one build_layout applies on the host.  Phases, a barrier between each:
//   1. longest and smallest frame count (wave reduction, one LDS atomic per wave);
//   2. len / klen / vlen of every utterance (utt_lens), the work list filled with padding items;
//   3. every utterance's place in the dealing order, by counting those dealt before it (dealt_before);
//   4. thread 0: the row walk (start, pcum = valid frames of the utterances before b: its row offset in the packed output);
//   5. attention blocks per utterance IN DEALING ORDER;
//   6. thread 0: the dealing (Dealer::place -> woff_tmp), the overflow flags, dims and the caller's copy of it;
//   7. the items of every utterance, kXcds apart from its first -- or, flags set, the empty layout.
// dims = status = {rows used, work list length, overflow flags, longest utterance, valid frames, 0, 0, 0}.
__global__ __launch_bounds__(kLayoutThreads) void frame_layout_dev(const int* olens, int B, int compat, int masked, int row_cap, int work_cap,
                                                                   int lmax_cap, int pe_rows, int* start, int* len, int* klen, int* vlen,
                                                                   int* rank_tmp, int* woff_tmp, int* pcum, int2* work, int* dims, int* status = nullptr, int gap = kGap) {
    // The serial parts (phases 4 and 6) run on one thread: their operands are staged in LDS first -- from global memory every iteration
    // was a dependent round trip.  Round 2: 53 -> 28 us per call at B = 64; what is left is the barrier phases, each draining thread 0's
    // global stores, and the launch.
    constexpr int kStage = 4096;                      // utterances staged in LDS (beyond: the same code on the global arrays)
    __shared__ int s_len[kStage], s_vlen[kStage], s_order[kStage];
    __shared__ int s_max, s_min;
    const int tid = threadIdx.x;
    const bool staged = B <= kStage;
    if (tid == 0) { s_max = 0; s_min = 0x7fffffff; }
    __syncthreads();
    int mx = 0, mn = 0x7fffffff;
    for (int b = tid; b < B; b += kLayoutThreads) { mx = max(mx, olens[b]); mn = min(mn, olens[b]); }
    for (int o = 32; o > 0; o >>= 1) { mx = max(mx, __shfl_xor(mx, o)); mn = min(mn, __shfl_xor(mn, o)); }
    if ((tid & 63) == 0) { atomicMax(&s_max, mx); atomicMin(&s_min, mn); }      // one LDS atomic per wave, not 1024 on one address
    __syncthreads();
    mx = s_max;
    for (int b = tid; b < B; b += kLayoutThreads) {
        const UttLens u = utt_lens(max(olens[b], 0), mx, compat, masked);
        vlen[b] = u.vlen;
        len[b] = u.len;
        klen[b] = u.klen;
        if (staged) { s_vlen[b] = u.vlen; s_len[b] = u.len; }
    }
    for (int i = tid; i < work_cap; i += kLayoutThreads) work[i] = make_int2(-1, 0);
    __syncthreads();
    const bool own = keys_are_own(compat, masked);      // (klen of utt_lens, its loop-invariant choice made once)
    for (int b = tid; b < B; b += kLayoutThreads) {
        const int k = own ? max(olens[b], 0) : mx;
        int r = 0;
        for (int j = 0; j < B; ++j) {
            const int vj = staged ? s_vlen[j] : max(olens[j], 0);
            r += dealt_before(own ? vj : mx, j, k, b);
        }
        if (staged) s_order[r] = b; else rank_tmp[r] = b;
    }
    __syncthreads();
    __shared__ int s_row, s_frames;
    if (tid == 0) {
        int row = gap;
        int frames = 0;
        for (int b = 0; b < B; ++b) {
            row = row_start(row);
            start[b] = row;
            row = row_after(row, staged ? s_len[b] : len[b], gap);
            pcum[b] = frames;
            frames += staged ? s_vlen[b] : vlen[b];
        }
        s_row = rows_used(row); s_frames = frames;
    }
    __syncthreads();
    // (in dealing order, so that the serial loop below walks two arrays front to back instead of chasing s_order[r] -> s_len[b] through
    //  LDS: two dependent round trips per utterance on one thread.  s_vlen is free: phase 4 was its last reader)
    if (staged)
        for (int r = tid; r < B; r += kLayoutThreads) s_vlen[r] = att_blocks(s_len[s_order[r]]);
    __syncthreads();
    if (tid == 0) {
        const int row = s_row, frames = s_frames;
        Dealer deal;
        // (the operands of utterance r + 1 are fetched before place() searches the queues for utterance r: the search is some 25 dependent
        //  VALU instructions, which ran behind both loads' round trips when the blocks were fetched as its argument: + 4 us at B = 64)
        int b = staged ? s_order[0] : rank_tmp[0];
        int blocks = staged ? s_vlen[0] : att_blocks(len[b]);
        for (int r = 0; r < B; ++r) {
            const int rn = min(r + 1, B - 1);
            const int bn = staged ? s_order[rn] : rank_tmp[rn];
            const int blocks_n = staged ? s_vlen[rn] : att_blocks(len[bn]);
            woff_tmp[b] = deal.place(blocks);
            b = bn; blocks = blocks_n;
        }
        const int ovf = overflow_flags(row, deal.depth, mx, s_min, row_cap, work_cap, lmax_cap, pe_rows);
        const int nwork = ovf ? 0 : deal.items();
        dims[0] = row; dims[1] = nwork; dims[2] = ovf; dims[3] = mx; dims[4] = frames; dims[5] = 0; dims[6] = 0; dims[7] = 0;
        if (status) {     // the caller's copy of the same eight words
            status[0] = row; status[1] = nwork; status[2] = ovf; status[3] = mx; status[4] = frames; status[5] = 0; status[6] = 0; status[7] = 0;
        }
    }
    __syncthreads();
    if (dims[2] != 0) {           // a capacity is too small: leave an empty layout (all rows are gap rows, no work) so that
        for (int b = tid; b < B; b += kLayoutThreads) { start[b] = row_start(gap); len[b] = 0; klen[b] = 0; vlen[b] = 0; }    // nothing indexes out of range
        return;
    }
    for (int b = tid; b < B; b += kLayoutThreads) {
        const int nq = att_blocks(len[b]), o = woff_tmp[b];
        for (int q = 0; q < nq; ++q) work[o + kXcds * q] = make_int2(b, q);
    }
}

// reduction_factor r > 1: the Postnet's row layout = the decoder's with every row expanded to r rows
__global__ void scale_layout(const int* start, const int* len, const int* vlen, const int* dims, int B, int r, int* start2, int* len2,
                             int* vlen2, int* dims2) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { start2[b] = start[b] * r; len2[b] = len[b] * r; vlen2[b] = vlen[b] * r; }
    if (b == 0 && dims != nullptr) {
        dims2[0] = dims[0] * r;      // rows in use
#pragma unroll
        for (int i = 1; i < 8; ++i) dims2[i] = dims[i];
    }
}

// ---- host side
struct HostLayout {
    int B = 0, R = 0, Rpad = 0;
    std::vector<int> start, len, klen, vlen;
    std::vector<int2> work;
    int work_cap = -1;      // device-driven layout: R / Rpad / work_cap are capacities, the vectors stay empty
    int nwork() const { return work_cap >= 0 ? work_cap : (int)work.size(); }
};
struct DevLayout {
    int *start = nullptr, *len = nullptr, *klen = nullptr, *vlen = nullptr, *row_pos = nullptr, *row_seq = nullptr;
    int2* work = nullptr;
    int* dims = nullptr;    // device-driven layout: {rows used, work items, overflow flags, longest utterance, valid frames, 0, 0, 0}
    int* pcum = nullptr;    // device-driven layout: valid frames before each utterance (packed-output row offsets)
};

// the layout of B utterances of valid[b] positions, the longest of `longest` (utt_lens: compat, masked)
inline void build_layout(HostLayout& L, int B, const int64_t* valid, int longest, int compat, int masked, int gap) {
    L.B = B;
    L.start.resize(B); L.len.resize(B); L.klen.resize(B); L.vlen.resize(B);
    int row = gap;
    for (int b = 0; b < B; ++b) {
        const UttLens u = utt_lens((int)valid[b], longest, compat, masked);
        L.len[b] = u.len; L.klen[b] = u.klen; L.vlen[b] = u.vlen;
        L.start[b] = row = row_start(row);
        row = row_after(row, u.len, gap);
    }
    L.R = rows_used(row);
    L.Rpad = rows_padded(L.R);
    std::vector<int> order(B), first(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return dealt_before(L.klen[x], x, L.klen[y], y); });
    Dealer deal;
    for (int b : order) first[b] = deal.place(att_blocks(L.len[b]));
    L.work.assign(deal.items(), make_int2(-1, 0));
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < att_blocks(L.len[b]); ++q) L.work[first[b] + kXcds * q] = make_int2(b, q);
}

// the encoder's layout: Tmax rows per utterance under padded-batch semantics, keys = the utterance's own phonemes
inline void token_layout(const fs2_batch& b, HostLayout& L, int gap) { build_layout(L, b.B, b.ilens, b.Tmax, b.compat_padded, /*masked=*/1, gap); }

inline void frame_layout(const fs2_batch& b, const int64_t* olens, int masked, HostLayout& L, int gap) {
    build_layout(L, b.B, olens, (int)std::max<int64_t>(0, *std::max_element(olens, olens + b.B)), b.compat_padded, masked, gap);
}

// device-driven layout: the capacities stand for the layout nobody on the host knows
inline void capacity_layout(const fs2_batch& b, int64_t row_capacity, int lmax_cap, HostLayout& L) {
    L.B = b.B; L.R = (int)row_capacity; L.Rpad = rows_padded((int)row_capacity);
    L.work_cap = work_capacity(row_capacity, b.B, lmax_cap);
    L.start.clear(); L.len.clear(); L.klen.clear(); L.vlen.clear(); L.work.clear();
}

}  // namespace fs2
