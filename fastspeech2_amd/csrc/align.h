// Forced alignment of recorded frames to synthesized frames: every frame of the recording is assigned to exactly one state (a frame
// of the synthesis), monotonically, so that the counts per phoneme are durations that add up to the recording's length -- behind
// fs2_op_align (include/fs2.h; tests/align_oracle.py states the same in numpy).  Not a header of its own:
// fs2_runtime.hip includes it inside its unnamed namespace, after dtw.h (dtw_dist, dtw_upload, dtw_launch_dist, and through it
// pair_plan.h: the host side it shares with dtw.h).  Plain HIP C++, restricted to what tests/kernel_standin/hip_standin.h provides.
//
// The definition.  d(i, j) is dtw.h's.  Q(0, 0) = d(0, 0); Q(i, 0) = +inf for i > 0; Q(i, j) = d(i, j) + min over k = 0 .. S of
// Q(i - k, j - 1), S = max_step: the predecessor is chosen in the order k = 0, 1, 2 with a strict "<" (a tie keeps the smaller k); a
// predecessor outside the matrix counts as +inf, that is, it is never compared.  s(M-1) = N-1 and s(j-1) = s(j) - k(s(j), j).
//
// The matrix is kept with the sides SWAPPED: dtw_dist is handed the recording as its a side and the synthesis as its b side, so it
// writes d as [M, N] -- column j of the recurrence is one contiguous row of memory -- and (a - b)^2 = (b - a)^2 in double, so the
// values are d(i, j) bit for bit.  pair_plan.h swaps them once (kAlignOp.swapped), so a DtwPair of this file reads: a0, n = first frame
// and frames of the RECORDING (M); b0, m = first state and states of the SYNTHESIS (N); aux = n_labels (-1: no labels).
//
// align_sweep: one workgroup of kAlignThreads threads per pair.  It overwrites d with Q in place, row after row (frame after frame):
// thread t computes the states t, t + kAlignThreads, ... of frame j from row j - 1, which it reads back from global memory after the
// one barrier per frame.  After the last barrier thread 0 walks back from (N-1, M-1): it re-derives every k from the stored Q with
// the comparisons of the recurrence in the same order (so the same decisions), writes s(j) and counts: s is monotone and the labels
// are non-decreasing, so a label's frames are one run and its count is written once, when the run ends -- no atomics.  Every loop
// is bounded by N, M or dur_stride; nothing waits on another workgroup.
//
// records_combine<8, 2, -1> (record_op.h; one workgroup): copies the records out and forms the batch record over the pairs in index
// order -- column 2 counts the pairs without an alignment, the other columns are sums over the aligned ones.

constexpr int kAlignThreads = 256;          // threads of align_sweep
constexpr int kAlignUnroll = 4;             // states a thread has in flight per pass over a row
constexpr int kAlignTerms = FS2_ALIGN_TERMS;
static_assert(FS2_ALIGN_TERMS == 8, "record layout of include/fs2.h");

// the predecessor of state i in the previous frame's row: -> the chosen cost, k in `k`.  k > 0 only if Q(i - k, j - 1) exists
// (i - k >= 0) AND is strictly smaller than the best so far, whatever the data hold (a comparison with NaN is false): i - k >= 0.
__device__ inline double align_pred(const double* prev, int i, int S, int& k) {
    double best = prev[i];
    k = 0;
    if (i >= 1) {
        const double p = prev[i - 1];
        if (p < best) { best = p; k = 1; }
    }
    if (S == 2 && i >= 2) {
        const double p = prev[i - 2];
        if (p < best) { best = p; k = 2; }
    }
    return best;
}

__global__ __launch_bounds__(kAlignThreads) void align_sweep(const DtwPair* recs, int S, const int32_t* labels, char* ws, int64_t* durations,
                                                              int64_t dur_stride, int32_t* state, double* terms) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const DtwPair rec = recs[blockIdx.x];
    const int M = rec.n, N = rec.m;
    const int nl = labels ? (int)rec.aux : N;
    double* out = terms + (size_t)blockIdx.x * kAlignTerms;
    int64_t* dur = durations ? durations + (int64_t)blockIdx.x * dur_stride : nullptr;
    int32_t* st = state ? state + rec.a0 : nullptr;
    if (dur)
        for (int64_t t = tid; t < dur_stride; t += kAlignThreads) dur[t] = 0;
    if (N < 1 || M < 1 || (int64_t)N - 1 > (int64_t)S * (M - 1)) {       // no alignment exists (every thread alike)
        if (st)
            for (int j = tid; j < M; j += kAlignThreads) st[j] = -1;
        if (tid < kAlignTerms) out[tid] = tid == 0 ? (double)N : tid == 1 ? (double)M : tid == 2 ? 1.0 : 0.0;
        return;
    }
    const double inf = __builtin_huge_val();
    double* Q = (double*)(ws + rec.d_off);                                // [M, N]: row j holds d(., j), then Q(., j)
    for (int i = tid; i < N; i += kAlignThreads)
        if (i > 0) Q[i] = inf;                                            // Q(0, 0) = d(0, 0) stays
    __syncthreads();
    for (int j = 1; j < M; ++j) {
        const double* prev = Q + (int64_t)(j - 1) * N;
        double* cur = Q + (int64_t)j * N;
        for (int i0 = tid; i0 < N; i0 += kAlignThreads * kAlignUnroll) {
            double best[kAlignUnroll], dv[kAlignUnroll];
#pragma unroll
            for (int u = 0; u < kAlignUnroll; ++u) {
                const int i = i0 + u * kAlignThreads;
                int k;
                best[u] = i < N ? align_pred(prev, i, S, k) : 0.0;
                dv[u] = i < N ? cur[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kAlignUnroll; ++u) {
                const int i = i0 + u * kAlignThreads;
                if (i < N) cur[i] = dv[u] + best[u];
            }
        }
        __syncthreads();
    }
    const double cost = Q[(int64_t)(M - 1) * N + N - 1];
    if (!isfinite(cost)) {                                                // (every thread alike: all read the same value)
        if (st)
            for (int j = tid; j < M; j += kAlignThreads) st[j] = -1;
        if (tid < kAlignTerms) out[tid] = tid == 0 ? (double)N : tid == 1 ? (double)M : tid == 2 ? 2.0 : tid == 3 ? cost : 0.0;
        return;
    }
    if (tid != 0) return;
    // the walk back: M - 1 dependent steps.  `s` stays in [0, N - 1] by align_pred's rule, so every read lies in the pair's own matrix
    // and every write in its own rows.  A label outside [0, nl) is skipped: nothing is written for it.
    int s = N - 1, used = 0, run = 0, longest = 0, seen = 0;
    int lab = labels ? labels[rec.b0 + s] : s;
    int64_t count = 0;                                                    // frames of the label `lab` so far
    for (int j = M - 1; j >= 0; --j) {
        if (st) st[j] = s;
        ++count;
        ++run;
        int k = 0;
        if (j > 0) align_pred(Q + (int64_t)(j - 1) * N, s, S, k);
        if (j == 0 || k > 0) {                                            // frame j is the first frame of state s
            ++used;
            longest = max(longest, run);
            run = 0;
            const int below = j == 0 ? -1 : labels ? labels[rec.b0 + s - k] : s - k;
            if (j == 0 || below != lab) {                                 // ... and of its label, whose count is complete
                if (lab >= 0 && lab < nl) {
                    if (dur) dur[lab] = count;
                    ++seen;
                }
                count = 0;
                lab = below;
            }
        }
        s -= k;
    }
    out[0] = (double)N; out[1] = (double)M; out[2] = 0.0; out[3] = cost;
    out[4] = (double)used; out[5] = (double)longest; out[6] = (double)(nl - seen); out[7] = 0.0;
}

// ---- host side: pair_plan.h's plan, then per group dtw_dist (on the swapped sides) and align_sweep ----
size_t align_workspace_bytes(int32_t B, const int32_t* a_lens, const int32_t* b_lens, size_t cap) { return pair_workspace_bytes(kAlignOp, B, a_lens, b_lens, cap); }

int al_align(void* stream, const fs2_op_align_args* a) {
    const char* who = kAlignOp.who;
    if (const int rc = pair_check_args(kAlignOp, a)) return rc;
    if (a->max_step != 1 && a->max_step != 2) return fail(nullptr, FS2_ERR_ARG, "%s: max_step = %d, not 1 or 2", who, a->max_step);
    if (a->dur_stride < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative dur_stride", who);
    const int32_t B = a->B;
    if (B > 0 && !a->labels != !a->n_labels) return fail(nullptr, FS2_ERR_ARG, "%s: labels and n_labels must be given together", who);
    for (int b = 0; b < B; ++b) {
        if (a->labels && (a->n_labels[b] < 0 || a->n_labels[b] > a->dur_stride))
            return fail(nullptr, FS2_ERR_ARG, "%s: n_labels = %d of pair %d outside [0, dur_stride = %lld]", who, a->n_labels[b], b, (long long)a->dur_stride);
        if (!a->labels && a->a_lens[b] > a->dur_stride)
            return fail(nullptr, FS2_ERR_ARG, "%s: dur_stride = %lld below the %d states of pair %d", who, (long long)a->dur_stride, a->a_lens[b], b);
    }
    PairPlan p;
    if (const int rc = pair_plan(kAlignOp, a, a->labels ? a->n_labels : nullptr, p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)a->workspace;
    DtwPair* recs = p.at.recs;
    double* recs_out = p.at.terms;
    dtw_upload(p, s);
    // one dtw_dist and one align_sweep per group, in stream order: a group's matrices are dead when the next group's are written
    pair_groups(p, [&](const PairGroup& g) {
        dtw_launch_dist(p, g, recs, ws, s);
        hipLaunchKernelGGL(align_sweep, dim3((unsigned)g.count), dim3(kAlignThreads), 0, s, recs + g.first, a->max_step, a->labels, ws,
                           a->durations ? a->durations + (int64_t)g.first * a->dur_stride : nullptr, a->dur_stride, a->state,
                           recs_out + (size_t)g.first * kAlignTerms);
    });
    hipLaunchKernelGGL((records_combine<kAlignTerms, 2, -1>), dim3(1), dim3(256), 0, s, recs_out, B, a->terms, a->batch);
    return rec_finish(who);
}
