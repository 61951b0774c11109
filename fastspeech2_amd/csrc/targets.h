// Training targets from the per-frame energy and F0 arrays: the reference's remove_outlier (utils/util.py:26-49, applied to every
// energy and pitch array the data loader returns) and the corpus statistics of compute_statistics.py, behind
// fs2_op_clean_targets (include/fs2.h; tests/targets_oracle.py states the same in numpy).
// Not a header of its own: fs2_runtime.hip includes it inside its unnamed namespace, after fail() and align_up(); the checks, the
// workspace carve and the record upload are record_op.h's.  Plain HIP C++.
//
// Per utterance x (float32, n >= 1 values), every operation rounded to float32 on its own (nothing here may be contracted into a
// fused multiply-add: a fused p25 - 1.5 iqr decides a value that ties with the threshold the other way):
//   s = sort(x); for q in {1, 3}: h = q (n - 1), j = h / 4, g = (h % 4) / 4, a = s[j], b = s[min(j + 1, n - 1)], d = b - a,
//   p = g < 0.5 ? a + d g : b - d (1 - g)                                     (numpy's linear percentile: p25, p75)
//   w = 1.5 (p75 - p25), lower = p25 - w, upper = p75 + w; x[i] is an outlier iff x[i] <= lower or x[i] >= upper
//   M = max_i (outlier_i ? 0 : x[i]); y[i] = x[i] == 0 ? 0 : outlier_i ? M : x[i]
// An utterance with a NaN or an infinity is copied unchanged (quartiles NaN, 0 outliers) and left out of the statistics.
//
// tg_clean: one workgroup of 256 threads per utterance.  Values become order-preserving 32-bit keys (-0 as +0), staged in LDS when the
// utterance fits kTgStage values and re-read from global memory in every sweep when it does not (no limit on the length).  s[j] for
// both quartiles comes from a radix select: four passes of 8 bits, per pass a 256-bin histogram per quartile in LDS (integer adds:
// the counts do not depend on the order of the adds) and a prefix over the bins by one wave.  s[j + 1] is s[j] when more than j + 1
// values are <= s[j], else the smallest key above it (one more sweep with an integer LDS minimum).  A sweep then counts the outliers
// and finds M, a barrier follows, and the last sweep writes y (so y == x is legal) and gathers the statistics of y.  Sums are carried
// in double and reduced in a fixed tree (xor butterfly in the wave, then the four waves in order): no floating-point atomics, and an
// utterance's numbers depend on its own values only.  tg_combine folds the per-utterance records in a fixed order with Chan's update.

#include "record_op.h"
constexpr int kTgThreads = 256;
constexpr int kTgStage = 4096;            // keys of an utterance kept in LDS (16 KB); a longer one is re-read from global memory
constexpr int kTgRecsPerChunk = 500;      // (start, length) records per upload launch (kernel-argument bytes: 500 * 8 + 8 < 4 KB)
constexpr int kTgStats = 12;              // doubles of a statistics record

// A statistics record (the caller's `stats` and the per-utterance partials share the layout; include/fs2.h documents it)
enum { kTgNTotal = 0, kTgNOutliers, kTgNNonfinite, kTgNNoPositive, kTgN, kTgMin, kTgNonzeroMin, kTgMax, kTgMean, kTgStd, kTgM2, kTgReserved };

struct TgRec { int start, len; };

__device__ inline uint32_t tg_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u << 1) == 0 ? 0x80000000u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ inline float tg_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ inline double tg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int tg_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline float tg_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ inline float tg_wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// numpy's _lerp between the neighbours a = s[j], b = s[j + 1] at g = (h % 4) / 4 (g and 1 - g are exact).  Contraction is switched
// off here and in tg_thresholds: hipcc contracts by default (its __fmul_rn / __fadd_rn are plain operators), and a fused multiply-add
// rounds once where numpy rounds twice.
__device__ inline float tg_lerp(float a, float b, int h4) {
#pragma clang fp contract(off)
    const float g = 0.25f * (float)h4, d = b - a;
    const float dg = d * g, dh = d * (1.0f - g);
    return h4 < 2 ? a + dg : b - dh;
}

// w = 1.5 (p75 - p25) rounded to float32, then lower = p25 - w and upper = p75 + w: three roundings each, as the reference's
// is_outlier makes them.  A fused p25 - 1.5 iqr decides a value that ties with the threshold the other way.
__device__ inline void tg_thresholds(float p25, float p75, float& lower, float& upper) {
#pragma clang fp contract(off)
    const float iqr = p75 - p25;
    const float w = 1.5f * iqr;
    lower = p25 - w;
    upper = p75 + w;
}

__global__ __launch_bounds__(kTgThreads) void tg_clean(const TgRec* recs, const float* x, float* y, float* quartiles, int* n_outliers,
                                                       double* partials) {
    __shared__ uint32_t keys[kTgStage];
    __shared__ uint32_t hist[2][256];
    __shared__ uint32_t sel_prefix[2], sel_rank[2][2], sel_below[2], sel_equal[2], next_key[2];      // sel_rank[pass & 1]: read in a pass, written for the next
    __shared__ double red_d[3][4];
    __shared__ float red_f[4][4];          // [0]: M; [1 .. 3]: the extrema of the last sweep (slots of their own: no barrier lies between)
    __shared__ int red_i[3][4];
    const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const TgRec rec = recs[b];
    const uint32_t n = rec.len > 0 ? (uint32_t)rec.len : 0u;      // (unsigned: i += 256 must not overflow near 2^31 - 1 values)
    const float* xs = x + rec.start;
    float* ys = y + rec.start;
    double* part = partials + (size_t)b * kTgStats;
    if (n == 0) {                 // an empty utterance produces nothing: the identity record
        if (quartiles && tid < 2) quartiles[2 * b + tid] = __uint_as_float(0x7fc00000u);
        if (n_outliers && tid == 0) n_outliers[b] = 0;
        if (tid < kTgStats)
            part[tid] = (tid == kTgMin || tid == kTgNonzeroMin) ? (double)INFINITY : (tid == kTgMax ? -(double)INFINITY : 0.0);
        return;
    }
    const bool staged = n <= kTgStage;

    // ---- sweep 0: keys into LDS, any NaN / infinity ----
    int bad = 0;
    for (uint32_t i = tid; i < n; i += kTgThreads) {
        const float v = xs[i];
        bad |= !isfinite(v);
        if (staged) keys[i] = tg_key(v);
    }
    if (tid < 2) { sel_prefix[tid] = 0; next_key[tid] = 0xffffffffu; }
    if (tid == 0) { sel_rank[0][0] = (uint32_t)((int64_t)(n - 1) / 4); sel_rank[0][1] = (uint32_t)(3 * (int64_t)(n - 1) / 4); }
    bad = __syncthreads_or(bad);
    if (bad) {                    // copied unchanged, left out of the statistics
        for (uint32_t i = tid; i < n; i += kTgThreads) ys[i] = xs[i];
        if (quartiles && tid < 2) quartiles[2 * b + tid] = __uint_as_float(0x7fc00000u);
        if (n_outliers && tid == 0) n_outliers[b] = 0;
        if (tid < kTgStats)
            part[tid] = (tid == kTgMin || tid == kTgNonzeroMin) ? (double)INFINITY
                                                                 : (tid == kTgMax ? -(double)INFINITY : (tid == kTgNNonfinite ? 1.0 : 0.0));
        return;
    }
    auto key_at = [&](uint32_t i) { return staged ? keys[i] : tg_key(xs[i]); };

    // ---- radix select of s[j] for both quartiles: the digit of bits [shift, shift + 8) among the keys that share the prefix ----
    for (int shift = 24, pass = 0; shift >= 0; shift -= 8, ++pass) {
        hist[0][tid] = 0; hist[1][tid] = 0;
        __syncthreads();
        const uint32_t p0 = sel_prefix[0], p1 = sel_prefix[1];
        const uint32_t mask = shift == 24 ? 0u : ~0u << (shift + 8);
        for (uint32_t i = tid; i < n; i += kTgThreads) {
            const uint32_t k = key_at(i), dgt = (k >> shift) & 255u;
            if ((k & mask) == p0) atomicAdd(&hist[0][dgt], 1u);
            if ((k & mask) == p1) atomicAdd(&hist[1][dgt], 1u);
        }
        __syncthreads();
        if (wv == 0) {            // lane l owns bins 4 l .. 4 l + 3: an inclusive scan over the lanes, then the bin that holds the rank
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint32_t c0 = hist[q][4 * lane], c1 = hist[q][4 * lane + 1], c2 = hist[q][4 * lane + 2], c3 = hist[q][4 * lane + 3];
                uint32_t inc = c0 + c1 + c2 + c3;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(inc, o);
                    if (lane >= o) inc += up;
                }
                const uint32_t rank = sel_rank[pass & 1][q];
                uint32_t lo = inc - (c0 + c1 + c2 + c3);          // keys in the bins below this lane's
                const uint32_t cs[4] = {c0, c1, c2, c3};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (rank >= lo && rank < lo + cs[u]) {         // exactly one (lane, u): the counts sum to more than the rank
                        sel_prefix[q] |= (uint32_t)(4 * lane + u) << shift;
                        sel_rank[(pass + 1) & 1][q] = rank - lo;
                        sel_equal[q] = cs[u];                      // after the last pass: keys equal to s[j] ...
                        sel_below[q] = rank - lo;                  // ... and how many of them come before rank j
                    }
                    lo += cs[u];
                }
            }
        }
        __syncthreads();
    }
    // s[j + 1] = s[j] if a further equal key follows rank j, else the smallest key above s[j] (none: j = n - 1, then s[j] itself)
    const uint32_t k0 = sel_prefix[0], k1 = sel_prefix[1];
    const bool need0 = sel_below[0] + 1 >= sel_equal[0], need1 = sel_below[1] + 1 >= sel_equal[1];
    if (need0 || need1) {
        uint32_t m0 = 0xffffffffu, m1 = 0xffffffffu;
        for (uint32_t i = tid; i < n; i += kTgThreads) {
            const uint32_t k = key_at(i);
            if (k > k0) m0 = min(m0, k);
            if (k > k1) m1 = min(m1, k);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            m0 = min(m0, (uint32_t)__shfl_xor((int)m0, o));
            m1 = min(m1, (uint32_t)__shfl_xor((int)m1, o));
        }
        if (lane == 0) { atomicMin(&next_key[0], m0); atomicMin(&next_key[1], m1); }
        __syncthreads();
    }
    const int h1 = (int)((int64_t)(n - 1) % 4), h3 = (int)(3 * (int64_t)(n - 1) % 4);
    const bool last0 = (int64_t)(n - 1) / 4 >= n - 1, last1 = 3 * (int64_t)(n - 1) / 4 >= n - 1;      // j = n - 1 (n = 1 only)
    const float a0 = tg_value(k0), a1 = tg_value(k1);
    const float b0 = (need0 && !last0) ? tg_value(next_key[0]) : a0, b1 = (need1 && !last1) ? tg_value(next_key[1]) : a1;
    const float p25 = tg_lerp(a0, b0, h1), p75 = tg_lerp(a1, b1, h3);
    float lower, upper;
    tg_thresholds(p25, p75, lower, upper);

    // ---- sweep: outliers, M, and what the mean of the non-zero cleaned values needs ----
    float M = -INFINITY;          // max over (outlier ? 0 : x); an utterance of outliers only has M = 0
    int n_out = 0, n_out_nz = 0, n_kept_nz = 0;
    double sum_kept = 0.0;
    for (uint32_t i = tid; i < n; i += kTgThreads) {
        const float v = tg_value(key_at(i));
        const bool out = v <= lower || v >= upper;
        M = fmaxf(M, out ? 0.f : v);
        n_out += out;
        n_out_nz += out && v != 0.f;
        n_kept_nz += !out && v != 0.f;
        sum_kept += (!out && v != 0.f) ? (double)v : 0.0;
    }
    M = tg_wave_max(M);
    n_out = tg_wave_sum(n_out); n_out_nz = tg_wave_sum(n_out_nz); n_kept_nz = tg_wave_sum(n_kept_nz);
    sum_kept = tg_wave_sum(sum_kept);
    if (lane == 0) { red_f[0][wv] = M; red_i[0][wv] = n_out; red_i[1][wv] = n_out_nz; red_i[2][wv] = n_kept_nz; red_d[0][wv] = sum_kept; }
    __syncthreads();              // every read of x is done: y may be x from here on
    M = fmaxf(fmaxf(red_f[0][0], red_f[0][1]), fmaxf(red_f[0][2], red_f[0][3]));
    n_out = (red_i[0][0] + red_i[0][1]) + (red_i[0][2] + red_i[0][3]);
    n_out_nz = (red_i[1][0] + red_i[1][1]) + (red_i[1][2] + red_i[1][3]);
    n_kept_nz = (red_i[2][0] + red_i[2][1]) + (red_i[2][2] + red_i[2][3]);
    sum_kept = (red_d[0][0] + red_d[0][1]) + (red_d[0][2] + red_d[0][3]);
    const int n_nz = n_kept_nz + (M != 0.f ? n_out_nz : 0);       // cleaned values != 0: the outliers become M
    const double mean = n_nz ? (sum_kept + (M != 0.f ? (double)n_out_nz * (double)M : 0.0)) / (double)n_nz : 0.0;

    // ---- last sweep: write y; sum (y - mean)^2 and (y - mean) over y != 0, extrema of y ----
    double m2 = 0.0, sd = 0.0;
    float mn = INFINITY, nzmin = INFINITY, mx = -INFINITY;
    for (uint32_t i = tid; i < n; i += kTgThreads) {
        const float v = staged ? tg_value(keys[i]) : xs[i];
        const bool out = v <= lower || v >= upper;
        const float yv = v == 0.f ? 0.f : (out ? M : v);
        ys[i] = yv;
        if (yv != 0.f) {
            const double dv = (double)yv - mean;
            m2 += dv * dv;
            sd += dv;
        }
        mn = fminf(mn, yv); mx = fmaxf(mx, yv);
        if (yv > 0.f) nzmin = fminf(nzmin, yv);
    }
    m2 = tg_wave_sum(m2); sd = tg_wave_sum(sd);
    mn = tg_wave_min(mn); nzmin = tg_wave_min(nzmin); mx = tg_wave_max(mx);
    if (lane == 0) { red_d[1][wv] = m2; red_d[2][wv] = sd; red_f[1][wv] = mn; red_f[2][wv] = nzmin; red_f[3][wv] = mx; }
    __syncthreads();
    if (tid == 0) {
        m2 = (red_d[1][0] + red_d[1][1]) + (red_d[1][2] + red_d[1][3]);
        sd = (red_d[2][0] + red_d[2][1]) + (red_d[2][2] + red_d[2][3]);
        mn = fminf(fminf(red_f[1][0], red_f[1][1]), fminf(red_f[1][2], red_f[1][3]));
        nzmin = fminf(fminf(red_f[2][0], red_f[2][1]), fminf(red_f[2][2], red_f[2][3]));
        mx = fmaxf(fmaxf(red_f[3][0], red_f[3][1]), fmaxf(red_f[3][2], red_f[3][3]));
        if (quartiles) { quartiles[2 * b] = p25; quartiles[2 * b + 1] = p75; }
        if (n_outliers) n_outliers[b] = n_out;
        part[kTgNTotal] = (double)n;
        part[kTgNOutliers] = (double)n_out;
        part[kTgNNonfinite] = 0.0;
        part[kTgNNoPositive] = nzmin == INFINITY ? 1.0 : 0.0;
        part[kTgN] = (double)n_nz;
        part[kTgMin] = (double)mn;
        part[kTgNonzeroMin] = (double)nzmin;
        part[kTgMax] = (double)mx;
        part[kTgMean] = mean;
        part[kTgStd] = 0.0;
        part[kTgM2] = n_nz ? fmax(m2 - sd * sd / (double)n_nz, 0.0) : 0.0;      // the two-pass sum, corrected for the rounded mean
        part[kTgReserved] = 0.0;
    }
}

// (n, mean, M2) of two sets -> of their union (Chan, Golub, LeVeque 1979)
struct TgMoments { double n, mean, m2; };
__device__ inline TgMoments tg_chan(const TgMoments& a, const TgMoments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, delta = b.mean - a.mean;
    return {n, a.mean + delta * (b.n / n), (a.m2 + b.m2) + delta * delta * (a.n * b.n / n)};
}

// One workgroup folds the B per-utterance records into stats: thread t takes records t, t + 256, ... in order, then a fixed tree
// (lane l takes lane l + o for o = 32 .. 1, then thread 0 takes the four waves in order).  The same batch gives the same bits.
__global__ __launch_bounds__(kTgThreads) void tg_combine(const double* partials, int B, double* stats) {
    __shared__ double red[4][8];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    double cnt[4] = {0.0, 0.0, 0.0, 0.0};
    double mn = INFINITY, nzmin = INFINITY, mx = -INFINITY;
    TgMoments m{0.0, 0.0, 0.0};
    for (int b = tid; b < B; b += kTgThreads) {
        const double* p = partials + (size_t)b * kTgStats;
#pragma unroll
        for (int c = 0; c < 4; ++c) cnt[c] += p[c];
        mn = fmin(mn, p[kTgMin]); nzmin = fmin(nzmin, p[kTgNonzeroMin]); mx = fmax(mx, p[kTgMax]);
        m = tg_chan(m, TgMoments{p[kTgN], p[kTgMean], p[kTgM2]});
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) cnt[c] += __shfl_down(cnt[c], o);
        mn = fmin(mn, __shfl_down(mn, o)); nzmin = fmin(nzmin, __shfl_down(nzmin, o)); mx = fmax(mx, __shfl_down(mx, o));
        const TgMoments other{__shfl_down(m.n, o), __shfl_down(m.mean, o), __shfl_down(m.m2, o)};
        if (lane + o < 64) m = tg_chan(m, other);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) red[wv][c] = cnt[c];
        red[wv][4] = mn; red[wv][5] = nzmin; red[wv][6] = mx;
    }
    __shared__ TgMoments redm[4];
    if (lane == 0) redm[wv] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
#pragma unroll
            for (int c = 0; c < 4; ++c) cnt[c] += red[w][c];
            mn = fmin(mn, red[w][4]); nzmin = fmin(nzmin, red[w][5]); mx = fmax(mx, red[w][6]);
            m = tg_chan(m, redm[w]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) stats[c] = cnt[c];
        stats[kTgN] = m.n;
        stats[kTgMin] = mn; stats[kTgNonzeroMin] = nzmin; stats[kTgMax] = mx;
        stats[kTgMean] = m.mean;
        stats[kTgStd] = m.n > 0.0 ? sqrt(m.m2 / m.n) : 0.0;
        stats[kTgM2] = m.m2;
        stats[kTgReserved] = 0.0;
    }
}

// ---- host side: workspace = the (start, length) records, then one statistics record per utterance ----
struct TgLayout { TgRec* recs; double* partials; size_t bytes; };
inline TgLayout tg_layout(int32_t B, void* ws = nullptr) {
    Carve c{(char*)ws};
    TgLayout r{c.take<TgRec>(B), c.take<double>(B, kTgStats), 0};
    r.bytes = c.off;
    return r;
}
size_t tg_workspace_bytes(int32_t B) { return B < 0 ? 0 : tg_layout(B).bytes; }

int tg_clean_targets(void* stream, const float* x, int32_t B, const int32_t* starts, const int32_t* lens, void* workspace, size_t workspace_bytes,
                     float* y, float* quartiles, int32_t* n_outliers, double* stats) {
    const char* who = "fs2_op_clean_targets";
    if (B < 0 || (B > 0 && (!starts || !lens))) return fail(nullptr, FS2_ERR_ARG, "%s: bad batch (B = %d) or null starts / lens", who, B);
    if (const int rc = rec_check_rows(who, "utterance", B, starts, lens)) return rc;
    if (B == 0 && !stats) return FS2_OK;
    if (std::any_of(lens, lens + B, [](int32_t n) { return n > 0; }) && (!x || !y)) return fail(nullptr, FS2_ERR_ARG, "%s: null x / y", who);
    const TgLayout at = tg_layout(B, workspace);      // (B = 0: no workspace, and tg_combine reads none)
    if (const int rc = rec_check_workspace(who, B, workspace, workspace_bytes, at.bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    auto up = rec_uploader<TgRec, kTgRecsPerChunk>(B, at.recs, s);
    for (int b = 0; b < B; ++b) up.put(b, TgRec{starts[b], lens[b]});
    if (B > 0) hipLaunchKernelGGL(tg_clean, dim3((unsigned)B), dim3(kTgThreads), 0, s, at.recs, x, y, quartiles, n_outliers, at.partials);
    if (stats) hipLaunchKernelGGL(tg_combine, dim3(1), dim3(kTgThreads), 0, s, at.partials, B, stats);
    return rec_finish(who);
}
