// HBM-bound kernels of the path (the row metadata is layout.h's): embedding + positional encoding, duration post-op,
// length regulator (prefix sum + expand), bucketize + embedding add, packed -> padded output copies.
// All of them move whole rows with 16-byte accesses, one wavefront per row.
#pragma once
#include "common.h"
#include "layout_rule.h"
#include "row_step_args.h"

namespace fs2 {

// h[row] = E[xs[b, t]] * xscale + alpha * pe[t]      (reference encoder.py:196, embedding.py:77-80,105-120)
__global__ __launch_bounds__(256) void embed_pe(const int64_t* xs, int Tmax, const float* E, int idim, int D,
                                                const float* pe, const float* alpha_p, float xscale,
                                                const int* row_pos, const int* row_seq, int R, float* h, void* planes = nullptr) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    const int t = row_pos[row];
    float* dst = h + (size_t)row * D;
    if (t < 0) {
        for (int c = lane * 4; c < D; c += 256) {
            *reinterpret_cast<float4*>(dst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (planes) store_planes4(planes, row, D / 32, c, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    const int b = row_seq[row];
    int64_t id = (t < Tmax) ? xs[(size_t)b * Tmax + t] : 0;
    if (id < 0 || id >= idim) id = 0;
    const float alpha = alpha_p ? alpha_p[0] : 1.f;
    const float* e = E + (size_t)id * D;
    const float* p = pe + (size_t)t * D;
    for (int c = lane * 4; c < D; c += 256) {
        const float4 ev = *reinterpret_cast<const float4*>(e + c);
        const float4 pv = *reinterpret_cast<const float4*>(p + c);
        float4 o;
        o.x = ev.x * xscale + alpha * pv.x;
        o.y = ev.y * xscale + alpha * pv.y;
        o.z = ev.z * xscale + alpha * pv.z;
        o.w = ev.w * xscale + alpha * pv.w;
        *reinterpret_cast<float4*>(dst + c) = o;
        if (planes) store_planes4(planes, row, D / 32, c, f32x4{o.x, o.y, o.z, o.w});
    }
}

// d = clamp(round_half_even(exp(y) - 1), 0) as int64 (reference duration_predictor.py:77-81: torch.clamp(torch.round(xs.exp() -
// offset), min=0).long()).  rintf = round half to even (torch.round); +inf and values beyond the int64 range saturate.
__device__ __forceinline__ int64_t duration_from_log(float y) {
    const float f = fmaxf(rintf(expf(y) - 1.0f), 0.f);
    return (f >= 9.0e18f) ? INT64_MAX : (int64_t)f;      // (NaN: fmaxf returns 0)
}

__global__ void duration_kernel(const float* d_log, int64_t n, int64_t* d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = duration_from_log(d_log[i]);
}

// Duration post-op (reference duration_predictor.py:77-84): packed per-row log-durations ->
// padded [B,Tmax] outputs; d = clamp(round_half_even(exp(y) - 1), 0), pads -> 0.
__global__ void dur_finalize(const float* dlog_rows, const int* start, const int* vlen, int B, int Tmax,
                             float* d_log, int64_t* d_int, int64_t* d_int2 = nullptr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Tmax) return;
    const int b = i / Tmax, t = i - b * Tmax;
    float y = 0.f;
    int64_t d = 0;
    if (t < vlen[b]) {
        y = dlog_rows[start[b] + t];
        d = duration_from_log(y);
    }
    if (d_log) d_log[i] = y;
    if (d_int) d_int[i] = d;
    if (d_int2) d_int2[i] = d;      // the caller's copy (saves a device-to-device memcpy launch)
}

// Per-utterance inclusive prefix sum of the durations actually used (reference length_regulator.py:60,
// 85-88: slice to ilen, an all-zero row becomes all ones).  One workgroup per utterance.
// alpha: the length regulator's speed control (length_regulator.py:57-59): d <- round_half_even(float(d) * alpha) when alpha != 1.
// A duration beyond the int range saturates at kDurMax (duration_from_log saturates at INT64_MAX for +inf; a caller's ds may hold anything): narrowed blindly, 2^32 + 5
// frames became 5 and INT64_MAX became -1, and the utterance came back with a small positive frame count.
constexpr int kDurMax = 0x7fffffff;
__device__ __forceinline__ int scaled_duration(int64_t d, float alpha) {
    if (d <= 0) return 0;
    if (alpha == 1.0f) return d > kDurMax ? kDurMax : (int)d;
    const float f = rintf((float)d * alpha);
    return f > 0.f ? (f >= 2147483648.f ? kDurMax : (int)f) : 0;
}

// ids != nullptr (fs2_encode): an utterance whose row of xs (all Tmax positions, pads included) holds a phoneme id outside [0, idim) gets the frame count -1 -- the reference's
// torch.nn.Embedding raises for it (fastspeech.py:65-67, core/encoder.py:196); embed_pe reads row 0 instead of indexing out of range, and
// the marker reaches the caller with the frame counts it reads anyway (host-driven layout) or as FS2_OVF_BAD_ID in the status word of
// fs2_decode's device-driven layout (frame_layout_dev), whose outputs are then NaN-filled.
// An utterance whose durations sum beyond the int range gets the frame count kDurMax (the total is formed in 64 bits and saturates; its cum entries are then
// meaningless): no positional table and no row capacity holds it, so fs2_decode refuses it (host-driven layout) or flags it (FS2_OVF_LMAX / _PE) instead of
// running on a wrapped count.
// scum != nullptr (FS2_VARSHORT): beside cum, the running sums of the SHORT durations min(d, K) (layout_rule.h) and, in so32[b], their total.
__global__ __launch_bounds__(256) void dur_scan(const int64_t* ds, int Tmax, const int* ilen, int* cum,
                                                int64_t* olens, int* olens32, float alpha = 1.0f, const int64_t* ids = nullptr, int idim = 0,
                                                int* scum = nullptr, int* so32 = nullptr, int K = 0) {
    __shared__ int wsum[4], wsum2[4];
    __shared__ long long wtot[4];
    __shared__ int carry_s, carry2_s;
    __shared__ int bad_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = ilen[b];
    const int64_t* d = ds + (size_t)b * Tmax;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    // pass 1: total
    long long tot = 0;
    int bad = 0;
    for (int t = tid; t < T; t += 256) tot += scaled_duration(d[t], alpha);
    // (ALL Tmax positions of the row, pads included: the reference's nn.Embedding indexes the whole padded xs, so an id outside [0, idim) in the pad
    //  region -- a -1 padding convention, say -- raises there too; round-5 advisor finding)
    if (ids != nullptr)
        for (int t = tid; t < Tmax; t += 256) { const int64_t id = ids[(size_t)b * Tmax + t]; bad |= (id < 0 || id >= idim) ? 1 : 0; }
    if (bad) bad_s = 1;
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (lane == 0) wtot[wave] = tot;
    __syncthreads();
    const long long total64 = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    const int total = total64 > kDurMax ? kDurMax : (int)total64;
    const bool ones = (total == 0);
    __syncthreads();
    if (tid == 0) { carry_s = 0; carry2_s = 0; }
    __syncthreads();
    for (int base = 0; base < T; base += 256) {
        const int t = base + tid;
        int v = (t < T) ? (ones ? 1 : scaled_duration(d[t], alpha)) : 0;
        int x = v, x2 = vs_short_dur(v, K);   // inclusive scans inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o), y2 = __shfl_up(x2, o);
            if (lane >= o) { x += y; x2 += y2; }
        }
        if (lane == 63) { wsum[wave] = x; wsum2[wave] = x2; }
        __syncthreads();
        int off = carry_s, off2 = carry2_s;
        for (int w = 0; w < wave; ++w) { off += wsum[w]; off2 += wsum2[w]; }
        if (t < T) cum[(size_t)b * Tmax + t] = off + x;
        if (scum && t < T) scum[(size_t)b * Tmax + t] = off2 + x2;
        __syncthreads();
        if (tid == 255) { carry_s = off + x; carry2_s = off2 + x2; }
        __syncthreads();
    }
    if (tid == 0) {
        const int tt = bad_s ? -1 : (ones ? T : total);
        if (olens) olens[b] = tt;
        if (olens32) olens32[b] = tt;
        if (so32) so32[b] = carry2_s;
    }
}

// The token a frame belongs to: idx = #{i : cum[b,i] <= j} (first i with cum[b,i] > j); -1 for gap rows and frames beyond the utterance.
__device__ __forceinline__ int lr_token_index(int b, int j, const int* cum, int Tmax, const int* ilen, const int* vlen) {
    if (b < 0 || j < 0 || j >= vlen[b]) return -1;
    const int* c = cum + (size_t)b * Tmax;
    int lo = 0, hi = ilen[b];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The length regulator's index output and nothing else (one thread per row): what is left of it where every consumer of the expanded rows
// gathers from token-level products instead (var_gather0 / dec_in_gather below).
__global__ void lr_index_only(const int* cum, int Tmax, const int* ilen, const int* row_pos, const int* row_seq, const int* vlen, int R, int* index_rows) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= R) return;
    index_rows[row] = lr_token_index(row_seq[row], row_pos[row], cum, Tmax, ilen, vlen);
}

// Length-regulator expand (reference length_regulator.py:90-95 + utils/util.py:91-104):
// out[row] = hs[tok_start[b] + idx], idx = #{i : cum[b,i] <= j}; rows beyond the utterance -> 0.
// One wavefront per output row.  If row_seq == nullptr the output is a dense [B, uniform_len] layout.
__global__ __launch_bounds__(256) void lr_expand(const float* hs, int D, const int* tok_start, const int* ilen,
                                                 const int* cum, int Tmax, const int* row_pos, const int* row_seq,
                                                 int uniform_len, const int* vlen, int R, float* out,
                                                 int* index_rows, void* planes = nullptr) {     // planes: also as split-bf16 planes (D / 32 chunks)
    // (the row as a scalar: everything up to the copy -- utterance, position, the binary search over the duration sums -- is then scalar
    //  loads and SALU, a chain of K$ round trips instead of vector-memory ones)
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    int b, j;
    if (row_seq) { b = row_seq[row]; j = row_pos[row]; } else { b = row / uniform_len; j = row - b * uniform_len; }
    float* dst = out + (size_t)row * D;
    int idx = -1;
    if (b >= 0 && j < vlen[b]) {
        const int* c = cum + (size_t)b * Tmax;
        int lo = 0, hi = ilen[b];   // first i with c[i] > j
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] <= j) lo = mid + 1; else hi = mid;
        }
        idx = lo;
    }
    if (index_rows && lane == 0) index_rows[row] = idx;
    if (idx < 0) {
        for (int c4 = lane * 4; c4 < D; c4 += 256) {
            *reinterpret_cast<float4*>(dst + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (planes) store_planes4(planes, row, D / 32, c4, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    const float* src = hs + (size_t)(tok_start[b] + idx) * D;
    for (int c4 = lane * 4; c4 < D; c4 += 256) {
        const float4 v = *reinterpret_cast<const float4*>(src + c4);
        *reinterpret_cast<float4*>(dst + c4) = v;
        if (planes) store_planes4(planes, row, D / 32, c4, f32x4{v.x, v.y, v.z, v.w});
    }
}

// torch.bucketize(x, bins, right=False): first i with x <= bins[i]; NaN -> nb (the `!(b >= x)` form keeps
// torch's NaN behaviour).  reference variance_predictor.py:158,231
__device__ __forceinline__ int bucket_index(float x, const float* bins, int nb) {
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!(bins[mid] >= x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void bucketize_kernel(const float* x, int64_t n, const float* bins, int nb, int* idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = bucket_index(x[i], bins, nb);
}

// Variance adaptor tail (reference fastspeech.py:218-219 with the one-hot GEMMs collapsed to gathers):
// h[row] = (h[row] + Tp[qp]) + Te[qe], Tx[q][c] = fl(W[c][q] + b[c]) precomputed at weight load, which is
// bit-identical to one_hot(q) @ W^T + b.  e/p come from the caller ([B, stride], teacher forcing) or from
// the predictors (per packed row).  One wavefront per row.
__global__ __launch_bounds__(256) void bucket_embed(float* h, int D, const int* row_pos, const int* row_seq, int R,
                                                    const float* es, int es_stride, const float* ps, int ps_stride,
                                                    const float* e_rows, const float* p_rows,
                                                    const float* ebins, const float* pbins, int nb,
                                                    const float* Te, const float* Tp, int* qe_rows, int* qp_rows, void* planes = nullptr) {
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));      // (scalar: the two bin searches become scalar-load chains)
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    const int j = row_pos[row];
    if (j < 0) {
        if (lane == 0) { if (qe_rows) qe_rows[row] = -1; if (qp_rows) qp_rows[row] = -1; }
        if (planes)
            for (int c = lane * 4; c < D; c += 256) store_planes4(planes, row, D / 32, c, f32x4{0.f, 0.f, 0.f, 0.f});
        return;
    }
    const int b = row_seq[row];
    const float e = es ? (j < es_stride ? es[(size_t)b * es_stride + j] : 0.f) : e_rows[row];
    const float p = ps ? (j < ps_stride ? ps[(size_t)b * ps_stride + j] : 0.f) : p_rows[row];
    const int qe = bucket_index(e, ebins, nb);
    const int qp = bucket_index(p, pbins, nb);
    if (lane == 0) { if (qe_rows) qe_rows[row] = qe; if (qp_rows) qp_rows[row] = qp; }
    float* dst = h + (size_t)row * D;
    const float* te = Te + (size_t)qe * D;
    const float* tp = Tp + (size_t)qp * D;
    for (int c = lane * 4; c < D; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(dst + c);
        const float4 a = *reinterpret_cast<const float4*>(tp + c);
        const float4 g = *reinterpret_cast<const float4*>(te + c);
        v.x = (v.x + a.x) + g.x;
        v.y = (v.y + a.y) + g.y;
        v.z = (v.z + a.z) + g.z;
        v.w = (v.w + a.w) + g.w;
        *reinterpret_cast<float4*>(dst + c) = v;
        if (planes) store_planes4(planes, row, D / 32, c, f32x4{v.x, v.y, v.z, v.w});
    }
}

// ---- multiply before expanding (fs2_runtime.hip: tok.proj): the two kernels below gather the token-level products per frame (row_step_args.h: TokGatherArgs) ----

// First layer of both variance predictors from the token-level products: y[f] = P0[tok(f-1)] + P1[tok(f)] + P2[tok(f+1)] + b -> ReLU -> LayerNorm(1e-12),
// written as split-bf16 planes at the column offset of the group.  A neighbour that is a gap row or lies beyond the utterance contributes zero, as the
// zero rows of the expanded tensor did; rows that are no frame (row_pos < 0) become zero rows.  One wavefront per (row, predictor).
__global__ __launch_bounds__(256) void var_gather0(TokGatherArgs a) {
    const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int row = unit >> 1, grp = unit & 1;
    const int lane = threadIdx.x & 63;
    if (row >= a.R) return;
    const int N = a.chans, co = grp * N, nch = 2 * N / 32;
    if (a.row_pos[row] < 0) {
        for (int c = lane * 4; c < N; c += 256) store_planes4(a.vp, row, nch, co + c, f32x4{0.f, 0.f, 0.f, 0.f});
        return;
    }
    const int t0 = a.tok_start[a.row_seq[row]];
    const float* src[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int r = row + d - 1;
        const int tk = (r >= 0 && r < a.R) ? a.lri[r] : -1;
        src[d] = tk >= 0 ? a.P + (size_t)(t0 + tk) * a.ldp + d * 2 * N + co : nullptr;
    }
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j * 256;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < N) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (src[d]) {
                    const float4 q = *reinterpret_cast<const float4*>(src[d] + c);
                    v[j].x += q.x; v[j].y += q.y; v[j].z += q.z; v[j].w += q.w;
                }
            const float4 b = *reinterpret_cast<const float4*>(a.bias + co + c);
            v[j].x = fmaxf(v[j].x + b.x, 0.f); v[j].y = fmaxf(v[j].y + b.y, 0.f); v[j].z = fmaxf(v[j].z + b.z, 0.f); v[j].w = fmaxf(v[j].w + b.w, 0.f);
        }
        s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)N;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j * 256;
        if (c < N) {
            const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.f / sqrtf(q / (float)N + 1e-12f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j * 256;
        if (c < N) {
            const float4 g = *reinterpret_cast<const float4*>(a.ln_g + co + c);
            const float4 b = *reinterpret_cast<const float4*>(a.ln_b + co + c);
            store_planes4(a.vp, row, nch, co + c, f32x4{(v[j].x - mean) * rstd * g.x + b.x, (v[j].y - mean) * rstd * g.y + b.y,
                                                      (v[j].z - mean) * rstd * g.z + b.z, (v[j].w - mean) * rstd * g.w + b.w});
        }
    }
}

// Variance-adaptor tail and decoder input layer from the token-level products (replaces bucket_embed + the input layer's GEMM):
// bucket search with bucket_embed's rule, then (P[tok, dec.in columns] + TP[qp]) + TE[qe] -> LayerNorm(1e-5) -> ReLU -> * x_scale + alpha pe[pos].
// A frame row without a token (padded-batch semantics: positions beyond the utterance) has a zero first term, as its zero row had.  One wavefront per row.
__global__ __launch_bounds__(256) void dec_in_gather(TokGatherArgs a) {
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));      // (scalar: the two bin searches become scalar-load chains)
    const int lane = threadIdx.x & 63;
    if (row >= a.R) return;
    const int D = a.D, nch = D / 32;
    const int pos = a.row_pos[row];
    float* y = a.x0 ? a.x0 + (size_t)row * D : nullptr;
    if (pos < 0) {
        if (lane == 0) { if (a.qe_rows) a.qe_rows[row] = -1; if (a.qp_rows) a.qp_rows[row] = -1; }
        for (int c = lane * 4; c < D; c += 256) {
            if (y) *reinterpret_cast<float4*>(y + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            store_planes4(a.x0p, row, nch, c, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }
    const int b = a.row_seq[row];
    const int sr = a.f2s ? a.f2s[row] : -1;
    const bool e_short = a.sqe && sr >= 0, p_short = a.sqp && sr >= 0;
    const float e = a.es ? (pos < a.es_stride ? a.es[(size_t)b * a.es_stride + pos] : 0.f) : (a.sqe ? 0.f : a.e_rows[row]);
    const float p = a.ps ? (pos < a.ps_stride ? a.ps[(size_t)b * a.ps_stride + pos] : 0.f) : (a.sqp ? 0.f : a.p_rows[row]);
    const int qe = e_short ? a.sqe[sr] : bucket_index(e, a.ebins, a.nb);
    const int qp = p_short ? a.sqp[sr] : bucket_index(p, a.pbins, a.nb);
    if (lane == 0) { if (a.qe_rows) a.qe_rows[row] = qe; if (a.qp_rows) a.qp_rows[row] = qp; }
    const int tk = a.lri[row];
    const float* ph = tk >= 0 ? a.P + (size_t)(a.tok_start[b] + tk) * a.ldp + a.col0 : nullptr;
    const float* te = a.TE + (size_t)qe * D;
    const float* tp = a.TP + (size_t)qp * D;
    float4 v[4];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j * 256;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < D) {
            if (ph) v[j] = *reinterpret_cast<const float4*>(ph + c);
            const float4 g = *reinterpret_cast<const float4*>(tp + c);
            const float4 h = *reinterpret_cast<const float4*>(te + c);
            v[j].x = (v[j].x + g.x) + h.x; v[j].y = (v[j].y + g.y) + h.y; v[j].z = (v[j].z + g.z) + h.z; v[j].w = (v[j].w + g.w) + h.w;
        }
        s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j * 256;
        if (c < D) {
            const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.f / sqrtf(q / (float)D + 1e-5f);
    const float alpha = a.pe_alpha ? a.pe_alpha[0] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j * 256;
        if (c < D) {
            const float4 g = *reinterpret_cast<const float4*>(a.ln_g2 + c);
            const float4 bt = *reinterpret_cast<const float4*>(a.ln_b2 + c);
            const float4 pv = *reinterpret_cast<const float4*>(a.pe + (size_t)pos * D + c);
            float4 t;
            t.x = fmaxf((v[j].x - mean) * rstd * g.x + bt.x, 0.f) * a.x_scale + alpha * pv.x;
            t.y = fmaxf((v[j].y - mean) * rstd * g.y + bt.y, 0.f) * a.x_scale + alpha * pv.y;
            t.z = fmaxf((v[j].z - mean) * rstd * g.z + bt.z, 0.f) * a.x_scale + alpha * pv.z;
            t.w = fmaxf((v[j].w - mean) * rstd * g.w + bt.w, 0.f) * a.x_scale + alpha * pv.w;
            if (y) *reinterpret_cast<float4*>(y + c) = t;
            store_planes4(a.x0p, row, nch, c, f32x4{t.x, t.y, t.z, t.w});
        }
    }
}

// tap `tap` of a convolution weight [N][C][k] as a Linear weight [N][C] (load time: the rows of tok.proj's stacked weight)
__global__ void conv_tap_rows(const float* w, int N, int C, int k, int tap, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N * C) out[i] = w[(size_t)i * k + tap];
}

// packed rows [R, W] -> padded [B, Lout, W]; positions >= limit[b] are filled with `fill`.
template <typename T>
__global__ void unpack_rows(const T* src, int W, const int* start, const int* limit, int B, int Lout, T* dst, T fill) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)B * Lout * W;
    if (i >= total) return;
    const int w = (int)(i % W);
    const int64_t bj = i / W;
    const int j = (int)(bj % Lout), b = (int)(bj / Lout);
    dst[i] = (j < limit[b]) ? src[(size_t)(start[b] + j) * W + w] : fill;
}

// the same for float rows with W % 4 == 0 (the mel outputs: W = 80): 16-byte accesses, one (row, 4 channels) piece per thread
// ovf (device-driven layout): the overflow flags of the call; when set the outputs of the call do not exist -> NaN instead of zeros
__global__ void unpack_rows4(const float* src, int W4, const int* start, const int* limit, int B, int Lout, float* dst, const int* ovf = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * Lout * W4) return;
    const int w = (int)(i % W4);
    const int64_t bj = i / W4;
    const int j = (int)(bj % Lout), b = (int)(bj / Lout);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ovf && *ovf != 0) { const float q = __builtin_nanf(""); v = make_float4(q, q, q, q); }
    else if (j < limit[b]) v = reinterpret_cast<const float4*>(src)[(size_t)(start[b] + j) * W4 + w];
    reinterpret_cast<float4*>(dst)[i] = v;
}

// gapped packed rows -> dense packed rows (valid frames only, utterances back to back): dst row cum_scale cum[b] + j
// (ovf as in unpack_rows4; dst then holds R rows: the row capacity).  cum_scale: the reduction factor when the rows are mel frames
// (r per decoder frame) and cum[] counts decoder frames.
__global__ void pack_rows(const float* src, int W, const int* row_pos, const int* row_seq, const int* vlen, const int* cum, int R,
                          float* dst, const int* ovf = nullptr, int cum_scale = 1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int w4 = W / 4;
    if (i >= (int64_t)R * w4) return;
    if (ovf && *ovf != 0) { const float q = __builtin_nanf(""); reinterpret_cast<float4*>(dst)[i] = make_float4(q, q, q, q); return; }
    const int row = (int)(i / w4), c = (int)(i - (int64_t)row * w4) * 4;
    const int b = row_seq[row];
    if (b < 0) return;
    const int j = row_pos[row];
    if (j >= vlen[b]) return;
    *reinterpret_cast<float4*>(dst + ((size_t)cum[b] * cum_scale + j) * W + c) = *reinterpret_cast<const float4*>(src + (size_t)row * W + c);
}

// split-bf16 planes [R][nchunks x 128 B] -> fp32 rows [R][ld] (hi + lo, exact): what fs2_op_attention hands back when asked to run
// the attention kernels in the model's output form (FS2_OP_ATT_PLANES: the context leaves the kernel as planes only)
__global__ void planes_to_rows(const void* planes, int nchunks, int R, int D, float* dst, int ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int d4 = D / 4;
    if (i >= (int64_t)R * d4) return;
    const int row = (int)(i / d4), c = (int)(i - (int64_t)row * d4) * 4;
    const char* p = reinterpret_cast<const char*>(planes) + plane_byte((size_t)row, nchunks, c);
    const bf16x4_t h = *reinterpret_cast<const bf16x4_t*>(p), l = *reinterpret_cast<const bf16x4_t*>(p + 64);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)h[j] + (float)l[j];
    *reinterpret_cast<f32x4*>(dst + (size_t)row * ld + c) = v;
}

// device-driven layout: when the overflow flags (dims[2]) are set the outputs of the call are invalid -> fill them with NaN
__global__ void poison_on_overflow(const int* dims, float* a, int64_t na, float* b, int64_t nb, float* c, int64_t nc) {
    if (dims[2] == 0) return;
    const float q = __builtin_nanf("");
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < na; i += stride) a[i] = q;
    for (int64_t i = i0; i < nb; i += stride) b[i] = q;
    for (int64_t i = i0; i < nc; i += stride) c[i] = q;
}

// [N, W] -> [W, N] through a 32 x 33 LDS tile (coalesced on both sides)
__global__ __launch_bounds__(256) void transpose_rows(const float* src, int64_t N, int W, float* dst) {
    __shared__ float t[32][33];
    const int64_t n0 = (int64_t)blockIdx.x * 32;
    const int w0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int64_t n = n0 + r; const int w = w0 + tx;
        t[r][tx] = (n < N && w < W) ? src[n * W + w] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int w = w0 + r; const int64_t n = n0 + tx;
        if (w < W && n < N) dst[(int64_t)w * N + n] = t[tx][r];
    }
}

// ---- weight repacking (run once per load_state_dict) ----
// conv / linear weight [N][C][k] -> [Npad][k][Cpad] (fs2_runtime.hip: gemm_rows_from restates this row stride), zero padded, optionally scaled per output channel by
// gamma / sqrt(var + eps) (eval-mode BatchNorm folded into the Postnet convs, reference modules.py:285-348).
// ldw: elements between consecutive output rows of the source (0: C; larger for a column slice of a wider Linear weight, k = 1).
__global__ void repack_weight(const float* w, int N, int C, int k, int Npad, int Cpad, const float* bn_g,
                              const float* bn_v, float bn_eps, float* out, int ldw = 0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)Npad * k * Cpad;
    if (i >= total) return;
    const int c = (int)(i % Cpad);
    const int tap = (int)((i / Cpad) % k);
    const int n = (int)(i / ((int64_t)Cpad * k));
    float v = 0.f;
    if (n < N && c < C) {
        v = w[((size_t)n * (ldw ? ldw : C) + c) * k + tap];
        if (bn_g) v *= bn_g[n] / sqrtf(bn_v[n] + bn_eps);
    }
    out[i] = v;
}

// folded BatchNorm bias: beta - mean * gamma / sqrt(var + eps)
__global__ void bn_fold_bias(const float* g, const float* b, const float* m, const float* v, float eps, int N, float* out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) out[n] = b[n] - m[n] * (g[n] / sqrtf(v[n] + eps));
}

// embedding table of a Linear applied to one-hot rows: T[q][c] = W[c][q] + b[c]
__global__ void onehot_table(const float* W, const float* bias, int D, int nbins, float* T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * nbins) return;
    const int c = i % D, q = i / D;
    T[i] = W[(size_t)c * nbins + q] + bias[c];
}

}  // namespace fs2
