// Phase-continuity initial phase for Griffin-Lim (Single Pass Spectrogram Inversion: Beauregard, Harish and Wyse 2015), from the
// magnitudes alone: fs2_op_spsi_phase_geom / fs2_op_spsi_phase_dev (include/fs2.h).  The phase goes to
// gl_prologue through the init_phase pointer it has always had; no kernel of griffin_lim.h changes.
//
// Semantics (tests/spsi_oracle.py states them in numpy; the results are equal bit for bit).  Per utterance, M [L, NB] float32,
// phases in turns, acc[NB] = 0 before frame 0; every operation rounded to float32 on its own, no fused multiply-add.  For row m:
//   peak j, 1 <= j <= NB - 2: m[j] > m[j-1] and m[j] > m[j+1].  A non-peak bin b is rising iff m[b] < m[b+1], falling iff m[b] < m[b-1].
//   owner of a non-peak bin: the nearest peak to its right if every bin from it up to that peak is rising; else the nearest peak to
//   its left if every bin from it down to that peak is falling; else none.  Bins 0 and NB - 1: none.  A peak owns itself.
//   peak j, a, b, c = m[j-1], m[j], m[j+1]: den = (a - 2 b) + c; p = den != 0 ? (0.5 (a - c)) / den : 0;
//     w = float((hop j) mod n_fft) / n_fft + p float(hop / n_fft); pk = acc[j] + w; pk -= floorf(pk); right = c > a
//   bin k owned by j, d = k - j: new[k] = pk + h, - 1 if >= 1; h = 0.5 if right and (d == 1 or d < 0), or not right and (d == -1 or
//     d > 0); else 0 (the peak itself: 0).  Unowned: new[k] = acc[k].  Then acc <- new, phase[t][k] = acc[k] * 6.28318548f.
//
// Work split.  Only acc chains the frames; everything else is per row.
//   spsi_analyse  one workgroup per kSpsiTile workspace rows: M (from mel rows as max(P . exp(mel), 0), or copied) into LDS, the
//                 rising / falling / peak flags as 64-bit masks (one ballot per 64 bins), then per bin the owner by a find-first-set
//                 in the masks (no walk over bins), the half-turn flag and the owner's w: 2 + 4 bytes per bin into the workspace.
//   spsi_chain    one workgroup per utterance, acc double-buffered in LDS: per frame one gather acc[owner], one add, one wrap, one
//                 barrier, and the phase row is written.  The 6 bytes per bin of the next kSpsiAhead frames are loaded into
//                 registers before the current kSpsiAhead frames are stepped, so the loop never waits on HBM per frame.
// An utterance's result depends on its own rows alone: it is the same bits alone or in any batch, packed or padded.  No atomics.
//
// Budget from shapes at c3 (35.6 k frames, 64 utterances, longest ~1,000): spsi_analyse reads 35.6 k x 320 B of mels and the 164 KB of
// P once per 16 frames from L2 (~0.37 GB), writes 35.6 k x 513 x 6 B = 110 MB: tens of us.  spsi_chain is latency: ~1,000 frames x
// (LDS gather + barrier, a few hundred cycles) on 64 of the 256 CUs: of the order of 0.1 - 0.2 ms.  Measured: BASELINE.md section 5.8.
//
// Plain HIP C++, restricted to what tests/kernel_standin/hip_standin.h provides plus the wave ballot (tests/kernel_standin/spsi_main.cpp);
// fs2_runtime.hip includes it after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

namespace fs2 {

constexpr int kSpsiThreads = 256, kSpsiTile = 16, kSpsiAhead = 8, kSpsiMaxMels = 128;
constexpr int kSpsiUttsPerChunk = 240;                  // records per upload launch (kernel-argument bytes: 240 * 16 + 16 < 4 KB)
constexpr unsigned kSpsiNone = 0x7FFFu, kSpsiHalf = 0x8000u;     // owner word: bin of the owner | kSpsiHalf, or kSpsiNone

// One utterance: L rows from src_row0 of the caller's source (and phase, and mag_out), from ws_row0 of the workspace (prefix sum of L).
struct SpsiUtt {
    int src_row0, ws_row0, L, pad;
};
struct SpsiUttChunk {
    int n, base, frames, pad;
    SpsiUtt u[kSpsiUttsPerChunk];
};
// hdr[0] = workspace rows in use (sum of L), hdr[1] = flags (FS2_OVF_*; != 0: every record is empty and nothing is computed)
constexpr int kSpsiHdrInts = 4;

// Host-planned call: records from kernel arguments (no host copy, no synchronisation).
__global__ void spsi_upload(SpsiUttChunk c, SpsiUtt* utt, int* hdr) {
    const int i = threadIdx.x;
    if (i < c.n) utt[c.base + i] = c.u[i];
    if (i == 0 && c.base == 0) { hdr[0] = c.frames; hdr[1] = 0; hdr[2] = 0; hdr[3] = 0; }
}

// Device-driven call, one workgroup: validates the frame counts before anything is indexed with them, then writes the records.
// Thread t owns the utterances [t per, (t + 1) per); a length is clamped to [0, frame_capacity + 1] before it enters a sum, so no sum
// overflows whatever lens holds.  Flags as gl_plan_scan's (griffin_lim.h): 64 negative, 1 rows, 2 longer than src_stride, 32 | upstream.
__global__ __launch_bounds__(kSpsiThreads) void spsi_plan(const int64_t* lens, const int32_t* upstream, int B, int src_stride, int64_t frame_capacity,
                                                         SpsiUtt* utt, int* hdr) {
    __shared__ int64_t sL[kSpsiThreads];
    __shared__ int sF[kSpsiThreads];
    const int tid = threadIdx.x, per = (B + kSpsiThreads - 1) / kSpsiThreads;
    const int b0 = min(B, tid * per), b1 = min(B, b0 + per);
    int64_t nL = 0;
    int fl = 0;
    for (int b = b0; b < b1; ++b) {
        int64_t L = lens[b];
        if (L < 0) { fl |= 64; L = 0; }
        if (L > frame_capacity) { fl |= 1; L = frame_capacity + 1; }
        if (src_stride && L > src_stride) fl |= 2;
        nL += L;
    }
    sL[tid] = nL; sF[tid] = fl;
    __syncthreads();
    for (int o = 1; o < kSpsiThreads; o <<= 1) {
        int64_t pL = 0;
        int pF = 0;
        if (tid >= o) { pL = sL[tid - o]; pF = sF[tid - o]; }
        __syncthreads();
        sL[tid] += pL; sF[tid] |= pF;
        __syncthreads();
    }
    const int64_t frames = sL[kSpsiThreads - 1];
    int flags = sF[kSpsiThreads - 1];
    if (frames > frame_capacity) flags |= 1;
    if (upstream && upstream[2] != 0) flags |= 32 | upstream[2];
    int64_t rL = sL[tid] - nL;
    for (int b = b0; b < b1; ++b) {
        SpsiUtt u{};
        if (!flags) {
            const int L = (int)lens[b];                  // validated: 0 <= L <= frame_capacity
            u.ws_row0 = (int)rL;
            u.src_row0 = src_stride ? b * src_stride : (int)rL;
            u.L = L;
            rL += L;
        }
        utt[b] = u;
    }
    if (tid == 0) { hdr[0] = flags ? 0 : (int)frames; hdr[1] = flags; hdr[2] = 0; hdr[3] = 0; }
}

// w of the peak j of a row in LDS
template <int NFFT>
__device__ inline float spsi_peak_w(const float* m, int j, int hop, float hop_over_n) {
#pragma clang fp contract(off)      // one rounding per operation: tests/spsi_oracle.py computes the same bits
    const float a = m[j - 1], b = m[j], c = m[j + 1];
    const float den = (a - 2.0f * b) + c;
    const float p = den != 0.0f ? (0.5f * (a - c)) / den : 0.0f;
    const float frac = (float)((hop * j) & (NFFT - 1)) / (float)NFFT;      // exact
    const float adv = p * hop_over_n;
    return frac + adv;
}

// One frame of the chain for one bin: g = acc of the previous frame at spsi_gather_bin (the owner, or the bin itself where it has
// none), o / w = the bin's owner word and its owner's w.  No branch.
__device__ inline unsigned spsi_gather_bin(int k, unsigned o) { return o == kSpsiNone ? (unsigned)k : (o & kSpsiNone); }
__device__ inline float spsi_step(float g, unsigned o, float w) {
#pragma clang fp contract(off)
    float pk = g + w;
    pk -= floorf(pk);
    float v = pk + ((o & kSpsiHalf) ? 0.5f : 0.0f);
    if (v >= 1.0f) v -= 1.0f;
    return o == kSpsiNone ? g : v;
}

template <int NFFT>
__global__ __launch_bounds__(kSpsiThreads) void spsi_analyse(const SpsiUtt* utt, const int* hdr, int B, int hop, float hop_over_n, const float* src,
                                                            int src_width, const float* pinv, uint16_t* own, float* wv, float* mag_out) {
    constexpr int NB = NFFT / 2 + 1, NW = (NB + 63) / 64;
    __shared__ float sm[kSpsiTile][NB];
    __shared__ float e[kSpsiTile][kSpsiMaxMels];
    __shared__ unsigned long long rise[kSpsiTile][NW], fall[kSpsiTile][NW], peak[kSpsiTile][NW];
    __shared__ int srow[kSpsiTile];
    const int total = hdr[0];
    const int r0 = blockIdx.x * kSpsiTile;
    if (hdr[1] != 0 || r0 >= total) return;
    const int nf = min(kSpsiTile, total - r0);
    const int tid = threadIdx.x;
    if (tid < nf) {
        // the utterance of workspace row r: the first b with ws_row0[b] + L[b] > r (the ends never decrease; r < total: there is one)
        const int r = r0 + tid;
        int lo = 0, hi = B - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (utt[mid].ws_row0 + utt[mid].L > r) hi = mid; else lo = mid + 1;
        }
        srow[tid] = utt[lo].src_row0 + (r - utt[lo].ws_row0);
    }
    __syncthreads();
    const bool mel = src_width != NB;
    if (mel) {
        const int nm = src_width;
        for (int i = tid; i < nf * nm; i += kSpsiThreads) {
            const int f = i / nm, j = i - f * nm;
            e[f][j] = expf(src[(int64_t)srow[f] * nm + j]);
        }
        __syncthreads();
        for (int k = tid; k < NB; k += kSpsiThreads) {
            float acc[kSpsiTile];
#pragma unroll
            for (int f = 0; f < kSpsiTile; ++f) acc[f] = 0.f;
            const float* p = pinv + (int64_t)k * nm;
            for (int j = 0; j < nm; ++j) {
                const float q = p[j];
#pragma unroll
                for (int f = 0; f < kSpsiTile; ++f) acc[f] += q * e[f][j];       // rows f >= nf hold stale finite-or-not values: never used
            }
#pragma unroll
            for (int f = 0; f < kSpsiTile; ++f)
                if (f < nf) sm[f][k] = fmaxf(acc[f], 0.f);
        }
    } else {
        for (int i = tid; i < nf * NB; i += kSpsiThreads) {
            const int f = i / NB, k = i - f * NB;
            sm[f][k] = src[(int64_t)srow[f] * NB + k];
        }
    }
    __syncthreads();
    if (mag_out)
        for (int i = tid; i < nf * NB; i += kSpsiThreads) {
            const int f = i / NB, k = i - f * NB;
            mag_out[(int64_t)srow[f] * NB + k] = sm[f][k];
        }
    // flags of every bin as masks: wave w takes the frames w, w + 4, ..; bit (k & 63) of word (k >> 6).  Bin NB - 1 is never rising and
    // bin 0 never falling, so the searches below end inside the row.
    const int wave = tid >> 6, lane = tid & 63;
    for (int f = wave; f < kSpsiTile; f += kSpsiThreads / 64) {
        for (int c = 0; c < NW; ++c) {
            const int k = c * 64 + lane;
            bool up = false, down = false, pk = false;
            if (f < nf && k < NB) {
                const float v = sm[f][k];
                const bool lt_next = k <= NB - 2 && v < sm[f][k + 1], lt_prev = k >= 1 && v < sm[f][k - 1];
                pk = k >= 1 && k <= NB - 2 && v > sm[f][k - 1] && v > sm[f][k + 1];
                up = lt_next; down = lt_prev;
            }
            const unsigned long long mu = __ballot(up), md = __ballot(down), mp = __ballot(pk);
            if (lane == 0) { rise[f][c] = mu; fall[f][c] = md; peak[f][c] = mp; }
        }
    }
    __syncthreads();
    for (int f = wave; f < nf; f += kSpsiThreads / 64) {
        const float* m = sm[f];
        const int64_t o0 = (int64_t)(r0 + f) * NB;
        for (int k = lane; k < NB; k += 64) {
            const int c = k >> 6, bit = k & 63;
            int q = -1;
            if ((peak[f][c] >> bit) & 1) {
                q = k;
            } else if (k >= 1 && k <= NB - 2) {
                if ((rise[f][c] >> bit) & 1) {
                    // the first bin above k that is not rising
                    int cc = c;
                    unsigned long long x = (~rise[f][cc] >> bit) << bit;
                    while (x == 0) x = ~rise[f][++cc];
                    const int t = cc * 64 + __builtin_ctzll(x);
                    if ((peak[f][t >> 6] >> (t & 63)) & 1) q = t;
                }
                if (q < 0 && ((fall[f][c] >> bit) & 1)) {
                    // the last bin below k that is not falling
                    int cc = c;
                    unsigned long long x = (~fall[f][cc] << (63 - bit)) >> (63 - bit);
                    while (x == 0) x = ~fall[f][--cc];
                    const int t = cc * 64 + 63 - __builtin_clzll(x);
                    if ((peak[f][t >> 6] >> (t & 63)) & 1) q = t;
                }
            }
            unsigned word = kSpsiNone;
            float w = 0.f;
            if (q >= 0) {
                w = spsi_peak_w<NFFT>(m, q, hop, hop_over_n);
                const bool right = m[q + 1] > m[q - 1];
                const int d = k - q;
                const bool half = d != 0 && (right ? (d == 1 || d < 0) : (d == -1 || d > 0));
                word = (unsigned)q | (half ? kSpsiHalf : 0u);
            }
            own[o0 + k] = (uint16_t)word;
            wv[o0 + k] = w;
        }
    }
}

// spsi_chain's registers for kSpsiAhead frames: NPT owner words and NPT floats per thread and frame
template <int NPT> struct SpsiRows {
    unsigned o[kSpsiAhead][NPT];
    float w[kSpsiAhead][NPT];
};

// rows [t0, t0 + kSpsiAhead) of the utterance; rows beyond it are loaded from its last row (clamped, never used)
template <int NB, int NPT>
__device__ inline void spsi_load_rows(SpsiRows<NPT>& r, const uint16_t* ob, const float* wb, int t0, int L) {
#pragma unroll
    for (int a = 0; a < kSpsiAhead; ++a) {
        const int64_t at = (int64_t)min(t0 + a, L - 1) * NB;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            r.o[a][i] = ob[at + i * kSpsiThreads];
            r.w[a][i] = wb[at + i * kSpsiThreads];
        }
    }
}

// frame t = t0 + A of the rows in r: every gather, then every step, one barrier
template <int NB, int NPT, int A>
__device__ inline void spsi_frame(const SpsiRows<NPT>& r, float (*acc)[NB - 1], float* out, int t0, int tid) {
    const int t = t0 + A;
    const float* prev = acc[t & 1];
    float* next = acc[(t & 1) ^ 1];
    float g[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) g[i] = prev[spsi_gather_bin(tid + i * kSpsiThreads, r.o[A][i])];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const float v = spsi_step(g[i], r.o[A][i], r.w[A][i]);
        next[tid + i * kSpsiThreads] = v;
        out[(int64_t)t * NB + i * kSpsiThreads] = v * 6.28318548f;
    }
    __syncthreads();
}

// all kSpsiAhead frames of r (FULL), or those below L
template <int NB, int NPT, bool FULL>
__device__ inline void spsi_frames(const SpsiRows<NPT>& r, float (*acc)[NB - 1], float* out, int t0, int L, int tid) {
    static_assert(kSpsiAhead == 8, "unrolled by hand");
    if (FULL || t0 + 0 < L) spsi_frame<NB, NPT, 0>(r, acc, out, t0, tid);      // (t0 + A < L: the same for every thread of the workgroup)
    if (FULL || t0 + 1 < L) spsi_frame<NB, NPT, 1>(r, acc, out, t0, tid);
    if (FULL || t0 + 2 < L) spsi_frame<NB, NPT, 2>(r, acc, out, t0, tid);
    if (FULL || t0 + 3 < L) spsi_frame<NB, NPT, 3>(r, acc, out, t0, tid);
    if (FULL || t0 + 4 < L) spsi_frame<NB, NPT, 4>(r, acc, out, t0, tid);
    if (FULL || t0 + 5 < L) spsi_frame<NB, NPT, 5>(r, acc, out, t0, tid);
    if (FULL || t0 + 6 < L) spsi_frame<NB, NPT, 6>(r, acc, out, t0, tid);
    if (FULL || t0 + 7 < L) spsi_frame<NB, NPT, 7>(r, acc, out, t0, tid);
}

// Bins 0 and NB - 1 never have an owner: their phase is 0 on every frame.  The threads step the bins [0, NB - 1) = kSpsiThreads x NPT
// exactly, so the frame loop has no guard and no branch around a load: a load behind a branch makes the compiler wait for every load
// in flight at the next use, which would put the HBM latency back into every frame.  Two register sets take turns (no copy from one
// to the other, which would wait for the stores just issued as well): while one is stepped, the other is in flight.
template <int NFFT>
__global__ __launch_bounds__(kSpsiThreads) void spsi_chain(const SpsiUtt* utt, const int* hdr, const uint16_t* own, const float* wv, float* phase) {
    constexpr int NB = NFFT / 2 + 1, NPT = (NB - 1) / kSpsiThreads;
    static_assert(NPT * kSpsiThreads == NB - 1, "the chain's threads cover the bins [0, NB - 1) exactly");
    __shared__ float acc[2][NB - 1];
    if (hdr[1] != 0) return;
    const SpsiUtt u = utt[blockIdx.x];
    const int L = u.L, tid = threadIdx.x;
    if (L <= 0) return;
#pragma unroll
    for (int i = 0; i < NPT; ++i) acc[0][tid + i * kSpsiThreads] = 0.f;
    for (int t = tid; t < L; t += kSpsiThreads) phase[(int64_t)(u.src_row0 + t) * NB + (NB - 1)] = 0.f;
    const uint16_t* ob = own + (int64_t)u.ws_row0 * NB + tid;
    const float* wb = wv + (int64_t)u.ws_row0 * NB + tid;
    float* out = phase + (int64_t)u.src_row0 * NB + tid;
    SpsiRows<NPT> ra, rb;
    spsi_load_rows<NB, NPT>(ra, ob, wb, 0, L);
    __syncthreads();
    int t0 = 0;
    while (true) {
        if (t0 + kSpsiAhead > L) { spsi_frames<NB, NPT, false>(ra, acc, out, t0, L, tid); break; }
        spsi_load_rows<NB, NPT>(rb, ob, wb, t0 + kSpsiAhead, L);
        spsi_frames<NB, NPT, true>(ra, acc, out, t0, L, tid);
        t0 += kSpsiAhead;
        if (t0 + kSpsiAhead > L) { spsi_frames<NB, NPT, false>(rb, acc, out, t0, L, tid); break; }
        spsi_load_rows<NB, NPT>(ra, ob, wb, t0 + kSpsiAhead, L);
        spsi_frames<NB, NPT, true>(rb, acc, out, t0, L, tid);
        t0 += kSpsiAhead;
    }
}

// ---- workspace layout and launch sequences (host), shared by fs2_op_spsi_phase_geom / _dev and the host stand-in of the tests ----
struct SpsiLayout {
    size_t off_hdr = 0, off_utt = 0, off_own = 0, off_w = 0, bytes = 0;
};

inline SpsiLayout spsi_layout(int n_bins, int64_t B, int64_t frames) {
    SpsiLayout l;
    size_t off = 0;
    auto take = [&](size_t n) { off = (off + 255) / 256 * 256; size_t o = off; off += n; return o; };
    l.off_hdr = take(kSpsiHdrInts * sizeof(int));
    l.off_utt = take((size_t)(B > 1 ? B : 1) * sizeof(SpsiUtt));
    l.off_own = take((size_t)frames * n_bins * sizeof(uint16_t));
    l.off_w = take((size_t)frames * n_bins * sizeof(float));
    l.bytes = (off + 255) / 256 * 256;
    return l;
}

// spsi_analyse over `rows` workspace rows and spsi_chain over B utterances, the records and the header being in place (or being
// written ahead on the stream)
inline hipError_t spsi_launch(hipStream_t s, int n_fft, int hop, const float* src, int src_width, const float* pinv, int B, int64_t rows, char* ws,
                              const SpsiLayout& at, float* phase, float* mag_out) {
    const SpsiUtt* utt = (const SpsiUtt*)(ws + at.off_utt);
    const int* hdr = (const int*)(ws + at.off_hdr);
    uint16_t* own = (uint16_t*)(ws + at.off_own);
    float* wv = (float*)(ws + at.off_w);
    const float hop_over_n = (float)((double)hop / (double)n_fft);
    const dim3 ga((unsigned)((rows + kSpsiTile - 1) / kSpsiTile)), gb((unsigned)B), blk(kSpsiThreads);
    if (n_fft == 512) {
        hipLaunchKernelGGL((spsi_analyse<512>), ga, blk, 0, s, utt, hdr, B, hop, hop_over_n, src, src_width, pinv, own, wv, mag_out);
        hipLaunchKernelGGL((spsi_chain<512>), gb, blk, 0, s, utt, hdr, own, wv, phase);
    } else if (n_fft == 1024) {
        hipLaunchKernelGGL((spsi_analyse<1024>), ga, blk, 0, s, utt, hdr, B, hop, hop_over_n, src, src_width, pinv, own, wv, mag_out);
        hipLaunchKernelGGL((spsi_chain<1024>), gb, blk, 0, s, utt, hdr, own, wv, phase);
    } else {
        hipLaunchKernelGGL((spsi_analyse<2048>), ga, blk, 0, s, utt, hdr, B, hop, hop_over_n, src, src_width, pinv, own, wv, mag_out);
        hipLaunchKernelGGL((spsi_chain<2048>), gb, blk, 0, s, utt, hdr, own, wv, phase);
    }
    return hipGetLastError();
}

// Host-planned: starts / lens validated by the caller (>= 0, sum `frames` > 0)
inline hipError_t spsi_run_host(hipStream_t s, int n_fft, int hop, const float* src, int src_width, const float* pinv, int B, const int32_t* starts,
                                const int32_t* lens, int64_t frames, char* ws, const SpsiLayout& at, float* phase, float* mag_out) {
    int row = 0;
    for (int i = 0; i < B; i += kSpsiUttsPerChunk) {
        SpsiUttChunk c{};
        c.n = B - i < kSpsiUttsPerChunk ? B - i : kSpsiUttsPerChunk;
        c.base = i;
        c.frames = (int)frames;
        for (int j = 0; j < c.n; ++j) {
            c.u[j].src_row0 = starts[i + j];
            c.u[j].ws_row0 = row;
            c.u[j].L = lens[i + j];
            row += lens[i + j];
        }
        hipLaunchKernelGGL(spsi_upload, dim3(1), dim3(kSpsiThreads), 0, s, c, (SpsiUtt*)(ws + at.off_utt), (int*)(ws + at.off_hdr));
    }
    return spsi_launch(s, n_fft, hop, src, src_width, pinv, B, frames, ws, at, phase, mag_out);
}

// Device-driven: the grids are sized from the capacities, surplus workgroups leave at once
inline hipError_t spsi_run_dev(hipStream_t s, int n_fft, int hop, const float* src, int src_width, const float* pinv, int B, const int64_t* lens_dev,
                               int src_stride, int64_t frame_capacity, const int32_t* upstream, char* ws, const SpsiLayout& at, float* phase,
                               float* mag_out) {
    hipLaunchKernelGGL(spsi_plan, dim3(1), dim3(kSpsiThreads), 0, s, lens_dev, upstream, B, src_stride, frame_capacity, (SpsiUtt*)(ws + at.off_utt),
                       (int*)(ws + at.off_hdr));
    return spsi_launch(s, n_fft, hop, src, src_width, pinv, B, frame_capacity, ws, at, phase, mag_out);
}

}  // namespace fs2
