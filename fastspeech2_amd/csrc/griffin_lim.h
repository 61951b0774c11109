// Griffin-Lim vocoder and the analysis STFT (fs2_op_griffin_lim[_geom] / fs2_op_stft[_geom], include/fs2.h).
//
// Transform: n_fft N in {512, 1024, 2048}, hop H <= win_length W <= N, ceil(N / H) <= 8, N / 2 + 1 bins, periodic Hann window of W
// samples zero-padded to N at the centre (the reference's STFT class, utils/stft.py:41-151; default N = W = 1024, H = 256).  For an
// utterance of L frames (T = H (L - 1) samples):
//   ISTFT  x = OLA_f(w . irfft(C_f)) / wss, trimmed by N / 2 at both ends  (STFT.inverse, stft.py:112-151)
//   STFT   X_f = rfft(w . frame_f) of the signal reflect-padded by N / 2   (STFT.transform, stft.py:80-110)
//   GL     C = M . A / |A|, A = X - momentum / (1 + momentum) . T, T <- X   (griffin_lim, audio_processing.py:224-240; momentum 0 = reference)
//          or, mel-constrained (fs2_op_griffin_lim_mel_geom / _dev; GlMelProj below), C = g . A with the
//          per-bin gain g that makes the mel of |A| the caller's
// Utterances with L < L_min = floor(N / 2H) + 2 (T <= N / 2) are too short for the reflect padding: their T samples are written as
// zeros and no iteration touches them.
//
// Work split.  A workgroup (256 threads = 4 waves) owns a tile of F consecutive frames of one utterance, tiles counted from the
// utterance's first frame.  It inverse-transforms its frames plus a halo of h = max(ceil(N / H) - 1, 1) frames on each side (exactly
// what the STFT of its frames and its own output samples read, the reflect padding at both utterance ends included), overlap-adds
// them in LDS in increasing frame order, normalises by the window envelope, forward-transforms its own frames and writes their new
// complex spectrum C = M . phasor.  Every number depends only on the utterance's own frames and on utterance-local indices, never on
// the tile boundaries or the batch: an utterance comes out bit-identical whether it is vocoded alone or inside any batch, and a sample
// computed by two tiles (halo) is the same in both.  No atomics: results are deterministic.  The spectra ping-pong between two
// workspace buffers across iterations.  The tile rule is checked exhaustively on the host (tests/test_vocoder_geometry_host.py).
//
// FFT.  An N-point real transform is an N/2-point complex one (z[m] = x[2m] + i x[2m+1]) plus a split pass.  The complex transform is
// a Stockham sequence, one wave per transform: lane j holds V = N / 128 complex values in registers, the passes exchange through an
// (N / 2)-entry LDS buffer per wave.  512 = 8^3 (fft512, the default geometry's), 256 = 4^4 and 1024 = 8^3 . 2 (st_pass: every
// lane busy in every pass).  Twiddles and the window come from a table the table kernel writes once per call (double precision,
// rounded to fp32).  All arithmetic fp32 on the VALU.
//
// The default geometry (1024 / 256, F = 32) is its own instantiation with the hop and the tile as constants (HOP_C = 256, static
// LDS); every other geometry takes hop, F and the halo at run time and the signal buffer as dynamic LDS (F: DESIGN.md section 14).
//
// Budget at the default (shapes, c3 = 35.6 k frames): per iteration the fused kernel reads C of (F + 6) / F frames (4104 B each) and
// M (2052 B) and writes C (4104 B) per frame: ~0.42 GB at F = 32, ~70 us at 6 TB/s; FFT work ~2.4 real 1024-point transforms per
// frame, ~60 kFLOP, ~2.2 GFLOP per iteration (~14 us at 157 TF).  The LDS traffic of the three passes (~0.3 MB per frame and
// iteration, ~11 GB) at ~80 TB/s of LDS bandwidth is the tightest bound (~0.14 ms); measured figures: BASELINE.md section 5.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl_slot_rule.h"
#include "gl_tile_rule.h"

namespace fs2 {

constexpr int kGlNfft = 1024, kGlHop = 256, kGlBins = 513, kGlThreads = 256;   // the default geometry (kGlTile: gl_tile_rule.h)
constexpr int kGlTilesPerChunk = 120;        // tile records per upload launch (kernel-argument bytes: 120 * 32 + 8 < 4 KB)
constexpr int kGlMaxMels = 128;

// ---- tile rule: gl_tile_rule.h (gl_halo, gl_tail, gl_lmin, gl_sig_max, gl_tile_frames; restated in vocoder.py: tile_rule) ----

// Run-time geometry of one call (the default instantiation ignores all but n_mels)
struct GlGeom {
    int hop, F, halo, tail, lmin, sig_max, n_mels, pad;
};

// One tile: frames [f0, f0 + F) of an utterance (clipped to L).  Written to the workspace by gl_upload_tiles from kernel
// arguments, so the call needs no host-to-device copy and no host synchronisation.
struct GlTile {
    int src_row0;   // packed row of the utterance's frame 0 in the caller's source (mel / magnitude rows, or analysis frames)
    int ws_row0;    // packed row of the utterance's frame 0 in the workspace spectra (prefix sum of L)
    int L;          // frames of the utterance
    int f0;         // first frame of this tile, utterance-local
    int wav0;       // first sample of the utterance in the packed waveform
    int T;          // samples of the utterance (analysis: as given; synthesis: hop (L - 1))
    int pad0, pad1;
};
struct GlTileChunk {
    int n, base;
    GlTile t[kGlTilesPerChunk];
};

__global__ void gl_upload_tiles(GlTileChunk c, GlTile* dst) {
    const int i = threadIdx.x;
    if (i < c.n) dst[c.base + i] = c.t[i];
}

// tw[m] = exp(-2 pi i m / N), win[m] = periodic Hann of wl samples (scipy.signal.get_window("hann", wl, fftbins=True)) centred in N
// (librosa.util.pad_center: (N - wl) / 2 zeros before), from double.
__global__ void gl_tables(float2* tw, float* win, int n, int wl) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    double s, c;
    sincospi((double)m / (double)(n / 2), &s, &c);
    tw[m] = make_float2((float)c, (float)-s);
    const int lp = (n - wl) / 2;
    double sw, cw;
    sincospi(2.0 * (double)(m - lp) / (double)wl, &sw, &cw);
    win[m] = (m >= lp && m < lp + wl) ? (float)(0.5 - 0.5 * cw) : 0.f;
}

// ---- seeded initial phase: counter-based, keyed by (seed, utterance-local frame, bin); restated in fastspeech2_amd/vocoder.py ----
__host__ __device__ inline uint32_t gl_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ inline float gl_seed_angle(uint32_t seed, uint32_t f, uint32_t k, uint32_t nbins) {
#pragma clang fp contract(off)     // two roundings, no FMA: the host restatement (vocoder.seed_angles) computes the same bits
    const uint32_t h = gl_mix32((k + nbins * f) ^ gl_mix32(seed + 0x9E3779B9u));
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f);                          // exact
    return u * 6.28318548f - 3.14159274f;                                             // uniform on [-pi, pi)
}

// Prologue, one workgroup per tile: M = max(P . exp(mel), 0) (src_width n_mels; P = pinv(mel basis) [bins, n_mels]) or M = src
// (src_width = bins), C0 = M . exp(i theta0) with theta0 given [rows of src, bins] or seeded; the momentum state T = 0.
// NMEL_C = 80: the default's mel width as a constant (float4 rows of P); 0: n_mels <= 128 at run time.
template <int NFFT, int NMEL_C>
__global__ __launch_bounds__(kGlThreads) void gl_prologue(const GlTile* tiles, GlGeom g, const float* src, int src_width, const float* pinv,
                                                          const float* init_phase, uint32_t seed, float* M, float2* C, float2* Tm) {
    constexpr int NB = NFFT / 2 + 1;
    const GlTile t = tiles[blockIdx.x];
    if (t.L < g.lmin) return;     // never iterated, never read (the final ISTFT writes zeros)
    const int nm = NMEL_C ? NMEL_C : g.n_mels;
    const int nf = min(g.F, t.L - t.f0);
    __shared__ float e[kGlTile][NMEL_C ? NMEL_C : kGlMaxMels];
    const bool mel = src_width != NB;
    if (mel) {
        for (int i = threadIdx.x; i < nf * nm; i += kGlThreads) {
            const int f = i / nm, j = i - f * nm;
            e[f][j] = expf(src[(int64_t)(t.src_row0 + t.f0 + f) * nm + j]);
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < NB; k += kGlThreads) {
        float acc[kGlTile];
        if (mel) {
#pragma unroll
            for (int f = 0; f < kGlTile; ++f) acc[f] = 0.f;
            if constexpr (NMEL_C != 0) {
                const float4* p = reinterpret_cast<const float4*>(pinv + (int64_t)k * NMEL_C);
                for (int j4 = 0; j4 < NMEL_C / 4; ++j4) {
                    const float4 q = p[j4];
#pragma unroll
                    for (int f = 0; f < kGlTile; ++f) {
                        if (f < nf)
                            acc[f] += q.x * e[f][4 * j4] + q.y * e[f][4 * j4 + 1] + q.z * e[f][4 * j4 + 2] + q.w * e[f][4 * j4 + 3];
                    }
                }
            } else {
                const float* p = pinv + (int64_t)k * nm;
                for (int j = 0; j < nm; ++j) {
                    const float q = p[j];
#pragma unroll
                    for (int f = 0; f < kGlTile; ++f)
                        if (f < nf) acc[f] += q * e[f][j];
                }
            }
        }
#pragma unroll
        for (int f = 0; f < kGlTile; ++f) {
            if (f < nf) {
                const int fl = t.f0 + f;
                const float m = mel ? fmaxf(acc[f], 0.f) : src[(int64_t)(t.src_row0 + fl) * NB + k];
                const float th = init_phase ? init_phase[(int64_t)(t.src_row0 + fl) * NB + k] : gl_seed_angle(seed, (uint32_t)fl, (uint32_t)k, NB);
                float s, c;
                sincosf(th, &s, &c);
                const int64_t o = (int64_t)(t.ws_row0 + fl) * NB + k;
                M[o] = m;
                C[o] = make_float2(m * c, m * s);
                if (Tm) Tm[o] = make_float2(0.f, 0.f);
            }
        }
    }
}

// ---- N2-point complex FFT, one wave, lane j holds v[r] = z[j + 64 r] on entry and Z[j + 64 r] on exit (r < N2 / 64) ----
__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <int D> __device__ inline float2 cmul_di(float2 a) { return make_float2(-D * a.y, D * a.x); }   // a . (D i)

// in-register 8-point DFT, V[k] = sum_n v[n] exp(D 2 pi i n k / 8), natural order in and out
template <int D> __device__ inline void fft8(float2* v) {
    const float h = 0.70710678118654752f;
    float2 e[4], o[4];
    {
        const float2 t0 = cadd(v[0], v[4]), t1 = csub(v[0], v[4]), t2 = cadd(v[2], v[6]), t3 = cmul_di<D>(csub(v[2], v[6]));
        e[0] = cadd(t0, t2); e[2] = csub(t0, t2); e[1] = cadd(t1, t3); e[3] = csub(t1, t3);
    }
    {
        const float2 t0 = cadd(v[1], v[5]), t1 = csub(v[1], v[5]), t2 = cadd(v[3], v[7]), t3 = cmul_di<D>(csub(v[3], v[7]));
        o[0] = cadd(t0, t2); o[2] = csub(t0, t2); o[1] = cadd(t1, t3); o[3] = csub(t1, t3);
    }
    o[1] = cmul(o[1], make_float2(h, D * h));
    o[2] = cmul_di<D>(o[2]);
    o[3] = cmul(o[3], make_float2(-h, D * h));
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = cadd(e[k], o[k]); v[k + 4] = csub(e[k], o[k]); }
}

template <int D> __device__ inline void fft4(float2* v) {
    const float2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), t3 = cmul_di<D>(csub(v[1], v[3]));
    v[0] = cadd(t0, t2); v[2] = csub(t0, t2); v[1] = cadd(t1, t3); v[3] = csub(t1, t3);
}

template <int D> __device__ inline void fft2(float2* v) {
    const float2 a = v[0];
    v[0] = cadd(a, v[1]); v[1] = csub(a, v[1]);
}

// Stockham radix-8: three passes (stride p = 1, 8, 64); output index (j / p) p 8 + j % p + r p.  Every thread of the block calls it
// (the barriers are block-wide); buf is this wave's 512-entry scratch, tw the 1024-entry table.  D = -1 forward, +1 inverse.
template <int D> __device__ inline void fft512(float2* v, float2* buf, const float2* tw, int j) {
    fft8<D>(v);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) buf[8 * j + r] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        v[r] = buf[j + 64 * r];
        if (r) { const float2 w = tw[16 * (j & 7) * r]; v[r] = cmul(v[r], make_float2(w.x, D == -1 ? w.y : -w.y)); }
    }
    fft8<D>(v);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) buf[(j >> 3) * 64 + (j & 7) + 8 * r] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        v[r] = buf[j + 64 * r];
        if (r) { const float2 w = tw[2 * j * r]; v[r] = cmul(v[r], make_float2(w.x, D == -1 ? w.y : -w.y)); }
    }
    fft8<D>(v);
}

// One radix-R Stockham pass of an N2-point transform at stride P (the product of the earlier radices).  Lane j owns the butterflies
// b = j + 64 i (i < V / R); butterfly b's inputs are x[b + (N2 / R) r] = v[i + (V / R) r] (v[m] = x[j + 64 m]: the layout both on
// entry and after the buffer is read back), each times exp(D 2 pi i r (b % P) / (P R)) (table entry 2 r (b % P) N2 / (P R)).  Its
// outputs go to (b / P) P R + b % P + s P; the last pass (P R = N2) lands them on b + s P = j + 64 (i + (V / R) s), in registers.
template <int N2, int R, int P, int D> __device__ inline void st_pass(float2* v, float2* buf, const float2* tw, int j) {
    constexpr int V = N2 / 64, G = V / R;
    static_assert(G >= 1 && G * R == V, "radix must divide the values per lane");
    if constexpr (P > 1) {
        __syncthreads();
#pragma unroll
        for (int m = 0; m < V; ++m) v[m] = buf[j + 64 * m];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int k = (j + 64 * i) % P;
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const float2 w = tw[2 * r * k * (N2 / (P * R))];
                v[i + G * r] = cmul(v[i + G * r], make_float2(w.x, D == -1 ? w.y : -w.y));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        float2 a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = v[i + G * r];
        if constexpr (R == 8) fft8<D>(a);
        else if constexpr (R == 4) fft4<D>(a);
        else fft2<D>(a);
#pragma unroll
        for (int s = 0; s < R; ++s) v[i + G * s] = a[s];
    }
    if constexpr (P * R < N2) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int b = j + 64 * i, k = b % P;
#pragma unroll
            for (int s = 0; s < R; ++s) buf[(b / P) * P * R + k + s * P] = v[i + G * s];
        }
    }
}

template <int N2, int D> __device__ inline void fft_c(float2* v, float2* buf, const float2* tw, int j) {
    if constexpr (N2 == 512) {
        fft512<D>(v, buf, tw, j);
    } else if constexpr (N2 == 256) {
        st_pass<256, 4, 1, D>(v, buf, tw, j);
        st_pass<256, 4, 4, D>(v, buf, tw, j);
        st_pass<256, 4, 16, D>(v, buf, tw, j);
        st_pass<256, 4, 64, D>(v, buf, tw, j);
    } else {
        static_assert(N2 == 1024, "n_fft 512, 1024 or 2048");
        st_pass<1024, 8, 1, D>(v, buf, tw, j);
        st_pass<1024, 8, 8, D>(v, buf, tw, j);
        st_pass<1024, 8, 64, D>(v, buf, tw, j);
        st_pass<1024, 2, 512, D>(v, buf, tw, j);
    }
}

// Frame f's inverse: x[n] = w[n] irfft(C_f)[n] into out[0..N) (the wave's scratch, viewed as floats).  Bins 0 and N/2 lose their
// imaginary parts (what the reference's pinv basis does).
template <int NFFT>
__device__ inline void gl_frame_istft(const float2* __restrict__ Cf, bool valid, float2* buf, const float2* tw, const float* win, int j) {
    constexpr int N2 = NFFT / 2, V = N2 / 64;
    float2 v[V];
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int k = j + 64 * r;                       // Z[k] = E[k] + i O[k] (x 2: the 1/N is applied at the end)
        float2 a = make_float2(0.f, 0.f), b = a;
        if (valid) { a = Cf[k]; b = Cf[N2 - k]; }
        if (k == 0) { a.y = 0.f; b.y = 0.f; }
        const float2 E = make_float2(a.x + b.x, a.y - b.y);
        const float2 t = tw[k];                          // O = (a - conj b) exp(+2 pi i k / N)
        const float2 O = cmul(make_float2(a.x - b.x, a.y + b.y), make_float2(t.x, -t.y));
        v[r] = make_float2(E.x - O.y, E.y + O.x);
    }
    fft_c<N2, 1>(v, buf, tw, j);
    __syncthreads();
    float* out = reinterpret_cast<float*>(buf);
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int m = j + 64 * r;
        out[2 * m] = v[r].x * (1.0f / NFFT) * win[2 * m];
        out[2 * m + 1] = v[r].y * (1.0f / NFFT) * win[2 * m + 1];
    }
}

// Forward: v[r] = z[j + 64 r] (windowed, packed real pairs) -> lane j gets X[j + 64 r] in X[r]; lane 0 also X[N/2] in xl.
template <int NFFT>
__device__ inline void gl_frame_rfft(float2* v, float2* X, float2& xl, float2* buf, const float2* tw, int j) {
    constexpr int N2 = NFFT / 2, V = N2 / 64;
    fft_c<N2, -1>(v, buf, tw, j);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < V; ++r) buf[j + 64 * r] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int k = j + 64 * r;
        const float2 a = v[r], b = buf[(N2 - k) & (N2 - 1)];
        const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
        const float2 O = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));     // (a - conj b) / (2 i)
        X[r] = cadd(E, cmul(tw[k], O));
    }
    xl = make_float2(v[0].x - v[0].y, 0.f);             // X[N/2] = E[0] - O[0] (meaningful on lane 0)
}

// window envelope at pre-trim position p of an utterance of L frames (window_sumsquare, audio_processing.py:171-222: frames in order)
template <int NFFT>
__device__ inline float gl_wss(int p, int L, const float* win, int hop) {
    const int fa = max(0, (p - NFFT + hop) / hop), fb = min(L - 1, p / hop);
    float s = 0.f;
    for (int f = fa; f <= fb; ++f) {
        const int n = p - hop * f;
        if (n < NFFT) { const float w = win[n]; s += w * w; }
    }
    return s;
}

constexpr int kGlSigMax = gl_sig_max(kGlNfft, kGlHop, kGlTile);   // pre-trim samples a default tile's frames + halo span

// ---- mel-constrained projection (PROJ = 1 of gl_iterate) ----
// What the iteration reads beside the spectra: the caller's log-mel rows and mel basis [n_mels, bins], and the band tables
// gl_band_tables writes from that basis once per call.  An empty record (all NULL) is what the plain projection passes.
struct GlMelProj {
    const float* mel;        // the call's src: log-mel rows [.., n_mels], indexed by GlTile::src_row0 as the prologue does
    const float* basis;      // [n_mels, bins], non-negative
    const int2* row_rng;     // [kGlMaxMels]: bins [x, y) outside which row c of the basis is zero
    const int2* bin_rng;     // [bins]: mel rows [x, y) outside which column k is zero
    const float* inv_w;      // [bins]: 1 / sum_c B[c, k] (from double), 0 where the column is zero
    const float* band;       // [bins][kGlMaxMels]: band[b][c] = B[c, row_rng[c].x + b], 0 beyond the row's range: the rows of the basis
                             // shifted to their first bin and transposed, so that lane c walks its band with coalesced loads
};

constexpr size_t gl_band_bytes(int n_bins) {
    return kGlMaxMels * sizeof(int2) + (size_t)n_bins * (sizeof(int2) + sizeof(float) + kGlMaxMels * sizeof(float));
}

// (n_bins + 255) / 256 workgroups of 256 threads per call.  The ranges are the first and one past the last non-zero entry: a Slaney
// basis gives contiguous bands (a bin lies in at most two), a dense basis full ranges; zeros inside a range only cost their multiply.
// Rows: one wave per row (its lanes stride over the bins, a fixed butterfly joins them).  Bins: one thread per bin.
__global__ __launch_bounds__(kGlThreads) void gl_band_tables(const float* basis, int nm, int nb, int2* row_rng, int2* bin_rng, float* inv_w,
                                                             float* band) {
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int c = blockIdx.x * 4 + wv; c < kGlMaxMels; c += gridDim.x * 4) {
        const float* br = basis + (int64_t)c * nb;
        int lo = nb, hi = 0;
        if (c < nm)
            for (int k = j; k < nb; k += 64)
                if (br[k] != 0.f) { lo = min(lo, k); hi = max(hi, k + 1); }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
        if (hi == 0) lo = 0;
        if (j == 0) row_rng[c] = make_int2(lo, hi);
        for (int b = j; b < nb; b += 64) band[(int64_t)b * kGlMaxMels + c] = lo + b < hi ? br[lo + b] : 0.f;
    }
    const int k = blockIdx.x * kGlThreads + tid;
    if (k < nb) {
        int lo = 0, hi = 0;
        double w = 0.0;
        for (int c = 0; c < nm; ++c) {
            const float b = basis[(int64_t)c * nb + k];
            if (b != 0.f) { if (hi == 0) lo = c; hi = c + 1; }
            w += (double)b;
        }
        bin_rng[k] = make_int2(lo, hi);
        inv_w[k] = w > 0.0 ? (float)(1.0 / w) : 0.f;
    }
}

// MODE 0: one Griffin-Lim iteration, C_in -> C_out for the tile's own frames.  MODE 1: the final ISTFT, writes the tile's samples
// [hop f0, hop (f0 + F)) of the waveform (zeros for L < L_min).  HOP_C = 256 (with NFFT 1024): the default geometry, hop and tile as
// constants and the signal in static LDS; HOP_C = 0: hop, F and the halo from g, the signal in dynamic LDS (g.sig_max floats).
// PROJ 0: C = M . A / |A|.  PROJ 1 (MODE 0 only): C = g . A, the per-bin gain g that makes the mel of |A| the caller's (mp; M is
// not read): a = |A|, y = B a, r = min(exp(mel) / max(y, 1e-12), 1e4), g = (B^T r) / (B^T 1), 0 where no filter covers the bin.
template <int NFFT, int HOP_C, int MODE, bool MOMENTUM, int PROJ = 0>
__global__ __launch_bounds__(kGlThreads) void gl_iterate(const GlTile* tiles, GlGeom g, const float2* gtw, const float* gwin, const float* M,
                                                         const float2* Cin, float2* Cout, float2* Tm, float beta, float* wav, GlMelProj mp) {
    constexpr int N2 = NFFT / 2, V = N2 / 64, NB = N2 + 1;
    __shared__ float2 tw[NFFT];
    __shared__ float win[NFFT];
    __shared__ float2 scratch[4][N2];
    float* sig;
    if constexpr (HOP_C != 0) {
        __shared__ float sig_s[gl_sig_max(NFFT, HOP_C, kGlTile)];
        sig = sig_s;
    } else {
        extern __shared__ float gl_sig_dyn[];
        sig = gl_sig_dyn;
    }
    const int hop = HOP_C ? HOP_C : g.hop, F = HOP_C ? kGlTile : g.F, halo = HOP_C ? gl_halo(NFFT, HOP_C) : g.halo;
    const int tail = HOP_C ? gl_tail(NFFT, HOP_C) : g.tail, lmin = HOP_C ? gl_lmin(NFFT, HOP_C) : g.lmin;
    const GlTile t = tiles[blockIdx.x];
    const int L = t.L, T = hop * (L - 1);
    if (L < lmin) {       // too short for the reflect padding: documented zeros
        if (MODE == 1)
            for (int s = hop * t.f0 + threadIdx.x; s < min(T, hop * (t.f0 + F)); s += kGlThreads) wav[t.wav0 + s] = 0.f;
        return;
    }
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int i = tid; i < NFFT; i += kGlThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    const int nf = min(F, L - t.f0);
    // halo frames each side; a tile that reaches the utterance's last frame also needs frame L - tail (the reflection of its last
    // sample, hop (L - 1) - N / 2 - 1, lies below the halo)
    const int fa = max(0, min(t.f0 - halo, L - tail)), fb = min(L - 1, t.f0 + nf - 1 + halo), nh = fb - fa + 1;
    const int SL = hop * (fb - fa) + NFFT;                 // <= sig_max
    for (int q = tid; q < SL; q += kGlThreads) sig[q] = 0.f;
    // ---- ISTFT of frames fa..fb, four per round (wave w: frame fa + 4 k + w), overlap-added in frame order ----
    for (int k = 0; k < nh; k += 4) {
        const int f = fa + k + wv;
        const bool valid = f <= fb;
        gl_frame_istft<NFFT>(Cin + (int64_t)(t.ws_row0 + min(f, fb)) * NB, valid, scratch[wv], tw, win, j);
        __syncthreads();
        const int q0 = hop * k, q1 = min(SL, q0 + 3 * hop + NFFT);
        for (int q = q0 + tid; q < q1; q += kGlThreads) {
            float acc = sig[q];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int n = q - hop * (k + w);
                if (k + w < nh && n >= 0 && n < NFFT) acc += reinterpret_cast<const float*>(scratch[w])[n];
            }
            sig[q] = acc;
        }
    }
    __syncthreads();
    for (int q = tid; q < SL; q += kGlThreads) {
        const float s = gl_wss<NFFT>(hop * fa + q, L, win, hop);
        if (s > 1.17549435e-38f) sig[q] = sig[q] / s;
    }
    __syncthreads();
    const int qoff = NFFT / 2 - hop * fa;                  // trimmed sample s lives at sig[s + qoff]
    if (MODE == 1) {
        const int s1 = min(T, hop * (t.f0 + nf));
        for (int s = hop * t.f0 + tid; s < s1; s += kGlThreads) wav[t.wav0 + s] = sig[s + qoff];
        return;
    }
    // ---- STFT of the own frames, projection onto M ----
    for (int k = 0; k < nf; k += 4) {
        const int f = t.f0 + k + wv;
        const bool valid = k + wv < nf;
        float2 v[V];
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const int n = 2 * (j + 64 * r);
            float x[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int s = hop * f - NFFT / 2 + n + u;
                s = s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s);
                x[u] = valid ? sig[s + qoff] * win[n + u] : 0.f;
            }
            v[r] = make_float2(x[0], x[1]);
        }
        float2 X[V], xl;
        gl_frame_rfft<NFFT>(v, X, xl, scratch[wv], tw, j);
        if constexpr (PROJ == 0) {
            if (valid) {
                const int64_t row = (int64_t)(t.ws_row0 + f) * NB;
#pragma unroll
                for (int r = 0; r <= V; ++r) {
                    if (r == V && j) break;
                    const int k2 = r == V ? N2 : j + 64 * r;
                    const float2 x = r == V ? xl : X[r];
                    float2 a = x;
                    if (MOMENTUM) { const float2 tp = Tm[row + k2]; a = make_float2(x.x - beta * tp.x, x.y - beta * tp.y); Tm[row + k2] = x; }
                    const float mag = sqrtf(a.x * a.x + a.y * a.y);
                    const float m = M[row + k2];
                    Cout[row + k2] = mag > 0.f ? make_float2(m * (a.x / mag), m * (a.y / mag)) : make_float2(m, 0.f);
                }
            }
        } else {
            // |A| of this wave's frame (N/2 + 1 floats) and the band ratios r (n_mels <= 128 floats) behind it, in the wave's own
            // scratch: N/2 + 1 + 128 <= N for every NFFT.  A stays in registers.  nf is block-uniform and `valid` only predicates,
            // so every wave meets the three barriers.
            static_assert(NB + kGlMaxMels <= NFFT, "|A| and r share one wave's scratch");
            float* am = reinterpret_cast<float*>(scratch[wv]);
            float* rr = am + NB;
            const int nm = g.n_mels;
            const int64_t row = (int64_t)(t.ws_row0 + f) * NB;
            float2 A[V], al = xl;
            __syncthreads();                            // gl_frame_rfft's last reads of the scratch
            if (valid) {
#pragma unroll
                for (int r = 0; r <= V; ++r) {
                    if (r == V && j) break;
                    const int k2 = r == V ? N2 : j + 64 * r;
                    const float2 x = r == V ? xl : X[r];
                    float2 a = x;
                    if (MOMENTUM) { const float2 tp = Tm[row + k2]; a = make_float2(x.x - beta * tp.x, x.y - beta * tp.y); Tm[row + k2] = x; }
                    if (r == V) al = a; else A[r] = a;
                    am[k2] = sqrtf(a.x * a.x + a.y * a.y);
                }
            }
            __syncthreads();
            if (valid) {
                // lane j: the bands j and j + 64, each over its own bins in increasing order, four steps of both in flight
                const float* mrow = mp.mel + (int64_t)(t.src_row0 + f) * nm;
                const int c0 = j, c1 = j + 64;
                const int2 r0 = c0 < nm ? mp.row_rng[c0] : make_int2(0, 0), r1 = c1 < nm ? mp.row_rng[c1] : make_int2(0, 0);
                const int n0 = r0.y - r0.x, n1 = r1.y - r1.x, nmax = max(n0, n1);
                float y0 = 0.f, y1 = 0.f;
                for (int b = 0; b < nmax; b += 4) {
                    float q0[4], q1[4], a0[4], a1[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float* bp = mp.band + (int64_t)min(b + u, NB - 1) * kGlMaxMels;
                        q0[u] = bp[c0]; q1[u] = bp[c1];
                        a0[u] = am[min(r0.x + b + u, NB - 1)]; a1[u] = am[min(r1.x + b + u, NB - 1)];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (b + u < n0) y0 += q0[u] * a0[u];
                        if (b + u < n1) y1 += q1[u] * a1[u];
                    }
                }
                if (c0 < nm) rr[c0] = fminf(expf(mrow[c0]) / fmaxf(y0, 1e-12f), 1e4f);
                if (c1 < nm) rr[c1] = fminf(expf(mrow[c1]) / fmaxf(y1, 1e-12f), 1e4f);
            }
            __syncthreads();
            if (valid) {
#pragma unroll
                for (int r = 0; r <= V; ++r) {
                    if (r == V && j) break;
                    const int k2 = r == V ? N2 : j + 64 * r;
                    const float2 a = r == V ? al : A[r];
                    const int2 rg = mp.bin_rng[k2];
                    float s = 0.f;
                    for (int c = rg.x; c < rg.y; ++c) s += mp.basis[(int64_t)c * NB + k2] * rr[c];
                    const float gk = s * mp.inv_w[k2];
                    Cout[row + k2] = make_float2(gk * a.x, gk * a.y);
                }
            }
        }
    }
}

// Analysis STFT, one workgroup per tile of frames: |X| [rows, bins], log(clamp(B . |X|, 1e-5)) [rows, n_mels] and the frame energy
// ||X||_2 over the bins of |X| [rows] (torch.norm(mag, dim=0) of the reference's preprocessing), each optional, from one launch.
// Waveforms of <= N / 2 samples (no reflect padding possible) give |X| = 0, energy 0 and log-mel = log(1e-5).
template <int NFFT, int HOP_C>
__global__ __launch_bounds__(kGlThreads) void gl_stft(const GlTile* tiles, GlGeom g, const float2* gtw, const float* gwin, const float* wavp,
                                                      float* mag, const float* basis, float* logmel, float* energy) {
    constexpr int N2 = NFFT / 2, V = N2 / 64, NB = N2 + 1;
    __shared__ float2 tw[NFFT];
    __shared__ float win[NFFT];
    __shared__ float2 scratch[4][N2];
    const int hop = HOP_C ? HOP_C : g.hop, nm = g.n_mels;
    const GlTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int i = tid; i < NFFT; i += kGlThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    const int nf = min(HOP_C ? kGlTile : g.F, t.L - t.f0), T = t.T;
    const bool ok = T > NFFT / 2;
    const float* x = wavp + t.wav0;
    for (int k = 0; k < nf; k += 4) {
        const int f = t.f0 + k + wv;
        const bool valid = k + wv < nf;
        float2 v[V];
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const int n = 2 * (j + 64 * r);
            float xx[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int s = hop * f - NFFT / 2 + n + u;
                s = s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s);
                xx[u] = (valid && ok) ? x[s] * win[n + u] : 0.f;
            }
            v[r] = make_float2(xx[0], xx[1]);
        }
        float2 X[V], xl;
        gl_frame_rfft<NFFT>(v, X, xl, scratch[wv], tw, j);
        __syncthreads();
        float* am = reinterpret_cast<float*>(scratch[wv]);   // |X| of this wave's frame, N/2 + 1 floats
#pragma unroll
        for (int r = 0; r < V; ++r) am[j + 64 * r] = sqrtf(X[r].x * X[r].x + X[r].y * X[r].y);
        if (j == 0) am[N2] = fabsf(xl.x);
        __syncthreads();
        if (valid) {
            const int64_t row = (int64_t)(t.src_row0 + f);
            if (mag)
                for (int b = j; b < NB; b += 64) mag[row * NB + b] = am[b];
            if (logmel)
                for (int c = j; c < nm; c += 64) {
                    const float* br = basis + c * NB;
                    float acc = 0.f;
                    for (int b = 0; b < NB; ++b) acc += br[b] * am[b];
                    logmel[row * nm + c] = logf(fmaxf(acc, 1e-5f));
                }
        }
        if (energy) {          // lane j sums bins j, j + 64, ... in order, then a fixed butterfly over the wave: deterministic
            float e2 = 0.f;
            for (int b = j; b < NB; b += 64) e2 += am[b] * am[b];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) e2 += __shfl_xor(e2, o);
            if (valid && j == 0) energy[t.src_row0 + f] = sqrtf(e2);
        }
    }
}

// ---- device-driven plan (fs2_op_griffin_lim_dev) ----
// The frame counts stay on the device: gl_plan_scan validates them and scans the batch, gl_plan_emit writes one GlTile per slot of a
// grid sized from the capacities (gl_slot_rule.h), gl_plan_fill writes the samples no tile owns.  The tile kernels above then run
// over all slots; an empty record (L = 0) leaves each of them at once.  The records are the only thing the tile kernels index with,
// and they are emitted only after every length passed the checks: whatever lens holds, nothing is read or written outside src, the
// workspace and wav as sized from the capacities.  No atomics.
constexpr int kGlPlanThreads = 1024;
constexpr int kGlOvfRows = 1, kGlOvfLmax = 2, kGlOvfUpstream = 32, kGlOvfNegative = 64, kGlOvfWav = 128;     // FS2_OVF_* (include/fs2.h)

struct GlPlanArgs {
    const int64_t* lens;          // [B] frames per utterance (device)
    const int32_t* upstream;      // int32[8] status of the producer of src (fs2_decode), or NULL
    int B, hop, F;
    int src_stride;               // 0: packed source (utterance b at the prefix sum of L); else rows per utterance
    int wav_stride;               // 0: packed waveform; else samples per utterance
    int64_t frame_capacity;       // rows of the workspace spectra (and of a packed source)
    int64_t wav_capacity;         // floats of wav
    int *row0, *wav0, *tile_end, *Lv;     // [B] each, workspace: what gl_plan_emit reads
    int64_t* sample_lens;         // [B] out
    int32_t* status;              // int32[8] out: {frames, tiles, flags, longest utterance, valid samples, 0, 0, 0}
};

// One workgroup.  Thread t owns the utterances [t per, (t + 1) per); their sums are scanned across the block in LDS (Hillis-Steele).
// A length is clamped to [0, frame_capacity + 1] before it enters a sum, so no sum can overflow whatever lens holds.
__global__ __launch_bounds__(kGlPlanThreads) void gl_plan_scan(GlPlanArgs a) {
    __shared__ int64_t sL[kGlPlanThreads], sW[kGlPlanThreads], sT[kGlPlanThreads];
    __shared__ int sF[kGlPlanThreads], sM[kGlPlanThreads];
    const int tid = threadIdx.x, per = (a.B + kGlPlanThreads - 1) / kGlPlanThreads;
    const int b0 = min(a.B, tid * per), b1 = min(a.B, b0 + per);
    int64_t nL = 0, nW = 0, nT = 0;
    int fl = 0, mx = 0;
    for (int b = b0; b < b1; ++b) {
        int64_t L = a.lens[b];
        if (L < 0) { fl |= kGlOvfNegative; L = 0; }
        if (L > a.frame_capacity) { fl |= kGlOvfRows; L = a.frame_capacity + 1; }
        const int64_t T = (int64_t)a.hop * (L > 1 ? L - 1 : 0);
        if (a.src_stride && L > a.src_stride) fl |= kGlOvfLmax;
        if (a.wav_stride && T > a.wav_stride) fl |= kGlOvfLmax;
        nL += L; nW += T; nT += gl_tile_count((int)L, a.F);
        mx = max(mx, (int)L);
    }
    sL[tid] = nL; sW[tid] = nW; sT[tid] = nT; sF[tid] = fl; sM[tid] = mx;
    __syncthreads();
    for (int o = 1; o < kGlPlanThreads; o <<= 1) {
        int64_t pL = 0, pW = 0, pT = 0;
        int pF = 0, pM = 0;
        if (tid >= o) { pL = sL[tid - o]; pW = sW[tid - o]; pT = sT[tid - o]; pF = sF[tid - o]; pM = sM[tid - o]; }
        __syncthreads();
        sL[tid] += pL; sW[tid] += pW; sT[tid] += pT; sF[tid] |= pF; sM[tid] = max(sM[tid], pM);
        __syncthreads();
    }
    const int64_t frames = sL[kGlPlanThreads - 1], samples = sW[kGlPlanThreads - 1], tiles = sT[kGlPlanThreads - 1];
    int flags = sF[kGlPlanThreads - 1];
    if (frames > a.frame_capacity) flags |= kGlOvfRows;
    if (!a.wav_stride && samples > a.wav_capacity) flags |= kGlOvfWav;
    if (a.upstream && a.upstream[2] != 0) flags |= kGlOvfUpstream | a.upstream[2];
    // exclusive prefixes of this thread's first utterance, then the chunk once more
    int64_t rL = sL[tid] - nL, rW = sW[tid] - nW, rT = sT[tid] - nT;
    for (int b = b0; b < b1; ++b) {
        if (flags) {
            a.row0[b] = 0; a.wav0[b] = 0; a.tile_end[b] = 0; a.Lv[b] = 0; a.sample_lens[b] = 0;
            continue;
        }
        const int L = (int)a.lens[b];                   // validated: 0 <= L <= frame_capacity
        const int T = a.hop * max(L - 1, 0);
        rT += gl_tile_count(L, a.F);
        a.row0[b] = (int)rL;
        a.wav0[b] = a.wav_stride ? b * a.wav_stride : (int)rW;
        a.tile_end[b] = (int)rT;
        a.Lv[b] = L;
        a.sample_lens[b] = T;
        rL += L; rW += T;
    }
    if (tid == 0) {
        const int64_t big = 2147483647;
        a.status[0] = (int)(frames < big ? frames : big);
        a.status[1] = flags ? 0 : (int)tiles;
        a.status[2] = flags;
        a.status[3] = sM[kGlPlanThreads - 1];
        a.status[4] = flags ? 0 : (int)samples;
        a.status[5] = 0; a.status[6] = 0; a.status[7] = 0;
    }
}

// One thread per slot: the GlTile the host plan (griffin_lim_host.h: gl_plan) writes for the slot's tile, or an empty record.
__global__ void gl_plan_emit(GlPlanArgs a, int n_slots, GlTile* tiles) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    GlTile t{};
    if (a.status[2] == 0) {
        const GlSlot r = gl_slot_tile(a.tile_end, a.B, a.F, s);
        if (r.b >= 0) {
            const int L = a.Lv[r.b];
            t.ws_row0 = a.row0[r.b];
            t.src_row0 = a.src_stride ? r.b * a.src_stride : t.ws_row0;
            t.L = L; t.f0 = r.f0;
            t.wav0 = a.wav0[r.b];
            t.T = a.hop * (L - 1);
        }
    }
    tiles[s] = t;
}

// The samples no tile owns: zeros beyond the valid total (packed) or beyond each utterance's samples (padded); on any flag the whole
// capacity is NaN.  Grid-stride over wav_capacity.
__global__ void gl_plan_fill(GlPlanArgs a, float* wav) {
    const int flags = a.status[2];
    const int64_t valid = a.status[4], n = a.wav_capacity, step = (int64_t)gridDim.x * blockDim.x;
    const float nan = __int_as_float(0x7fc00000);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        if (flags) { wav[i] = nan; continue; }
        if (!a.wav_stride) {
            if (i >= valid) wav[i] = 0.f;
        } else {
            const int64_t b = i / a.wav_stride;
            if (b >= a.B || i - b * a.wav_stride >= a.sample_lens[b]) wav[i] = 0.f;
        }
    }
}

}  // namespace fs2
