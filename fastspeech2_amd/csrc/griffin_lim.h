// Griffin-Lim vocoder and the analysis STFT (fs2_op_griffin_lim / fs2_op_stft, include/fs2.h).
//
// Fixed transform: n_fft = win_length = 1024, hop = 256, 513 bins, periodic Hann window (the reference's configs/default.yaml
// audio values, utils/stft.py:41-151).  For an utterance of L frames (T = 256 (L - 1) samples):
//   ISTFT  x = OLA_f(w . irfft(C_f)) / wss, trimmed by 512 at both ends     (STFT.inverse, stft.py:112-151)
//   STFT   X_f = rfft(w . frame_f) of the signal reflect-padded by 512     (STFT.transform, stft.py:80-110)
//   GL     C = M . A / |A|, A = X - momentum / (1 + momentum) . T, T <- X   (griffin_lim, audio_processing.py:224-240; momentum 0 = reference)
// Utterances with L < 4 are too short for the reflect padding: their T samples are written as zeros and no iteration touches them.
//
// Work split.  A workgroup (256 threads = 4 waves) owns a tile of kGlTile consecutive frames of one utterance, tiles counted from the
// utterance's first frame.  It inverse-transforms its frames plus a halo of 3 frames on each side (exactly what the STFT of its frames
// reads, the reflect padding at both utterance ends included), overlap-adds them in LDS in increasing frame order, normalises by the
// window envelope, forward-transforms its own frames and writes their new complex spectrum C = M . phasor.  Every number depends only
// on the utterance's own frames and on utterance-local indices, never on the tile boundaries or the batch: an utterance comes out
// bit-identical whether it is vocoded alone or inside any batch, and a sample computed by two tiles (halo) is the same in both.
// No atomics: results are deterministic.  The spectra ping-pong between two workspace buffers across iterations.
//
// FFT.  A 1024-point real transform is a 512-point complex one (z[m] = x[2m] + i x[2m+1]) plus a split pass.  The complex transform is
// a radix-8 Stockham sequence of three passes, one wave per transform: lane j holds 8 complex values in registers, the in-register
// 8-point DFT is three radix-2 layers, the passes exchange through a 4 KB LDS buffer per wave.  Twiddles and the window come from a
// table the table kernel writes once per call (double precision, rounded to fp32).  All arithmetic fp32 on the VALU.
//
// Budget (shapes, c3 = 35.6 k frames): per iteration the fused kernel reads C of (F + 6) / F frames (4104 B each) and M (2052 B) and
// writes C (4104 B) per frame: ~0.42 GB at F = 32, ~70 us at 6 TB/s; FFT work ~2.4 real 1024-point transforms per frame, ~60 kFLOP,
// ~2.2 GFLOP per iteration (~14 us at 157 TF).  The LDS traffic of the three passes (~0.3 MB per frame and iteration, ~11 GB) at
// ~80 TB/s of LDS bandwidth is the tightest bound (~0.14 ms); measured figures: BASELINE.md section 5.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fs2 {

constexpr int kGlNfft = 1024, kGlHop = 256, kGlBins = 513, kGlHalo = 3, kGlTile = 32, kGlThreads = 256;
constexpr int kGlTilesPerChunk = 120;        // tile records per upload launch (kernel-argument bytes: 120 * 32 + 8 < 4 KB)

// One tile: frames [f0, f0 + kGlTile) of an utterance (clipped to L).  Written to the workspace by gl_upload_tiles from kernel
// arguments, so the call needs no host-to-device copy and no host synchronisation.
struct GlTile {
    int src_row0;   // packed row of the utterance's frame 0 in the caller's source (mel / magnitude rows, or analysis frames)
    int ws_row0;    // packed row of the utterance's frame 0 in the workspace spectra (prefix sum of L)
    int L;          // frames of the utterance
    int f0;         // first frame of this tile, utterance-local
    int wav0;       // first sample of the utterance in the packed waveform
    int T;          // samples of the utterance (analysis: as given; synthesis: 256 (L - 1))
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

// tw[m] = exp(-2 pi i m / 1024), win[n] = periodic Hann (scipy.signal.get_window("hann", 1024, fftbins=True)), from double.
__global__ void gl_tables(float2* tw, float* win) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= kGlNfft) return;
    double s, c;
    sincospi((double)m / 512.0, &s, &c);
    tw[m] = make_float2((float)c, (float)-s);
    win[m] = (float)(0.5 - 0.5 * c);
}

// ---- seeded initial phase: counter-based, keyed by (seed, utterance-local frame, bin); restated in fastspeech2_amd/vocoder.py ----
__host__ __device__ inline uint32_t gl_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ inline float gl_seed_angle(uint32_t seed, uint32_t f, uint32_t k) {
#pragma clang fp contract(off)     // two roundings, no FMA: the host restatement (vocoder.seed_angles) computes the same bits
    const uint32_t h = gl_mix32((k + 513u * f) ^ gl_mix32(seed + 0x9E3779B9u));
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f);                          // exact
    return u * 6.28318548f - 3.14159274f;                                             // uniform on [-pi, pi)
}

// Prologue, one workgroup per tile: M = max(P . exp(mel), 0) (src_width 80; P = pinv(mel basis) [513, 80]) or M = src (src_width 513),
// C0 = M . exp(i theta0) with theta0 given [rows of src, 513] or seeded; the momentum state T = 0.
__global__ __launch_bounds__(kGlThreads) void gl_prologue(const GlTile* tiles, const float* src, int src_width, const float* pinv,
                                                          const float* init_phase, uint32_t seed, float* M, float2* C, float2* Tm) {
    const GlTile t = tiles[blockIdx.x];
    if (t.L < 4) return;          // never iterated, never read (the final ISTFT writes zeros)
    const int nf = min(kGlTile, t.L - t.f0);
    __shared__ float e[kGlTile][80];
    if (src_width == 80) {
        for (int i = threadIdx.x; i < nf * 80; i += kGlThreads) {
            const int f = i / 80, j = i - f * 80;
            e[f][j] = expf(src[(int64_t)(t.src_row0 + t.f0 + f) * 80 + j]);
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < kGlBins; k += kGlThreads) {
        float acc[kGlTile];
        if (src_width == 80) {
#pragma unroll
            for (int f = 0; f < kGlTile; ++f) acc[f] = 0.f;
            const float4* p = reinterpret_cast<const float4*>(pinv + (int64_t)k * 80);
            for (int j4 = 0; j4 < 20; ++j4) {
                const float4 q = p[j4];
#pragma unroll
                for (int f = 0; f < kGlTile; ++f) {
                    if (f < nf)
                        acc[f] += q.x * e[f][4 * j4] + q.y * e[f][4 * j4 + 1] + q.z * e[f][4 * j4 + 2] + q.w * e[f][4 * j4 + 3];
                }
            }
        }
#pragma unroll
        for (int f = 0; f < kGlTile; ++f) {
            if (f < nf) {
                const int fl = t.f0 + f;
                const float m = src_width == 80 ? fmaxf(acc[f], 0.f) : src[(int64_t)(t.src_row0 + fl) * kGlBins + k];
                const float th = init_phase ? init_phase[(int64_t)(t.src_row0 + fl) * kGlBins + k] : gl_seed_angle(seed, (uint32_t)fl, (uint32_t)k);
                float s, c;
                sincosf(th, &s, &c);
                const int64_t o = (int64_t)(t.ws_row0 + fl) * kGlBins + k;
                M[o] = m;
                C[o] = make_float2(m * c, m * s);
                if (Tm) Tm[o] = make_float2(0.f, 0.f);
            }
        }
    }
}

// ---- 512-point complex FFT, one wave, lane j holds v[r] = z[j + 64 r] on entry and Z[j + 64 r] on exit ----
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

// Frame f's inverse: x[n] = w[n] irfft(C_f)[n] into out[0..1023] (the wave's scratch, viewed as floats).  Bins 0 and 512 lose their
// imaginary parts (what the reference's pinv basis does).
__device__ inline void gl_frame_istft(const float2* __restrict__ Cf, bool valid, float2* buf, const float2* tw, const float* win, int j) {
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k = j + 64 * r;                       // Z[k] = E[k] + i O[k] (x 2: the 1/1024 is applied at the end)
        float2 a = make_float2(0.f, 0.f), b = a;
        if (valid) { a = Cf[k]; b = Cf[512 - k]; }
        if (k == 0) { a.y = 0.f; b.y = 0.f; }
        const float2 E = make_float2(a.x + b.x, a.y - b.y);
        const float2 t = tw[k];                          // O = (a - conj b) exp(+2 pi i k / 1024)
        const float2 O = cmul(make_float2(a.x - b.x, a.y + b.y), make_float2(t.x, -t.y));
        v[r] = make_float2(E.x - O.y, E.y + O.x);
    }
    fft512<1>(v, buf, tw, j);
    __syncthreads();
    float* out = reinterpret_cast<float*>(buf);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int m = j + 64 * r;
        out[2 * m] = v[r].x * (1.0f / 1024.0f) * win[2 * m];
        out[2 * m + 1] = v[r].y * (1.0f / 1024.0f) * win[2 * m + 1];
    }
}

// Forward: v[r] = z[j + 64 r] (windowed, packed real pairs) -> lane j gets X[j + 64 r] in X[r]; lane 0 also X[512] in x512.
__device__ inline void gl_frame_rfft(float2* v, float2* X, float2& x512, float2* buf, const float2* tw, int j) {
    fft512<-1>(v, buf, tw, j);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) buf[j + 64 * r] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int k = j + 64 * r;
        const float2 a = v[r], b = buf[(512 - k) & 511];
        const float2 E = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
        const float2 O = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));     // (a - conj b) / (2 i)
        X[r] = cadd(E, cmul(tw[k], O));
    }
    x512 = make_float2(v[0].x - v[0].y, 0.f);           // X[512] = E[0] - O[0] (meaningful on lane 0)
}

// window envelope at pre-trim position p of an utterance of L frames (window_sumsquare, audio_processing.py:171-222: frames in order)
__device__ inline float gl_wss(int p, int L, const float* win) {
    const int fa = max(0, (p - kGlNfft + kGlHop) / kGlHop), fb = min(L - 1, p / kGlHop);
    float s = 0.f;
    for (int f = fa; f <= fb; ++f) {
        const int n = p - kGlHop * f;
        if (n < kGlNfft) { const float w = win[n]; s += w * w; }
    }
    return s;
}

constexpr int kGlSigMax = kGlHop * (kGlTile + 2 * kGlHalo - 1) + kGlNfft;   // pre-trim samples a tile's frames + halo span

// MODE 0: one Griffin-Lim iteration, C_in -> C_out for the tile's own frames.  MODE 1: the final ISTFT, writes the tile's samples
// [256 f0, 256 (f0 + kGlTile)) of the waveform (zeros for L < 4).
template <int MODE, bool MOMENTUM>
__global__ __launch_bounds__(kGlThreads) void gl_iterate(const GlTile* tiles, const float2* gtw, const float* gwin, const float* M,
                                                         const float2* Cin, float2* Cout, float2* Tm, float beta, float* wav) {
    __shared__ float2 tw[kGlNfft];
    __shared__ float win[kGlNfft];
    __shared__ float2 scratch[4][512];
    __shared__ float sig[kGlSigMax];
    const GlTile t = tiles[blockIdx.x];
    const int L = t.L, T = kGlHop * (L - 1);
    if (L < 4) {          // too short for the reflect padding: documented zeros
        if (MODE == 1)
            for (int s = kGlHop * t.f0 + threadIdx.x; s < min(T, kGlHop * (t.f0 + kGlTile)); s += kGlThreads) wav[t.wav0 + s] = 0.f;
        return;
    }
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int i = tid; i < kGlNfft; i += kGlThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    const int nf = min(kGlTile, L - t.f0);
    // halo: 3 frames each side; a tile that starts at the utterance's last frame also needs frame L - 5 (the reflection of its last
    // sample, 256 (L - 1) - 513, lies below 256 (f0 - 2))
    const int fa = max(0, min(t.f0 - kGlHalo, L - 5)), fb = min(L - 1, t.f0 + nf - 1 + kGlHalo), nh = fb - fa + 1;
    const int SL = kGlHop * (fb - fa) + kGlNfft;          // <= kGlSigMax
    for (int q = tid; q < SL; q += kGlThreads) sig[q] = 0.f;
    // ---- ISTFT of frames fa..fb, four per round (wave w: frame fa + 4 k + w), overlap-added in frame order ----
    for (int k = 0; k < nh; k += 4) {
        const int f = fa + k + wv;
        const bool valid = f <= fb;
        gl_frame_istft(Cin + (int64_t)(t.ws_row0 + min(f, fb)) * kGlBins, valid, scratch[wv], tw, win, j);
        __syncthreads();
        const int q0 = kGlHop * k, q1 = min(SL, q0 + 3 * kGlHop + kGlNfft);
        for (int q = q0 + tid; q < q1; q += kGlThreads) {
            float acc = sig[q];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int n = q - kGlHop * (k + w);
                if (k + w < nh && n >= 0 && n < kGlNfft) acc += reinterpret_cast<const float*>(scratch[w])[n];
            }
            sig[q] = acc;
        }
    }
    __syncthreads();
    for (int q = tid; q < SL; q += kGlThreads) {
        const float s = gl_wss(kGlHop * fa + q, L, win);
        if (s > 1.17549435e-38f) sig[q] = sig[q] / s;
    }
    __syncthreads();
    const int qoff = kGlNfft / 2 - kGlHop * fa;             // trimmed sample s lives at sig[s + qoff]
    if (MODE == 1) {
        const int s1 = min(T, kGlHop * (t.f0 + nf));
        for (int s = kGlHop * t.f0 + tid; s < s1; s += kGlThreads) wav[t.wav0 + s] = sig[s + qoff];
        return;
    }
    // ---- STFT of the own frames, projection onto M ----
    for (int k = 0; k < nf; k += 4) {
        const int f = t.f0 + k + wv;
        const bool valid = k + wv < nf;
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = 2 * (j + 64 * r);
            float x[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int s = kGlHop * f - kGlNfft / 2 + n + u;
                s = s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s);
                x[u] = valid ? sig[s + qoff] * win[n + u] : 0.f;
            }
            v[r] = make_float2(x[0], x[1]);
        }
        float2 X[8], x512;
        gl_frame_rfft(v, X, x512, scratch[wv], tw, j);
        if (valid) {
            const int64_t row = (int64_t)(t.ws_row0 + f) * kGlBins;
#pragma unroll
            for (int r = 0; r <= 8; ++r) {
                if (r == 8 && j) break;
                const int k2 = r == 8 ? 512 : j + 64 * r;
                const float2 x = r == 8 ? x512 : X[r];
                float2 a = x;
                if (MOMENTUM) { const float2 tp = Tm[row + k2]; a = make_float2(x.x - beta * tp.x, x.y - beta * tp.y); Tm[row + k2] = x; }
                const float mag = sqrtf(a.x * a.x + a.y * a.y);
                const float m = M[row + k2];
                Cout[row + k2] = mag > 0.f ? make_float2(m * (a.x / mag), m * (a.y / mag)) : make_float2(m, 0.f);
            }
        }
    }
}

// Analysis STFT, one workgroup per tile of frames: |X| [rows, 513] and optionally log(clamp(B . |X|, 1e-5)) [rows, 80].
// Utterances shorter than 513 samples (no reflect padding possible) give |X| = 0 and log-mel = log(1e-5).
__global__ __launch_bounds__(kGlThreads) void gl_stft(const GlTile* tiles, const float2* gtw, const float* gwin, const float* wavp,
                                                      float* mag, const float* basis, float* logmel) {
    __shared__ float2 tw[kGlNfft];
    __shared__ float win[kGlNfft];
    __shared__ float2 scratch[4][512];
    const GlTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int i = tid; i < kGlNfft; i += kGlThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    const int nf = min(kGlTile, t.L - t.f0), T = t.T;
    const bool ok = T > kGlNfft / 2;
    const float* x = wavp + t.wav0;
    for (int k = 0; k < nf; k += 4) {
        const int f = t.f0 + k + wv;
        const bool valid = k + wv < nf;
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = 2 * (j + 64 * r);
            float xx[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int s = kGlHop * f - kGlNfft / 2 + n + u;
                s = s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s);
                xx[u] = (valid && ok) ? x[s] * win[n + u] : 0.f;
            }
            v[r] = make_float2(xx[0], xx[1]);
        }
        float2 X[8], x512;
        gl_frame_rfft(v, X, x512, scratch[wv], tw, j);
        __syncthreads();
        float* am = reinterpret_cast<float*>(scratch[wv]);   // |X| of this wave's frame, 513 floats
#pragma unroll
        for (int r = 0; r < 8; ++r) am[j + 64 * r] = sqrtf(X[r].x * X[r].x + X[r].y * X[r].y);
        if (j == 0) am[512] = fabsf(x512.x);
        __syncthreads();
        if (valid) {
            const int64_t row = (int64_t)(t.src_row0 + f);
            if (mag)
                for (int b = j; b < kGlBins; b += 64) mag[row * kGlBins + b] = am[b];
            if (logmel)
                for (int c = j; c < 80; c += 64) {
                    const float* br = basis + c * kGlBins;
                    float acc = 0.f;
                    for (int b = 0; b < kGlBins; ++b) acc += br[b] * am[b];
                    logmel[row * 80 + c] = logf(fmaxf(acc, 1e-5f));
                }
        }
    }
}

}  // namespace fs2
