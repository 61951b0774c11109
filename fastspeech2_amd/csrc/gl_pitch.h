// Pitch (F0) beside the analysis STFT: fs2_op_stft_pitch_geom (include/fs2.h).  Included by griffin_lim.h's
// users right after it; everything the STFT itself needs (tables, tiles, the per-wave FFT) is griffin_lim.h's, unchanged.
//
// The estimator is an autocorrelation one (Boersma 1993 without the path search, parabolic instead of sinc interpolation).  It is not
// the reference's pitch, which comes from pyworld's DIO (dataset/audio_processing.py:54-70).  Per frame, with y the windowed frame:
//   r = irfft(|rfft(y)|^2)                      circular autocorrelation of y, r[0] = sum y^2; r[0] <= 1e-12: unvoiced, strength 0
//   rho[t] = (r[t] / r[0]) / (rw[t] / rw[0])    rw the same of the window, in double (gl_pitch_table)
//   candidates t in [tmin, tmax]: rho[t] > rho[t-1], rho[t] >= rho[t+1], rho[t] > 0; a, c, b = rho[t-1], rho[t], rho[t+1]
//   d = 0.5 (a - b) / (a - 2c + b), t* = t + d, p = c - 0.25 (a - b) d, S = p - octave_cost log2(f0_floor t* / sr)
//   winner: the largest S, ties to the smaller t; voiced iff p >= voicing_threshold; f0 = sr / t* or 0; strength = p (0: no candidate)
//
// gl_features is gl_stft plus, per wave and frame, one more inverse transform and a lag scan.  The frame's |X|^2 goes to a per-wave
// LDS buffer (the inverse's split pass reads bins k and N/2 - k), the inverse runs in the wave's FFT scratch as gl_frame_istft does,
// and its last step multiplies by the table rw[0] / rw[t] where gl_frame_istft multiplies by the window.  Lanes stride over the lags,
// each keeps its best (S, t), a fixed xor butterfly reduces them (larger S, then smaller t: every lane ends with the same winner) and
// lane 0 writes f0 and strength.  No atomics; a frame's numbers depend on its own samples only.  The |X|, log-mel and energy code is
// gl_stft's, statement for statement: their bits are gl_stft's.
//
// gl_candidates (fs2_op_stft_pitch_cands_geom) is gl_features with another scan at its end: instead of the
// winner it writes the first K candidates in the order "larger S, then smaller t" (sr / t* and p; empty slots 0 / 0), which the path
// search of pitch_path.h takes.  It is a kernel of its own and gl_features is left as it was, text and code: an earlier form that
// shared one body between the two changed the last bit of gl_features' log-mel at n_fft = 2048.
#pragma once
#include "griffin_lim.h"

namespace fs2 {

struct GlPitch {
    int tmin, tmax;           // candidate lags, 2 <= tmin <= tmax <= win / 2 (checked on the host)
    float sr;                 // sample rate
    float floor_over_sr;      // f0_floor / sr
    float threshold;          // voicing threshold on the winner's p
    float octave_cost;
};

// acw[t] = rw[0] / rw[t] for t <= wl / 2 + 1 (what a lag scan up to wl / 2 reads), 0 up to the table's end at N / 2 + 1;
// rw[t] = sum_n w[n] w[(n + t) mod N] of the window gl_tables writes, here in double throughout.  A block of 256 threads owns 8
// lags, 32 lanes each; the partial sums meet in a fixed butterfly.
constexpr int gl_pitch_lags(int n_fft) { return n_fft / 2 + 2; }      // entries of the table

__global__ __launch_bounds__(256) void gl_pitch_table(float* acw, int n, int wl) {
    __shared__ double w[2048];
    const int lp = (n - wl) / 2;
    for (int m = threadIdx.x; m < n; m += 256) {
        double s, c;
        sincospi(2.0 * (double)(m - lp) / (double)wl, &s, &c);
        w[m] = (m >= lp && m < lp + wl) ? 0.5 - 0.5 * c : 0.0;
    }
    __syncthreads();
    const int t = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    const bool used = t <= wl / 2 + 1;       // <= N / 2 + 1
    double r0 = 0.0, rt = 0.0;
    if (used)
        for (int m = l; m < n; m += 32) {
            r0 += w[m] * w[m];
            rt += w[m] * w[(m + t) & (n - 1)];
        }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
        r0 += __shfl_xor(r0, o);
        rt += __shfl_xor(rt, o);
    }
    if (l == 0 && t < gl_pitch_lags(n)) acw[t] = (used && rt > 0.0) ? (float)(r0 / rt) : 0.f;
}

// The wave's frame autocorrelation: P[0 .. N/2] = |X|^2 (LDS) -> out[t] = irfft(P)[t] . acw[t] for t <= N / 2 + 1 in buf (as floats).
// (WHO: one instantiation per calling kernel.  With a single caller the compiler inlines it, which is the code gl_features has always
// had; with two it turns the 2048-point one into a function call.)
template <int NFFT, int WHO = 0>
__device__ inline void gl_frame_autocorr(const float* P, float2* buf, const float2* tw, const float* acw, int j) {
    constexpr int N2 = NFFT / 2, V = N2 / 64;
    float2 v[V];
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int k = j + 64 * r;                        // gl_frame_istft's split pass with a real spectrum
        const float a = P[k], b = P[N2 - k];
        const float2 t = tw[k];
        const float2 O = make_float2((a - b) * t.x, -(a - b) * t.y);
        v[r] = make_float2((a + b) - O.y, O.x);
    }
    fft_c<N2, 1>(v, buf, tw, j);
    __syncthreads();
    float* out = reinterpret_cast<float*>(buf);
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int m = j + 64 * r;
        if (2 * m < gl_pitch_lags(NFFT)) {               // the lags the table covers (the scan reads up to win / 2 + 1)
            out[2 * m] = v[r].x * (1.0f / NFFT) * acw[2 * m];
            out[2 * m + 1] = v[r].y * (1.0f / NFFT) * acw[2 * m + 1];
        }
    }
}

// gl_stft (same arguments, same |X| / log-mel / energy) plus f0 [rows] and strength [rows], each optional.
template <int NFFT, int HOP_C>
__global__ __launch_bounds__(kGlThreads) void gl_features(const GlTile* tiles, GlGeom g, const float2* gtw, const float* gwin, const float* gacw,
                                                          const float* wavp, float* mag, const float* basis, float* logmel, float* energy,
                                                          GlPitch pp, float* f0, float* strength) {
    constexpr int N2 = NFFT / 2, V = N2 / 64, NB = N2 + 1;
    __shared__ float2 tw[NFFT];
    __shared__ float win[NFFT];
    __shared__ float acw[gl_pitch_lags(NFFT)];
    __shared__ float2 scratch[4][N2];
    __shared__ float pw[4][NB];
    const int hop = HOP_C ? HOP_C : g.hop, nm = g.n_mels;
    const GlTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int i = tid; i < NFFT; i += kGlThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    for (int i = tid; i < gl_pitch_lags(NFFT); i += kGlThreads) acw[i] = gacw[i];
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
        float* P = pw[wv];                                   // |X|^2 of it
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const float p2 = X[r].x * X[r].x + X[r].y * X[r].y;
            am[j + 64 * r] = sqrtf(p2);
            P[j + 64 * r] = p2;
        }
        if (j == 0) { am[N2] = fabsf(xl.x); P[N2] = xl.x * xl.x; }
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
        // ---- pitch: rho[t] = rc[t] / rc[0] with rc = irfft(|X|^2) . rw[0] / rw ----
        gl_frame_autocorr<NFFT>(P, scratch[wv], tw, acw, j);
        __syncthreads();
        const float* rc = reinterpret_cast<const float*>(scratch[wv]);
        const float r0 = rc[0];
        float bS = -INFINITY, bT = 0.f, bP = 0.f;      // this lane's best candidate: S, t*, p
        int bt = 0x7fffffff;                           // its integer lag
        if (r0 > 1e-12f)
            for (int tau = pp.tmin + j; tau <= pp.tmax; tau += 64) {
                const float a = rc[tau - 1] / r0, c = rc[tau] / r0, b = rc[tau + 1] / r0;
                if (c > a && c >= b && c > 0.f) {
                    const float d = 0.5f * (a - b) / ((a - c) + (b - c));
                    const float ts = (float)tau + d, p = c - 0.25f * (a - b) * d;
                    const float S = p - pp.octave_cost * log2f(pp.floor_over_sr * ts);
                    if (S > bS) { bS = S; bT = ts; bP = p; bt = tau; }      // lags ascend: an equal S keeps the smaller lag
                }
            }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float oS = __shfl_xor(bS, o), oT = __shfl_xor(bT, o), oP = __shfl_xor(bP, o);
            const int ot = __shfl_xor(bt, o);
            if (oS > bS || (oS == bS && ot < bt)) { bS = oS; bT = oT; bP = oP; bt = ot; }
        }
        if (valid && j == 0) {
            const bool cand = bt != 0x7fffffff;
            if (f0) f0[t.src_row0 + f] = (cand && bP >= pp.threshold) ? pp.sr / bT : 0.f;
            if (strength) strength[t.src_row0 + f] = cand ? bP : 0.f;
        }
    }
}

// gl_features with another scan at its end: cand_f0 [rows, K] = sr / t* and cand_strength [rows, K] = p of the first K candidates per
// frame in the order "larger S, then smaller lag" (1 <= K <= FS2_PITCH_MAX_CANDS, checked on the host; empty slots 0 / 0), each
// optional, in place of the winner's f0 and strength.  Everything up to the scan is gl_features' text, statement for statement, so
// that rho, and with it slot 0, carries gl_features' bits (tests/test_gpu_pitch_path.py holds it to that); the host asks this kernel
// for the candidates alone (gl_analyze takes |X|, log-mel and energy from gl_stft itself), so those statements are skipped at run time.
template <int NFFT, int HOP_C>
__global__ __launch_bounds__(kGlThreads) void gl_candidates(const GlTile* tiles, GlGeom g, const float2* gtw, const float* gwin, const float* gacw,
                                                            const float* wavp, float* mag, const float* basis, float* logmel, float* energy,
                                                            GlPitch pp, int K, float* cand_f0, float* cand_strength) {
    constexpr int N2 = NFFT / 2, V = N2 / 64, NB = N2 + 1;
    __shared__ float2 tw[NFFT];
    __shared__ float win[NFFT];
    __shared__ float acw[gl_pitch_lags(NFFT)];
    __shared__ float2 scratch[4][N2];
    __shared__ float pw[4][NB];
    const int hop = HOP_C ? HOP_C : g.hop, nm = g.n_mels;
    const GlTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    for (int i = tid; i < NFFT; i += kGlThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    for (int i = tid; i < gl_pitch_lags(NFFT); i += kGlThreads) acw[i] = gacw[i];
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
        float* P = pw[wv];                                   // |X|^2 of it
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const float p2 = X[r].x * X[r].x + X[r].y * X[r].y;
            am[j + 64 * r] = sqrtf(p2);
            P[j + 64 * r] = p2;
        }
        if (j == 0) { am[N2] = fabsf(xl.x); P[N2] = xl.x * xl.x; }
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
        // ---- pitch: rho[t] = rc[t] / rc[0] with rc = irfft(|X|^2) . rw[0] / rw ----
        gl_frame_autocorr<NFFT, 1>(P, scratch[wv], tw, acw, j);
        __syncthreads();
        const float* rc = reinterpret_cast<const float*>(scratch[wv]);
        const float r0 = rc[0];
        // The lane's lags are scored once into registers, with gl_features' statements (a lane owns at most NFFT / 128 of the at most
        // NFFT / 2 - 1 lags; -inf: no candidate there).  p is spelled with two roundings, as the compiler makes it in gl_features, where
        // left to itself it fuses them in this unrolled form.  Then K rounds of gl_features' lane scan and butterfly, each admitting
        // only what comes strictly after the previous round's winner in the order (S, then lag); round 0 admits everything: it is
        // gl_features' scan.  All 64 lanes take part in every shuffle of every round (K is the same for all); a round without a winner
        // writes 0 / 0, and so does every round after it.
        constexpr int NL = NFFT / 128;
        float cS[NL], cT[NL], cP[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int tau = pp.tmin + j + 64 * i;
            cS[i] = -INFINITY; cT[i] = 0.f; cP[i] = 0.f;
            if (r0 > 1e-12f && tau <= pp.tmax) {
                const float a = rc[tau - 1] / r0, c = rc[tau] / r0, b = rc[tau + 1] / r0;
                if (c > a && c >= b && c > 0.f) {
                    const float d = 0.5f * (a - b) / ((a - c) + (b - c));
                    const float ts = (float)tau + d;
                    float p;
                    {
#pragma clang fp contract(off)
                        p = c - 0.25f * (a - b) * d;
                    }
                    cS[i] = fmaf(-pp.octave_cost, log2f(pp.floor_over_sr * ts), p);
                    cT[i] = ts;
                    cP[i] = p;
                }
            }
        }
        float pS = INFINITY;                           // the previous round's winner
        int pt = -1;
        for (int r = 0; r < K; ++r) {
            float bS = -INFINITY, bT = 0.f, bP = 0.f;
            int bt = 0x7fffffff;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int tau = pp.tmin + j + 64 * i;
                const bool after = cS[i] < pS || (cS[i] == pS && tau > pt);
                if (after && cS[i] > bS) { bS = cS[i]; bT = cT[i]; bP = cP[i]; bt = tau; }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float oS = __shfl_xor(bS, o), oT = __shfl_xor(bT, o), oP = __shfl_xor(bP, o);
                const int ot = __shfl_xor(bt, o);
                if (oS > bS || (oS == bS && ot < bt)) { bS = oS; bT = oT; bP = oP; bt = ot; }
            }
            if (valid && j == 0) {
                const bool cand = bt != 0x7fffffff;
                const int64_t slot = (int64_t)(t.src_row0 + f) * K + r;
                if (cand_f0) cand_f0[slot] = cand ? pp.sr / bT : 0.f;
                if (cand_strength) cand_strength[slot] = cand ? bP : 0.f;
            }
            pS = bS;
            pt = bt;
        }
    }
}

}  // namespace fs2
