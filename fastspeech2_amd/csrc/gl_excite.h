// Excitation from F0 and its STFT phase as the initial phase of Griffin-Lim: fs2_op_excitation_geom / _dev and fs2_op_f0_phase_geom /
// _dev (include/fs2.h).  The phase goes to gl_prologue through the init_phase pointer it has always had; no
// kernel of griffin_lim.h changes.  With n_iter = 0 the vocoder is then a one-pass source-filter synthesis: the magnitudes filter the
// excitation, and the pitch of the waveform is the commanded one.
//
// Semantics (tests/excitation_oracle.py states them in numpy).  Per utterance: L frames, hop H, f0[0..L-1] float32 in Hz, N = H (L - 1)
// samples, frame t centred on sample t H.  A frame is voiced iff f0[t] is finite and f0_floor <= f0[t] <= f0_ceil; segment t (samples
// t H .. t H + H - 1, t <= L - 2) is voiced iff frames t and t + 1 are, then a = f0[t], d = f0[t+1] - f0[t], else a = d = 0.  In double,
// every operation rounded on its own:
//   S_t = (H a + d (H - 1) 0.5) / sr;  Theta_0 = 0, Theta_{t+1} = frac(Theta_t + S_t) in frame order               (turns)
//   sample n = t H + i: theta = frac(Theta_t + ((i + 1) a + (d (i (i + 1))) / (2 H)) / sr), f = a + (d i) / H,
//   Hn = the largest integer with Hn f < sr / 2, at least 1
//   voiced:   e[n] = sqrt(2 / Hn) sum_{h = 1..Hn} cos(2 pi h theta), evaluated in float32 as sin((Hn + 1/2) x) / (2 sin(x / 2)) - 1/2
//             with both arguments reduced in double to at most a quarter turn first (and the limit Hn at theta = 0)
//   unvoiced: e[n] = (u - 0.5) sqrt(12), u = (gl_mix32(n ^ gl_mix32(seed + 0x9E3779B9)) >> 8) / 2^24, n utterance-local
//   phase[t][k] = atan2f(Im, Re) of the STFT of e as gl_stft transforms a waveform (reflect padding, the window and twiddle table of
//   gl_tables, gl_frame_rfft); 0 where both parts are 0; every row 0 where N <= n_fft / 2.
//
// Work split.  Only Theta chains the frames.
//   exc_prefix   one workgroup per utterance: S_t of 256 frames at a time in parallel into LDS, then one lane adds them in frame order
//                (L double additions of the longest utterance: microseconds) and writes Theta per workspace row.
//   exc_samples  one workgroup per workspace row (= segment): every sample is a closed form of Theta_t, a, d and i.
//   exc_phase    one workgroup per kExcTile workspace rows, one wave per frame: reads the excitation exc_samples wrote (so the phase is
//                by construction that of the float32 samples fs2_op_excitation_* returns), transforms, writes atan2f.
// An utterance's result depends on its own rows alone: the same bits alone or in any batch, packed or padded, host-planned or
// device-driven.  Vector stores and plain C++; no atomics.
//
// Budget from shapes at c3 (35.6 k frames, 64 utterances, longest ~1,000, hop 256): exc_samples writes 9.1 M samples (36 MB) at ~40
// double and ~60 float operations each, ~1 GFLOP: tens of us.  exc_phase reads them 4 times over (n_fft / hop) from L2 / HBM (146 MB),
// does 35.6 k real 1024-point transforms (~25 kFLOP each, ~0.9 GFLOP) and writes 35.6 k x 513 x 4 B = 73 MB: tens of us, below
// spsi_chain's serial ~0.1 - 0.2 ms.  exc_prefix: ~1,000 LDS reads and double additions in one lane, ~0.1 ms worst case, on 64 CUs.
// Measured: BASELINE.md section 5.19 (f0_phase 0.18 ms beside spsi_phase's 0.44 ms).
//
// Not a header of its own: the includer provides, before it, float2 / make_float2, fs2::gl_mix32, fs2::gl_tables and
// fs2::gl_frame_rfft<NFFT> -- griffin_lim.h in fs2_runtime.hip, a shim in tests/kernel_standin/excitation_main.cpp.
#pragma once
#include <stdint.h>

namespace fs2 {

constexpr int kExcThreads = 256, kExcTile = 32;
constexpr int kExcUttsPerChunk = 240;                   // records per upload launch (kernel-argument bytes: 240 * 16 + 16 < 4 KB)

// One utterance: L values from src_row0 of the caller's f0 (and rows of phase), from ws_row0 of the workspace (prefix sum of L), its
// hop (L - 1) samples from wav0 of the output (the caller's waveform, or the workspace's excitation buffer).
struct ExcUtt {
    int src_row0, ws_row0, L, wav0;
};
struct ExcUttChunk {
    int n, base, frames, samples;
    ExcUtt u[kExcUttsPerChunk];
};
// hdr[0] = workspace rows in use (sum of L), hdr[1] = flags (FS2_OVF_*; != 0: every record is empty and nothing is computed),
// hdr[2] = samples (sum of hop max(L - 1, 0))
constexpr int kExcHdrInts = 4;

struct ExcOptions {
    double f0_floor, f0_ceil, sr;
    uint32_t seed;
    int hop;
};

// Host-planned call: records from kernel arguments (no host copy, no synchronisation).
__global__ void exc_upload(ExcUttChunk c, ExcUtt* utt, int* hdr) {
    const int i = threadIdx.x;
    if (i < c.n) utt[c.base + i] = c.u[i];
    if (i == 0 && c.base == 0) { hdr[0] = c.frames; hdr[1] = 0; hdr[2] = c.samples; hdr[3] = 0; }
}

// Device-driven call, one workgroup: validates the frame counts before anything is indexed with them, then writes the records.
// Thread t owns the utterances [t per, (t + 1) per); a length is clamped to [0, frame_capacity + 1] before it enters a sum, so no sum
// overflows whatever lens holds.  Flags as gl_plan_scan's (griffin_lim.h): 64 negative, 1 rows, 2 longer than src_stride, 32 | upstream,
// 128 the samples do not fit wav_stride / wav_capacity.  wav_stride 0: the waveforms packed back to back, else utterance b at b wav_stride.
__global__ __launch_bounds__(kExcThreads) void exc_plan(const int64_t* lens, const int32_t* upstream, int B, int src_stride, int64_t frame_capacity,
                                                       int hop, int wav_stride, int64_t wav_capacity, ExcUtt* utt, int* hdr) {
    __shared__ int64_t sL[kExcThreads], sW[kExcThreads];
    __shared__ int sF[kExcThreads];
    const int tid = threadIdx.x, per = (B + kExcThreads - 1) / kExcThreads;
    const int b0 = min(B, tid * per), b1 = min(B, b0 + per);
    int64_t nL = 0, nW = 0;
    int fl = 0;
    for (int b = b0; b < b1; ++b) {
        int64_t L = lens[b];
        if (L < 0) { fl |= 64; L = 0; }
        if (L > frame_capacity) { fl |= 1; L = frame_capacity + 1; }
        if (src_stride && L > src_stride) fl |= 2;
        const int64_t T = (int64_t)hop * (L > 1 ? L - 1 : 0);
        if (wav_stride && T > wav_stride) fl |= 128;
        nL += L;
        nW += T;
    }
    sL[tid] = nL; sW[tid] = nW; sF[tid] = fl;
    __syncthreads();
    for (int o = 1; o < kExcThreads; o <<= 1) {
        int64_t pL = 0, pW = 0;
        int pF = 0;
        if (tid >= o) { pL = sL[tid - o]; pW = sW[tid - o]; pF = sF[tid - o]; }
        __syncthreads();
        sL[tid] += pL; sW[tid] += pW; sF[tid] |= pF;
        __syncthreads();
    }
    const int64_t frames = sL[kExcThreads - 1], samples = sW[kExcThreads - 1];
    int flags = sF[kExcThreads - 1];
    if (frames > frame_capacity) flags |= 1;
    if (!wav_stride && samples > wav_capacity) flags |= 128;
    if (upstream && upstream[2] != 0) flags |= 32 | upstream[2];
    int64_t rL = sL[tid] - nL, rW = sW[tid] - nW;
    for (int b = b0; b < b1; ++b) {
        ExcUtt u{};
        if (!flags) {
            const int L = (int)lens[b];                  // validated: 0 <= L <= frame_capacity
            u.ws_row0 = (int)rL;
            u.src_row0 = src_stride ? b * src_stride : (int)rL;
            u.L = L;
            u.wav0 = wav_stride ? b * wav_stride : (int)rW;
            rL += L;
            rW += (int64_t)hop * (L > 1 ? L - 1 : 0);
        }
        utt[b] = u;
    }
    if (tid == 0) { hdr[0] = flags ? 0 : (int)frames; hdr[1] = flags; hdr[2] = flags ? 0 : (int)samples; hdr[3] = 0; }
}

__device__ inline bool exc_voiced(float f0, double lo, double hi) {
    const double f = (double)f0;
    return f - f == 0.0 && f >= lo && f <= hi;           // f - f == 0: finite
}

// a and d of segment t of an utterance whose f0 starts at f; false: unvoiced
__device__ inline bool exc_segment(const float* f, int t, const ExcOptions& o, double& a, double& d) {
    const float fa = f[t], fb = f[t + 1];
    const bool v = exc_voiced(fa, o.f0_floor, o.f0_ceil) && exc_voiced(fb, o.f0_floor, o.f0_ceil);
    a = v ? (double)fa : 0.0;
    d = v ? (double)fb - (double)fa : 0.0;
    return v;
}

// the utterance of workspace row r < hdr[0]: the first b with ws_row0[b] + L[b] > r (the ends never decrease: there is one)
__device__ inline int exc_find(const ExcUtt* utt, int B, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (utt[mid].ws_row0 + utt[mid].L > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Theta of every frame, one workgroup per utterance
__global__ __launch_bounds__(kExcThreads) void exc_prefix(const ExcUtt* utt, const int* hdr, const float* f0, ExcOptions o, double* theta) {
#pragma clang fp contract(off)      // one rounding per operation: tests/excitation_oracle.py computes the same Theta
    __shared__ double sS[kExcThreads];
    if (hdr[1] != 0) return;
    const ExcUtt u = utt[blockIdx.x];
    const int L = u.L, tid = threadIdx.x;
    if (L <= 0) return;
    const float* f = f0 + u.src_row0;
    double* th = theta + u.ws_row0;
    double carry = 0.0;
    if (tid == 0) th[0] = 0.0;
    for (int t0 = 0; t0 < L - 1; t0 += kExcThreads) {
        const int t = t0 + tid;
        if (t < L - 1) {
            double a, d;
            exc_segment(f, t, o, a, d);
            sS[tid] = ((double)o.hop * a + d * (double)(o.hop - 1) * 0.5) / o.sr;
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(kExcThreads, L - 1 - t0);
            for (int k = 0; k < n; ++k) {
                const double x = carry + sS[k];
                carry = x - floor(x);
                th[t0 + k + 1] = carry;
            }
        }
        __syncthreads();
    }
}

// sample i of a segment (utterance-local sample n)
__device__ inline float exc_sample(bool voiced, double a, double d, double Th, int i, int n, const ExcOptions& o) {
#pragma clang fp contract(off)
    if (!voiced) {
        const uint32_t h = gl_mix32((uint32_t)n ^ gl_mix32(o.seed + 0x9E3779B9u));
        const float u = (float)(h >> 8) * (1.0f / 16777216.0f);                      // exact
        return (u - 0.5f) * 3.46410162f;
    }
    const double x = Th + ((double)(i + 1) * a + (d * (double)(i * (i + 1))) / (double)(2 * o.hop)) / o.sr;
    const double th = x - floor(x);
    const double f = a + (d * (double)i) / (double)o.hop, half = o.sr / 2.0;
    double Hn = floor(half / f);
    for (int k = 0; k < 2; ++k) {                       // whatever the division rounded to: the largest Hn with Hn f < sr / 2
        if (Hn * f >= half) Hn -= 1.0;
        if ((Hn + 1.0) * f < half) Hn += 1.0;
    }
    if (Hn < 1.0) Hn = 1.0;
    // sum_{h = 1..Hn} cos(h x) = sin((Hn + 1/2) x) / (2 sin(x / 2)) - 1/2, x = 2 pi c with c = theta in [-1/2, 1/2): the numerator's
    // argument (Hn + 1/2) c is reduced to [-1/4, 1/4] turns in double, so both sines see at most a quarter turn in float32
    const double c = th >= 0.5 ? th - 1.0 : th;
    double q = (Hn + 0.5) * c;
    q -= floor(q + 0.5);
    if (q > 0.25) q = 0.5 - q;
    else if (q < -0.25) q = -0.5 - q;
    const float cf = (float)c;
    const float den = sinf(3.14159274f * cf), num = sinf(6.28318548f * (float)q);
    const float sum = fabsf(cf) < 1e-30f ? (float)Hn : num / (2.0f * den) - 0.5f;
    return sqrtf(2.0f / (float)Hn) * sum;
}

// One workgroup per workspace row r: the samples of its segment.  The last frame of an utterance has none.
__global__ __launch_bounds__(kExcThreads) void exc_samples(const ExcUtt* utt, const int* hdr, int B, const float* f0, ExcOptions o, const double* theta,
                                                          float* out) {
    const int r = blockIdx.x;
    if (hdr[1] != 0 || r >= hdr[0]) return;
    const ExcUtt u = utt[exc_find(utt, B, r)];
    const int t = r - u.ws_row0;
    if (t >= u.L - 1) return;
    double a, d;
    const bool v = exc_segment(f0 + u.src_row0, t, o, a, d);
    const double Th = theta[r];
    float* dst = out + u.wav0 + (int64_t)t * o.hop;
    for (int i = threadIdx.x; i < o.hop; i += kExcThreads) dst[i] = exc_sample(v, a, d, Th, i, t * o.hop + i, o);
}

__device__ inline float exc_angle(float2 X) { return (X.x == 0.f && X.y == 0.f) ? 0.f : atan2f(X.y, X.x); }

// One workgroup per kExcTile workspace rows, wave w the frames w, w + 4, ..: phase = angle of the STFT of the excitation in exc.
template <int NFFT>
__global__ __launch_bounds__(kExcThreads) void exc_phase(const ExcUtt* utt, const int* hdr, int B, int hop, const float2* gtw, const float* gwin,
                                                        const float* exc, float* phase) {
    constexpr int N2 = NFFT / 2, V = N2 / 64, NB = N2 + 1;
    __shared__ float2 tw[NFFT];
    __shared__ float win[NFFT];
    __shared__ float2 scratch[4][N2];
    __shared__ int s_row[kExcTile], s_wav[kExcTile], s_T[kExcTile], s_t[kExcTile];
    const int total = hdr[0], r0 = blockIdx.x * kExcTile;
    if (hdr[1] != 0 || r0 >= total) return;              // the same for every thread of the workgroup
    const int nf = min(kExcTile, total - r0);
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    if (tid < nf) {
        const int r = r0 + tid;
        const ExcUtt u = utt[exc_find(utt, B, r)];
        s_t[tid] = r - u.ws_row0;
        s_row[tid] = u.src_row0 + (r - u.ws_row0);
        s_wav[tid] = u.wav0;
        s_T[tid] = hop * max(u.L - 1, 0);
    }
    for (int i = tid; i < NFFT; i += kExcThreads) { tw[i] = gtw[i]; win[i] = gwin[i]; }
    __syncthreads();
    for (int k = 0; k < nf; k += 4) {
        const bool valid = k + wv < nf;
        const int fi = valid ? k + wv : 0;
        const int T = s_T[fi], t = s_t[fi];
        const bool ok = valid && T > NFFT / 2;           // shorter: no reflect padding possible, the row is 0
        const float* x = exc + s_wav[fi];
        float2 v[V];
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const int n = 2 * (j + 64 * r);
            float xx[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int s = hop * t - NFFT / 2 + n + u;
                s = s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s);
                xx[u] = ok ? x[s] * win[n + u] : 0.f;
            }
            v[r] = make_float2(xx[0], xx[1]);
        }
        float2 X[V], xl;
        gl_frame_rfft<NFFT>(v, X, xl, scratch[wv], tw, j);
        if (valid) {
            float* row = phase + (int64_t)s_row[fi] * NB;
#pragma unroll
            for (int r = 0; r < V; ++r) row[j + 64 * r] = exc_angle(X[r]);
            if (j == 0) row[N2] = exc_angle(xl);
        }
        __syncthreads();
    }
}

// ---- workspace layout and launch sequences (host), shared by the entry points and the host stand-in of the tests ----
struct ExcLayout {
    size_t off_hdr = 0, off_utt = 0, off_theta = 0, off_tw = 0, off_win = 0, off_exc = 0, bytes = 0;
};

// frames: the workspace rows (sum of L, or the capacity); the excitation buffer holds hop samples per row
inline ExcLayout exc_layout(int n_fft, int hop, int64_t B, int64_t frames) {
    ExcLayout l;
    size_t off = 0;
    auto take = [&](size_t n) { off = (off + 255) / 256 * 256; size_t o = off; off += n; return o; };
    l.off_hdr = take(kExcHdrInts * sizeof(int));
    l.off_utt = take((size_t)(B > 1 ? B : 1) * sizeof(ExcUtt));
    l.off_theta = take((size_t)frames * sizeof(double));
    l.off_tw = take((size_t)n_fft * sizeof(float2));
    l.off_win = take((size_t)n_fft * sizeof(float));
    l.off_exc = take((size_t)frames * hop * sizeof(float));
    l.bytes = (off + 255) / 256 * 256;
    return l;
}

// exc_prefix over B utterances and exc_samples over `rows` workspace rows into wav (NULL: the workspace's buffer), then with `phase`
// the tables and exc_phase; the records and the header being in place (or being written ahead on the stream)
inline hipError_t exc_launch(hipStream_t s, int n_fft, int win, const ExcOptions& o, const float* f0, int B, int64_t rows, char* ws, const ExcLayout& at,
                             float* wav, float* phase) {
    const ExcUtt* utt = (const ExcUtt*)(ws + at.off_utt);
    const int* hdr = (const int*)(ws + at.off_hdr);
    double* theta = (double*)(ws + at.off_theta);
    float* exc = wav ? wav : (float*)(ws + at.off_exc);
    const dim3 blk(kExcThreads);
    hipLaunchKernelGGL(exc_prefix, dim3((unsigned)B), blk, 0, s, utt, hdr, f0, o, theta);
    hipLaunchKernelGGL(exc_samples, dim3((unsigned)rows), blk, 0, s, utt, hdr, B, f0, o, (const double*)theta, exc);
    if (phase) {
        float2* tw = (float2*)(ws + at.off_tw);
        float* wn = (float*)(ws + at.off_win);
        hipLaunchKernelGGL(gl_tables, dim3((n_fft + 255) / 256), dim3(256), 0, s, tw, wn, n_fft, win);
        const dim3 g((unsigned)((rows + kExcTile - 1) / kExcTile));
        if (n_fft == 512) hipLaunchKernelGGL((exc_phase<512>), g, blk, 0, s, utt, hdr, B, o.hop, (const float2*)tw, (const float*)wn, (const float*)exc, phase);
        else if (n_fft == 1024) hipLaunchKernelGGL((exc_phase<1024>), g, blk, 0, s, utt, hdr, B, o.hop, (const float2*)tw, (const float*)wn, (const float*)exc, phase);
        else hipLaunchKernelGGL((exc_phase<2048>), g, blk, 0, s, utt, hdr, B, o.hop, (const float2*)tw, (const float*)wn, (const float*)exc, phase);
    }
    return hipGetLastError();
}

// Host-planned: starts / lens validated by the caller (>= 0, sum `frames` > 0, hop frames < 2^31); the waveforms packed back to back
inline hipError_t exc_run_host(hipStream_t s, int n_fft, int win, const ExcOptions& o, const float* f0, int B, const int32_t* starts, const int32_t* lens,
                               int64_t frames, char* ws, const ExcLayout& at, float* wav, float* phase) {
    int64_t samples = 0;
    for (int b = 0; b < B; ++b) samples += (int64_t)o.hop * (lens[b] > 1 ? lens[b] - 1 : 0);
    int row = 0, w0 = 0;
    for (int i = 0; i < B; i += kExcUttsPerChunk) {
        ExcUttChunk c{};
        c.n = B - i < kExcUttsPerChunk ? B - i : kExcUttsPerChunk;
        c.base = i;
        c.frames = (int)frames;
        c.samples = (int)samples;
        for (int j = 0; j < c.n; ++j) {
            const int L = lens[i + j];
            c.u[j].src_row0 = starts[i + j];
            c.u[j].ws_row0 = row;
            c.u[j].L = L;
            c.u[j].wav0 = w0;
            row += L;
            w0 += o.hop * (L > 1 ? L - 1 : 0);
        }
        hipLaunchKernelGGL(exc_upload, dim3(1), dim3(kExcThreads), 0, s, c, (ExcUtt*)(ws + at.off_utt), (int*)(ws + at.off_hdr));
    }
    return exc_launch(s, n_fft, win, o, f0, B, frames, ws, at, wav, phase);
}

// Device-driven: the grids are sized from the capacities, surplus workgroups leave at once.  wav NULL (the phase alone): the
// excitation goes to the workspace's buffer, packed, which holds hop frame_capacity samples.
inline hipError_t exc_run_dev(hipStream_t s, int n_fft, int win, const ExcOptions& o, const float* f0, int B, const int64_t* lens_dev, int src_stride,
                              int64_t frame_capacity, const int32_t* upstream, char* ws, const ExcLayout& at, float* wav, int wav_stride,
                              int64_t wav_capacity, float* phase) {
    hipLaunchKernelGGL(exc_plan, dim3(1), dim3(kExcThreads), 0, s, lens_dev, upstream, B, src_stride, frame_capacity, o.hop, wav ? wav_stride : 0,
                       wav ? wav_capacity : (int64_t)o.hop * frame_capacity, (ExcUtt*)(ws + at.off_utt), (int*)(ws + at.off_hdr));
    return exc_launch(s, n_fft, win, o, f0, B, frame_capacity, ws, at, wav, phase);
}

}  // namespace fs2
