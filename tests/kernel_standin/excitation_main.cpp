// exc_upload / exc_plan / exc_prefix / exc_samples / exc_phase of csrc/gl_excite.h on the host stand-in, through the launch sequences the
// library uses (exc_run_host, exc_run_dev).
// Usage: excitation_main IN OUT
//   IN:  int32 n_fft, hop, win, B, rows, dev, src_stride, frame_capacity, sample_rate, seed, want (1 wav, 2 phase), wav_stride,
//        wav_capacity, 0, 0, 0; float64 f0_floor, f0_ceil; int32 starts[B], lens[B]; float32 f0[rows].  dev = 1: the device-driven
//        sequence (lens as int64, starts ignored: src_stride 0 = packed, else rows per utterance; frame_capacity rows of workspace).
//   OUT: float32 phase[rows, bins] (want 2) or float32 wav[samples] (want 1; samples = wav_capacity with dev, else sum hop max(L - 1, 0)),
//        -777 where nothing was written; then int32 hdr[4] of the workspace.
// Every buffer is a heap block of exactly its size, so that a sanitizer build sees an access beyond it.
//
// gl_excite.h expects its includer to provide float2, gl_mix32, gl_tables and gl_frame_rfft: the library takes them from griffin_lim.h,
// which needs the HIP headers.  The shim below restates the hash and the tables, and transforms a frame by the definition of the DFT in
// double: what runs here is every index, record, prefix, sample and phase statement of gl_excite.h; the float32 FFT itself only the GPU
// tests see.
#include "hip_standin.h"

struct float2 { float x, y; };
inline float2 make_float2(float x, float y) { return float2{x, y}; }

namespace fs2 {

inline uint32_t gl_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

void gl_tables(float2* tw, float* win, int n, int wl) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const double pi = 3.14159265358979323846;
    tw[m] = make_float2((float)std::cos(2.0 * pi * m / n), (float)-std::sin(2.0 * pi * m / n));
    const int lp = (n - wl) / 2;
    win[m] = (m >= lp && m < lp + wl) ? (float)(0.5 - 0.5 * std::cos(2.0 * pi * (m - lp) / wl)) : 0.f;
}

template <int NFFT> const std::vector<double>& dft_table() {
    static const std::vector<double> t = [] {
        std::vector<double> v(2 * NFFT);
        for (int m = 0; m < NFFT; ++m) { v[2 * m] = std::cos(2.0 * 3.14159265358979323846 * m / NFFT); v[2 * m + 1] = -std::sin(2.0 * 3.14159265358979323846 * m / NFFT); }
        return v;
    }();
    return t;
}

// the interface of griffin_lim.h: v[r] = z[j + 64 r] (packed real pairs) -> lane j gets X[j + 64 r]; xl = X[N/2]
template <int NFFT> void gl_frame_rfft(float2* v, float2* X, float2& xl, float2* buf, const float2*, int j) {
    constexpr int N2 = NFFT / 2, V = N2 / 64;
    const std::vector<double>& tb = dft_table<NFFT>();
    __syncthreads();
    for (int r = 0; r < V; ++r) buf[j + 64 * r] = v[r];
    __syncthreads();
    const float* x = reinterpret_cast<const float*>(buf);
    for (int r = 0; r < V; ++r) {
        const int k = j + 64 * r;
        double re = 0.0, im = 0.0;
        for (int n = 0; n < NFFT; ++n) {
            const int m = (int)(((int64_t)n * k) % NFFT);
            re += x[n] * tb[2 * m]; im += x[n] * tb[2 * m + 1];
        }
        X[r] = make_float2((float)re, (float)im);
    }
    double s = 0.0;
    for (int n = 0; n < NFFT; ++n) s += (n & 1) ? -(double)x[n] : (double)x[n];
    xl = make_float2((float)s, 0.f);
}

}  // namespace fs2

#include "gl_excite.h"
using namespace fs2;

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n) {
    v.assign(n, T{});
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[16];
    double lim[2];
    if (!f || fread(h, 4, 16, f) != 16 || fread(lim, 8, 2, f) != 2) return 2;
    const int n_fft = h[0], hop = h[1], win = h[2], B = h[3], rows = h[4], dev = h[5], stride = h[6], cap = h[7], sr = h[8], want = h[10], wav_stride = h[11],
              wav_cap = h[12], NB = n_fft / 2 + 1;
    const uint32_t seed = (uint32_t)h[9];
    std::vector<int32_t> starts, lens;
    std::vector<float> f0;
    if (!read_into(f, starts, B) || !read_into(f, lens, B) || !read_into(f, f0, rows)) return 2;
    fclose(f);
    int64_t frames = 0, samples = 0;
    for (int b = 0; b < B; ++b) { frames += lens[b] > 0 ? lens[b] : 0; samples += (int64_t)hop * (lens[b] > 1 ? lens[b] - 1 : 0); }
    std::vector<float> phase(want == 2 ? (size_t)rows * NB : 0, -777.f), wav(want == 1 ? (size_t)(dev ? wav_cap : samples) : 0, -777.f);
    const ExcLayout at = exc_layout(n_fft, hop, B, dev ? cap : frames);
    std::vector<char> ws(at.bytes, (char)0x5a);
    const ExcOptions o{lim[0], lim[1], (double)sr, seed, hop};
    float* pw = want == 1 ? wav.data() : nullptr;
    float* pp = want == 2 ? phase.data() : nullptr;
    if (dev) {
        std::vector<int64_t> l64(lens.begin(), lens.end());
        exc_run_dev(nullptr, n_fft, win, o, f0.data(), B, l64.data(), stride, cap, (const int32_t*)nullptr, ws.data(), at, pw, wav_stride, wav_cap, pp);
    } else {
        if (frames == 0) return 3;
        exc_run_host(nullptr, n_fft, win, o, f0.data(), B, starts.data(), lens.data(), frames, ws.data(), at, pw, pp);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (!phase.empty()) fwrite(phase.data(), 4, phase.size(), out);
    if (!wav.empty()) fwrite(wav.data(), 4, wav.size(), out);
    fwrite(ws.data() + at.off_hdr, 4, 4, out);
    fclose(out);
    return 0;
}
