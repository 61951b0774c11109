// spsi_upload / spsi_plan / spsi_analyse / spsi_chain of csrc/gl_spsi.h on the host stand-in, through the launch sequences the library uses
// (spsi_run_host, spsi_run_dev).
// Usage: spsi_main IN OUT
//   IN:  int32 n_fft, hop, src_width, B, rows, dev, src_stride, frame_capacity; int32 starts[B], lens[B]; float32 src[rows, src_width];
//        float32 pinv[n_fft / 2 + 1, src_width] when src_width != n_fft / 2 + 1.  dev = 1: the device-driven sequence (lens as int64, starts
//        ignored: src_stride 0 = packed, else rows per utterance; frame_capacity rows of workspace).
//   OUT: float32 phase[rows, bins] (-777 where nothing was written), float32 mag_out[rows, bins] (likewise), int32 hdr[4] of the workspace.
// Every buffer is a heap block of exactly its size, so that a sanitizer build sees an access beyond it.
#include "hip_standin.h"

// the wave ballot, which hip_standin.h does not have: bit l = lane l's predicate, through the per-wave exchange buffer
inline unsigned long long __ballot(int pred) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_shfl[w][l][0] = pred ? 1 : 0;
    g_wave_bar[w]->arrive_and_wait();
    unsigned long long m = 0;
    for (int i = 0; i < 64; ++i) m |= (unsigned long long)g_shfl[w][i][0] << i;
    g_wave_bar[w]->arrive_and_wait();
    return m;
}

#include "gl_spsi.h"
using namespace fs2;

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n) {
    v.assign(n, T{});
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[8];
    if (!f || fread(h, 4, 8, f) != 8) return 2;
    const int n_fft = h[0], hop = h[1], width = h[2], B = h[3], rows = h[4], dev = h[5], stride = h[6], cap = h[7], NB = n_fft / 2 + 1;
    std::vector<int32_t> starts, lens;
    std::vector<float> src, pinv;
    if (!read_into(f, starts, B) || !read_into(f, lens, B) || !read_into(f, src, (size_t)rows * width)) return 2;
    if (width != NB && !read_into(f, pinv, (size_t)NB * width)) return 2;
    fclose(f);
    std::vector<float> phase((size_t)rows * NB, -777.f), mag((size_t)rows * NB, -777.f);
    int64_t frames = 0;
    for (int b = 0; b < B; ++b) frames += lens[b] > 0 ? lens[b] : 0;
    const SpsiLayout at = spsi_layout(NB, B, dev ? cap : frames);
    std::vector<char> ws(at.bytes, (char)0x5a);
    const float* pv = pinv.empty() ? nullptr : pinv.data();
    if (dev) {
        std::vector<int64_t> l64(lens.begin(), lens.end());
        spsi_run_dev(nullptr, n_fft, hop, src.data(), width, pv, B, l64.data(), stride, cap, (const int32_t*)nullptr, ws.data(), at, phase.data(), mag.data());
    } else {
        if (frames == 0) return 3;
        spsi_run_host(nullptr, n_fft, hop, src.data(), width, pv, B, starts.data(), lens.data(), frames, ws.data(), at, phase.data(), mag.data());
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(phase.data(), 4, phase.size(), o);
    fwrite(mag.data(), 4, mag.size(), o);
    fwrite(ws.data() + at.off_hdr, 4, 4, o);
    fclose(o);
    return 0;
}
