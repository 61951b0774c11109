// Tile rule of the fused Griffin-Lim kernel (griffin_lim.h: gl_iterate), shared by the kernels and the
// host plan.  Plain C++ with no HIP dependency, so tests/test_vocoder_geometry_host.py compiles it on the host and compares it with
// fastspeech2_amd/vocoder.py: tile_rule, whose exhaustive check then covers this code.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define GL_HD __host__ __device__
#else
#define GL_HD
#endif

namespace fs2 {

constexpr int kGlTile = 32;                  // frames per tile at the default geometry, and the most any geometry takes
constexpr int kGlMaxLds = 163840;            // LDS one workgroup may declare on gfx950 (160 KiB)

// halo frames each side: a sample lies in ceil(N / H) frames; at H = N the final ISTFT's samples reach one frame past the tile
GL_HD constexpr int gl_halo(int n, int hop) { return (n + hop - 1) / hop - 1 > 1 ? (n + hop - 1) / hop - 1 : 1; }
// a tile whose frames include the last one also reads the reflection of pre-trim position T - 1, which frame L - gl_tail covers
GL_HD constexpr int gl_tail(int n, int hop) { return n / hop + 1; }                 // ceil((N + 1) / H)
GL_HD constexpr int gl_lmin(int n, int hop) { return n / (2 * hop) + 2; }           // fewest frames with T > N / 2
GL_HD constexpr int gl_sig_max(int n, int hop, int F) { return hop * (F + 2 * gl_halo(n, hop) - 1) + n; }
constexpr int gl_static_lds(int n) { return 28 * n; }    // tw (8 N) + window (4 N) + four waves' FFT buffers (16 N) bytes

// Tile frames per geometry: the largest F <= 32 (halving) whose LDS fits one workgroup.
inline int gl_tile_frames(int n, int hop) {
    int F = kGlTile;
    while (F > 1 && gl_static_lds(n) + 4 * gl_sig_max(n, hop, F) > kGlMaxLds) F /= 2;
    return F;
}

}  // namespace fs2
