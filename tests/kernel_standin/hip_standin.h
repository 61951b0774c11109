// Host stand-in for the HIP constructs fastspeech2_amd/csrc/targets.h uses, so that its kernels' code can run without a GPU
// (tests/test_targets_kernel_host.py): one workgroup at a time, one std::thread per lane, __shared__ as function statics,
// barriers as std::barrier, shuffles through a per-wave exchange buffer, LDS atomics as host atomics.  It checks the kernels'
// logic (the select, the sweeps, the reductions, what is read after which barrier -- build it with -fsanitize=thread for that);
// it says nothing about what hipcc makes of the arithmetic.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __shared__ static
#define __launch_bounds__(x)
struct dim3 { unsigned x = 1, y = 1, z = 1; dim3(unsigned a = 1) : x(a) {} };
inline thread_local dim3 threadIdx, blockIdx, blockDim;
struct int2 { int x, y; };
inline int2 make_int2(int x, int y) { return int2{x, y}; }
constexpr int kStandinWaves = 16;      // a workgroup of up to 1024 threads
typedef void* hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline const char* hipGetErrorString(hipError_t) { return "?"; }
inline std::barrier<>* g_block_bar;
inline std::barrier<>* g_wave_bar[kStandinWaves];
inline std::atomic<int> g_or{0};
alignas(16) inline unsigned char g_shfl[kStandinWaves][64][16];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
inline int __syncthreads_or(int v) {
    if (v) g_or.store(1);
    __syncthreads();
    int r = g_or.load();
    __syncthreads();
    if (threadIdx.x == 0) g_or.store(0);
    __syncthreads();
    return r;
}
template <typename T> T shfl_from(T v, int src) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    std::memcpy(g_shfl[w][l], &v, sizeof(T));
    g_wave_bar[w]->arrive_and_wait();
    T r;
    std::memcpy(&r, g_shfl[w][(src >= 0 && src < 64) ? src : l], sizeof(T));
    g_wave_bar[w]->arrive_and_wait();
    return r;
}
template <typename T> T __shfl_xor(T v, int o) { return shfl_from(v, (int)(threadIdx.x & 63) ^ o); }
template <typename T> T __shfl_up(T v, int o) { return shfl_from(v, (int)(threadIdx.x & 63) - o); }
template <typename T> T __shfl_down(T v, int o) { return shfl_from(v, (int)(threadIdx.x & 63) + o); }
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline uint32_t atomicMin(uint32_t* p, uint32_t v) {
    uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
inline int atomicMin(int* p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
inline int atomicMax(int* p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
using std::min; using std::max; using std::isfinite;
template <typename K, typename... A> void launch(K k, dim3 grid, dim3 blk, A... a) {
    for (unsigned b = 0; b < grid.x; ++b) {
        std::barrier<> bb(blk.x);
        std::deque<std::barrier<>> wb;
        g_block_bar = &bb;
        for (int w = 0; w < kStandinWaves; ++w) g_wave_bar[w] = &wb.emplace_back(64);
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < blk.x; ++t)
            ts.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); blockDim = blk; k(a...); });
        for (auto& t : ts) t.join();
    }
}
#define hipLaunchKernelGGL(k, grid, blk, lds, s, ...) launch(k, grid, blk, __VA_ARGS__)
