// libfs2_hip.so -- runtime + C ABI (include/fs2.h) of the MI355X FastSpeech2 mel-generation path.
// Orchestrates the kernels over the gapped packed row layout: gemm_planes.h / attn_bf16.h (split-bf16 and bf16 modes, activations as
// planes), gemm_f32.h / attn_f32.h (exact fp32 mode), elementwise.h (HBM-bound steps), layout.h (the layout, host- and device-built).  Weight repacking at load
// time, workspace carving (no allocation inside a forward), host- or device-driven frame layout, per-launch hipEvent profiling.
// Replaces the tensor work of reference fastspeech.py:169-243 (`FeedForwardTransformer._forward`).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <list>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fs2.h"
#include "attn_bf16.h"
#include "attn_w32.h"
#include "attn_f32.h"
#include "attn_plan.h"
#include "common.h"
#include "elementwise.h"
#include "varshort.h"
#include "layout_rule.h"
#include "layout.h"
#include "gemm_bf16.h"
#include "gemm_plan.h"
#include "gemm_planes.h"
#include "gemm_row4.h"
#include "model_launches.h"
#include "call_plan.h"
#include "gemm_mx.h"
#include "weight_plan.h"
#include "gemm_f32.h"
#include "griffin_lim.h"
#include "gl_pitch.h"
#include "gl_spsi.h"
#include "gl_excite.h"

using namespace fs2;

namespace {

std::string g_create_error;

// struct Options -- the A/B switches of the kernel choice -- lives in gemm_plan.h; it is read from the environment ONCE, here, when the library is first used.
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// ---- the ISA-audit gate (round-5 advisor finding: the gate used to live in the ctypes binding only).  attn_w32 and gemm_row4_bf16 keep their
// accumulators in literal registers the compiler does not know to be live; fastspeech2_amd/_lib.py::build() audits the device
// assembly of the binary it ships and records the outcome in libfs2_hip.audit.json next to it, tied to the file's SHA-256.  The library looks for
// that record of ITSELF when it is first used: without a clean one the three switches below start at 0 for every consumer (ctypes, the TorchScript
// op, a C program linked against the ABI) and only an explicit fs2_set_option turns them on (probes).
struct Sha256 {
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    unsigned char buf[64]; size_t fill = 0; uint64_t total = 0;
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const unsigned char* p) {
        static const uint32_t K[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
            0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
            0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
            0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
            0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
            0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const unsigned char* p, size_t n) {
        total += n;
        while (n) {
            const size_t k = std::min(n, 64 - fill);
            memcpy(buf + fill, p, k); fill += k; p += k; n -= k;
            if (fill == 64) { block(buf); fill = 0; }
        }
    }
    std::string hex16() {      // first 16 hex digits of the digest (what _lib.py records as so_sha16)
        const uint64_t bits = total * 8;
        unsigned char pad[72] = {0x80};
        const size_t padn = (fill < 56 ? 56 - fill : 120 - fill);
        unsigned char len[8];
        for (int i = 0; i < 8; ++i) len[i] = (unsigned char)(bits >> (56 - 8 * i));
        update(pad, padn); update(len, 8);
        char out[17];
        snprintf(out, sizeof out, "%08x%08x", h[0], h[1]);
        return out;
    }
};
bool audit_clean_of_this_binary() {
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void*>(&fs2_abi_version), &info) || !info.dli_fname) return false;
    const std::string so = info.dli_fname;
    const size_t slash = so.rfind('/');
    const std::string rec_path = (slash == std::string::npos ? std::string() : so.substr(0, slash + 1)) + "libfs2_hip.audit.json";
    std::ifstream rf(rec_path);
    if (!rf) return false;
    const std::string rec((std::istreambuf_iterator<char>(rf)), std::istreambuf_iterator<char>());
    const size_t k = rec.find("\"so_sha16\"");
    if (k == std::string::npos) return false;
    const size_t q0 = rec.find('"', rec.find(':', k) + 1), q1 = q0 == std::string::npos ? q0 : rec.find('"', q0 + 1);
    if (q1 == std::string::npos) return false;
    const std::string want = rec.substr(q0 + 1, q1 - q0 - 1);
    const size_t c = rec.find("\"clean\"");
    const size_t v = c == std::string::npos ? c : rec.find_first_not_of(" :", c + 7);
    if (v == std::string::npos || rec.compare(v, 4, "true") != 0) return false;
    std::ifstream sf(so, std::ios::binary);
    if (!sf) return false;
    Sha256 sh;
    std::vector<unsigned char> blk(1 << 20);
    while (sf) {
        sf.read(reinterpret_cast<char*>(blk.data()), (std::streamsize)blk.size());
        if (sf.gcount() > 0) sh.update(blk.data(), (size_t)sf.gcount());
    }
    return sh.hex16() == want;
}
bool audit_clean() {
    static const bool ok = audit_clean_of_this_binary();
    return ok;
}

Options& opts() {
    static Options o = [] {
        Options x;
        x.bm = env_int("FS2_BM", -1); x.row8 = env_int("FS2_ROW8", -1); x.qkv8 = env_int("FS2_QKV8", -1);
        x.nosplitk = env_int("FS2_NOSPLITK", 0) != 0; x.f32_rows = env_int("FS2_F32_ROWS", 0) != 0; x.mt8 = env_int("FS2_MT8", -1); x.qkv_split = env_int("FS2_QKV_SPLIT", -1); x.op_att_planes = env_int("FS2_OP_ATT_PLANES", 0); x.fuse_var = env_int("FS2_FUSE_VAR", 1); x.bal = env_int("FS2_BAL", 0); x.w32 = env_int("FS2_ATTN_W32", -1);
        x.row4 = env_int("FS2_ROW4", -1); x.mt4 = env_int("FS2_MT4", -1); x.ffn2_mx = env_int("FS2_FFN2_MX", 1); x.qkv4 = env_int("FS2_QKV4", -1); x.post_mx = env_int("FS2_POST_MX", 1);
        x.tokproj = env_int("FS2_TOKPROJ", 3) & 3; x.tokproj_f32 = env_int("FS2_TOKPROJ_F32", 0) != 0;
        x.varshort = env_int("FS2_VARSHORT", 1) != 0;
        if (!audit_clean()) {
            x.w32 = 0; x.row4 = 0; x.qkv4 = 0;
            fprintf(stderr, "libfs2_hip: no clean ISA-audit record of this binary (libfs2_hip.audit.json next to it): attn_w32 and gemm_row4_bf16 are switched "
                            "off, attn_bf16 / gemm_row8_bf16 run instead; rebuild with `python -c 'import __graft_entry__ as g; g.build()'`\n");
        }
        return x;
    }();
    return o;
}

// max over the rows n of a [N][K] weight of (sum_k |w[n][k]|) xmax + |b[n]|: the a-priori bound of relu(w x + b) for |x| <= xmax (weight-load time only)
__global__ void row_l1_bound_kernel(const float* w, const float* b, int N, int K, float xmax, unsigned* out) {
    const int n = blockIdx.x;
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += blockDim.x) s += fabsf(w[(size_t)n * K + k]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint((part[0] + part[1] + part[2] + part[3]) * xmax + (b ? fabsf(b[n]) : 0.f)));
}
float device_row_l1_bound(hipStream_t s, const float* w, const float* b, int N, int K, float xmax, unsigned* scratch) {
    hipMemsetAsync(scratch, 0, 4, s);
    hipLaunchKernelGGL(row_l1_bound_kernel, dim3(N), dim3(256), 0, s, w, b, N, K, xmax, scratch);
    unsigned u = 0;
    hipMemcpyAsync(&u, scratch, 4, hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// max |x| of a device array (weight-load time only: one small launch + a blocking 4-byte read-back)
__global__ void absmax_kernel(const float* x, int64_t n, unsigned* out) {
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));      // non-negative floats order like their bit patterns
}
float device_absmax(hipStream_t s, const float* x, int64_t n, unsigned* scratch) {
    hipMemsetAsync(scratch, 0, 4, s);
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, s, x, n, scratch);
    unsigned bits = 0;
    hipMemcpyAsync(&bits, scratch, 4, hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    float f; memcpy(&f, &bits, 4);
    return f;
}
inline int fp8_scale_exponent(float bound) { return bound > 0.f ? (int)std::floor(std::log2(448.0 / (double)bound)) : 0; }

// Every entry point that takes a handle runs on the handle's device and leaves the caller's current device as it found it.
struct DeviceGuard {
    int prev = -1; bool switched = false; hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = (err == hipSuccess); }
    }
    ~DeviceGuard() { if (switched) hipSetDevice(prev); }
};

struct ProfRec { std::string name; hipEvent_t e0, e1; double flops, bytes; };

}  // namespace

struct fs2_handle {
    fs2_config cfg;
    std::string err;
    bool loaded = false;
    std::vector<void*> allocs;
    // weights
    float* enc_embed = nullptr;
    Stack enc, dec;
    Predictor dur, energy, pitch;
    FusedPredictors var2;
    float *ebins = nullptr, *pbins = nullptr, *Te = nullptr, *Tp = nullptr;
    Gemm dec_in; float *dec_in_lng = nullptr, *dec_in_lnb = nullptr;
    // multiply before expanding (FS2_TOKPROJ): the stacked k = 1 weight [tap0: energy | pitch][tap1: ..][tap2: ..][dec.in] of tok.proj (N == 0: this model has none)
    // and the embedding tables behind the input layer's weights, TPd = (pitch_embed.W^T + b_p) W_in^T + b_in, TEd = (energy_embed.W^T + b_e) W_in^T: [n_bins, ddim]
    Gemm tokw; float *TEd = nullptr, *TPd = nullptr;
    Gemm feat;
    std::vector<Gemm> post;
    Encoded left;              // state carried from encode to decode (call_plan.h)
    HostLayout tok;            // fs2_encode's host layout (kept for its storage)
    float* kp = nullptr; size_t kp_cap = 0;   // split-K scratch of the call in progress (carved from its workspace)
    int cur_regime = 0;        // regime_rows of the call in progress (0: the launch's own row count)
    int* counters = nullptr;   // device int[16], zeroed at creation: [0] = waves of attn_w32 that left the fast path (fs2_get_counter)
    int* cur_status = nullptr; // device-driven layout: the status words of the call in progress ([5] counts the same event for that call alone)
    int gap = kGap;            // zero rows between packed utterances: max(kMinGap, largest conv halo of this model)
    std::vector<void*> graph_pinned;   // host staging owned by captured graphs (see upload_layout)
    // profiling
    bool prof = false;
    std::string prof_filter;      // when non-empty only launches with exactly this name are bracketed
    std::vector<ProfRec> recs;
};

namespace {

int fail(fs2_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(h, expr)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(h, FS2_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int round_up(int x, int a) { return (x + a - 1) / a * a; }

struct Bump {   // carve a caller-provided workspace
    char* base; size_t off = 0, cap;
    Bump(void* p, size_t c) : base((char*)p), cap(c) {}
    template <typename T> T* take(size_t n) {
        off = align_up(off, 256);
        T* p = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return p;
    }
    bool ok() const { return off <= cap; }
};

// ------------------------------------------------------------------ profiling wrappers
struct Scope {
    fs2_handle* h; hipStream_t s; size_t idx = (size_t)-1;
    Scope(fs2_handle* h_, hipStream_t s_, const char* name, double flops, double bytes) : h(h_), s(s_) {
        if (h && h->prof && (h->prof_filter.empty() || h->prof_filter == name)) {
            ProfRec r; r.name = name; r.flops = flops; r.bytes = bytes;
            hipEventCreate(&r.e0); hipEventCreate(&r.e1);
            hipEventRecord(r.e0, s);
            h->recs.push_back(r); idx = h->recs.size() - 1;
        }
    }
    ~Scope() { if (idx != (size_t)-1) hipEventRecord(h->recs[idx].e1, s); }
};

// Kernels that need more than 64 KB of dynamic LDS must raise their limit once per (kernel, device); the flags live at the
// call site (one array per kernel instantiation), indexed by the current device.
struct LdsAttr { bool done[32] = {}; };
inline void allow_lds(const void* kernel, size_t bytes, LdsAttr& st) {
    int dev = 0;
    hipGetDevice(&dev);
    bool& d = st.done[dev & 31];
    if (!d) { hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); d = true; }
}

// ------------------------------------------------------------------ kernel launchers
static_assert(kPlanErrArg == FS2_ERR_ARG && kPlanErrHip == FS2_ERR_HIP && kPlanErrState == FS2_ERR_STATE && kPlanErrUnsupported == FS2_ERR_UNSUPPORTED &&
              kPlanFp32 == FS2_PREC_FP32 && kPlanBf16x3 == FS2_PREC_BF16X3 && kPlanMaxHalo == kMaxHalo && kPlanBN == kB16BN && kPrecMixF16x2 == FS2_PREC_MIX_F16X2 &&
              kPrecMixF16x1 == FS2_PREC_MIX_F16X1 && kPrecMixMx == FS2_PREC_MIX_MX && kPrecMixMx4 == FS2_PREC_MIX_MX4, "gemm_plan.h and model_launches.h restate these");

// One launcher for every GEMM and attention kernel, keyed by the kernel: it owns the per-(kernel, device) flag of the LDS attribute.
// lds_max: the most any launch of K asks for, where that is not the same for every launch (0: lds).
template <auto K, class A>
hipError_t launch_kernel(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& a, size_t lds_max = 0) {
    static LdsAttr attr;
    allow_lds(reinterpret_cast<const void*>(K), lds_max ? lds_max : lds, attr);
    hipLaunchKernelGGL(K, grid, block, lds, s, a);
    return hipGetLastError();
}
template <int V> using Int = std::integral_constant<int, V>;
// pick<V...>(v, f): f(std::integral_constant<int, V>) for the V that equals v -- a run-time template coordinate of the plan to the instantiation built for it
template <int V, int... Vs, typename F>
hipError_t pick(int v, F&& f) {
    if (v == V) return f(Int<V>{});
    if constexpr (sizeof...(Vs) > 0) return pick<Vs...>(v, f);
    else return hipErrorInvalidValue;
}
// CV(X): the int that pick handed a generic lambda as its integral_constant parameter X, as a constant expression (a template argument).  A macro only
// because `X.value` / `decltype(X)::value` of a lambda parameter is not usable as one by every compiler this builds with; it lives for run_plan and run_attn_plan alone.
#define CV(x) decltype(x)::value
constexpr int row4_variant(int epi, int arith, int res) { return epi * 100 + arith * 10 + res; }      // gemm_row4_bf16's (EPI, ARITH, RES) as one case label

template <int NSPLIT, int BM, bool K1, int ARITH>
hipError_t launch_pl(hipStream_t s, const GemmArgs& a, size_t extra_lds = 0) {
    dim3 grid((a.N + kB16BN - 1) / kB16BN, ((a.qk_hi ? a.Rvt : a.R) + BM - 1) / BM, a.ksplit > 1 ? a.ksplit : 1);
    return launch_kernel<gemm_pl_bf16<NSPLIT, BM, K1, ARITH>>(grid, dim3(256), pl_lds_bytes<BM, K1>() + extra_lds, s, a);
}
// (the DMA-spreading schedule of gemm_row4_bf16 is fixed at SCHED = 2: same-box A/B in the model, c3: 0 -> 7.21, 2 -> 7.20, 4 -> 7.17 M frames/s; stand-alone 2 and 4 are 5-13 % ahead of 0)
template <int MT, int EPI, int ARITH, int RES>
hipError_t launch_row4(hipStream_t s, const GemmArgs& a) {
    return launch_kernel<gemm_row4_bf16<3, 3, MT, EPI, 2, ARITH, RES>>(dim3((a.R + 32 * MT - 1) / (32 * MT)), dim3(256), row4_lds_bytes<3, MT>(), s, a);
}

// The instantiation a plan names, launched on the arguments derived from it (launch_gemm).  The kernels are instantiated, and so laid out in the code
// object, in the order of the cases and of pick's values (profiles/gemm_plan_kernels.txt holds the list).
hipError_t run_plan(hipStream_t s, const GemmPlan& p, const GemmArgs& t) {
    switch (p.kernel) {
    case GemmKernel::Row4: {
        auto row4 = [&](auto EPI, auto ARITH, auto RES) { return pick<5, 4>(p.mt, [&](auto MT) { return launch_row4<CV(MT), CV(EPI), CV(ARITH), CV(RES)>(s, t); }); };
        // the six (EPI, ARITH, RES) variants the library holds (gemm_row4.h; plan_gemm produces no other): a new one is a line here
        switch (row4_variant(p.epi, p.arith, p.res)) {
        case row4_variant(2, 0, 3): return row4(Int<2>{}, Int<0>{}, Int<3>{});      // input layer: positional encoding, no residual
        case row4_variant(1, 0, 1): return row4(Int<1>{}, Int<0>{}, Int<1>{});      // out-proj + LN1 of mix_mx: mx planes out
        case row4_variant(4, 0, 1): return row4(Int<4>{}, Int<0>{}, Int<1>{});      // ... of mix_mx4: mx4 planes + row scales out
        case row4_variant(0, 2, 2): return row4(Int<0>{}, Int<2>{}, Int<2>{});      // FFN2 + LN2 in the mx arithmetic, residual from mx planes
        case row4_variant(0, 0, 2): return row4(Int<0>{}, Int<0>{}, Int<2>{});      // split-bf16 arithmetic, residual from mx planes
        case row4_variant(0, 0, 1): return row4(Int<0>{}, Int<0>{}, Int<1>{});      // split-bf16 arithmetic, residual from split-bf16 planes
        }
        break;
    }
    case GemmKernel::Qkv4:
        return pick<5, 4>(p.mt, [&](auto MT) {
            static_assert((size_t)32 * CV(MT) * kQkvLd * 4 <= row4_lds_bytes<3, CV(MT)>(), "the V pass transposes its tile through the operand ring's memory");
            return launch_kernel<gemm_row4_bf16<3, 3, CV(MT), 3, 2, 0>>(dim3((t.Rvt + 32 * CV(MT) - 1) / (32 * CV(MT)), 3), dim3(256), row4_lds_bytes<3, CV(MT)>(), s, t);
        });
    case GemmKernel::PlMx:
        return pick<160, 192, 224, 256, 128, 64>(p.bm, [&](auto BM) { return launch_pl<1, CV(BM), false, 2>(s, t); });
    case GemmKernel::PlMx4:
        // + the A tile's scale bytes (8 per row and cross unit) + two stages of weight block scales; two workgroups per CU must still fit (a first build reserved 32 bytes per
        // row = 78.3 KB per workgroup and ran 25 % slower: one workgroup per CU)
        return launch_pl<1, 256, false, 3>(s, t, kMx4RowScaleLds + 2048);
    case GemmKernel::PlF16:
        return pick<3, 2, 1>(p.nsplit, [&](auto NS) {
            return pick<256, 128, 64>(p.bm, [&](auto BM) { return launch_pl<CV(NS), CV(BM), false, 1>(s, t); });
        });
    case GemmKernel::Qkv8:
        return pick<3, 2>(p.nb, [&](auto NB) {
            return pick<3, 1>(p.nsplit, [&](auto NS) {
                return pick<3, 2>(p.mt, [&](auto MT) {
                    return pick<1, 0>(p.apart, [&](auto AP) {
                        const dim3 grid((t.Rvt + 64 * CV(MT) - 1) / (64 * CV(MT)), CV(AP) ? 3 : 1);
                        return launch_kernel<gemm_qkv8_bf16<CV(NS), CV(NB), CV(MT), CV(AP) != 0>>(grid, dim3(512), qkv8_lds_bytes<CV(NB), CV(MT)>(), s, t);
                    });
                });
            });
        });
    case GemmKernel::Row8cTwoLn:
        return pick<3, 1>(p.nsplit, [&](auto NS) { return launch_kernel<gemm_row8c_bf16<CV(NS), 4, 2, 2>>(dim3((t.R + 127) / 128, 1), dim3(512), row8c_lds_bytes<4, 2>(), s, t); });
    case GemmKernel::Row8c:
    case GemmKernel::Row8cGrouped:
        return pick<3, 2>(p.nb, [&](auto NB) {
            return pick<3, 1>(p.nsplit, [&](auto NS) {
                return pick<3, 2>(p.mt, [&](auto MT) {
                    const dim3 grid((t.R + 64 * CV(MT) - 1) / (64 * CV(MT)), t.k_groups > 1 ? t.k_groups : 1);
                    return launch_kernel<gemm_row8c_bf16<CV(NS), CV(NB), CV(MT), 1>>(grid, dim3(512), row8c_lds_bytes<CV(NB), CV(MT)>(), s, t);
                });
            });
        });
    case GemmKernel::Row8:
        return pick<3, 2>(p.nb, [&](auto NB) {
            return pick<3, 1>(p.nsplit, [&](auto NS) {
                return pick<3, 2>(p.mt, [&](auto MT) {
                    const dim3 grid((t.R + 64 * CV(MT) - 1) / (64 * CV(MT)));
                    return launch_kernel<gemm_row8_bf16<CV(NS), CV(NB), CV(MT)>>(grid, dim3(512), row8_lds_bytes<CV(NB), CV(MT)>(), s, t);
                });
            });
        });
    case GemmKernel::PlBf16:
        if (p.nsplit == 3) {
            if (p.k1) return pick<128, 64>(p.bm, [&](auto BM) { return launch_pl<3, CV(BM), true, 0>(s, t); });
            return pick<160, 192, 224, 256, 128, 64>(p.bm, [&](auto BM) { return launch_pl<3, CV(BM), false, 0>(s, t); });
        }
        if (p.k1) return pick<128, 64>(p.bm, [&](auto BM) { return launch_pl<1, CV(BM), true, 0>(s, t); });
        return pick<256, 128, 64>(p.bm, [&](auto BM) { return launch_pl<1, CV(BM), false, 0>(s, t); });
    case GemmKernel::RowsF32:
        return pick<5, 16, 24>(p.nb, [&](auto NT) { return launch_kernel<gemm_rows_f32<CV(NT)>>(dim3((t.R + kRowsBM - 1) / kRowsBM), dim3(256), rows_lds_bytes<CV(NT)>(), s, t); });
    case GemmKernel::TileF32:
    case GemmKernel::TileRowsF32:
        return launch_kernel<gemm_tile_f32>(dim3((t.R + kTileBM - 1) / kTileBM, (t.N + kTileBN - 1) / kTileBN), dim3(256), kTileLds, s, t);
    case GemmKernel::None: break;
    }
    return hipErrorInvalidValue;
}

// Plan (gemm_plan.h: which kernel, which tile, split-K, where the rows go), then execute: build the A planes if the producer did not, launch the
// kernel on the arguments the plan implies, run ln_rows where the epilogue is a pass of its own.
int launch_gemm(fs2_handle* h, hipStream_t s, const char* name, GemmArgs a, int precision = FS2_PREC_FP32) {
    if (h) call_defaults(a, h->kp, h->kp_cap, h->cur_regime);
    const GemmPlan p = plan_gemm(a, precision, opts());
    if (p.err) return fail(h, p.err, p.msg, name, p.m0, p.m1);
    a.ksplit = 1;
    // the launched arguments: a, with the output routed and the epilogue split off as the plan says
    GemmArgs t = a;
    if (precision != FS2_PREC_FP32) t.W = reinterpret_cast<const float*>(a.Wb);
    if (p.y == RowsOut::Scratch) { t.Y = a.scratch; t.ldy = a.N; }
    if (p.y == RowsOut::KpartSlab) { t.Y = a.kpart; t.ldy = a.N; }
    if (p.rows_pass) { t.act_post = 0; t.Yp = nullptr; }      // the row kernel applies the epilogue and writes the planes
    if (p.ksplit > 1) {
        t.ksplit = p.ksplit;
        t.relu_pre = 0;                                      // partial sums: ReLU only after they are added (ln_rows)
        t.kpart = a.kpart + (p.y == RowsOut::KpartSlab ? (size_t)a.R * a.N : 0);
        t.kpart_stride = (size_t)a.R * t.ldy;
    }
    if (p.build_planes) t.Xp = a.xp_scratch;
    if (p.kernel == GemmKernel::Row8cGrouped) { t.N = a.N / a.k_groups; t.ln_groups = 0; }      // a workgroup row per group (grid.y), N = one group's outputs

    char nm[112];
    if (p.build_planes) {
        snprintf(nm, sizeof nm, "%s.planes", name);
        Scope sc(h, s, nm, 0.0, 8.0 * a.R * a.Cpad);
        const int64_t n = (int64_t)a.R * (a.Cpad / 4);
        hipLaunchKernelGGL(to_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.X, a.ldx, a.C, a.R, a.Cpad / 32, a.xp_scratch, a.mx ? 2 : (a.f16_terms ? 1 : 0), a.yp_scale);
    }
    hipError_t e;
    {
        Scope sc(h, s, name, 2.0 * a.R * (double)a.N * a.C * a.ktaps, 4.0 * ((double)a.R * a.C + (double)a.N * a.C * a.ktaps + (double)a.R * a.N));
        e = run_plan(s, p, t);
    }
    if (e == hipSuccess && p.rows_pass) {
        snprintf(nm, sizeof nm, "%s.rows", name);
        Scope sc(h, s, nm, 0.0, 8.0 * a.R * a.N);
        GemmArgs r = a;
        r.Y = t.Y; r.ldy = t.ldy; r.ksplit = t.ksplit; r.kpart = t.kpart; r.kpart_stride = t.kpart_stride;
        hipLaunchKernelGGL(ln_rows, dim3(((size_t)a.R * (a.ln_groups > 1 ? a.ln_groups : 1) + 3) / 4), dim3(256), 0, s, r);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(h, FS2_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e));
    return FS2_OK;
}

// ------------------------------------------------------------------ self-attention: attn_plan.h decides, these run the decision
static_assert(kPlanFp32 == FS2_PREC_FP32 && kPlanBf16x3 == FS2_PREC_BF16X3 && kPlanErrUnsupported == FS2_ERR_UNSUPPORTED && kAttBlk == 2 * kAttBQ, "attn_plan.h, att_grid64");

// A self-attention launch: its pointers and the numbers the plan reads (c.qkv_rows and the plane distances: launch_attention takes them from the pointers).
struct AttnIo {
    const float* qkv = nullptr;                    // fp32 QKV rows [R, 3D]; nullptr: the projection has left the bf16 operands
    float* ctx = nullptr; void* ctxp = nullptr;    // the context as fp32 rows [R, D] and / or (bf16 kernels) as planes
    __bf16 *qkh = nullptr, *qkl = nullptr, *vth = nullptr, *vtl = nullptr;      // bf16 kernels: qk_hi/lo [Rvt][2D], vt_hi/lo [D][Rvt] (Rvt % 32 == 0)
    const DevLayout* dl = nullptr;
    int mask_q = 0; double flops = 0.0;
    AttnCall c;
    int *slow_count = nullptr, *slow_count2 = nullptr;      // attn_w32's counters of the handle (without one: the caller's, if any) and of the call in progress (launch_attention sets them)
};

// the layout fields AttnArgs and AttnB16Args share
template <class A>
void attn_layout_args(A& a, const AttnIo& io) {
    const DevLayout& dl = *io.dl;
    a.start = dl.start; a.len = dl.len; a.klen = dl.klen; a.work = dl.work;
    a.nwork = dl.dims ? dl.dims + 1 : nullptr;      // device-driven layout: the count of valid items, next to the row count in dims
    a.nitems = io.c.nwork; a.D = io.c.D; a.mask_q = io.mask_q;
}

// The instantiation an attention plan names, on the arguments of the launch.  Instantiated in the order of the branches and of pick's values, like run_plan's.
hipError_t run_attn_plan(hipStream_t s, const AttnPlan& p, const AttnIo& io) {
    const dim3 grid(p.grid_x, p.grid_y);
    const int D = io.c.D;
    if (p.kernel == AttnKernel::F32) {
        AttnArgs a;
        attn_layout_args(a, io);
        a.qkv = io.qkv; a.ld = 3 * D; a.ctx = io.ctx; a.ldc = D; a.scale = p.softmax_scale;
        return pick<128, 192, 64, 256>(p.dk, [&](auto DK) { return launch_kernel<attn_f32<CV(DK)>>(grid, dim3(256), attn_lds_bytes<CV(DK)>(), s, a); });
    }
    AttnB16Args a;
    attn_layout_args(a, io);
    a.qk_hi = io.qkh; a.qk_lo = io.qkl; a.ldqk = 2 * D; a.vt_hi = io.vth; a.vt_lo = io.vtl; a.Rvt = io.c.Rvt; a.ctx = io.ctx; a.ldc = D;
    a.ctxp = io.ctxp; a.ctxp_chunks = D / 32; a.slow_count = io.slow_count; a.slow_count2 = io.slow_count2;
    a.qk_lo_bytes = (unsigned)io.c.qk_lo_dist; a.vt_lo_bytes = (unsigned)io.c.vt_lo_dist;
    if (p.kernel == AttnKernel::W32)
        return pick<128, 192>(p.dk, [&](auto DK) { return launch_kernel<attn_w32<CV(DK)>>(grid, dim3(256), attn_w32_lds_bytes<CV(DK)>(), s, a); });
    if (p.kernel == AttnKernel::B16)
        return pick<128, 192, 64, 256>(p.dk, [&](auto DK) {
            return pick<3, 1>(p.nsplit, [&](auto NS) { return launch_kernel<attn_bf16<CV(DK), CV(NS)>>(grid, dim3(256), attn_b16_lds_bytes<CV(DK)>(), s, a); });
        });
    return hipErrorInvalidValue;
}
#undef CV

// what the plan reads of the pointers
void attn_call_pointers(AttnIo& io) {
    io.c.qkv_rows = io.qkv != nullptr;
    io.c.qk_lo_dist = reinterpret_cast<const char*>(io.qkl) - reinterpret_cast<const char*>(io.qkh);
    io.c.vt_lo_dist = reinterpret_cast<const char*>(io.vtl) - reinterpret_cast<const char*>(io.vth);
}

// Plan (attn_plan.h), then execute: qkv_split under "<name>.split" where the operands arrive as fp32 rows, the kernel under `name`.
int launch_attention(fs2_handle* h, hipStream_t s, const char* name, AttnIo io) {
    attn_call_pointers(io);
    AttnCall& c = io.c;
    if (h) io.slow_count = h->counters;      // (without a handle the caller's counter stays: fs2_op_launch_attention)
    io.slow_count2 = (h && h->cur_status) ? h->cur_status + 5 : nullptr;
    const AttnPlan p = plan_attention(c, opts());
    if (p.err) return fail(h, p.err, p.msg, p.m0);
    if (p.kernel == AttnKernel::None) return FS2_OK;
    if (p.split_pass) {
        char nm[112];
        snprintf(nm, sizeof nm, "%s.split", name);
        Scope sc(h, s, nm, 0.0, 4.0 * c.R * 3.0 * c.D * 2);
        QkvSplitArgs q;
        q.qkv = io.qkv; q.R = c.R; q.Rvt = c.Rvt; q.D = c.D; q.dk = p.dk; q.scale = p.softmax_scale;
        q.qk_hi = io.qkh; q.qk_lo = io.qkl; q.vt_hi = io.vth; q.vt_lo = io.vtl;
        const hipError_t e = launch_kernel<qkv_split>(dim3(c.Rvt / 32), dim3(256), (size_t)32 * (c.D + 1) * 4, s, q, (size_t)32 * (1024 + 1) * 4);
        if (e != hipSuccess) return fail(h, FS2_ERR_HIP, "%s launch: %s", nm, hipGetErrorString(e));
    }
    Scope sc(h, s, name, io.flops, 0.0);
    const hipError_t e = run_attn_plan(s, p, io);
    if (e != hipSuccess) return fail(h, FS2_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e));
    return FS2_OK;
}

// ------------------------------------------------------------------ layouts (layout.h builds them, layout_rule.h places them in `meta`)
static_assert(kOvfRows == FS2_OVF_ROWS && kOvfLmax == FS2_OVF_LMAX && kOvfPe == FS2_OVF_PE && kOvfEmpty == FS2_OVF_EMPTY && kOvfBadId == FS2_OVF_BAD_ID,
              "layout_rule.h restates these");

size_t layout_dev_ints(const HostLayout& L) { return (size_t)MetaDev::ints(L.B, L.Rpad, L.nwork()); }

// uploads start/len/klen/vlen/work, then derives row_pos/row_seq on the device
int upload_layout(fs2_handle* h, hipStream_t s, const HostLayout& L, int* dev, DevLayout& D) {
    std::vector<int> host;
    host.reserve(4 * L.B + 2 * L.work.size());
    host.insert(host.end(), L.start.begin(), L.start.end());
    host.insert(host.end(), L.len.begin(), L.len.end());
    host.insert(host.end(), L.klen.begin(), L.klen.end());
    host.insert(host.end(), L.vlen.begin(), L.vlen.end());
    for (auto& w : L.work) { host.push_back(w.x); host.push_back(w.y); }
    const void* src = host.data();
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive) {
        // Inside a HIP-graph capture the copy becomes a memcpy node that reads its source at every replay: give it pinned host
        // memory that lives as long as the handle (a pageable std::vector is neither capturable nor alive at replay time).
        void* pin = nullptr;
        if (!h) return fail(h, FS2_ERR_STATE, "layout upload inside a graph capture needs a model handle");
        HIP_TRY(h, hipHostMalloc(&pin, host.size() * sizeof(int), hipHostMallocDefault));
        memcpy(pin, host.data(), host.size() * sizeof(int));
        h->graph_pinned.push_back(pin);
        src = pin;
    }
    HIP_TRY(h, hipMemcpyAsync(dev, src, host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    const MetaHost m = MetaHost::at(L.B, L.Rpad, L.nwork());
    D.start = dev + m.start; D.len = dev + m.len; D.klen = dev + m.klen; D.vlen = dev + m.vlen;
    D.work = reinterpret_cast<int2*>(dev + m.work);
    D.row_pos = dev + m.row_pos; D.row_seq = dev + m.row_seq;
    hipLaunchKernelGGL(build_row_meta, dim3((L.Rpad + 255) / 256), dim3(256), 0, s, D.start, D.len, L.B, L.Rpad, D.row_pos, D.row_seq);
    HIP_TRY(h, hipGetLastError());
    return FS2_OK;
}

// device-driven variant: the layout arrays are produced by frame_layout_dev from the device frame counts
int device_layout(fs2_handle* h, hipStream_t s, const HostLayout& L, int* dev, DevLayout& D, const int* olens32, int compat, int masked,
                  int lmax_cap, int pe_rows, int* status) {
    const MetaDev m = MetaDev::at(L.B, L.Rpad, L.nwork());
    D.start = dev + m.start; D.len = dev + m.len; D.klen = dev + m.klen; D.vlen = dev + m.vlen;
    D.pcum = dev + m.pcum; D.dims = dev + m.dims;
    D.work = reinterpret_cast<int2*>(dev + m.work);
    D.row_pos = dev + m.row_pos; D.row_seq = dev + m.row_seq;
    hipLaunchKernelGGL(frame_layout_dev, dim3(1), dim3(kLayoutThreads), 0, s, olens32, L.B, compat, masked, L.R, L.nwork(), lmax_cap, pe_rows,
                       D.start, D.len, D.klen, D.vlen, dev + m.rank, dev + m.woff, D.pcum, D.work, D.dims, status, h ? h->gap : kGap);
    hipLaunchKernelGGL(build_row_meta, dim3((L.Rpad + 255) / 256), dim3(256), 0, s, D.start, D.len, L.B, L.Rpad, D.row_pos, D.row_seq);
    HIP_TRY(h, hipGetLastError());
    return FS2_OK;
}

// ------------------------------------------------------------------ the model's launches: model_launches.h forms them, these run them
// standalone LayerNorm over rows (ln_args)
int launch_ln(fs2_handle* h, hipStream_t s, const char* name, const GemmArgs& a) {
    if (a.N > 1024 || a.N % 4) return fail(h, FS2_ERR_UNSUPPORTED, "%s: LayerNorm width %d", name, a.N);
    Scope sc(h, s, name, 0.0, 8.0 * a.R * a.N);
    hipLaunchKernelGGL(ln_rows, dim3((a.R + 3) / 4), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, FS2_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e));
    return FS2_OK;
}

// a GEMM or LayerNorm step under its profile name "<tag>.<name>" (tag == nullptr: the name alone)
int launch_step(fs2_handle* h, hipStream_t s, const char* tag, const Step& st, int prec) {
    char nm[96];
    snprintf(nm, sizeof nm, "%s%s%s", tag ? tag : "", tag ? "." : "", st.name);
    return st.kind == StepKind::LayerNorm ? launch_ln(h, s, nm, st.a) : launch_gemm(h, s, nm, st.a, prec);
}

// ------------------------------------------------------------------ the row steps between the GEMMs
// One function per step: it owns the profile name and the grid and block arithmetic.  fs2_encode / fs2_decode_ctl call it with their handle, the test hook
// fs2_op_launch_row_step with h == nullptr (no profile record, errors to the process-wide message), as launch_gemm and launch_attention allow.
#define ROW_STEP_TRY(h, name) do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(h, FS2_ERR_HIP, "%s launch: %s", name, hipGetErrorString(e_)); } while (0)

// enc.embed: rows = E[xs] x_scale + alpha pe[pos], optionally also as planes
int embed_launch(fs2_handle* h, hipStream_t s, const RowStepArgs& a) {
    Scope sc(h, s, "enc.embed", 0, 4.0 * a.R * a.D * 2);
    hipLaunchKernelGGL(embed_pe, dim3((a.R + 3) / 4), dim3(256), 0, s, a.xs, a.Tmax, a.E, a.idim, a.D, a.pe, a.pe_alpha, a.x_scale, a.row_pos, a.row_seq, a.R, a.rows, a.planes);
    ROW_STEP_TRY(h, "enc.embed");
    return FS2_OK;
}

// dur.post: the padded duration outputs, then the scan of the durations actually used (a.ds, or the ones just written)
int dur_post_launch(fs2_handle* h, hipStream_t s, const RowStepArgs& a) {
    Scope sc(h, s, "dur.post", 0, 0);
    const int n = a.B * a.Tmax;
    hipLaunchKernelGGL(dur_finalize, dim3((n + 255) / 256), dim3(256), 0, s, a.dlog_rows, a.start, a.vlen, a.B, a.Tmax, a.d_log, a.d_int, a.d_int2);
    ROW_STEP_TRY(h, "dur.post");
    hipLaunchKernelGGL(dur_scan, dim3(a.B), dim3(256), 0, s, a.ds ? a.ds : a.d_int, a.Tmax, a.vlen, a.cum, a.olens, a.olens32, a.alpha, a.xs, a.idim, a.scum, a.so32, a.K);
    ROW_STEP_TRY(h, "dur.post");
    return FS2_OK;
}

// lr.index under FS2_VARSHORT: the frames' tokens and the short layout in one launch
int lr_index_short_launch(fs2_handle* h, hipStream_t s, const ShortLayoutArgs& sl) {
    Scope sc(h, s, "lr.index", 0, 4.0 * (2.0 * sl.R + 3.0 * sl.Rs_pad));
    hipLaunchKernelGGL(lr_index_short, dim3((std::max(sl.R, sl.Rs_pad) + 255) / 256), dim3(256), 0, s, sl);
    ROW_STEP_TRY(h, "lr.index");
    return FS2_OK;
}

// lr.index: the length regulator's index alone
int lr_index_launch(fs2_handle* h, hipStream_t s, const RowStepArgs& a) {
    Scope sc(h, s, "lr.index", 0, 4.0 * a.R);
    hipLaunchKernelGGL(lr_index_only, dim3((a.R + 255) / 256), dim3(256), 0, s, a.cum_in, a.Tmax, a.ilen, a.row_pos, a.row_seq, a.vlen, a.R, a.index_rows);
    ROW_STEP_TRY(h, "lr.index");
    return FS2_OK;
}

// lr.expand: the length regulator, rows (and planes) with the index
int lr_expand_launch(fs2_handle* h, hipStream_t s, const RowStepArgs& a) {
    Scope sc(h, s, "lr.expand", 0, 4.0 * a.R * a.D * 2);
    hipLaunchKernelGGL(lr_expand, dim3((a.R + 3) / 4), dim3(256), 0, s, a.src_rows, a.D, a.tok_start, a.ilen, a.cum_in, a.Tmax, a.row_pos, a.row_seq, 0, a.vlen, a.R, a.rows, a.index_rows,
                       a.planes);
    ROW_STEP_TRY(h, "lr.expand");
    return FS2_OK;
}

// var.gather0: layer 0 of both predictors from the token-level products (one wavefront per (row, predictor))
int var_gather0_launch(fs2_handle* h, hipStream_t s, const TokGatherArgs& tg) {
    Scope sc(h, s, "var.gather0", 0.0, 4.0 * tg.R * tg.chans * (6.0 + 2.0));
    hipLaunchKernelGGL(var_gather0, dim3((2 * (size_t)tg.R + 3) / 4), dim3(256), 0, s, tg);
    ROW_STEP_TRY(h, "var.gather0");
    return FS2_OK;
}

// var.embed: bucket search and embedding add in place
int var_embed_launch(fs2_handle* h, hipStream_t s, const RowStepArgs& a) {
    Scope sc(h, s, "var.embed", 0, 4.0 * a.R * a.D * 4);
    hipLaunchKernelGGL(bucket_embed, dim3((a.R + 3) / 4), dim3(256), 0, s, a.rows, a.D, a.row_pos, a.row_seq, a.R, a.es, a.es_stride, a.ps, a.ps_stride, a.e_rows, a.p_rows, a.ebins, a.pbins,
                       a.nb, a.Te, a.Tp, a.qe_rows, a.qp_rows, a.planes);
    ROW_STEP_TRY(h, "var.embed");
    return FS2_OK;
}

// dec.in.gather: bucket search + embedding add + decoder input layer as one row kernel over the token-level products.  FS2_VARSHORT (tg.f2s): the predictions
// are per short row; where they are the source (tg.sqe / tg.sqp) their buckets are searched there first (var_bucket_short: two 255-bin searches per short row
// instead of per frame), under this launch's profile name, and the row kernel reads the indices through the frame-to-short map
int dec_in_gather_launch(fs2_handle* h, hipStream_t s, const TokGatherArgs& tg) {
    Scope sc(h, s, "dec.in.gather", 0, 4.0 * tg.R * tg.D * (tg.x0 ? 3.0 : 2.0));
    if (tg.f2s && (tg.sqe || tg.sqp)) {
        hipLaunchKernelGGL(var_bucket_short, dim3((tg.Rs + 255) / 256), dim3(256), 0, s, tg.sqe ? tg.e_rows : nullptr, tg.sqp ? tg.p_rows : nullptr, tg.srow_pos, tg.Rs, tg.ebins, tg.pbins,
                           tg.nb, const_cast<int*>(tg.sqe), const_cast<int*>(tg.sqp));
        ROW_STEP_TRY(h, "dec.in.gather");
    }
    hipLaunchKernelGGL(dec_in_gather, dim3((tg.R + 3) / 4), dim3(256), 0, s, tg);
    ROW_STEP_TRY(h, "dec.in.gather");
    return FS2_OK;
}

// <tag>.in.planes: fp32 rows -> split-bf16 planes, for a stack whose producer wrote none
int to_planes_launch(fs2_handle* h, hipStream_t s, const char* name, const float* rows, int R, int D, void* planes) {
    Scope sc(h, s, name, 0.0, 8.0 * R * D);
    const int64_t n = (int64_t)R * (D / 4);
    hipLaunchKernelGGL(to_planes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, D, D, R, D / 32, planes);
    ROW_STEP_TRY(h, name);
    return FS2_OK;
}

// dec.out.rows: fp32 rows rebuilt from the planes (hi + lo)
int planes_to_rows_launch(fs2_handle* h, hipStream_t s, const char* name, const void* planes, int R, int D, float* rows) {
    Scope sc(h, s, name, 0.0, 8.0 * R * D);
    const int64_t n = (int64_t)R * (D / 4);
    hipLaunchKernelGGL(planes_to_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, planes, D / 32, R, D, rows, D);
    ROW_STEP_TRY(h, name);
    return FS2_OK;
}

// FFT-block stack, every block variant (block_steps).  b.x0 holds the input and then the output; po: the planes b.x0p alone do.
int run_stack(fs2_handle* h, hipStream_t s, const char* tag, const Stack& st, int D, int heads, const Rows& r, const HostLayout& L, const DevLayout& dl,
              int mask_q, const StackBufs& b, int prec, bool x0p_ready, int ffn_terms, bool po = false) {
    char nm[96];
    double att_flops = 0;
    for (size_t i = 0; i < L.klen.size(); ++i) att_flops += 4.0 * D * (double)L.klen[i] * std::min(L.len[i], mask_q ? L.klen[i] : L.len[i]);
    const bool pl = prec != FS2_PREC_FP32;
    int rc;
    if (pl && !st.pre_ln && !x0p_ready) {
        snprintf(nm, sizeof nm, "%s.in.planes", tag);
        if ((rc = to_planes_launch(h, s, nm, b.x0, r.R, D, b.x0p))) return rc;
    }
    for (const Layer& ly : st.layers)
        for (const Step& step : block_steps(st, ly, D, r, b, prec, ffn_terms, po, opts())) {
            if (step.kind != StepKind::Attention) rc = launch_step(h, s, tag, step, prec);
            else {
                snprintf(nm, sizeof nm, "%s.%s", tag, step.name);
                rc = launch_attention(h, s, nm, AttnIo{step.a.X, step.a.Y, step.a.Yp, (__bf16*)b.qkh, (__bf16*)b.qkl, (__bf16*)b.vth, (__bf16*)b.vtl, &dl, mask_q, att_flops,
                                                       AttnCall{st.Dp, heads, st.dk, prec, r.R, r.Rpad, h->cur_regime, L.nwork()}});
            }
            if (rc) return rc;
        }
    if (st.pre_ln) {      // Encoder.forward: xs = after_norm(xs); downstream consumers read x0 (fp32) and, in the bf16 modes, its planes
        snprintf(nm, sizeof nm, "%s.after_norm", tag);
        if ((rc = launch_ln(h, s, nm, ln_args(b.x0, D, r, D, st.after_g, st.after_b, b.x0, pl ? b.x0p : nullptr)))) return rc;
    }
    return FS2_OK;
}

int run_predictor(fs2_handle* h, hipStream_t s, const char* tag, const Predictor& p, const float* X, int ldx, const Rows& r, float* tmp0, float* tmp1, float* out_rows,
                  int prec, const void* Xp, void* xps) {
    for (size_t l = 0; l < p.conv.size(); ++l)
        if (int rc = launch_step(h, s, tag, predictor_step(p, l, X, ldx, r, tmp0, tmp1, out_rows, prec, Xp, xps), prec)) return rc;
    return FS2_OK;
}

// tg: layer 0 from the token-level products (tok.proj): a row kernel in place of the convolution(s)
int run_predictors_fused(fs2_handle* h, hipStream_t s, const FusedPredictors& v, const float* X, int ldx, const Rows& r, const void* Xp, void* xps, float* vp, float* vs,
                         float* e_rows, float* p_rows, int prec, const TokGatherArgs* tg = nullptr) {
    if (tg)
        if (int rc = var_gather0_launch(h, s, *tg)) return rc;
    for (const Step& st : fused_predictor_steps(v, h->energy, h->pitch, !tg, X, ldx, r, Xp, xps, vp, vs, e_rows, p_rows, opts()))
        if (int rc = launch_step(h, s, nullptr, st, prec)) return rc;
    return FS2_OK;
}

// ------------------------------------------------------------------ weight loading
// src [rows, cols] -> dst with every block of dk rows (by_cols: columns) moved to a block of dkp (dst pre-zeroed)
__global__ void pad_heads(const float* src, int rows, int cols, int dk, int dkp, int by_cols, float* dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (size_t)r * cols);
    if (by_cols) dst[(size_t)r * ((cols / dk) * dkp) + (c / dk) * dkp + c % dk] = src[i];
    else dst[((size_t)(r / dk) * dkp + r % dk) * cols + c] = src[i];
}

// What build_weight reads besides the plan: the tensors of every part (w: at the first column of a concat half), the BatchNorm statistics, and the two launch
// arguments that differ between its callers.
struct WeightSrc {
    const float* w[3] = {};
    const float* bias[3] = {};
    const float *bn_g = nullptr, *bn_b = nullptr, *bn_m = nullptr, *bn_v = nullptr;
    float bn_eps = 1e-5f;
    bool wb_f16 = false;      // the "split-bf16" image holds fp16 (fs2_op_conv_gemm in the fp16 arithmetic)
};

// The one executor of a weight plan (weight_plan.h): the images the plan gives bytes, from `alloc(image, bytes)` (nullptr: it has recorded the failure), filled on
// stream s.  kw is measured here, from the source the plan names; scratch: 16 bytes for that (needed where the plan has an mx source).  Every repack kernel is
// launched here and nowhere else.
template <class Alloc>
bool build_weight(hipStream_t s, const WeightAsk& a, const WeightPlan& p, const WeightSrc& src, unsigned* scratch, Alloc&& alloc, Gemm& g) {
    g.N = p.N; g.C = a.C; g.ktaps = a.ktaps; g.Cpad = p.Cpad;
    void* img[kWeightImages] = {};
    for (int i = 0; i < kWeightImages; ++i)
        if (p.bytes[i] && !(img[i] = alloc((WeightImage)i, p.bytes[i]))) return false;
    g.w = (float*)img[kImgW]; g.wb = img[kImgWb]; g.wf = img[kImgWf]; g.wm = img[kImgWm]; g.wm4 = img[kImgWm4]; g.ws4 = (unsigned char*)img[kImgWs4]; g.bias = (float*)img[kImgBias];
    for (int i : {kImgW, kImgWb, kImgWf})
        if (img[i]) hipMemsetAsync(img[i], 0, p.bytes[i], s);
    const int k = a.ktaps, Neach = a.Neach;
    // kw from max |w| of `from` ([.][C][k], or the fp32 image with rows of ld floats: BatchNorm folded in), then the mx and mx4 images of it
    auto mx_images = [&](const float* from, int64_t count, int ld) {
        g.kw = fp8_scale_exponent(device_absmax(s, from, count, scratch));
        if (g.wm)
            hipLaunchKernelGGL(repack_weight_mx, dim3((unsigned)((p.bytes[kImgWm] / 2 + 255) / 256)), dim3(256), 0, s, from, p.N, a.C, k, p.Npad, g.kw,
                               reinterpret_cast<unsigned short*>(g.wm), ld);
        if (g.wm4) {      // (fp4 cross terms, one scale byte per 16-channel block: preset to 127 = 2^0)
            hipMemsetAsync(g.ws4, 127, p.bytes[kImgWs4], s);
            hipLaunchKernelGGL(repack_weight_mx4, dim3((unsigned)((p.bytes[kImgWm4] / 4 + 255) / 256)), dim3(256), 0, s, from, p.N, a.C, k, p.Npad, g.ws4, reinterpret_cast<unsigned*>(g.wm4));
        }
    };
    // (the measurement waits for the stream: from the tensor it runs first, so that the repacks below are still running while the host looks up the next layer)
    if (p.mx_src == MxSource::Tensor) mx_images(src.w[0], (int64_t)Neach * a.C * k, 0);
    for (int part = 0; part < a.parts; ++part) {      // (the parts are whole row ranges of the fp32 and bf16 images: each is repacked as a layer of Npad = Neach rows)
        const int64_t tb = (int64_t)Neach * k * p.nchunks * 32, total = (int64_t)Neach * k * p.Cpad;
        for (int f16 = 0; f16 <= 1; ++f16)
            if (void* dst = f16 ? g.wf : g.wb)
                hipLaunchKernelGGL(repack_weight_bf16, dim3((unsigned)((tb + 255) / 256)), dim3(256), 0, s, src.w[part], Neach, a.C, k, Neach, p.nchunks, src.bn_g, src.bn_v,
                                   src.bn_eps, reinterpret_cast<__bf16*>(dst) + (size_t)part * Neach * k * p.nchunks * 64, f16 || src.wb_f16 ? 1 : 0, a.src_cols);
        if (g.w)
            hipLaunchKernelGGL(repack_weight, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src.w[part], Neach, a.C, k, Neach, p.Cpad, src.bn_g, src.bn_v, src.bn_eps,
                               g.w + (size_t)part * Neach * k * p.Cpad, a.src_cols);
    }
    // (from the fp32 image just made; the layer's operand is a tanh output: |x| <= 1 is the a-priori bound of kPostKa)
    if (p.mx_src == MxSource::Folded) mx_images(g.w, (int64_t)p.Npad * k * p.Cpad, p.Cpad);
    if (g.bias && a.bias)
        for (int part = 0; part < a.parts; ++part) hipMemcpyAsync(g.bias + (size_t)part * Neach, src.bias[part], Neach * sizeof(float), hipMemcpyDeviceToDevice, s);
    else if (g.bias)
        hipLaunchKernelGGL(bn_fold_bias, dim3((Neach + 255) / 256), dim3(256), 0, s, src.bn_g, src.bn_b, src.bn_m, src.bn_v, src.bn_eps, Neach, g.bias);
    return true;
}

struct Loader {
    fs2_handle* h; hipStream_t s;
    std::map<std::string, const fs2_tensor_desc*> m;
    int rc = FS2_OK;
    unsigned* absmax_scratch = nullptr;
    // tensors of the loader's own making, looked up like the caller's (head-padded projection weights, tok.proj's stacked weight): released with the loader
    struct Synth { fs2_tensor_desc desc; std::string name; float* mem; };
    std::list<Synth> synth;
    ~Loader() {
        if (absmax_scratch) hipFree(absmax_scratch);
        if (!synth.empty()) hipStreamSynchronize(s);
        for (Synth& t : synth) hipFree(t.mem);
    }
    // Registers `name`: a tensor of n floats of device memory, described like `like` (the caller sets the shape).  nullptr on error.
    Synth* add_synth(const std::string& name, const fs2_tensor_desc& like, size_t n) {
        float* p = nullptr;
        if (hipMalloc((void**)&p, n * sizeof(float)) != hipSuccess) { if (!rc) rc = fail(h, FS2_ERR_HIP, "hipMalloc failed"); return nullptr; }
        synth.push_back(Synth{like, name, p});
        Synth& t = synth.back();
        t.desc.name = t.name.c_str(); t.desc.data = p;
        m[t.name] = &t.desc;
        return &t;
    }
    // Registers "<name>#pad": the tensor `name` ([D, C] weight, or [D] bias when C == 0) with every head's dk rows (pad_cols: columns)
    // moved to a block of dkp, zeros in between.  Returns the new name ("" on error).
    std::string padded_tensor(const std::string& name, int heads, int dk, int dkp, int D, int C, bool pad_cols) {
        const fs2_tensor_desc* d = C ? get(name, {D, pad_cols ? heads * dk : C}) : get(name, {D});
        if (!d) return "";
        const int Dp = heads * dkp;
        const size_t n = C ? (pad_cols ? (size_t)D * Dp : (size_t)Dp * C) : (size_t)Dp;
        Synth* t = add_synth(name + "#pad", *d, n);
        if (!t) return "";
        fs2_tensor_desc* nd = &t->desc;
        hipMemsetAsync(t->mem, 0, n * sizeof(float), s);
        const int rows = pad_cols ? D : heads * dk, cols = C ? (pad_cols ? heads * dk : C) : 1;
        hipLaunchKernelGGL(pad_heads, dim3((unsigned)(((size_t)rows * cols + 255) / 256)), dim3(256), 0, s, (const float*)d->data, rows, cols, dk, dkp, pad_cols ? 1 : 0, t->mem);
        if (C) { nd->shape[0] = pad_cols ? D : Dp; nd->shape[1] = pad_cols ? Dp : C; } else nd->shape[0] = Dp;
        return t->name;
    }
    const fs2_tensor_desc* get(const std::string& name, const int64_t* shape, int ndim) {
        auto it = m.find(name);
        if (it == m.end()) { if (!rc) rc = fail(h, FS2_ERR_WEIGHT, "missing tensor %s", name.c_str()); return nullptr; }
        const fs2_tensor_desc* d = it->second;
        bool ok = d->ndim == ndim;
        for (int i = 0; ok && i < ndim; ++i) ok = d->shape[i] == shape[i];
        if (!ok) { if (!rc) rc = fail(h, FS2_ERR_WEIGHT, "tensor %s has the wrong shape", name.c_str()); return nullptr; }
        return d;
    }
    const fs2_tensor_desc* get(const std::string& name, std::initializer_list<int64_t> shape) { return get(name, shape.begin(), (int)shape.size()); }
    const float* data(const std::string& name, const int64_t* shape, int ndim) {
        const fs2_tensor_desc* d = get(name, shape, ndim);
        return d ? (const float*)d->data : nullptr;
    }
    // the one allocation of weight memory: owned by the handle (free_weights); msg: what a failure says
    void* take(size_t bytes, const std::string& msg) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { if (!rc) rc = fail(h, FS2_ERR_HIP, "%s", msg.c_str()); return nullptr; }
        h->allocs.push_back(p);
        return p;
    }
    float* dalloc(size_t n) { return (float*)take(std::max<size_t>(n, 1) * sizeof(float), "hipMalloc of " + std::to_string(n) + " floats failed"); }
    void* image(WeightImage i, size_t bytes) {
        static const char* const what[kWeightImages] = {nullptr, "bf16 weights", "the mx weight image", "the mx4 weight image", "the mx4 weight image", "fp16 weights", nullptr};
        static_assert(kImgWb == 1 && kImgWm == 2 && kImgWm4 == 3 && kImgWs4 == 4 && kImgWf == 5, "the messages follow the images");
        return what[i] ? take(bytes, std::string("hipMalloc of ") + what[i] + " failed") : dalloc(bytes / sizeof(float));
    }
    float* copy(const std::string& name, std::initializer_list<int64_t> shape) {
        const fs2_tensor_desc* d = get(name, shape);
        if (!d) return nullptr;
        size_t n = 1;
        for (int64_t v : shape) n *= (size_t)v;
        float* p = dalloc(n);
        if (p && hipMemcpyAsync(p, d->data, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess && !rc) rc = fail(h, FS2_ERR_HIP, "copy of %s failed", name.c_str());
        return p;
    }
    // two reference tensors of n elements each, back to back (parameters of stacked layers)
    float* copy2(const std::string& a_, const std::string& b_, std::initializer_list<int64_t> shape) {
        const fs2_tensor_desc *da = get(a_, shape), *db = get(b_, shape);
        if (!da || !db) return nullptr;
        size_t n = 1;
        for (int64_t v : shape) n *= (size_t)v;
        float* p = dalloc(2 * n);
        if (p) {
            hipMemcpyAsync(p, da->data, n * sizeof(float), hipMemcpyDeviceToDevice, s);
            hipMemcpyAsync(p + n, db->data, n * sizeof(float), hipMemcpyDeviceToDevice, s);
        }
        return p;
    }
    // The layer `ask` describes, from the tensors named: one weight (and bias, where the ask has one) per part; bn_prefix: the BatchNorm folded in, where it has one.
    // The plan says which images it gets and which shapes the tensors must have; the memory is the handle's.
    Gemm gemm(const WeightAsk& ask, const std::vector<std::string>& wnames, const std::vector<std::string>& bnames = {}, const std::string& bn_prefix = "") {
        const WeightPlan p = plan_weight(ask);
        WeightSrc src;
        bool ok = true;
        if (ask.bn) {
            src.bn_g = data(bn_prefix + ".weight", &p.vec_len, 1); src.bn_b = data(bn_prefix + ".bias", &p.vec_len, 1);
            src.bn_m = data(bn_prefix + ".running_mean", &p.vec_len, 1); src.bn_v = data(bn_prefix + ".running_var", &p.vec_len, 1);
            ok = src.bn_g && src.bn_b && src.bn_m && src.bn_v;
        }
        for (int part = 0; ok && part < ask.parts; ++part) {
            src.w[part] = data(wnames[part], p.w_shape, p.w_ndim);
            if ((ok = src.w[part] != nullptr)) src.w[part] += ask.col_off;
        }
        for (int part = 0; ok && ask.bias && part < ask.parts; ++part) ok = (src.bias[part] = data(bnames[part], &p.vec_len, 1)) != nullptr;
        if (ok && p.mx_src != MxSource::None && !absmax_scratch && hipMalloc((void**)&absmax_scratch, 16) != hipSuccess) { if (!rc) rc = fail(h, FS2_ERR_HIP, "hipMalloc failed"); ok = false; }
        Gemm g;
        if (ok) build_weight(s, ask, p, src, absmax_scratch, [this](WeightImage i, size_t bytes) { return image(i, bytes); }, g);
        return g;
    }
};

void load_stack(Loader& L, Stack& st, const std::string& pre, int nlayers, int D, int heads, int units, int k, const std::string& pe_pre,
                bool scaled, bool pre_ln, bool concat) {
    st.layers.resize(nlayers);
    st.dk = D / heads;
    const int dkp = padded_head_dim(st.dk);
    st.Dp = heads * dkp;
    st.pre_ln = pre_ln; st.concat = concat;
    if (pre_ln) { st.after_g = L.copy(pre + ".after_norm.weight", {D}); st.after_b = L.copy(pre + ".after_norm.bias", {D}); }
    for (int i = 0; i < nlayers; ++i) {
        const std::string p = pre + ".encoders_." + std::to_string(i);
        Layer& ly = st.layers[i];
        if (st.Dp == D) {
            ly.qkv = L.gemm(ask_qkv(D, D), {p + ".self_attn.linear_q.weight", p + ".self_attn.linear_k.weight", p + ".self_attn.linear_v.weight"},
                            {p + ".self_attn.linear_q.bias", p + ".self_attn.linear_k.bias", p + ".self_attn.linear_v.bias"});
            ly.out = L.gemm(ask_attn_out(D, D), {p + ".self_attn.linear_out.weight"}, {p + ".self_attn.linear_out.bias"});
        } else {      // head dim padded to a kernel size: zero rows in W_q / W_k / W_v (and their biases), zero columns in W_out
            std::vector<std::string> wn, bn;
            for (const char* t : {"q", "k", "v"}) {
                wn.push_back(L.padded_tensor(p + ".self_attn.linear_" + t + ".weight", heads, st.dk, dkp, D, D, false));
                bn.push_back(L.padded_tensor(p + ".self_attn.linear_" + t + ".bias", heads, st.dk, dkp, D, 0, false));
            }
            const std::string wo = L.padded_tensor(p + ".self_attn.linear_out.weight", heads, st.dk, dkp, D, D, true);
            if (L.rc) return;
            ly.qkv = L.gemm(ask_qkv(D, st.Dp), wn, bn);
            ly.out = L.gemm(ask_attn_out(D, st.Dp), {wo}, {p + ".self_attn.linear_out.bias"});
        }
        // (a Linear FFN hands in 2-d tensors, a Conv1d one 3-d tensors even for one tap)
        auto two_d = [&](const std::string& name) { auto it = L.m.find(name); return it != L.m.end() && it->second->ndim == 2; };
        const WeightAsk w1 = ask_ffn_w1(D, units, k, k == 1 && two_d(p + ".feed_forward.w_1.weight"));
        ly.w1 = L.gemm(w1, {p + ".feed_forward.w_1.weight"}, {p + ".feed_forward.w_1.bias"});
        ly.w2 = L.gemm(ask_ffn_w2(w1, two_d(p + ".feed_forward.w_2.weight")), {p + ".feed_forward.w_2.weight"}, {p + ".feed_forward.w_2.bias"});
        if (concat) {
            ly.cat_x = L.gemm(ask_concat_half(D, 0), {p + ".concat_linear.weight"}, {p + ".concat_linear.bias"});
            ly.cat_a = L.gemm(ask_concat_half(D, 1), {p + ".concat_linear.weight"});
        }
        ly.ln1g = L.copy(p + ".norm1.weight", {D}); ly.ln1b = L.copy(p + ".norm1.bias", {D});
        if (ly.w1.wm && ly.ln1g && ly.ln1b) {      // a-priori bound of the LayerNorm output that feeds the FFN conv
            const float gm = device_absmax(L.s, ly.ln1g, D, L.absmax_scratch), bm = device_absmax(L.s, ly.ln1b, D, L.absmax_scratch);
            const float xmax = std::sqrt((float)D) * gm + bm;
            ly.ka = fp8_scale_exponent(xmax);
            // the hidden layer's bound: l1 norms of w_1's rows (the fp32 tensor the caller handed in is still there during the load)
            if (ly.w2.wm) ly.kh = fp8_scale_exponent(device_row_l1_bound(L.s, (const float*)L.m[p + ".feed_forward.w_1.weight"]->data, ly.w1.bias, units, D * k, xmax, L.absmax_scratch));
        }
        ly.ln2g = L.copy(p + ".norm2.weight", {D}); ly.ln2b = L.copy(p + ".norm2.bias", {D});
    }
    auto it = L.m.find(pe_pre + ".pe");
    if (it == L.m.end() || it->second->ndim != 3 || it->second->shape[2] != D) {
        if (!L.rc) L.rc = fail(L.h, FS2_ERR_WEIGHT, "missing/odd positional table %s.pe", pe_pre.c_str());
        return;
    }
    st.pe_rows = (int)it->second->shape[1];
    st.pe = L.copy(pe_pre + ".pe", {1, st.pe_rows, D});
    st.alpha = scaled ? L.copy(pe_pre + ".alpha", {}) : nullptr;
}

void load_predictor(Loader& L, Predictor& p, const std::string& pre, int nlayers, int idim, int chans, int k) {
    p.conv.clear(); p.lng.clear(); p.lnb.clear();
    for (int l = 0; l < nlayers; ++l) {
        const std::string c = pre + ".conv." + std::to_string(l);
        p.conv.push_back(L.gemm(ask_predictor_conv(l == 0 ? idim : chans, chans, k), {c + ".0.weight"}, {c + ".0.bias"}));
        p.lng.push_back(L.copy(c + ".2.layer_norm.weight", {chans}));
        p.lnb.push_back(L.copy(c + ".2.layer_norm.bias", {chans}));
    }
    p.lin_w = L.copy(pre + ".linear.weight", {1, chans});
    p.lin_b = L.copy(pre + ".linear.bias", {1});
}

// Columns of tok.proj's output (fs2_handle::tokw) for this configuration, 0 where the token-level form does not exist: it needs the decoder input layer and the
// fused predictors (FusedPredictors: two layers, var_chans % 128 == 0, adim % 32 == 0) with a 3-tap first convolution (the derivation holds for any odd size; 3 is built).
// A function of the configuration alone: the token workspace reserves the rows whatever FS2_TOKPROJ says, so the option can change between calls.
inline int tok_proj_cols(const fs2_config& c) {
    const bool ok = c.decoder_input_layer && c.var_kernel == 3 && c.var_layers == 2 && c.var_chans % 128 == 0 && c.var_chans <= 1024 && c.adim % 32 == 0 &&
                    c.ddim % 32 == 0 && c.ddim <= 1024;
    return ok ? 6 * c.var_chans + c.ddim : 0;
}

// Load-time half of "multiply before expanding": the stacked weight of tok.proj and the two tables behind the input layer's weights (exact fp32 GEMMs on the device;
// the tables depend on weights only).  Needs h->Te / h->Tp / h->dec_in.
void load_tok_proj(Loader& L, fs2_handle* h) {
    const fs2_config& c = h->cfg;
    hipStream_t s = L.s;
    const int ch = c.var_chans, Nt = tok_proj_cols(c);
    const fs2_tensor_desc* wsrc[2] = {L.get("energy_predictor.predictor.conv.0.0.weight", {ch, c.adim, 3}), L.get("pitch_predictor.predictor.conv.0.0.weight", {ch, c.adim, 3})};
    const fs2_tensor_desc* win = L.get("decoder.embed.0.weight", {c.ddim, c.adim});
    if (!wsrc[0] || !wsrc[1] || !win) return;
    Loader::Synth* t = L.add_synth("tok_proj#stack", *win, (size_t)Nt * c.adim);
    if (!t) return;
    t->desc.ndim = 2; t->desc.shape[0] = Nt; t->desc.shape[1] = c.adim;
    float* stk = t->mem;
    for (int tap = 0; tap < 3; ++tap)
        for (int g = 0; g < 2; ++g)
            hipLaunchKernelGGL(conv_tap_rows, dim3((ch * c.adim + 255) / 256), dim3(256), 0, s, (const float*)wsrc[g]->data, ch, c.adim, 3, tap, stk + (size_t)(tap * 2 + g) * ch * c.adim);
    hipMemcpyAsync(stk + (size_t)6 * ch * c.adim, win->data, (size_t)c.ddim * c.adim * sizeof(float), hipMemcpyDeviceToDevice, s);
    h->tokw = L.gemm(ask_tok_proj(c.adim, Nt), {t->name});
    h->TPd = L.dalloc((size_t)c.n_bins * c.ddim);
    h->TEd = L.dalloc((size_t)c.n_bins * c.ddim);
    if (L.rc || !h->TPd || !h->TEd || !h->Te || !h->Tp) { h->tokw = Gemm(); return; }
    for (int t = 0; t < 2; ++t) {      // TPd carries the input layer's bias
        GemmArgs a = gemm_args(h->dec_in, t ? h->Te : h->Tp, c.adim, c.n_bins, nullptr, t ? h->TEd : h->TPd, c.ddim);
        if (t) a.bias = nullptr;
        const int rc = launch_gemm(nullptr, s, t ? "load.TEd" : "load.TPd", a, FS2_PREC_FP32);
        if (rc && !L.rc) L.rc = fail(h, rc, "%s", g_create_error.c_str());
    }
}

void free_weights(fs2_handle* h) {
    for (void* p : h->allocs) hipFree(p);
    h->allocs.clear();
    h->loaded = false;
}

struct TokenBufs {
    int* meta; StackBufs sb; float *p0, *p1, *dlog_rows; int64_t* dint; int *cum, *o32;
    float* kp; size_t kp_cap;
    float* tokp;      // tok.proj's output rows (nullptr: this model or precision has none)
    // the duration scan of the short durations (FS2_VARSHORT), in p0 / p1: the duration predictor's scratch is free once dur.post has run, and nothing of the
    // workspace may grow (tests: the recorded sizes).  short_buf: they fit
    int *scum, *so32; bool short_buf;
};

// The buffers of an FFT-block stack, x0 to xps: contiguous and in this order in both workspaces.  D: the stack's width, Dp: its attention width; hid, x0p, x1p, xps:
// floats per row of those buffers (what else they hold: at the callers).
void carve_stack(Bump& bp, size_t R, size_t D, size_t Dp, size_t hid, size_t x0p, size_t x1p, size_t xps, StackBufs& sb) {
    sb.x0 = bp.take<float>(R * D);
    sb.x1 = bp.take<float>(R * D);
    sb.qkv = bp.take<float>(R * 3 * Dp);
    sb.ctx = bp.take<float>(R * Dp);
    sb.hid = bp.take<float>(R * hid);
    sb.qkh = bp.take<__bf16>(R * 2 * Dp);
    sb.qkl = bp.take<__bf16>(R * 2 * Dp);
    sb.vth = bp.take<__bf16>(R * Dp);
    sb.vtl = bp.take<__bf16>(R * Dp);
    sb.x0p = bp.take<float>(R * x0p);
    sb.x1p = bp.take<float>(R * x1p);
    sb.xps = bp.take<float>(R * xps);
}

// carve the token workspace; if ws == nullptr only sizes it
size_t carve_tokens(const fs2_config& c, const fs2_batch& b, const HostLayout& L, void* ws, size_t cap, TokenBufs* tb, bool* ok) {
    Bump bp(ws, cap);
    const size_t R = L.Rpad;
    TokenBufs t;
    t.meta = bp.take<int>(layout_dev_ints(L));
    const size_t pw = round_up(c.adim, 32);
    // (attention width: heads x padded head dim; bf16 modes: the hidden layer as planes, 32-channel chunks)
    carve_stack(bp, R, c.adim, att_width(c.adim, c.aheads), round_up(c.eunits, 32), pw, pw, round_up(std::max(c.adim, c.dur_chans), 32), t.sb);
    t.p0 = bp.take<float>(R * c.dur_chans);
    t.p1 = bp.take<float>(R * c.dur_chans);
    t.dlog_rows = bp.take<float>(R);
    t.dint = bp.take<int64_t>((size_t)b.B * b.Tmax);
    t.cum = bp.take<int>((size_t)b.B * b.Tmax);
    t.o32 = bp.take<int>(b.B);
    t.kp_cap = kpart_floats(R);
    t.kp = bp.take<float>(t.kp_cap);
    // tok.proj's output rows (taken last: every other offset is as it was; none in fp32, which never takes the path)
    t.tokp = (tok_proj_cols(c) && b.precision != FS2_PREC_FP32) ? bp.take<float>(R * (size_t)tok_proj_cols(c)) : nullptr;
    t.scum = reinterpret_cast<int*>(t.p0); t.so32 = reinterpret_cast<int*>(t.p1);
    t.short_buf = (size_t)b.B * b.Tmax <= R * (size_t)c.dur_chans && (size_t)b.B <= R * (size_t)c.dur_chans;
    if (tb) *tb = t;
    if (ok) *ok = bp.ok();
    return align_up(bp.off, 256);
}

struct FrameBufs {
    int* meta; float* hfr; float *t0, *t1, *e_rows, *p_rows; StackBufs sb; float *before, *after; int *qe, *qp, *lri;
    float *vp = nullptr, *vs = nullptr;      // fused pitch + energy predictors: planes of the stacked hidden layer [R][2 chans], fp32 scratch [R, 2 chans]
    float* kp; size_t kp_cap;
    // reduction_factor r > 1: the Postnet runs on r rows per decoder row (its own row metadata and ping-pong buffers)
    int* meta2 = nullptr; float *pa2 = nullptr, *pb2 = nullptr, *xps2 = nullptr;
    // FS2_VARSHORT: the short layout (varshort.h: sstart | slen of B, sdims of kDimsInts; per short row position, utterance, token), the frame-to-short map
    // and the bucket indices per short row.  The short rows are never more than the frame rows: every array holds Rpad.  They live in hfr -- the path runs where
    // nothing reads the expanded rows (tokproj == 3), so they are not built -- because nothing of the workspace may grow (tests: the recorded sizes); the
    // predictions per short row take e_rows / p_rows, which then hold nothing else.  short_buf: they fit
    int *smeta = nullptr, *srow_pos = nullptr, *srow_seq = nullptr, *slri = nullptr, *f2s = nullptr, *sqe = nullptr, *sqp = nullptr;
    bool short_buf = false;
};

size_t carve_frames(const fs2_config& c, const HostLayout& L, void* ws, size_t cap, FrameBufs* fb, bool* ok) {
    Bump bp(ws, cap);
    const size_t R = L.Rpad;
    FrameBufs f;
    f.meta = bp.take<int>(layout_dev_ints(L));
    f.hfr = bp.take<float>(R * c.adim);
    {
        Bump sh(f.hfr, R * c.adim * sizeof(float));
        f.smeta = sh.take<int>((size_t)meta_align(2 * (long long)L.B) + kDimsInts);
        f.srow_pos = sh.take<int>(R); f.srow_seq = sh.take<int>(R); f.slri = sh.take<int>(R); f.f2s = sh.take<int>(R);
        f.sqe = sh.take<int>(R); f.sqp = sh.take<int>(R);
        f.short_buf = sh.ok();
    }
    f.t0 = bp.take<float>(R * c.var_chans);
    f.t1 = bp.take<float>(R * c.var_chans);
    f.e_rows = bp.take<float>(R);
    f.p_rows = bp.take<float>(R);
    f.vp = bp.take<float>(R * 2 * (size_t)c.var_chans);
    f.vs = bp.take<float>(R * 2 * (size_t)c.var_chans);
    // (hid: also the Postnet's ping-pong rows; x0p / x1p: also the Postnet's planes, x1p the length-regulator output's too; xps: of every launch that builds its planes)
    carve_stack(bp, R, c.ddim, att_width(c.ddim, c.aheads), std::max(round_up(c.dunits, 32), 2 * c.postnet_chans), round_up(std::max(c.ddim, c.postnet_chans), 32),
                round_up(std::max(std::max(c.adim, c.ddim), c.postnet_chans), 32), round_up(std::max(std::max(c.adim, c.ddim), std::max(std::max(c.var_chans, c.postnet_chans), c.odim)), 32), f.sb);
    f.sb.xs4 = bp.take<unsigned char>(R * 32 + 64);      // mx4: one scale byte per (row, 16-channel slot of a cross unit), 32 per row
    const size_t rf = (size_t)std::max(c.reduction_factor, 1);
    f.before = bp.take<float>(R * rf * c.odim);
    f.after = bp.take<float>(R * rf * c.odim);
    if (rf > 1) {
        f.meta2 = bp.take<int>((size_t)Meta2::ints(L.B, R * rf));
        f.pa2 = bp.take<float>(R * rf * c.postnet_chans);
        f.pb2 = bp.take<float>(R * rf * c.postnet_chans);
        f.xps2 = bp.take<float>(R * rf * (size_t)round_up(std::max(c.postnet_chans, c.odim), 32));
    }
    f.qe = bp.take<int>(R);
    f.qp = bp.take<int>(R);
    f.lri = bp.take<int>(R);
    f.kp_cap = kpart_floats(R);
    f.kp = bp.take<float>(f.kp_cap);
    if (fb) *fb = f;
    if (ok) *ok = bp.ok();
    return align_up(bp.off, 256);
}

template <typename T>
int unpack(fs2_handle* h, hipStream_t s, const T* src, int W, const int* start, const int* limit, int B, int Lout, T* dst, T fill, const int* ovf = nullptr) {
    const int64_t total = (int64_t)B * Lout * W;
    if (total == 0) return FS2_OK;
    if constexpr (std::is_same<T, float>::value) {
        if (fill == 0.f && unpack_vec(W, src, dst)) {      // (looks at the overflow flags itself: call_plan.h)
            hipLaunchKernelGGL(unpack_rows4, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, src, W / 4, start, limit, B, Lout, dst, ovf);
            HIP_TRY(h, hipGetLastError());
            return FS2_OK;
        }
    }
    hipLaunchKernelGGL(unpack_rows<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, W, start, limit, B, Lout, dst, fill);
    HIP_TRY(h, hipGetLastError());
    return FS2_OK;
}


// ---------------------------------------------------------------------------------- vocoder (griffin_lim.h)
#include "griffin_lim_host.h"

// ---------------------------------------------------------------------------------- training targets (kernels and host side)
#include "targets.h"

// ---------------------------------------------------------------------------------- loss terms of the teacher-forced forward
#include "losses.h"

// ---------------------------------------------------------------------------------- DTW distance of the free-running validation
#include "dtw.h"

// ---------------------------------------------------------------------------------- forced alignment: phoneme durations of a recording
#include "align.h"

// ---------------------------------------------------------------------------------- pitch path search over per-frame candidates
#include "pitch_path.h"

// ---------------------------------------------------------------------------------- pitch / energy control, per-phoneme means
#include "prosody.h"

// ------------------------------------------------------------------ pieces of fs2_decode (call_plan.h: DecodePlan says which of them run)
// (behind the operator headers: decode_outputs is the first to instantiate unpack<T>, and the kernels of the code object stand in the order of first instantiation)
// what var.gather0 and dec.in.gather share: the token-level products and the frame rows that gather them
TokGatherArgs tok_gather_args(const fs2_handle* h, const FrameBufs& f, const DevLayout& dl, int R) {
    TokGatherArgs tg;
    memset(&tg, 0, sizeof tg);
    tg.P = h->left.tokP; tg.ldp = h->tokw.N; tg.tok_start = h->left.start; tg.lri = f.lri; tg.row_pos = dl.row_pos; tg.row_seq = dl.row_seq; tg.R = R;
    tg.chans = h->cfg.var_chans; tg.bias = h->var2.c0.bias; tg.ln_g = h->var2.ln0g; tg.ln_b = h->var2.ln0b; tg.vp = f.vp;
    return tg;
}

// dec.in.gather's block: the frame rows of tok_gather_args plus the tables of the variance adaptor's tail and of the decoder input layer; p.varshort: the frame-to-short
// map and, where the predictions are the source, the short rows whose buckets var_bucket_short searches first (dec_in_gather_launch)
TokGatherArgs dec_in_gather_args(const fs2_handle* h, const fs2_decode_io* io, TokGatherArgs tg, const FrameBufs& f, const DecodePlan& p, int Rs) {
    const fs2_config& c = h->cfg;
    tg.col0 = 6 * c.var_chans; tg.D = c.ddim; tg.es = io->es; tg.ps = io->ps; tg.es_stride = io->es_stride; tg.ps_stride = io->ps_stride;
    tg.e_rows = f.e_rows; tg.p_rows = f.p_rows; tg.ebins = h->ebins; tg.pbins = h->pbins; tg.nb = c.n_bins - 1; tg.TE = h->TEd; tg.TP = h->TPd;
    tg.qe_rows = f.qe; tg.qp_rows = f.qp; tg.ln_g2 = h->dec_in_lng; tg.ln_b2 = h->dec_in_lnb;
    tg.pe = h->dec.pe; tg.pe_alpha = h->dec.alpha; tg.x_scale = c.use_scaled_pos_enc ? 1.f : sqrtf((float)c.ddim);
    tg.x0 = p.po ? nullptr : f.sb.x0; tg.x0p = f.sb.x0p;
    if (p.varshort) {
        tg.f2s = f.f2s; tg.sqe = p.short_qe ? f.sqe : nullptr; tg.sqp = p.short_qp ? f.sqp : nullptr;
        tg.srow_pos = f.srow_pos; tg.Rs = Rs;
    }
    return tg;
}

// dec.in.pe, the TorchScript twin: the decoder input is just x (* sqrt(d)) + alpha * pe   (encoder.py:138-141)
int dec_in_pe_launch(fs2_handle* h, hipStream_t s, const FrameBufs& f, const DevLayout& dl, int R, bool planes) {
    const fs2_config& c = h->cfg;
    Scope sc(h, s, "dec.in.pe", 0.0, 8.0 * R * c.ddim);
    HIP_TRY(h, hipMemcpyAsync(f.sb.x0, f.hfr, (size_t)R * c.ddim * sizeof(float), hipMemcpyDeviceToDevice, s));
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.N = c.ddim; a.R = R; a.row_pos = dl.row_pos; a.Y = f.sb.x0; a.ldy = c.ddim;
    a.pe = h->dec.pe; a.pe_ld = c.ddim; a.pe_alpha = h->dec.alpha; a.x_scale = c.use_scaled_pos_enc ? 1.f : sqrtf((float)c.ddim);
    if (planes) { a.Yp = f.sb.x0p; a.yp_chunks = c.ddim / 32; }
    hipLaunchKernelGGL(ln_rows, dim3((R + 3) / 4), dim3(256), 0, s, a);
    HIP_TRY(h, hipGetLastError());
    return FS2_OK;
}

// reduction_factor r (reference fastspeech.py:153,228-230): feat_out emits r mel frames per decoder frame; its [R, odim r] output
// IS the [R r, odim] row image the Postnet runs on (decoder row i -> rows i r .. i r + r - 1, gap rows stay zero rows), so only the
// row metadata is rebuilt at the finer rate.  r = 1 uses the decoder's own metadata and buffers.
int mel_layout(fs2_handle* h, hipStream_t s, const FrameBufs& f, const DevLayout& dl, int B, int Rpad, int rf, DevLayout& dl2) {
    dl2 = dl;
    if (rf == 1) return FS2_OK;
    const int Rpad2 = Rpad * rf;
    const Meta2 m = Meta2::at(B, Rpad2);
    dl2.start = f.meta2 + m.start; dl2.len = f.meta2 + m.len; dl2.vlen = f.meta2 + m.vlen; dl2.klen = dl2.len;
    dl2.dims = dl.dims ? f.meta2 + m.dims : nullptr;
    dl2.row_pos = f.meta2 + m.row_pos; dl2.row_seq = f.meta2 + m.row_seq;
    hipLaunchKernelGGL(scale_layout, dim3((B + 255) / 256), dim3(256), 0, s, dl.start, dl.len, dl.vlen, dl.dims, B, rf, dl2.start, dl2.len, dl2.vlen, dl2.dims);
    hipLaunchKernelGGL(build_row_meta, dim3((Rpad2 + 255) / 256), dim3(256), 0, s, dl2.start, dl2.len, B, Rpad2, dl2.row_pos, dl2.row_seq);
    HIP_TRY(h, hipGetLastError());
    return FS2_OK;
}

// The outputs of fs2_decode, all under the profile name "unpack": the packed rows to the caller's padded [B, Lmax] buffers, the mel also back to back
// (after_packed), and in the device-driven layout NaN over the mel outputs whose writer does not look at the overflow flags itself (p.poison_*).
// dl2 / mel_after: the layout and the rows of the final mel (mel outputs hold Lmax * reduction_factor frames per utterance).
int decode_outputs(fs2_handle* h, hipStream_t s, const fs2_decode_io* io, const DecodePlan& p, const FrameBufs& f, const DevLayout& dl, const DevLayout& dl2, int R, const float* mel_after) {
    const fs2_config& c = h->cfg;
    const int B = io->batch.B, Lmax = io->Lmax, rf = p.rf;
    int rc;
    Scope sc(h, s, "unpack", 0, 4.0 * R * c.odim * 4);
    const int* lim_len = dl.len;    // every stored row (pads carry real values in compat mode)
    const int* lim_msk = p.ep_stored ? dl.len : dl.vlen;
    const int* ovf = p.devlay ? dl.dims + 2 : nullptr;
    if (io->after && (rc = unpack<float>(h, s, mel_after, c.odim, dl2.start, dl2.len, B, Lmax * rf, io->after, 0.f, ovf))) return rc;
    if (io->before && (rc = unpack<float>(h, s, f.before, c.odim, dl2.start, dl2.len, B, Lmax * rf, io->before, 0.f, ovf))) return rc;
    if (p.varshort) {      // the predictions exist per short row: expanded through the frame-to-short map, and only here, where a caller asks for them
        for (int k = 0; k < 2; ++k) {
            float* dst = k ? io->p_out : io->e_out;
            if (!dst || (int64_t)B * Lmax == 0) continue;
            hipLaunchKernelGGL(unpack_short, dim3((unsigned)(((int64_t)B * Lmax + 255) / 256)), dim3(256), 0, s, k ? f.p_rows : f.e_rows, f.f2s, dl.start, lim_msk, B, Lmax, dst);
            HIP_TRY(h, hipGetLastError());
        }
    } else {
        if (io->e_out && (rc = unpack<float>(h, s, f.e_rows, 1, dl.start, lim_msk, B, Lmax, io->e_out, 0.f))) return rc;
        if (io->p_out && (rc = unpack<float>(h, s, f.p_rows, 1, dl.start, lim_msk, B, Lmax, io->p_out, 0.f))) return rc;
    }
    if (io->qe && (rc = unpack<int>(h, s, f.qe, 1, dl.start, lim_len, B, Lmax, io->qe, -1))) return rc;
    if (io->qp && (rc = unpack<int>(h, s, f.qp, 1, dl.start, lim_len, B, Lmax, io->qp, -1))) return rc;
    if (io->lr_index && (rc = unpack<int>(h, s, f.lri, 1, dl.start, dl.vlen, B, Lmax, io->lr_index, -1))) return rc;
    if (io->dec_out && (rc = unpack<float>(h, s, f.sb.x0, c.ddim, dl.start, lim_len, B, Lmax, io->dec_out, 0.f))) return rc;
    if (io->after_packed) {
        if (c.odim % 4) return fail(h, FS2_ERR_UNSUPPORTED, "after_packed needs odim %% 4 == 0");
        const int* dcum;
        if (p.devlay) {
            dcum = dl.pcum;      // built by frame_layout_dev; the caller's buffer holds row_capacity rows (>= the frames)
        } else {
            std::vector<int> cum(B);
            int run = 0;
            for (int i = 0; i < B; ++i) { cum[i] = run; run += (int)io->olens[i]; }
            int* up = f.qe;    // the bucket-index rows are already unpacked: reuse their storage for the offsets
            HIP_TRY(h, hipMemcpyAsync(up, cum.data(), cum.size() * sizeof(int), hipMemcpyHostToDevice, s));
            dcum = up;
        }
        // (r > 1: the rows are mel frames -- the Postnet's layout dl2, r rows per decoder row -- and the offsets r times the decoder-frame sums)
        const int R2 = R * rf;
        const int64_t n = (int64_t)R2 * (c.odim / 4);
        hipLaunchKernelGGL(pack_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mel_after, c.odim, dl2.row_pos, dl2.row_seq, dl2.vlen, dcum, R2, io->after_packed,
                           p.packed_ovf ? ovf : (const int*)nullptr, rf);
        HIP_TRY(h, hipGetLastError());
    }
    if (p.poison()) {
        const int64_t mel = (int64_t)B * Lmax * rf * c.odim;
        hipLaunchKernelGGL(poison_on_overflow, dim3(256), dim3(256), 0, s, dl.dims, io->after, p.poison_after ? mel : (int64_t)0, io->after_packed,
                           p.poison_packed ? io->row_capacity * rf * c.odim : (int64_t)0, io->before, p.poison_before ? mel : (int64_t)0);
        HIP_TRY(h, hipGetLastError());
    }
    return FS2_OK;
}

}  // namespace

// =====================================================================================================
extern "C" {

int32_t fs2_abi_version(void) { return FS2_ABI_VERSION; }

// every caller-filled struct starts with its own sizeof as the caller's header saw it: a binding built against another revision
// of include/fs2.h is refused here instead of having its fields read at the wrong offsets
#define ABI_CHECK(h, what, ptr, type)                                                                                         \
    do {                                                                                                                      \
        if ((ptr)->struct_size != (uint32_t)sizeof(type))                                                                     \
            return fail(h, FS2_ERR_ARG, FS2_STRUCT_SIZE_FMT, what, #type, (unsigned)(ptr)->struct_size, FS2_ABI_VERSION,         \
                        sizeof(type)); /* (the wording of record_op.h's rec_check_struct) */                                  \
    } while (0)

int fs2_create(const fs2_config* cfg, fs2_handle** out) {
    if (!cfg || !out) return fail(nullptr, FS2_ERR_ARG, "fs2_create: null argument");
    *out = nullptr;
    ABI_CHECK(nullptr, "fs2_create", cfg, fs2_config);
    if (cfg->reduction_factor < 1 || cfg->reduction_factor > 8) return fail(nullptr, FS2_ERR_UNSUPPORTED, "reduction_factor %d outside [1, 8]", cfg->reduction_factor);
    if (cfg->aheads <= 0 || cfg->adim % cfg->aheads || cfg->ddim % cfg->aheads) return fail(nullptr, FS2_ERR_ARG, "adim/ddim not divisible by aheads");
    if (!padded_head_dim(cfg->adim / cfg->aheads) || !padded_head_dim(cfg->ddim / cfg->aheads))
        return fail(nullptr, FS2_ERR_UNSUPPORTED, "attention head dims above 256 (adim / aheads = %d, ddim / aheads = %d) are not implemented", cfg->adim / cfg->aheads, cfg->ddim / cfg->aheads);
    if (!cfg->decoder_input_layer && cfg->ddim != cfg->adim) return fail(nullptr, FS2_ERR_ARG, "decoder_input_layer = 0 needs ddim == adim");
    if (cfg->n_bins != cfg->adim) return fail(nullptr, FS2_ERR_ARG, "n_bins (%d) must equal adim (%d): the reference feeds one_hot(256) into Linear(adim, adim)", cfg->n_bins, cfg->adim);
    if (cfg->ffn_kernel % 2 == 0 || cfg->dur_kernel % 2 == 0 || cfg->var_kernel % 2 == 0 || (cfg->postnet_layers > 0 && cfg->postnet_filts % 2 == 0))
        return fail(nullptr, FS2_ERR_UNSUPPORTED, "even convolution kernel sizes are not supported");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, FS2_ERR_HIP, "no HIP device is visible: libfs2_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, FS2_ERR_ARG, "device %d out of range (%d visible)", cfg->device, ndev);
    {
        DeviceGuard g(cfg->device);      // only proves the device can be made current; the caller's current device is restored
        if (g.err != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(g.err));
    }
    fs2_handle* h = new fs2_handle();
    h->cfg = *cfg;
    {
        DeviceGuard g(cfg->device);
        if (hipMalloc((void**)&h->counters, 16 * sizeof(int)) != hipSuccess || hipMemset(h->counters, 0, 16 * sizeof(int)) != hipSuccess) {
            delete h;
            return fail(nullptr, FS2_ERR_HIP, "hipMalloc of the handle's counters failed");
        }
    }
    {   // zero rows between packed utterances: the largest conv halo of this model (launch_gemm refuses kernels > kMaxHalo + 1 taps)
        int p = std::max(std::max(cfg->ffn_kernel, cfg->dur_kernel), cfg->var_kernel);
        if (cfg->postnet_layers > 0) p = std::max(p, cfg->postnet_filts);
        h->gap = std::min(kGap, std::max(kMinGap, (p - 1) / 2));
    }
    *out = h;
    return FS2_OK;
}

void fs2_destroy(fs2_handle* h) {
    if (!h) return;
    DeviceGuard g(h->cfg.device);
    free_weights(h);
    if (h->counters) hipFree(h->counters);
    for (auto& r : h->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (void* p : h->graph_pinned) hipHostFree(p);
    delete h;
}

const char* fs2_last_error(const fs2_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fs2_load_weights(fs2_handle* h, const fs2_tensor_desc* t, int32_t n, void* stream) {
    if (!h || !t || n <= 0) return fail(h, FS2_ERR_ARG, "fs2_load_weights: bad arguments");
    DeviceGuard g(h->cfg.device);
    HIP_TRY(h, g.err);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipStreamSynchronize(s));   // nothing may still be reading the old weights
    free_weights(h);
    h->left = Encoded();
    const fs2_config& c = h->cfg;
    Loader L{h, s, {}, FS2_OK};
    for (int i = 0; i < n; ++i) if (t[i].name) L.m[t[i].name] = &t[i];

    h->enc_embed = L.copy("encoder.embed.0.weight", {c.idim, c.adim});
    load_stack(L, h->enc, "encoder", c.elayers, c.adim, c.aheads, c.eunits, c.ffn_kernel, "encoder.embed.1", c.use_scaled_pos_enc,
               c.enc_normalize_before != 0, c.enc_concat_after != 0);
    load_stack(L, h->dec, "decoder", c.dlayers, c.ddim, c.aheads, c.dunits, c.ffn_kernel, c.decoder_input_layer ? "decoder.embed.4" : "decoder.embed.0",
               c.use_scaled_pos_enc, c.dec_normalize_before != 0, c.dec_concat_after != 0);
    load_predictor(L, h->dur, "duration_predictor", c.dur_layers, c.adim, c.dur_chans, c.dur_kernel);
    load_predictor(L, h->energy, "energy_predictor.predictor", c.var_layers, c.adim, c.var_chans, c.var_kernel);
    load_predictor(L, h->pitch, "pitch_predictor.predictor", c.var_layers, c.adim, c.var_chans, c.var_kernel);
    h->var2 = FusedPredictors();
    if (c.var_layers == 2 && c.var_chans % 128 == 0 && c.adim % 32 == 0) {
        const std::string e = "energy_predictor.predictor", q = "pitch_predictor.predictor";
        FusedPredictors& v = h->var2;
        v.c0 = L.gemm(ask_fused_predictor_conv(c.adim, c.var_chans, c.var_kernel), {e + ".conv.0.0.weight", q + ".conv.0.0.weight"}, {e + ".conv.0.0.bias", q + ".conv.0.0.bias"});
        v.c1 = L.gemm(ask_fused_predictor_conv(c.var_chans, c.var_chans, c.var_kernel), {e + ".conv.1.0.weight", q + ".conv.1.0.weight"}, {e + ".conv.1.0.bias", q + ".conv.1.0.bias"});
        v.ln0g = L.copy2(e + ".conv.0.2.layer_norm.weight", q + ".conv.0.2.layer_norm.weight", {c.var_chans});
        v.ln0b = L.copy2(e + ".conv.0.2.layer_norm.bias", q + ".conv.0.2.layer_norm.bias", {c.var_chans});
        v.ln1g = L.copy2(e + ".conv.1.2.layer_norm.weight", q + ".conv.1.2.layer_norm.weight", {c.var_chans});
        v.ln1b = L.copy2(e + ".conv.1.2.layer_norm.bias", q + ".conv.1.2.layer_norm.bias", {c.var_chans});
        v.lin_w = L.copy2(e + ".linear.weight", q + ".linear.weight", {1, c.var_chans});
        v.lin_b = L.copy2(e + ".linear.bias", q + ".linear.bias", {1});
        v.ok = !L.rc;
    }
    h->ebins = L.copy("energy_predictor.energy_bins", {c.n_bins - 1});
    h->pbins = L.copy("pitch_predictor.pitch_bins", {c.n_bins - 1});
    h->Te = L.dalloc((size_t)c.n_bins * c.adim);
    h->Tp = L.dalloc((size_t)c.n_bins * c.adim);
    {
        const fs2_tensor_desc *we = L.get("energy_embed.weight", {c.adim, c.n_bins}), *be = L.get("energy_embed.bias", {c.adim});
        const fs2_tensor_desc *wp = L.get("pitch_embed.weight", {c.adim, c.n_bins}), *bp = L.get("pitch_embed.bias", {c.adim});
        if (we && be && wp && bp && h->Te && h->Tp) {
            const int tot = c.adim * c.n_bins;
            hipLaunchKernelGGL(onehot_table, dim3((tot + 255) / 256), dim3(256), 0, s, (const float*)we->data, (const float*)be->data, c.adim, c.n_bins, h->Te);
            hipLaunchKernelGGL(onehot_table, dim3((tot + 255) / 256), dim3(256), 0, s, (const float*)wp->data, (const float*)bp->data, c.adim, c.n_bins, h->Tp);
        }
    }
    if (c.decoder_input_layer) {
        h->dec_in = L.gemm(ask_dec_in(c.adim, c.ddim), {"decoder.embed.0.weight"}, {"decoder.embed.0.bias"});
        h->dec_in_lng = L.copy("decoder.embed.1.weight", {c.ddim});
        h->dec_in_lnb = L.copy("decoder.embed.1.bias", {c.ddim});
    }
    h->tokw = Gemm(); h->TEd = h->TPd = nullptr;
    if (tok_proj_cols(c) && h->var2.ok && !L.rc) load_tok_proj(L, h);
    h->feat = L.gemm(ask_feat_out(c.ddim, c.odim * std::max(c.reduction_factor, 1)), {"feat_out.weight"}, {"feat_out.bias"});
    h->post.clear();
    for (int l = 0; l < c.postnet_layers; ++l) {
        const std::string p = "postnet.postnet." + std::to_string(l);
        const int ic = (l == 0) ? c.odim : c.postnet_chans;
        const int oc = (l == c.postnet_layers - 1) ? c.odim : c.postnet_chans;
        h->post.push_back(L.gemm(ask_postnet(ic, oc, c.postnet_filts, c.use_batch_norm != 0), {p + ".0.weight"}, {}, p + ".1"));
    }
    if (L.rc) { free_weights(h); return L.rc; }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));   // source tensors may be released by the caller after return
    h->loaded = true;
    return FS2_OK;
}

int fs2_set_profiling(fs2_handle* h, int32_t on) {
    if (!h) return FS2_ERR_ARG;
    h->prof = on != 0;
    for (auto& r : h->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    h->recs.clear();
    return FS2_OK;
}

int fs2_set_profile_filter(fs2_handle* h, const char* name) {
    if (!h) return FS2_ERR_ARG;
    h->prof_filter = name ? name : "";
    return FS2_OK;
}

int fs2_get_profile(fs2_handle* h, const char** names, float* ms, double* flops, double* bytes, int32_t cap) {
    if (!h) return FS2_ERR_ARG;
    int n = 0;
    for (auto& r : h->recs) {
        if (n >= cap) break;
        hipEventSynchronize(r.e1);
        float t = 0.f;
        hipEventElapsedTime(&t, r.e0, r.e1);
        if (names) names[n] = r.name.c_str();
        if (ms) ms[n] = t;
        if (flops) flops[n] = r.flops;
        if (bytes) bytes[n] = r.bytes;
        ++n;
    }
    return n;
}

size_t fs2_token_workspace_bytes(const fs2_handle* h, const fs2_batch* b) {
    if (!h || !b || b->B <= 0 || !b->ilens) return 0;
    HostLayout L;
    token_layout(*b, L, h->gap);
    return carve_tokens(h->cfg, *b, L, nullptr, 0, nullptr, nullptr);
}

// Four steps: checks, layout and carve, plan, then the launches, which branch on the plan's fields only.
int fs2_encode(fs2_handle* h, void* stream, const fs2_encode_io* io) {
    if (!h || !io) return fail(h, FS2_ERR_ARG, "fs2_encode: null argument");
    ABI_CHECK(h, "fs2_encode", io, fs2_encode_io);
    if (!h->loaded) return fail(h, FS2_ERR_STATE, "fs2_encode: weights not loaded");
    if (const Refusal r = check_encode(*io, h->enc.pe_rows); r.err) return fail(h, r.err, "%s", r.msg);
    DeviceGuard g(h->cfg.device);
    HIP_TRY(h, g.err);
    hipStream_t s = (hipStream_t)stream;
    const fs2_config& c = h->cfg;
    const fs2_batch& b = io->batch;
    h->left = Encoded();
    token_layout(b, h->tok, h->gap);
    const HostLayout& L = h->tok;
    TokenBufs t; bool ok;
    carve_tokens(c, b, L, io->workspace, io->workspace_bytes, &t, &ok);
    if (!ok) return fail(h, FS2_ERR_WORKSPACE, "fs2_encode: workspace too small");
    h->kp = t.kp; h->kp_cap = t.kp_cap;
    const StackBufs& sb = t.sb;
    const int tok_regime = regime_rows_of(b, /*token_level=*/true);
    h->cur_regime = tok_regime; h->cur_status = nullptr;
    const EncodePlan p = plan_encode(c, opts(), b.precision, h->tokw.N, t.tokp != nullptr, t.short_buf && !b.compat_padded);
    int rc;
    DevLayout dl;
    if ((rc = upload_layout(h, s, L, t.meta, dl))) return rc;
    RowStepArgs ra;      // enc.embed and dur.post on the token rows
    memset(&ra, 0, sizeof ra);
    ra.row_pos = dl.row_pos; ra.row_seq = dl.row_seq; ra.R = L.R; ra.start = dl.start; ra.vlen = dl.vlen; ra.B = b.B; ra.Tmax = b.Tmax; ra.D = c.adim;
    ra.rows = sb.x0; ra.planes = p.embed_planes ? sb.x0p : nullptr;
    ra.xs = io->xs; ra.E = h->enc_embed; ra.idim = c.idim; ra.pe = h->enc.pe; ra.pe_alpha = h->enc.alpha; ra.x_scale = c.use_scaled_pos_enc ? 1.0f : sqrtf((float)c.adim);
    ra.dlog_rows = t.dlog_rows; ra.d_log = io->d_log; ra.d_int = t.dint; ra.d_int2 = io->d_int; ra.ds = io->ds; ra.cum = t.cum; ra.olens = io->olens; ra.olens32 = t.o32;
    ra.alpha = io->duration_alpha > 0.f ? io->duration_alpha : 1.f; ra.scum = p.short_scan ? t.scum : nullptr; ra.so32 = p.short_scan ? t.so32 : nullptr; ra.K = var_window(c);
    if ((rc = embed_launch(h, s, ra))) return rc;
    const Rows rows{L.R, L.Rpad, dl.row_pos, dl.dims, tok_regime};
    if ((rc = run_stack(h, s, "enc", h->enc, c.adim, c.aheads, rows, L, dl, /*mask_q=*/1, sb, p.prec, /*x0p_ready=*/p.embed_planes, p.ffn_terms))) return rc;
    if ((rc = run_predictor(h, s, "dur", h->dur, sb.x0, c.adim, rows, t.p0, t.p1, t.dlog_rows, p.prec, p.planes ? sb.x0p : nullptr, sb.xps))) return rc;
    if ((rc = dur_post_launch(h, s, ra))) return rc;
    if (io->enc_out) {
        if ((rc = unpack<float>(h, s, sb.x0, c.adim, dl.start, dl.vlen, b.B, b.Tmax, io->enc_out, 0.f))) return rc;
    }
    if (p.tok_proj) {      // (call_plan.h: EncodePlan)
        if ((rc = launch_step(h, s, nullptr, tok_proj_step(h->tokw, p.tok_n0, sb.x0, c.adim, rows, sb.x0p, sb.xps, t.tokp, h->kp), p.tok_prec))) return rc;
    }
    Encoded& e = h->left;
    e.B = b.B; e.Tmax = b.Tmax; e.compat = b.compat_padded; e.ws = io->workspace;
    e.rows = sb.x0; e.tokP = p.tok_proj ? t.tokp : nullptr; e.tokP_conv = p.tok_conv;
    e.start = dl.start; e.vlen = dl.vlen; e.cum = t.cum; e.o32 = t.o32;
    if (p.short_scan) { e.scum = t.scum; e.so32 = t.so32; }
    e.valid = true;
    return FS2_OK;
}

size_t fs2_frame_workspace_bytes(const fs2_handle* h, const fs2_batch* b, const int64_t* olens) {
    if (!h || !b || !olens || b->B <= 0) return 0;
    HostLayout L;
    frame_layout(*b, olens, 0, L, h->gap);
    return carve_frames(h->cfg, L, nullptr, 0, nullptr, nullptr);
}

// device-driven layout: every utterance start is rounded up to kAttAlign rows and followed by kGap zero rows
int64_t fs2_row_capacity(const fs2_batch* b, int64_t total_frames_bound) {
    if (!b || b->B <= 0 || total_frames_bound <= 0) return 0;
    return rows_padded(row_bound(total_frames_bound, b->B));
}

size_t fs2_frame_workspace_bytes_cap(const fs2_handle* h, const fs2_batch* b, int64_t row_capacity, int32_t lmax_cap) {
    if (!h || !b || b->B <= 0 || row_capacity <= 0 || row_capacity > INT32_MAX - 256 || lmax_cap <= 0) return 0;
    HostLayout L;
    capacity_layout(*b, row_capacity, lmax_cap, L);
    return carve_frames(h->cfg, L, nullptr, 0, nullptr, nullptr);
}

int fs2_decode(fs2_handle* h, void* stream, const fs2_decode_io* io) { return fs2_decode_ctl(h, stream, io, nullptr); }

int fs2_decode_ctl(fs2_handle* h, void* stream, const fs2_decode_io* io, const fs2_prosody* ctl) {
    if (!h || !io) return fail(h, FS2_ERR_ARG, "fs2_decode: null argument");
    ABI_CHECK(h, "fs2_decode", io, fs2_decode_io);
    if (ctl) ABI_CHECK(h, "fs2_decode_ctl", ctl, fs2_prosody);
    if (const Refusal r = check_decode(*io, ctl, h->left, h->cfg.idim, h->dec.pe_rows); r.err) return fail(h, r.err, "%s", r.msg);
    const fs2_config& c = h->cfg;
    const fs2_batch& b = io->batch;
    const Encoded& enc = h->left;
    DeviceGuard g(c.device);
    HIP_TRY(h, g.err);
    hipStream_t s = (hipStream_t)stream;
    DecodeAsk ask = decode_ask(*io, ctl);
    HostLayout L;
    if (ask.devlay) capacity_layout(b, io->row_capacity, io->Lmax, L);
    else frame_layout(b, io->olens, io->masked, L, h->gap);
    FrameBufs f; bool ok;
    carve_frames(c, L, io->workspace, io->workspace_bytes, &f, &ok);
    if (!ok) return fail(h, FS2_ERR_WORKSPACE, "fs2_decode: workspace too small");
    h->kp = f.kp; h->kp_cap = f.kp_cap;
    int rc;
    DevLayout dl;
    if (ask.devlay) {
        if ((rc = device_layout(h, s, L, f.meta, dl, enc.o32, b.compat_padded, io->masked, io->Lmax, h->dec.pe_rows, io->status))) return rc;
    } else if ((rc = upload_layout(h, s, L, f.meta, dl))) return rc;
    const int R = L.R;
    // Kernel variants with different summation orders (LayerNorm fused into the row-complete GEMM or not) are chosen from a row
    // count.  The exact one is unknown to the host in the device-driven mode, and the capacity differs from it, so both modes use
    // the same ESTIMATE instead (regime_rows_of): 8 frames per phoneme plus the per-utterance alignment rows -- of this batch, or of
    // the larger batch the caller says this one is a shard of (fs2_batch.regime_*).
    const int regime_rows = regime_rows_of(b, /*token_level=*/false);
    h->cur_regime = regime_rows; h->cur_status = ask.devlay ? io->status : nullptr;
    const Rows rows{R, L.Rpad, dl.row_pos, dl.dims, regime_rows};
    DecIn dec_in;
    if (c.decoder_input_layer) dec_in = DecIn{&h->dec_in, h->dec_in_lng, h->dec_in_lnb, c.use_scaled_pos_enc ? 1.f : sqrtf((float)c.ddim)};
    const float* mel_after = c.postnet_layers > 0 ? f.after : f.before;
    ask.R = R; ask.short_buf = f.short_buf; ask.after_vec = unpack_vec(c.odim, mel_after, io->after); ask.before_vec = unpack_vec(c.odim, f.before, io->before);
    const DecodePlan p = plan_decode(c, opts(), b.precision, ask, enc, h->var2.ok, dec_in, h->dec, rows, f.sb);
    const int prec = p.prec;

    void* hfr_planes = p.hfr_planes ? f.sb.x1p : nullptr;
    const TokGatherArgs tg = tok_gather_args(h, f, dl, R);
    // FS2_VARSHORT: the rows the predictors run on -- at most K frames per phoneme, laid out by lr.index; their count is the device's (sdims), the host
    // sizes by the bound, and the kernel variants are chosen from the regime estimate at K frames per phoneme
    const int K = var_window(c);
    long long phonemes = 0;
    for (int i = 0; i < b.B; ++i) phonemes += b.ilens[i];
    const int Rs = p.varshort ? std::min(vs_row_bound(R, phonemes, b.B, K), R) : 0;
    int* const sdims = f.smeta + meta_align(2 * (long long)b.B);
    const Rows srows{Rs, rows_padded(Rs), f.srow_pos, sdims, regime_short_rows_of(b, K)};
    if (p.varshort) {
        ShortLayoutArgs sl;
        memset(&sl, 0, sizeof sl);
        sl.cum = enc.cum; sl.scum = enc.scum; sl.Tmax = b.Tmax; sl.ilen = enc.vlen; sl.so32 = enc.so32;
        sl.row_pos = dl.row_pos; sl.row_seq = dl.row_seq; sl.vlen = dl.vlen; sl.R = R; sl.ovf = p.devlay ? dl.dims + 2 : nullptr;
        sl.B = b.B; sl.gap = h->gap; sl.K = K; sl.Rs = Rs; sl.Rs_pad = srows.Rpad;
        sl.lri = f.lri; sl.f2s = f.f2s; sl.sstart = f.smeta; sl.slen = f.smeta + b.B; sl.sdims = sdims;
        sl.srow_pos = f.srow_pos; sl.srow_seq = f.srow_seq; sl.slri = f.slri;
        if ((rc = lr_index_short_launch(h, s, sl))) return rc;
    } else {      // the length regulator: its index alone where every consumer gathers from the token-level products, else rows (and planes) with it
        RowStepArgs ra;
        memset(&ra, 0, sizeof ra);
        ra.row_pos = dl.row_pos; ra.row_seq = dl.row_seq; ra.R = R; ra.vlen = dl.vlen; ra.B = b.B; ra.Tmax = b.Tmax; ra.D = c.adim;
        ra.cum_in = enc.cum; ra.ilen = enc.vlen; ra.tok_start = enc.start; ra.src_rows = enc.rows; ra.index_rows = f.lri; ra.rows = f.hfr; ra.planes = hfr_planes;
        if ((rc = p.tokproj == 3 ? lr_index_launch(h, s, ra) : lr_expand_launch(h, s, ra))) return rc;
    }
    if (p.varshort) {      // the same launches on the short rows: their metadata, their device row count, their regime
        TokGatherArgs ts = tg;
        ts.lri = f.slri; ts.row_pos = f.srow_pos; ts.row_seq = f.srow_seq; ts.R = Rs;
        if ((rc = run_predictors_fused(h, s, h->var2, f.hfr, c.adim, srows, hfr_planes, f.sb.xps, f.vp, f.vs, f.e_rows, f.p_rows, prec, &ts))) return rc;
    } else if (p.fused_var) {
        if ((rc = run_predictors_fused(h, s, h->var2, f.hfr, c.adim, rows, hfr_planes, f.sb.xps, f.vp, f.vs, f.e_rows, f.p_rows, prec, (p.tokproj & 1) ? &tg : nullptr))) return rc;
    } else {
        if (p.need_e && (rc = run_predictor(h, s, "energy", h->energy, f.hfr, c.adim, rows, f.t0, f.t1, f.e_rows, prec, hfr_planes, f.sb.xps))) return rc;
        if (p.need_p && (rc = run_predictor(h, s, "pitch", h->pitch, f.hfr, c.adim, rows, f.t0, f.t1, f.p_rows, prec, hfr_planes, f.sb.xps))) return rc;
    }
    if (p.control) {   // the predictions become the controlled values in place: both consumers below, and e_out / p_out, see those
        const ProsodyTrack ctl_p{ctl->pitch_scale, ctl->pitch_shift, ctl->pitch_scale_cols, ctl->pitch_shift_cols};
        const ProsodyTrack ctl_e{ctl->energy_scale, ctl->energy_shift, ctl->energy_scale_cols, ctl->energy_shift_cols};
        const int n = ask.ctl_pitch + ask.ctl_energy;
        const int Rc = p.varshort ? Rs : R;      // (the control is a function of utterance and phoneme alone: per short row it is what it is per frame)
        Scope sc(h, s, "var.control", 2.0 * Rc * n, 4.0 * Rc * (3.0 + 3.0 * n));
        if (p.varshort) hipLaunchKernelGGL(prosody_apply, dim3((Rs + 255) / 256), dim3(256), 0, s, f.p_rows, f.e_rows, f.srow_pos, f.srow_seq, f.slri, Rs, b.B, b.Tmax, ctl_p, ctl_e);
        else hipLaunchKernelGGL(prosody_apply, dim3((R + 255) / 256), dim3(256), 0, s, f.p_rows, f.e_rows, dl.row_pos, dl.row_seq, f.lri, R, b.B, b.Tmax, ctl_p, ctl_e);
        HIP_TRY(h, hipGetLastError());
    }
    if (!(p.tokproj & 2)) {
        RowStepArgs ra;
        memset(&ra, 0, sizeof ra);
        ra.row_pos = dl.row_pos; ra.row_seq = dl.row_seq; ra.R = R; ra.D = c.adim; ra.rows = f.hfr; ra.planes = hfr_planes;
        ra.es = io->es; ra.es_stride = io->es_stride; ra.ps = io->ps; ra.ps_stride = io->ps_stride; ra.e_rows = f.e_rows; ra.p_rows = f.p_rows;
        ra.ebins = h->ebins; ra.pbins = h->pbins; ra.nb = c.n_bins - 1; ra.Te = h->Te; ra.Tp = h->Tp; ra.qe_rows = f.qe; ra.qp_rows = f.qp;
        if ((rc = var_embed_launch(h, s, ra))) return rc;
    }
    if (p.tokproj & 2) {
        if ((rc = dec_in_gather_launch(h, s, dec_in_gather_args(h, io, tg, f, p, Rs)))) return rc;
    } else if (c.decoder_input_layer) {   // decoder input layer: Linear -> LN -> ReLU -> + alpha * pe   (reference encoder.py:118-125)
        if ((rc = launch_step(h, s, nullptr, dec_in_step(dec_in, h->dec, f.hfr, c.adim, hfr_planes, rows, f.sb, prec, p.po), prec))) return rc;
    } else if ((rc = dec_in_pe_launch(h, s, f, dl, R, p.planes))) return rc;
    if ((rc = run_stack(h, s, "dec", h->dec, c.ddim, c.aheads, rows, L, dl, p.mask_q, f.sb, prec, /*x0p_ready=*/p.planes, p.ffn_terms, p.po))) return rc;
    if (p.po && io->dec_out) {      // the API hands the decoder output out as fp32 rows: rebuilt from the planes (hi + lo) only when asked for
        if ((rc = planes_to_rows_launch(h, s, "dec.out.rows", f.sb.x0p, R, c.ddim, f.sb.x0))) return rc;
    }
    const int rf = p.rf;
    DevLayout dl2;      // the Postnet's and the mel outputs' layout: rf rows per decoder row
    if ((rc = mel_layout(h, s, f, dl, b.B, L.Rpad, rf, dl2))) return rc;
    // planes hand-off through the tail: decoder -> feat_out (fp32 mel + planes of it) -> Postnet convs ping-pong x0p / x1p
    if ((rc = launch_step(h, s, nullptr, feat_out_step(h->feat, rows, f.sb, f.before, prec, p.post_pl), prec))) return rc;
    if (c.postnet_layers > 0) {
        const Rows rows2{R * rf, L.Rpad * rf, dl2.row_pos, dl2.dims, 0};
        const PostBufs pb{f.before, f.after, rf > 1 ? f.pa2 : f.sb.hid, rf > 1 ? f.pb2 : f.sb.hid + (size_t)L.Rpad * c.postnet_chans, rf > 1 ? f.xps2 : f.sb.xps};
        for (int l = 0; l < c.postnet_layers; ++l)
            if ((rc = launch_step(h, s, nullptr, postnet_step(h->post, l, c.odim, rows2, pb, f.sb, p.post_pl, p.ffn_terms, opts()), prec))) return rc;
    }
    return decode_outputs(h, s, io, p, f, dl, dl2, R, mel_after);
}

// ---------------------------------------------------------------------------------- single operators
#define OP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { g_create_error = std::string(#expr) + ": " + hipGetErrorString(e_); return FS2_ERR_HIP; } } while (0)

// temporary device memory of an operator entry point: released on every exit path (after the stream drained)
struct DevTmp {
    hipStream_t s;
    std::vector<void*> ptrs;
    explicit DevTmp(hipStream_t s_) : s(s_) {}
    ~DevTmp() { if (!ptrs.empty()) hipStreamSynchronize(s); for (void* p : ptrs) hipFree(p); }
    hipError_t alloc(void** out, size_t bytes) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) { ptrs.push_back(p); *out = p; }
        return e;
    }
};

int fs2_op_conv_gemm(void* stream, const fs2_op_gemm_args* o) {
    if (!o) return fail(nullptr, FS2_ERR_ARG, "fs2_op_conv_gemm: null argument");
    ABI_CHECK(nullptr, "fs2_op_conv_gemm", o, fs2_op_gemm_args);
    if (!o->x || !o->w || o->R <= 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_conv_gemm: bad arguments");
    if (o->precision < FS2_PREC_FP32 || o->precision > FS2_PREC_MIX_MX4) return fail(nullptr, FS2_ERR_ARG, "unknown precision %d", o->precision);
    const bool mx = o->precision == FS2_PREC_MIX_MX || o->precision == FS2_PREC_MIX_MX4;   // THIS operator in the fp16 + block-scaled-fp8 arithmetic (convolutions, C % 128 == 0; the fp4 form exists inside the model only: its operand comes with row scales from a LayerNorm epilogue)
    const int f16t = mx ? 1 : ffn_f16_terms(o->precision);      // mixed modes: THIS operator on fp16 operands with 2 / 1 MFMAs per fragment pair
    hipStream_t s = (hipStream_t)stream;
    const WeightAsk ask = ask_conv_op(o->N, o->C, o->ktaps, mx);
    const WeightPlan wp = plan_weight(ask);
    if (mx && !wp.has(kImgWm)) return fail(nullptr, FS2_ERR_UNSUPPORTED, "the mx arithmetic needs a convolution with C %% 128 == 0 and N %% 128 == 0");
    DevTmp tmp(s);
    unsigned* scr = nullptr;      // (device_absmax)
    if (mx) OP_TRY(tmp.alloc((void**)&scr, 16));
    WeightSrc src;
    src.w[0] = o->w; src.bn_eps = 0.f; src.wb_f16 = f16t != 0;
    Gemm g;
    hipError_t werr = hipSuccess;
    if (!build_weight(s, ask, wp, src, scr, [&](WeightImage, size_t bytes) { void* p = nullptr; werr = tmp.alloc(&p, bytes); return p; }, g)) OP_TRY(werr);
    float* scratch = nullptr;
    OP_TRY(tmp.alloc((void**)&scratch, (size_t)o->R * o->N * sizeof(float)));
    void* xps = nullptr;          // planes of x for the bf16 modes (gemm_planes.h)
    if (o->precision != FS2_PREC_FP32) OP_TRY(tmp.alloc((void**)&xps, (size_t)o->R * g.Cpad * sizeof(float)));
    int* rp = nullptr;
    g.bias = const_cast<float*>(o->bias);
    GemmArgs a = gemm_args(g, o->x, o->C, o->R, nullptr, o->y, o->N);
    a.scratch = scratch;
    if (o->row_valid) {   // row_valid (0/1) -> row_pos (-1 / 0)
        OP_TRY(tmp.alloc((void**)&rp, (size_t)o->R * sizeof(int)));
        std::vector<int> hv(o->R);
        OP_TRY(hipMemcpyAsync(hv.data(), o->row_valid, (size_t)o->R * sizeof(int), hipMemcpyDeviceToHost, s));
        OP_TRY(hipStreamSynchronize(s));
        for (auto& v : hv) v = v ? 0 : -1;
        OP_TRY(hipMemcpyAsync(rp, hv.data(), (size_t)o->R * sizeof(int), hipMemcpyHostToDevice, s));
        a.row_pos = rp;
    }
    a.resid = o->resid; a.ldr = o->N; a.relu_pre = o->relu_pre; a.ln_g = o->ln_gamma; a.ln_b = o->ln_beta; a.ln_eps = o->ln_eps;
    a.act_post = o->act_post; a.dot_w = o->dot_w; a.dot_b = o->dot_b; a.dot_out = o->dot_out;
    a.xp_scratch = xps;
    a.f16_terms = mx ? 0 : f16t;
    if (mx) {      // (the activation scale is measured from x itself: the operator has no LayerNorm to bound it)
        const int ka = fp8_scale_exponent(device_absmax(s, o->x, (int64_t)o->R * o->C, scr));
        a.mx = 1; a.Wb = g.wm; a.yp_scale = exp2f((float)ka); a.mx_scale = scale_byte4(127 - ka - 11); a.mx_scale_b = scale_byte4(127 - g.kw);
    }
    return launch_gemm(nullptr, s, "op.conv_gemm", a, base_precision(o->precision));      // (tmp drains the stream and frees)
}

// Test hook (include/fs2.h): the launch path of the model -- plan_gemm, then launch_gemm -- on a caller-formed argument block; the plan goes back to the caller
// first, so that a test knows which kernel its numbers came from.
int fs2_op_launch_gemm(void* stream, const void* gemm_args, uint32_t args_size, int32_t precision, int32_t* plan_out, int32_t plan_cap) {
    if (!gemm_args || !plan_out) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_gemm: null argument");
    if (args_size != sizeof(GemmArgs)) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_gemm: argument block of %u bytes, this library's GemmArgs has %zu", args_size, sizeof(GemmArgs));
    if (plan_cap < FS2_GEMM_PLAN_FIELDS) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_gemm: plan_out holds %d fields, %d are written", plan_cap, FS2_GEMM_PLAN_FIELDS);
    if (precision != FS2_PREC_FP32 && precision != FS2_PREC_BF16X3 && precision != FS2_PREC_BF16) return fail(nullptr, FS2_ERR_ARG, "unknown precision %d", precision);
    GemmArgs a;
    memcpy(&a, gemm_args, sizeof a);
    const GemmPlan p = plan_gemm(a, precision, opts());
    const int32_t fields[FS2_GEMM_PLAN_FIELDS] = {(int32_t)p.kernel, p.nsplit, p.nb, p.bm, p.mt, p.apart, p.epi, p.arith, p.res, p.ksplit, p.rows_pass, p.build_planes};
    memcpy(plan_out, fields, sizeof fields);
    return launch_gemm(nullptr, (hipStream_t)stream, "op.launch_gemm", a, precision);
}

// Test hook (include/fs2.h): the weight repack of the mixed modes as fs2_load_weights runs it -- build_weight, the loader's executor: kw from max |w|, the scale
// image preset to 127 -- on the plan of that one image, into the caller's buffers.
int fs2_op_repack_weight(void* stream, const float* w, int32_t N, int32_t C, int32_t ktaps, int32_t format, void* image, size_t image_bytes,
                         void* scale_image, size_t scale_bytes, int32_t* kw_out) {
    if (!w || !image || !kw_out) return fail(nullptr, FS2_ERR_ARG, "fs2_op_repack_weight: null argument");
    if (format != FS2_REPACK_MX && format != FS2_REPACK_MX4) return fail(nullptr, FS2_ERR_ARG, "fs2_op_repack_weight: unknown format %d", format);
    if (N <= 0 || N % 128 != 0 || C <= 0 || C % 128 != 0 || ktaps < 1 || ktaps % 2 == 0 || ktaps - 1 > kMaxHalo)
        return fail(nullptr, FS2_ERR_ARG, "fs2_op_repack_weight: needs N %% 128 == 0, C %% 128 == 0 and an odd kernel size up to %d (N %d, C %d, k %d)", kMaxHalo + 1, N, C, ktaps);
    const bool mx4 = format == FS2_REPACK_MX4;
    const WeightPlan wp = plan_image_alone(N, C, ktaps, mx4);
    const size_t bytes = wp.bytes[mx4 ? kImgWm4 : kImgWm], sbytes = wp.bytes[kImgWs4];
    if (image_bytes != bytes) return fail(nullptr, FS2_ERR_ARG, "fs2_op_repack_weight: image of %zu bytes, the format takes %zu", image_bytes, bytes);
    if (mx4 && (!scale_image || scale_bytes != sbytes)) return fail(nullptr, FS2_ERR_ARG, "fs2_op_repack_weight: scale image of %zu bytes, the format takes %zu", scale_image ? scale_bytes : (size_t)0, sbytes);
    hipStream_t s = (hipStream_t)stream;
    DevTmp tmp(s);
    unsigned* scr = nullptr;
    OP_TRY(tmp.alloc((void**)&scr, 16));
    WeightSrc src;
    src.w[0] = w;
    Gemm g;
    build_weight(s, ask_conv_op(N, C, ktaps, true), wp, src, scr, [&](WeightImage i, size_t) { return i == kImgWs4 ? scale_image : image; }, g);
    *kw_out = g.kw;
    OP_TRY(hipGetLastError());
    OP_TRY(hipStreamSynchronize(s));
    return FS2_OK;
}

int fs2_op_attention(void* stream, const float* qkv, float* ctx, int32_t D, int32_t heads, int32_t B, const int32_t* seq_start,
                     const int32_t* seq_len, const int32_t* seq_klen, int32_t mask_q, int32_t precision) {
    if (!qkv || !ctx || B <= 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_attention: bad arguments");
    if (precision < FS2_PREC_FP32 || precision > FS2_PREC_BF16) return fail(nullptr, FS2_ERR_ARG, "unknown precision %d", precision);
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> host;
    std::vector<int2> work;
    int R = 0;
    for (int b = 0; b < B; ++b) {
        for (int q = 0; q < att_blocks(std::max(seq_len[b], 0)); ++q) work.push_back(make_int2(b, q));
        R = std::max(R, seq_start[b] + seq_len[b]);
        if (precision != FS2_PREC_FP32 && seq_start[b] % kAttAlign) return fail(nullptr, FS2_ERR_ARG, "bf16 attention needs sequence starts aligned to %d rows", kAttAlign);
    }
    host.insert(host.end(), seq_start, seq_start + B);
    host.insert(host.end(), seq_len, seq_len + B);
    host.insert(host.end(), seq_klen, seq_klen + B);
    for (auto& w : work) { host.push_back(w.x); host.push_back(w.y); }
    DevTmp tmp(s);
    int* dev = nullptr;
    OP_TRY(tmp.alloc((void**)&dev, host.size() * sizeof(int) + 16));
    OP_TRY(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    DevLayout dl;
    dl.start = dev; dl.len = dev + B; dl.klen = dev + 2 * B; dl.work = reinterpret_cast<int2*>(dev + 3 * B);
    AttnIo io{qkv, ctx, nullptr, nullptr, nullptr, nullptr, nullptr, &dl, mask_q, 0.0, AttnCall{D, heads, 0, precision, R, 0, 0, (int)work.size()}};
    if (precision != FS2_PREC_FP32) {
        const int Rvt = io.c.Rvt = round_up(R + kTailRows, 128);      // (8-key V^T vectors that straddle the last key stay inside the planes)
        __bf16* planes = nullptr;
        OP_TRY(tmp.alloc((void**)&planes, (size_t)Rvt * D * 6 * sizeof(__bf16)));
        io.qkh = planes; io.qkl = planes + (size_t)Rvt * 2 * D; io.vth = io.qkl + (size_t)Rvt * 2 * D; io.vtl = io.vth + (size_t)Rvt * D;
        if (opts().op_att_planes > 0 && D % 32 == 0) {
            // the model's output form: the kernels write the context as planes only (attn_w32: the LDS-staged epilogue), converted below
            io.ctx = nullptr;
            OP_TRY(tmp.alloc(&io.ctxp, (size_t)Rvt * D * 4));
            OP_TRY(hipMemsetAsync(io.ctxp, 0xff, (size_t)Rvt * D * 4, s));      // (NaN in both halves: a query row the kernels leave unwritten shows in ctx)
        }
    }
    const int rc = launch_attention(nullptr, s, "op.attention", io);
    if (rc == FS2_OK && io.ctxp) {
        const int64_t n = (int64_t)R * (D / 4);
        hipLaunchKernelGGL(planes_to_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, io.ctxp, D / 32, R, D, ctx, D);
        OP_TRY(hipGetLastError());
    }
    return rc;      // (tmp drains the stream and frees)
}

// Test hook (include/fs2.h): the launch path of the model -- plan_attention, then launch_attention -- on the caller's device buffers; the plan goes back to the
// caller first, so that a test knows which kernel its numbers came from.
int fs2_op_launch_attention(void* stream, const fs2_op_attn_args* o, int32_t* plan_out, int32_t plan_cap) {
    if (!o || !plan_out) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_attention: null argument");
    if (o->struct_size != sizeof(fs2_op_attn_args)) return fail(nullptr, FS2_ERR_ARG, "fs2_op_attn_args.struct_size %u != %zu", o->struct_size, sizeof(fs2_op_attn_args));
    if (plan_cap < FS2_ATTN_PLAN_FIELDS) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_attention: plan_out holds %d fields, %d are written", plan_cap, FS2_ATTN_PLAN_FIELDS);
    if (o->precision != FS2_PREC_FP32 && o->precision != FS2_PREC_BF16X3 && o->precision != FS2_PREC_BF16) return fail(nullptr, FS2_ERR_ARG, "unknown precision %d", o->precision);
    const bool f32 = o->precision == FS2_PREC_FP32;
    if (!o->start || !o->len || !o->klen || !o->work || (f32 ? !o->qkv || !o->ctx : !o->qk_hi || !o->qk_lo || !o->vt_hi || !o->vt_lo || (!o->ctx && !o->ctxp)))
        return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_attention: null buffer (precision %d)", o->precision);
    if (o->nitems < 0 || o->D <= 0 || o->heads <= 0 || o->R < 0 || o->Rvt < 0 || (!f32 && o->Rvt % 32)) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_attention: bad sizes");
    DevLayout dl;
    dl.start = const_cast<int*>(o->start); dl.len = const_cast<int*>(o->len); dl.klen = const_cast<int*>(o->klen);
    dl.work = reinterpret_cast<int2*>(const_cast<int*>(o->work)); dl.dims = const_cast<int*>(o->dims);
    AttnIo io{o->qkv, o->ctx, f32 ? nullptr : o->ctxp, (__bf16*)o->qk_hi, (__bf16*)o->qk_lo, (__bf16*)o->vt_hi, (__bf16*)o->vt_lo, &dl, o->mask_q, 0.0,
              AttnCall{o->D, o->heads, o->dk_true, o->precision, o->R, o->Rvt, o->regime_rows, o->nitems}};
    io.slow_count = o->slow_count;
    attn_call_pointers(io);
    const AttnPlan p = plan_attention(io.c, opts());
    int32_t scale_bits;
    memcpy(&scale_bits, &p.softmax_scale, sizeof scale_bits);
    const int32_t fields[FS2_ATTN_PLAN_FIELDS] = {(int32_t)p.kernel, p.dk, p.nsplit, (int32_t)p.grid_x, (int32_t)p.grid_y, (int32_t)p.split_pass, scale_bits};
    memcpy(plan_out, fields, sizeof fields);
    return launch_attention(nullptr, (hipStream_t)stream, "op.launch_attention", io);
}

// Test hook (include/fs2.h): ONE row step between the GEMMs through the function fs2_encode / fs2_decode_ctl launch it with, on the library's own argument block.
int fs2_op_launch_row_step(void* stream, int32_t step, const void* args, uint32_t args_size) {
    if (!args) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_row_step: null argument block");
    hipStream_t s = (hipStream_t)stream;
    const bool gather = step == FS2_ROW_STEP_VAR_GATHER0 || step == FS2_ROW_STEP_DEC_IN_GATHER, shortl = step == FS2_ROW_STEP_LR_INDEX_SHORT;
    if (step < 0 || step >= FS2_ROW_STEP_COUNT) return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_row_step: unknown step %d", step);
    const size_t want = gather ? sizeof(TokGatherArgs) : (shortl ? sizeof(ShortLayoutArgs) : sizeof(RowStepArgs));
    if (args_size != want)
        return fail(nullptr, FS2_ERR_ARG, "fs2_op_launch_row_step: argument block of %u bytes, this library's %s has %zu", args_size,
                    gather ? "TokGatherArgs" : (shortl ? "ShortLayoutArgs" : "RowStepArgs"), want);
    if (gather) {
        TokGatherArgs tg;
        memcpy(&tg, args, sizeof tg);
        return step == FS2_ROW_STEP_VAR_GATHER0 ? var_gather0_launch(nullptr, s, tg) : dec_in_gather_launch(nullptr, s, tg);
    }
    if (shortl) {
        ShortLayoutArgs sl;
        memcpy(&sl, args, sizeof sl);
        return lr_index_short_launch(nullptr, s, sl);
    }
    RowStepArgs a;
    memcpy(&a, args, sizeof a);
    switch (step) {
        case FS2_ROW_STEP_EMBED: return embed_launch(nullptr, s, a);
        case FS2_ROW_STEP_DUR_POST: return dur_post_launch(nullptr, s, a);
        case FS2_ROW_STEP_LR_INDEX: return lr_index_launch(nullptr, s, a);
        case FS2_ROW_STEP_LR_EXPAND: return lr_expand_launch(nullptr, s, a);
        case FS2_ROW_STEP_VAR_EMBED: return var_embed_launch(nullptr, s, a);
        case FS2_ROW_STEP_TO_PLANES: return to_planes_launch(nullptr, s, "op.in.planes", a.rows, a.R, a.D, a.planes);
        default: return planes_to_rows_launch(nullptr, s, "op.out.rows", a.planes, a.R, a.D, a.rows);
    }
}

int fs2_op_length_regulate(void* stream, const float* hs, const int64_t* ds, const int64_t* ilens_host, int32_t B, int32_t Tmax,
                           int32_t D, int32_t Lmax, float alpha, float* out, int32_t* index, int64_t* olens) {
    if (!hs || !ds || !ilens_host || !out || B <= 0 || D % 4 || !(alpha > 0.f)) return fail(nullptr, FS2_ERR_ARG, "fs2_op_length_regulate: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> host(2 * B);
    for (int b = 0; b < B; ++b) { host[b] = b * Tmax; host[B + b] = (int)ilens_host[b]; }
    DevTmp tmp(s);
    int* dev = nullptr;
    OP_TRY(tmp.alloc((void**)&dev, ((size_t)3 * B + (size_t)B * Tmax) * sizeof(int)));
    OP_TRY(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    int *tok_start = dev, *ilen = dev + B, *o32 = dev + 2 * B, *cum = dev + 3 * B;
    hipLaunchKernelGGL(dur_scan, dim3(B), dim3(256), 0, s, ds, Tmax, ilen, cum, olens, o32, alpha);
    const int R = B * Lmax;
    hipLaunchKernelGGL(lr_expand, dim3((R + 3) / 4), dim3(256), 0, s, hs, D, tok_start, ilen, cum, Tmax, (const int*)nullptr,
                       (const int*)nullptr, Lmax, o32, R, out, index);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "length_regulate: %s", hipGetErrorString(e));
    return FS2_OK;
}

int fs2_op_unpack_rows(void* stream, const float* src, int32_t W, int32_t B, const int32_t* starts, const int32_t* lens, int32_t Lout,
                       float* dst) {
    if (!src || !dst || !starts || !lens || B <= 0 || W <= 0 || Lout <= 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_unpack_rows: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // per-process scratch for the two small index arrays (grown on demand, never freed: a few KB)
    static int* dev = nullptr; static int cap = 0;
    if (2 * B > cap) {
        if (dev) hipFree(dev);
        cap = std::max(2 * B, 4096);
        OP_TRY(hipMalloc((void**)&dev, (size_t)cap * sizeof(int)));
    }
    std::vector<int> host(2 * B);
    for (int i = 0; i < B; ++i) { host[i] = starts[i]; host[B + i] = lens[i]; }
    OP_TRY(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    const int64_t total = (int64_t)B * Lout * W;
    if (W % 4 == 0 && (reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) % 16 == 0)
        hipLaunchKernelGGL(unpack_rows4, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, src, W / 4, dev, dev + B, B, Lout, dst);
    else
        hipLaunchKernelGGL(unpack_rows<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, W, dev, dev + B, B, Lout, dst, 0.f);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "unpack_rows: %s", hipGetErrorString(e));
    return FS2_OK;
}

int fs2_op_unpack_rows_dev(void* stream, const float* src, int32_t W, int32_t B, const int32_t* starts_dev, const int32_t* lens_dev,
                           int32_t Lout, float* dst) {
    if (!src || !dst || !starts_dev || !lens_dev || B <= 0 || W <= 0 || Lout <= 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_unpack_rows_dev: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)B * Lout * W;
    if (W % 4 == 0 && (reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) % 16 == 0)
        hipLaunchKernelGGL(unpack_rows4, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, src, W / 4, starts_dev, lens_dev, B, Lout, dst);
    else
        hipLaunchKernelGGL(unpack_rows<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, W, starts_dev, lens_dev, B, Lout, dst, 0.f);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "unpack_rows: %s", hipGetErrorString(e));
    return FS2_OK;
}

int fs2_op_transpose(void* stream, const float* src, int64_t N, int32_t W, float* dst) {
    if (!src || !dst || N < 0 || W <= 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_transpose: bad arguments");
    if (N == 0) return FS2_OK;
    hipLaunchKernelGGL(transpose_rows, dim3((unsigned)((N + 31) / 32), (W + 31) / 32), dim3(256), 0, (hipStream_t)stream, src, N, W, dst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "transpose: %s", hipGetErrorString(e));
    return FS2_OK;
}

int fs2_op_duration(void* stream, const float* d_log, int64_t n, int64_t* d) {
    if (!d_log || !d || n < 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_duration: bad arguments");
    if (n == 0) return FS2_OK;
    hipLaunchKernelGGL(duration_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_log, n, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "duration: %s", hipGetErrorString(e));
    return FS2_OK;
}

int fs2_set_option(const char* name, int32_t value) {
    if (!name) return fail(nullptr, FS2_ERR_ARG, "fs2_set_option: null name");
    Options& o = opts();
    const std::string n = name;
    if (n == "FS2_BM") o.bm = value;
    else if (n == "FS2_ROW8") o.row8 = value;
    else if (n == "FS2_QKV8") o.qkv8 = value;
    else if (n == "FS2_NOSPLITK") o.nosplitk = value > 0;
    else if (n == "FS2_F32_ROWS") o.f32_rows = value > 0;
    else if (n == "FS2_MT8") o.mt8 = value;
    else if (n == "FS2_QKV_SPLIT") o.qkv_split = value;
    else if (n == "FS2_OP_ATT_PLANES") o.op_att_planes = value;
    else if (n == "FS2_FUSE_VAR") o.fuse_var = value != 0;
    else if (n == "FS2_BAL") o.bal = value < 0 ? 0 : value;
    else if (n == "FS2_ATTN_W32") o.w32 = value;
    else if (n == "FS2_ROW4") o.row4 = value;
    else if (n == "FS2_MT4") o.mt4 = value;
    else if (n == "FS2_FFN2_MX") o.ffn2_mx = value != 0;
    else if (n == "FS2_QKV4") o.qkv4 = value;
    else if (n == "FS2_POST_MX") o.post_mx = value != 0;
    else if (n == "FS2_TOKPROJ") o.tokproj = value < 0 ? 3 : (value & 3);
    else if (n == "FS2_TOKPROJ_F32") o.tokproj_f32 = value > 0;
    else if (n == "FS2_VARSHORT") o.varshort = value != 0;      // (-1: the default, on)
    else return fail(nullptr, FS2_ERR_ARG, "fs2_set_option: unknown option %s", name);
    return FS2_OK;
}

int fs2_get_option(const char* name, int32_t* value) {
    if (!name || !value) return fail(nullptr, FS2_ERR_ARG, "fs2_get_option: null argument");
    const Options& o = opts();
    const std::string n = name;
    if (n == "FS2_AUDIT_CLEAN") *value = audit_clean() ? 1 : 0;
    else if (n == "attn_w32_active") *value = o.w32 != 0;
    else if (n == "row4_active") *value = o.row4 != 0;
    else if (n == "qkv4_active") *value = o.qkv4 != 0 && o.row4 != 0;
    else if (n == "FS2_BM") *value = o.bm;
    else if (n == "FS2_ROW8") *value = o.row8;
    else if (n == "FS2_QKV8") *value = o.qkv8;
    else if (n == "FS2_NOSPLITK") *value = o.nosplitk;
    else if (n == "FS2_F32_ROWS") *value = o.f32_rows;
    else if (n == "FS2_MT8") *value = o.mt8;
    else if (n == "FS2_QKV_SPLIT") *value = o.qkv_split;
    else if (n == "FS2_OP_ATT_PLANES") *value = o.op_att_planes;
    else if (n == "FS2_FUSE_VAR") *value = o.fuse_var;
    else if (n == "FS2_BAL") *value = o.bal;
    else if (n == "FS2_ATTN_W32") *value = o.w32;
    else if (n == "FS2_ROW4") *value = o.row4;
    else if (n == "FS2_MT4") *value = o.mt4;
    else if (n == "FS2_FFN2_MX") *value = o.ffn2_mx;
    else if (n == "FS2_QKV4") *value = o.qkv4;
    else if (n == "FS2_POST_MX") *value = o.post_mx;
    else if (n == "FS2_TOKPROJ") *value = o.tokproj;
    else if (n == "FS2_TOKPROJ_F32") *value = o.tokproj_f32;
    else if (n == "FS2_VARSHORT") *value = o.varshort;
    else return fail(nullptr, FS2_ERR_ARG, "fs2_get_option: unknown option %s", name);
    return FS2_OK;
}

int fs2_get_counter(fs2_handle* h, void* stream, const char* name, int64_t* value, int32_t reset) {
    if (!h || !name || !value) return fail(h, FS2_ERR_ARG, "fs2_get_counter: null argument");
    if (std::string(name) != "attn_slow_path_waves") return fail(h, FS2_ERR_ARG, "fs2_get_counter: unknown counter %s", name);
    DeviceGuard g(h->cfg.device);
    HIP_TRY(h, g.err);
    hipStream_t s = (hipStream_t)stream;
    int v = 0;
    HIP_TRY(h, hipMemcpyAsync(&v, h->counters, sizeof(int), hipMemcpyDeviceToHost, s));
    if (reset) HIP_TRY(h, hipMemsetAsync(h->counters, 0, sizeof(int), s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *value = v;
    return FS2_OK;
}

int fs2_op_bucketize(void* stream, const float* x, int64_t n, const float* bins, int32_t nb, int32_t* idx) {
    if (!x || !bins || !idx || n < 0) return fail(nullptr, FS2_ERR_ARG, "fs2_op_bucketize: bad arguments");
    if (n == 0) return FS2_OK;
    hipLaunchKernelGGL(bucketize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, bins, nb, idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "bucketize: %s", hipGetErrorString(e));
    return FS2_OK;
}

// The vocoder's entry points (griffin_lim_host.h): each fills one GlCall -- who, kind, geometry, batch, workspace, source, iteration,
// output -- and hands it to gl_call; a query hands the same who-kind-geometry-batch to gl_workspace_bytes.
size_t fs2_op_vocode_workspace_bytes(int32_t B, const int32_t* lens) { return fs2_op_vocode_workspace_bytes_geom(kGlNfft, kGlHop, kGlNfft, 80, B, lens); }

size_t fs2_op_vocode_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* lens) {
    return gl_workspace_bytes({"fs2_op_vocode_workspace_bytes_geom", GlKind::Synthesis, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, lens)});
}

int fs2_op_griffin_lim(void* stream, const float* src, int32_t src_width, const float* mel_pinv, int32_t B, const int32_t* starts,
                       const int32_t* lens, int32_t n_iter, float momentum, uint32_t seed, const float* init_phase, void* workspace,
                       size_t workspace_bytes, float* wav) {
    return gl_call(stream, {"fs2_op_griffin_lim", GlKind::Synthesis, {kGlNfft, kGlHop, kGlNfft, 80}, gl_host_batch(B, starts, lens),
                            {workspace, workspace_bytes}, {src, src_width, mel_pinv, nullptr}, {n_iter, momentum, seed, init_phase}, {wav}});
}

int fs2_op_griffin_lim_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* src, int32_t src_width, const float* mel_pinv, int32_t B,
                            const int32_t* starts, const int32_t* lens, int32_t n_iter, float momentum, uint32_t seed, const float* init_phase,
                            void* workspace, size_t workspace_bytes, float* wav) {
    return gl_call(stream, {"fs2_op_griffin_lim_geom", GlKind::Synthesis, {n_fft, hop, win, n_mels}, gl_host_batch(B, starts, lens),
                            {workspace, workspace_bytes}, {src, src_width, mel_pinv, nullptr}, {n_iter, momentum, seed, init_phase}, {wav}});
}

size_t fs2_op_vocode_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity) {
    return gl_workspace_bytes({"fs2_op_vocode_workspace_bytes_cap", GlKind::Synthesis, {n_fft, hop, win, n_mels},
                               gl_device_batch(B, nullptr, 0, frame_capacity, nullptr)});
}

int fs2_op_griffin_lim_dev(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* src, int32_t src_width, const float* mel_pinv,
                           int32_t B, const int64_t* lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status, int32_t n_iter,
                           float momentum, uint32_t seed, const float* init_phase, void* workspace, size_t workspace_bytes, float* wav, int32_t wav_stride,
                           int64_t wav_capacity, int64_t* sample_lens_dev, int32_t* status) {
    return gl_call(stream, {"fs2_op_griffin_lim_dev", GlKind::Synthesis, {n_fft, hop, win, n_mels},
                            gl_device_batch(B, lens_dev, src_stride, frame_capacity, upstream_status), {workspace, workspace_bytes},
                            {src, src_width, mel_pinv, nullptr}, {n_iter, momentum, seed, init_phase},
                            {wav, wav_stride, wav_capacity, sample_lens_dev, status}});
}

size_t fs2_op_vocode_mel_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* lens) {
    return gl_workspace_bytes({"fs2_op_vocode_mel_workspace_bytes_geom", GlKind::MelSynthesis, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, lens)});
}

int fs2_op_griffin_lim_mel_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* src, int32_t src_width, const float* mel_pinv,
                                const float* mel_basis, int32_t B, const int32_t* starts, const int32_t* lens, int32_t n_iter, float momentum, uint32_t seed,
                                const float* init_phase, void* workspace, size_t workspace_bytes, float* wav) {
    return gl_call(stream, {"fs2_op_griffin_lim_mel_geom", GlKind::MelSynthesis, {n_fft, hop, win, n_mels}, gl_host_batch(B, starts, lens),
                            {workspace, workspace_bytes}, {src, src_width, mel_pinv, mel_basis}, {n_iter, momentum, seed, init_phase}, {wav}});
}

size_t fs2_op_vocode_mel_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity) {
    return gl_workspace_bytes({"fs2_op_vocode_mel_workspace_bytes_cap", GlKind::MelSynthesis, {n_fft, hop, win, n_mels},
                               gl_device_batch(B, nullptr, 0, frame_capacity, nullptr)});
}

int fs2_op_griffin_lim_mel_dev(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* src, int32_t src_width, const float* mel_pinv,
                               const float* mel_basis, int32_t B, const int64_t* lens_dev, int32_t src_stride, int64_t frame_capacity,
                               const int32_t* upstream_status, int32_t n_iter, float momentum, uint32_t seed, const float* init_phase, void* workspace,
                               size_t workspace_bytes, float* wav, int32_t wav_stride, int64_t wav_capacity, int64_t* sample_lens_dev, int32_t* status) {
    return gl_call(stream, {"fs2_op_griffin_lim_mel_dev", GlKind::MelSynthesis, {n_fft, hop, win, n_mels},
                            gl_device_batch(B, lens_dev, src_stride, frame_capacity, upstream_status), {workspace, workspace_bytes},
                            {src, src_width, mel_pinv, mel_basis}, {n_iter, momentum, seed, init_phase},
                            {wav, wav_stride, wav_capacity, sample_lens_dev, status}});
}

size_t fs2_op_spsi_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* lens) {
    return gl_workspace_bytes({"fs2_op_spsi_workspace_bytes_geom", GlKind::SpsiPhase, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, lens)});
}

size_t fs2_op_spsi_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity) {
    return gl_workspace_bytes({"fs2_op_spsi_workspace_bytes_cap", GlKind::SpsiPhase, {n_fft, hop, win, n_mels},
                               gl_device_batch(B, nullptr, 0, frame_capacity, nullptr)});
}

int fs2_op_spsi_phase_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* src, int32_t src_width, const float* mel_pinv,
                           int32_t B, const int32_t* starts, const int32_t* lens, void* workspace, size_t workspace_bytes, float* phase, float* mag_out) {
    GlCall c{"fs2_op_spsi_phase_geom", GlKind::SpsiPhase, {n_fft, hop, win, n_mels}, gl_host_batch(B, starts, lens), {workspace, workspace_bytes},
             {src, src_width, mel_pinv, nullptr}};
    c.spsi = {phase, mag_out};
    return gl_call(stream, c);
}

int fs2_op_spsi_phase_dev(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* src, int32_t src_width, const float* mel_pinv,
                          int32_t B, const int64_t* lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status, void* workspace,
                          size_t workspace_bytes, float* phase, float* mag_out) {
    GlCall c{"fs2_op_spsi_phase_dev", GlKind::SpsiPhase, {n_fft, hop, win, n_mels}, gl_device_batch(B, lens_dev, src_stride, frame_capacity, upstream_status),
             {workspace, workspace_bytes}, {src, src_width, mel_pinv, nullptr}};
    c.spsi = {phase, mag_out};
    return gl_call(stream, c);
}

size_t fs2_op_f0_phase_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* lens) {
    return gl_workspace_bytes({"fs2_op_f0_phase_workspace_bytes_geom", GlKind::F0Phase, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, lens)});
}

size_t fs2_op_f0_phase_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity) {
    return gl_workspace_bytes({"fs2_op_f0_phase_workspace_bytes_cap", GlKind::F0Phase, {n_fft, hop, win, n_mels},
                               gl_device_batch(B, nullptr, 0, frame_capacity, nullptr)});
}

int fs2_op_f0_phase_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* f0, int32_t B, const int32_t* starts,
                         const int32_t* lens, double f0_floor, double f0_ceil, int32_t sample_rate, uint32_t seed, void* workspace, size_t workspace_bytes,
                         float* phase) {
    GlCall c{"fs2_op_f0_phase_geom", GlKind::F0Phase, {n_fft, hop, win, n_mels}, gl_host_batch(B, starts, lens), {workspace, workspace_bytes}, {},
             {0, 0.f, seed, nullptr}};
    c.spsi = {phase, nullptr};
    c.exc = {f0, f0_floor, f0_ceil, sample_rate};
    return gl_call(stream, c);
}

int fs2_op_f0_phase_dev(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* f0, int32_t B, const int64_t* lens_dev,
                        int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status, double f0_floor, double f0_ceil, int32_t sample_rate,
                        uint32_t seed, void* workspace, size_t workspace_bytes, float* phase) {
    GlCall c{"fs2_op_f0_phase_dev", GlKind::F0Phase, {n_fft, hop, win, n_mels}, gl_device_batch(B, lens_dev, src_stride, frame_capacity, upstream_status),
             {workspace, workspace_bytes}, {}, {0, 0.f, seed, nullptr}};
    c.spsi = {phase, nullptr};
    c.exc = {f0, f0_floor, f0_ceil, sample_rate};
    return gl_call(stream, c);
}

int fs2_op_excitation_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* f0, int32_t B, const int32_t* starts,
                           const int32_t* lens, double f0_floor, double f0_ceil, int32_t sample_rate, uint32_t seed, void* workspace,
                           size_t workspace_bytes, float* wav) {
    GlCall c{"fs2_op_excitation_geom", GlKind::F0Phase, {n_fft, hop, win, n_mels}, gl_host_batch(B, starts, lens), {workspace, workspace_bytes}, {},
             {0, 0.f, seed, nullptr}, {wav, 0, 0, nullptr, nullptr}};
    c.exc = {f0, f0_floor, f0_ceil, sample_rate};
    return gl_call(stream, c);
}

int fs2_op_excitation_dev(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* f0, int32_t B, const int64_t* lens_dev,
                          int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status, double f0_floor, double f0_ceil, int32_t sample_rate,
                          uint32_t seed, void* workspace, size_t workspace_bytes, float* wav, int32_t wav_stride, int64_t wav_capacity) {
    GlCall c{"fs2_op_excitation_dev", GlKind::F0Phase, {n_fft, hop, win, n_mels}, gl_device_batch(B, lens_dev, src_stride, frame_capacity, upstream_status),
             {workspace, workspace_bytes}, {}, {0, 0.f, seed, nullptr}, {wav, wav_stride, wav_capacity, nullptr, nullptr}};
    c.exc = {f0, f0_floor, f0_ceil, sample_rate};
    return gl_call(stream, c);
}

size_t fs2_op_stft_workspace_bytes(int32_t B, const int32_t* wav_lens) { return fs2_op_stft_workspace_bytes_geom(kGlNfft, kGlHop, kGlNfft, 80, B, wav_lens); }

size_t fs2_op_stft_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* wav_lens) {
    return gl_workspace_bytes({"fs2_op_stft_workspace_bytes_geom", GlKind::Analysis, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, wav_lens)});
}

int fs2_op_stft(void* stream, const float* wav, int32_t B, const int32_t* wav_starts, const int32_t* wav_lens, void* workspace,
                size_t workspace_bytes, float* mag, const float* mel_basis, float* logmel) {
    GlCall c{"fs2_op_stft", GlKind::Analysis, {kGlNfft, kGlHop, kGlNfft, 80}, gl_host_batch(B, wav_starts, wav_lens), {workspace, workspace_bytes}, {wav}};
    c.feat = {mag, mel_basis, logmel};
    return gl_call(stream, c);
}

int fs2_op_stft_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* wav, int32_t B, const int32_t* wav_starts, const int32_t* wav_lens,
                     void* workspace, size_t workspace_bytes, float* mag, const float* mel_basis, float* logmel, float* energy) {
    GlCall c{"fs2_op_stft_geom", GlKind::Analysis, {n_fft, hop, win, n_mels}, gl_host_batch(B, wav_starts, wav_lens), {workspace, workspace_bytes}, {wav}};
    c.feat = {mag, mel_basis, logmel, energy};
    return gl_call(stream, c);
}

size_t fs2_op_stft_pitch_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* wav_lens) {
    return gl_workspace_bytes({"fs2_op_stft_pitch_workspace_bytes_geom", GlKind::AnalysisPitch, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, wav_lens)});
}

int fs2_op_stft_pitch_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* wav, int32_t B, const int32_t* wav_starts,
                           const int32_t* wav_lens, void* workspace, size_t workspace_bytes, float* mag, const float* mel_basis, float* logmel, float* energy,
                           int32_t sample_rate, double f0_floor, double f0_ceil, double voicing_threshold, double octave_cost, float* f0, float* strength) {
    GlCall c{"fs2_op_stft_pitch_geom", GlKind::AnalysisPitch, {n_fft, hop, win, n_mels}, gl_host_batch(B, wav_starts, wav_lens), {workspace, workspace_bytes}, {wav}};
    c.feat = {mag, mel_basis, logmel, energy, {sample_rate, f0_floor, f0_ceil, voicing_threshold, octave_cost}, f0, strength};
    return gl_call(stream, c);
}

size_t fs2_op_stft_pitch_cands_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t* wav_lens) {
    return gl_workspace_bytes({"fs2_op_stft_pitch_cands_workspace_bytes_geom", GlKind::AnalysisPitch, {n_fft, hop, win, n_mels}, gl_host_batch(B, nullptr, wav_lens)});
}

int fs2_op_stft_pitch_cands_geom(void* stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float* wav, int32_t B, const int32_t* wav_starts,
                                 const int32_t* wav_lens, void* workspace, size_t workspace_bytes, float* mag, const float* mel_basis, float* logmel, float* energy,
                                 int32_t sample_rate, double f0_floor, double f0_ceil, double voicing_threshold, double octave_cost, int32_t n_candidates,
                                 float* cand_f0, float* cand_strength) {
    if (n_candidates < 1) return fail(nullptr, FS2_ERR_ARG, "fs2_op_stft_pitch_cands_geom: n_candidates = %d outside 1 .. %d", n_candidates, FS2_PITCH_MAX_CANDS);
    GlCall c{"fs2_op_stft_pitch_cands_geom", GlKind::AnalysisPitch, {n_fft, hop, win, n_mels}, gl_host_batch(B, wav_starts, wav_lens), {workspace, workspace_bytes}, {wav}};
    c.feat = {mag, mel_basis, logmel, energy, {sample_rate, f0_floor, f0_ceil, voicing_threshold, octave_cost}, nullptr, nullptr, n_candidates, cand_f0, cand_strength};
    return gl_call(stream, c);
}

size_t fs2_op_pitch_path_workspace_bytes(int32_t B, const int32_t* frame_lens) { return path_workspace_bytes(B, frame_lens); }

int fs2_op_pitch_path(void* stream, const fs2_op_pitch_path_args* a) { return pp_pitch_path(stream, a); }

size_t fs2_op_targets_workspace_bytes(int32_t B) { return tg_workspace_bytes(B); }

int fs2_op_clean_targets(void* stream, const float* x, int32_t B, const int32_t* starts, const int32_t* lens, void* workspace, size_t workspace_bytes,
                         float* y, float* quartiles, int32_t* n_outliers, double* stats) {
    return tg_clean_targets(stream, x, B, starts, lens, workspace, workspace_bytes, y, quartiles, n_outliers, stats);
}

size_t fs2_op_loss_workspace_bytes(int32_t B, const int32_t* olens) { return lt_workspace_bytes(B, olens); }

int fs2_op_loss_terms(void* stream, const fs2_op_loss_args* a) { return lt_loss_terms(stream, a); }

size_t fs2_op_dtw_workspace_bytes(int32_t B, const int32_t* a_lens, const int32_t* b_lens, size_t cap_bytes) {
    return dtw_workspace_bytes(B, a_lens, b_lens, cap_bytes);
}

int fs2_op_dtw(void* stream, const fs2_op_dtw_args* a) { return dt_dtw(stream, a); }

size_t fs2_op_align_workspace_bytes(int32_t B, const int32_t* a_lens, const int32_t* b_lens, size_t cap_bytes) {
    return align_workspace_bytes(B, a_lens, b_lens, cap_bytes);
}

int fs2_op_align(void* stream, const fs2_op_align_args* a) { return al_align(stream, a); }

int fs2_op_label_means(void* stream, const float* x, const int32_t* labels, const int64_t* lens_dev, int32_t B, int32_t x_stride, int32_t n_labels,
                       int32_t positive_only, float* mean, int32_t* count) {
    return pr_label_means(stream, x, labels, lens_dev, B, x_stride, n_labels, positive_only, mean, count);
}

}  // extern "C"
