// The scaffold of the record operators -- fs2_op_clean_targets (targets.h), fs2_op_loss_terms (losses.h), fs2_op_dtw (dtw.h),
// fs2_op_align (align.h), fs2_op_pitch_path (pitch_path.h); DESIGN.md section 7.6 -- ONCE.  Each of them checks a caller-filled batch of
// (start, length) rows, carves a caller workspace, sends per-utterance records to the device as kernel arguments (no copy, no
// synchronisation), runs one workgroup per utterance, pair or tile that writes a record of doubles, folds the records into a batch
// record in index order, and ends on hipGetLastError.  What they share stands here: the argument checks, the workspace carve, the
// record upload and the plain combine.  Not a header of its own: the operator headers include it inside the includer's unnamed
// namespace, after fail() and align_up().  Restricted to what tests/kernel_standin/hip_standin.h provides; the first half is plain
// C++ (tests/pair_plan_probe.cpp compiles it through pair_plan.h with the host compiler alone).
#pragma once

// ---- argument checks.  The one wording of a struct_size refusal (ABI_CHECK of fs2_runtime.hip formats with it too): who, type, got, ABI, expected
#define FS2_STRUCT_SIZE_FMT "%s: %s.struct_size is %u but this library (ABI %d) expects %zu: the binding does not match include/fs2.h"
template <class Args> int rec_check_struct(const char* who, const char* type, const Args* a) {
    if (!a) return fail(nullptr, FS2_ERR_ARG, "%s: null argument", who);
    if (a->struct_size != (uint32_t)sizeof(Args)) return fail(nullptr, FS2_ERR_ARG, FS2_STRUCT_SIZE_FMT, who, type, (unsigned)a->struct_size, FS2_ABI_VERSION, sizeof(Args));
    return FS2_OK;
}
// starts and lengths are non-negative and every row index stays below 2^31 (`what`: "utterance", "pair")
inline int rec_check_rows(const char* who, const char* what, int32_t B, const int32_t* starts, const int32_t* lens) {
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative length of %s %d", who, what, b);
        if (starts[b] < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative start of %s %d", who, what, b);
        if ((int64_t)starts[b] + lens[b] > INT32_MAX) return fail(nullptr, FS2_ERR_ARG, "%s: %s %d ends beyond 2^31 - 1 rows", who, what, b);
    }
    return FS2_OK;
}
// a batch that launches anything needs its workspace, and `need` bytes of it (`note`: what `need` stands for, or "")
inline int rec_check_workspace(const char* who, int32_t B, const void* workspace, size_t have, size_t need, const char* note = "") {
    if (B > 0 && !workspace) return fail(nullptr, FS2_ERR_ARG, "%s: null workspace", who);
    if (B > 0 && have < need) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes%s", who, have, need, note);
    return FS2_OK;
}

// ---- workspace: an operator states its regions once, in a function of a Carve; the *_workspace_bytes query walks it over no workspace
// (every pointer null, `off` the size) and the operator over the caller's.  Regions are 256-byte aligned; an empty batch is sized as one element.
struct Carve {
    char* base;
    size_t off = 0;
    template <class T> T* take(int64_t n, size_t per = 1) {      // n items of `per` T each
        T* p = base ? (T*)(base + off) : nullptr;
        off = align_up(off + (size_t)std::max<int64_t>(n, 1) * per * sizeof(T), 256);
        return p;
    }
};

// ---- upload: the records [base, base + n) of a batch travel as the argument of one launch ----
template <class Rec, int N> struct RecChunk { int n, base; Rec r[N]; };
// put(i, rec) for i = 0 .. B - 1 in order -> launch(chunk) when a chunk is full or the batch ends: ceil(B / N) calls
template <class Rec, int N, class Launch> struct RecChunker {
    static_assert(sizeof(RecChunk<Rec, N>) < 4096, "the records travel as kernel arguments");
    int B;
    Launch launch;                 // launch(const RecChunk<Rec, N>&)
    RecChunk<Rec, N> c{};          // (entries beyond n keep an earlier chunk's records: nobody reads them)
    void put(int i, const Rec& rec) {
        const int k = i % N;
        c.r[k] = rec;
        if (k + 1 == N || i + 1 == B) { c.n = k + 1; c.base = i - k; launch(c); }
    }
};
template <class Rec, int N, class Launch> RecChunker<Rec, N, Launch> rec_chunker(int B, Launch launch) { return {B, launch}; }

#ifdef __global__      // ---- the device half: under hipcc and on the stand-in (both define __global__), not under a plain host compiler ----
template <class Rec, int N> __global__ void upload_recs(RecChunk<Rec, N> c, Rec* dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c.n) dst[c.base + i] = c.r[i];
}
template <class Rec, int N> auto upload_launch(Rec* dst, hipStream_t s) {      // the launch of one chunk
    return [=](const RecChunk<Rec, N>& c) { hipLaunchKernelGGL((upload_recs<Rec, N>), dim3((N + 255) / 256), dim3(256), 0, s, c, dst); };
}
template <class Rec, int N> auto rec_uploader(int B, Rec* dst, hipStream_t s) { return rec_chunker<Rec, N>(B, upload_launch<Rec, N>(dst, s)); }

// One workgroup copies the B records of TERMS doubles out and forms the batch record over them in index order: thread tid < TERMS owns
// column tid.  Without FLAG (-1) a column is the plain sum.  With it, a record is fine iff its column FLAG is 0.0: column FLAG counts the
// records that are not, and every other column runs over the fine ones only -- a sum, or for column MAXCOL (-1: none) the maximum, from 0.0.
template <int TERMS, int FLAG, int MAXCOL> __global__ __launch_bounds__(256) void records_combine(const double* recs, int B, double* terms, double* batch) {
    const int tid = threadIdx.x;
    if (terms)
        for (int64_t i = tid; i < (int64_t)B * TERMS; i += 256) terms[i] = recs[i];
    if (batch && tid < TERMS) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) {
            const double v = recs[(size_t)b * TERMS + tid];
            if constexpr (FLAG < 0) s += v;
            else {
                const bool fine = recs[(size_t)b * TERMS + FLAG] == 0.0;
                if (tid == FLAG) s += fine ? 0.0 : 1.0;
                else if (fine && tid == MAXCOL) s = v > s ? v : s;
                else if (fine) s += v;
            }
        }
        batch[tid] = s;
    }
}

inline int rec_finish(const char* who) {      // the tail of every operator
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FS2_OK : fail(nullptr, FS2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
}
#endif
