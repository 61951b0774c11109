// The pitch path search: per utterance, the best sequence of states through the K candidates per frame that gl_candidates
// (gl_pitch.h) or anything else supplies -- behind fs2_op_pitch_path (include/fs2.h; DESIGN.md section 14.11;
// tests/pitch_path_oracle.py states the same in numpy).  Not a header of its own: fs2_runtime.hip includes it inside its unnamed
// namespace (fail(), align_up()).  Plain HIP C++, restricted to what tests/kernel_standin/hip_standin.h provides plus an indexed
// __shfl (tests/kernel_standin/pitch_path_main.cpp defines it).
//
// The definition.  State 0 is "unvoiced", state c = 1 .. K is candidate c - 1 of the frame, which exists iff cand_f0 > 0.  All in
// double, from the float32 inputs, no contraction:
//   u(t, 0) = voicing_threshold;  u(t, c) = p - octave_cost * log2(f0_floor / f);  lg(t, c) = log2(f)
//   trans(j -> c) = 0 (both unvoiced) | vu (exactly one unvoiced) | oj * |lg(t-1, j) - lg(t, c)| (both voiced)
//   vu = voiced_unvoiced_cost * s, oj = octave_jump_cost * s, s = 0.01 / time_step        (formed once, on the host)
//   D(0, c) = u(0, c);  D(t, c) = u(t, c) + max over the existing j = 0, 1, .. of [D(t-1, j) - trans(j -> c)], a strict ">": a tie
//   keeps the smaller j.  The end state is the largest D(T-1, c), a tie to the smaller c; then the walk back.
// A missing state carries u = D = -inf.  State 0 always exists and its D is finite, every comparison starts from it and is a
// strict ">", so a missing state is never chosen -- the same choices as never comparing it.
//
// pitch_path: one wave per utterance, lane c <= K owns state c; the lanes beyond K repeat state 0 (every lane takes part in every
// shuffle) and write nothing.  The frames go through LDS in chunks of kPathChunk.  Forward, per chunk: all lanes load the chunk's
// candidates coalesced and form u and lg (the only log2 calls), lane fr finds frame fr's own argmax of u; then the sequential loop,
// which per frame reads u and lg from LDS, fetches the K + 1 previous D by shuffle and leaves its back pointer (4 bits) in LDS;
// then lane fr packs frame fr's nine back pointers and the frame's argmax (nibble 9) into one 64-bit word and the chunk's words go
// to the workspace coalesced.  Only D is carried from frame to frame.  Backward, per chunk from the last: the words come back into
// LDS coalesced, lane 0 walks inside the chunk (one LDS read per frame, no global load on the chain), then lane fr writes frame
// fr's f0, state and strength and counts.  The counts are integers and a maximum: their order of combination changes nothing.
// No atomics, nothing waits on another workgroup, every loop is bounded by T, K or the chunk.  A back pointer is at most K by
// construction and is clamped to K where it is read, so whatever the inputs hold every access stays in the utterance's own rows.
//
// records_combine<8, 1, 5> (record_op.h; one workgroup): copies the records out and forms the batch record over the utterances in index
// order -- column 1 counts the refused utterances, column 5 is the maximum and the others are sums over the rest.

#include "record_op.h"
constexpr int kPathChunk = 64;                          // frames staged in LDS at a time (= the lanes of the wave)
constexpr int kPathStates = FS2_PITCH_MAX_CANDS + 1;
constexpr int kPathTerms = FS2_PITCH_PATH_TERMS;
constexpr int kPathUttsPerLaunch = 128;                 // utterances whose rows travel with one launch, as kernel arguments
static_assert(FS2_PITCH_MAX_CANDS == 8 && FS2_PITCH_PATH_TERMS == 8, "word and record layout of include/fs2.h");
static_assert(4 * (kPathStates + 1) <= 64 && kPathStates < 16, "nine back pointers and the frame's argmax, 4 bits each, in one word");

struct PathUtt { int row0, T; int64_t word0; };         // first row and frames of the utterance; its first word in the workspace
struct PathBatch { int n, base; PathUtt u[kPathUttsPerLaunch]; };
static_assert(sizeof(PathUtt) == 16 && sizeof(PathBatch) < 4096, "the utterances travel as kernel arguments");
struct PathCosts { double f0_floor, threshold, octave_cost, oj, vu; };

__global__ __launch_bounds__(kPathChunk) void pitch_path(PathBatch pb, int K, PathCosts pc, const float* cand_f0, const float* cand_p,
                                                         uint64_t* words, float* f0, int32_t* state, float* strength, double* recs) {
#pragma clang fp contract(off)
    constexpr int C = kPathChunk, NS = kPathStates;
    __shared__ double su[C * NS];                       // u of the chunk's frames
    __shared__ double slg[(C + 1) * NS];                // lg: slot 0 is the frame before the chunk, slot fr + 1 frame fr
    __shared__ unsigned char sbp[C * 16];               // back pointers of the chunk, 16 per frame
    __shared__ uint64_t sw[C];                          // the chunk's words (backward)
    __shared__ int sst[C + 1];                          // the chunk's states, then the state of the frame after it (backward)
    const int lane = threadIdx.x;
    const PathUtt ut = pb.u[blockIdx.x];
    const int T = ut.T;
    const int64_t row0 = ut.row0;
    double* out = recs + (size_t)(pb.base + blockIdx.x) * kPathTerms;
    if (T < 1) {
        if (lane < kPathTerms) out[lane] = 0.0;
        return;
    }
    const bool own = lane <= K;
    const int cs = own ? lane : 0;
    const double inf = __builtin_huge_val();
    const float inff = __builtin_huge_valf();
    const float* cf = cand_f0 + row0 * K;
    const float* cp = cand_p + row0 * K;
    uint64_t* wd = words + ut.word0;
    double D = 0.0;
    int bad = 0;
    for (int t0 = 0; t0 < T; t0 += C) {
        const int n = min(C, T - t0);
        for (int i = lane; i < n * K; i += C) {
            const int fr = i / K, k = i - fr * K;
            const float f = cf[(int64_t)t0 * K + i], p = cp[(int64_t)t0 * K + i];
            bad |= !(f >= 0.f && f < inff && p >= 0.f && p < inff);
            const bool ex = f > 0.f;
            su[fr * NS + k + 1] = ex ? (double)p - pc.octave_cost * log2(pc.f0_floor / (double)f) : -inf;
            slg[(fr + 1) * NS + k + 1] = ex ? log2((double)f) : 0.0;
        }
        if (lane < n) {
            su[lane * NS] = pc.threshold;
            slg[(lane + 1) * NS] = 0.0;
        }
        __syncthreads();
        int am = 0;                                     // frame `lane`'s own argmax of u: ascending, strict ">"
        if (lane < n) {
            double b = su[lane * NS];
            for (int k = 1; k <= K; ++k) {
                const double v = su[lane * NS + k];
                if (v > b) { b = v; am = k; }
            }
        }
        for (int fr = 0; fr < n; ++fr) {
            const double myu = su[fr * NS + cs], mylg = slg[(fr + 1) * NS + cs];
            int bj = 0;
            if (t0 + fr == 0) {
                D = myu;
            } else {
                const double* plg = slg + fr * NS;      // lg of the frame before
                double best = __shfl(D, 0) - (cs == 0 ? 0.0 : pc.vu);
                for (int j = 1; j <= K; ++j) {
                    const double Dj = __shfl(D, j);
                    const double tr = cs == 0 ? pc.vu : pc.oj * fabs(plg[j] - mylg);
                    const double v = Dj - tr;
                    if (v > best) { best = v; bj = j; }
                }
                D = myu + best;
            }
            if (own) sbp[fr * 16 + lane] = (unsigned char)bj;
        }
        __syncthreads();
        if (lane < n) {
            uint64_t w = (uint64_t)am << (4 * NS);
            for (int k = 0; k <= K; ++k) w |= (uint64_t)sbp[lane * 16 + k] << (4 * k);
            wd[t0 + lane] = w;
        }
        if (lane < NS) slg[lane] = slg[n * NS + lane];  // the next chunk's "frame before"
        __syncthreads();
    }
    // the end state: the largest D(T-1, c), a tie to the smaller c
    double eD = own ? D : -inf;
    int ec = lane;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double oD = __shfl_xor(eD, o);
        const int oc = __shfl_xor(ec, o);
        bad |= __shfl_xor(bad, o);
        if (oD > eD || (oD == eD && oc < ec)) { eD = oD; ec = oc; }
    }
    if (bad) {                                          // (every lane alike)
        for (int t = lane; t < T; t += C) {
            if (f0) f0[row0 + t] = 0.f;
            if (state) state[row0 + t] = -1;
            if (strength) strength[row0 + t] = 0.f;
        }
        if (lane < kPathTerms) out[lane] = lane == 0 ? (double)T : lane == 1 ? 2.0 : 0.0;
        return;
    }
    int s = min(ec, K);                                 // lane 0's: the state of the frame the walk stands at
    int nv = 0, nsw = 0, nch = 0;
    double mx = 0.0;
    for (int t0 = (T - 1) / C * C; t0 >= 0; t0 -= C) {
        const int n = min(C, T - t0);
        if (lane < n) sw[lane] = wd[t0 + lane];
        __syncthreads();
        if (lane == 0) {
            const int after = sst[0];                   // the first state of the chunk walked before this one (unused for the last chunk)
            for (int fr = n - 1; fr >= 0; --fr) {
                sst[fr] = s;
                s = min((int)((sw[fr] >> (4 * s)) & 15), K);
            }
            sst[n] = after;
        }
        __syncthreads();
        if (lane < n) {
            const int t = t0 + lane, c = sst[lane];
            const bool v = c > 0;
            const float f = v ? cf[(int64_t)t * K + c - 1] : 0.f, p = v ? cp[(int64_t)t * K + c - 1] : 0.f;
            if (f0) f0[row0 + t] = f;
            if (state) state[row0 + t] = c - 1;
            if (strength) strength[row0 + t] = p;
            nv += v;
            nch += c != (int)((sw[lane] >> (4 * NS)) & 15);
            if (t + 1 < T) {
                const int c2 = sst[lane + 1];
                nsw += v != (c2 > 0);
                if (v && c2 > 0) {
                    const double step = fabs(log2((double)f) - log2((double)cf[(int64_t)(t + 1) * K + c2 - 1]));
                    if (step > mx) mx = step;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        nv += __shfl_xor(nv, o);
        nsw += __shfl_xor(nsw, o);
        nch += __shfl_xor(nch, o);
        const double om = __shfl_xor(mx, o);
        if (om > mx) mx = om;
    }
    if (lane == 0) {
        out[0] = (double)T; out[1] = 0.0; out[2] = eD; out[3] = (double)nv;
        out[4] = (double)nsw; out[5] = mx; out[6] = (double)nch; out[7] = 0.0;
    }
}

// ---- host side: workspace = one record per utterance, then one word per frame ----
struct PathRegions { double* recs; uint64_t* words; size_t bytes; int64_t frames; };

// false: a negative B or length, or null lens with B > 0
inline bool path_regions(int32_t B, const int32_t* lens, void* ws, PathRegions& r) {
    if (B < 0 || (B > 0 && !lens)) return false;
    int64_t frames = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0) return false;
        frames += lens[b];
    }
    Carve c{(char*)ws};
    r = PathRegions{c.take<double>(B, kPathTerms), c.take<uint64_t>(frames), 0, frames};
    r.bytes = c.off;
    return true;
}

size_t path_workspace_bytes(int32_t B, const int32_t* frame_lens) {
    PathRegions r;
    return path_regions(B, frame_lens, nullptr, r) ? r.bytes : 0;
}

int pp_pitch_path(void* stream, const fs2_op_pitch_path_args* a) {
    const char* who = "fs2_op_pitch_path";
    if (const int rc = rec_check_struct(who, "fs2_op_pitch_path_args", a)) return rc;
    const int32_t B = a->B, K = a->n_candidates;
    if (K < 1 || K > FS2_PITCH_MAX_CANDS) return fail(nullptr, FS2_ERR_ARG, "%s: n_candidates = %d outside 1 .. %d", who, K, FS2_PITCH_MAX_CANDS);
    if (!(a->time_step > 0.0) || !std::isfinite(a->time_step) || !(a->f0_floor > 0.0) || !std::isfinite(a->f0_floor))
        return fail(nullptr, FS2_ERR_ARG, "%s: time_step %g and f0_floor %g must be positive and finite", who, a->time_step, a->f0_floor);
    if (!std::isfinite(a->voicing_threshold) || !std::isfinite(a->octave_cost))
        return fail(nullptr, FS2_ERR_ARG, "%s: voicing_threshold %g and octave_cost %g must be finite", who, a->voicing_threshold, a->octave_cost);
    if (!(a->octave_jump_cost >= 0.0) || !std::isfinite(a->octave_jump_cost) || !(a->voiced_unvoiced_cost >= 0.0) || !std::isfinite(a->voiced_unvoiced_cost))
        return fail(nullptr, FS2_ERR_ARG, "%s: octave_jump_cost %g and voiced_unvoiced_cost %g must be finite and not negative", who, a->octave_jump_cost,
                    a->voiced_unvoiced_cost);
    PathRegions l;                                      // (B = 0: no workspace, and nothing is launched that reads a region)
    if (!path_regions(B, a->frame_lens, a->workspace, l) || (B > 0 && !a->frame_starts))
        return fail(nullptr, FS2_ERR_ARG, "%s: bad batch (B = %d, a negative or missing length or start)", who, B);
    for (int b = 0; b < B; ++b)
        if (a->frame_starts[b] < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative start of utterance %d", who, b);
    if (l.frames * K > INT32_MAX) return fail(nullptr, FS2_ERR_UNSUPPORTED, "%s: %lld frames of %d candidates", who, (long long)l.frames, K);
    hipStream_t s = (hipStream_t)stream;
    if (l.frames > 0 && (!a->cand_f0 || !a->cand_strength)) return fail(nullptr, FS2_ERR_ARG, "%s: null candidates", who);
    if (const int rc = rec_check_workspace(who, B, a->workspace, a->workspace_bytes, l.bytes)) return rc;
    const double scale = 0.01 / a->time_step;
    const PathCosts pc{a->f0_floor, a->voicing_threshold, a->octave_cost, a->octave_jump_cost * scale, a->voiced_unvoiced_cost * scale};
    int64_t word0 = 0;
    for (int base = 0; base < B; base += kPathUttsPerLaunch) {
        PathBatch pb;
        pb.n = std::min(kPathUttsPerLaunch, B - base);
        pb.base = base;
        for (int i = 0; i < pb.n; ++i) {
            pb.u[i] = PathUtt{a->frame_starts[base + i], a->frame_lens[base + i], word0};
            word0 += a->frame_lens[base + i];
        }
        hipLaunchKernelGGL(pitch_path, dim3((unsigned)pb.n), dim3(kPathChunk), 0, s, pb, K, pc, a->cand_f0, a->cand_strength, l.words, a->f0, a->state,
                           a->strength, l.recs);
    }
    if (a->terms || a->batch) hipLaunchKernelGGL((records_combine<kPathTerms, 1, 5>), dim3(1), dim3(256), 0, s, l.recs, B, a->terms, a->batch);
    return rec_finish(who);
}
