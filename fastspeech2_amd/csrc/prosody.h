// Pitch and energy control of the free-running synthesis, and per-phoneme means of a per-frame track -- behind fs2_decode_ctl and
// fs2_op_label_means (include/fs2.h; tests/prosody_oracle.py states both in numpy).  Not a header of its own:
// fs2_runtime.hip includes it inside its unnamed namespace (fail()).  Plain HIP C++, restricted to what
// tests/kernel_standin/hip_standin.h provides.
//
// prosody_apply: one thread per packed frame row, between the variance predictors and the two consumers of their outputs
// (bucket_embed, dec_in_gather).  For a row of utterance b = row_seq[row] that was expanded from phoneme t = lri[row]:
//     v' = fadd_rn(fmul_rn(v, scale), shift),  scale = scale_ptr ? scale_ptr[b * cols_s + (cols_s == 1 ? 0 : t)] : 1,
//                                              shift = shift_ptr ? shift_ptr[b * cols_h + (cols_h == 1 ? 0 : t)] : 0
// for the pitch row and the energy row alike, in place.  The product and the sum are rounded one after the other: contraction is
// switched off where they are formed, and they are written with the plain operators (hipcc contracts a * b + c into one fused
// operation by default; its __fmul_rn / __fadd_rn are inline functions around the plain operators, compiled under that default,
// so after inlining they are contracted even inside a contract(off) region -- the ISA showed v_fmac_f32 -- and the fused result
// differs from a float32 restatement in the last bit; see also targets.h).  Gap rows (row_pos < 0) and rows without a phoneme (t < 0) are left alone.  A track without control (both pointers
// NULL) is neither read nor written.
//
// label_means: one thread per (utterance b, label t).  The labels of the valid frames [0, min(lens[b], x_stride)) are non-decreasing,
// so the frames of label t are one run, found by a lower and an upper bound; its values are added in frame order in a double.
// No atomics, no LDS; the searches halve an interval inside the utterance's own frames and the sum runs over a part of it, so
// whatever the labels hold nothing outside [0, lens[b]) of the utterance's own row is read and every loop ends.

struct ProsodyTrack {           // the control of one track: device [B, cols] each, cols 1 or Tmax; NULL = neutral
    const float *scale, *shift;
    int scale_cols, shift_cols;
};

__device__ inline float prosody_value(float v, const ProsodyTrack& c, int b, int t) {
#pragma clang fp contract(off)
    const float scale = c.scale ? c.scale[(size_t)b * c.scale_cols + (c.scale_cols == 1 ? 0 : t)] : 1.0f;
    const float shift = c.shift ? c.shift[(size_t)b * c.shift_cols + (c.shift_cols == 1 ? 0 : t)] : 0.0f;
    const float scaled = v * scale;                                        // rounded to float32 ...
    return scaled + shift;                                                 // ... and rounded again
}

// B, Tmax: the extents of the control tensors -- a row whose utterance or phoneme lies outside them is left alone
__global__ __launch_bounds__(256) void prosody_apply(float* p_rows, float* e_rows, const int* row_pos, const int* row_seq, const int* lri, int R,
                                                     int B, int Tmax, ProsodyTrack pitch, ProsodyTrack energy) {
    const int row = (int)(blockIdx.x * 256 + threadIdx.x);
    if (row >= R || row_pos[row] < 0) return;
    const int t = lri[row], b = row_seq[row];
    if (t < 0 || t >= Tmax || b < 0 || b >= B) return;
    if (pitch.scale || pitch.shift) p_rows[row] = prosody_value(p_rows[row], pitch, b, t);
    if (energy.scale || energy.shift) e_rows[row] = prosody_value(e_rows[row], energy, b, t);
}

__global__ __launch_bounds__(256) void label_means(const float* x, const int32_t* labels, const int64_t* lens, int B, int x_stride, int n_labels,
                                                   int positive_only, float* mean, int32_t* count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * n_labels) return;
    const int b = (int)(i / n_labels), t = (int)(i - (int64_t)b * n_labels);
    const int64_t len = lens[b];
    const int n = len < 0 ? 0 : len > x_stride ? x_stride : (int)len;
    const int32_t* lab = labels + (size_t)b * x_stride;
    const float* xb = x + (size_t)b * x_stride;
    int lo = 0, hi = n;                                                    // first frame whose label is >= t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (lab[mid] < t) lo = mid + 1; else hi = mid;
    }
    const int first = lo;
    hi = n;                                                                // first frame behind it whose label is > t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (lab[mid] <= t) lo = mid + 1; else hi = mid;
    }
    double sum = 0.0;
    int32_t cnt = 0;
    for (int j = first; j < lo; ++j) {
        const float v = xb[j];
        if (!positive_only || v > 0.0f) { sum += (double)v; ++cnt; }
    }
    mean[i] = cnt ? (float)(sum / (double)cnt) : 0.0f;
    count[i] = cnt;
}

// ---- host side ----
int pr_label_means(void* stream, const float* x, const int32_t* labels, const int64_t* lens_dev, int32_t B, int32_t x_stride, int32_t n_labels,
                   int32_t positive_only, float* mean, int32_t* count) {
    const char* who = "fs2_op_label_means";
    if (B < 0 || x_stride < 0 || n_labels < 0) return fail(nullptr, FS2_ERR_ARG, "%s: negative B = %d, x_stride = %d or n_labels = %d", who, B, x_stride, n_labels);
    if (B == 0) return FS2_OK;
    if (!lens_dev) return fail(nullptr, FS2_ERR_ARG, "%s: null lens", who);
    if (x_stride > 0 && (!x || !labels)) return fail(nullptr, FS2_ERR_ARG, "%s: null x / labels", who);
    if (n_labels > 0 && (!mean || !count)) return fail(nullptr, FS2_ERR_ARG, "%s: null mean / count", who);
    const int64_t total = (int64_t)B * n_labels;
    if (total > INT32_MAX) return fail(nullptr, FS2_ERR_ARG, "%s: B * n_labels = %lld beyond 2^31 - 1", who, (long long)total);
    if (total == 0) return FS2_OK;
    hipLaunchKernelGGL(label_means, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, labels, lens_dev, B, x_stride, n_labels,
                       positive_only, mean, count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return FS2_OK;
}
