/*
 * fs2.h -- C ABI of libfs2_hip.so: the MI355X (gfx950) FastSpeech2 mel-generation forward pass.
 *
 * The reference (rishikksh20/FastSpeech2) has no FFI: its hot path sits behind a Python
 * torch.nn.Module, `fastspeech.FeedForwardTransformer` (reference fastspeech.py:28).  This header is
 * the boundary a maintainer of the reference would bind (ctypes stub in INTEGRATION.md) to replace the
 * tensor work inside `_forward` (fastspeech.py:169-243) -- encoder/decoder FFT blocks
 * (core/encoder.py:46-71,185-204; core/attention.py:30-74; core/modules.py:237-248), duration / pitch /
 * energy predictors (core/duration_modeling/duration_predictor.py:64-86; core/variance_predictor.py:39-60,
 * 154-159), length regulator (core/duration_modeling/length_regulator.py:38-95) and Postnet
 * (core/modules.py:350-359) -- with hand-written HIP kernels.
 *
 * Conventions: plain pointers and sizes only (no torch types); every function returns 0 or a negative
 * FS2_ERR_* code and never throws; `fs2_last_error` gives the message.  "device" pointers are HIP device
 * memory on the handle's device, "host" pointers are ordinary host memory.  All launches go to the
 * caller's hipStream_t (passed as void*); no function allocates device memory except fs2_create /
 * fs2_load_weights (weight storage).  A handle is bound to one device and is not thread-safe.
 *
 * A forward pass is two calls, because the number of mel frames is data dependent:
 *   fs2_encode  : phoneme ids -> encoder -> duration predictor -> frame counts (olens, device)
 *   (caller reads olens back: the one unavoidable host sync of the path)
 *   fs2_decode  : length regulator -> pitch/energy -> decoder -> mel projection -> Postnet
 */
#ifndef FS2_H_
#define FS2_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_OK 0
#define FS2_ERR_ARG (-1)         /* bad argument / shape                                   */
#define FS2_ERR_HIP (-2)         /* a HIP runtime call failed                              */
#define FS2_ERR_STATE (-3)       /* call order violated (e.g. decode before encode)        */
#define FS2_ERR_WEIGHT (-4)      /* a required tensor is missing or has the wrong shape    */
#define FS2_ERR_WORKSPACE (-5)   /* workspace too small                                    */
#define FS2_ERR_UNSUPPORTED (-6) /* configuration outside what the kernels implement       */

/* arithmetic modes of the GEMM-shaped kernels */
#define FS2_PREC_FP32 0   /* f32-input MFMA (v_mfma_f32_16x16x4_f32), exact fp32            */
#define FS2_PREC_BF16X3 1 /* split-bf16: hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 */
#define FS2_PREC_BF16 2   /* plain bf16 inputs, fp32 accumulate                             */
/* mixed modes: as FS2_PREC_BF16X3, except that the FFN convolution w_1 (the dominant kernel) runs on fp16
 * operands (v_mfma_f32_16x16x32_f16): activations split hi + lo, weights rounded to fp16 once (2 MFMAs per
 * fragment pair), or both operands rounded once (1 MFMA).  Measured error / speed: BASELINE.md section 4. */
#define FS2_PREC_MIX_F16X2 3
#define FS2_PREC_MIX_F16X1 4
/* as FS2_PREC_BF16X3, except that the 9-tap FFN convolution computes a.w = ah.wh (fp16 MFMA) + ra.wh + ah.rw (block-scaled
 * fp8 MFMA, v_mfma_scale_f32_16x16x128_f8f6f4): ~2.2 MFMA-equivalents per product at split-bf16-class accuracy */
#define FS2_PREC_MIX_MX 5
/* as FS2_PREC_MIX_MX with both cross terms of the decoder's FFN convolution in block-scaled fp4 (e2m1; one E8M0 scale per 16-channel block of a frame / of a weight row and tap):
 * 1.5 MFMA-equivalents per product.  Applies where the decoder's activations travel as planes only (big frame-level regimes: gemm_row4_bf16
 * produces the operand with its row scales); everywhere else the mode IS FS2_PREC_MIX_MX.  Measured error / speed: BASELINE.md section 4. */
#define FS2_PREC_MIX_MX4 6

typedef struct fs2_handle fs2_handle;

/* ABI revision of this header.  The four structs that are the argument of an entry point -- fs2_config, fs2_encode_io,
 * fs2_decode_io, fs2_op_gemm_args -- start with `struct_size`, which the library compares with its own sizeof: a caller
 * built against a different revision gets FS2_ERR_ARG (and a message naming both sizes) instead of fields read at the
 * wrong offsets.  Two structs carry no size field: `fs2_batch`, embedded in the io structs and so covered by their check
 * and passed alone only to the workspace-size / row-capacity queries, and `fs2_tensor_desc`, the array elements handed to
 * fs2_load_weights.  Their layout is frozen within a revision: any change to them bumps FS2_ABI_VERSION, and a binding
 * compares its own FS2_ABI_VERSION with fs2_abi_version() before the first call (fastspeech2_amd/_lib.py: lib();
 * csrc/fs2_torch_op.cpp: check_abi()). */
#define FS2_ABI_VERSION 4
int32_t fs2_abi_version(void);

/* Model hyper-parameters: the hp.model / hp.data fields FeedForwardTransformer.__init__ reads
 * (reference fastspeech.py:53-160). */
typedef struct fs2_config {
    uint32_t struct_size;               /* = sizeof(fs2_config): checked by fs2_create (FS2_ERR_ARG on mismatch), so a
                                           binding compiled against another revision of this header is rejected, not misread */
    int32_t idim, odim;                 /* phoneme symbols (68), mel bins (80)               */
    int32_t adim, aheads, elayers, eunits;
    int32_t ddim, dlayers, dunits;
    int32_t ffn_kernel;                 /* positionwise_conv_kernel_size; 1 for "linear"      */
    int32_t dur_layers, dur_chans, dur_kernel;   /* duration predictor (from hp)              */
    int32_t var_layers, var_chans, var_kernel;   /* pitch/energy predictors (hard-wired 2/256/3,
                                                    reference variance_predictor.py:125,198)   */
    int32_t n_bins;                     /* 256 quantisation levels                            */
    int32_t postnet_layers, postnet_chans, postnet_filts, use_batch_norm;
    int32_t use_scaled_pos_enc;
    int32_t reduction_factor;           /* r in [1, 8]: feat_out emits r mel frames per decoder frame; the mel outputs
                                           (before / after) then hold Lmax * r frames and after_packed r * sum(olens) rows */
    int32_t device;                     /* HIP device ordinal                                 */
    int32_t decoder_input_layer;        /* 1: Linear -> LN -> ReLU -> +pe (fastspeech.py:120-135, encoder.py:118-125);
                                           0: +pe only (the TorchScript twin, utils/fastspeech2_script.py:112-127;
                                           needs ddim == adim)                                */
    /* FFT-block variants (reference core/encoder.py:53-71,201-202; hp.model.{encoder,decoder}_{normalize_before,concat_after}) */
    int32_t enc_normalize_before, dec_normalize_before;   /* LayerNorm in front of the sub-layers + after_norm at the end */
    int32_t enc_concat_after, dec_concat_after;           /* x + concat_linear(cat(x, self_attn(x))) instead of x + self_attn(x) */
} fs2_config;

/* One reference-layout tensor (state_dict entry), fp32, resident on the device. */
typedef struct fs2_tensor_desc {
    const char *name;   /* e.g. "decoder.encoders_.0.feed_forward.w_1.weight" */
    const void *data;   /* device pointer, contiguous, float32                 */
    int32_t ndim;
    int64_t shape[4];
} fs2_tensor_desc;

/* Host-side description of a batch (lengths are host data: the reference also reads them on the host,
 * utils/util.py:263-264). */
typedef struct fs2_batch {
    int32_t B;              /* utterances                                                      */
    int32_t Tmax;           /* padded phoneme length of xs                                      */
    const int64_t *ilens;   /* host [B] phoneme counts                                          */
    int32_t compat_padded;  /* 0: per-utterance semantics (batch invariant; what inference()
                               computes).  1: reproduce the reference's padded-batch numerics
                               (conv / unmasked attention see the pad rows)      */
    int32_t precision;      /* FS2_PREC_*                                                      */
    /* Kernel-variant regime (ABI 4).  Some launches exist in variants that sum in different orders (LayerNorm fused into the
     * row-complete GEMM or not, deterministic split-K, the 32- or the 64-query attention kernel); which one runs is a function
     * of the SIZE of the batch only -- of these two numbers, never of a capacity or of the data.  0 / 0 = this call's own batch
     * (sum of ilens, B).  A caller that runs a SHARD of a larger batch (one rank of the multi-GPU split, a batch cut into
     * pieces) passes the WHOLE batch's numbers on every piece: every utterance is then computed by exactly the kernels the
     * one-call run of the whole batch uses, and its result is bit-identical to that run's (SURVEY.md section 8e's criterion;
     * the per-utterance semantics of reference fastspeech.py:169-243).  Both numbers must be given together. */
    int64_t regime_tokens;      /* phonemes of the batch the variants are chosen for (0: sum of ilens)  */
    int32_t regime_utterances;  /* utterances of that batch (0: B)                                      */
} fs2_batch;

typedef struct fs2_encode_io {
    uint32_t struct_size;     /* = sizeof(fs2_encode_io); fs2_encode returns FS2_ERR_ARG on mismatch         */
    fs2_batch batch;
    const int64_t *xs;        /* device [B, Tmax] phoneme ids (0 = pad)                         */
    const int64_t *ds;        /* device [B, Tmax] durations to use (teacher forcing / override),
                                 or NULL: use the predicted durations                           */
    float *d_log;             /* device [B, Tmax] log-domain predictor output, pads = 0, or NULL */
    int64_t *d_int;           /* device [B, Tmax] clamp(round(exp(y)-1),0), pads = 0, or NULL    */
    int64_t *olens;           /* device [B] frames per utterance = sum of the durations used
                                 (an all-zero row counts as all ones, length_regulator.py:86-88);
                                 -1 for an utterance whose row of xs (all Tmax positions, the padding behind
                                 ilens included) holds a phoneme id outside [0, idim): the
                                 reference's nn.Embedding raises there (fastspeech.py:65-67), a caller
                                 of the host-driven layout must too (fs2_decode refuses the value), the
                                 device-driven layout reports FS2_OVF_BAD_ID                     */
    float *enc_out;           /* device [B, Tmax, adim] encoder output, pads = 0, or NULL        */
    void *workspace;          /* device, fs2_token_workspace_bytes(); must stay alive and
                                 untouched until the matching fs2_decode returns                 */
    size_t workspace_bytes;
    float duration_alpha;     /* length-regulator speed control (length_regulator.py:57-59): the durations
                                 used become round(d * alpha); 0 or 1 = unchanged.  d_int stays unscaled */
} fs2_encode_io;

typedef struct fs2_decode_io {
    uint32_t struct_size;     /* = sizeof(fs2_decode_io); fs2_decode returns FS2_ERR_ARG on mismatch         */
    fs2_batch batch;
    const int64_t *olens;     /* HOST [B]: the values fs2_encode wrote to its device olens       */
    int32_t Lmax;             /* padded frame length of the outputs (>= max olens)               */
    int32_t masked;           /* compat_padded only: 1 = decoder attention / predictor outputs
                                 masked by olens (teacher-forced `_forward`), 0 = no masks
                                 (inference)                                                     */
    const float *es;          /* device [B, es_stride] energies to quantise, or NULL: predict    */
    const float *ps;          /* device [B, ps_stride] pitches to quantise,  or NULL: predict    */
    int32_t es_stride, ps_stride;
    float *before;            /* device [B, Lmax, odim] mel before Postnet (pads = 0 unless compat) */
    float *after;             /* device [B, Lmax, odim] mel after Postnet (may be NULL when after_packed
                                 is given: the sharded path ships only the packed form)             */
    float *e_out, *p_out;     /* device [B, Lmax] predictor outputs (or NULL)                     */
    int32_t *qe, *qp;         /* device [B, Lmax] bucket indices actually embedded (or NULL)      */
    int32_t *lr_index;        /* device [B, Lmax] phoneme index of every frame, -1 at pads (or NULL) */
    float *dec_out;           /* device [B, Lmax, ddim] decoder output (or NULL)                  */
    void *token_workspace;    /* the workspace given to fs2_encode                               */
    void *workspace;          /* device, fs2_frame_workspace_bytes()                              */
    size_t workspace_bytes;
    float *after_packed;      /* device [r * sum(olens), odim] (r = reduction_factor): the valid frames of
                                 `after`, utterances back to back in batch order (what the multi-GPU
                                 all-gather ships), or NULL                                                   */
    /* Device-driven frame layout (no host read-back of the frame counts between fs2_encode and fs2_decode):
     * set olens = NULL and give capacities instead.  The frame counts are taken from the device copy fs2_encode
     * left in the token workspace, the packed-row layout and the attention work list are built by a kernel, grids
     * are sized for the capacities and the surplus tiles exit at once.  Lmax is then the per-utterance capacity of
     * the padded outputs.  status (device int32[8], required in this mode) receives
     * {total rows used, attention work items, overflow flags, longest utterance, valid frames, waves of this call's decoder
     * attention that left attn_w32's fast path (see fs2_get_counter), 0, 0}; overflow
     * flags != 0 (FS2_OVF_*) means a capacity was too small and the outputs are invalid -- before / after /
     * after_packed are then filled with NaN: rerun with larger capacities or with host olens.  after_packed,
     * if given, must hold r * row_capacity rows in this mode. */
    int64_t row_capacity;     /* 0 = host-driven layout (olens required)                                      */
    int32_t *status;
} fs2_decode_io;

#define FS2_OVF_ROWS 1        /* packed rows needed > row_capacity                                           */
#define FS2_OVF_LMAX 2        /* an utterance is longer than Lmax                                            */
#define FS2_OVF_PE 4          /* an utterance is longer than the decoder's positional table                  */
#define FS2_OVF_EMPTY 8       /* an utterance has no frames                                                  */
#define FS2_OVF_BAD_ID 16     /* an utterance holds a phoneme id outside [0, idim): fs2_encode left the frame count -1
                                 for it (the reference's torch.nn.Embedding raises, fastspeech.py:65-67)                */
/* flags of the device-driven vocoder only (fs2_op_griffin_lim_dev, below; it also reports FS2_OVF_ROWS / FS2_OVF_LMAX) */
#define FS2_OVF_UPSTREAM 32   /* the status block of the call that produced the frames carries flags (they are OR-ed in as well) */
#define FS2_OVF_NEG_LEN 64    /* a frame count is negative                                                    */
#define FS2_OVF_WAV 128       /* packed samples needed > wav_capacity                                         */

/* rows to reserve for fs2_decode's device-driven layout given an estimate of the total frame count (alignment
 * and gap rows of the packed layout included) */
int64_t fs2_row_capacity(const fs2_batch *batch, int64_t total_frames_bound);
size_t fs2_frame_workspace_bytes_cap(const fs2_handle *h, const fs2_batch *batch, int64_t row_capacity, int32_t lmax_capacity);

/* lifecycle (replaces FeedForwardTransformer.__init__ / .to(device) / load_state_dict,
 * reference fastspeech.py:37-167, inference.py:156-166).  Every function that takes a handle runs on the
 * handle's device and restores the caller's current HIP device before returning. */
int fs2_create(const fs2_config *cfg, fs2_handle **out);
void fs2_destroy(fs2_handle *h);
const char *fs2_last_error(const fs2_handle *h); /* h may be NULL: last creation error */
int fs2_load_weights(fs2_handle *h, const fs2_tensor_desc *tensors, int32_t n, void *stream);

/* forward pass (replaces FeedForwardTransformer._forward, reference fastspeech.py:169-243) */
size_t fs2_token_workspace_bytes(const fs2_handle *h, const fs2_batch *batch);
int fs2_encode(fs2_handle *h, void *stream, const fs2_encode_io *io);
size_t fs2_frame_workspace_bytes(const fs2_handle *h, const fs2_batch *batch, const int64_t *olens_host);
int fs2_decode(fs2_handle *h, void *stream, const fs2_decode_io *io);

/* Per-launch timing: while profiling is on, every kernel launch is bracketed by hipEvents recorded on
 * the caller's stream; records accumulate until fs2_set_profiling is called again (which clears them).
 * fs2_get_profile waits for the events and fills names/ms/flops/bytes (algorithmic work of each launch)
 * up to `cap`; returns the number of records. */
int fs2_set_profiling(fs2_handle *h, int32_t on);
int fs2_set_profile_filter(fs2_handle *h, const char *name); /* NULL / "": every launch; else only launches of that name */
int fs2_get_profile(fs2_handle *h, const char **names, float *ms, double *flops, double *bytes, int32_t cap);

/* ---- single operators, exported for per-kernel parity tests (all pointers device unless noted) ---- */

/* y = epilogue(conv1d_k(x) or linear(x)); x:[R,C] rows packed with zero gap rows already in place;
 * w: reference layout [N,C,k] (k=1: [N,C]); epilogue order: +bias, +resid, relu_pre, LayerNorm(eps),
 * act_post (0 none,1 relu,2 tanh), dot with dot_w (+dot_b) -> dot_out[R].  row_valid[R] (int32, may be NULL)
 * marks rows to be written as zeros when 0.  (reference modules.py:237-248, encoder.py:60-69) */
typedef struct fs2_op_gemm_args {
    uint32_t struct_size;     /* = sizeof(fs2_op_gemm_args) */
    int32_t R, C, N, ktaps, precision;
    const float *x, *w, *bias, *resid;
    int32_t relu_pre;
    const float *ln_gamma, *ln_beta;
    float ln_eps;
    int32_t act_post;
    const float *dot_w, *dot_b;
    float *dot_out;
    float *y;
    const int32_t *row_valid;
} fs2_op_gemm_args;
int fs2_op_conv_gemm(void *stream, const fs2_op_gemm_args *a);

/* TEST HOOK: plan and run ONE dense-layer launch from the library's own internal argument block (fs2::GemmArgs of
 * csrc/gemm_args.h, copied from `gemm_args`), exactly as the model's launches are planned and run -- the way the kernel-level
 * tests (tests/test_gpu_row_kernels.py) reach the kernels and epilogues the operator above cannot express: planes in and out,
 * the residual as planes, the positional-encoding epilogue, the fused QKV split.  Nothing is allocated, converted or checked on
 * the caller's behalf: the caller owns every buffer the block points to and its size (operand images, outputs, scratch, as the
 * kernel the plan names reads and writes them).  The block is NOT a stable ABI -- it changes with the kernels -- which is why
 * `args_size` must equal this library's sizeof(fs2::GemmArgs): FS2_ERR_ARG otherwise, as for a NULL `gemm_args` / `plan_out`,
 * a `plan_cap` below FS2_GEMM_PLAN_FIELDS or a precision other than FS2_PREC_FP32 / _BF16X3 / _BF16.
 * plan_out[0 .. FS2_GEMM_PLAN_FIELDS) receives the decision (csrc/gemm_plan.h: GemmPlan) before anything is launched: kernel
 * (the GemmKernel enumerator), nsplit, nb, bm, mt, apart, epi, arith, res, ksplit, rows_pass, build_planes.  A launch the plan
 * refuses returns the plan's error code and message and launches nothing. */
#define FS2_GEMM_PLAN_FIELDS 12
int fs2_op_launch_gemm(void *stream, const void *gemm_args, uint32_t args_size, int32_t precision, int32_t *plan_out,
                       int32_t plan_cap);

/* TEST HOOK: the library's own weight repack of the mixed modes, run exactly as fs2_load_weights runs it, so that the
 * kernel-level tests (tests/test_gpu_mx_kernels.py) can hold the images byte for byte against the CPU statement of the
 * formats (tests/gemm_raw.py).  w: device fp32 [N][C][ktaps] (a convolution's weight; N % 128 == 0, C % 128 == 0, ktaps odd).
 * format FS2_REPACK_MX: `image` receives the mx image [N][C / 32 units][tap][128 B] (csrc/gemm_mx.h: repack_weight_mx),
 * `scale_image` is not touched.  FS2_REPACK_MX4: `image` receives the mx4 image [N][C / 64 + C / 128 units][tap][128 B] and
 * `scale_image` its E8M0 scale image [N / 128][C / 128][tap][4][128][2] (repack_weight_mx4), preset to 127 as at load.
 * `image_bytes` / `scale_bytes` must be exactly the images' sizes: FS2_ERR_ARG otherwise, before anything is launched.
 * *kw_out: the exponent of the static weight scale fs2_load_weights derives from max |w| (the mx image is written under it; the
 * mx4 image carries its scales itself).  Device pointers; the stream is drained before the call returns. */
#define FS2_REPACK_MX 1
#define FS2_REPACK_MX4 2
int fs2_op_repack_weight(void *stream, const float *w, int32_t N, int32_t C, int32_t ktaps, int32_t format, void *image,
                         size_t image_bytes, void *scale_image, size_t scale_bytes, int32_t *kw_out);

/* scaled-dot-product self-attention over packed sequences: qkv [R, 3*D] (q | k | v, head-major inside
 * each), ctx [R, D].  seq_start/len/klen: HOST [B]; in the bf16 modes seq_start must be a multiple of 8.  Keys >= klen
 * never reach the output whatever their rows hold (NaN included).  Query rows >= klen produce zeros when mask_q.
 * (reference core/attention.py:47-70) */
int fs2_op_attention(void *stream, const float *qkv, float *ctx, int32_t D, int32_t heads, int32_t B,
                     const int32_t *seq_start, const int32_t *seq_len, const int32_t *seq_klen,
                     int32_t mask_q, int32_t precision);

/* TEST HOOK: plan and run ONE self-attention launch exactly as the model's are planned and run (csrc/attn_plan.h:
 * plan_attention, then the split pass where fp32 QKV rows are given, then the kernel), the sibling of fs2_op_launch_gemm and
 * the way the kernel-level tests (tests/test_gpu_attn_kernels.py) reach what the operator above cannot express: operand planes
 * of known values (or the planes a QKV projection left), the model's dealt, padded and counted work lists, the context as
 * planes, attn_w32's slow-path counter.  Nothing is allocated or converted: every pointer is a DEVICE buffer the caller owns and
 * sizes as the kernels read and write it.
 *   qkv                fp32 rows [R][3 D], or NULL (FS2_PREC_FP32 needs them; the bf16 modes run qkv_split on them first)
 *   qk_hi/lo, vt_hi/lo the bf16 operand planes [Rvt][2 D] and [D][Rvt] (the bf16 modes; Rvt % 32 == 0)
 *   ctx, ctxp          the context as fp32 rows [R][D] and / or (bf16 modes) as split-bf16 planes; at least one
 *   start, len, klen   per utterance; work: (utterance, 128-query block) items, (-1, 0) = padding
 *   dims               NULL: `nitems` items are valid; else the kernels read the valid count from dims[1] and `nitems` is the
 *                      capacity the grid is sized for (the device-driven layout)
 *   slow_count         NULL, or the counter attn_w32 adds one to per wave that leaves its fast path
 * plan_out[0 .. FS2_ATTN_PLAN_FIELDS) receives the decision before anything is launched: kernel (the AttnKernel enumerator),
 * dk, nsplit, grid_x, grid_y, split_pass, the bits of softmax_scale.  A launch the plan refuses returns the plan's error code
 * and message and launches nothing.  FS2_ERR_ARG: a struct_size other than sizeof(fs2_op_attn_args), a NULL argument or a NULL
 * buffer the precision needs, a precision other than FS2_PREC_FP32 / _BF16X3 / _BF16, a `plan_cap` below FS2_ATTN_PLAN_FIELDS. */
typedef struct {
    uint32_t struct_size; /* sizeof(fs2_op_attn_args) */
    int32_t nitems, D, heads, dk_true, R, Rvt, regime_rows, mask_q, precision;
    const float *qkv;
    void *qk_hi, *qk_lo, *vt_hi, *vt_lo;
    float *ctx;
    void *ctxp;
    const int32_t *start, *len, *klen;
    const int32_t *work;
    const int32_t *dims;
    int32_t *slow_count;
} fs2_op_attn_args;
#define FS2_ATTN_PLAN_FIELDS 7
int fs2_op_launch_attention(void *stream, const fs2_op_attn_args *a, int32_t *plan_out, int32_t plan_cap);

/* TEST HOOK: run ONE of the row steps that stand between the dense launches of fs2_encode / fs2_decode -- the sibling of
 * fs2_op_launch_gemm and fs2_op_launch_attention, and the way the kernel-level tests (tests/test_gpu_rowstep_kernels.py) reach
 * them.  The step is launched by the very function the model launches it with (fs2_runtime.hip: *_launch, which owns the grid
 * and block arithmetic), from the library's own internal argument block of that step (csrc/row_step_args.h), copied from `args`:
 *   FS2_ROW_STEP_VAR_GATHER0, _DEC_IN_GATHER   fs2::TokGatherArgs (dec.in.gather runs var_bucket_short first where sqe / sqp are given)
 *   FS2_ROW_STEP_LR_INDEX_SHORT               fs2::ShortLayoutArgs
 *   every other step                          fs2::RowStepArgs
 * The blocks are NOT a stable ABI -- they change with the kernels -- which is why `args_size` must equal this library's sizeof of
 * the step's block.  Nothing is allocated, converted or checked on the caller's behalf: every pointer is a DEVICE buffer the
 * caller owns and sizes as the kernels read and write it.  FS2_ERR_ARG, before anything is launched: a NULL `args`, an unknown
 * `step`, an `args_size` other than the block's. */
#define FS2_ROW_STEP_EMBED 0          /* enc.embed: embed_pe                                        */
#define FS2_ROW_STEP_DUR_POST 1       /* dur.post: dur_finalize, dur_scan                           */
#define FS2_ROW_STEP_LR_INDEX 2       /* lr.index: lr_index_only                                    */
#define FS2_ROW_STEP_LR_INDEX_SHORT 3 /* lr.index under FS2_VARSHORT: lr_index_short                */
#define FS2_ROW_STEP_LR_EXPAND 4      /* lr.expand: lr_expand                                       */
#define FS2_ROW_STEP_VAR_GATHER0 5    /* var.gather0: var_gather0                                   */
#define FS2_ROW_STEP_VAR_EMBED 6      /* var.embed: bucket_embed                                    */
#define FS2_ROW_STEP_DEC_IN_GATHER 7  /* dec.in.gather: var_bucket_short, dec_in_gather             */
#define FS2_ROW_STEP_TO_PLANES 8      /* <tag>.in.planes: to_planes (rows -> planes)                */
#define FS2_ROW_STEP_PLANES_TO_ROWS 9 /* dec.out.rows: planes_to_rows (planes -> rows)              */
#define FS2_ROW_STEP_COUNT 10
int fs2_op_launch_row_step(void *stream, int32_t step, const void *args, uint32_t args_size);

/* length regulator on a padded batch: hs [B,Tmax,D], ds [B,Tmax] (i64), ilens HOST [B] ->
 * out [B,Lmax,D] (pads 0), index [B,Lmax] (-1 pads), olens device [B].  Lmax must be >= max olens.
 * alpha > 0: speed control, durations become round(d * alpha) (1 = unchanged).
 * (reference length_regulator.py:38-95, utils/util.py:91-104) */
int fs2_op_length_regulate(void *stream, const float *hs, const int64_t *ds, const int64_t *ilens_host,
                           int32_t B, int32_t Tmax, int32_t D, int32_t Lmax, float alpha, float *out,
                           int32_t *index, int64_t *olens);

/* dst [B, Lout, W] <- packed rows src [sum(lens), W] (utterance b = rows [starts[b], starts[b]+lens[b])), zero
 * padded; starts/lens: HOST [B].  Inverse of fs2_decode_io.after_packed; replaces utils/util.py:91-104 pad_2d_tensor. */
int fs2_op_unpack_rows(void *stream, const float *src, int32_t W, int32_t B, const int32_t *starts, const int32_t *lens,
                       int32_t Lout, float *dst);

/* same with DEVICE starts / lens (no host copy, no synchronisation): the sync-free multi-GPU gather */
int fs2_op_unpack_rows_dev(void *stream, const float *src, int32_t W, int32_t B, const int32_t *starts_dev, const int32_t *lens_dev,
                           int32_t Lout, float *dst);

/* dst [W, N] <- src [N, W]^T : packed mel frames [sum L, 80] -> vocoder layout [80, sum L] (the reference does
 * mel.transpose + np.concatenate on the host, inference.py:173-178; MelGAN takes [1, 80, L], utils/plot.py:96-105) */
int fs2_op_transpose(void *stream, const float *src, int64_t N, int32_t W, float *dst);

/* idx[i] = bucketize(x[i], bins[nb]) (right=False, NaN -> nb)  (variance_predictor.py:158,231) */
int fs2_op_bucketize(void *stream, const float *x, int64_t n, const float *bins, int32_t nb, int32_t *idx);

/* d[i] = clamp(round_half_even(exp(d_log[i]) - 1), 0) as int64: the duration predictor's inference post-op
 * (duration_predictor.py:77-81) on a flat array.  NaN -> 0; exp overflow saturates to INT64_MAX (torch's
 * .long() of +inf is implementation defined). */
int fs2_op_duration(void *stream, const float *d_log, int64_t n, int64_t *d);

/* ---- Griffin-Lim vocoder and analysis STFT (fastspeech2_amd/csrc/griffin_lim.h; reference utils/stft.py:41-151,
 * dataset/audio_processing.py:224-240).  Fixed transform: n_fft = win_length = 1024, hop 256, 513 bins, periodic Hann window.
 * starts / lens are HOST int32 arrays; every launch goes to `stream`; nothing synchronises with the host.  An utterance of L frames
 * gives 256 * (L - 1) samples (none for L <= 1); utterance b's samples start at 256 * sum_{j<b} max(L_j - 1, 0) of `wav`.  L < 4 is
 * too short for the reflect padding of the reference's STFT: those utterances give zeros.  Every utterance's waveform is
 * bit-identical whether it is vocoded alone or inside any batch (the seeded phase is keyed by utterance-local frame indices). ---- */

/* workspace bytes of fs2_op_griffin_lim for B utterances of lens[b] frames (0 on a bad argument) */
size_t fs2_op_vocode_workspace_bytes(int32_t B, const int32_t *lens);

/* src [rows, src_width]: utterance b = rows [starts[b], starts[b] + lens[b]).  src_width 80: log-mel frames (log(clamp(mel_basis .
 * |S|, 1e-5)), the model's output), magnitudes M = max(mel_pinv . exp(mel), 0) with mel_pinv = pinv(mel basis) [513, 80];
 * src_width 513: linear magnitudes M (mel_pinv ignored); any other width FS2_ERR_UNSUPPORTED.  Initial phase: init_phase [rows, 513]
 * angles in src's row layout, or (NULL) uniform on [-pi, pi) from a counter-based hash of (seed, utterance-local frame, bin).
 * n_iter >= 0 iterations of C = M . A / |A|, A = X - momentum / (1 + momentum) . X_prev (momentum 0: the reference's griffin_lim;
 * > 0: fast Griffin-Lim).  wav: float32 [256 * sum max(L_b - 1, 0)]. */
int fs2_op_griffin_lim(void *stream, const float *src, int32_t src_width, const float *mel_pinv, int32_t B, const int32_t *starts,
                       const int32_t *lens, int32_t n_iter, float momentum, uint32_t seed, const float *init_phase, void *workspace,
                       size_t workspace_bytes, float *wav);

/* workspace bytes of fs2_op_stft for B waveforms of wav_lens[b] samples */
size_t fs2_op_stft_workspace_bytes(int32_t B, const int32_t *wav_lens);

/* Analysis STFT (STFT.transform / TacotronSTFT.mel_spectrogram, stft.py:80-110,188-204): waveform b = wav[wav_starts[b] ..
 * + wav_lens[b]) gives wav_lens[b] / 256 + 1 frames, packed back to back in batch order: mag [frames, 513] = |X| (or NULL),
 * logmel [frames, 80] = log(clamp(mel_basis . |X|, 1e-5)) with mel_basis [80, 513] (or NULL).  A waveform of <= 512 samples
 * cannot be reflect-padded: its frames give |X| = 0, log-mel log(1e-5). */
int fs2_op_stft(void *stream, const float *wav, int32_t B, const int32_t *wav_starts, const int32_t *wav_lens, void *workspace,
                size_t workspace_bytes, float *mag, const float *mel_basis, float *logmel);

/* ---- The same four operations for another transform geometry (the reference's STFT(filter_length, hop_length, win_length) and
 * TacotronSTFT's n_mel_channels), named by the four int32 arguments n_fft, hop, win, n_mels.  Supported: n_fft 512, 1024 or 2048;
 * hop <= win <= n_fft; ceil(n_fft / hop) <= 8; n_mels 1 .. 128.  The window is a periodic Hann of `win` samples zero-padded to n_fft
 * at the centre; bins = n_fft / 2 + 1.  Anything else: FS2_ERR_UNSUPPORTED (workspace queries: 0).  Everything said above holds with
 * 256 -> hop, 513 -> bins, 80 -> n_mels, L < 4 -> L < L_min = n_fft / (2 hop) + 2 (integer division) and 512 samples -> n_fft / 2.
 * At (1024, 256, 1024, 80) the results equal those of the entry points above bit for bit. ---- */

size_t fs2_op_vocode_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *lens);

/* src_width n_mels (with mel_pinv [bins, n_mels]) or bins; init_phase [rows, bins]; wav: float32 [hop * sum max(L_b - 1, 0)]. */
int fs2_op_griffin_lim_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *src, int32_t src_width,
                            const float *mel_pinv, int32_t B, const int32_t *starts, const int32_t *lens, int32_t n_iter, float momentum,
                            uint32_t seed, const float *init_phase, void *workspace, size_t workspace_bytes, float *wav);

size_t fs2_op_stft_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *wav_lens);

/* wav_lens[b] / hop + 1 frames per waveform: mag [frames, bins], logmel [frames, n_mels] with mel_basis [n_mels, bins], and
 * energy [frames] = the L2 norm of each frame's |X| over its bins (the reference preprocessing's energy target), each optional (NULL),
 * all from one launch. */
int fs2_op_stft_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *wav, int32_t B,
                     const int32_t *wav_starts, const int32_t *wav_lens, void *workspace, size_t workspace_bytes, float *mag,
                     const float *mel_basis, float *logmel, float *energy);

/* ---- Pitch (F0) beside the analysis STFT (fastspeech2_amd/csrc/gl_pitch.h): fs2_op_stft_geom plus, from
 * the same launch, f0 [frames] in Hz (0 = unvoiced) and strength [frames], each optional (NULL); mag, logmel and energy are those of
 * fs2_op_stft_geom bit for bit.  The estimator is an autocorrelation one (Boersma 1993 without the path search) and NOT the
 * reference's pitch, which is pyworld's DIO (dataset/audio_processing.py:54-70).  Per frame, y the windowed frame:
 *   r = irfft(|rfft(y)|^2), rw the same of the window; rho[t] = (r[t] / r[0]) / (rw[t] / rw[0]); r[0] <= 1e-12: unvoiced
 *   candidates: lags t in [tmin, tmax] = [floor(sample_rate / f0_ceil), ceil(sample_rate / f0_floor)] with rho[t] > rho[t-1],
 *   rho[t] >= rho[t+1] and rho[t] > 0, refined by a parabola through a = rho[t-1], c = rho[t], b = rho[t+1]:
 *   d = 0.5 (a - b) / (a - 2c + b), t* = t + d, p = c - 0.25 (a - b) d, S = p - octave_cost log2(f0_floor t* / sample_rate)
 *   the winner has the largest S (ties: the smaller t); voiced iff p >= voicing_threshold; f0 = sample_rate / t* where voiced,
 *   strength = the winner's p, 0 without a candidate.
 * A waveform of <= n_fft / 2 samples gives f0 = strength = 0.  The lags must satisfy 2 <= tmin and tmax <= win / 2 (the lowest usable
 * f0_floor is 2 sample_rate / win): otherwise FS2_ERR_UNSUPPORTED.  The workspace holds one table more than fs2_op_stft_geom's. ---- */

size_t fs2_op_stft_pitch_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *wav_lens);

int fs2_op_stft_pitch_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *wav, int32_t B,
                           const int32_t *wav_starts, const int32_t *wav_lens, void *workspace, size_t workspace_bytes, float *mag,
                           const float *mel_basis, float *logmel, float *energy, int32_t sample_rate, double f0_floor, double f0_ceil,
                           double voicing_threshold, double octave_cost, float *f0, float *strength);

/* ---- The first n_candidates candidates per frame instead of the winner alone (gl_pitch.h: gl_candidates):
 * the arguments of fs2_op_stft_pitch_geom with n_candidates, cand_f0 and cand_strength in place of f0 and strength.  The frames, rho,
 * the candidate rule, t*, p and S are those above; the candidates of a frame are put in the order "larger S, then smaller t" and the
 * first n_candidates are written: cand_f0 [frames, n_candidates] = sample_rate / t*, cand_strength [frames, n_candidates] = p, both
 * float32, empty slots 0 / 0, each optional (NULL).  Slot 0 is the winner of fs2_op_stft_pitch_geom bit for bit (its f0 whatever the
 * voicing threshold, which this entry point checks and does not use); mag, logmel and energy are those of fs2_op_stft_geom bit for
 * bit.  FS2_ERR_ARG: n_candidates outside [1, FS2_PITCH_MAX_CANDS]; otherwise as fs2_op_stft_pitch_geom, whose workspace it
 * uses. ---- */
#define FS2_PITCH_MAX_CANDS 8

size_t fs2_op_stft_pitch_cands_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *wav_lens);

int fs2_op_stft_pitch_cands_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *wav, int32_t B,
                                 const int32_t *wav_starts, const int32_t *wav_lens, void *workspace, size_t workspace_bytes, float *mag,
                                 const float *mel_basis, float *logmel, float *energy, int32_t sample_rate, double f0_floor, double f0_ceil,
                                 double voicing_threshold, double octave_cost, int32_t n_candidates, float *cand_f0, float *cand_strength);

/* ---- Device-driven Griffin-Lim: the frame counts stay on the device (what fs2_decode's device-driven layout leaves there), so mel
 * frames become waveforms without a host read-back in between.  The tiles are planned by kernels inside capacities the host knows;
 * grids are sized for the capacities and surplus workgroups exit at once.  Results equal those of fs2_op_griffin_lim_geom for the same
 * frame counts bit for bit. ---- */

/* workspace bytes for B utterances whose frame counts sum to at most frame_capacity (host only; 0 on a bad argument); never less
 * than fs2_op_vocode_workspace_bytes_geom gives for any such batch */
size_t fs2_op_vocode_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity);

/* lens_dev: DEVICE int64 [B] frames per utterance.  src_stride 0: packed source, utterance b starts at row sum_{j<b} L_j and src
 * (and init_phase) hold frame_capacity rows; src_stride > 0: padded source, utterance b starts at row b * src_stride and src holds
 * B * src_stride rows.  wav_stride 0: packed waveform as fs2_op_griffin_lim_geom writes it, the samples of wav [wav_capacity] beyond
 * the valid ones zero; wav_stride > 0: utterance b at wav + b * wav_stride (B * wav_stride <= wav_capacity), zero beyond its own
 * samples.  sample_lens_dev: device int64 [B] = hop * max(L_b - 1, 0).  upstream_status: the device int32[8] status of the
 * fs2_decode that produced src, or NULL.  status: device int32[8] = {frames used, tiles used, flags, longest utterance, valid
 * samples, 0, 0, 0}.  flags != 0 (FS2_OVF_NEG_LEN: an L_b < 0; FS2_OVF_ROWS: sum L_b > frame_capacity; FS2_OVF_LMAX: an L_b >
 * src_stride or hop * (L_b - 1) > wav_stride; FS2_OVF_WAV: packed samples > wav_capacity; FS2_OVF_UPSTREAM | the upstream flags)
 * means nothing was vocoded: all wav_capacity samples are NaN and sample_lens_dev is zero.  The lengths are validated on the device
 * before any tile is planned: whatever lens_dev holds, nothing outside src, the workspace and wav as sized above is touched.
 * Asynchronous on `stream`: no allocation, no host read of device memory, no synchronisation; may be called while the stream is
 * being captured into a graph (after one call outside a capture for a geometry other than the default one).  Host-checked limits:
 * B >= 1, 1 <= frame_capacity, frame_capacity * bins < 2^31, wav_capacity < 2^31. */
int fs2_op_griffin_lim_dev(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *src, int32_t src_width,
                           const float *mel_pinv, int32_t B, const int64_t *lens_dev, int32_t src_stride, int64_t frame_capacity,
                           const int32_t *upstream_status, int32_t n_iter, float momentum, uint32_t seed, const float *init_phase,
                           void *workspace, size_t workspace_bytes, float *wav, int32_t wav_stride, int64_t wav_capacity,
                           int64_t *sample_lens_dev, int32_t *status);

/* ---- Mel-constrained Griffin-Lim: fs2_op_griffin_lim_geom / fs2_op_griffin_lim_dev with another
 * projection inside an iteration.  The prologue (M = max(mel_pinv . exp(mel), 0), C0 = M . exp(i theta0)), the transforms, the
 * momentum form A = X - momentum / (1 + momentum) . T, T <- X and the final ISTFT are unchanged; where the plain call sets
 * C = M . A / |A|, these set, per frame with B = mel_basis [n_mels, bins] (non-negative) and mel the frame's log-mel row of src:
 *   a[k] = |A[k]|;  y[c] = sum_k B[c,k] a[k];  r[c] = min(exp(mel[c]) / max(y[c], 1e-12), 1e4);
 *   g[k] = (sum_c B[c,k] r[c]) / (sum_c B[c,k]), 0 where no filter covers bin k;  C[k] = g[k] A[k]
 * so the mel of the magnitudes the next ISTFT starts from is the caller's.  n_iter = 0 gives the plain call's result bit for bit.
 * Arguments are the plain siblings' plus mel_basis (device).  src_width must be n_mels: a magnitude source (src_width = bins) is
 * FS2_ERR_ARG, as is a NULL mel_basis.  The workspace holds three band tables more than the plain call's (the queries below); an
 * utterance's waveform is bit-identical alone or inside any batch, and in the host-planned and the device-driven form. ---- */

size_t fs2_op_vocode_mel_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *lens);

int fs2_op_griffin_lim_mel_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *src, int32_t src_width,
                                const float *mel_pinv, const float *mel_basis, int32_t B, const int32_t *starts, const int32_t *lens,
                                int32_t n_iter, float momentum, uint32_t seed, const float *init_phase, void *workspace,
                                size_t workspace_bytes, float *wav);

size_t fs2_op_vocode_mel_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity);

int fs2_op_griffin_lim_mel_dev(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *src, int32_t src_width,
                               const float *mel_pinv, const float *mel_basis, int32_t B, const int64_t *lens_dev, int32_t src_stride,
                               int64_t frame_capacity, const int32_t *upstream_status, int32_t n_iter, float momentum, uint32_t seed,
                               const float *init_phase, void *workspace, size_t workspace_bytes, float *wav, int32_t wav_stride,
                               int64_t wav_capacity, int64_t *sample_lens_dev, int32_t *status);

/* ---- Phase-continuity initial phase for Griffin-Lim (fastspeech2_amd/csrc/gl_spsi.h): Single Pass
 * Spectrogram Inversion (Beauregard, Harish and Wyse 2015) builds, from the magnitudes alone, angles to pass as `init_phase` to the
 * entry points above; from them Griffin-Lim needs fewer iterations than from the seeded random phase.  Geometries, src / src_width /
 * mel_pinv, starts / lens and the FS2_ERR_UNSUPPORTED / FS2_ERR_ARG rules are those of fs2_op_griffin_lim_geom; every utterance with
 * L >= 1 is computed (there is no L_min).  Per utterance, M [L, bins] = max(mel_pinv . exp(mel), 0) or the magnitudes given; float32,
 * every operation rounded on its own, no fused multiply-add; phases in turns, acc[bins] = 0 before frame 0.  For the row m of frame t:
 *   peak j (1 <= j <= bins - 2): m[j] > m[j-1] and m[j] > m[j+1].  A non-peak bin b is rising iff m[b] < m[b+1], falling iff
 *   m[b] < m[b-1] (IEEE comparisons: a NaN is neither).  The owner of a non-peak bin is the nearest peak to its right if every bin
 *   from it up to that peak is rising, else the nearest peak to its left if every bin from it down to that peak is falling, else
 *   none; bins 0 and bins - 1 have none; a peak owns itself.
 *   peak j, a, b, c = m[j-1], m[j], m[j+1]: den = (a - 2 b) + c; p = den != 0 ? (0.5 (a - c)) / den : 0;
 *     w = float((hop j) mod n_fft) / n_fft + p float(hop / n_fft); pk = acc[j] + w; pk -= floorf(pk); right = c > a
 *   bin k owned by j, d = k - j: new[k] = pk + h, - 1 if >= 1, with h = 0.5 if right and (d == 1 or d < 0), or if not right and
 *     (d == -1 or d > 0), else 0.  An unowned bin keeps acc[k].  Then acc <- new and phase[t][k] = acc[k] * 6.28318548f.
 * phase [rows, bins] is written in src's row layout, radians in [0, 2 pi); rows no utterance covers are not written.  mag_out
 * [rows, bins] (or NULL) receives the M the phase was computed from, in the same layout.  An utterance's phase is bit-identical
 * alone or inside any batch, packed or padded, and in the host-planned and the device-driven form.  No atomics. ---- */

/* workspace bytes for B utterances of lens[b] frames (HOST array; 0 on a bad argument) */
size_t fs2_op_spsi_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *lens);

/* workspace bytes of the device-driven form for B utterances whose frame counts sum to at most frame_capacity (0 on a bad argument) */
size_t fs2_op_spsi_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity);

/* starts / lens: HOST int32 arrays as in fs2_op_griffin_lim_geom.  Every launch goes to `stream`; nothing synchronises. */
int fs2_op_spsi_phase_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *src, int32_t src_width,
                           const float *mel_pinv, int32_t B, const int32_t *starts, const int32_t *lens, void *workspace,
                           size_t workspace_bytes, float *phase, float *mag_out);

/* lens_dev (DEVICE int64 [B]), src_stride, frame_capacity and upstream_status as in fs2_op_griffin_lim_dev; phase and mag_out hold
 * frame_capacity rows (packed) or B * src_stride rows (padded).  The lengths are validated on the device before anything is indexed
 * with them: on a negative length, a sum beyond frame_capacity, a length above src_stride or upstream flags the call writes nothing
 * to phase or mag_out and touches nothing outside src, the workspace and phase (the fs2_op_griffin_lim_dev that follows reports the
 * flags and fills its waveform with NaN).  No allocation, no host read of device memory, no synchronisation; may be captured into a
 * graph.  Host-checked limits: B >= 1, 1 <= frame_capacity, frame_capacity * bins < 2^31, B * src_stride * bins < 2^31. */
int fs2_op_spsi_phase_dev(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *src, int32_t src_width,
                          const float *mel_pinv, int32_t B, const int64_t *lens_dev, int32_t src_stride, int64_t frame_capacity,
                          const int32_t *upstream_status, void *workspace, size_t workspace_bytes, float *phase, float *mag_out);

/* ---- Excitation from F0 and its STFT phase as the initial phase of Griffin-Lim (fastspeech2_amd/csrc/gl_excite.h; DESIGN.md section
 * 14.12).  f0 holds one float32 value in Hz per source row (the rows that starts / lens, or lens_dev / src_stride, name exactly as for
 * fs2_op_spsi_phase_*).  Per utterance of L frames at hop H: N = H (L - 1) samples, frame t centred on sample t H.  Frame t is voiced
 * iff f0[t] is finite and f0_floor <= f0[t] <= f0_ceil; segment t (samples t H .. t H + H - 1, t <= L - 2) is voiced iff frames t and
 * t + 1 are: a = f0[t], d = f0[t+1] - f0[t], else a = d = 0.  In double, every operation rounded on its own, sr = sample_rate:
 *   S_t = (H a + d (H - 1) 0.5) / sr;  Theta_0 = 0, Theta_{t+1} = frac(Theta_t + S_t) in frame order (turns; frac(x) = x - floor(x))
 *   sample n = t H + i: theta = frac(Theta_t + ((i + 1) a + (d (i (i + 1))) / (2 H)) / sr), f = a + (d i) / H,
 *   Hn = the largest integer with Hn f < sr / 2 (at least 1)
 *   voiced:   e[n] = sqrt(2 / Hn) sum_{h = 1..Hn} cos(2 pi h theta): a band-limited pulse train of unit power (the kernel evaluates
 *             the sum's closed form in float32; tests/excitation_oracle.py states the sum and the tolerance)
 *   unvoiced: e[n] = (u - 0.5) sqrt(12), u = (mix32(n ^ mix32(seed + 0x9E3779B9)) >> 8) / 2^24 with the hash of the seeded initial
 *             phase and n the utterance-local sample: uniform noise of unit power.  The seed changes unvoiced samples only.
 * fs2_op_excitation_* write e; fs2_op_f0_phase_* write phase[row][k] = atan2f(Im, Re) of the STFT of e as fs2_op_stft_geom transforms
 * a waveform (reflect padding, periodic Hann of win in n_fft), 0 where both parts are 0, every row of an utterance 0 where
 * N <= n_fft / 2: float32 radians [rows, bins] in the row layout of f0, what `init_phase` of the synthesis takes.  Rows no utterance
 * covers are not written.  With n_iter = 0 the synthesis from this phase is a one-pass source-filter vocoder whose pitch is the f0
 * given.  An utterance's samples and phase are bit-identical alone or inside any batch, packed or padded, host-planned or
 * device-driven.  No atomics.  FS2_ERR_ARG: sample_rate < 1, f0_floor <= 0, f0_ceil < f0_floor or not finite. ---- */

/* workspace bytes of all four calls below for B utterances of lens[b] frames (HOST array; 0 on a bad argument) */
size_t fs2_op_f0_phase_workspace_bytes_geom(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, const int32_t *lens);

/* workspace bytes of the device-driven forms for B utterances whose frame counts sum to at most frame_capacity (0 on a bad argument) */
size_t fs2_op_f0_phase_workspace_bytes_cap(int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, int32_t B, int64_t frame_capacity);

/* starts / lens: HOST int32 arrays as in fs2_op_griffin_lim_geom.  Every launch goes to `stream`; nothing synchronises. */
int fs2_op_f0_phase_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *f0, int32_t B,
                         const int32_t *starts, const int32_t *lens, double f0_floor, double f0_ceil, int32_t sample_rate, uint32_t seed,
                         void *workspace, size_t workspace_bytes, float *phase);

/* wav: the waveforms packed back to back, sum_b hop max(lens[b] - 1, 0) samples */
int fs2_op_excitation_geom(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *f0, int32_t B,
                           const int32_t *starts, const int32_t *lens, double f0_floor, double f0_ceil, int32_t sample_rate, uint32_t seed,
                           void *workspace, size_t workspace_bytes, float *wav);

/* lens_dev (DEVICE int64 [B]), src_stride, frame_capacity and upstream_status as in fs2_op_spsi_phase_dev; f0 and phase hold
 * frame_capacity rows (packed) or B * src_stride rows (padded).  The lengths are validated on the device before anything is indexed
 * with them: on a negative length, a sum beyond frame_capacity, a length above src_stride or upstream flags the call writes nothing
 * outside the workspace, whose first four ints are then {0, flags (FS2_OVF_*), 0, 0} (without a flag: {frames, 0, samples, 0}).  No
 * allocation, no host read of device memory, no synchronisation; may be captured into a graph.  Host-checked limits: B >= 1,
 * 1 <= frame_capacity, rows * bins < 2^31, hop * frame_capacity < 2^31. */
int fs2_op_f0_phase_dev(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *f0, int32_t B,
                        const int64_t *lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t *upstream_status,
                        double f0_floor, double f0_ceil, int32_t sample_rate, uint32_t seed, void *workspace, size_t workspace_bytes,
                        float *phase);

/* wav [wav_capacity]: wav_stride 0: the waveforms packed back to back; else utterance b at b * wav_stride (B * wav_stride <=
 * wav_capacity < 2^31).  Samples that do not fit (their sum beyond wav_capacity, hop (L - 1) > wav_stride) are FS2_OVF_WAV: nothing
 * is written.  Samples no utterance owns are not written. */
int fs2_op_excitation_dev(void *stream, int32_t n_fft, int32_t hop, int32_t win, int32_t n_mels, const float *f0, int32_t B,
                          const int64_t *lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t *upstream_status,
                          double f0_floor, double f0_ceil, int32_t sample_rate, uint32_t seed, void *workspace, size_t workspace_bytes,
                          float *wav, int32_t wav_stride, int64_t wav_capacity);

/* ---- Training targets from the per-frame energy and F0 arrays (fastspeech2_amd/csrc/targets.h): the
 * reference's remove_outlier (utils/util.py:26-49, applied to every energy and pitch array its data loader returns) and the corpus
 * statistics of its compute_statistics.py, for B utterances packed in x: utterance b = x[starts[b] .. + lens[b]).  Per utterance
 * (float32, n >= 1 values), every operation rounded to float32 on its own, no fused multiply-add:
 *   s = sort(x); for q in {1, 3}: h = q (n - 1), j = h / 4, g = (h % 4) / 4, a = s[j], b = s[min(j + 1, n - 1)], d = b - a,
 *   p = g < 0.5 ? a + d g : b - d (1 - g)        (numpy.percentile(x, 25 / 75) of float32 data, bit for bit: p25, p75)
 *   w = 1.5 (p75 - p25); x[i] is an outlier iff x[i] <= p25 - w or x[i] >= p75 + w  (p25 == p75: every value is one)
 *   M = max_i (outlier_i ? 0 : x[i]);  y[i] = x[i] == 0 ? 0 : outlier_i ? M : x[i]
 * An utterance with a NaN or an infinity is copied unchanged: its quartiles are NaN, its outlier count 0, and the statistics leave
 * it out.  An utterance of 0 values produces nothing (quartiles NaN, count 0).  There is no limit on an utterance's length.
 * stats: device double[12] over the cleaned values y of the finite utterances --
 *   [0] n_total        values          [1] n_outliers   flagged values      [2] n_nonfinite  utterances with a NaN / infinity
 *   [3] n_no_positive  utterances (n >= 1, finite) without any y > 0        [4] n            values y != 0
 *   [5] min  [6] nonzero_min = min over y > 0 (+inf: none)  [7] max         (min +inf and max -inf without a value)
 *   [8] mean  [9] std = sqrt(M2 / n)  [10] M2 = sum (y - mean)^2, all three over y != 0, in double (0 when n = 0)   [11] 0
 * The sums are reduced in a fixed order without floating-point atomics: the same batch gives the same bits on every call, and an
 * utterance's y, quartiles and count do not depend on the batch it is in. ---- */

/* workspace bytes of fs2_op_clean_targets for B utterances (host only; 0 on a bad argument, B < 0) */
size_t fs2_op_targets_workspace_bytes(int32_t B);

/* starts, lens: HOST int32 [B] (read before the call returns).  y: device float32, indexed as x, may equal x (in place).
 * quartiles [B, 2] = p25, p75; n_outliers [B] int32; stats double[12] as above: device, each optional (NULL).  Asynchronous on
 * `stream`: no allocation, no host read of device memory, no synchronisation. */
int fs2_op_clean_targets(void *stream, const float *x, int32_t B, const int32_t *starts, const int32_t *lens, void *workspace,
                         size_t workspace_bytes, float *y, float *quartiles, int32_t *n_outliers, double *stats);

/* ---- Loss terms of the teacher-forced forward, per utterance (fastspeech2_amd/csrc/losses.h): what the
 * reference's FeedForwardTransformer.forward() (fastspeech.py:280-333, the seven report values) and its evaluation.py (12-41, the mean
 * L1 of duration, energy and pitch per utterance) reduce the model's outputs and the targets to.  Every difference is formed in double
 * from the float32 / int64 inputs (exact); |.|, the square and log((double)ds + 1.0) are taken in double; sums are carried in double
 * and reduced in a fixed order without floating-point atomics.  A record is FS2_LOSS_TERMS doubles:
 *   [0] ilen   [1] olen   [2] Tmax - ilen   [3] Lmax - olen
 *   [4] sum |before - ys|   [5] sum |after - ys|                        frames [0, olen), all odim bins
 *   [6] sum (d_outs - log(ds + 1))^2                                    tokens [0, ilen)
 *   [7] sum (e_outs - es)^2   [8] sum (p_outs - ps)^2                   frames [0, olen)
 *   [9] sum |d_outs - ds|     tokens [0, ilen): evaluation.py:31 as written, the log-domain output against the linear durations
 *   [10] sum |e_outs - es|    [11] sum |p_outs - ps|                    frames [0, olen)
 *   [12] .. [16]  the sums of [4] .. [8] over the pad frames [olen, Lmax) / pad tokens [ilen, Tmax): what the reference's means
 *                 include under use_masking = False.  0 with pads = 0, and nothing outside [0, len) of any utterance is then read
 *   [17] .. [19]  0
 * An utterance's [4] .. [11] depend on its own values only: not on B, on its place in the batch, on a stride, on Lmax or on the
 * alignment of a pointer.  The batch record has the same layout: [0] .. [3] and every sum added up over the B utterances in a fixed
 * order (the same batch gives the same bits on every call). ---- */
#define FS2_LOSS_TERMS 20

/* before, after: [B, pred_stride_f, odim]; ys: [B, y_stride_f, odim]; d_outs: [B, pred_stride_t]; ds: int64 [B, ds_stride_t];
 * e_outs, p_outs: [B, pred_stride_f]; es, ps: [B, tgt_stride_f] -- device, float32 unless noted, strides in elements of the second
 * dimension.  A prediction and its target may be NULL together (before and after share ys): its sums are 0.  Tmax >= max ilens and
 * Lmax >= max olens are the padded extents the pad sums run to; neither may exceed a stride of a tensor that is given.
 * ilens, olens: HOST int32 [B] (read before the call returns).  terms: device double [B, FS2_LOSS_TERMS]; batch: device
 * double [FS2_LOSS_TERMS]; each optional (NULL).  B = 0 writes a zero batch record.  (The struct is declared in two statements so
 * that tools/gen_binding_doc.py, whose list of mirrored structs is fixed, leaves it alone; fastspeech2_amd/_lib.py: OpLossArgs.) */
struct fs2_op_loss_args {
    uint32_t struct_size;     /* = sizeof(fs2_op_loss_args) */
    int32_t B, odim, Tmax, Lmax, pads;
    int32_t pred_stride_f, y_stride_f, pred_stride_t, ds_stride_t, tgt_stride_f;
    const float *before, *after, *ys, *d_outs;
    const int64_t *ds;
    const float *e_outs, *es, *p_outs, *ps;
    const int32_t *ilens, *olens;
    void *workspace;
    size_t workspace_bytes;
    double *terms, *batch;
};
typedef struct fs2_op_loss_args fs2_op_loss_args;

/* workspace bytes of fs2_op_loss_terms for utterances of olens frames (HOST int32 [B]); host only; 0 on a bad argument (B < 0, a
 * negative length, null olens with B > 0) */
size_t fs2_op_loss_workspace_bytes(int32_t B, const int32_t *olens);

/* Asynchronous on `stream`: no allocation, no host read of device memory, no synchronisation; legal during stream capture.  Two
 * launches plus the upload of the length records (kernel arguments).  FS2_ERR_ARG: wrong struct_size, a negative length,
 * ilen > Tmax, olen > Lmax, an extent beyond a stride, a prediction without its target, a null workspace with B > 0;
 * FS2_ERR_WORKSPACE: workspace_bytes below fs2_op_loss_workspace_bytes(B, olens). */
int fs2_op_loss_terms(void *stream, const fs2_op_loss_args *a);

/* ---- Dynamic time warping between B pairs of feature sequences a [N, D] (synthesized) and b [M, D] (reference) of different
 * lengths, with the energy and F0 errors over the aligned frame pairs (fastspeech2_amd/csrc/dtw.h): the
 * numbers of the free-running validation.  d(i, j) = sqrt(sum_k (a[i, k] - b[j, k])^2) in double, k in increasing order, nothing
 * contracted; C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)), the predecessor chosen in that order with a strict "<"
 * (outside the matrix: +inf).  Each cell carries the record of its path, so the record of (N-1, M-1) is the result; the path itself
 * is not returned.  A record is FS2_DTW_TERMS doubles:
 *   [0] N   [1] M   [2] steps = frame pairs on the path   [3] cost C(N-1, M-1)
 *   [4] sum |e_a[i] - e_b[j]|   [5] sum |p_a[i] - p_b[j]|                        over the path, in path order
 *   [6] pairs with both pitches non-zero   [7] sum |p_a[i] - p_b[j]| over those   [8] pairs with exactly one pitch non-zero
 *   [9] .. [11]  0
 * N = 0 or M = 0 gives [0], [1] and zeros.  A pair's record depends on its own values only: not on B, on its place in the batch,
 * on a stride or on the workspace handed in.  The batch record has the same layout: every entry added up over the pairs in index
 * order.  A non-finite value in a valid frame makes that pair's cost non-finite and touches no other pair. ---- */
#define FS2_DTW_TERMS 12

/* a, b: device float32, row r of the a side at a + r * a_stride (strides in floats, >= D); pair i owns the rows
 * [a_starts[i], a_starts[i] + a_lens[i]) of a and [b_starts[i], b_starts[i] + b_lens[i]) of b, so padded and packed layouts are both
 * served.  e_a, p_a / e_b, p_b: device float32 scalar tracks indexed by the same rows (energy; pitch, 0 = unvoiced); each track is
 * given for both sides or for neither (NULL: its sums are 0).  a_starts, a_lens, b_starts, b_lens: HOST int32 [B] (read before the
 * call returns).  1 <= D <= 128.  terms: device double [B, FS2_DTW_TERMS]; batch: device double [FS2_DTW_TERMS]; each optional.
 * B = 0 writes a zero batch record.  (Declared in two statements for the reason given at fs2_op_loss_args; _lib.py: OpDtwArgs.) */
struct fs2_op_dtw_args {
    uint32_t struct_size;     /* = sizeof(fs2_op_dtw_args) */
    int32_t B, D;
    int64_t a_stride, b_stride;
    const float *a, *b, *e_a, *e_b, *p_a, *p_b;
    const int32_t *a_starts, *a_lens, *b_starts, *b_lens;
    void *workspace;
    size_t workspace_bytes;
    double *terms, *batch;
};
typedef struct fs2_op_dtw_args fs2_op_dtw_args;

/* workspace bytes of fs2_op_dtw for pairs of a_lens x b_lens frames (HOST int32 [B]): min(what all pairs need at once,
 * max(cap_bytes, what the largest single pair needs)) -- with less than everything the call works through groups of consecutive
 * pairs, reusing the workspace in stream order.  Host only; 0 on a bad argument (B < 0, a negative length, a null pointer with
 * B > 0, a matrix of more than 2^40 cells). */
size_t fs2_op_dtw_workspace_bytes(int32_t B, const int32_t *a_lens, const int32_t *b_lens, size_t cap_bytes);

/* Asynchronous on `stream`: no allocation, no host read of device memory, no synchronisation; legal during stream capture.  Per
 * group of pairs one launch for the distance matrices and one for the sweep, plus the upload of the pair records (kernel
 * arguments) and one combining launch.  FS2_ERR_ARG: wrong struct_size, D outside [1, 128], a stride below D, a negative start or
 * length, a track given for one side only, a null workspace with B > 0; FS2_ERR_WORKSPACE: workspace_bytes below
 * fs2_op_dtw_workspace_bytes(B, a_lens, b_lens, 0). */
int fs2_op_dtw(void *stream, const fs2_op_dtw_args *a);

/* ---- Forced alignment of B pairs: the frames b [M, D] of a recording are assigned, monotonically, to the states a [N, D] (the
 * frames of the synthesis), each frame to exactly one state, and the frames per label (phoneme) are counted: durations that add up
 * to M (fastspeech2_amd/csrc/align.h).  d(i, j) as above.  Q(0, 0) = d(0, 0); Q(i, 0) = +inf for i > 0;
 * Q(i, j) = d(i, j) + min over k = 0 .. max_step of Q(i - k, j - 1), the predecessor chosen in the order k = 0, 1, 2 with a strict
 * "<" (outside the matrix: +inf).  s(M-1) = N-1, s(j-1) = s(j) - k(s(j), j).  An alignment exists iff N >= 1, M >= 1 and
 * N - 1 <= max_step (M - 1).  Results per pair:
 *   state      s(j) for every frame j: the pair-local index of its state
 *   durations  durations[t] = the frames j with label(s(j)) = t; label(i) = labels[i], or i without labels (n_labels = N then).  The
 *              whole row [0, dur_stride) is written, zeros beyond n_labels
 *   a record of FS2_ALIGN_TERMS doubles:
 *   [0] N   [1] M   [2] flags: 0 fine, 1 no alignment exists, 2 the cost is not finite   [3] cost Q(N-1, M-1)
 *   [4] states that received a frame   [5] the longest run of frames in one state   [6] labels in [0, n_labels) without a frame   [7] 0
 * With flags != 0 the durations row is zeros, state is -1 and [4] .. [6] are 0; [3] is 0 for flag 1 and the computed cost for flag 2.
 * A pair's results depend on its own values only: not on B, on its place in the batch, on a stride or on the workspace handed in; a
 * non-finite value in one pair touches no other pair.  The batch record has the same layout: [2] = the pairs with flags != 0, every
 * other entry added up over the pairs with flags 0 in index order.  The labels of a pair must be non-decreasing and lie in
 * [0, n_labels): a label outside that range is SKIPPED (its frames are counted nowhere), and with a decreasing sequence a label's
 * count is that of one of its runs; neither writes outside the pair's own durations row. ---- */
#define FS2_ALIGN_TERMS 8

/* a, b, their strides, starts and lengths: as fs2_op_dtw_args.  max_step: 1 or 2.  labels: device int32 indexed by the rows of a, or
 * NULL; n_labels: HOST int32 [B], NULL iff labels is NULL, 0 <= n_labels[i] <= dur_stride (without labels: a_lens[i] <= dur_stride).
 * durations: device int64 [B, dur_stride]; state: device int32 indexed by the rows of b; terms: device double [B, FS2_ALIGN_TERMS];
 * batch: device double [FS2_ALIGN_TERMS]; each of the four optional.  B = 0 writes a zero batch record.  (Declared in two
 * statements for the reason given at fs2_op_loss_args; _lib.py: OpAlignArgs.) */
struct fs2_op_align_args {
    uint32_t struct_size;     /* = sizeof(fs2_op_align_args) */
    int32_t B, D, max_step;
    int64_t a_stride, b_stride, dur_stride;
    const float *a, *b;
    const int32_t *labels;
    const int32_t *a_starts, *a_lens, *b_starts, *b_lens, *n_labels;
    void *workspace;
    size_t workspace_bytes;
    int64_t *durations;
    int32_t *state;
    double *terms, *batch;
};
typedef struct fs2_op_align_args fs2_op_align_args;

/* workspace bytes of fs2_op_align: min(what all pairs need at once, max(cap_bytes, what the largest single pair needs)), as
 * fs2_op_dtw_workspace_bytes; host only; 0 on a bad argument. */
size_t fs2_op_align_workspace_bytes(int32_t B, const int32_t *a_lens, const int32_t *b_lens, size_t cap_bytes);

/* Asynchronous on `stream`: no allocation, no host read of device memory, no synchronisation; legal during stream capture.  Per
 * group of pairs one launch for the distance matrices and one for the sweep with its walk back, plus the upload of the pair records
 * (kernel arguments) and one combining launch.  FS2_ERR_ARG: wrong struct_size, D outside [1, 128], max_step outside {1, 2}, a
 * stride below D, a negative start or length, n_labels[i] outside [0, dur_stride], dur_stride below a_lens[i] without labels, labels
 * without n_labels (or the reverse), a null workspace with B > 0; FS2_ERR_WORKSPACE: workspace_bytes below
 * fs2_op_align_workspace_bytes(B, a_lens, b_lens, 0). */
int fs2_op_align(void *stream, const fs2_op_align_args *a);

/* ---- Pitch path search over B utterances (fastspeech2_amd/csrc/pitch_path.h): per utterance of T frames
 * with n_candidates = K candidates each (fs2_op_stft_pitch_cands_geom's, or any other source's), the best sequence of states.  State
 * 0 is "unvoiced", state c = 1 .. K is candidate c - 1, which exists iff cand_f0 > 0.  All in double, from the float32 inputs:
 *   u(t, 0) = voicing_threshold;  u(t, c) = p - octave_cost log2(f0_floor / f)
 *   trans(j -> c) = 0 (both unvoiced), voiced_unvoiced_cost s (exactly one unvoiced), octave_jump_cost s |log2 f_j - log2 f_c| (both
 *   voiced), s = 0.01 / time_step (time_step: seconds per frame)
 *   D(0, c) = u(0, c);  D(t, c) = u(t, c) + max over the existing j, ascending, of [D(t-1, j) - trans(j -> c)] with a strict ">" (a
 *   tie keeps the smaller j); the end state is the largest D(T-1, c), a tie to the smaller c; then the walk back.
 * Results per frame: f0 (the chosen candidate's, 0 = unvoiced), state (c - 1, -1 = unvoiced), strength (the chosen p, 0 = unvoiced);
 * per utterance a record of FS2_PITCH_PATH_TERMS doubles:
 *   [0] T   [1] flags: 0 fine, 2 a candidate value (f0 or strength) is not finite or is negative   [2] D of the path
 *   [3] voiced frames   [4] voiced / unvoiced switches   [5] the largest |log2 f(t-1) - log2 f(t)| over consecutive voiced frames
 *   [6] frames whose state differs from the frame's own argmax of u (ties to the smaller state)   [7] 0
 * With flags 2 the utterance's frames are 0 / -1 / 0 and [2] .. [6] are 0.  T = 0 writes no frame (its record is zeros).  An
 * utterance's results depend on its own values only: not on B, on its place in the batch or on the workspace.  The batch record:
 * [1] = the utterances with flags != 0, [5] the maximum and every other entry the sum over the utterances with flags 0, in index
 * order. ---- */
#define FS2_PITCH_PATH_TERMS 8

/* cand_f0, cand_strength: device float32 [rows, n_candidates]; frame_starts / frame_lens: HOST int32 [B], the first row and the
 * frames of every utterance; f0 / strength: device float32 [rows], state: device int32 [rows], terms: device double
 * [B, FS2_PITCH_PATH_TERMS], batch: device double [FS2_PITCH_PATH_TERMS], each of the five optional.  B = 0 writes a zero batch
 * record.  (Declared in two statements for the reason given at fs2_op_loss_args; _lib.py: OpPitchPathArgs.) */
struct fs2_op_pitch_path_args {
    uint32_t struct_size;     /* = sizeof(fs2_op_pitch_path_args) */
    int32_t B, n_candidates;
    double time_step, f0_floor, voicing_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost;
    const float *cand_f0, *cand_strength;
    const int32_t *frame_starts, *frame_lens;
    void *workspace;
    size_t workspace_bytes;
    float *f0;
    int32_t *state;
    float *strength;
    double *terms, *batch;
};
typedef struct fs2_op_pitch_path_args fs2_op_pitch_path_args;

/* workspace bytes of fs2_op_pitch_path: 8 bytes per frame (a frame's back pointers) plus the records; host only; 0 on a bad
 * argument (negative B or length, null frame_lens with B > 0). */
size_t fs2_op_pitch_path_workspace_bytes(int32_t B, const int32_t *frame_lens);

/* Asynchronous on `stream`: no allocation, no host read of device memory, no synchronisation; legal during stream capture.  One
 * launch per 128 utterances (one wave per utterance; their rows travel as kernel arguments) and one combining launch.  FS2_ERR_ARG:
 * wrong struct_size, n_candidates outside [1, FS2_PITCH_MAX_CANDS], time_step or f0_floor not positive and finite, a non-finite
 * voicing_threshold or octave_cost, an octave_jump_cost or voiced_unvoiced_cost that is negative or not finite, a negative B, start
 * or length, null starts / lens / candidates / workspace with B > 0; FS2_ERR_UNSUPPORTED: more than INT32_MAX candidate slots;
 * FS2_ERR_WORKSPACE: workspace_bytes below fs2_op_pitch_path_workspace_bytes(B, frame_lens). */
int fs2_op_pitch_path(void *stream, const fs2_op_pitch_path_args *a);

/* ---- Pitch and energy control of the free-running synthesis (fastspeech2_amd/csrc/prosody.h).  Between the
 * variance predictors and the quantisation of their outputs, every predicted value v of a frame of utterance b that was expanded from
 * phoneme t becomes
 *   v' = fadd_rn(fmul_rn(v, scale), shift),  scale = scale_ptr ? scale_ptr[b * cols_s + (cols_s == 1 ? 0 : t)] : 1.0f,
 *                                            shift = shift_ptr ? shift_ptr[b * cols_h + (cols_h == 1 ? 0 : t)] : 0.0f
 * in float32, the product and the sum rounded one after the other (no fused multiply-add), for pitch and for energy alike.  cols = 1:
 * one value per utterance; cols = batch.Tmax: one per phoneme.  The bucket rule and everything behind it are unchanged; e_out / p_out
 * return the CONTROLLED values, the ones that were quantised.  The units are the predictors' (the units of the training targets:
 * with F0 in Hz, pitch_scale = 2^(n / 12) raises the voice by n semitones).  (Declared in two statements for the reason given at
 * fs2_op_loss_args; _lib.py: Prosody.) ---- */
struct fs2_prosody {
    uint32_t struct_size;     /* = sizeof(fs2_prosody) */
    const float *pitch_scale, *pitch_shift, *energy_scale, *energy_shift;   /* device [B, cols], or NULL = neutral */
    int32_t pitch_scale_cols, pitch_shift_cols, energy_scale_cols, energy_shift_cols;   /* 1 (per utterance) or Tmax (per phoneme) */
};
typedef struct fs2_prosody fs2_prosody;

/* fs2_decode with control: fs2_decode(h, stream, io) is fs2_decode_ctl(h, stream, io, NULL).  ctl == NULL, or all four pointers NULL:
 * no extra launch, every output is what fs2_decode gives.  Otherwise one launch more (profile name "var.control"), in the host-driven
 * and in the device-driven layout; like fs2_decode it allocates nothing, reads no device memory and does not synchronise, so it is legal
 * during stream capture.  FS2_ERR_ARG: wrong struct_size; a cols of a given pointer that is neither 1 nor batch.Tmax; pitch control
 * together with io->ps, or energy control together with io->es (control acts on predictions); batch.compat_padded != 0 (control has
 * per-utterance semantics only). */
int fs2_decode_ctl(fs2_handle *h, void *stream, const fs2_decode_io *io, const fs2_prosody *ctl);

/* Per-label (per-phoneme) means of a per-frame track: x float32 [B, x_stride], labels int32 [B, x_stride] (fs2_decode_io.lr_index:
 * non-decreasing over the valid frames, anything beyond them), lens_dev DEVICE int64 [B] = the valid frames (clamped to [0, x_stride])
 * -> mean float32 [B, n_labels], count int32 [B, n_labels], both written whole: count[b, t] = the frames j < lens[b] with
 * labels[b, j] == t (positive_only != 0: only those with x[b, j] > 0, the voiced frames of an F0 track), mean[b, t] = (float)(their
 * sum, added in frame order in double, / count), 0 where count is 0.  Labels that are not non-decreasing give unspecified values;
 * nothing outside the utterance's own valid frames is read.  Asynchronous on `stream`: one launch, no allocation, no host read of
 * device memory, no synchronisation; legal during stream capture.  FS2_ERR_ARG: B, x_stride or n_labels negative, B * n_labels beyond
 * 2^31 - 1, a null pointer with a non-empty extent.  B = 0 does nothing. */
int fs2_op_label_means(void *stream, const float *x, const int32_t *labels, const int64_t *lens_dev, int32_t B, int32_t x_stride,
                       int32_t n_labels, int32_t positive_only, float *mean, int32_t *count);

/* Kernel-choice switches for A/B measurements and tests ("FS2_BM", "FS2_ROW8", "FS2_QKV8", "FS2_NOSPLITK",
 * "FS2_F32_ROWS", "FS2_MT8", "FS2_FUSE_VAR", "FS2_BAL", "FS2_ATTN_W32", "FS2_ROW4", "FS2_MT4", "FS2_QKV4", "FS2_FFN2_MX", "FS2_POST_MX", "FS2_TOKPROJ", "FS2_TOKPROJ_F32", "FS2_VARSHORT"; -1 = automatic).
 * "FS2_TOKPROJ": 0 = frame-level launches, 1 = the predictors' first convolution, 2 = the decoder input layer, 3 (default) = both from the token-level products of fs2_encode
 * (takes effect with the next fs2_encode; fp32 never takes it); "FS2_TOKPROJ_F32": those products on the exact fp32 GEMM.
 * "FS2_VARSHORT": 1 (default) = the fused variance predictors, the prosody control and the bucket search of the predictions run on at most K = 5 frames per phoneme (the
 * first two, the last two and one interior frame: every other frame of a phoneme has the interior one's values) wherever FS2_TOKPROJ = 3 holds and the batch has per-utterance
 * semantics; 0 = on every frame.  Selected by configuration and option alone, never by the batch; takes effect with the next fs2_encode.  Their initial values come from the environment variables of the same
 * names, read once when the library is first used; the launch path never reads the environment. */
int fs2_set_option(const char *name, int32_t value);

/* Reads a switch back (the value fs2_set_option / the environment left: -1 = automatic), or one of the read-only facts about
 * THIS binary a benchmark line should carry:
 *   "FS2_AUDIT_CLEAN"   1 if a clean ISA-audit record of exactly this binary (libfs2_hip.audit.json next to it, tied to the
 *                       file's SHA-256) was found when the library was first used, else 0.  The kernels whose accumulators
 *                       are literal registers (attn_w32, gemm_row4_bf16) run only in an audited binary: without the record
 *                       FS2_ATTN_W32 / FS2_ROW4 / FS2_QKV4 start at 0 for EVERY consumer of the library (ctypes, the
 *                       TorchScript op, a C program) and can only be switched on by an explicit fs2_set_option;
 *   "attn_w32_active" / "row4_active" / "qkv4_active"   1 if that kernel is allowed to run (its switch is not 0).
 * Unknown name: FS2_ERR_ARG. */
int fs2_get_option(const char *name, int32_t *value);

/* Cumulative event counters of a handle (device memory, read back with one blocking 8-byte copy behind `stream`):
 *   "attn_slow_path_waves"  waves of attn_w32 that left the fast path because a row's probabilities, relative to its FIRST key
 *                           tile's maximum, summed beyond 2^60 (peaked attention of a trained model: reference
 *                           core/attention.py:55-62 has no such notion, its softmax is one formula) and were recomputed by the
 *                           plain fp32 two-pass loop: correct, but ~30 x slower per wave.  0 on flat (random-init) attention.
 * reset != 0 zeroes the counter after reading it. */
int fs2_get_counter(fs2_handle *h, void *stream, const char *name, int64_t *value, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* FS2_H_ */
