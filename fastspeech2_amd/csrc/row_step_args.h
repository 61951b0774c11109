// The argument blocks of the row steps between the GEMMs (elementwise.h, varshort.h): plain data, no HIP types, so that the CPU test which mirrors them
// (tests/rowstep_raw_probe.cpp, tests/rowstep_raw.py) compiles the same structs as the kernels and the runtime's launch functions (fs2_runtime.hip: *_launch),
// and the test hook fs2_op_launch_row_step (include/fs2.h) can copy them in.  None of them is a stable ABI: they change with the kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fs2 {

// ---- multiply before expanding (fs2_runtime.hip: tok.proj) ----
// The length regulator repeats every encoder row once per frame, and the first layer behind it is linear: the products of the encoder rows with the
// weights of the predictors' first convolution (one k = 1 product per tap) and of the decoder input layer are computed once per TOKEN, as the rows
// P [token rows, ldp] = [tap0: energy | pitch][tap1: energy | pitch][tap2: energy | pitch][dec.in], and var_gather0 / dec_in_gather gather them per frame.
struct TokGatherArgs {
    const float* P; int ldp;            // token-level products (fs2_encode), fp32 rows
    const int* tok_start;               // [B] first token row of every utterance
    const int* lri;                     // [R] token of every frame row (lr_index_only), -1: none
    const int *row_pos, *row_seq;       // frame-row metadata
    int R;
    // var_gather0
    int chans;                          // channels of one predictor's first layer
    const float *bias, *ln_g, *ln_b;    // stacked energy | pitch: [2 chans]
    void* vp;                           // planes of the stacked hidden layer [R][2 chans]
    // dec_in_gather
    int col0, D;                        // first dec.in column of P; decoder width
    const float *es, *ps; int es_stride, ps_stride;      // teacher forcing ([B, stride]) or nullptr
    const float *e_rows, *p_rows;       // the predictions per packed row
    const float *ebins, *pbins; int nb;
    const float *TE, *TP;               // [n_bins, D]: the embedding tables behind the input layer's weights (TP carries its bias)
    int *qe_rows, *qp_rows;
    // FS2_VARSHORT: the predictions exist per SHORT row and their buckets were searched there (varshort.h): a frame reads them through f2s [R]
    // (-1: no short row).  sqe / sqp == nullptr: that index is searched per frame, from es / ps (teacher forcing) or e_rows / p_rows
    const int *f2s, *sqe, *sqp;
    const float *ln_g2, *ln_b2;         // LayerNorm of the input layer
    const float* pe; const float* pe_alpha; float x_scale;
    float* x0; void* x0p;               // fp32 rows (or nullptr: planes only) and split-bf16 planes of the decoder input
    // what var_bucket_short, launched in front of dec_in_gather where sqe / sqp are given, takes beyond the above: the short rows' positions and their count
    const int* srow_pos; int Rs;
};

// ---- FS2_VARSHORT: the short layout (varshort.h: lr_index_short) ----
struct ShortLayoutArgs {
    // in: the duration scan (dur_scan) and the token layout
    const int *cum, *scum; int Tmax;      // running sums of the durations and of the short durations [B, Tmax]
    const int* ilen;                      // [B] phonemes
    const int* so32;                      // [B] short frames
    // in: the frame rows
    const int *row_pos, *row_seq, *vlen; int R;
    const int* ovf;                       // device-driven layout: its overflow flags (set: the frame layout is empty, and so is the short one); nullptr: host-driven
    int B, gap, K;
    int Rs, Rs_pad;                       // rows the short arrays hold (vs_row_bound, never more than the frame rows); srow_* are written up to Rs_pad
    // out: per frame row
    int* lri;                             // [R] token of the frame (lr_index_only's output)
    int* f2s;                             // [R] short row of the frame, -1: none
    // out: the short layout
    int *sstart, *slen;                   // [B]
    int* sdims;                           // [0] = short rows in use (the launches on short rows take it as Rp)
    int *srow_pos, *srow_seq, *slri;      // [Rs_pad] position, utterance and token of a short row (-1: gap row)
};

// ---- every other row step: one flat block; a step reads the fields under its name and those under "rows" ----
struct RowStepArgs {
    // rows: the packed rows the step runs on and their utterances
    const int *row_pos, *row_seq; int R;  // [R] position inside the utterance (-1: gap row) and utterance of every row
    const int *start, *vlen; int B;       // [B] first row and true length of every utterance in that layout
    int Tmax, D;                          // padded token count of the batch; row width
    float* rows; void* planes;            // the step's fp32 rows [R][D] and split-bf16 planes of them (in or out by step; planes may be nullptr where optional)
    // enc.embed (embed_pe): rows = E[xs] x_scale + alpha pe[pos]
    const int64_t* xs; const float* E; int idim;
    const float* pe; const float* pe_alpha; float x_scale;
    // dur.post (dur_finalize, dur_scan); start / vlen are the token layout's
    const float* dlog_rows; float* d_log; int64_t *d_int, *d_int2;
    const int64_t* ds;                    // the durations the scan takes (teacher forcing), nullptr: d_int
    int* cum; int64_t* olens; int* olens32; float alpha;
    int *scum, *so32; int K;              // FS2_VARSHORT: the short sums, or nullptr
    // lr.index (lr_index_only) and lr.expand (lr_expand: rows = src_rows[tok_start + index]); vlen is the frame layout's
    const float* src_rows; const int *tok_start, *ilen; const int* cum_in; int* index_rows;
    // var.embed (bucket_embed): rows += Tp[qp] + Te[qe] in place
    const float *es, *ps; int es_stride, ps_stride;
    const float *e_rows, *p_rows;
    const float *ebins, *pbins; int nb;
    const float *Te, *Tp;
    int *qe_rows, *qp_rows;
};

}  // namespace fs2
