// The call plan: what fs2_encode and fs2_decode refuse, and which launches a call consists of, decided once per call.
// gemm_plan.h / attn_plan.h decide HOW a launch runs, model_launches.h forms its arguments; this header decides WHETHER it runs.  fs2_runtime.hip checks,
// lays out and carves, plans, then launches in straight-line code that branches on plan fields only; tests/gemm_plan_probe.cpp branches on the same fields on
// the CPU (names, decisions, call_refusals).  HIP-free like gemm_plan.h: plain structs, host arrays and pointers nobody follows here.
// The one rule: a new option or output that changes which launches a call makes is decided in plan_encode / plan_decode and nowhere else.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/fs2.h"
#include "layout_rule.h"
#include "model_launches.h"

namespace fs2 {

// ------------------------------------------------------------------ what a call inherits
// The split-K scratch of a call (4 slabs of kSplitRows x 1024 floats at most; gemm_plan.h: enough for every launch with R <= kSplitRows).
inline size_t kpart_floats(size_t Rpad) { return (size_t)4 * std::min<size_t>(Rpad, kSplitRows) * 1024; }

// The row counts the kernel-variant choices are functions of (fs2.h: fs2_batch.regime_*): ESTIMATES of the packed rows of the batch the variants
// are chosen for -- this call's own, or the larger one the caller names -- at token level (one row per phoneme) and at frame level (8 frames per
// phoneme; LJSpeech: 7.9), plus the alignment and gap rows of every utterance.  Functions of (phonemes, utterances) only: the host knows both in
// the host- and in the device-driven layout, and a shard that names the whole batch gets the whole batch's numbers.  Any value gives correct
// results; the same value gives the same kernels, hence the same bits.
inline long regime_tokens_of(const fs2_batch& b, bool token_level) {
    if (b.regime_tokens > 0) return (long)b.regime_tokens;
    long n = 0;
    for (int i = 0; i < b.B; ++i) n += (token_level && b.compat_padded) ? (long)b.Tmax : (long)b.ilens[i];      // (padded-batch semantics: the encoder runs on Tmax rows per utterance)
    return n;
}
inline int regime_rows_of(const fs2_batch& b, bool token_level) {
    const long utts = b.regime_utterances > 0 ? b.regime_utterances : b.B;
    return row_bound((token_level ? 1 : 8) * regime_tokens_of(b, token_level), utts);
}
// ... and at SHORT level (FS2_VARSHORT: the variance predictors on at most K frames per phoneme): K frames per phoneme, formed the same way
inline int regime_short_rows_of(const fs2_batch& b, int K) {
    const long utts = b.regime_utterances > 0 ? b.regime_utterances : b.B;
    return row_bound((long long)K * regime_tokens_of(b, false), utts);
}
// K of the variance predictors: var_layers convolutions of var_kernel taps
inline int var_window(const fs2_config& c) { return vs_window(c.var_layers, c.var_kernel); }

// What fs2_encode leaves for the fs2_decode of the same batch: reset as a whole when an accepted fs2_encode starts, filled when it has launched everything.
struct Encoded {
    bool valid = false;
    int B = 0, Tmax = 0, compat = 0;        // the batch, which fs2_decode's must match ...
    const void* ws = nullptr;               // ... and its token workspace, which holds everything below
    const float* rows = nullptr;            // the encoder output [token rows, adim]
    const float* tokP = nullptr;            // tok.proj's output [token rows, tokw.N] (nullptr: not computed)
    bool tokP_conv = false;                 // ... its predictor columns were computed too (else only the input layer's)
    const int *start = nullptr, *vlen = nullptr;      // the token layout: first row and phonemes of every utterance
    const int* cum = nullptr;               // the duration scan: running frame sums [B, Tmax] ...
    const int* o32 = nullptr;               // ... and frame counts [B] (int32; the device-driven layout is built from them)
    const int *scum = nullptr, *so32 = nullptr;      // the same of the short durations min(d, K) (EncodePlan::short_scan; nullptr: not computed)
};

// ------------------------------------------------------------------ checks
// A refusal: the FS2_ERR_* code and the message of the handle (FS2_OK: accepted).  Codes, texts and their order are the entry points' contract.
struct Refusal { int err = FS2_OK; char msg[512] = ""; };
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline Refusal refuse(int err, const char* fmt, ...) {
    Refusal r;
    r.err = err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof r.msg, fmt, ap);
    va_end(ap);
    return r;
}

inline Refusal check_batch(const fs2_batch& b) {
    if (b.B <= 0 || b.Tmax <= 0 || !b.ilens) return refuse(FS2_ERR_ARG, "batch: B=%d Tmax=%d ilens=%p", b.B, b.Tmax, (const void*)b.ilens);
    for (int i = 0; i < b.B; ++i)
        if (b.ilens[i] <= 0 || b.ilens[i] > b.Tmax) return refuse(FS2_ERR_ARG, "ilens[%d]=%lld outside [1,%d]", i, (long long)b.ilens[i], b.Tmax);
    if (b.precision < FS2_PREC_FP32 || b.precision > FS2_PREC_MIX_MX4) return refuse(FS2_ERR_ARG, "unknown precision mode %d", b.precision);
    if (b.regime_tokens < 0 || b.regime_utterances < 0 || (b.regime_tokens > 0) != (b.regime_utterances > 0))
        return refuse(FS2_ERR_ARG, "batch: regime_tokens=%lld / regime_utterances=%d must be given together (0 / 0 = this call's own batch)", (long long)b.regime_tokens, b.regime_utterances);
    return Refusal();
}

// fs2_encode.  enc_pe_rows: the rows of the encoder's positional table (the stored length of an utterance is layout_rule.h's: Tmax under padded-batch semantics).
inline Refusal check_encode(const fs2_encode_io& io, int enc_pe_rows) {
    const fs2_batch& b = io.batch;
    if (const Refusal r = check_batch(b); r.err) return r;
    if (!io.xs || !io.olens || !io.workspace) return refuse(FS2_ERR_ARG, "fs2_encode: xs/olens/workspace must be given");
    if (io.duration_alpha < 0.f) return refuse(FS2_ERR_ARG, "fs2_encode: duration_alpha %g must be > 0 (0 = 1.0)", (double)io.duration_alpha);
    int longest = 0;
    for (int i = 0; i < b.B; ++i) longest = std::max(longest, utt_lens((int)b.ilens[i], b.Tmax, b.compat_padded, /*masked=*/1).len);
    if (longest > enc_pe_rows) return refuse(FS2_ERR_ARG, "sequence longer than the positional table (%d rows): extend `pe` and reload", enc_pe_rows);
    return Refusal();
}

// the device-driven layout: no host frame counts, capacities instead
inline bool device_driven(const fs2_decode_io& io) { return io.olens == nullptr && io.row_capacity > 0; }
inline bool controls(const float* scale, const float* shift) { return scale || shift; }

// fs2_decode / fs2_decode_ctl (ctl == nullptr: no control).  The control is refused as a whole before anything else is looked at.
inline Refusal check_decode(const fs2_decode_io& io, const fs2_prosody* ctl, const Encoded& enc, int idim, int dec_pe_rows) {
    const fs2_batch& b = io.batch;
    const bool ctl_pitch = ctl && controls(ctl->pitch_scale, ctl->pitch_shift), ctl_energy = ctl && controls(ctl->energy_scale, ctl->energy_shift);
    if (ctl_pitch || ctl_energy) {
        const int T = b.Tmax;
        const struct { const float* p; int cols; const char* name; } given[4] = {{ctl->pitch_scale, ctl->pitch_scale_cols, "pitch_scale"}, {ctl->pitch_shift, ctl->pitch_shift_cols, "pitch_shift"},
                                                                                  {ctl->energy_scale, ctl->energy_scale_cols, "energy_scale"}, {ctl->energy_shift, ctl->energy_shift_cols, "energy_shift"}};
        for (const auto& g : given)
            if (g.p && g.cols != 1 && g.cols != T) return refuse(FS2_ERR_ARG, "fs2_decode_ctl: %s_cols = %d is neither 1 (per utterance) nor Tmax = %d (per phoneme)", g.name, g.cols, T);
        if (ctl_pitch && io.ps) return refuse(FS2_ERR_ARG, "fs2_decode_ctl: pitch control together with given pitches (io->ps): control acts on predictions");
        if (ctl_energy && io.es) return refuse(FS2_ERR_ARG, "fs2_decode_ctl: energy control together with given energies (io->es): control acts on predictions");
        if (b.compat_padded) return refuse(FS2_ERR_ARG, "fs2_decode_ctl: control has per-utterance semantics only (batch.compat_padded must be 0)");
    }
    if (!enc.valid) return refuse(FS2_ERR_STATE, "fs2_decode called without a preceding fs2_encode");
    if (const Refusal r = check_batch(b); r.err) return r;
    if (b.B != enc.B || b.Tmax != enc.Tmax || b.compat_padded != enc.compat || io.token_workspace != enc.ws)
        return refuse(FS2_ERR_STATE, "fs2_decode: batch does not match the preceding fs2_encode");
    const bool devlay = device_driven(io);
    if ((!io.olens && !devlay) || !io.workspace || (!io.after && !io.after_packed))
        return refuse(FS2_ERR_ARG, "fs2_decode: olens (or row_capacity) / workspace / after (or after_packed) must be given");
    if (devlay) {
        if (!io.status) return refuse(FS2_ERR_ARG, "fs2_decode: the device-driven layout needs a status buffer");
        if (io.row_capacity > INT32_MAX - 256 || io.Lmax <= 0) return refuse(FS2_ERR_ARG, "row_capacity %lld / Lmax %d", (long long)io.row_capacity, io.Lmax);
    } else {
        int mx = 0;
        for (int i = 0; i < b.B; ++i) {
            if (io.olens[i] == -1) return refuse(FS2_ERR_ARG, "utterance %d holds a phoneme id outside [0, %d) (fs2_encode marks it with the frame count -1)", i, idim);
            if (io.olens[i] <= 0) return refuse(FS2_ERR_ARG, "olens[%d]=%lld", i, (long long)io.olens[i]);
            mx = std::max(mx, (int)io.olens[i]);
        }
        if (io.Lmax < mx) return refuse(FS2_ERR_ARG, "Lmax %d < longest utterance %d", io.Lmax, mx);
        if (mx > dec_pe_rows) return refuse(FS2_ERR_ARG, "utterance of %d frames exceeds the positional table (%d rows): extend `pe` and reload", mx, dec_pe_rows);
    }
    return Refusal();
}

// ------------------------------------------------------------------ decisions: fs2_encode
struct EncodePlan {
    int prec = kPlanFp32, ffn_terms = 0;      // the arithmetic of the GEMMs; the FFN convolution's (model_launches.h: ffn_f16_terms)
    bool planes = false;          // activations also travel as split-bf16 planes (x0p holds those of x0 before and after the stack)
    bool embed_planes = false;    // ... and embed_pe writes the first ones (else the stack builds them: enc.in.planes)
    // tok.proj: the encoder rows times the stacked weights of the predictors' first convolution (one k = 1 product per tap) and of the decoder input layer, once
    // per token instead of once per frame (fs2_decode: var.gather0 / dec.in.gather).  One kernel whatever the batch (64-row tiles, N > 1024: never split-K).
    bool tok_proj = false;
    bool tok_conv = false;        // the predictors' columns too: only where fs2_decode can use them (bit 0 and the fused predictors) ...
    int tok_n0 = 0;               // ... else the launch is sliced to the input layer's columns [n0, N) (a multiple of 128 rows into the weight images: whole tiles)
    int tok_prec = kPlanFp32;     // FS2_TOKPROJ_F32: the exact fp32 GEMM instead of the precision's own arithmetic
    // FS2_VARSHORT: the duration scan also leaves the running sums of the short durations -- wherever fs2_decode can take the short path (DecodePlan::varshort)
    bool short_scan = false;
};
// tokw_N: the columns of the model's stacked tok.proj weight (0: it has none); tokp_buf: the token workspace has the buffer for its output
// short_buf: the token workspace can hold the short scan and the batch has per-utterance semantics
inline EncodePlan plan_encode(const fs2_config& c, const Options& o, int precision, int tokw_N, bool tokp_buf, bool short_buf = false) {
    EncodePlan p;
    p.prec = base_precision(precision); p.ffn_terms = ffn_f16_terms(precision);
    p.planes = p.prec != kPlanFp32;
    p.embed_planes = p.planes && c.adim % 32 == 0;
    p.tok_proj = p.planes && tokw_N && tokp_buf && o.tokproj;
    p.tok_conv = p.tok_proj && (o.tokproj & 1) && o.fuse_var;
    p.tok_n0 = (p.tok_proj && !p.tok_conv) ? 6 * c.var_chans : 0;
    p.tok_prec = o.tokproj_f32 ? kPlanFp32 : p.prec;
    p.short_scan = p.tok_conv && (o.tokproj & 3) == 3 && o.varshort && short_buf;
    return p;
}

// ------------------------------------------------------------------ decisions: fs2_decode
// Which pointers of fs2_decode_io (and of the control) a call gives, and the scalars the decisions read.
struct DecodeAsk {
    bool devlay = false;                      // device_driven(io)
    bool es = false, ps = false;              // energies / pitches given (else predicted)
    bool e_out = false, p_out = false, dec_out = false, after = false, before = false, after_packed = false;
    bool ctl_pitch = false, ctl_energy = false;
    bool after_vec = false, before_vec = false;      // unpack_vec(odim, the rows that output is unpacked from, the output): unpack_rows4 writes it
    int compat = 0, masked = 0;
    bool short_buf = false;                   // the frame workspace can hold the short layout (FS2_VARSHORT)
    long R = 0; long long row_capacity = 0;   // the rows of the frame layout; the capacity the caller's after_packed holds
};
inline DecodeAsk decode_ask(const fs2_decode_io& io, const fs2_prosody* ctl) {
    DecodeAsk a;
    a.devlay = device_driven(io);
    a.es = io.es; a.ps = io.ps; a.e_out = io.e_out; a.p_out = io.p_out; a.dec_out = io.dec_out; a.after = io.after; a.before = io.before; a.after_packed = io.after_packed;
    a.ctl_pitch = ctl && controls(ctl->pitch_scale, ctl->pitch_shift); a.ctl_energy = ctl && controls(ctl->energy_scale, ctl->energy_shift);
    a.compat = io.batch.compat_padded; a.masked = io.masked; a.row_capacity = io.row_capacity;
    return a;
}
// unpack's fast path (unpack_rows4: float4 copies that look at the overflow flags themselves): fp32 rows of W % 4 == 0 channels, zero fill, both ends 16-byte aligned
inline bool unpack_vec(int W, const void* src, const void* dst) { return W % 4 == 0 && (reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) % 16 == 0; }

struct DecodePlan {
    int prec = kPlanFp32, ffn_terms = 0;
    bool devlay = false;
    bool planes = false;          // activations also travel as planes through the decoder and the tail
    // bf16 modes: the length-regulator output (and later its sum with the pitch / energy embeddings) is also written as planes, in x1p (free until the
    // decoder stack's first LayerNorm): the A operand of both variance predictors and of the decoder input layer
    bool hfr_planes = false;
    bool need_e = false, need_p = false;      // the energy / the pitch predictor runs: nothing given to quantise, or its output is asked for
    bool fused_var = false;       // ... both as one launch per layer (FusedPredictors)
    // Multiply before expanding (FS2_TOKPROJ; a function of the model, the precision and which outputs are asked for -- never of the batch): the predictors' first
    // layer (bit 0; where the fused predictors run) and the decoder input layer (bit 1) gather fs2_encode's token-level products; with both (3) nothing reads the
    // expanded rows, which are then not built: lr.index in place of lr.expand, no var.embed.
    int tokproj = 0;
    // FS2_VARSHORT (layout_rule.h): the fused predictors, the control and the bucket search of the predictions run on the short rows -- at most K frames
    // per phoneme -- which lr.index lays out beside the token index; dec.in.gather reads the bucket indices through the frame-to-short map, and e_out /
    // p_out, where asked for, are unpacked through it.  Where nothing reads the expanded rows (tokproj == 3) and the batch has per-utterance semantics;
    // a function of configuration and options like tokproj -- never of the batch's data.
    bool varshort = false;
    bool short_qe = false, short_qp = false;      // ... that index is searched per short row (else per frame: es / ps given)
    bool control = false;         // var.control: the predictions become the controlled values in place
    // Planes-only residual stream (model_launches.h: planes_only): the decoder's LayerNorm-fused launches write planes and nothing else -- the fp32 rows x0 / x1
    // are not written at all, and dec_out, where asked for, is rebuilt from the planes (dec.out.rows).
    bool po = false;
    int mask_q = 0;               // the decoder attention masks the queries behind an utterance's own length (padded-batch semantics, teacher-forced)
    int rf = 1;                   // reduction_factor: mel frames per decoder row; > 1: the Postnet runs on a layout of its own, rf rows per decoder row
    bool post_pl = false;         // planes hand-off through the tail: feat_out writes the planes the Postnet's first layer reads (rf > 1: they would be in the decoder-row layout)
    bool ep_stored = false;       // e_out / p_out are unpacked up to every stored row (pads carry real values: padded batch, unmasked), else up to the valid frames
    // Device-driven layout: the kernels that write the mel outputs look at the overflow flags themselves and write NaN when a capacity was too small (nobody can
    // mistake the outputs of such a call for silence): unpack_rows4 where it applies, pack_rows where its grid covers the whole capacity.  poison_on_overflow
    // covers the outputs they leave.
    bool packed_ovf = false;      // pack_rows checks the flags itself
    bool poison_after = false, poison_before = false, poison_packed = false;
    bool poison() const { return poison_after || poison_before || poison_packed; }
};
// enc: what the encode left; in / dec / r / b: the decoder's input layer (in.g == nullptr: none), stack, rows and buffers, as planes_only takes them
inline DecodePlan plan_decode(const fs2_config& c, const Options& o, int precision, const DecodeAsk& a, const Encoded& enc, bool var2_ok, const DecIn& in, const Stack& dec, const Rows& r,
                              const StackBufs& b) {
    DecodePlan p;
    p.prec = base_precision(precision); p.ffn_terms = ffn_f16_terms(precision);
    p.devlay = a.devlay;
    p.planes = p.prec != kPlanFp32;
    p.hfr_planes = p.planes && c.adim % 32 == 0;
    p.need_e = !a.es || a.e_out; p.need_p = !a.ps || a.p_out;
    p.fused_var = p.need_e && p.need_p && p.planes && var2_ok && p.hfr_planes && o.fuse_var;
    p.tokproj = (p.planes && enc.tokP && c.decoder_input_layer) ? (o.tokproj & ((p.fused_var && enc.tokP_conv) ? 3 : 2)) : 0;
    p.varshort = p.tokproj == 3 && o.varshort && enc.scum && a.short_buf && !a.compat;
    p.short_qe = p.varshort && !a.es; p.short_qp = p.varshort && !a.ps;
    p.control = a.ctl_pitch || a.ctl_energy;
    p.po = p.planes && planes_only(in, dec, c.ddim, r, b, p.prec, p.ffn_terms, o);
    p.mask_q = (a.compat && a.masked) ? 1 : 0;
    p.rf = std::max(c.reduction_factor, 1);
    p.post_pl = p.planes && c.postnet_layers > 1 && p.rf == 1;
    p.ep_stored = a.compat && !a.masked;
    p.packed_ovf = a.devlay && a.R == a.row_capacity;
    p.poison_after = a.devlay && a.after && !a.after_vec;
    p.poison_before = a.devlay && a.before && !a.before_vec;
    p.poison_packed = a.devlay && a.after_packed && !p.packed_ovf;
    return p;
}

}  // namespace fs2
