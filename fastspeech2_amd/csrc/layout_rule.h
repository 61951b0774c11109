// The gapped packed-row layout and the attention work list, stated once, for the host builder (layout.h:
// build_layout), the device builder (layout.h: frame_layout_dev) and the runtime's capacity and workspace formulas.  Plain C++ with no
// HIP dependency: tests/test_layout_host.py compiles it with the host compiler (tests/layout_probe.cpp) and compares it with the rule
// restated in Python.
//
// Rows: utterance b owns rows [start[b], start[b] + len[b]) of every activation buffer.  The running row begins at `gap`; every start
// is rounded up to kAttAlign rows, `gap` zero rows follow every utterance, kTailRows more follow the last one.
// Work list: (utterance, kAttBlk-query block) items in kXcds interleaved queues (entry kXcds i + j = i-th item of queue j: workgroup
// x of a launch runs on XCD x % kXcds, and every XCD has its own L2, so all blocks of an utterance go to one queue).  Utterances are
// dealt longest key range first, each to the currently shortest queue; the queues are padded to one depth with (-1, 0) items.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define LR_HD __host__ __device__
#define LR_UNROLL _Pragma("unroll")
#else
#define LR_HD
#define LR_UNROLL
#endif

namespace fs2 {

constexpr int kGap = 8;         // upper bound of the zero rows between packed sequences (capacity formulas); a model uses
constexpr int kMinGap = 4;      // max(kMinGap, its largest conv halo (k - 1) / 2): 4 for the default 9-tap FFN (fs2_handle::gap)
constexpr int kTailRows = 8;    // zero rows every layout appends behind its last utterance (attn_bf16.h: V^T vectors that straddle the last key)
constexpr int kAttAlign = 8;    // utterance starts are multiples of this many rows: a 16-byte V^T load is 8 consecutive keys (rows).
                                // (Round 1 used 32: an average of 12 more dead rows per utterance in every row-proportional kernel, 2.6 % at c3.)
constexpr int kAttBlk = 128;    // queries per work-list item: one workgroup of attn_w32 (4 waves x 32), two of the 64-query kernels
constexpr int kXcds = 8;        // MI355X: 8 accelerator dies, workgroups of a launch are dealt to them round-robin
constexpr int kRowTile = 128;   // Rpad: the row count every buffer is sized for is a multiple of the tallest GEMM tile
constexpr int kRowLimit = 0x7fffffff - 256;      // the most rows a capacity may name
static_assert((kAttAlign & (kAttAlign - 1)) == 0 && kGap <= kAttAlign && kMinGap <= kGap, "row_start rounds with a mask; an empty layout starts at kAttAlign");

// overflow flags of the device-driven layout: include/fs2.h FS2_OVF_* (fs2_runtime.hip asserts the equality)
constexpr int kOvfRows = 1, kOvfLmax = 2, kOvfPe = 4, kOvfEmpty = 8, kOvfBadId = 16;

LR_HD constexpr int lr_max(int a, int b) { return a > b ? a : b; }
LR_HD constexpr int lr_round_up(int x, int a) { return (x + a - 1) / a * a; }

// ---- lengths: rows stored (len), attention keys (klen) and true length (vlen) of an utterance of `valid` positions in a batch whose
// longest has `longest`.  compat (padded-batch semantics): every utterance is stored at the longest's length and, unless masked,
// attends over all of it.
struct UttLens { int len, klen, vlen; };
LR_HD constexpr bool keys_are_own(int compat, int masked) { return !compat || masked; }      // else every utterance attends over `longest` keys
LR_HD constexpr UttLens utt_lens(int valid, int longest, int compat, int masked) {
    return UttLens{compat ? longest : valid, keys_are_own(compat, masked) ? valid : longest, valid};
}

// ---- row walk: row = gap; per utterance { start = row_start(row); row = row_after(start, len, gap); }; rows_used(row)
LR_HD constexpr int row_start(int row) { return (row + kAttAlign - 1) & ~(kAttAlign - 1); }
LR_HD constexpr int row_after(int start, int len, int gap) { return start + len + gap; }
LR_HD constexpr int rows_used(int row) { return row + kTailRows; }
LR_HD constexpr int rows_padded(int rows) { return lr_round_up(rows, kRowTile); }

// ---- attention blocks of an utterance of len >= 0 rows
LR_HD constexpr int att_blocks(int len) { return (int)((unsigned)(len + kAttBlk - 1) / (unsigned)kAttBlk); }
// ---- grid.x of the 64-query kernels (attn_f32, attn_bf16) over a work list of nitems: 2 x (items rounded up to a multiple of kXcds) workgroups;
// common.h: att_item64 says which half of which item workgroup x serves
LR_HD constexpr unsigned att_grid64(int nitems) { return 2u * (unsigned)((nitems + kXcds - 1) & ~(kXcds - 1)); }

// ---- dealing order: utterance a (key range ka) is dealt before utterance b (kb): longer key range first, ties in batch order.
// A strict total order: the host sorts by it, the device counts for every utterance those dealt before it.
LR_HD constexpr bool dealt_before(int ka, int a, int kb, int b) { return ka > kb || (ka == kb && a < b); }

// ---- dealing: place() gives an utterance's blocks to the shortest queue (the lowest on ties) and returns the list position of its
// first item; the next ones follow kXcds apart.  qlen is only ever indexed by unrolled constants, so on the device it stays in registers.
struct Dealer {
    int qlen[kXcds] = {};
    int depth = 0;            // the longest queue
    LR_HD int place(int blocks) {
        int j = 0, best = qlen[0];
        LR_UNROLL
        for (int t = 1; t < kXcds; ++t)
            if (qlen[t] < best) { best = qlen[t]; j = t; }
        LR_UNROLL
        for (int t = 0; t < kXcds; ++t) qlen[t] += (t == j) ? blocks : 0;
        depth = lr_max(depth, best + blocks);
        return best * kXcds + j;
    }
    LR_HD int items() const { return depth * kXcds; }      // list length, padding included
};

// ---- the flags word of the device-driven layout: what the batch needs against what the caller reserved.  smallest: the least frame
// count as the duration scan left it (-1 marks an utterance with a phoneme id out of range).
LR_HD constexpr int overflow_flags(int rows, int depth, int longest, int smallest, int row_cap, int work_cap, int lmax_cap, int pe_rows) {
    return ((rows > row_cap || depth * kXcds > work_cap) ? kOvfRows : 0) | (longest > lmax_cap ? kOvfLmax : 0) | (longest > pe_rows ? kOvfPe : 0) |
           (smallest < 0 ? kOvfBadId : (smallest <= 0 ? kOvfEmpty : 0));
}

// ---- capacities
// rows that `frames` positions in `utts` utterances take at most: the first start is kAttAlign, every later one rounds up by less than
// kAttAlign, at most kGap rows follow each utterance and kTailRows the last (8 + 15 (utts - 1) + 8 + 8 <= 16 utts + 8)
LR_HD constexpr int row_bound(long long frames, long long utts) {
    const long long r = frames + utts * (kGap + kAttAlign) + kGap;
    return (int)(r < kRowLimit ? r : kRowLimit);
}
// work-list entries that suffice whenever the rows fit row_capacity and no utterance exceeds lmax_cap: no queue is longer than the
// mean (at most row_capacity / kAttBlk + B blocks over kXcds queues) plus one utterance's blocks
LR_HD constexpr int work_capacity(long long row_capacity, int B, int lmax_cap) {
    return kXcds * (((int)(row_capacity / kAttBlk) + B + kXcds - 1) / kXcds + lmax_cap / kAttBlk + 2);
}

// ---- the `meta` block: int offsets of the layout arrays inside one workspace region.  dims (16 ints reserved) and row_pos are
// 16-byte aligned for the kernels' vector loads.  The alignment is taken on the OFFSET: the region starts at a Bump::take, which is
// 256 bytes from a workspace base that is itself an allocation (hipMalloc / the caching allocator: 256-byte aligned or more), so an
// offset that is a multiple of 4 ints is a 16-byte aligned address.  end <= ints(...) of the same form: the `slack` ints cover the
// two roundings (3 ints each at most).
constexpr int kDimsInts = 16, kMetaSlack = 64;
LR_HD constexpr long long meta_align(long long i) { return (i + 3) & ~3LL; }

struct MetaHost {       // host-driven: start | len | klen | vlen | work, uploaded in one copy; row_pos | row_seq built on the device
    long long start, len, klen, vlen, work, row_pos, row_seq, end;
    LR_HD static constexpr MetaHost at(long long B, long long Rpad, long long nwork) {
        const long long rp = meta_align(4 * B + 2 * nwork);
        return MetaHost{0, B, 2 * B, 3 * B, 4 * B, rp, rp + Rpad, rp + 2 * Rpad};
    }
};
struct MetaDev {        // device-driven: everything is written by frame_layout_dev (rank, woff: its scratch) and build_row_meta
    long long start, len, klen, vlen, rank, woff, pcum, dims, work, row_pos, row_seq, end;
    LR_HD static constexpr MetaDev at(long long B, long long Rpad, long long nwork) {
        const long long d = meta_align(7 * B), w = d + kDimsInts, rp = meta_align(w + 2 * nwork);
        return MetaDev{0, B, 2 * B, 3 * B, 4 * B, 5 * B, 6 * B, d, w, rp, rp + Rpad, rp + 2 * Rpad};
    }
    // what either form takes: seven arrays of B, dims, the work list (two ints per item), two arrays of Rpad
    LR_HD static constexpr long long ints(long long B, long long Rpad, long long nwork) { return 7 * B + kDimsInts + 2 * nwork + 2 * Rpad + kMetaSlack; }
};
struct Meta2 {          // reduction factor r > 1: the Postnet's layout, Rpad2 = r Rpad rows (scale_layout, build_row_meta); klen = len
    long long start, len, vlen, dims, row_pos, row_seq, end;
    LR_HD static constexpr Meta2 at(long long B, long long Rpad2) {
        const long long d = meta_align(3 * B), rp = d + kDimsInts;
        return Meta2{0, B, 2 * B, d, rp, rp + Rpad2, rp + 2 * Rpad2};
    }
    LR_HD static constexpr long long ints(long long B, long long Rpad2) { return 4 * B + 2 * Rpad2 + kMetaSlack; }
};

// ---- the variance predictors on at most K frames per phoneme (FS2_VARSHORT; DESIGN.md: "Variance predictors on short rows"), for the host (call_plan.h,
// fs2_runtime.hip) and the device (varshort.h; elementwise.h: dur_scan); tests/test_varshort_host.py compares it with the rule restated in Python
// (tests/varshort_probe.cpp).  The length regulator repeats a phoneme's encoder row d times, and a predictor is a stack of convolutions whose outputs are taken
// per frame: the output at offset o of the phoneme depends on the inputs at most h = sum of the layers' halos (kernel - 1) / 2 frames away, so every frame that
// has h frames of its own phoneme on both sides sees the same inputs and gives the same output.  The SHORT sequence keeps min(d, K) frames of every phoneme,
// K = 1 + 2 h: its first h, its last h and one interior frame; the predictor on the short sequence gives, row for row, the values of the full sequence at the
// kept frames, and every other frame takes the interior one's.
// K = 1 + sum over the layers of (kernel - 1): `layers` convolutions of `kernel` taps (odd)
LR_HD constexpr int vs_window(int layers, int kernel) { return 1 + layers * (kernel - 1); }
// frames a phoneme of d frames keeps
LR_HD constexpr int vs_short_dur(int d, int K) { return d <= 0 ? 0 : (d < K ? d : K); }
// offset inside the short phoneme of the frame at offset o (0 <= o < d) of a phoneme of d frames: the first h and the last h keep their
// distance to their edge, everything between them is the interior frame h; d <= K: nothing is dropped
LR_HD constexpr int vs_short_offset(int o, int d, int K) {
    const int h = (K - 1) / 2;
    return d <= K ? o : (o < h ? o : (o >= d - h ? K - (d - o) : h));
}
// rows the short layout takes at most: no phoneme keeps more than K frames and none more than it has, so the short durations sum to at most
// min(frame bound, K x phonemes) -- the short layout cannot overflow what this sizes, and has no overflow flag
LR_HD constexpr int vs_row_bound(long long frames_bound, long long phonemes, long long utts, int K) {
    const long long kp = (long long)K * phonemes;
    return row_bound(frames_bound < kp ? frames_bound : kp, utts);
}

}  // namespace fs2
