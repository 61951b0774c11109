// The host side of the operators that fill one distance matrix per pair of sequences and sweep it, fs2_op_dtw (dtw.h) and fs2_op_align
// (align.h; DESIGN.md sections 14.6, 14.7), ONCE: the workspace layout (the pair records, the pairs' result records, then per group of
// pairs their d matrices and edge buffers) and its query, the argument checks, the pair records, their upload chunks and -- the one
// decision -- which consecutive pairs share a group (one dtw_dist and one sweep launch, one stretch of the workspace).  Only pair_walk
// decides that: the uploaded records (tile0, d_off) and the launch parameters (first, count, tiles) are two views of the same walk.
// Plain C++, no HIP construct, nothing allocated: tests/pair_plan_probe.cpp compiles it with the host compiler.  Not a header of its
// own: dtw.h includes it at its top, inside the includer's unnamed namespace, after fail() and align_up() (losses.h).  It includes
// record_op.h for that header's plain C++ half: the struct_size, row and workspace checks, the workspace carve and the upload chunks.
#pragma once
#include "record_op.h"
constexpr int kPairCols = 256, kPairTile = 64;      // = kDtwCols, kDtwTile (dtw.h asserts it): a column block of dtw_sweep, a tile of dtw_dist
constexpr int kDtwMaxD = 128;
constexpr int kDtwCellBytes = 48;         // sizeof(DtwCell) (dtw.h): one entry of an edge buffer
constexpr int kDtwRecsPerChunk = 96;      // pair records per upload launch (kernel-argument bytes: 96 * 40 + 8 < 4 KB)
constexpr int64_t kDtwMaxCells = (int64_t)1 << 40;

// what differs between the operators
struct PairOp {
    const char *who, *args;      // the names in messages: the operator, its argument struct
    int terms;            // doubles of a result record
    bool swapped;         // dtw_dist gets the caller's b side as its a side: d is kept [M, N] (align.h says why)
    bool edges;           // a pair of more than kPairCols columns owns two edge buffers, [2, n] cells, behind its d
};
constexpr PairOp kDtwOp{"fs2_op_dtw", "fs2_op_dtw_args", FS2_DTW_TERMS, false, true}, kAlignOp{"fs2_op_align", "fs2_op_align_args", FS2_ALIGN_TERMS, true, false};

struct DtwPair {
    int a0, n, b0, m;         // first row and rows of the a side, of the b side (as dtw_dist gets them: PairOp::swapped)
    int tile0, tcols;         // first tile of the pair in its group's dtw_dist grid, tiles per tile row
    int64_t d_off;            // byte offset in the workspace of d [n, m] double
    int64_t aux;              // fs2_op_dtw: byte offset in the workspace of the two edge buffers; fs2_op_align: n_labels (-1: no labels)
};
using DtwPairChunk = RecChunk<DtwPair, kDtwRecsPerChunk>;               // one upload launch: the records [base, base + n)
static_assert(sizeof(DtwPair) == 40, "the records travel as kernel arguments");

// the pair records, the pairs' result records (their addresses in the workspace it was carved from, and their byte offsets), then from
// byte off_group the groups' matrices: `all` bytes hold every pair's at once, `largest` the largest pair's alone
struct DtwLayout { DtwPair* recs; double* terms; size_t off_recs, off_terms, off_group, all, largest; };

inline int64_t dtw_tiles(int32_t n, int32_t m) { return (((int64_t)n + kPairTile - 1) / kPairTile) * (((int64_t)m + kPairTile - 1) / kPairTile); }
inline size_t dtw_d_bytes(int32_t n, int32_t m) { return n && m ? align_up((size_t)n * (size_t)m * sizeof(double), 256) : 0; }
// (n, m: the shape as dtw_dist gets it)
inline size_t pair_bytes(const PairOp& op, int32_t n, int32_t m) {
    if (!n || !m) return 0;
    return dtw_d_bytes(n, m) + (op.edges && m > kPairCols ? align_up(2 * (size_t)n * kDtwCellBytes, 256) : 0);
}

// false: a negative length, or a matrix of more than kDtwMaxCells cells
inline bool pair_regions(const PairOp& op, int32_t B, const int32_t* a_lens, const int32_t* b_lens, void* ws, DtwLayout& r) {
    size_t sum = 0, largest = 0;
    for (int b = 0; b < B; ++b) {
        if (a_lens[b] < 0 || b_lens[b] < 0 || (int64_t)a_lens[b] * b_lens[b] > kDtwMaxCells) return false;
        const size_t pb = op.swapped ? pair_bytes(op, b_lens[b], a_lens[b]) : pair_bytes(op, a_lens[b], b_lens[b]);
        sum += pb;
        largest = std::max(largest, pb);
    }
    Carve c{(char*)ws};
    r = DtwLayout{};
    r.recs = c.take<DtwPair>(B);
    r.off_terms = c.off;
    r.terms = c.take<double>(B, (size_t)op.terms);
    r.off_group = c.off;
    r.all = c.off + sum;
    r.largest = c.off + largest;
    return true;
}

inline size_t pair_workspace_bytes(const PairOp& op, int32_t B, const int32_t* a_lens, const int32_t* b_lens, size_t cap_bytes) {
    DtwLayout r;
    if (B < 0 || (B > 0 && (!a_lens || !b_lens)) || !pair_regions(op, B, a_lens, b_lens, nullptr, r)) return 0;
    return std::min(r.all, std::max(cap_bytes, r.largest));
}

// the checks of the arguments both fs2_op_*_args have (same names, same meaning); an operator's own checks follow in its file
template <class Args> int pair_check_args(const PairOp& op, const Args* a) {
    const char* who = op.who;
    if (const int rc = rec_check_struct(who, op.args, a)) return rc;
    const int32_t B = a->B;
    if (B < 0 || (B > 0 && (!a->a_starts || !a->a_lens || !a->b_starts || !a->b_lens)))
        return fail(nullptr, FS2_ERR_ARG, "%s: bad batch (B = %d) or null a_starts / a_lens / b_starts / b_lens", who, B);
    if (a->D < 1 || a->D > kDtwMaxD) return fail(nullptr, FS2_ERR_ARG, "%s: D = %d outside [1, %d]", who, a->D, kDtwMaxD);
    if (a->a_stride < a->D || a->b_stride < a->D)
        return fail(nullptr, FS2_ERR_ARG, "%s: row stride %lld / %lld below D = %d", who, (long long)a->a_stride, (long long)a->b_stride, a->D);
    if (const int rc = rec_check_rows(who, "pair", B, a->a_starts, a->a_lens)) return rc;
    if (const int rc = rec_check_rows(who, "pair", B, a->b_starts, a->b_lens)) return rc;
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || (a->a_lens[b] > 0 && a->b_lens[b] > 0);
    if (any && (!a->a || !a->b)) return fail(nullptr, FS2_ERR_ARG, "%s: null a / b", who);
    return FS2_OK;
}

// a checked batch, its sides as dtw_dist gets them (PairOp::swapped is applied when the plan is made; the walk and the launches do not know of it)
struct PairPlan {
    const PairOp* op;
    int32_t B, D;
    const float *a, *b;
    int64_t a_stride, b_stride;
    const int32_t *a_starts, *a_lens, *b_starts, *b_lens, *n_labels;      // n_labels: null without labels (and for fs2_op_dtw)
    DtwLayout at;                                                       // (B = 0: no workspace, recs and terms null, and nobody reads either)
    size_t avail;                                                         // workspace bytes for a group's matrices
};

// after pair_check_args: the regions and the workspace checks -> p
template <class Args> int pair_plan(const PairOp& op, const Args* a, const int32_t* n_labels, PairPlan& p) {
    DtwLayout at;
    if (!pair_regions(op, a->B, a->a_lens, a->b_lens, a->workspace, at)) return fail(nullptr, FS2_ERR_ARG, "%s: a matrix of more than 2^40 cells", op.who);
    if (const int rc = rec_check_workspace(op.who, a->B, a->workspace, a->workspace_bytes, at.largest, " (the largest pair alone)")) return rc;
    const size_t avail = a->B > 0 ? a->workspace_bytes - at.off_group : 0;
    if (op.swapped) p = PairPlan{&op, a->B, a->D, a->b, a->a, a->b_stride, a->a_stride, a->b_starts, a->b_lens, a->a_starts, a->a_lens, n_labels, at, avail};
    else p = PairPlan{&op, a->B, a->D, a->a, a->b, a->a_stride, a->b_stride, a->a_starts, a->a_lens, a->b_starts, a->b_lens, n_labels, at, avail};
    return FS2_OK;
}

// consecutive pairs share a group while their matrices fit `avail` bytes and their tiles one grid
struct DtwGroups {
    size_t avail, used = 0;
    int64_t tiles = 0;
    int count = 0;
    // -> true if the pair opens a new group (the caller closes the previous one first)
    bool opens(size_t pair_bytes, int64_t pair_tiles) const {
        return count > 0 && (used + pair_bytes > avail || tiles + pair_tiles > INT32_MAX);
    }
    void reset() { used = 0; tiles = 0; count = 0; }
    void add(size_t pair_bytes, int64_t pair_tiles) { used += pair_bytes; tiles += pair_tiles; ++count; }
};
struct PairGroup { int first, count; int64_t tiles; };      // the pairs [first, first + count); tiles of dtw_dist's grid (0: all pairs empty)

// THE walk: record(i, DtwPair) for every pair in index order, group(PairGroup) when a group is complete (before the record that opens the next)
template <class R, class G> void pair_walk(const PairPlan& p, R&& record, G&& group) {
    DtwGroups g{p.avail};
    int first = 0;
    for (int i = 0; i < p.B; ++i) {
        const int32_t n = p.a_lens[i], m = p.b_lens[i];
        const size_t pb = pair_bytes(*p.op, n, m);
        const int64_t nt = n && m ? dtw_tiles(n, m) : 0;
        if (g.opens(pb, nt)) { group(PairGroup{first, g.count, g.tiles}); first = i; g.reset(); }
        const int64_t d_off = (int64_t)(p.at.off_group + g.used);
        record(i, DtwPair{p.a_starts[i], n, p.b_starts[i], m, (int)g.tiles, (int)(((int64_t)m + kPairTile - 1) / kPairTile), d_off,
                          p.op->edges ? d_off + (int64_t)dtw_d_bytes(n, m) : p.n_labels ? (int64_t)p.n_labels[i] : (int64_t)-1});
        g.add(pb, nt);
    }
    if (g.count > 0) group(PairGroup{first, g.count, g.tiles});
}

// the records in chunks of kDtwRecsPerChunk, each handed to upload(const DtwPairChunk&): ceil(B / kDtwRecsPerChunk) calls
template <class F> void pair_chunks(const PairPlan& p, F&& upload) {
    auto ch = rec_chunker<DtwPair, kDtwRecsPerChunk>(p.B, upload);
    pair_walk(p, [&](int i, const DtwPair& r) { ch.put(i, r); }, [](const PairGroup&) {});
}

// body(const PairGroup&) per group, in index order: the caller launches dtw_dist and its own sweep
template <class F> void pair_groups(const PairPlan& p, F&& body) { pair_walk(p, [](int, const DtwPair&) {}, body); }
