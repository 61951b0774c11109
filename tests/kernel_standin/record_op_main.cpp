// The scaffold of the record operators (csrc/record_op.h) on the host stand-in, on hand-made data (tests/test_record_op_host.py).
//   record_op_main --combine IN OUT   IN: int32 op, B; float64 recs[B][TERMS].  OUT: float64 terms[B][TERMS], batch[TERMS] of the
//                                     operator's records_combine instantiation (op: 2 dtw, 3 align, 4 pitch path)
//   record_op_main --upload KIND B    upload_recs through rec_chunker: KIND 0 a record of two ints in chunks of 4, KIND 1 the pair
//                                     record in chunks of 96.  Prints "chunk base n" per launch and "landed 1" when record i holds
//                                     the values made for index i, for every i < B
//   record_op_main --workspace IN     IN: int32 count; per case int32 op, B, nulls (bit 0: a_lens, bit 1: b_lens), n, uint64 cap,
//                                     int32 a_lens[n], b_lens[n] (op: 0 targets, 1 losses, 2 dtw, 3 align, 4 pitch path).  Prints per
//                                     case the *_workspace_bytes query, then the byte offsets of the operator's regions in a workspace
//                                     (-1 where the operator refuses the lengths)
// Every buffer a kernel writes is a heap block of exactly its size, so that a sanitizer build sees a write beyond it.
#include "standin_host.h"
#include "hip_standin_record.h"
template <typename T> T __shfl(T v, int src) { return shfl_from(v, src); }
namespace {
#include "targets.h"
#include "losses.h"
#include "dtw.h"
#include "align.h"
#include "pitch_path.h"

int combine(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    int32_t h[2];
    if (!f || fread(h, 4, 2, f) != 2) return 2;
    const int op = h[0], B = h[1], T = op == 2 ? kDtwTerms : op == 3 ? kAlignTerms : kPathTerms;
    std::vector<double> recs((size_t)B * T), terms((size_t)B * T, -777.0), batch(T, -777.0);
    if (!recs.empty() && fread(recs.data(), 8, recs.size(), f) != recs.size()) return 2;
    fclose(f);
    if (op == 2) hipLaunchKernelGGL((records_combine<kDtwTerms, -1, -1>), dim3(1), dim3(256), 0, nullptr, recs.data(), B, terms.data(), batch.data());
    else if (op == 3) hipLaunchKernelGGL((records_combine<kAlignTerms, 2, -1>), dim3(1), dim3(256), 0, nullptr, recs.data(), B, terms.data(), batch.data());
    else hipLaunchKernelGGL((records_combine<kPathTerms, 1, 5>), dim3(1), dim3(256), 0, nullptr, recs.data(), B, terms.data(), batch.data());
    FILE* o = fopen(out, "wb");
    if (!o) return 2;
    if (B) fwrite(terms.data(), 8, terms.size(), o);
    fwrite(batch.data(), 8, batch.size(), o);
    fclose(o);
    return 0;
}

struct Two { int a, b; };
inline Two make(int i, Two*) { return Two{i, ~i}; }
inline DtwPair make(int i, DtwPair*) { return DtwPair{i, i + 1, i + 2, i + 3, i + 4, i + 5, (int64_t)i * 1000003, -(int64_t)i}; }
inline bool same(const Two& x, const Two& y) { return x.a == y.a && x.b == y.b; }
inline bool same(const DtwPair& x, const DtwPair& y) {
    return x.a0 == y.a0 && x.n == y.n && x.b0 == y.b0 && x.m == y.m && x.tile0 == y.tile0 && x.tcols == y.tcols && x.d_off == y.d_off && x.aux == y.aux;
}

template <class Rec, int N> int upload(int B) {
    std::vector<Rec> dst((size_t)B, make(-7, (Rec*)nullptr));
    auto launch = upload_launch<Rec, N>(dst.data(), nullptr);
    auto ch = rec_chunker<Rec, N>(B, [&](const RecChunk<Rec, N>& c) { printf("chunk %d %d\n", c.base, c.n); launch(c); });
    for (int i = 0; i < B; ++i) ch.put(i, make(i, (Rec*)nullptr));
    bool ok = true;
    for (int i = 0; i < B; ++i) ok = ok && same(dst[i], make(i, (Rec*)nullptr));
    printf("landed %d\n", (int)ok);
    return 0;
}

int workspace(const char* path) {
    alignas(256) static char ws[256];      // the regions' addresses are formed, never followed
    FILE* f = fopen(path, "rb");
    int32_t count = 0;
    if (!f || fread(&count, 4, 1, f) != 1) return 2;
    for (int i = 0; i < count; ++i) {
        int32_t h[4];
        uint64_t cap;
        if (fread(h, 4, 4, f) != 4 || fread(&cap, 8, 1, f) != 1) return 2;
        std::vector<int32_t> lens(2 * (size_t)h[3]);
        if (!lens.empty() && fread(lens.data(), 4, lens.size(), f) != lens.size()) return 2;
        const int32_t op = h[0], B = h[1], *al = (h[2] & 1) ? nullptr : lens.data(), *bl = (h[2] & 2) ? nullptr : lens.data() + h[3];
        const size_t bytes = op == 0 ? tg_workspace_bytes(B) : op == 1 ? lt_workspace_bytes(B, al) : op == 2 ? dtw_workspace_bytes(B, al, bl, (size_t)cap)
                           : op == 3 ? align_workspace_bytes(B, al, bl, (size_t)cap) : path_workspace_bytes(B, al);
        long long o0 = -1, o1 = -1, end = -1;
        const bool lens_given = B == 0 || (B > 0 && al && (bl || op < 2 || op == 4));
        if (op == 0 && B >= 0) {
            const TgLayout r = tg_layout(B, ws);
            o0 = (char*)r.recs - ws; o1 = (char*)r.partials - ws; end = (long long)r.bytes;
        } else if (op == 1 && lens_given) {
            LtRegions r;
            if (lt_regions(B, al, ws, r)) { o0 = (char*)r.recs - ws; o1 = (char*)r.partials - ws; end = (long long)r.bytes; }
        } else if ((op == 2 || op == 3) && lens_given) {
            DtwLayout r;
            if (pair_regions(op == 2 ? kDtwOp : kAlignOp, B, al, bl, ws, r)) { o0 = (char*)r.recs - ws; o1 = (char*)r.terms - ws; end = (long long)r.off_group; }
        } else if (op == 4 && lens_given) {
            PathRegions r;
            if (path_regions(B, al, ws, r)) { o0 = (char*)r.recs - ws; o1 = (char*)r.words - ws; end = (long long)r.bytes; }
        }
        printf("%zu %lld %lld %lld\n", bytes, o0, o1, end);
    }
    fclose(f);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--combine")) return combine(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "--upload")) return atoi(argv[2]) ? upload<DtwPair, kDtwRecsPerChunk>(atoi(argv[3])) : upload<Two, 4>(atoi(argv[3]));
    if (argc == 3 && !strcmp(argv[1], "--workspace")) return workspace(argv[2]);
    return 2;
}
