// Host-compiled driver of csrc/layout_rule.h for tests/test_layout_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe layout GAP COMPAT MASKED N ...     the layout of utterances of N valid positions, put together from the rule's pieces alone
//                                            (utt_lens, the row walk, dealt_before, Dealer::place): "start ..", "len ..", "klen ..",
//                                            "vlen ..", "rows R Rpad", "depth D", "work b:q .."
//   probe meta B RPAD NWORK RF               "host ..", "dev ..", "meta2 .." (the offsets in declaration order, then end), "ints DEV META2"
//   probe caps FRAMES UTTS ROWCAP B LMAX     "row_bound N", "work_capacity N"
//   probe flags ROWS DEPTH LONGEST SMALLEST ROWCAP WORKCAP LMAXCAP PEROWS     "flags F"
//   probe consts                             "consts kGap kMinGap kTailRows kAttAlign kAttBlk kXcds"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "layout_rule.h"

using namespace fs2;

namespace {

void line(const char* name, const std::vector<int>& v) {
    printf("%s", name);
    for (int x : v) printf(" %d", x);
    printf("\n");
}

int layout(int argc, char** argv) {
    const int gap = atoi(argv[2]), compat = atoi(argv[3]), masked = atoi(argv[4]), B = argc - 5;
    std::vector<int> valid(B), start(B), len(B), klen(B), vlen(B), order(B), first(B);
    int mx = 0;
    for (int b = 0; b < B; ++b) mx = std::max(mx, valid[b] = atoi(argv[5 + b]));
    int row = gap;
    for (int b = 0; b < B; ++b) {
        const UttLens u = utt_lens(valid[b], mx, compat, masked);
        len[b] = u.len; klen[b] = u.klen; vlen[b] = u.vlen;
        start[b] = row = row_start(row);
        row = row_after(row, u.len, gap);
        order[b] = b;
    }
    std::sort(order.begin(), order.end(), [&](int x, int y) { return dealt_before(klen[x], x, klen[y], y); });
    Dealer deal;
    for (int b : order) first[b] = deal.place(att_blocks(len[b]));
    std::vector<int> wb(deal.items(), -1), wq(deal.items(), 0);
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < att_blocks(len[b]); ++q) { wb[first[b] + kXcds * q] = b; wq[first[b] + kXcds * q] = q; }
    line("start", start); line("len", len); line("klen", klen); line("vlen", vlen);
    printf("rows %d %d\ndepth %d\nwork", rows_used(row), rows_padded(rows_used(row)), deal.depth);
    for (size_t i = 0; i < wb.size(); ++i) printf(" %d:%d", wb[i], wq[i]);
    printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 5 && !strcmp(argv[1], "layout")) return layout(argc, argv);
    if (argc == 6 && !strcmp(argv[1], "meta")) {
        const long long B = atoll(argv[2]), Rpad = atoll(argv[3]), nwork = atoll(argv[4]), rf = atoll(argv[5]);
        const MetaHost h = MetaHost::at(B, Rpad, nwork);
        const MetaDev d = MetaDev::at(B, Rpad, nwork);
        const Meta2 m = Meta2::at(B, Rpad * rf);
        printf("host %lld %lld %lld %lld %lld %lld %lld %lld\n", h.start, h.len, h.klen, h.vlen, h.work, h.row_pos, h.row_seq, h.end);
        printf("dev %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", d.start, d.len, d.klen, d.vlen, d.rank, d.woff, d.pcum, d.dims, d.work, d.row_pos,
               d.row_seq, d.end);
        printf("meta2 %lld %lld %lld %lld %lld %lld %lld\n", m.start, m.len, m.vlen, m.dims, m.row_pos, m.row_seq, m.end);
        printf("ints %lld %lld\n", MetaDev::ints(B, Rpad, nwork), Meta2::ints(B, Rpad * rf));
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "caps")) {
        printf("row_bound %d\nwork_capacity %d\n", row_bound(atoll(argv[2]), atoll(argv[3])), work_capacity(atoll(argv[4]), atoi(argv[5]), atoi(argv[6])));
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "flags")) {
        int v[8];
        for (int i = 0; i < 8; ++i) v[i] = atoi(argv[2 + i]);
        printf("flags %d\n", overflow_flags(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "consts")) {
        printf("consts %d %d %d %d %d %d\n", kGap, kMinGap, kTailRows, kAttAlign, kAttBlk, kXcds);
        return 0;
    }
    return 2;
}
