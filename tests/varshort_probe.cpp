// Host-compiled driver of csrc/layout_rule.h for tests/test_varshort_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe window LAYERS KERNEL                  "window K"
//   probe map K D ...                           per duration D: "d D short S offsets o0 o1 .." (the short offset of every frame offset 0 .. D-1)
//   probe bound FRAMES PHONEMES UTTS K          "bound N"
//   probe layout GAP K D .. / D ..              utterances of phonemes of D frames, '/' between utterances; put together from the rule's pieces and
//                                               layout_rule.h's row walk: "start ..", "len ..", "rows R", and per utterance "f2s r0 r1 .." (the short
//                                               row of every frame)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "layout_rule.h"

using namespace fs2;

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "window")) {
        printf("window %d\n", vs_window(atoi(argv[2]), atoi(argv[3])));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "map")) {
        const int K = atoi(argv[2]);
        for (int i = 3; i < argc; ++i) {
            const int d = atoi(argv[i]);
            printf("d %d short %d offsets", d, vs_short_dur(d, K));
            for (int o = 0; o < d; ++o) printf(" %d", vs_short_offset(o, d, K));
            printf("\n");
        }
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "bound")) {
        printf("bound %d\n", vs_row_bound(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoi(argv[5])));
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "layout")) {
        const int gap = atoi(argv[2]), K = atoi(argv[3]);
        std::vector<std::vector<int>> utts(1);
        for (int i = 4; i < argc; ++i) {
            if (!strcmp(argv[i], "/")) utts.emplace_back();
            else utts.back().push_back(atoi(argv[i]));
        }
        std::vector<int> start, len;
        int row = gap;
        for (const auto& u : utts) {
            int s = 0;
            for (int d : u) s += vs_short_dur(d, K);
            row = row_start(row);
            start.push_back(row); len.push_back(s);
            row = row_after(row, s, gap);
        }
        printf("start");
        for (int x : start) printf(" %d", x);
        printf("\nlen");
        for (int x : len) printf(" %d", x);
        printf("\nrows %d\n", rows_used(row));
        for (size_t b = 0; b < utts.size(); ++b) {
            printf("f2s");
            int s0 = 0;
            for (int d : utts[b]) {
                for (int o = 0; o < d; ++o) printf(" %d", start[b] + s0 + vs_short_offset(o, d, K));
                s0 += vs_short_dur(d, K);
            }
            printf("\n");
        }
        return 0;
    }
    return 2;
}
