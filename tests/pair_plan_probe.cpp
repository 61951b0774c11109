// Host-compiled driver of csrc/pair_plan.h for tests/test_pair_plan_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe OP bytes CAP [nulllens] N:M ...        fs2_op_*_workspace_bytes for the pairs: "bytes <n>"
//   probe OP plan WS [labels] [nulllens] N:M ... the operator's checks and plan for a workspace of WS bytes (WS = "cap:<CAP>": what the query
//                                                answers for CAP): "rc <code>", and when 0 "layout ...", a "rec ..." per pair, a "group ..." per
//                                                group, a "chunk ..." per upload chunk
// OP: dtw | align.  The sides are packed: pair i starts where pair i - 1 ended.  labels (align): n_labels[i] = N.  nulllens: a_lens = NULL.
// A refusal prints "fail <code> <message>".  Nothing is allocated for the matrices: the workspace is an address nobody follows.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fs2.h"

namespace {

int fail(void*, int code, const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    printf("fail %d %s\n", code, msg);
    return code;
}
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
#include "pair_plan.h"

struct Input {
    std::vector<int32_t> as, al, bs, bl;
    bool labels = false, nulllens = false;
};

template <class Args> Args args_of(const Input& in, size_t ws_bytes) {
    static float mark;      // a non-null address nobody follows
    Args x{};
    x.struct_size = sizeof(x);
    x.B = (int32_t)in.al.size(); x.D = 3; x.a_stride = x.b_stride = 3;
    x.a = x.b = &mark;
    x.a_starts = in.as.data(); x.a_lens = in.nulllens ? nullptr : in.al.data(); x.b_starts = in.bs.data(); x.b_lens = in.bl.data();
    x.workspace = &mark; x.workspace_bytes = ws_bytes;
    return x;
}

template <class Args> int plan(const PairOp& op, const Input& in, size_t ws_bytes) {
    const Args x = args_of<Args>(in, ws_bytes);
    PairPlan p;
    int rc = pair_check_args(op, &x);
    if (!rc) rc = pair_plan(op, &x, in.labels ? in.al.data() : nullptr, p);
    printf("rc %d\n", rc);
    if (rc) return 0;
    printf("layout %zu %zu %zu %zu %zu\n", p.at.off_recs, p.at.off_terms, p.at.off_group, p.at.all, p.at.largest);
    pair_walk(p, [](int i, const DtwPair& r) { printf("rec %d %d %d %d %d %d %d %lld %lld\n", i, r.a0, r.n, r.b0, r.m, r.tile0, r.tcols, (long long)r.d_off, (long long)r.aux); },
              [](const PairGroup& g) { printf("group %d %d %lld\n", g.first, g.count, (long long)g.tiles); });
    pair_chunks(p, [](const DtwPairChunk& c) {
        printf("chunk %d %d", c.base, c.n);
        for (int k = 0; k < c.n; ++k) printf(" %d:%d", c.r[k].a0, c.r[k].b0);
        printf("\n");
    });
    int groups = 0;
    pair_groups(p, [&](const PairGroup&) { ++groups; });
    printf("groups %d\n", groups);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const bool align = !strcmp(argv[1], "align");
    if (!align && strcmp(argv[1], "dtw")) return 2;
    const PairOp& op = align ? kAlignOp : kDtwOp;
    Input in;
    int32_t a0 = 0, b0 = 0;
    for (int i = 4; i < argc; ++i) {
        long long n, m;
        if (!strcmp(argv[i], "labels")) in.labels = true;
        else if (!strcmp(argv[i], "nulllens")) in.nulllens = true;
        else if (sscanf(argv[i], "%lld:%lld", &n, &m) == 2) {
            in.as.push_back(a0); in.al.push_back((int32_t)n); in.bs.push_back(b0); in.bl.push_back((int32_t)m);
            a0 += (int32_t)std::max(n, 0LL); b0 += (int32_t)std::max(m, 0LL);
        } else return 2;
    }
    const int32_t B = (int32_t)in.al.size();
    const int32_t* al = in.nulllens ? nullptr : in.al.data();
    if (!strcmp(argv[2], "bytes")) {
        printf("bytes %zu\n", pair_workspace_bytes(op, B, al, in.bl.data(), (size_t)strtoull(argv[3], nullptr, 10)));
        return 0;
    }
    if (strcmp(argv[2], "plan")) return 2;
    const size_t ws = !strncmp(argv[3], "cap:", 4) ? pair_workspace_bytes(op, B, al, in.bl.data(), (size_t)strtoull(argv[3] + 4, nullptr, 10))
                                                   : (size_t)strtoull(argv[3], nullptr, 10);
    return align ? plan<fs2_op_align_args>(op, in, ws) : plan<fs2_op_dtw_args>(op, in, ws);
}
