// tg_clean_targets of csrc/targets.h on the host stand-in.  Usage: targets_main IN OUT [inplace]
//   IN:  int32 B, int32 lens[B], float32 x[sum lens]
//   OUT: float32 y[sum lens], float32 quartiles[B][2], int32 n_outliers[B], float64 stats[12]
#include "standin_host.h"
namespace {
#include "targets.h"
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int B = 0;
    if (!f || fread(&B, 4, 1, f) != 1) return 2;
    std::vector<int> lens(B), starts(B);
    if (B && fread(lens.data(), 4, B, f) != (size_t)B) return 2;
    int total = 0;
    for (int b = 0; b < B; ++b) { starts[b] = total; total += lens[b]; }
    std::vector<float> x(total), y(total, -777.f), q(2 * B);
    std::vector<int> n_out(B);
    double stats[12];
    if (total && fread(x.data(), 4, total, f) != (size_t)total) return 2;
    fclose(f);
    std::vector<char> ws(tg_workspace_bytes(B));
    float* yp = argc > 3 ? x.data() : y.data();
    if (int rc = tg_clean_targets(nullptr, x.data(), B, starts.data(), lens.data(), ws.data(), ws.size(), yp, q.data(), n_out.data(), stats)) return rc;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(yp, 4, total, o); fwrite(q.data(), 4, 2 * B, o); fwrite(n_out.data(), 4, B, o); fwrite(stats, 8, 12, o);
    fclose(o);
    return 0;
}
