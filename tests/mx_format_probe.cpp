// Host-compiled driver of the mx4 scale rule of csrc/common.h for tests/test_gemm_raw_host.py (hipcc, host side only: the two functions are __host__ __device__).
//   probe <hex bits of an fp32> ...    one line per argument: "<bits> <mx4_scale_byte(m)> <hex bits of mx4_inv_scale(that byte)>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const unsigned u = (unsigned)strtoul(argv[i], nullptr, 16);
        float m;
        memcpy(&m, &u, 4);
        const int eb = fs2::mx4_scale_byte(m);
        const float inv = fs2::mx4_inv_scale(eb);
        unsigned v;
        memcpy(&v, &inv, 4);
        printf("%08x %d %08x\n", u, eb, v);
    }
    return 0;
}
