// Host-compiled driver of include/fs2.h and csrc/attn_plan.h for tests/test_attn_raw_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe layout          sizeof(fs2_op_attn_args) and the offset of every field: what the ctypes mirror of fastspeech2_amd/_lib.py must equal; then "plan_fields N"
//   probe kernels         the enumerators of AttnKernel with their values: what fs2_op_launch_attention reports as plan_out[0]
#include <cstddef>
#include <cstdio>
#include <string>

#include "attn_plan.h"
#include "fs2.h"

using namespace fs2;

#define FIELD(f) printf(#f " %zu\n", offsetof(fs2_op_attn_args, f));

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layout") {
        printf("sizeof %zu\n", sizeof(fs2_op_attn_args));
        FIELD(struct_size) FIELD(nitems) FIELD(D) FIELD(heads) FIELD(dk_true) FIELD(R) FIELD(Rvt) FIELD(regime_rows) FIELD(mask_q) FIELD(precision)
        FIELD(qkv) FIELD(qk_hi) FIELD(qk_lo) FIELD(vt_hi) FIELD(vt_lo) FIELD(ctx) FIELD(ctxp) FIELD(start) FIELD(len) FIELD(klen) FIELD(work) FIELD(dims)
        FIELD(slow_count)
        printf("plan_fields %d\n", FS2_ATTN_PLAN_FIELDS);
        return 0;
    }
    if (mode == "kernels") {
        printf("%d none\n%d f32\n%d b16\n%d w32\n", (int)AttnKernel::None, (int)AttnKernel::F32, (int)AttnKernel::B16, (int)AttnKernel::W32);
        return 0;
    }
    fprintf(stderr, "usage: probe layout | kernels\n");
    return 2;
}
