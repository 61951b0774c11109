// Host-compiled driver of csrc/gemm_args.h and csrc/gemm_plan.h for tests/test_gemm_raw_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe layout          sizeof(GemmArgs) and the offset of every field: what the ctypes mirror of tests/gemm_raw.py must equal
//   probe kernels         the enumerators of GemmKernel with their values: what fs2_op_launch_gemm reports as plan_out[0]
//   probe plans <file>    one line per launch, "<id> <precision> <option=value,...|-> <hex bytes of the argument block>": the plan of that block under those
//                         switches, as "<id> <kernel> nsplit nb bm mt apart epi arith res ksplit rows_pass build_planes err"
// plan_gemm reads integers and the null-ness of pointers only, so the bytes of a block whose pointers are placeholders plan exactly as the block
// with device pointers does: a launch that would be refused, or would land on another kernel, shows here and not on a GPU.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "gemm_plan.h"

using namespace fs2;

namespace {

const char* kernel_name(GemmKernel k) {
    switch (k) {
    case GemmKernel::None: return "none";
    case GemmKernel::RowsF32: return "rows_f32";
    case GemmKernel::TileF32: return "tile_f32";
    case GemmKernel::TileRowsF32: return "tile_rows_f32";
    case GemmKernel::PlBf16: return "pl_bf16";
    case GemmKernel::PlF16: return "pl_f16";
    case GemmKernel::PlMx: return "pl_mx";
    case GemmKernel::PlMx4: return "pl_mx4";
    case GemmKernel::Row8: return "row8";
    case GemmKernel::Row8c: return "row8c";
    case GemmKernel::Row8cGrouped: return "row8c_grouped";
    case GemmKernel::Row8cTwoLn: return "row8c_two_ln";
    case GemmKernel::Row4: return "row4";
    case GemmKernel::Qkv8: return "qkv8";
    case GemmKernel::Qkv4: return "qkv4";
    }
    return "?";
}

#define FIELD(f) printf(#f " %zu\n", offsetof(GemmArgs, f));
int layout() {
    printf("sizeof %zu\n", sizeof(GemmArgs));
    FIELD(X) FIELD(ldx) FIELD(C) FIELD(W) FIELD(Cpad) FIELD(ktaps) FIELD(N) FIELD(R) FIELD(row_pos) FIELD(bias) FIELD(resid) FIELD(ldr) FIELD(relu_pre)
    FIELD(ln_g) FIELD(ln_b) FIELD(ln_eps) FIELD(act_post) FIELD(pe) FIELD(pe_ld) FIELD(pe_alpha) FIELD(x_scale) FIELD(dot_w) FIELD(dot_b) FIELD(dot_out)
    FIELD(Y) FIELD(ldy) FIELD(Ysrc) FIELD(ldsrc) FIELD(Wb) FIELD(qk_hi) FIELD(qk_lo) FIELD(vt_hi) FIELD(vt_lo) FIELD(att_D) FIELD(Rvt) FIELD(q_scale)
    FIELD(scratch) FIELD(Xp) FIELD(xp_scratch) FIELD(Yp) FIELD(yp_chunks) FIELD(yp_f16) FIELD(f16_terms) FIELD(yp_scale) FIELD(mx) FIELD(mx_scale)
    FIELD(mx_scale_b) FIELD(ksplit) FIELD(kpart) FIELD(kpart_stride) FIELD(kpart_cap) FIELD(regime_rows) FIELD(xp_row_chunks) FIELD(k_groups)
    FIELD(ln_groups) FIELD(dot_gstride) FIELD(yp_col_off) FIELD(Rp) FIELD(residp) FIELD(residp_chunks) FIELD(residp_mx) FIELD(residp_scale)
    FIELD(yp_rowscale) FIELD(x_rowscale) FIELD(w_rowscale)
    return 0;
}

int kernels() {
    for (int k = 0; k <= (int)GemmKernel::Qkv4; ++k) printf("%d %s\n", k, kernel_name((GemmKernel)k));
    return 0;
}

bool set_option(Options& o, const std::string& name, int v) {
    if (name == "FS2_BM") o.bm = v;
    else if (name == "FS2_ROW8") o.row8 = v;
    else if (name == "FS2_QKV8") o.qkv8 = v;
    else if (name == "FS2_MT8") o.mt8 = v;
    else if (name == "FS2_QKV_SPLIT") o.qkv_split = v;
    else if (name == "FS2_ROW4") o.row4 = v;
    else if (name == "FS2_MT4") o.mt4 = v;
    else if (name == "FS2_QKV4") o.qkv4 = v;
    else return false;
    return true;
}

int plans(const char* path) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string id, optstr, hex;
        int precision = 0;
        if (!(ls >> id >> precision >> optstr >> hex)) continue;
        Options o;
        if (optstr != "-") {
            std::istringstream os(optstr);
            std::string item;
            while (std::getline(os, item, ',')) {
                const size_t eq = item.find('=');
                if (eq == std::string::npos || !set_option(o, item.substr(0, eq), atoi(item.c_str() + eq + 1))) { fprintf(stderr, "%s: unknown switch %s\n", id.c_str(), item.c_str()); return 2; }
            }
        }
        if (hex.size() != 2 * sizeof(GemmArgs)) { fprintf(stderr, "%s: a block of %zu bytes, GemmArgs has %zu\n", id.c_str(), hex.size() / 2, sizeof(GemmArgs)); return 2; }
        unsigned char bytes[sizeof(GemmArgs)];
        for (size_t i = 0; i < sizeof(GemmArgs); ++i) bytes[i] = (unsigned char)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        GemmArgs a;
        memcpy(&a, bytes, sizeof a);
        const GemmPlan p = plan_gemm(a, precision, o);
        printf("%s %s %d %d %d %d %d %d %d %d %d %d %d %d\n", id.c_str(), kernel_name(p.kernel), p.nsplit, p.nb, p.bm, p.mt, p.apart, p.epi, p.arith, p.res, p.ksplit, (int)p.rows_pass,
               (int)p.build_planes, p.err);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layout") return layout();
    if (mode == "kernels") return kernels();
    if (mode == "plans" && argc > 2) return plans(argv[2]);
    fprintf(stderr, "usage: probe layout | kernels | plans <file>\n");
    return 2;
}
