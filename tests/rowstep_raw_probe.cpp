// Host-compiled driver of include/fs2.h and csrc/row_step_args.h for tests/test_rowstep_host.py (g++ -std=c++17 -Wall -Werror, no HIP).
//   probe tok | short | flat     sizeof of the block and the offset of every field: what the ctypes mirrors of tests/rowstep_raw.py must equal
//   probe steps                  the FS2_ROW_STEP_* enumerators with their values, then "count N"
#include <cstddef>
#include <cstdio>
#include <string>

#include "fs2.h"
#include "row_step_args.h"

using namespace fs2;

#define FIELD(f) printf(#f " %zu\n", offsetof(ARGS, f));

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "tok") {
#define ARGS TokGatherArgs
        printf("sizeof %zu\n", sizeof(ARGS));
        FIELD(P) FIELD(ldp) FIELD(tok_start) FIELD(lri) FIELD(row_pos) FIELD(row_seq) FIELD(R) FIELD(chans) FIELD(bias) FIELD(ln_g) FIELD(ln_b) FIELD(vp) FIELD(col0) FIELD(D)
        FIELD(es) FIELD(ps) FIELD(es_stride) FIELD(ps_stride) FIELD(e_rows) FIELD(p_rows) FIELD(ebins) FIELD(pbins) FIELD(nb) FIELD(TE) FIELD(TP) FIELD(qe_rows) FIELD(qp_rows)
        FIELD(f2s) FIELD(sqe) FIELD(sqp) FIELD(ln_g2) FIELD(ln_b2) FIELD(pe) FIELD(pe_alpha) FIELD(x_scale) FIELD(x0) FIELD(x0p) FIELD(srow_pos) FIELD(Rs)
#undef ARGS
        return 0;
    }
    if (mode == "short") {
#define ARGS ShortLayoutArgs
        printf("sizeof %zu\n", sizeof(ARGS));
        FIELD(cum) FIELD(scum) FIELD(Tmax) FIELD(ilen) FIELD(so32) FIELD(row_pos) FIELD(row_seq) FIELD(vlen) FIELD(R) FIELD(ovf) FIELD(B) FIELD(gap) FIELD(K) FIELD(Rs) FIELD(Rs_pad)
        FIELD(lri) FIELD(f2s) FIELD(sstart) FIELD(slen) FIELD(sdims) FIELD(srow_pos) FIELD(srow_seq) FIELD(slri)
#undef ARGS
        return 0;
    }
    if (mode == "flat") {
#define ARGS RowStepArgs
        printf("sizeof %zu\n", sizeof(ARGS));
        FIELD(row_pos) FIELD(row_seq) FIELD(R) FIELD(start) FIELD(vlen) FIELD(B) FIELD(Tmax) FIELD(D) FIELD(rows) FIELD(planes) FIELD(xs) FIELD(E) FIELD(idim) FIELD(pe) FIELD(pe_alpha)
        FIELD(x_scale) FIELD(dlog_rows) FIELD(d_log) FIELD(d_int) FIELD(d_int2) FIELD(ds) FIELD(cum) FIELD(olens) FIELD(olens32) FIELD(alpha) FIELD(scum) FIELD(so32) FIELD(K)
        FIELD(src_rows) FIELD(tok_start) FIELD(ilen) FIELD(cum_in) FIELD(index_rows) FIELD(es) FIELD(ps) FIELD(es_stride) FIELD(ps_stride) FIELD(e_rows) FIELD(p_rows) FIELD(ebins)
        FIELD(pbins) FIELD(nb) FIELD(Te) FIELD(Tp) FIELD(qe_rows) FIELD(qp_rows)
#undef ARGS
        return 0;
    }
    if (mode == "steps") {
        printf("%d embed\n%d dur_post\n%d lr_index\n%d lr_index_short\n%d lr_expand\n%d var_gather0\n%d var_embed\n%d dec_in_gather\n%d to_planes\n%d planes_to_rows\n",
               FS2_ROW_STEP_EMBED, FS2_ROW_STEP_DUR_POST, FS2_ROW_STEP_LR_INDEX, FS2_ROW_STEP_LR_INDEX_SHORT, FS2_ROW_STEP_LR_EXPAND, FS2_ROW_STEP_VAR_GATHER0,
               FS2_ROW_STEP_VAR_EMBED, FS2_ROW_STEP_DEC_IN_GATHER, FS2_ROW_STEP_TO_PLANES, FS2_ROW_STEP_PLANES_TO_ROWS);
        printf("count %d\n", FS2_ROW_STEP_COUNT);
        return 0;
    }
    fprintf(stderr, "usage: probe tok | short | flat | steps\n");
    return 2;
}
