// lt_loss_terms of csrc/losses.h on the host stand-in.  Usage: losses_main IN OUT [misalign]   |   losses_main --checks
//   IN:  int32 B, odim, Tmax, Lmax, pads, pred_stride_f, y_stride_f, pred_stride_t, ds_stride_t, tgt_stride_f; int32 ilens[B], olens[B];
//        float32 before, after [B, pred_stride_f, odim], ys [B, y_stride_f, odim], d_outs [B, pred_stride_t]; int64 ds [B, ds_stride_t];
//        float32 e_outs [B, pred_stride_f], es [B, tgt_stride_f], p_outs [B, pred_stride_f], ps [B, tgt_stride_f]
//   OUT: float64 terms[B][20], float64 batch[20]
// misalign: before / after / ys start 4 bytes off a 16-byte boundary (the 4-byte load path).  --checks: one line "name code" per
// refused (or accepted) argument set.  Every buffer is a heap block of exactly its size, so that a sanitizer build sees a read beyond it.
#include "standin_host.h"
namespace {
#include "targets.h"
#include "losses.h"

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n, size_t lead = 0) {
    v.assign(n + lead, T{});
    return n == 0 || fread(v.data() + lead, sizeof(T), n, f) == n;
}

int checks() {
    const int B = 2, odim = 4, T = 3, L = 5;
    std::vector<float> mel(B * L * odim, 1.f), fr(B * L, 1.f), tok(B * T, 1.f);
    std::vector<int64_t> ds(B * T, 1);
    int32_t il[2] = {3, 2}, ol[2] = {5, 1};
    std::vector<char> ws(lt_workspace_bytes(B, ol));
    std::vector<double> terms(B * FS2_LOSS_TERMS), batch(FS2_LOSS_TERMS);
    fs2_op_loss_args ok{};
    ok.struct_size = sizeof(ok);
    ok.B = B; ok.odim = odim; ok.Tmax = T; ok.Lmax = L; ok.pads = 1;
    ok.pred_stride_f = ok.y_stride_f = ok.tgt_stride_f = L; ok.pred_stride_t = ok.ds_stride_t = T;
    ok.before = ok.after = ok.ys = mel.data(); ok.d_outs = tok.data(); ok.ds = ds.data();
    ok.e_outs = ok.es = ok.p_outs = ok.ps = fr.data();
    ok.ilens = il; ok.olens = ol; ok.workspace = ws.data(); ok.workspace_bytes = ws.size();
    ok.terms = terms.data(); ok.batch = batch.data();
    auto run = [&](const char* name, auto edit) {
        fs2_op_loss_args a = ok;
        int32_t il2[2] = {il[0], il[1]}, ol2[2] = {ol[0], ol[1]};
        a.ilens = il2; a.olens = ol2;
        edit(a, il2, ol2);
        printf("%s %d\n", name, lt_loss_terms(nullptr, &a));
    };
    run("ok", [](auto&, int32_t*, int32_t*) {});
    run("struct_size", [](auto& a, int32_t*, int32_t*) { a.struct_size += 8; });
    run("negative_B", [](auto& a, int32_t*, int32_t*) { a.B = -1; });
    run("null_lens", [](auto& a, int32_t*, int32_t*) { a.olens = nullptr; });
    run("negative_ilen", [](auto&, int32_t* i, int32_t*) { i[1] = -1; });
    run("negative_olen", [](auto&, int32_t*, int32_t* o) { o[0] = -2; });
    run("olen_above_Lmax", [](auto& a, int32_t*, int32_t*) { a.Lmax = 4; });
    run("ilen_above_Tmax", [](auto& a, int32_t*, int32_t*) { a.Tmax = 2; });
    run("Lmax_above_pred_stride", [](auto& a, int32_t*, int32_t*) { a.pred_stride_f = 4; });
    run("Lmax_above_y_stride", [](auto& a, int32_t*, int32_t*) { a.y_stride_f = 4; });
    run("Lmax_above_tgt_stride", [](auto& a, int32_t*, int32_t*) { a.tgt_stride_f = 4; });
    run("Tmax_above_pred_stride", [](auto& a, int32_t*, int32_t*) { a.pred_stride_t = 2; });
    run("Tmax_above_ds_stride", [](auto& a, int32_t*, int32_t*) { a.ds_stride_t = 2; });
    run("before_without_ys", [](auto& a, int32_t*, int32_t*) { a.ys = nullptr; });
    run("d_outs_without_ds", [](auto& a, int32_t*, int32_t*) { a.ds = nullptr; });
    run("es_without_e_outs", [](auto& a, int32_t*, int32_t*) { a.e_outs = nullptr; });
    run("p_outs_without_ps", [](auto& a, int32_t*, int32_t*) { a.ps = nullptr; });
    run("null_workspace", [](auto& a, int32_t*, int32_t*) { a.workspace = nullptr; });
    run("workspace_one_byte_short", [](auto& a, int32_t*, int32_t*) { a.workspace_bytes -= 1; });
    run("all_groups_null", [](auto& a, int32_t*, int32_t*) {
        a.before = a.after = a.ys = a.d_outs = a.e_outs = a.es = a.p_outs = a.ps = nullptr; a.ds = nullptr;
        a.pred_stride_f = a.y_stride_f = a.tgt_stride_f = a.pred_stride_t = a.ds_stride_t = 0;
    });
    run("nothing_asked", [](auto& a, int32_t*, int32_t*) { a.terms = a.batch = nullptr; a.workspace = nullptr; });
    batch.assign(FS2_LOSS_TERMS, 7.0);
    run("B0", [](auto& a, int32_t*, int32_t*) { a.B = 0; a.workspace = nullptr; a.workspace_bytes = 0; a.terms = nullptr; });
    double s = 0.0;
    for (double v : batch) s += fabs(v);
    printf("B0_batch_abs_sum %d\n", (int)s);
    int32_t neg[1] = {-1};
    printf("workspace_negative_B %zu\nworkspace_null_olens %zu\nworkspace_negative_olen %zu\nworkspace_B0 %d\n", lt_workspace_bytes(-1, ol),
           lt_workspace_bytes(1, nullptr), lt_workspace_bytes(1, neg), lt_workspace_bytes(0, nullptr) > 0);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--checks")) return checks();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[10];
    if (!f || fread(h, 4, 10, f) != 10) return 2;
    const int B = h[0], odim = h[1];
    const size_t lead = argc > 3 ? 1 : 0, psf = h[5], ysf = h[6], pst = h[7], dst = h[8], tsf = h[9];
    std::vector<int32_t> il, ol;
    std::vector<float> before, after, ys, d_outs, e_outs, es, p_outs, ps;
    std::vector<int64_t> ds;
    if (!read_into(f, il, B) || !read_into(f, ol, B) || !read_into(f, before, B * psf * odim, lead) || !read_into(f, after, B * psf * odim, lead) ||
        !read_into(f, ys, B * ysf * odim, lead) || !read_into(f, d_outs, B * pst) || !read_into(f, ds, B * dst) || !read_into(f, e_outs, B * psf) ||
        !read_into(f, es, B * tsf) || !read_into(f, p_outs, B * psf) || !read_into(f, ps, B * tsf))
        return 2;
    fclose(f);
    std::vector<char> ws(lt_workspace_bytes(B, ol.data()));
    std::vector<double> out((size_t)(B + 1) * FS2_LOSS_TERMS, -777.0);
    fs2_op_loss_args a{};
    a.struct_size = sizeof(a);
    a.B = B; a.odim = odim; a.Tmax = h[2]; a.Lmax = h[3]; a.pads = h[4];
    a.pred_stride_f = h[5]; a.y_stride_f = h[6]; a.pred_stride_t = h[7]; a.ds_stride_t = h[8]; a.tgt_stride_f = h[9];
    a.before = before.data() + lead; a.after = after.data() + lead; a.ys = ys.data() + lead;
    a.d_outs = d_outs.data(); a.ds = ds.data(); a.e_outs = e_outs.data(); a.es = es.data(); a.p_outs = p_outs.data(); a.ps = ps.data();
    a.ilens = il.data(); a.olens = ol.data(); a.workspace = ws.data(); a.workspace_bytes = ws.size();
    a.terms = out.data(); a.batch = out.data() + (size_t)B * FS2_LOSS_TERMS;
    if (int rc = lt_loss_terms(nullptr, &a)) return rc < 0 ? 100 - rc : rc;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    fclose(o);
    return 0;
}
