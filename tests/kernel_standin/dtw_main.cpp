// dt_dtw of csrc/dtw.h on the host stand-in.  Usage: dtw_main IN OUT   |   dtw_main --checks
//   IN:  int64 cap_bytes; int32 B, D, a_stride, b_stride, a_rows, b_rows, tracks; int32 a_starts[B], a_lens[B], b_starts[B], b_lens[B];
//        float32 a [a_rows, a_stride], b [b_rows, b_stride]; with tracks: float32 e_a [a_rows], e_b [b_rows], p_a [a_rows], p_b [b_rows]
//   OUT: float64 terms[B][12], float64 batch[12]
// The workspace is what fs2_op_dtw_workspace_bytes answers for cap_bytes.  --checks: one line "name code" per refused (or accepted)
// argument set.  Every buffer is a heap block of exactly its size, so that a sanitizer build sees a read beyond it.
#include "standin_host.h"
#include "hip_standin_record.h"
namespace {
#include "dtw.h"

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n) {
    v.assign(n, T{});
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int checks() {
    const int B = 2, D = 3;
    std::vector<float> a(7 * D, 1.f), b(6 * D, 2.f), ta(7, 1.f), tb(6, 1.f);
    int32_t as[2] = {0, 4}, al[2] = {4, 3}, bs[2] = {0, 2}, bl[2] = {2, 4};
    std::vector<char> ws(dtw_workspace_bytes(B, al, bl, 0));
    std::vector<double> terms(B * FS2_DTW_TERMS), batch(FS2_DTW_TERMS);
    fs2_op_dtw_args ok{};
    ok.struct_size = sizeof(ok);
    ok.B = B; ok.D = D; ok.a_stride = ok.b_stride = D;
    ok.a = a.data(); ok.b = b.data(); ok.e_a = ok.p_a = ta.data(); ok.e_b = ok.p_b = tb.data();
    ok.workspace = ws.data(); ok.workspace_bytes = ws.size();
    ok.terms = terms.data(); ok.batch = batch.data();
    auto run = [&](const char* name, auto edit) {
        fs2_op_dtw_args x = ok;
        int32_t as2[2] = {as[0], as[1]}, al2[2] = {al[0], al[1]}, bs2[2] = {bs[0], bs[1]}, bl2[2] = {bl[0], bl[1]};
        x.a_starts = as2; x.a_lens = al2; x.b_starts = bs2; x.b_lens = bl2;
        edit(x, as2, al2);
        printf("%s %d\n", name, dt_dtw(nullptr, &x));
    };
    run("ok", [](auto&, int32_t*, int32_t*) {});
    printf("ok_steps %d\n", (int)(terms[2] + terms[FS2_DTW_TERMS + 2]));      // 4 x 2 and 3 x 4 of constant frames: the diagonal first, 4 + 4
    run("struct_size", [](auto& x, int32_t*, int32_t*) { x.struct_size += 8; });
    run("negative_B", [](auto& x, int32_t*, int32_t*) { x.B = -1; });
    run("null_lens", [](auto& x, int32_t*, int32_t*) { x.b_lens = nullptr; });
    run("null_starts", [](auto& x, int32_t*, int32_t*) { x.a_starts = nullptr; });
    run("negative_len", [](auto&, int32_t*, int32_t* l) { l[1] = -1; });
    run("negative_start", [](auto&, int32_t* s, int32_t*) { s[0] = -2; });
    run("D_0", [](auto& x, int32_t*, int32_t*) { x.D = 0; });
    run("D_129", [](auto& x, int32_t*, int32_t*) { x.D = 129; x.a_stride = x.b_stride = 129; });
    run("stride_below_D", [](auto& x, int32_t*, int32_t*) { x.b_stride = 2; });
    run("e_a_without_e_b", [](auto& x, int32_t*, int32_t*) { x.e_b = nullptr; });
    run("p_b_without_p_a", [](auto& x, int32_t*, int32_t*) { x.p_a = nullptr; });
    run("null_a", [](auto& x, int32_t*, int32_t*) { x.a = nullptr; });
    run("null_workspace", [](auto& x, int32_t*, int32_t*) { x.workspace = nullptr; });
    run("workspace_one_byte_short", [](auto& x, int32_t*, int32_t*) { x.workspace_bytes -= 1; });
    run("no_tracks", [](auto& x, int32_t*, int32_t*) { x.e_a = x.e_b = x.p_a = x.p_b = nullptr; });
    run("nothing_asked", [](auto& x, int32_t*, int32_t*) { x.terms = x.batch = nullptr; x.workspace = nullptr; });
    batch.assign(FS2_DTW_TERMS, 7.0);
    run("B0", [](auto& x, int32_t*, int32_t*) { x.B = 0; x.workspace = nullptr; x.workspace_bytes = 0; x.terms = nullptr; });
    double s = 0.0;
    for (double v : batch) s += fabs(v);
    printf("B0_batch_abs_sum %d\n", (int)s);
    int32_t neg[1] = {-1}, one[1] = {1}, big[1] = {INT32_MAX};
    printf("workspace_negative_B %zu\nworkspace_null_lens %zu\nworkspace_negative_len %zu\nworkspace_too_many_cells %zu\nworkspace_B0 %d\n",
           dtw_workspace_bytes(-1, al, bl, 0), dtw_workspace_bytes(1, nullptr, bl, 0), dtw_workspace_bytes(1, neg, one, 0),
           dtw_workspace_bytes(1, big, big, 0), dtw_workspace_bytes(0, nullptr, nullptr, 0) > 0);
    const size_t all = dtw_workspace_bytes(B, al, bl, (size_t)1 << 40), least = dtw_workspace_bytes(B, al, bl, 0);
    printf("workspace_cap_between %d\n", least < all && dtw_workspace_bytes(B, al, bl, least + 1) == least + 1);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--checks")) return checks();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int64_t cap;
    int32_t h[7];
    if (!f || fread(&cap, 8, 1, f) != 1 || fread(h, 4, 7, f) != 7) return 2;
    const int B = h[0], D = h[1];
    const size_t ast = h[2], bst = h[3], arows = h[4], brows = h[5];
    const bool tracks = h[6] != 0;
    std::vector<int32_t> as, al, bs, bl;
    std::vector<float> a, b, e_a, e_b, p_a, p_b;
    if (!read_into(f, as, B) || !read_into(f, al, B) || !read_into(f, bs, B) || !read_into(f, bl, B) || !read_into(f, a, arows * ast) ||
        !read_into(f, b, brows * bst))
        return 2;
    if (tracks && (!read_into(f, e_a, arows) || !read_into(f, e_b, brows) || !read_into(f, p_a, arows) || !read_into(f, p_b, brows))) return 2;
    fclose(f);
    std::vector<char> ws(dtw_workspace_bytes(B, al.data(), bl.data(), (size_t)cap));
    std::vector<double> out((size_t)(B + 1) * FS2_DTW_TERMS, -777.0);
    fs2_op_dtw_args x{};
    x.struct_size = sizeof(x);
    x.B = B; x.D = D; x.a_stride = (int64_t)ast; x.b_stride = (int64_t)bst;
    x.a = a.data(); x.b = b.data();
    if (tracks) { x.e_a = e_a.data(); x.e_b = e_b.data(); x.p_a = p_a.data(); x.p_b = p_b.data(); }
    x.a_starts = as.data(); x.a_lens = al.data(); x.b_starts = bs.data(); x.b_lens = bl.data();
    x.workspace = ws.data(); x.workspace_bytes = ws.size();
    x.terms = out.data(); x.batch = out.data() + (size_t)B * FS2_DTW_TERMS;
    if (int rc = dt_dtw(nullptr, &x)) return rc < 0 ? 100 - rc : rc;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    fclose(o);
    return 0;
}
