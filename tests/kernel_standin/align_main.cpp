// al_align of csrc/align.h on the host stand-in.  Usage: align_main IN OUT   |   align_main --checks
//   IN:  int64 cap_bytes; int32 B, D, a_stride, b_stride, a_rows, b_rows, max_step, with_labels, dur_stride;
//        int32 a_starts[B], a_lens[B], b_starts[B], b_lens[B], n_labels[B]; float32 a [a_rows, a_stride], b [b_rows, b_stride];
//        with labels: int32 labels [a_rows]
//   OUT: float64 terms[B][8], float64 batch[8], int64 durations[B][dur_stride], int32 state[b_rows]
// The workspace is what fs2_op_align_workspace_bytes answers for cap_bytes.  --checks: one line "name code" per refused (or accepted)
// argument set.  Every buffer is a heap block of exactly its size, so that a sanitizer build sees an access beyond it.
#include "standin_host.h"
#include "hip_standin_record.h"      // (for dtw_sweep, which is compiled with dtw.h; only dtw_dist runs here)
namespace {
#include "dtw.h"
#include "align.h"

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n) {
    v.assign(n, T{});
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int checks() {
    const int B = 2, D = 3, stride = 5;
    std::vector<float> a(7 * D, 1.f), b(6 * D, 2.f);
    std::vector<int32_t> lab{0, 0, 1, 1, 0, 2, 2};
    int32_t as[2] = {0, 4}, al[2] = {4, 3}, bs[2] = {0, 2}, bl[2] = {2, 4}, nl[2] = {2, 3};
    std::vector<char> ws(align_workspace_bytes(B, al, bl, 0));
    std::vector<double> terms(B * FS2_ALIGN_TERMS), batch(FS2_ALIGN_TERMS);
    std::vector<int64_t> dur(B * stride);
    std::vector<int32_t> state(6);
    fs2_op_align_args ok{};
    ok.struct_size = sizeof(ok);
    ok.B = B; ok.D = D; ok.max_step = 2; ok.a_stride = ok.b_stride = D; ok.dur_stride = stride;
    ok.a = a.data(); ok.b = b.data(); ok.labels = lab.data();
    ok.workspace = ws.data(); ok.workspace_bytes = ws.size();
    ok.durations = dur.data(); ok.state = state.data(); ok.terms = terms.data(); ok.batch = batch.data();
    auto run = [&](const char* name, auto edit) {
        fs2_op_align_args x = ok;
        int32_t as2[2] = {as[0], as[1]}, al2[2] = {al[0], al[1]}, bs2[2] = {bs[0], bs[1]}, bl2[2] = {bl[0], bl[1]}, nl2[2] = {nl[0], nl[1]};
        x.a_starts = as2; x.a_lens = al2; x.b_starts = bs2; x.b_lens = bl2; x.n_labels = nl2;
        edit(x, as2, al2, nl2);
        printf("%s %d\n", name, al_align(nullptr, &x));
    };
    run("ok", [](auto&, int32_t*, int32_t*, int32_t*) {});
    // 4 states x 2 frames: no alignment at max_step = 2; 3 x 4 of constant values: a tie keeps k = 0, so the walk back stays in state 2
    // (label 2) down to frame 1, whose only finite predecessor is (0, 0)
    printf("ok_flags %d%d\nok_durations %d%d%d%d%d_%d%d%d%d%d\nok_state %d%d_%d%d%d%d\n", (int)terms[2], (int)terms[FS2_ALIGN_TERMS + 2],
           (int)dur[0], (int)dur[1], (int)dur[2], (int)dur[3], (int)dur[4], (int)dur[5], (int)dur[6], (int)dur[7], (int)dur[8], (int)dur[9],
           state[0], state[1], state[2], state[3], state[4], state[5]);
    run("struct_size", [](auto& x, int32_t*, int32_t*, int32_t*) { x.struct_size += 8; });
    run("negative_B", [](auto& x, int32_t*, int32_t*, int32_t*) { x.B = -1; });
    run("null_lens", [](auto& x, int32_t*, int32_t*, int32_t*) { x.b_lens = nullptr; });
    run("null_starts", [](auto& x, int32_t*, int32_t*, int32_t*) { x.a_starts = nullptr; });
    run("negative_len", [](auto&, int32_t*, int32_t* l, int32_t*) { l[1] = -1; });
    run("negative_start", [](auto&, int32_t* s, int32_t*, int32_t*) { s[0] = -2; });
    run("D_0", [](auto& x, int32_t*, int32_t*, int32_t*) { x.D = 0; });
    run("D_129", [](auto& x, int32_t*, int32_t*, int32_t*) { x.D = 129; x.a_stride = x.b_stride = 129; });
    run("max_step_0", [](auto& x, int32_t*, int32_t*, int32_t*) { x.max_step = 0; });
    run("max_step_3", [](auto& x, int32_t*, int32_t*, int32_t*) { x.max_step = 3; });
    run("stride_below_D", [](auto& x, int32_t*, int32_t*, int32_t*) { x.b_stride = 2; });
    run("n_labels_negative", [](auto&, int32_t*, int32_t*, int32_t* n) { n[0] = -1; });
    run("n_labels_above_dur_stride", [](auto&, int32_t*, int32_t*, int32_t* n) { n[1] = 6; });
    run("n_labels_at_dur_stride", [](auto&, int32_t*, int32_t*, int32_t* n) { n[1] = 5; });
    run("labels_without_n_labels", [](auto& x, int32_t*, int32_t*, int32_t*) { x.n_labels = nullptr; });
    run("n_labels_without_labels", [](auto& x, int32_t*, int32_t*, int32_t*) { x.labels = nullptr; });
    run("no_labels", [](auto& x, int32_t*, int32_t*, int32_t*) { x.labels = nullptr; x.n_labels = nullptr; });
    run("no_labels_dur_stride_below_N", [](auto& x, int32_t*, int32_t*, int32_t*) { x.labels = nullptr; x.n_labels = nullptr; x.dur_stride = 3; });
    run("null_a", [](auto& x, int32_t*, int32_t*, int32_t*) { x.a = nullptr; });
    run("null_workspace", [](auto& x, int32_t*, int32_t*, int32_t*) { x.workspace = nullptr; });
    run("workspace_one_byte_short", [](auto& x, int32_t*, int32_t*, int32_t*) { x.workspace_bytes -= 1; });
    run("no_outputs", [](auto& x, int32_t*, int32_t*, int32_t*) { x.durations = nullptr; x.state = nullptr; x.terms = nullptr; x.batch = nullptr; });
    // labels that break the contract: outside [0, n_labels) and decreasing -- nothing beyond the pair's own row may be written
    dur.assign(dur.size(), -7);
    lab = {5, -3, 1, 1, 2, 1, 9};
    ok.labels = lab.data();
    run("bad_labels", [](auto& x, int32_t*, int32_t*, int32_t*) { x.max_step = 1; });
    int in_row = 1;
    for (int64_t v : dur) in_row &= v >= 0 && v <= 4;
    printf("bad_labels_rows_written_whole %d\n", in_row);
    batch.assign(FS2_ALIGN_TERMS, 7.0);
    run("B0", [](auto& x, int32_t*, int32_t*, int32_t*) { x.B = 0; x.workspace = nullptr; x.workspace_bytes = 0; x.terms = nullptr; });
    double s = 0.0;
    for (double v : batch) s += fabs(v);
    printf("B0_batch_abs_sum %d\n", (int)s);
    int32_t neg[1] = {-1}, one[1] = {1}, big[1] = {INT32_MAX};
    printf("workspace_negative_B %zu\nworkspace_null_lens %zu\nworkspace_negative_len %zu\nworkspace_too_many_cells %zu\nworkspace_B0 %d\n",
           align_workspace_bytes(-1, al, bl, 0), align_workspace_bytes(1, nullptr, bl, 0), align_workspace_bytes(1, neg, one, 0),
           align_workspace_bytes(1, big, big, 0), align_workspace_bytes(0, nullptr, nullptr, 0) > 0);
    const size_t all = align_workspace_bytes(B, al, bl, (size_t)1 << 40), least = align_workspace_bytes(B, al, bl, 0);
    printf("workspace_cap_between %d\n", least < all && align_workspace_bytes(B, al, bl, least + 1) == least + 1);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--checks")) return checks();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int64_t cap;
    int32_t h[9];
    if (!f || fread(&cap, 8, 1, f) != 1 || fread(h, 4, 9, f) != 9) return 2;
    const int B = h[0], D = h[1];
    const size_t ast = h[2], bst = h[3], arows = h[4], brows = h[5], dst = h[8];
    const bool with_labels = h[7] != 0;
    std::vector<int32_t> as, al, bs, bl, nl, lab;
    std::vector<float> a, b;
    if (!read_into(f, as, B) || !read_into(f, al, B) || !read_into(f, bs, B) || !read_into(f, bl, B) || !read_into(f, nl, B) ||
        !read_into(f, a, arows * ast) || !read_into(f, b, brows * bst))
        return 2;
    if (with_labels && !read_into(f, lab, arows)) return 2;
    fclose(f);
    std::vector<char> ws(align_workspace_bytes(B, al.data(), bl.data(), (size_t)cap));
    std::vector<double> out((size_t)(B + 1) * FS2_ALIGN_TERMS, -777.0);
    std::vector<int64_t> dur((size_t)B * dst, -777);
    std::vector<int32_t> state(brows, -777);
    fs2_op_align_args x{};
    x.struct_size = sizeof(x);
    x.B = B; x.D = D; x.max_step = h[6]; x.a_stride = (int64_t)ast; x.b_stride = (int64_t)bst; x.dur_stride = (int64_t)dst;
    x.a = a.data(); x.b = b.data();
    if (with_labels) { x.labels = lab.data(); x.n_labels = nl.data(); }
    x.a_starts = as.data(); x.a_lens = al.data(); x.b_starts = bs.data(); x.b_lens = bl.data();
    x.workspace = ws.data(); x.workspace_bytes = ws.size();
    x.durations = dur.data(); x.state = state.data();
    x.terms = out.data(); x.batch = out.data() + (size_t)B * FS2_ALIGN_TERMS;
    if (int rc = al_align(nullptr, &x)) return rc < 0 ? 100 - rc : rc;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    fwrite(dur.data(), 8, dur.size(), o);
    fwrite(state.data(), 4, state.size(), o);
    fclose(o);
    return 0;
}
