// pp_pitch_path of csrc/pitch_path.h on the host stand-in.  Usage: pitch_path_main IN OUT   |   pitch_path_main --checks
//   IN:  int32 B, K, rows; float64 time_step, f0_floor, voicing_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost;
//        int32 frame_starts[B], frame_lens[B]; float32 cand_f0 [rows, K], cand_strength [rows, K]
//   OUT: float64 terms[B][8], float64 batch[8], float32 f0[rows], int32 state[rows], float32 strength[rows]
// Rows no utterance covers keep -777.  --checks: one line "name code" per refused (or accepted) argument set.  Every buffer is a
// heap block of exactly its size, so that a sanitizer build sees an access beyond it.
#include "standin_host.h"
// the indexed shuffle, which the stand-in does not have: the value of lane `src` of the caller's wave
template <typename T> T __shfl(T v, int src) { return shfl_from(v, src); }
namespace {
#include "pitch_path.h"

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n) {
    v.assign(n, T{});
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int checks() {
    const int B = 2, K = 2, rows = 5;
    // utterance 0: three frames, the strong candidate at 200 Hz throughout; utterance 1: two frames without a candidate
    std::vector<float> cf{200.f, 100.f, 200.f, 0.f, 201.f, 400.f, 0.f, 0.f, 0.f, 0.f}, cp{0.9f, 0.5f, 0.8f, 0.f, 0.9f, 0.6f, 0.f, 0.f, 0.f, 0.f};
    int32_t st[2] = {0, 3}, ln[2] = {3, 2};
    std::vector<char> ws(path_workspace_bytes(B, ln));
    std::vector<double> terms(B * FS2_PITCH_PATH_TERMS), batch(FS2_PITCH_PATH_TERMS);
    std::vector<float> f0(rows), strength(rows);
    std::vector<int32_t> state(rows);
    fs2_op_pitch_path_args ok{};
    ok.struct_size = sizeof(ok);
    ok.B = B; ok.n_candidates = K;
    ok.time_step = 0.01; ok.f0_floor = 71.0; ok.voicing_threshold = 0.45; ok.octave_cost = 0.02; ok.octave_jump_cost = 0.35; ok.voiced_unvoiced_cost = 0.14;
    ok.cand_f0 = cf.data(); ok.cand_strength = cp.data();
    ok.workspace = ws.data(); ok.workspace_bytes = ws.size();
    ok.f0 = f0.data(); ok.state = state.data(); ok.strength = strength.data(); ok.terms = terms.data(); ok.batch = batch.data();
    auto run = [&](const char* name, auto edit) {
        fs2_op_pitch_path_args x = ok;
        int32_t st2[2] = {st[0], st[1]}, ln2[2] = {ln[0], ln[1]};
        x.frame_starts = st2; x.frame_lens = ln2;
        edit(x, st2, ln2);
        printf("%s %d\n", name, pp_pitch_path(nullptr, &x));
    };
    run("ok", [](auto&, int32_t*, int32_t*) {});
    printf("ok_state %d%d%d_%d%d\nok_voiced %d%d\nok_batch_frames %d\n", state[0], state[1], state[2], state[3], state[4], (int)terms[3],
           (int)terms[FS2_PITCH_PATH_TERMS + 3], (int)batch[0]);
    const double nan = std::nan(""), inf = __builtin_huge_val();
    run("struct_size", [](auto& x, int32_t*, int32_t*) { x.struct_size += 8; });
    run("K_0", [](auto& x, int32_t*, int32_t*) { x.n_candidates = 0; });
    run("K_9", [](auto& x, int32_t*, int32_t*) { x.n_candidates = 9; });
    run("negative_B", [](auto& x, int32_t*, int32_t*) { x.B = -1; });
    run("null_lens", [](auto& x, int32_t*, int32_t*) { x.frame_lens = nullptr; });
    run("null_starts", [](auto& x, int32_t*, int32_t*) { x.frame_starts = nullptr; });
    run("negative_len", [](auto&, int32_t*, int32_t* l) { l[1] = -1; });
    run("negative_start", [](auto&, int32_t* s, int32_t*) { s[0] = -2; });
    run("time_step_0", [](auto& x, int32_t*, int32_t*) { x.time_step = 0.0; });
    run("time_step_negative", [](auto& x, int32_t*, int32_t*) { x.time_step = -0.01; });
    run("time_step_nan", [=](auto& x, int32_t*, int32_t*) { x.time_step = nan; });
    run("time_step_inf", [=](auto& x, int32_t*, int32_t*) { x.time_step = inf; });
    run("f0_floor_0", [](auto& x, int32_t*, int32_t*) { x.f0_floor = 0.0; });
    run("f0_floor_nan", [=](auto& x, int32_t*, int32_t*) { x.f0_floor = nan; });
    run("threshold_nan", [=](auto& x, int32_t*, int32_t*) { x.voicing_threshold = nan; });
    run("octave_cost_inf", [=](auto& x, int32_t*, int32_t*) { x.octave_cost = inf; });
    run("octave_jump_cost_negative", [](auto& x, int32_t*, int32_t*) { x.octave_jump_cost = -0.1; });
    run("octave_jump_cost_nan", [=](auto& x, int32_t*, int32_t*) { x.octave_jump_cost = nan; });
    run("voiced_unvoiced_cost_negative", [](auto& x, int32_t*, int32_t*) { x.voiced_unvoiced_cost = -0.1; });
    run("voiced_unvoiced_cost_inf", [=](auto& x, int32_t*, int32_t*) { x.voiced_unvoiced_cost = inf; });
    run("zero_costs", [](auto& x, int32_t*, int32_t*) { x.octave_jump_cost = 0.0; x.voiced_unvoiced_cost = 0.0; });
    run("null_candidates", [](auto& x, int32_t*, int32_t*) { x.cand_f0 = nullptr; });
    run("null_workspace", [](auto& x, int32_t*, int32_t*) { x.workspace = nullptr; });
    run("workspace_one_byte_short", [](auto& x, int32_t*, int32_t*) { x.workspace_bytes -= 1; });
    run("no_outputs", [](auto& x, int32_t*, int32_t*) { x.f0 = nullptr; x.state = nullptr; x.strength = nullptr; x.terms = nullptr; x.batch = nullptr; });
    batch.assign(FS2_PITCH_PATH_TERMS, 7.0);
    run("B0", [](auto& x, int32_t*, int32_t*) { x.B = 0; x.workspace = nullptr; x.workspace_bytes = 0; x.terms = nullptr; x.frame_starts = nullptr; x.frame_lens = nullptr; });
    double s = 0.0;
    for (double v : batch) s += fabs(v);
    printf("B0_batch_abs_sum %d\n", (int)s);
    int32_t neg[1] = {-1}, one[1] = {1}, two[1] = {2};
    printf("workspace_negative_B %zu\nworkspace_null_lens %zu\nworkspace_negative_len %zu\nworkspace_B0 %d\nworkspace_per_frame %zu\n",
           path_workspace_bytes(-1, ln), path_workspace_bytes(1, nullptr), path_workspace_bytes(1, neg), path_workspace_bytes(0, nullptr) > 0,
           (path_workspace_bytes(1, two) >= path_workspace_bytes(1, one)) ? sizeof(uint64_t) : 0);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--checks")) return checks();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[3];
    double c[6];
    if (!f || fread(h, 4, 3, f) != 3 || fread(c, 8, 6, f) != 6) return 2;
    const int B = h[0], K = h[1];
    const size_t rows = h[2];
    std::vector<int32_t> st, ln;
    std::vector<float> cf, cp;
    if (!read_into(f, st, B) || !read_into(f, ln, B) || !read_into(f, cf, rows * K) || !read_into(f, cp, rows * K)) return 2;
    fclose(f);
    std::vector<char> ws(path_workspace_bytes(B, ln.data()));
    std::vector<double> out((size_t)(B + 1) * FS2_PITCH_PATH_TERMS, -777.0);
    std::vector<float> f0(rows, -777.f), strength(rows, -777.f);
    std::vector<int32_t> state(rows, -777);
    fs2_op_pitch_path_args x{};
    x.struct_size = sizeof(x);
    x.B = B; x.n_candidates = K;
    x.time_step = c[0]; x.f0_floor = c[1]; x.voicing_threshold = c[2]; x.octave_cost = c[3]; x.octave_jump_cost = c[4]; x.voiced_unvoiced_cost = c[5];
    x.cand_f0 = cf.data(); x.cand_strength = cp.data();
    x.frame_starts = st.data(); x.frame_lens = ln.data();
    x.workspace = ws.data(); x.workspace_bytes = ws.size();
    x.f0 = f0.data(); x.state = state.data(); x.strength = strength.data();
    x.terms = out.data(); x.batch = out.data() + (size_t)B * FS2_PITCH_PATH_TERMS;
    if (int rc = pp_pitch_path(nullptr, &x)) return rc < 0 ? 100 - rc : rc;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    fwrite(f0.data(), 4, f0.size(), o);
    fwrite(state.data(), 4, state.size(), o);
    fwrite(strength.data(), 4, strength.size(), o);
    fclose(o);
    return 0;
}
