// label_means, prosody_apply and pr_label_means of csrc/prosody.h on the host stand-in.
// Usage: prosody_main means IN OUT   |   prosody_main apply IN OUT   |   prosody_main --checks
//   means IN:  int32 B, S, n_labels, positive_only; int64 lens[B]; float32 x[B, S]; int32 labels[B, S]
//         OUT: float32 mean[B, n_labels]; int32 count[B, n_labels]                 (through pr_label_means, the host side of fs2_op_label_means)
//   apply IN:  int32 R, B, Tmax, cols[4] (pitch_scale, pitch_shift, energy_scale, energy_shift; 0 = NULL); int32 row_pos[R], row_seq[R], lri[R];
//              float32 p_rows[R], e_rows[R]; then float32 [B, cols] for every control that is given, in that order
//         OUT: float32 p_rows[R], e_rows[R]
// --checks: one line "name code" per refused (or accepted) argument set.  Every buffer is a heap block of exactly its size, so that a
// sanitizer build sees an access beyond it.
#include "standin_host.h"
namespace {
#include "prosody.h"

template <typename T> bool read_into(FILE* f, std::vector<T>& v, size_t n) {
    v.assign(n, T{});
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int means(const char* src, const char* dst) {
    FILE* f = fopen(src, "rb");
    int32_t h[4];
    if (!f || fread(h, 4, 4, f) != 4) return 2;
    const int B = h[0], S = h[1], nl = h[2];
    std::vector<int64_t> lens;
    std::vector<float> x;
    std::vector<int32_t> lab;
    if (!read_into(f, lens, B) || !read_into(f, x, (size_t)B * S) || !read_into(f, lab, (size_t)B * S)) return 2;
    fclose(f);
    std::vector<float> mean((size_t)B * nl, -777.f);
    std::vector<int32_t> count((size_t)B * nl, -777);
    if (int rc = pr_label_means(nullptr, x.data(), lab.data(), lens.data(), B, S, nl, h[3], mean.data(), count.data())) return rc < 0 ? 100 - rc : rc;
    FILE* o = fopen(dst, "wb");
    if (!o) return 2;
    fwrite(mean.data(), 4, mean.size(), o);
    fwrite(count.data(), 4, count.size(), o);
    fclose(o);
    return 0;
}

int apply(const char* src, const char* dst) {
    FILE* f = fopen(src, "rb");
    int32_t h[7];
    if (!f || fread(h, 4, 7, f) != 7) return 2;
    const int R = h[0], B = h[1], Tmax = h[2];
    std::vector<int32_t> row_pos, row_seq, lri;
    std::vector<float> p, e, ctl[4];
    if (!read_into(f, row_pos, R) || !read_into(f, row_seq, R) || !read_into(f, lri, R) || !read_into(f, p, R) || !read_into(f, e, R)) return 2;
    for (int k = 0; k < 4; ++k)
        if (h[3 + k] && !read_into(f, ctl[k], (size_t)B * h[3 + k])) return 2;
    fclose(f);
    auto ptr = [&](int k) { return h[3 + k] ? ctl[k].data() : (const float*)nullptr; };
    const ProsodyTrack pitch{ptr(0), ptr(1), h[3] ? h[3] : 1, h[4] ? h[4] : 1}, energy{ptr(2), ptr(3), h[5] ? h[5] : 1, h[6] ? h[6] : 1};
    hipLaunchKernelGGL(prosody_apply, dim3((R + 255) / 256), dim3(256), 0, nullptr, p.data(), e.data(), row_pos.data(), row_seq.data(), lri.data(), R, B, Tmax,
                       pitch, energy);
    FILE* o = fopen(dst, "wb");
    if (!o) return 2;
    fwrite(p.data(), 4, p.size(), o);
    fwrite(e.data(), 4, e.size(), o);
    fclose(o);
    return 0;
}

int checks() {
    const int B = 2, S = 5, nl = 3;
    std::vector<float> x{1.f, 2.f, 3.f, 4.f, 5.f, 6.f, -7.f, 0.f, 9.f, 10.f};
    std::vector<int32_t> lab{0, 0, 2, 2, 2, 1, 1, 1, 2, -1};
    std::vector<int64_t> lens{5, 4};
    std::vector<float> mean(B * nl, -777.f);
    std::vector<int32_t> count(B * nl, -777);
    auto run = [&](const char* name, int b, int s, int n, const float* xp, const int32_t* lp, const int64_t* np, float* mp, int32_t* cp) {
        printf("%s %d\n", name, pr_label_means(nullptr, xp, lp, np, b, s, n, 1, mp, cp));
    };
    run("ok", B, S, nl, x.data(), lab.data(), lens.data(), mean.data(), count.data());
    // positive_only: utterance 0 = {1, 2 | | 3, 4, 5}, utterance 1 = { | 6 (-7 and 0 left out) | 9}, the frame behind lens never read
    printf("ok_counts %d%d%d_%d%d%d\nok_means %d,%d,%d_%d,%d,%d\n", count[0], count[1], count[2], count[3], count[4], count[5], (int)(mean[0] * 2), (int)mean[1],
           (int)mean[2], (int)mean[3], (int)mean[4], (int)mean[5]);
    run("negative_B", -1, S, nl, x.data(), lab.data(), lens.data(), mean.data(), count.data());
    run("negative_x_stride", B, -1, nl, x.data(), lab.data(), lens.data(), mean.data(), count.data());
    run("negative_n_labels", B, S, -1, x.data(), lab.data(), lens.data(), mean.data(), count.data());
    run("null_x", B, S, nl, nullptr, lab.data(), lens.data(), mean.data(), count.data());
    run("null_labels", B, S, nl, x.data(), nullptr, lens.data(), mean.data(), count.data());
    run("null_lens", B, S, nl, x.data(), lab.data(), nullptr, mean.data(), count.data());
    run("null_mean", B, S, nl, x.data(), lab.data(), lens.data(), nullptr, count.data());
    run("null_count", B, S, nl, x.data(), lab.data(), lens.data(), mean.data(), nullptr);
    run("too_many_cells", 70000, S, 70000, x.data(), lab.data(), lens.data(), mean.data(), count.data());
    run("B0_all_null", 0, S, nl, nullptr, nullptr, nullptr, nullptr, nullptr);
    run("n_labels_0_null_outputs", B, S, 0, x.data(), lab.data(), lens.data(), nullptr, nullptr);
    mean.assign(B * nl, -777.f);
    count.assign(B * nl, -777);
    run("x_stride_0_null_inputs", B, 0, nl, nullptr, nullptr, lens.data(), mean.data(), count.data());
    int zeros = 1;
    for (int i = 0; i < B * nl; ++i) zeros &= mean[i] == 0.f && count[i] == 0;
    printf("x_stride_0_writes_zeros %d\n", zeros);
    // lens beyond x_stride and below 0 are clamped; labels that break the contract (decreasing, outside [0, n_labels)): every count
    // stays within the utterance's own frames and nothing beyond them is read (the sanitizer build watches the blocks' ends)
    std::vector<int64_t> wild{1000, -3};
    std::vector<int32_t> bad{2, 0, 1000000, -1, 1, 7, 7, 7, 7, 7};
    run("bad_labels", B, S, nl, x.data(), bad.data(), wild.data(), mean.data(), count.data());
    int in_range = 1;
    for (int i = 0; i < B * nl; ++i) in_range &= count[i] >= 0 && count[i] <= (i < nl ? S : 0);
    printf("bad_labels_counts_in_range %d\n", in_range);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--checks")) return checks();
    if (argc == 4 && !strcmp(argv[1], "means")) return means(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "apply")) return apply(argv[2], argv[3]);
    return 2;
}
