// frame_layout_dev + build_row_meta of csrc/layout.h on the host stand-in, against build_layout (frame_layout) run natively.
// Usage: layout_main IN
//   IN (text): B gap compat masked row_cap work_cap lmax_cap pe_rows, then B frame counts as the duration scan leaves them.
//              row_cap / work_cap / lmax_cap = 0: a sufficient one, sized as the runtime sizes it (fs2_row_capacity of the stored rows,
//              capacity_layout's work_cap, the longest utterance).
// One launch of each kernel, placed in a `meta` block by MetaDev as device_layout places them.  Prints
//   "dims d0 .. d7", and where no flag is set "host_start ..", "host_len ..", "host_klen ..", "host_vlen ..", "host_rows R Rpad",
//   "host_work b:q .." (build_layout's answer, for the test's own restatement of the rule), then a line "mismatch ..." per difference
//   between the device's arrays and the host's (flags set: between them and the empty layout) and "mismatches N".
// Every buffer is a heap block of exactly its size, so that a sanitizer build sees an access beyond it.
#include "hip_standin.h"
#include "fs2.h"
#include "layout.h"

using namespace fs2;

namespace {
int bad = 0;
void expect(bool ok, const char* what, long long i, long long got, long long want) {
    if (ok) return;
    if (++bad <= 20) printf("mismatch %s[%lld] %lld want %lld\n", what, i, got, want);
}
void line(const char* name, const std::vector<int>& v) {
    printf("%s", name);
    for (int x : v) printf(" %d", x);
    printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    int B, gap, compat, masked, row_cap, work_cap, lmax_cap, pe_rows;
    if (!f || fscanf(f, "%d %d %d %d %d %d %d %d", &B, &gap, &compat, &masked, &row_cap, &work_cap, &lmax_cap, &pe_rows) != 8 || B <= 0) return 2;
    std::vector<int> olens(B);
    for (int b = 0; b < B; ++b)
        if (fscanf(f, "%d", &olens[b]) != 1) return 2;
    fclose(f);
    int mx = 0;
    long long stored = 0;
    for (int v : olens) mx = std::max(mx, v);
    for (int v : olens) stored += utt_lens(std::max(v, 0), mx, compat, masked).len;
    if (row_cap == 0) row_cap = rows_padded(row_bound(stored, B));
    if (lmax_cap == 0) lmax_cap = mx;
    if (work_cap == 0) work_cap = work_capacity(row_cap, B, lmax_cap);
    const int Rpad = rows_padded(row_cap);
    const MetaDev m = MetaDev::at(B, Rpad, work_cap);
    if (m.end > MetaDev::ints(B, Rpad, work_cap)) return 3;
    std::vector<int> meta(MetaDev::ints(B, Rpad, work_cap), 0x5a5a5a5a), status(8, 0x5a5a5a5a);
    int* dev = meta.data();
    int2* work = reinterpret_cast<int2*>(dev + m.work);
    hipLaunchKernelGGL(frame_layout_dev, dim3(1), dim3(kLayoutThreads), 0, nullptr, (const int*)olens.data(), B, compat, masked, row_cap, work_cap, lmax_cap, pe_rows,
                       dev + m.start, dev + m.len, dev + m.klen, dev + m.vlen, dev + m.rank, dev + m.woff, dev + m.pcum, work, dev + m.dims, status.data(), gap);
    hipLaunchKernelGGL(build_row_meta, dim3((Rpad + 255) / 256), dim3(256), 0, nullptr, (const int*)(dev + m.start), (const int*)(dev + m.len), B, Rpad, dev + m.row_pos,
                       dev + m.row_seq);
    const int* dims = dev + m.dims;
    printf("dims");
    for (int i = 0; i < 8; ++i) printf(" %d", dims[i]);
    printf("\n");
    for (int i = 0; i < 8; ++i) expect(status[i] == dims[i], "status", i, status[i], dims[i]);
    for (int i = 5; i < 8; ++i) expect(dims[i] == 0, "dims", i, dims[i], 0);
    expect(dims[3] == mx, "dims", 3, dims[3], mx);

    HostLayout L;      // what the device must have built: the host's layout of the same counts, or the empty one
    std::vector<int> pcum(B, 0);
    if (dims[2] == 0) {
        fs2_batch bt{};
        bt.B = B; bt.compat_padded = compat;
        std::vector<int64_t> o64(olens.begin(), olens.end());
        frame_layout(bt, o64.data(), masked, L, gap);
        for (int b = 1; b < B; ++b) pcum[b] = pcum[b - 1] + L.vlen[b - 1];
        line("host_start", L.start); line("host_len", L.len); line("host_klen", L.klen); line("host_vlen", L.vlen);
        printf("host_rows %d %d\nhost_work", L.R, L.Rpad);
        for (const int2& w : L.work) printf(" %d:%d", w.x, w.y);
        printf("\n");
        expect(dims[0] == L.R, "dims", 0, dims[0], L.R);
        expect(dims[1] == (int)L.work.size(), "dims", 1, dims[1], (long long)L.work.size());
        expect(dims[4] == pcum[B - 1] + L.vlen[B - 1], "dims", 4, dims[4], pcum[B - 1] + L.vlen[B - 1]);
        for (int b = 0; b < B; ++b) expect(dev[m.pcum + b] == pcum[b], "pcum", b, dev[m.pcum + b], pcum[b]);
    } else {
        L.B = B;
        L.start.assign(B, row_start(gap)); L.len.assign(B, 0); L.klen.assign(B, 0); L.vlen.assign(B, 0);
        expect(dims[1] == 0, "dims", 1, dims[1], 0);
    }
    for (int b = 0; b < B; ++b) {
        expect(dev[m.start + b] == L.start[b], "start", b, dev[m.start + b], L.start[b]);
        expect(dev[m.len + b] == L.len[b], "len", b, dev[m.len + b], L.len[b]);
        expect(dev[m.klen + b] == L.klen[b], "klen", b, dev[m.klen + b], L.klen[b]);
        expect(dev[m.vlen + b] == L.vlen[b], "vlen", b, dev[m.vlen + b], L.vlen[b]);
    }
    for (int i = 0; i < work_cap; ++i) {
        const int2 want = i < (int)L.work.size() ? L.work[i] : make_int2(-1, 0);
        expect(work[i].x == want.x, "work.b", i, work[i].x, want.x);
        expect(work[i].y == want.y, "work.q", i, work[i].y, want.y);
    }
    std::vector<int> pos(Rpad, -1), seq(Rpad, -1);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < L.len[b]; ++j) { pos[L.start[b] + j] = j; seq[L.start[b] + j] = b; }
    for (int r = 0; r < Rpad; ++r) {
        expect(dev[m.row_pos + r] == pos[r], "row_pos", r, dev[m.row_pos + r], pos[r]);
        expect(dev[m.row_seq + r] == seq[r], "row_seq", r, dev[m.row_seq + r], seq[r]);
    }
    printf("mismatches %d\n", bad);
    return bad ? 1 : 0;
}
