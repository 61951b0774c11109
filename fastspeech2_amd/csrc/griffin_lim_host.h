// Host side of the vocoder (kernels: griffin_lim.h): geometry, workspace layout, host plan, launch sequence and the argument checks
// behind fs2_op_griffin_lim{,_geom,_dev}, fs2_op_griffin_lim_mel_{geom,dev}, fs2_op_stft{,_geom}, fs2_op_stft_pitch_geom and their workspace
// queries (include/fs2.h).
// The host-planned call, the device-driven call and the analysis STFT share one workspace layout (gl_layout), one check of the
// synthesis arguments (gl_check_synthesis), one GlIterArgs builder (gl_iter_args) and one choice of instantiation (gl_dispatch).
// Not a header of its own: fs2_runtime.hip includes it inside its unnamed namespace, after fail() and align_up(), so the library
// stays one translation unit; the extern "C" entry points are with the others at the end of fs2_runtime.hip.

// Geometry of a call: validated (n_fft, hop, win, n_mels) plus the tile rule (F, halo, tail frame, L_min, signal buffer) derived from it.
struct GlGeomHost {
    int n_fft = kGlNfft, hop = kGlHop, win = kGlNfft, n_mels = 80, n_bins = kGlBins;
    GlGeom g{};
    size_t sig_bytes = 0;                // dynamic LDS of the fused kernel (0: the default instantiation, static LDS)
    bool is_default() const { return n_fft == kGlNfft && hop == kGlHop; }
};

int gl_geom(int n_fft, int hop, int win, int n_mels, const char* who, GlGeomHost& out) {
    GlGeomHost h;
    h.n_fft = n_fft; h.hop = hop; h.win = win; h.n_mels = n_mels;
    if (h.n_fft != 512 && h.n_fft != 1024 && h.n_fft != 2048)
        return fail(nullptr, FS2_ERR_UNSUPPORTED, "%s: n_fft %d (512, 1024 or 2048)", who, h.n_fft);
    if (h.hop < 1 || h.hop > h.win || h.win > h.n_fft || (h.n_fft + h.hop - 1) / h.hop > 8)
        return fail(nullptr, FS2_ERR_UNSUPPORTED, "%s: hop %d, win %d at n_fft %d (hop <= win <= n_fft, ceil(n_fft / hop) <= 8)", who, h.hop, h.win, h.n_fft);
    if (h.n_mels < 1 || h.n_mels > kGlMaxMels) return fail(nullptr, FS2_ERR_UNSUPPORTED, "%s: n_mels %d (1 .. %d)", who, h.n_mels, kGlMaxMels);
    h.n_bins = h.n_fft / 2 + 1;
    h.g.hop = h.hop;
    h.g.F = h.is_default() ? kGlTile : gl_tile_frames(h.n_fft, h.hop);
    h.g.halo = gl_halo(h.n_fft, h.hop);
    h.g.tail = gl_tail(h.n_fft, h.hop);
    h.g.lmin = gl_lmin(h.n_fft, h.hop);
    h.g.sig_max = gl_sig_max(h.n_fft, h.hop, h.g.F);
    h.g.n_mels = h.n_mels;
    h.sig_bytes = h.is_default() ? 0 : (size_t)h.g.sig_max * sizeof(float);
    out = h;
    return FS2_OK;
}

// One choice of instantiation: f(NFFT, HOP_C) with both as std::integral_constant -- <1024, kGlHop> for the default transform
// (static LDS), <n_fft, 0> for every other one (hop at run time).
template <typename Fn>
auto gl_dispatch(const GlGeomHost& gh, Fn&& f) {
    using std::integral_constant;
    if (gh.is_default()) return f(integral_constant<int, 1024>{}, integral_constant<int, kGlHop>{});
    if (gh.n_fft == 512) return f(integral_constant<int, 512>{}, integral_constant<int, 0>{});
    if (gh.n_fft == 1024) return f(integral_constant<int, 1024>{}, integral_constant<int, 0>{});
    return f(integral_constant<int, 2048>{}, integral_constant<int, 0>{});
}

// Workspace of every vocoder call: tables, tile records, the device planner's per-utterance arrays (device-driven call only), then
// (synthesis only) M, the two spectrum buffers and the momentum state over `frames` frames packed back to back, then (analysis with
// pitch only) the window-autocorrelation table of gl_pitch.h, then (mel-constrained synthesis only) the band tables of
// gl_band_tables.  Each region starts 256-byte aligned.
struct GlLayout {
    size_t off_tw = 0, off_win = 0, off_tiles = 0, off_plan = 0, off_M = 0, off_C0 = 0, off_C1 = 0, off_T = 0, off_acw = 0, off_band = 0, bytes = 0;
};

// records: tile records (the exact tile count of a host plan, the slots of a device-driven call); planner_B: utterances the device
// planner keeps its 4 ints each for, < 0: a host-planned call, no such region.  0 records / 0 utterances still reserve one.
GlLayout gl_layout(const GlGeomHost& gh, size_t records, int64_t planner_B, int64_t frames, bool analysis, bool pitch = false, bool band = false) {
    GlLayout l;
    size_t off = 0;
    auto take = [&](size_t n) { off = align_up(off, 256); size_t o = off; off += n; return o; };
    l.off_tw = take(gh.n_fft * sizeof(float2));
    l.off_win = take(gh.n_fft * sizeof(float));
    l.off_tiles = take(std::max<size_t>(records, 1) * sizeof(GlTile));
    if (planner_B >= 0) l.off_plan = take(std::max<size_t>((size_t)planner_B, 1) * 4 * sizeof(int));
    if (!analysis) {
        const size_t n = (size_t)frames * gh.n_bins;
        l.off_M = take(n * sizeof(float));
        l.off_C0 = take(n * sizeof(float2));
        l.off_C1 = take(n * sizeof(float2));
        l.off_T = take(n * sizeof(float2));
    }
    if (pitch) l.off_acw = take(gl_pitch_lags(gh.n_fft) * sizeof(float));
    if (band) l.off_band = take(gl_band_bytes(gh.n_bins));
    l.bytes = align_up(off, 256);
    return l;
}

// Host plan of fs2_op_griffin_lim / fs2_op_stft: the exact tile list and the workspace laid out for it.  frames[b] = L_b; tiles cover
// utterances with L_b >= 2 (synthesis: they own samples) or every utterance with frames (analysis).
struct GlPlan {
    std::vector<GlTile> tiles;
    int64_t frames = 0, samples = 0;
    GlLayout at;
};

// analysis = false: lens are frame counts L_b, samples hop max(L_b - 1, 0).  analysis = true: lens are sample counts T_b,
// frames T_b / hop + 1.  starts: source rows (synthesis) or waveform samples (analysis), may be NULL for the size query.
int gl_plan(int B, const int32_t* starts, const int32_t* lens, bool analysis, const GlGeomHost& gh, GlPlan& p, bool pitch = false, bool band = false) {
    if (B < 0 || (B > 0 && !lens)) return fail(nullptr, FS2_ERR_ARG, "vocoder: bad batch (B = %d)", B);
    const int hop = gh.hop, F = gh.g.F, nb = gh.n_bins;
    int64_t row = 0, wav = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || (starts && starts[b] < 0)) return fail(nullptr, FS2_ERR_ARG, "vocoder: negative length / start of utterance %d", b);
        const int L = analysis ? lens[b] / hop + 1 : lens[b];
        const int64_t T = analysis ? (int64_t)lens[b] : (int64_t)hop * std::max(L - 1, 0);
        const bool owns = analysis ? L > 0 : L >= 2;
        if (T > INT32_MAX) return fail(nullptr, FS2_ERR_ARG, "vocoder: utterance %d too long (%lld samples)", b, (long long)T);
        if (owns)
            for (int f0 = 0; f0 < L; f0 += F) {
                GlTile t{};
                t.src_row0 = analysis ? (int)row : (starts ? starts[b] : 0);
                t.ws_row0 = (int)row;
                t.L = L; t.f0 = f0; t.T = (int)T;
                t.wav0 = analysis ? (starts ? starts[b] : 0) : (int)wav;
                p.tiles.push_back(t);
            }
        row += L;
        wav += T;
        if (row > INT32_MAX / nb || wav > INT32_MAX) return fail(nullptr, FS2_ERR_ARG, "vocoder: batch too large (%lld frames, %lld samples)", (long long)row, (long long)wav);
    }
    p.frames = row;
    p.samples = wav;
    p.at = gl_layout(gh, p.tiles.size(), -1, p.frames, analysis, pitch, band);
    return FS2_OK;
}

// Workgroups (= tile records) of a device-driven call of B utterances inside frame_capacity (gl_slot_rule.h), or -1: the
// capacities are negative or too large for one call.
int64_t gl_cap_slots(const GlGeomHost& gh, int64_t B, int64_t frame_capacity) {
    if (B < 0 || frame_capacity < 0 || frame_capacity > INT32_MAX / gh.n_bins) return -1;
    const int64_t slots = gl_slot_capacity(frame_capacity, gh.g.F, (int)B);
    return slots > INT32_MAX ? -1 : slots;
}

void gl_put_tables(hipStream_t s, const GlGeomHost& gh, const GlLayout& at, char* ws) {
    hipLaunchKernelGGL(gl_tables, dim3((gh.n_fft + 255) / 256), dim3(256), 0, s, (float2*)(ws + at.off_tw), (float*)(ws + at.off_win),
                       gh.n_fft, gh.win);
}

// tables + tile records into the workspace (kernel arguments, no host copy)
hipError_t gl_setup(hipStream_t s, const GlPlan& p, const GlGeomHost& gh, char* ws) {
    gl_put_tables(s, gh, p.at, ws);
    for (size_t i = 0; i < p.tiles.size(); i += kGlTilesPerChunk) {
        GlTileChunk c{};
        c.n = (int)std::min<size_t>(kGlTilesPerChunk, p.tiles.size() - i);
        c.base = (int)i;
        std::copy(p.tiles.begin() + i, p.tiles.begin() + i + c.n, c.t);
        hipLaunchKernelGGL(gl_upload_tiles, dim3(1), dim3(128), 0, s, c, (GlTile*)(ws + p.at.off_tiles));
    }
    return hipGetLastError();
}

// proj: the projection of an iteration (gl_iterate's PROJ): 0 onto M, 1 mel-constrained, with mp filled in
struct GlIterArgs {
    const GlTile* tiles; const float2* tw; const float* win; const float* M; float2* C[2]; float2* Tm; float beta; float* wav;
    int proj; GlMelProj mp;
};

// mel_basis != NULL: a mel-constrained call (its layout has the band region); src is then the call's log-mel source
GlIterArgs gl_iter_args(char* ws, const GlLayout& at, float momentum, float* wav, const float* src = nullptr, const float* mel_basis = nullptr,
                        int n_bins = 0) {
    GlIterArgs a{};
    a.tiles = (const GlTile*)(ws + at.off_tiles);
    a.tw = (const float2*)(ws + at.off_tw);
    a.win = (const float*)(ws + at.off_win);
    a.M = (const float*)(ws + at.off_M);
    a.C[0] = (float2*)(ws + at.off_C0);
    a.C[1] = (float2*)(ws + at.off_C1);
    a.Tm = momentum > 0.f ? (float2*)(ws + at.off_T) : nullptr;
    a.beta = momentum / (1.f + momentum);
    a.wav = wav;
    if (mel_basis) {
        a.proj = 1;
        a.mp.mel = src;
        a.mp.basis = mel_basis;
        a.mp.row_rng = (const int2*)(ws + at.off_band);
        a.mp.bin_rng = a.mp.row_rng + kGlMaxMels;
        a.mp.inv_w = (const float*)(a.mp.bin_rng + n_bins);
        a.mp.band = a.mp.inv_w + n_bins;
    }
    return a;
}

// prologue, n_iter fused iterations and the final ISTFT of one geometry (NFFT; HOP_C = 256: the default instantiation)
template <int NFFT, int HOP_C>
hipError_t gl_run(hipStream_t s, const GlGeomHost& gh, unsigned n_tiles, const float* src, int src_width, const float* pinv,
                  const float* init_phase, uint32_t seed, int n_iter, const GlIterArgs& a) {
    const dim3 grid(n_tiles), blk(kGlThreads);
    const GlGeom g = gh.g;
    const size_t lds = gh.sig_bytes;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (lds && hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    // Set on every eager call, not once per instantiation: the byte count follows the hop (<1024, 0> at hop 200 and at hop 300
    // differ).  Host work only, skipped while capturing: a captured call relies on the eager call before it.
    if (lds && cap == hipStreamCaptureStatusNone) {
        for (const void* k : {(const void*)gl_iterate<NFFT, HOP_C, 0, false>, (const void*)gl_iterate<NFFT, HOP_C, 0, true>,
                              (const void*)gl_iterate<NFFT, HOP_C, 1, false>})
            if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); e != hipSuccess) return e;
        if (a.proj)
            for (const void* k : {(const void*)gl_iterate<NFFT, HOP_C, 0, false, 1>, (const void*)gl_iterate<NFFT, HOP_C, 0, true, 1>})
                if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); e != hipSuccess) return e;
    }
    if (src_width == 80 && gh.n_mels == 80 && src_width != gh.n_bins)
        hipLaunchKernelGGL((gl_prologue<NFFT, 80>), grid, blk, 0, s, a.tiles, g, src, src_width, pinv, init_phase, seed, (float*)a.M, a.C[0], a.Tm);
    else
        hipLaunchKernelGGL((gl_prologue<NFFT, 0>), grid, blk, 0, s, a.tiles, g, src, src_width, pinv, init_phase, seed, (float*)a.M, a.C[0], a.Tm);
    const GlMelProj none{};
    if (a.proj && n_iter > 0)       // the band tables of this call's basis, read by the iterations only
        hipLaunchKernelGGL(gl_band_tables, dim3((gh.n_bins + kGlThreads - 1) / kGlThreads), blk, 0, s, a.mp.basis, gh.n_mels, gh.n_bins,
                           const_cast<int2*>(a.mp.row_rng), const_cast<int2*>(a.mp.bin_rng), const_cast<float*>(a.mp.inv_w),
                           const_cast<float*>(a.mp.band));
    for (int it = 0; it < n_iter; ++it) {
        if (a.proj && a.Tm) hipLaunchKernelGGL((gl_iterate<NFFT, HOP_C, 0, true, 1>), grid, blk, lds, s, a.tiles, g, a.tw, a.win, a.M, a.C[it & 1], a.C[(it + 1) & 1], a.Tm, a.beta, a.wav, a.mp);
        else if (a.proj) hipLaunchKernelGGL((gl_iterate<NFFT, HOP_C, 0, false, 1>), grid, blk, lds, s, a.tiles, g, a.tw, a.win, a.M, a.C[it & 1], a.C[(it + 1) & 1], a.Tm, a.beta, a.wav, a.mp);
        else if (a.Tm) hipLaunchKernelGGL((gl_iterate<NFFT, HOP_C, 0, true>), grid, blk, lds, s, a.tiles, g, a.tw, a.win, a.M, a.C[it & 1], a.C[(it + 1) & 1], a.Tm, a.beta, a.wav, none);
        else hipLaunchKernelGGL((gl_iterate<NFFT, HOP_C, 0, false>), grid, blk, lds, s, a.tiles, g, a.tw, a.win, a.M, a.C[it & 1], a.C[(it + 1) & 1], a.Tm, a.beta, a.wav, none);
    }
    hipLaunchKernelGGL((gl_iterate<NFFT, HOP_C, 1, false>), grid, blk, lds, s, a.tiles, g, a.tw, a.win, a.M, a.C[n_iter & 1], a.C[(n_iter + 1) & 1], nullptr, 0.f, a.wav, none);
    return hipGetLastError();
}

// what the host-planned and the device-driven synthesis check first, in this order (mel_proj: the mel-constrained entry points,
// which have no use for a magnitude source and need the basis)
int gl_check_synthesis(const char* who, const GlGeomHost& gh, int32_t src_width, const float* mel_pinv, int32_t n_iter, float momentum,
                       bool mel_proj = false, const float* mel_basis = nullptr) {
    if (src_width != gh.n_mels && src_width != gh.n_bins)
        return fail(nullptr, FS2_ERR_UNSUPPORTED, "%s: src_width %d (%d mel bins or %d linear bins of the %d-point STFT)", who, src_width, gh.n_mels,
                    gh.n_bins, gh.n_fft);
    if (src_width != gh.n_bins && !mel_pinv) return fail(nullptr, FS2_ERR_ARG, "%s: mel input needs mel_pinv [%d, %d]", who, gh.n_bins, gh.n_mels);
    if (n_iter < 0 || !(momentum >= 0.f) || !std::isfinite(momentum)) return fail(nullptr, FS2_ERR_ARG, "%s: n_iter %d, momentum %g", who, n_iter, momentum);
    if (mel_proj && src_width != gh.n_mels)
        return fail(nullptr, FS2_ERR_ARG, "%s: src_width %d is a magnitude source: there is no mel to constrain to (%d mel bins)", who, src_width, gh.n_mels);
    if (mel_proj && !mel_basis) return fail(nullptr, FS2_ERR_ARG, "%s: null mel_basis [%d, %d]", who, gh.n_mels, gh.n_bins);
    return FS2_OK;
}

// the launches of a synthesis whose tile records are in place (uploaded, or being written by the planner ahead on the stream)
int gl_synthesize(hipStream_t s, const GlGeomHost& gh, unsigned n_tiles, const float* src, int32_t src_width, const float* mel_pinv,
                  const float* init_phase, uint32_t seed, int32_t n_iter, const GlIterArgs& a) {
    const hipError_t e = gl_dispatch(gh, [&](auto n, auto h) {
        return gl_run<decltype(n)::value, decltype(h)::value>(s, gh, n_tiles, src, src_width, mel_pinv, init_phase, seed, n_iter, a);
    });
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "griffin_lim: %s", hipGetErrorString(e));
    return FS2_OK;
}

int gl_griffin_lim(const char* who, void* stream, const GlGeomHost& gh, const float* src, int32_t src_width, const float* mel_pinv, int32_t B,
                   const int32_t* starts, const int32_t* lens, int32_t n_iter, float momentum, uint32_t seed, const float* init_phase,
                   void* workspace, size_t workspace_bytes, float* wav, bool mel_proj = false, const float* mel_basis = nullptr) {
    if (int rc = gl_check_synthesis(who, gh, src_width, mel_pinv, n_iter, momentum, mel_proj, mel_basis)) return rc;
    if (B > 0 && (!starts || !lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
    GlPlan p;
    if (int rc = gl_plan(B, starts, lens, false, gh, p, false, mel_proj)) return rc;
    if (p.tiles.empty()) return FS2_OK;
    if (!src || !wav || !workspace) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    if (workspace_bytes < p.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, p.at.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    hipError_t e = gl_setup(s, p, gh, ws);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "griffin_lim setup: %s", hipGetErrorString(e));
    return gl_synthesize(s, gh, (unsigned)p.tiles.size(), src, src_width, mel_pinv, init_phase, seed, n_iter,
                         gl_iter_args(ws, p.at, momentum, wav, src, mel_proj ? mel_basis : nullptr, gh.n_bins));
}

static_assert(kGlOvfRows == FS2_OVF_ROWS && kGlOvfLmax == FS2_OVF_LMAX && kGlOvfUpstream == FS2_OVF_UPSTREAM && kGlOvfNegative == FS2_OVF_NEG_LEN &&
              kGlOvfWav == FS2_OVF_WAV, "griffin_lim.h restates the FS2_OVF_* bits");

// The device-driven call: the layout of a host plan with every size taken from the capacities (gl_cap_slots records,
// frame_capacity frames), plus the planner's per-utterance arrays.
int gl_griffin_lim_dev(const char* who, void* stream, const GlGeomHost& gh, const float* src, int32_t src_width, const float* mel_pinv, int32_t B,
                       const int64_t* lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status, int32_t n_iter,
                       float momentum, uint32_t seed, const float* init_phase, void* workspace, size_t workspace_bytes, float* wav,
                       int32_t wav_stride, int64_t wav_capacity, int64_t* sample_lens_dev, int32_t* status, bool mel_proj = false,
                       const float* mel_basis = nullptr) {
    if (int rc = gl_check_synthesis(who, gh, src_width, mel_pinv, n_iter, momentum, mel_proj, mel_basis)) return rc;
    if (B < 1 || frame_capacity < 1 || src_stride < 0 || wav_stride < 0)
        return fail(nullptr, FS2_ERR_ARG, "%s: B %d, frame_capacity %lld, src_stride %d, wav_stride %d", who, B, (long long)frame_capacity, src_stride, wav_stride);
    if (frame_capacity > INT32_MAX / gh.n_bins || wav_capacity < 0 || wav_capacity > INT32_MAX || (int64_t)B * src_stride > INT32_MAX)
        return fail(nullptr, FS2_ERR_ARG, "%s: capacities too large for one call (%lld frames, %lld samples)", who, (long long)frame_capacity, (long long)wav_capacity);
    if ((int64_t)B * wav_stride > wav_capacity)
        return fail(nullptr, FS2_ERR_ARG, "%s: padded output of %d x %d samples in a wav of %lld", who, B, wav_stride, (long long)wav_capacity);
    if (!src || !lens_dev || !workspace || !sample_lens_dev || !status || (wav_capacity > 0 && !wav)) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    const int64_t slots = gl_cap_slots(gh, B, frame_capacity);
    if (slots < 0) return fail(nullptr, FS2_ERR_ARG, "%s: capacities too large for one call", who);
    const GlLayout at = gl_layout(gh, (size_t)slots, B, frame_capacity, false, false, mel_proj);
    if (workspace_bytes < at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, at.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    gl_put_tables(s, gh, at, ws);
    GlPlanArgs pa{};
    pa.lens = lens_dev; pa.upstream = upstream_status;
    pa.B = B; pa.hop = gh.hop; pa.F = gh.g.F;
    pa.src_stride = src_stride; pa.wav_stride = wav_stride;
    pa.frame_capacity = frame_capacity; pa.wav_capacity = wav_capacity;
    int* plan = (int*)(ws + at.off_plan);
    pa.row0 = plan; pa.wav0 = plan + B; pa.tile_end = plan + 2 * (size_t)B; pa.Lv = plan + 3 * (size_t)B;
    pa.sample_lens = sample_lens_dev; pa.status = status;
    const int n_slots = (int)slots;          // >= B >= 1
    hipLaunchKernelGGL(gl_plan_scan, dim3(1), dim3(kGlPlanThreads), 0, s, pa);
    hipLaunchKernelGGL(gl_plan_emit, dim3((n_slots + 255) / 256), dim3(256), 0, s, pa, n_slots, (GlTile*)(ws + at.off_tiles));
    if (wav_capacity > 0)
        hipLaunchKernelGGL(gl_plan_fill, dim3((unsigned)std::min<int64_t>((wav_capacity + 1023) / 1024, 2048)), dim3(256), 0, s, pa, wav);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "griffin_lim plan: %s", hipGetErrorString(e));
    return gl_synthesize(s, gh, (unsigned)n_slots, src, src_width, mel_pinv, init_phase, seed, n_iter,
                         gl_iter_args(ws, at, momentum, wav, src, mel_proj ? mel_basis : nullptr, gh.n_bins));
}

int gl_stft_run(const char* who, void* stream, const GlGeomHost& gh, const float* wav, int32_t B, const int32_t* wav_starts,
                const int32_t* wav_lens, void* workspace, size_t workspace_bytes, float* mag, const float* mel_basis, float* logmel, float* energy) {
    if (B > 0 && (!wav_starts || !wav_lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
    if (logmel && !mel_basis) return fail(nullptr, FS2_ERR_ARG, "%s: logmel needs mel_basis [%d, %d]", who, gh.n_mels, gh.n_bins);
    GlPlan p;
    if (int rc = gl_plan(B, wav_starts, wav_lens, true, gh, p)) return rc;
    if (p.tiles.empty() || (!mag && !logmel && !energy)) return FS2_OK;
    if (!wav || !workspace) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    if (workspace_bytes < p.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, p.at.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    hipError_t e = gl_setup(s, p, gh, ws);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "stft setup: %s", hipGetErrorString(e));
    const dim3 grid((unsigned)p.tiles.size()), blk(kGlThreads);
    const GlTile* tiles = (const GlTile*)(ws + p.at.off_tiles);
    const float2* tw = (const float2*)(ws + p.at.off_tw);
    const float* win = (const float*)(ws + p.at.off_win);
    gl_dispatch(gh, [&](auto n, auto h) {
        hipLaunchKernelGGL((gl_stft<decltype(n)::value, decltype(h)::value>), grid, blk, 0, s, tiles, gh.g, tw, win, wav, mag, mel_basis, logmel, energy);
    });
    e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "stft: %s", hipGetErrorString(e));
    return FS2_OK;
}

// Lags of the pitch scan (gl_pitch.h): tmin = floor(sr / f0_ceil), tmax = ceil(sr / f0_floor), 2 <= tmin <= tmax <= win / 2 -- the
// window's autocorrelation is divided by, and beyond half the window it is too small to.  Restated in vocoder.py: pitch_lags.
int gl_pitch_args(const char* who, const GlGeomHost& gh, int32_t sample_rate, double f0_floor, double f0_ceil, double voicing_threshold,
                  double octave_cost, GlPitch& out) {
    if (sample_rate < 1 || !(f0_floor > 0.0) || !(f0_ceil >= f0_floor) || !std::isfinite(f0_ceil) || !std::isfinite(voicing_threshold) ||
        !std::isfinite(octave_cost))
        return fail(nullptr, FS2_ERR_ARG, "%s: sample_rate %d, f0_floor %g, f0_ceil %g, voicing_threshold %g, octave_cost %g", who, sample_rate, f0_floor,
                    f0_ceil, voicing_threshold, octave_cost);
    const double lo = std::floor((double)sample_rate / f0_ceil), hi = std::ceil((double)sample_rate / f0_floor);
    if (lo < 2.0 || hi > gh.win / 2)
        return fail(nullptr, FS2_ERR_UNSUPPORTED,
                    "%s: f0_floor %g .. f0_ceil %g at %d Hz need the lags %.0f .. %.0f, the window of %d samples allows 2 .. %d (lowest usable f0_floor "
                    "%g Hz = 2 sample_rate / win, highest f0_ceil %g Hz)", who, f0_floor, f0_ceil, sample_rate, lo, hi, gh.win, gh.win / 2,
                    2.0 * sample_rate / gh.win, sample_rate / 2.0);
    out.tmin = (int)lo; out.tmax = (int)hi;
    out.sr = (float)sample_rate;
    out.floor_over_sr = (float)(f0_floor / (double)sample_rate);
    out.threshold = (float)voicing_threshold;
    out.octave_cost = (float)octave_cost;
    return FS2_OK;
}

// gl_stft_run with the pitch outputs: the same plan and tables plus the window-autocorrelation table, one gl_features launch.  Without
// f0 and strength it is gl_stft_run (and needs no more workspace than it).
int gl_stft_pitch_run(const char* who, void* stream, const GlGeomHost& gh, const float* wav, int32_t B, const int32_t* wav_starts,
                      const int32_t* wav_lens, void* workspace, size_t workspace_bytes, float* mag, const float* mel_basis, float* logmel, float* energy,
                      int32_t sample_rate, double f0_floor, double f0_ceil, double voicing_threshold, double octave_cost, float* f0, float* strength) {
    GlPitch pp{};
    if (int rc = gl_pitch_args(who, gh, sample_rate, f0_floor, f0_ceil, voicing_threshold, octave_cost, pp)) return rc;
    if (!f0 && !strength) return gl_stft_run(who, stream, gh, wav, B, wav_starts, wav_lens, workspace, workspace_bytes, mag, mel_basis, logmel, energy);
    if (B > 0 && (!wav_starts || !wav_lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
    if (logmel && !mel_basis) return fail(nullptr, FS2_ERR_ARG, "%s: logmel needs mel_basis [%d, %d]", who, gh.n_mels, gh.n_bins);
    GlPlan p;
    if (int rc = gl_plan(B, wav_starts, wav_lens, true, gh, p, true)) return rc;
    if (p.tiles.empty()) return FS2_OK;
    if (!wav || !workspace) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    if (workspace_bytes < p.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, p.at.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    hipError_t e = gl_setup(s, p, gh, ws);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "stft setup: %s", hipGetErrorString(e));
    float* acw = (float*)(ws + p.at.off_acw);
    hipLaunchKernelGGL(gl_pitch_table, dim3((gl_pitch_lags(gh.n_fft) + 7) / 8), dim3(256), 0, s, acw, gh.n_fft, gh.win);
    const dim3 grid((unsigned)p.tiles.size()), blk(kGlThreads);
    const GlTile* tiles = (const GlTile*)(ws + p.at.off_tiles);
    const float2* tw = (const float2*)(ws + p.at.off_tw);
    const float* win = (const float*)(ws + p.at.off_win);
    gl_dispatch(gh, [&](auto n, auto h) {
        hipLaunchKernelGGL((gl_features<decltype(n)::value, decltype(h)::value>), grid, blk, 0, s, tiles, gh.g, tw, win, acw, wav, mag, mel_basis, logmel,
                           energy, pp, f0, strength);
    });
    e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "stft pitch: %s", hipGetErrorString(e));
    return FS2_OK;
}

// ---- SPSI initial phase (kernels and launch sequences: gl_spsi.h): the argument checks behind fs2_op_spsi_phase_geom / _dev ----

// what both forms check of the source first, by the rules of the synthesis (gl_check_synthesis)
int spsi_check_source(const char* who, const GlGeomHost& gh, int32_t src_width, const float* mel_pinv) {
    return gl_check_synthesis(who, gh, src_width, mel_pinv, 0, 0.f);
}

// frames of a host-planned batch (every utterance with L >= 1 is computed), or a failure code (< 0)
int64_t spsi_host_frames(const char* who, const GlGeomHost& gh, int B, const int32_t* starts, const int32_t* lens) {
    if (B < 0 || (B > 0 && !lens)) return fail(nullptr, FS2_ERR_ARG, "%s: bad batch (B = %d)", who, B);
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || (starts && starts[b] < 0)) return fail(nullptr, FS2_ERR_ARG, "%s: negative length / start of utterance %d", who, b);
        if (starts && (int64_t)starts[b] + lens[b] > INT32_MAX / gh.n_bins)
            return fail(nullptr, FS2_ERR_ARG, "%s: utterance %d ends beyond row %d", who, b, INT32_MAX / gh.n_bins);
        rows += lens[b];
        if (rows > INT32_MAX / gh.n_bins) return fail(nullptr, FS2_ERR_ARG, "%s: batch too large (%lld frames)", who, (long long)rows);
    }
    return rows;
}

int spsi_phase_host(const char* who, void* stream, const GlGeomHost& gh, const float* src, int32_t src_width, const float* mel_pinv, int32_t B,
                    const int32_t* starts, const int32_t* lens, void* workspace, size_t workspace_bytes, float* phase, float* mag_out) {
    if (int rc = spsi_check_source(who, gh, src_width, mel_pinv)) return rc;
    if (B > 0 && (!starts || !lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
    const int64_t frames = spsi_host_frames(who, gh, B, starts, lens);
    if (frames < 0) return (int)frames;
    if (frames == 0) return FS2_OK;
    if (!src || !phase || !workspace) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    const SpsiLayout at = spsi_layout(gh.n_bins, B, frames);
    if (workspace_bytes < at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, at.bytes);
    const hipError_t e = spsi_run_host((hipStream_t)stream, gh.n_fft, gh.hop, src, src_width, mel_pinv, B, starts, lens, frames, (char*)workspace, at, phase, mag_out);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return FS2_OK;
}

// the capacities of a device-driven call, by the rules of gl_griffin_lim_dev
bool spsi_caps_ok(const GlGeomHost& gh, int64_t B, int64_t src_stride, int64_t frame_capacity) {
    return B >= 1 && frame_capacity >= 1 && src_stride >= 0 && frame_capacity <= INT32_MAX / gh.n_bins && B * src_stride <= INT32_MAX / gh.n_bins;
}

int spsi_phase_dev(const char* who, void* stream, const GlGeomHost& gh, const float* src, int32_t src_width, const float* mel_pinv, int32_t B,
                   const int64_t* lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status, void* workspace,
                   size_t workspace_bytes, float* phase, float* mag_out) {
    if (int rc = spsi_check_source(who, gh, src_width, mel_pinv)) return rc;
    if (!spsi_caps_ok(gh, B, src_stride, frame_capacity))
        return fail(nullptr, FS2_ERR_ARG, "%s: B %d, frame_capacity %lld, src_stride %d (B >= 1, 1 <= frame_capacity, rows * bins < 2^31)", who, B,
                    (long long)frame_capacity, src_stride);
    if (!src || !lens_dev || !workspace || !phase) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    const SpsiLayout at = spsi_layout(gh.n_bins, B, frame_capacity);
    if (workspace_bytes < at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, at.bytes);
    const hipError_t e = spsi_run_dev((hipStream_t)stream, gh.n_fft, gh.hop, src, src_width, mel_pinv, B, lens_dev, src_stride, frame_capacity, upstream_status,
                                      (char*)workspace, at, phase, mag_out);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return FS2_OK;
}
