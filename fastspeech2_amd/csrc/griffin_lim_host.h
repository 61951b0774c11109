// Host side of the vocoder (kernels: griffin_lim.h, gl_spsi.h, gl_pitch.h, gl_excite.h): one description of a call, GlCall, and one path over it
// (include/fs2.h).
// A GlCall says what the call computes (GlKind), on which transform (GlGeomArgs), for which batch (GlBatch: host-planned or
// device-driven), where it may work (GlWork), from what (GlSource), how it iterates (GlIter) and what it writes (GlWavOut, GlFeatures,
// GlPhaseOut).  Every extern "C" entry point at the end of fs2_runtime.hip only fills one and hands it to gl_call (the calls) or
// gl_workspace_bytes (the queries), which make the geometry first.  The kind alone decides which workspace regions exist and which
// argument checks apply: the mel-constrained call is the plain call with another kind, pitch an optional part of the one analysis.
// A query and the call it sizes go through the same sizing function with the same description -- gl_size (synthesis and analysis:
// gl_plan and gl_layout), spsi_size (SPSI: spsi_layout), exc_size (excitation: exc_layout) -- so they agree by construction.  Only
// the domain differs: a query answers a
// size (or 0) where the call refuses in its own words, so the sizing of a device-driven batch fails without a text and the call gives it.
// The order of the checks is part of the interface (the message names the check that fired): gl_synthesize, gl_analyze,
// spsi_phase and f0_phase each state theirs.
// Not a header of its own: fs2_runtime.hip includes it inside its unnamed namespace, after fail() and align_up(), so the library
// stays one translation unit.

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

// ---- the description of a call: plain aggregates, every part an entry point does not name is zero ----

// What a call computes.  Synthesis projects every iteration onto the fixed M, MelSynthesis onto the magnitudes whose mel is the
// source's (gl_iterate's PROJ = 1; it reads GlSource::mel_basis); Analysis is the STFT with its features, AnalysisPitch adds f0 and
// strength; SpsiPhase is the initial phase of gl_spsi.h (a workspace of its own: spsi_layout); F0Phase the excitation from F0 of
// gl_excite.h with its STFT phase (GlExcite; a workspace of its own: exc_layout; it writes the phase, the waveform, or both).
enum class GlKind { Synthesis, MelSynthesis, Analysis, AnalysisPitch, SpsiPhase, F0Phase };

constexpr bool gl_is_analysis(GlKind k) { return k == GlKind::Analysis || k == GlKind::AnalysisPitch; }

struct GlGeomArgs { int32_t n_fft, hop, win, n_mels; };

// The batch in one of two forms.  Host-planned: starts and lens [B] on the host (synthesis: source rows and frame counts L_b;
// analysis: waveform samples and sample counts T_b; starts may be NULL for a size query).  Device-driven (on_device): the frame counts
// stay on the device, every size comes from the capacities, and upstream_status is the status of the producer of the frames, or NULL.
struct GlBatch {
    bool on_device; int32_t B;
    const int32_t *starts, *lens;
    const int64_t* lens_dev; int32_t src_stride; int64_t frame_capacity; const int32_t* upstream_status;
};

GlBatch gl_host_batch(int32_t B, const int32_t* starts, const int32_t* lens) { return {false, B, starts, lens, nullptr, 0, 0, nullptr}; }

GlBatch gl_device_batch(int32_t B, const int64_t* lens_dev, int32_t src_stride, int64_t frame_capacity, const int32_t* upstream_status) {
    return {true, B, nullptr, nullptr, lens_dev, src_stride, frame_capacity, upstream_status};
}

struct GlWork { void* ptr; size_t bytes; };

// Rows of log-mel (src_width = n_mels, mapped to magnitudes with mel_pinv [bins, n_mels]) or of magnitudes (src_width = bins);
// mel_basis [n_mels, bins]: what MelSynthesis constrains to.  The analysis reads src alone: its packed waveforms.
struct GlSource { const float* src; int32_t src_width; const float *mel_pinv, *mel_basis; };

struct GlIter { int32_t n_iter; float momentum; uint32_t seed; const float* init_phase; };

// wav alone for a host-planned call (packed, sized by the caller from lens); the rest belongs to the device-driven one
struct GlWavOut { float* wav; int32_t wav_stride; int64_t wav_capacity; int64_t* sample_lens_dev; int32_t* status; };

struct GlPitchOptions { int32_t sample_rate; double f0_floor, f0_ceil, voicing_threshold, octave_cost; };

// Outputs of the analysis, each optional; logmel needs mel_basis; pitch, f0 and strength belong to AnalysisPitch, and so do the
// candidates (n_cands = 0: the winner's f0 and strength; 1 .. FS2_PITCH_MAX_CANDS: cand_f0 and cand_strength [frames, n_cands])
struct GlFeatures {
    float* mag; const float* mel_basis; float *logmel, *energy; GlPitchOptions pitch; float *f0, *strength;
    int32_t n_cands; float *cand_f0, *cand_strength;
};

struct GlPhaseOut { float *phase, *mag_out; };

// F0Phase: one f0 per source row (Hz), which frames count as voiced, the rate the samples are spaced at
struct GlExcite { const float* f0; double f0_floor, f0_ceil; int32_t sample_rate; };

// who: the entry point, for the messages.  gh: made from geom by gl_call / gl_workspace_bytes before anything else is looked at.
struct GlCall {
    const char* who; GlKind kind; GlGeomArgs geom; GlBatch batch; GlWork work; GlSource source; GlIter iter; GlWavOut out;
    GlFeatures feat; GlPhaseOut spsi; GlGeomHost gh; GlExcite exc;
};

// ---- sizing of the synthesis and the analysis ----

// Their workspace: tables, tile records, the device planner's per-utterance arrays (device-driven call only), then (synthesis only)
// M, the two spectrum buffers and the momentum state over `frames` frames packed back to back, then (AnalysisPitch only) the
// window-autocorrelation table of gl_pitch.h, then (MelSynthesis only) the band tables of gl_band_tables.  Each region starts
// 256-byte aligned.
struct GlLayout {
    size_t off_tw = 0, off_win = 0, off_tiles = 0, off_plan = 0, off_M = 0, off_C0 = 0, off_C1 = 0, off_T = 0, off_acw = 0, off_band = 0, bytes = 0;
};

// records: tile records (the exact tile count of a host plan, the slots of a device-driven call); planner_B: utterances the device
// planner keeps its 4 ints each for, < 0: a host-planned call, no such region.  0 records / 0 utterances still reserve one.
GlLayout gl_layout(const GlGeomHost& gh, GlKind kind, size_t records, int64_t planner_B, int64_t frames) {
    GlLayout l;
    size_t off = 0;
    auto take = [&](size_t n) { off = align_up(off, 256); size_t o = off; off += n; return o; };
    l.off_tw = take(gh.n_fft * sizeof(float2));
    l.off_win = take(gh.n_fft * sizeof(float));
    l.off_tiles = take(std::max<size_t>(records, 1) * sizeof(GlTile));
    if (planner_B >= 0) l.off_plan = take(std::max<size_t>((size_t)planner_B, 1) * 4 * sizeof(int));
    if (!gl_is_analysis(kind)) {
        const size_t n = (size_t)frames * gh.n_bins;
        l.off_M = take(n * sizeof(float));
        l.off_C0 = take(n * sizeof(float2));
        l.off_C1 = take(n * sizeof(float2));
        l.off_T = take(n * sizeof(float2));
    }
    if (kind == GlKind::AnalysisPitch) l.off_acw = take(gl_pitch_lags(gh.n_fft) * sizeof(float));
    if (kind == GlKind::MelSynthesis) l.off_band = take(gl_band_bytes(gh.n_bins));
    l.bytes = align_up(off, 256);
    return l;
}

// What a call launches over: `records` workgroups (= tile records) and the workspace laid out for them.  tiles: the exact tile list of
// a host-planned batch (the planner kernels write the records of a device-driven one).
struct GlPlan {
    std::vector<GlTile> tiles;
    size_t records = 0;
    int64_t frames = 0, samples = 0;
    GlLayout at;
};

// Host plan.  Synthesis: lens are frame counts L_b, samples hop max(L_b - 1, 0), tiles cover the utterances with L_b >= 2 (they own
// samples).  Analysis: lens are sample counts T_b, frames T_b / hop + 1, tiles cover every utterance with frames.
int gl_plan(const GlCall& c, GlPlan& p) {
    const int B = c.batch.B;
    const int32_t *starts = c.batch.starts, *lens = c.batch.lens;
    const bool analysis = gl_is_analysis(c.kind);
    if (B < 0 || (B > 0 && !lens)) return fail(nullptr, FS2_ERR_ARG, "vocoder: bad batch (B = %d)", B);
    const int hop = c.gh.hop, F = c.gh.g.F, nb = c.gh.n_bins;
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
    p.records = p.tiles.size();
    p.frames = row;
    p.samples = wav;
    p.at = gl_layout(c.gh, c.kind, p.records, -1, p.frames);
    return FS2_OK;
}

// Workgroups (= tile records) of a device-driven call of B utterances inside frame_capacity (gl_slot_rule.h), or -1: the
// capacities are negative or too large for one call.
int64_t gl_cap_slots(const GlGeomHost& gh, int64_t B, int64_t frame_capacity) {
    if (B < 0 || frame_capacity < 0 || frame_capacity > INT32_MAX / gh.n_bins) return -1;
    const int64_t slots = gl_slot_capacity(frame_capacity, gh.g.F, (int)B);
    return slots > INT32_MAX ? -1 : slots;
}

// The one sizing of the synthesis and the analysis, for the queries and the calls alike.  A host-planned batch is planned, and fails
// with the plan's message.  A device-driven one has the layout of a host plan with every size taken from the capacities (gl_cap_slots
// records, frame_capacity frames) plus the planner's per-utterance arrays; capacities out of range fail WITHOUT a message: the query
// answers 0 and the call says it in its own words.  (B = 0, capacity 0 is a size here; the call refuses B < 1 before it asks.)
int gl_size(const GlCall& c, GlPlan& p) {
    if (!c.batch.on_device) return gl_plan(c, p);
    const int64_t slots = gl_cap_slots(c.gh, c.batch.B, c.batch.frame_capacity);
    if (slots < 0) return FS2_ERR_ARG;
    p.records = (size_t)slots;
    p.frames = c.batch.frame_capacity;
    p.at = gl_layout(c.gh, c.kind, p.records, c.batch.B, p.frames);
    return FS2_OK;
}

// ---- launches ----

void gl_put_tables(hipStream_t s, const GlGeomHost& gh, const GlLayout& at, char* ws) {
    hipLaunchKernelGGL(gl_tables, dim3((gh.n_fft + 255) / 256), dim3(256), 0, s, (float2*)(ws + at.off_tw), (float*)(ws + at.off_win),
                       gh.n_fft, gh.win);
}

// tables + tile records of a host plan into the workspace (kernel arguments, no host copy)
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

static_assert(kGlOvfRows == FS2_OVF_ROWS && kGlOvfLmax == FS2_OVF_LMAX && kGlOvfUpstream == FS2_OVF_UPSTREAM && kGlOvfNegative == FS2_OVF_NEG_LEN &&
              kGlOvfWav == FS2_OVF_WAV, "griffin_lim.h restates the FS2_OVF_* bits");

// tables, then the planner kernels of a device-driven call: they write the tile records, sample_lens and status, and fill the wav
hipError_t gl_setup_on_device(hipStream_t s, const GlCall& c, const GlPlan& p, char* ws) {
    const GlBatch& b = c.batch;
    const GlWavOut& o = c.out;
    gl_put_tables(s, c.gh, p.at, ws);
    GlPlanArgs pa{};
    pa.lens = b.lens_dev; pa.upstream = b.upstream_status;
    pa.B = b.B; pa.hop = c.gh.hop; pa.F = c.gh.g.F;
    pa.src_stride = b.src_stride; pa.wav_stride = o.wav_stride;
    pa.frame_capacity = b.frame_capacity; pa.wav_capacity = o.wav_capacity;
    int* plan = (int*)(ws + p.at.off_plan);
    pa.row0 = plan; pa.wav0 = plan + b.B; pa.tile_end = plan + 2 * (size_t)b.B; pa.Lv = plan + 3 * (size_t)b.B;
    pa.sample_lens = o.sample_lens_dev; pa.status = o.status;
    const int n_slots = (int)p.records;          // >= B >= 1
    hipLaunchKernelGGL(gl_plan_scan, dim3(1), dim3(kGlPlanThreads), 0, s, pa);
    hipLaunchKernelGGL(gl_plan_emit, dim3((n_slots + 255) / 256), dim3(256), 0, s, pa, n_slots, (GlTile*)(ws + p.at.off_tiles));
    if (o.wav_capacity > 0)
        hipLaunchKernelGGL(gl_plan_fill, dim3((unsigned)std::min<int64_t>((o.wav_capacity + 1023) / 1024, 2048)), dim3(256), 0, s, pa, o.wav);
    return hipGetLastError();
}

// prologue, n_iter fused iterations and the final ISTFT of one geometry (NFFT; HOP_C = 256: the default instantiation) over the
// tile records in place in ws: uploaded, or being written by the planner ahead on the stream
template <int NFFT, int HOP_C>
hipError_t gl_run(hipStream_t s, const GlCall& c, const GlPlan& p, char* ws) {
    // The instantiations of gl_iterate at this geometry, stated once: the iteration by [projection][momentum], and the final ISTFT.
    using Iterate = decltype(&gl_iterate<NFFT, HOP_C, 0, false, 0>);
    const Iterate iterate[2][2] = {{gl_iterate<NFFT, HOP_C, 0, false, 0>, gl_iterate<NFFT, HOP_C, 0, true, 0>},
                                   {gl_iterate<NFFT, HOP_C, 0, false, 1>, gl_iterate<NFFT, HOP_C, 0, true, 1>}};
    const Iterate final_istft = gl_iterate<NFFT, HOP_C, 1, false>;
    const GlGeomHost& gh = c.gh;
    const GlSource& in = c.source;
    const GlLayout& at = p.at;
    const int n_iter = c.iter.n_iter, proj = c.kind == GlKind::MelSynthesis;
    const float momentum = c.iter.momentum, beta = momentum / (1.f + momentum);
    const GlTile* tiles = (const GlTile*)(ws + at.off_tiles);
    const float2* tw = (const float2*)(ws + at.off_tw);
    const float* win = (const float*)(ws + at.off_win);
    float* M = (float*)(ws + at.off_M);
    float2* C[2] = {(float2*)(ws + at.off_C0), (float2*)(ws + at.off_C1)};
    float2* Tm = momentum > 0.f ? (float2*)(ws + at.off_T) : nullptr;
    GlMelProj mp{};                 // all zero for PROJ = 0
    if (proj) {                     // the layout has the band region; src is the call's log-mel source
        mp.mel = in.src;
        mp.basis = in.mel_basis;
        mp.row_rng = (const int2*)(ws + at.off_band);
        mp.bin_rng = mp.row_rng + kGlMaxMels;
        mp.inv_w = (const float*)(mp.bin_rng + gh.n_bins);
        mp.band = mp.inv_w + gh.n_bins;
    }
    const dim3 grid((unsigned)p.records), blk(kGlThreads);
    const GlGeom g = gh.g;
    const size_t lds = gh.sig_bytes;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (lds && hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    // Set on every eager call, not once per instantiation: the byte count follows the hop (<1024, 0> at hop 200 and at hop 300
    // differ).  Host work only, skipped while capturing: a captured call relies on the eager call before it, which is why every plain
    // instantiation gets it and not only the one this call launches (capture with momentum after an eager call without); the
    // mel-constrained ones get it on a mel-constrained call.
    if (lds && cap == hipStreamCaptureStatusNone) {
        for (const Iterate k : {iterate[0][0], iterate[0][1], final_istft})
            if (hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); e != hipSuccess) return e;
        if (proj)
            for (const Iterate k : {iterate[1][0], iterate[1][1]})
                if (hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); e != hipSuccess) return e;
    }
    if (in.src_width == 80 && gh.n_mels == 80 && in.src_width != gh.n_bins)
        hipLaunchKernelGGL((gl_prologue<NFFT, 80>), grid, blk, 0, s, tiles, g, in.src, in.src_width, in.mel_pinv, c.iter.init_phase, c.iter.seed, M, C[0], Tm);
    else
        hipLaunchKernelGGL((gl_prologue<NFFT, 0>), grid, blk, 0, s, tiles, g, in.src, in.src_width, in.mel_pinv, c.iter.init_phase, c.iter.seed, M, C[0], Tm);
    if (proj && n_iter > 0)         // the band tables of this call's basis, read by the iterations only
        hipLaunchKernelGGL(gl_band_tables, dim3((gh.n_bins + kGlThreads - 1) / kGlThreads), blk, 0, s, mp.basis, gh.n_mels, gh.n_bins,
                           const_cast<int2*>(mp.row_rng), const_cast<int2*>(mp.bin_rng), const_cast<float*>(mp.inv_w), const_cast<float*>(mp.band));
    const Iterate step = iterate[proj][Tm != nullptr];
    for (int i = 0; i < n_iter; ++i)
        hipLaunchKernelGGL(step, grid, blk, lds, s, tiles, g, tw, win, M, C[i & 1], C[(i + 1) & 1], Tm, beta, c.out.wav, mp);
    const GlMelProj none{};
    hipLaunchKernelGGL((gl_iterate<NFFT, HOP_C, 1, false>), grid, blk, lds, s, tiles, g, tw, win, M, C[n_iter & 1], C[(n_iter + 1) & 1], nullptr, 0.f, c.out.wav, none);
    return hipGetLastError();
}

// ---- the synthesis ----

// What every synthesis, and SPSI (whose GlIter is zero), checks first, in this order.  MelSynthesis has no use for a magnitude source
// and needs the basis.
int gl_check_synthesis(const GlCall& c) {
    const char* who = c.who;
    const GlGeomHost& gh = c.gh;
    const int32_t src_width = c.source.src_width, n_iter = c.iter.n_iter;
    const float momentum = c.iter.momentum;
    const bool mel_proj = c.kind == GlKind::MelSynthesis;
    if (src_width != gh.n_mels && src_width != gh.n_bins)
        return fail(nullptr, FS2_ERR_UNSUPPORTED, "%s: src_width %d (%d mel bins or %d linear bins of the %d-point STFT)", who, src_width, gh.n_mels,
                    gh.n_bins, gh.n_fft);
    if (src_width != gh.n_bins && !c.source.mel_pinv) return fail(nullptr, FS2_ERR_ARG, "%s: mel input needs mel_pinv [%d, %d]", who, gh.n_bins, gh.n_mels);
    if (n_iter < 0 || !(momentum >= 0.f) || !std::isfinite(momentum)) return fail(nullptr, FS2_ERR_ARG, "%s: n_iter %d, momentum %g", who, n_iter, momentum);
    if (mel_proj && src_width != gh.n_mels)
        return fail(nullptr, FS2_ERR_ARG, "%s: src_width %d is a magnitude source: there is no mel to constrain to (%d mel bins)", who, src_width, gh.n_mels);
    if (mel_proj && !c.source.mel_basis) return fail(nullptr, FS2_ERR_ARG, "%s: null mel_basis [%d, %d]", who, gh.n_mels, gh.n_bins);
    return FS2_OK;
}

// The capacities and pointers of a device-driven synthesis, in the order its messages are known by
int gl_check_device_batch(const GlCall& c) {
    const char* who = c.who;
    const GlBatch& b = c.batch;
    const GlWavOut& o = c.out;
    if (b.B < 1 || b.frame_capacity < 1 || b.src_stride < 0 || o.wav_stride < 0)
        return fail(nullptr, FS2_ERR_ARG, "%s: B %d, frame_capacity %lld, src_stride %d, wav_stride %d", who, b.B, (long long)b.frame_capacity, b.src_stride,
                    o.wav_stride);
    if (b.frame_capacity > INT32_MAX / c.gh.n_bins || o.wav_capacity < 0 || o.wav_capacity > INT32_MAX || (int64_t)b.B * b.src_stride > INT32_MAX)
        return fail(nullptr, FS2_ERR_ARG, "%s: capacities too large for one call (%lld frames, %lld samples)", who, (long long)b.frame_capacity,
                    (long long)o.wav_capacity);
    if ((int64_t)b.B * o.wav_stride > o.wav_capacity)
        return fail(nullptr, FS2_ERR_ARG, "%s: padded output of %d x %d samples in a wav of %lld", who, b.B, o.wav_stride, (long long)o.wav_capacity);
    if (!c.source.src || !b.lens_dev || !c.work.ptr || !o.sample_lens_dev || !o.status || (o.wav_capacity > 0 && !o.wav))
        return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    return FS2_OK;
}

// Synthesis and MelSynthesis, host-planned and device-driven.  Order of the checks -- host-planned: source and iteration arguments,
// null starts / lens, the plan, "nobody owns a sample" (FS2_OK before any pointer is looked at), null pointers; device-driven: source
// and iteration arguments, capacities, null pointers, the slots; for both the workspace last.
int gl_synthesize(hipStream_t s, const GlCall& c) {
    const char* who = c.who;
    const bool on_device = c.batch.on_device;
    if (int rc = gl_check_synthesis(c)) return rc;
    GlPlan p;
    if (on_device) {
        if (int rc = gl_check_device_batch(c)) return rc;
        if (gl_size(c, p)) return fail(nullptr, FS2_ERR_ARG, "%s: capacities too large for one call", who);
    } else {
        if (c.batch.B > 0 && (!c.batch.starts || !c.batch.lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
        if (int rc = gl_size(c, p)) return rc;
        if (p.tiles.empty()) return FS2_OK;
        if (!c.source.src || !c.out.wav || !c.work.ptr) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    }
    if (c.work.bytes < p.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, c.work.bytes, p.at.bytes);
    char* ws = (char*)c.work.ptr;
    hipError_t e = on_device ? gl_setup_on_device(s, c, p, ws) : gl_setup(s, p, c.gh, ws);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "griffin_lim %s: %s", on_device ? "plan" : "setup", hipGetErrorString(e));
    e = gl_dispatch(c.gh, [&](auto n, auto h) { return gl_run<decltype(n)::value, decltype(h)::value>(s, c, p, ws); });
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "griffin_lim: %s", hipGetErrorString(e));
    return FS2_OK;
}

// ---- the analysis ----

// Lags of the pitch scan (gl_pitch.h): tmin = floor(sr / f0_ceil), tmax = ceil(sr / f0_floor), 2 <= tmin <= tmax <= win / 2 -- the
// window's autocorrelation is divided by, and beyond half the window it is too small to.  Restated in vocoder.py: pitch_lags.
int gl_pitch_args(const char* who, const GlGeomHost& gh, const GlPitchOptions& o, GlPitch& out) {
    if (o.sample_rate < 1 || !(o.f0_floor > 0.0) || !(o.f0_ceil >= o.f0_floor) || !std::isfinite(o.f0_ceil) || !std::isfinite(o.voicing_threshold) ||
        !std::isfinite(o.octave_cost))
        return fail(nullptr, FS2_ERR_ARG, "%s: sample_rate %d, f0_floor %g, f0_ceil %g, voicing_threshold %g, octave_cost %g", who, o.sample_rate, o.f0_floor,
                    o.f0_ceil, o.voicing_threshold, o.octave_cost);
    const double lo = std::floor((double)o.sample_rate / o.f0_ceil), hi = std::ceil((double)o.sample_rate / o.f0_floor);
    if (lo < 2.0 || hi > gh.win / 2)
        return fail(nullptr, FS2_ERR_UNSUPPORTED,
                    "%s: f0_floor %g .. f0_ceil %g at %d Hz need the lags %.0f .. %.0f, the window of %d samples allows 2 .. %d (lowest usable f0_floor "
                    "%g Hz = 2 sample_rate / win, highest f0_ceil %g Hz)", who, o.f0_floor, o.f0_ceil, o.sample_rate, lo, hi, gh.win, gh.win / 2,
                    2.0 * o.sample_rate / gh.win, o.sample_rate / 2.0);
    out.tmin = (int)lo; out.tmax = (int)hi;
    out.sr = (float)o.sample_rate;
    out.floor_over_sr = (float)(o.f0_floor / (double)o.sample_rate);
    out.threshold = (float)o.voicing_threshold;
    out.octave_cost = (float)o.octave_cost;
    return FS2_OK;
}

// Analysis and AnalysisPitch: one gl_stft launch, or with the pitch outputs the window-autocorrelation table and one gl_features
// launch (gl_candidates where the call asks for candidates).  Order of the checks: the pitch options and the candidate count
// (AnalysisPitch; without f0 and strength, or their candidate forms, it is then exactly Analysis and needs no more workspace than it), null starts / lens, logmel without its basis, the plan, nothing to do (FS2_OK before any pointer is looked
// at), null pointers, the workspace last.
int gl_analyze(hipStream_t s, GlCall c) {
    const char* who = c.who;
    const GlGeomHost& gh = c.gh;
    const GlFeatures& o = c.feat;
    GlPitch pp{};
    if (c.kind == GlKind::AnalysisPitch) {
        if (int rc = gl_pitch_args(who, gh, o.pitch, pp)) return rc;
        if (o.n_cands < 0 || o.n_cands > FS2_PITCH_MAX_CANDS || (o.n_cands == 0 && (o.cand_f0 || o.cand_strength)))
            return fail(nullptr, FS2_ERR_ARG, "%s: n_candidates = %d outside 1 .. %d", who, o.n_cands, FS2_PITCH_MAX_CANDS);
        if (o.n_cands ? !o.cand_f0 && !o.cand_strength : !o.f0 && !o.strength) c.kind = GlKind::Analysis;
    }
    const bool pitch = c.kind == GlKind::AnalysisPitch;
    if (c.batch.B > 0 && (!c.batch.starts || !c.batch.lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
    if (o.logmel && !o.mel_basis) return fail(nullptr, FS2_ERR_ARG, "%s: logmel needs mel_basis [%d, %d]", who, gh.n_mels, gh.n_bins);
    GlPlan p;
    if (int rc = gl_size(c, p)) return rc;
    if (p.tiles.empty() || (!pitch && !o.mag && !o.logmel && !o.energy)) return FS2_OK;
    const float* wav = c.source.src;
    if (!wav || !c.work.ptr) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    if (c.work.bytes < p.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, c.work.bytes, p.at.bytes);
    char* ws = (char*)c.work.ptr;
    hipError_t e = gl_setup(s, p, gh, ws);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "stft setup: %s", hipGetErrorString(e));
    float* acw = (float*)(ws + p.at.off_acw);
    if (pitch) hipLaunchKernelGGL(gl_pitch_table, dim3((gl_pitch_lags(gh.n_fft) + 7) / 8), dim3(256), 0, s, acw, gh.n_fft, gh.win);
    const dim3 grid((unsigned)p.records), blk(kGlThreads);
    const GlTile* tiles = (const GlTile*)(ws + p.at.off_tiles);
    const float2* tw = (const float2*)(ws + p.at.off_tw);
    const float* win = (const float*)(ws + p.at.off_win);
    gl_dispatch(gh, [&](auto n, auto h) {
        constexpr int NFFT = decltype(n)::value, HOP_C = decltype(h)::value;
        if (pitch && o.n_cands) {
            // |X|, log-mel and energy beside candidates come from gl_stft itself, in a launch of its own: their bits are fs2_op_stft_geom's
            // by construction (gl_candidates' own copy of those statements was measured to differ in the last bit at n_fft = 2048: the
            // compiler contracts the transform differently there), and gl_candidates then skips that part of its body
            if (o.mag || o.logmel || o.energy)
                hipLaunchKernelGGL((gl_stft<NFFT, HOP_C>), grid, blk, 0, s, tiles, gh.g, tw, win, wav, o.mag, o.mel_basis, o.logmel, o.energy);
            hipLaunchKernelGGL((gl_candidates<NFFT, HOP_C>), grid, blk, 0, s, tiles, gh.g, tw, win, acw, wav, (float*)nullptr, o.mel_basis, (float*)nullptr,
                               (float*)nullptr, pp, o.n_cands, o.cand_f0, o.cand_strength);
        } else if (pitch)
            hipLaunchKernelGGL((gl_features<NFFT, HOP_C>), grid, blk, 0, s, tiles, gh.g, tw, win, acw, wav, o.mag, o.mel_basis, o.logmel, o.energy, pp, o.f0,
                               o.strength);
        else
            hipLaunchKernelGGL((gl_stft<NFFT, HOP_C>), grid, blk, 0, s, tiles, gh.g, tw, win, wav, o.mag, o.mel_basis, o.logmel, o.energy);
    });
    e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "%s: %s", pitch ? "stft pitch" : "stft", hipGetErrorString(e));
    return FS2_OK;
}

// ---- SPSI initial phase (kernels and launch sequences: gl_spsi.h) ----

// frames of a host-planned batch (every utterance with L >= 1 is computed), or a failure code (< 0)
int64_t spsi_host_frames(const GlCall& c) {
    const char* who = c.who;
    const int B = c.batch.B, rows_max = INT32_MAX / c.gh.n_bins;
    const int32_t *starts = c.batch.starts, *lens = c.batch.lens;
    if (B < 0 || (B > 0 && !lens)) return fail(nullptr, FS2_ERR_ARG, "%s: bad batch (B = %d)", who, B);
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || (starts && starts[b] < 0)) return fail(nullptr, FS2_ERR_ARG, "%s: negative length / start of utterance %d", who, b);
        if (starts && (int64_t)starts[b] + lens[b] > rows_max) return fail(nullptr, FS2_ERR_ARG, "%s: utterance %d ends beyond row %d", who, b, rows_max);
        rows += lens[b];
        if (rows > rows_max) return fail(nullptr, FS2_ERR_ARG, "%s: batch too large (%lld frames)", who, (long long)rows);
    }
    return rows;
}

// the capacities of a device-driven call, by the rules of the device-driven synthesis
bool spsi_caps_ok(const GlGeomHost& gh, int64_t B, int64_t src_stride, int64_t frame_capacity) {
    return B >= 1 && frame_capacity >= 1 && src_stride >= 0 && frame_capacity <= INT32_MAX / gh.n_bins && B * src_stride <= INT32_MAX / gh.n_bins;
}

struct SpsiSize {
    int64_t frames = 0;
    SpsiLayout at;
};

// The one sizing of SPSI, for the queries and the calls alike: the frames of a host-planned batch (failing with their message) or
// the capacity of a device-driven one (out of range: no message, as in gl_size; B = 0 is no size here), and spsi_layout over them.
int spsi_size(const GlCall& c, SpsiSize& z) {
    const GlBatch& b = c.batch;
    if (b.on_device && !spsi_caps_ok(c.gh, b.B, b.src_stride, b.frame_capacity)) return FS2_ERR_ARG;
    z.frames = b.on_device ? b.frame_capacity : spsi_host_frames(c);
    if (z.frames < 0) return (int)z.frames;
    z.at = spsi_layout(c.gh.n_bins, b.B, z.frames);
    return FS2_OK;
}

// Order of the checks: the source, by the rules of the synthesis; then host-planned: null starts / lens, the frames, no frames
// (FS2_OK before any pointer is looked at), null pointers; device-driven: the capacities, null pointers; for both the workspace last.
int spsi_phase(hipStream_t s, const GlCall& c) {
    const char* who = c.who;
    const GlGeomHost& gh = c.gh;
    const GlSource& in = c.source;
    const GlBatch& b = c.batch;
    if (int rc = gl_check_synthesis(c)) return rc;
    SpsiSize z;
    if (b.on_device) {
        if (spsi_size(c, z))
            return fail(nullptr, FS2_ERR_ARG, "%s: B %d, frame_capacity %lld, src_stride %d (B >= 1, 1 <= frame_capacity, rows * bins < 2^31)", who, b.B,
                        (long long)b.frame_capacity, b.src_stride);
        if (!in.src || !b.lens_dev || !c.work.ptr || !c.spsi.phase) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    } else {
        if (b.B > 0 && (!b.starts || !b.lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
        if (int rc = spsi_size(c, z)) return rc;
        if (z.frames == 0) return FS2_OK;
        if (!in.src || !c.spsi.phase || !c.work.ptr) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    }
    if (c.work.bytes < z.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, c.work.bytes, z.at.bytes);
    char* ws = (char*)c.work.ptr;
    const hipError_t e = b.on_device ? spsi_run_dev(s, gh.n_fft, gh.hop, in.src, in.src_width, in.mel_pinv, b.B, b.lens_dev, b.src_stride, b.frame_capacity,
                                                    b.upstream_status, ws, z.at, c.spsi.phase, c.spsi.mag_out)
                                     : spsi_run_host(s, gh.n_fft, gh.hop, in.src, in.src_width, in.mel_pinv, b.B, b.starts, b.lens, z.frames, ws, z.at,
                                                     c.spsi.phase, c.spsi.mag_out);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return FS2_OK;
}

// ---- excitation from F0 and its phase (kernels and launch sequences: gl_excite.h) ----

struct ExcSize {
    int64_t frames = 0;
    ExcLayout at;
};

// The one sizing of F0Phase, for the queries and the calls alike, by the rules of spsi_size; on top of them the samples, hop per
// frame, must index with an int.
int exc_size(const GlCall& c, ExcSize& z) {
    const GlBatch& b = c.batch;
    if (b.on_device && !spsi_caps_ok(c.gh, b.B, b.src_stride, b.frame_capacity)) return FS2_ERR_ARG;
    z.frames = b.on_device ? b.frame_capacity : spsi_host_frames(c);
    if (z.frames < 0) return (int)z.frames;
    if (z.frames * c.gh.hop > INT32_MAX) return b.on_device ? FS2_ERR_ARG : fail(nullptr, FS2_ERR_ARG, "%s: batch too large (%lld frames)", c.who, (long long)z.frames);
    z.at = exc_layout(c.gh.n_fft, c.gh.hop, b.B, z.frames);
    return FS2_OK;
}

// Order of the checks: the options; then host-planned: null starts / lens, the frames, no frames (FS2_OK before any pointer is
// looked at), null pointers; device-driven: the capacities, null pointers; for both the workspace last.
int f0_phase(hipStream_t s, const GlCall& c) {
    const char* who = c.who;
    const GlGeomHost& gh = c.gh;
    const GlBatch& b = c.batch;
    const GlExcite& x = c.exc;
    const GlWavOut& w = c.out;
    if (x.sample_rate < 1 || !(x.f0_floor > 0.0) || !(x.f0_ceil >= x.f0_floor) || !std::isfinite(x.f0_ceil))
        return fail(nullptr, FS2_ERR_ARG, "%s: sample_rate %d, f0_floor %g, f0_ceil %g (sample_rate >= 1, 0 < f0_floor <= f0_ceil, finite)", who, x.sample_rate,
                    x.f0_floor, x.f0_ceil);
    ExcSize z;
    if (b.on_device) {
        if (exc_size(c, z) || w.wav_stride < 0 || w.wav_capacity < 0 || w.wav_capacity > INT32_MAX || (int64_t)b.B * w.wav_stride > w.wav_capacity)
            return fail(nullptr, FS2_ERR_ARG,
                        "%s: B %d, frame_capacity %lld, src_stride %d, wav_stride %d, wav_capacity %lld (B >= 1, 1 <= frame_capacity, rows * bins < 2^31, "
                        "hop * frame_capacity < 2^31, B * wav_stride <= wav_capacity < 2^31)", who, b.B, (long long)b.frame_capacity, b.src_stride, w.wav_stride,
                        (long long)w.wav_capacity);
        if (!x.f0 || !b.lens_dev || !c.work.ptr || (!c.spsi.phase && !w.wav)) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    } else {
        if (b.B > 0 && (!b.starts || !b.lens)) return fail(nullptr, FS2_ERR_ARG, "%s: null starts / lens", who);
        if (int rc = exc_size(c, z)) return rc;
        if (z.frames == 0) return FS2_OK;
        if (!x.f0 || !c.work.ptr || (!c.spsi.phase && !w.wav)) return fail(nullptr, FS2_ERR_ARG, "%s: null pointer", who);
    }
    if (c.work.bytes < z.at.bytes) return fail(nullptr, FS2_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, c.work.bytes, z.at.bytes);
    char* ws = (char*)c.work.ptr;
    const ExcOptions o{x.f0_floor, x.f0_ceil, (double)x.sample_rate, c.iter.seed, gh.hop};
    const hipError_t e = b.on_device ? exc_run_dev(s, gh.n_fft, gh.win, o, x.f0, b.B, b.lens_dev, b.src_stride, b.frame_capacity, b.upstream_status, ws, z.at,
                                                   w.wav, w.wav_stride, w.wav_capacity, c.spsi.phase)
                                     : exc_run_host(s, gh.n_fft, gh.win, o, x.f0, b.B, b.starts, b.lens, z.frames, ws, z.at, w.wav, c.spsi.phase);
    if (e != hipSuccess) return fail(nullptr, FS2_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return FS2_OK;
}

// ---- the one path ----

int gl_call(void* stream, GlCall c) {
    if (int rc = gl_geom(c.geom.n_fft, c.geom.hop, c.geom.win, c.geom.n_mels, c.who, c.gh)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (c.kind == GlKind::SpsiPhase) return spsi_phase(s, c);
    if (c.kind == GlKind::F0Phase) return f0_phase(s, c);
    return gl_is_analysis(c.kind) ? gl_analyze(s, c) : gl_synthesize(s, c);
}

// the workspace gl_call needs for the same description (only kind, geometry and batch are read), 0 on every failure
size_t gl_workspace_bytes(GlCall c) {
    GlPlan p;
    SpsiSize z;
    ExcSize x;
    if (gl_geom(c.geom.n_fft, c.geom.hop, c.geom.win, c.geom.n_mels, c.who, c.gh)) return 0;
    if (c.kind == GlKind::SpsiPhase) return spsi_size(c, z) == FS2_OK ? z.at.bytes : 0;
    if (c.kind == GlKind::F0Phase) return exc_size(c, x) == FS2_OK ? x.at.bytes : 0;
    return gl_size(c, p) == FS2_OK ? p.at.bytes : 0;
}
