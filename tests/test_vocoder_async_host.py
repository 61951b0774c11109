"""Host side of the device-driven Griffin-Lim (fs2_op_griffin_lim_dev, fs2_op_vocode_workspace_bytes_cap): the
entry points exist, the capacity workspace bounds the exact one, the planner's slot -> tile rule (csrc/gl_slot_rule.h, compiled here
with the host compiler) equals its numpy restatement and the host plan's tile list, and the argument checks of ``sync=False`` that
need no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")
GEOMS = [(1024, 256, 1024), (2048, 300, 1200), (512, 160, 400), (1024, 200, 800)]


@pytest.fixture(scope="module")
def lib():
    from fastspeech2_amd import _lib
    _lib.build()
    return _lib.lib()


def test_entry_points_are_declared_and_bound():
    from fastspeech2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fs2.h")).read()
    declared = set(re.findall(r"\b(fs2_[a-z_0-9]+)\s*\(", hdr))
    for name in ("fs2_op_vocode_workspace_bytes_cap", "fs2_op_griffin_lim_dev"):
        assert name in declared and name in _lib.EXPORTS, name
    flags = {n: int(v) for n, v in re.findall(r"#define (FS2_OVF_[A-Z_]+) (\d+)", hdr)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values()), flags     # distinct single bits
    import fastspeech2_amd
    assert fastspeech2_amd.AsyncWaveforms is fastspeech2_amd.vocoder.AsyncWaveforms


def _splits(total, B, rng):
    """Length lists with sum <= total: everything in one utterance, spread evenly, B - 1 single frames plus one long, random."""
    yield [total] + [0] * (B - 1)
    yield [total // B] * B
    if total >= B:
        yield [1] * (B - 1) + [total - (B - 1)]
    for _ in range(60):
        cuts = np.sort(rng.integers(0, total + 1, size=B))
        yield np.diff(np.concatenate([[0], cuts])).tolist()


@pytest.mark.parametrize("geom", GEOMS)
def test_capacity_workspace_bounds_the_exact_one(lib, geom):
    n_fft, hop, win = geom
    rng = np.random.default_rng(n_fft + hop)
    n = 0
    for B, total in [(1, 1), (1, 997), (3, 40), (11, 1100), (64, 5000), (256, 35600), (1000, 1000), (1000, 999)]:
        cap = int(lib.fs2_op_vocode_workspace_bytes_cap(n_fft, hop, win, 80, B, total))
        assert cap > 0
        for lens in _splits(total, B, rng):
            assert len(lens) == B and sum(lens) <= total and min(lens) >= 0
            arr = (C.c_int32 * B)(*lens)
            exact = int(lib.fs2_op_vocode_workspace_bytes_geom(n_fft, hop, win, 80, B, arr))
            assert 0 < exact <= cap, (B, total, lens[:8], exact, cap)
            n += 1
    assert n >= 400
    # a capacity above the batch's frames is a bound too, and the query is monotone in it
    assert int(lib.fs2_op_vocode_workspace_bytes_cap(n_fft, hop, win, 80, 11, 2200)) >= int(lib.fs2_op_vocode_workspace_bytes_cap(n_fft, hop, win, 80, 11, 1100))


def test_capacity_workspace_rejects_what_the_geom_query_rejects(lib):
    q = lib.fs2_op_vocode_workspace_bytes_cap
    assert q(1024, 256, 1024, 80, 4, 100) > 0
    assert q(1000, 256, 1000, 80, 4, 100) == 0          # n_fft
    assert q(1024, 100, 1024, 80, 4, 100) == 0          # ceil(n_fft / hop) > 8
    assert q(1024, 512, 256, 80, 4, 100) == 0           # hop > win
    assert q(1024, 256, 2048, 80, 4, 100) == 0          # win > n_fft
    assert q(1024, 256, 1024, 0, 4, 100) == 0 and q(1024, 256, 1024, 129, 4, 100) == 0
    assert q(1024, 256, 1024, 80, -1, 100) == 0 and q(1024, 256, 1024, 80, 4, -1) == 0
    assert q(1024, 256, 1024, 80, 4, 2 ** 31 // 513 + 1) == 0      # frame_capacity * bins >= 2^31


def _host_plan_tiles(lens, F):
    return [(b, f0) for b, L in enumerate(lens) if L >= 2 for f0 in range(0, L, F)]


def _batches():
    F = 32
    yield [1, 2, 3, 4, 5, F, F + 1, 2 * F + 1, 997, 0, 7]
    yield [0]
    yield [1, 1, 0, 1]
    rng = np.random.default_rng(7)
    for B in (1, 2, 17, 256, 1000, 4096):
        for hi in (3, 70, 400):
            yield rng.integers(0, hi, size=B).tolist()


def test_cpp_slot_rule_matches_python_and_the_host_plan(tmp_path):
    """csrc/gl_slot_rule.h, compiled with the host compiler: every slot's (utterance, first frame) equals vocoder.slot_tiles and the
    tile list of the host plan (batch order, f0 = 0, F, 2F, .. for utterances with L >= 2) followed by empty slots -- at the exact
    capacity and at twice it, for F = 32 and the smaller tiles of other geometries."""
    from fastspeech2_amd.vocoder import slot_capacity, slot_tiles
    src = tmp_path / "probe.cpp"
    src.write_text("""
#include <cstdio>
#include <vector>
#include "gl_slot_rule.h"
int main() {
    int B, F; long long cap;
    while (std::scanf("%d %d %lld", &B, &F, &cap) == 3) {
        std::vector<int> end(B);
        int acc = 0;
        for (int b = 0; b < B; ++b) { int L; if (std::scanf("%d", &L) != 1) return 1; acc += fs2::gl_tile_count(L, F); end[b] = acc; }
        const long long slots = fs2::gl_slot_capacity(cap, F, B);
        std::printf("%lld", slots);
        for (long long s = 0; s < slots; ++s) { const fs2::GlSlot r = fs2::gl_slot_tile(end.data(), B, F, (int)s); std::printf(" %d %d", r.b, r.f0); }
        std::printf("\\n");
    }
    return 0;
}
""")
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True)
    cases = [(lens, F, cap) for lens in _batches() for F in (32, 16, 1) for cap in (sum(lens), 2 * sum(lens) + 5) if F > 1 or len(lens) <= 256]
    text = "".join("%d %d %d %s\n" % (len(lens), F, cap, " ".join(map(str, lens))) for lens, F, cap in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    for (lens, F, cap), line in zip(cases, out):
        v = np.array(line.split(), np.int64)
        slots, got = int(v[0]), v[1:].reshape(-1, 2)
        assert slots == slot_capacity(cap, F, len(lens)) == got.shape[0]
        want = slot_tiles(lens, F, cap)
        assert np.array_equal(got, want), (len(lens), F, cap)
        tiles = _host_plan_tiles(lens, F)
        assert len(tiles) <= slots
        assert [tuple(r) for r in got[:len(tiles)].tolist()] == tiles
        assert (got[len(tiles):, 0] == -1).all()


def test_sync_false_argument_checks_need_no_gpu():
    from fastspeech2_amd.vocoder import GriffinLim
    gl = GriffinLim()
    mels = torch.zeros(10, 80)
    with pytest.raises(TypeError, match="olens must be a CUDA int64 tensor"):
        gl(mels, [10], sync=False)
    with pytest.raises(TypeError, match="olens must be a CUDA int64 tensor"):
        gl(mels, torch.tensor([10]), sync=False)
    with pytest.raises(TypeError, match="olens must be int64"):
        gl(mels, torch.tensor([10], dtype=torch.int32), sync=False)
    with pytest.raises(ValueError, match="capacity must be >= 1"):
        gl(mels, torch.tensor([10]), sync=False, capacity=0)
    # the synchronous path keeps its order of checks (the device of mels first) and has no capacities
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(mels, [10])
    with pytest.raises(ValueError, match="sync=False"):
        gl(mels, [10], capacity=10)


# ---- characterisation of the host side the entry points share: the workspace sizes themselves and the calls refused before a launch ----
def _layout_bytes(n_fft, records, planner_B, frames):
    """The documented workspace layout (include/fs2.h): twiddles 8 n_fft, window 4 n_fft, tile records
    32 max(records, 1), then for the capacity form the planner's arrays 16 max(B, 1) (planner_B None: a host-planned call), then for
    synthesis M, C0, C1, T = 4, 8, 8, 8 bytes times frames times bins (frames None: analysis).  Every region starts 256-aligned and so
    does the end."""
    regions = [8 * n_fft, 4 * n_fft, 32 * max(records, 1)]
    if planner_B is not None:
        regions.append(16 * max(planner_B, 1))
    if frames is not None:
        n = frames * (n_fft // 2 + 1)
        regions += [4 * n, 8 * n, 8 * n, 8 * n]
    off = 0
    for r in regions:
        off = -(-off // 256) * 256 + r
    return -(-off // 256) * 256


def test_workspace_sizes_are_the_documented_layout(lib):
    from fastspeech2_amd.vocoder import slot_capacity, tile_rule
    n = 0
    for n_fft, hop, win in GEOMS:
        F = tile_rule(n_fft, hop)["F"]
        g = (n_fft, hop, win, 80)
        default = (n_fft, hop, win) == (1024, 256, 1024)
        rng = np.random.default_rng(n_fft * 7 + hop)
        for B in (1, 3, 64, 1000):
            for hi in (4, 70, 400):
                L = rng.integers(0, hi, size=B)                      # frame counts of a synthesis call
                T = rng.integers(0, hi * hop, size=B)                # sample counts of an analysis call
                Lc, Tc = (C.c_int32 * B)(*L.tolist()), (C.c_int32 * B)(*T.tolist())
                tiles = int(np.where(L >= 2, -(-L // F), 0).sum())
                want = _layout_bytes(n_fft, tiles, None, int(L.sum()))
                assert int(lib.fs2_op_vocode_workspace_bytes_geom(*g, B, Lc)) == want, (g, B, hi)
                cap = int(L.sum())
                want_cap = _layout_bytes(n_fft, slot_capacity(cap, F, B), B, cap)
                assert int(lib.fs2_op_vocode_workspace_bytes_cap(*g, B, cap)) == want_cap, (g, B, hi)
                want_stft = _layout_bytes(n_fft, int((-(-(T // hop + 1) // F)).sum()), None, None)
                assert int(lib.fs2_op_stft_workspace_bytes_geom(*g, B, Tc)) == want_stft, (g, B, hi)
                n += 3
                if default:
                    assert int(lib.fs2_op_vocode_workspace_bytes(B, Lc)) == want
                    assert int(lib.fs2_op_stft_workspace_bytes(B, Tc)) == want_stft
    assert n == 144
    # no utterance, no tile, no frame: one record is still reserved
    for g in GEOMS:
        assert int(lib.fs2_op_vocode_workspace_bytes_geom(*g, 80, 0, None)) == _layout_bytes(g[0], 0, None, 0)
        assert int(lib.fs2_op_stft_workspace_bytes_geom(*g, 80, 0, None)) == _layout_bytes(g[0], 0, None, None)
        assert int(lib.fs2_op_vocode_workspace_bytes_cap(*g, 80, 0, 0)) == _layout_bytes(g[0], 0, 0, 0)


OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -5, -6      # include/fs2.h
PTR = 0x1000           # stands for a device pointer: no call below gets as far as using one
DEFAULT_G = (1024, 256, 1024, 80)


def _i32s(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def _synthesis_call(entry, g=DEFAULT_G, src=PTR, width=80, pinv=PTR, B=None, lens=(10, 5), n_iter=2, momentum=0.0, ws=PTR, ws_bytes=0, wav=PTR):
    """(function name, arguments) of a host-planned synthesis call through the fixed or the _geom entry point."""
    B = (0 if lens is None else len(lens)) if B is None else B
    starts = None if lens is None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    tail = (src, width, pinv, B, _i32s(starts), _i32s(lens), n_iter, momentum, 0, None, ws, ws_bytes, wav)
    return ("fs2_op_griffin_lim", (None,) + tail) if entry == "fixed" else ("fs2_op_griffin_lim_geom", (None,) + tuple(g) + tail)


def _dev_call(g=DEFAULT_G, src=PTR, width=80, pinv=PTR, B=2, lens_dev=PTR, src_stride=0, frame_capacity=15, n_iter=2, momentum=0.0, ws=PTR,
              ws_bytes=0, wav=PTR, wav_stride=0, wav_capacity=256 * 14, sample_lens=PTR, status=PTR):
    return "fs2_op_griffin_lim_dev", (None,) + tuple(g) + (src, width, pinv, B, lens_dev, src_stride, frame_capacity, None, n_iter, momentum, 0, None,
                                                          ws, ws_bytes, wav, wav_stride, wav_capacity, sample_lens, status)


def _analysis_call(entry, g=DEFAULT_G, wav=PTR, B=None, lens=(3000, 700), ws=PTR, ws_bytes=0, mag=PTR, basis=None, logmel=None):
    B = (0 if lens is None else len(lens)) if B is None else B
    starts = None if lens is None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    tail = (wav, B, _i32s(starts), _i32s(lens), ws, ws_bytes, mag, basis, logmel)
    return ("fs2_op_stft", (None,) + tail) if entry == "fixed" else ("fs2_op_stft_geom", (None,) + tuple(g) + tail + (None,))


def _refused_or_empty_calls(lib):
    """(label, function name, arguments, return code) of calls that end before any launch: refused, or accepted as empty.  The codes
    are those of the library before its host code was folded into csrc/griffin_lim_host.h.  Every call passes ``workspace_bytes`` below
    what its batch needs, and the workspace is the last thing either path checks: a call that passed the check it is here for would
    still be refused (with FS2_ERR_WORKSPACE, failing the test) and launch nothing."""
    for e in ("fixed", "geom"):
        s = lambda **kw: _synthesis_call(e, **kw)
        a = lambda **kw: _analysis_call(e, **kw)
        need = int(lib.fs2_op_vocode_workspace_bytes(2, _i32s((10, 5))))
        need_a = int(lib.fs2_op_stft_workspace_bytes(2, _i32s((3000, 700))))
        yield ("src_width", e) + s(width=100) + (ERR_UNSUPPORTED,)
        yield ("src_width of another geometry's bins", e) + s(width=1025) + (ERR_UNSUPPORTED,)
        yield ("mel without pinv", e) + s(pinv=None) + (ERR_ARG,)
        yield ("n_iter < 0", e) + s(n_iter=-1) + (ERR_ARG,)
        yield ("momentum nan", e) + s(momentum=float("nan")) + (ERR_ARG,)
        yield ("momentum < 0", e) + s(momentum=-0.5) + (ERR_ARG,)
        yield ("momentum inf", e) + s(momentum=float("inf")) + (ERR_ARG,)
        yield ("null starts / lens", e) + s(lens=None, B=2) + (ERR_ARG,)
        yield ("negative length", e) + s(lens=(10, -1)) + (ERR_ARG,)
        yield ("B < 0", e) + s(lens=None, B=-1) + (ERR_ARG,)
        yield ("null src", e) + s(src=None) + (ERR_ARG,)
        yield ("null wav", e) + s(wav=None) + (ERR_ARG,)
        yield ("null workspace", e) + s(ws=None) + (ERR_ARG,)
        yield ("workspace one byte short", e) + s(ws_bytes=need - 1) + (ERR_WORKSPACE,)
        yield ("linear input needs no pinv", e) + s(width=513, pinv=None) + (ERR_WORKSPACE,)
        yield ("B = 0", e) + s(lens=None, src=None, wav=None, ws=None) + (OK,)
        yield ("nobody owns a sample", e) + s(lens=(1, 0, 1), src=None, wav=None, ws=None) + (OK,)
        yield ("stft: null starts / lens", e) + a(lens=None, B=2) + (ERR_ARG,)
        yield ("stft: logmel without basis", e) + a(logmel=PTR) + (ERR_ARG,)
        yield ("stft: negative length", e) + a(lens=(3000, -1)) + (ERR_ARG,)
        yield ("stft: null wav", e) + a(wav=None) + (ERR_ARG,)
        yield ("stft: null workspace", e) + a(ws=None) + (ERR_ARG,)
        yield ("stft: workspace one byte short", e) + a(ws_bytes=need_a - 1) + (ERR_WORKSPACE,)
        yield ("stft: B = 0", e) + a(lens=None, wav=None, ws=None) + (OK,)
        yield ("stft: nothing asked for", e) + a(mag=None, wav=None, ws=None) + (OK,)
    # an unsupported geometry is refused before any pointer is looked at
    for bad in ((1000, 256, 1000, 80), (1024, 100, 1024, 80), (1024, 512, 256, 80), (1024, 256, 2048, 80), (1024, 256, 1024, 129)):
        yield ("geometry", bad) + _synthesis_call("geom", g=bad, src=None, pinv=None, wav=None, ws=None, n_iter=-1) + (ERR_UNSUPPORTED,)
        yield ("geometry", bad) + _analysis_call("geom", g=bad, wav=None, ws=None, logmel=PTR) + (ERR_UNSUPPORTED,)
        yield ("geometry", bad) + _dev_call(g=bad, src=None, lens_dev=None, B=0, n_iter=-1) + (ERR_UNSUPPORTED,)
    d = _dev_call
    need = int(lib.fs2_op_vocode_workspace_bytes_cap(*DEFAULT_G, 2, 15))
    yield ("src_width", "dev") + d(width=100) + (ERR_UNSUPPORTED,)
    yield ("mel without pinv", "dev") + d(pinv=None) + (ERR_ARG,)
    yield ("n_iter < 0", "dev") + d(n_iter=-1) + (ERR_ARG,)
    yield ("momentum nan", "dev") + d(momentum=float("nan")) + (ERR_ARG,)
    yield ("momentum < 0", "dev") + d(momentum=-0.5) + (ERR_ARG,)
    yield ("B = 0", "dev") + d(B=0) + (ERR_ARG,)
    yield ("frame_capacity 0", "dev") + d(frame_capacity=0) + (ERR_ARG,)
    yield ("negative stride", "dev") + d(src_stride=-1) + (ERR_ARG,)
    yield ("frame_capacity * bins >= 2^31", "dev") + d(frame_capacity=2 ** 31 // 513 + 1) + (ERR_ARG,)
    yield ("wav_capacity < 0", "dev") + d(wav_capacity=-1) + (ERR_ARG,)
    yield ("padded output beyond wav", "dev") + d(wav_stride=256 * 7 + 1) + (ERR_ARG,)
    yield ("null src", "dev") + d(src=None) + (ERR_ARG,)
    yield ("null lens_dev", "dev") + d(lens_dev=None) + (ERR_ARG,)
    yield ("null workspace", "dev") + d(ws=None) + (ERR_ARG,)
    yield ("null sample_lens", "dev") + d(sample_lens=None) + (ERR_ARG,)
    yield ("null status", "dev") + d(status=None) + (ERR_ARG,)
    yield ("null wav with samples", "dev") + d(wav=None) + (ERR_ARG,)
    yield ("workspace one byte short", "dev") + d(ws_bytes=need - 1) + (ERR_WORKSPACE,)
    yield ("no samples, no wav", "dev") + d(wav=None, wav_capacity=0) + (ERR_WORKSPACE,)
    yield ("linear input needs no pinv", "dev") + d(width=513, pinv=None) + (ERR_WORKSPACE,)


def test_calls_refused_before_a_launch_keep_their_codes(lib):
    n = 0
    for label, where, fn, args, want in _refused_or_empty_calls(lib):
        got = int(getattr(lib, fn)(*args))
        assert got == want, (label, where, fn, got, want)
        if want != OK:
            assert lib.fs2_last_error(None), (label, where)
        n += 1
    assert n >= 80
