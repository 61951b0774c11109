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
