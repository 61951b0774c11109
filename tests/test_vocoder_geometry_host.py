"""Host-side checks of the vocoder at other transform geometries (no GPU): the generic float64 oracle against the default one and
against the reference's recorded outputs (tests/golden/g11_stft_geometries.npz, tools/gen_golden_stft_geometries.py), the shortest
utterance the reference can pad, an exhaustive check of the fused kernel's tile and halo rule, the hp.audio parsing table and the
seeded phase at other bin counts."""
import os

import numpy as np
import pytest
import torch

from tests import vocoder_oracle as O

# reference fp32 vs float64 oracle, relative to the peak, measured when the fixture was recorded (GL 0 / 1 / 30 iterations, energy)
MEASURED = {(2048, 300, 1200): (7.2e-7, 9.8e-7, 2.0e-5, 1.0e-6),
            (512, 160, 400): (8.5e-7, 6.7e-6, 6.7e-5, 5.9e-7),
            (1024, 200, 800): (8.2e-7, 1.7e-6, 5.1e-5, 9.2e-7)}
GEOMETRIES = [(1024, 256, 1024), (2048, 300, 1200), (512, 128, 512), (512, 160, 400), (1024, 200, 800), (2048, 512, 2048)]


@pytest.fixture(scope="module")
def g11(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g11_stft_geometries.npz")))


@pytest.fixture(scope="module")
def g10(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g10_griffin_lim.npz")))


def test_generic_oracle_is_the_default_oracle_at_1024_256(g10):
    o = O.Stft(1024, 256, 1024)
    sig = g10["signal"].astype(np.float64)
    X, Xd = o.stft(sig), O.stft(sig)
    assert np.abs(X - Xd).max() <= 1e-12 * np.abs(Xd).max()
    for n in (0, 1, 3):
        got, want = o.griffin_lim(g10["magnitudes"], g10["angles"], n), O.griffin_lim(g10["magnitudes"], g10["angles"], n)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), n
    assert np.array_equal(O.hann_padded(1024, 1024), O.hann())


@pytest.mark.parametrize("geom", sorted(MEASURED))
def test_oracle_matches_reference_fixture(g11, geom):
    n_fft, hop, win = geom
    k = "%d_%d_%d/" % geom
    o = O.Stft(n_fft, hop, win)
    M, A = g11[k + "magnitudes"], g11[k + "angles"]
    assert M.shape == (44, n_fft // 2 + 1)
    bars = MEASURED[geom]
    for i, n in enumerate((0, 1, 30)):
        ref = g11[k + "wav_iter%d" % n]
        got = o.griffin_lim(M, A, n)
        assert got.shape == ref.shape == (hop * 43,)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s n_iter %d: %.3e (bar %.1e)" % (geom, n, err, 10 * bars[i]))
        assert err <= 10 * bars[i], (n, err)
    e = o.energy(g11[k + "signal"])
    err = np.abs(e - g11[k + "energy"]).max() / np.abs(e).max()
    print("%s energy: %.3e (bar %.1e)" % (geom, err, 10 * bars[3]))
    assert err <= 10 * bars[3], err
    # the fixture's magnitudes are the reference's |STFT| of its signal
    Mo = np.abs(o.stft(g11[k + "signal"]))
    assert np.abs(Mo - M).max() <= 1e-5 * Mo.max()


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_l_min_is_where_reflect_padding_works(geom):
    n_fft, hop, win = geom
    lmin = n_fft // (2 * hop) + 2
    assert O.l_min(n_fft, hop) == lmin
    from fastspeech2_amd.vocoder import Geometry
    assert Geometry(n_fft, hop, win).l_min == lmin
    for L in range(1, lmin + 4):
        T = hop * (L - 1)
        x = torch.zeros(1, 1, max(T, 1))[..., :T]
        try:        # the reference's STFT.transform pads with torch's reflect mode
            torch.nn.functional.pad(x.unsqueeze(1), (n_fft // 2, n_fft // 2, 0, 0), mode="reflect")
            ok = True
        except (RuntimeError, ValueError):
            ok = False
        assert ok == (L >= lmin), (L, lmin)
        if L >= 2:
            ok_o = True
            try:
                O.Stft(n_fft, hop, win).stft(np.zeros(T))
            except ValueError:
                ok_o = False
            assert ok_o == (L >= lmin)


def _supported():
    for n in (512, 1024, 2048):
        for hop in range(-(-n // 8), n + 1):
            yield n, hop


def test_tile_rule_exhaustive():
    """For every supported (n_fft, hop) and every L_min <= L < 200: each tile's inverse-transformed frames [fa, fb] contain every
    frame that overlaps a sample its own frames read (the reflect padding at both ends included) or a sample it writes in the final
    ISTFT; every such sample lies inside the tile's signal buffer; the buffer fits the kernel's bound and the LDS; the tiles
    partition the frames."""
    from fastspeech2_amd.vocoder import tile_rule
    n_checked = 0
    for n, hop in _supported():
        r = tile_rule(n, hop)
        F, n2 = r["F"], n // 2
        assert 28 * n + 4 * r["sig_max"] <= 163840 and F >= 8
        if (n, hop) == (1024, 256):
            assert (F, r["halo"], r["tail"], r["lmin"], r["sig_max"]) == (32, 3, 5, 4, 256 * 37 + 1024)
        Ls, f0s = [], []
        for L in range(r["lmin"], 200):
            f0 = np.arange(0, L, F)
            Ls.append(np.full(f0.size, L))
            f0s.append(f0)
        L, f0 = np.concatenate(Ls), np.concatenate(f0s)
        nf = np.minimum(F, L - f0)
        fl = f0 + nf - 1
        T = hop * (L - 1)
        # the rule under test (csrc/griffin_lim.h gl_iterate, vocoder.tile_span)
        fa = np.maximum(0, np.minimum(f0 - r["halo"], L - r["tail"]))
        fb = np.minimum(L - 1, fl + r["halo"])
        # trimmed samples the own frames' STFT reads: direct part, reflections at the start and the end (a hull: conservative)
        lo, hi = hop * f0 - n2, hop * fl + n2 - 1
        assert (T > n2).all()
        smin = np.maximum(lo, 0)
        smax = np.minimum(hi, T - 1)
        refl_lo = lo < 0
        smax = np.where(refl_lo, np.maximum(smax, -lo), smax)
        refl_hi = hi >= T
        smin = np.where(refl_hi, np.minimum(smin, 2 * (T - 1) - hi), smin)
        assert (smin >= 0).all() and (smax <= T - 1).all()
        # samples the final ISTFT writes
        wmin, wmax = hop * f0, np.minimum(T, hop * (f0 + nf)) - 1
        smin2, smax2 = np.minimum(smin, wmin), np.maximum(smax, wmax)
        # frames overlapping pre-trim positions p = s + n/2: hop f <= p < hop f + n
        pmin, pmax = smin2 + n2, smax2 + n2
        need_a = np.maximum(0, (pmin - n) // hop + 1)
        need_b = np.minimum(L - 1, pmax // hop)
        bad = (need_a < fa) | (need_b > fb)
        assert not bad.any(), (n, hop, L[bad][:3], f0[bad][:3])
        # buffer: trimmed sample s at sig[s + n/2 - hop fa], length hop (fb - fa) + n <= sig_max
        qoff = n2 - hop * fa
        SL = hop * (fb - fa) + n
        assert (smin2 + qoff >= 0).all() and (smax2 + qoff < SL).all()
        assert (SL <= r["sig_max"]).all()
        n_checked += L.size
    assert n_checked > 1000000


def test_tile_span_matches_rule():
    from fastspeech2_amd.vocoder import tile_rule, tile_span
    assert tile_span(1024, 256, 97, 96) == (92, 96)           # a tile at the last frame of the default: frame L - 5 joins
    assert tile_span(1024, 256, 100, 32) == (29, 66)
    r = tile_rule(2048, 2048)
    assert r["halo"] == 1 and r["F"] == 8                      # hop = n_fft: the final ISTFT's samples reach one frame past the tile


ACCEPTED = [
    ({}, (1024, 256, 1024, 80)),
    ({"hop_length": 256}, (1024, 256, 1024, 80)),
    ({"num_mels": 80, "sample_rate": 22050, "hop_length": 256}, (1024, 256, 1024, 80)),
    ({"n_fft": 1024, "hop_length": 256, "win_length": 1024}, (1024, 256, 1024, 80)),
    ({"n_fft": 2048, "hop_length": 300, "win_length": 1200, "sample_rate": 24000}, (2048, 300, 1200, 80)),
    ({"n_fft": 512, "hop_length": 128, "win_length": 512}, (512, 128, 512, 80)),
    ({"n_fft": 512, "hop_length": 160, "win_length": 400, "sample_rate": 16000}, (512, 160, 400, 80)),
    ({"n_fft": 1024, "hop_length": 200, "win_length": 800}, (1024, 200, 800, 80)),
    ({"n_fft": 2048, "hop_length": 512, "win_length": 2048}, (2048, 512, 2048, 80)),
    ({"num_mels": 128}, (1024, 256, 1024, 128)),
    ({"n_mels": 64, "num_mels": 80}, (1024, 256, 1024, 64)),
]
REJECTED = [
    ({"n_fft": 800, "hop_length": 200, "win_length": 800}, "n_fft"),
    ({"n_fft": 1024, "hop_length": 256, "win_length": 2048}, "win_length"),
    ({"n_fft": 1024, "hop_length": 600, "win_length": 512}, "hop"),
    ({"n_fft": 2048, "hop_length": 200, "win_length": 2048}, "ceil"),
    ({"n_mels": 0}, "n_mels"),
    ({"num_mels": 129}, "n_mels"),
    ({"n_fft": 2048}, "hop_length, win_length"),
    ({"n_fft": 2048, "hop_length": 300}, "win_length"),
    ({"hop_length": 200}, "hop"),
    ({"win_length": 800}, "n_fft, hop_length"),
]


@pytest.mark.parametrize("audio,want", ACCEPTED)
def test_hp_audio_accepted(audio, want):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    gl = GriffinLim(DotDict({"audio": audio}))
    assert tuple(gl.geometry) == want
    assert gl.geometry.n_bins == want[0] // 2 + 1
    assert set(gl.params) == {"sample_rate", "n_fft", "n_mels", "fmin", "fmax"}
    assert gl.params["n_fft"] == want[0] and gl.params["n_mels"] == want[3]
    assert gl._basis_np.shape == (want[3], want[0] // 2 + 1) and gl._pinv_np.shape == (want[0] // 2 + 1, want[3])


@pytest.mark.parametrize("audio,match", REJECTED)
def test_hp_audio_rejected(audio, match):
    from fastspeech2_amd.hparams import DotDict
    from fastspeech2_amd.vocoder import GriffinLim
    with pytest.raises(ValueError, match=match):
        GriffinLim(DotDict({"audio": audio}))


def test_default_hparams_keep_the_default_geometry():
    from fastspeech2_amd import default_hparams
    from fastspeech2_amd.vocoder import GriffinLim
    assert tuple(GriffinLim(default_hparams()).geometry) == (1024, 256, 1024, 80)


def test_seed_angles_n_bins():
    from fastspeech2_amd.vocoder import seed_angles, _mix32
    assert np.array_equal(seed_angles(7, 5, n_bins=513), seed_angles(7, 5))
    a = seed_angles(3, 4, n_bins=1025)
    assert a.shape == (4, 1025)
    s = int(_mix32(np.uint32((3 + 0x9E3779B9) & 0xFFFFFFFF)))

    def mix(x):
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
        return x
    for f, k in ((0, 0), (3, 1024), (2, 7)):
        h = mix(((k + 1025 * f) & 0xFFFFFFFF) ^ s)
        want = np.float32(np.float32(h >> 8) * np.float32(1.0 / 16777216.0)) * np.float32(6.28318548) - np.float32(3.14159274)
        assert a[f, k] == want


def test_geometry_entry_points_are_bound():
    from fastspeech2_amd import _lib
    from fastspeech2_amd.vocoder import Geometry
    assert tuple(Geometry()) == (1024, 256, 1024, 80)         # the (n_fft, hop, win, n_mels) argument order of the _geom entry points
    for s in ("fs2_op_vocode_workspace_bytes_geom", "fs2_op_griffin_lim_geom", "fs2_op_stft_workspace_bytes_geom", "fs2_op_stft_geom"):
        assert s in _lib.EXPORTS


def test_cpp_tile_rule_matches_python(tmp_path):
    """The kernels and the host plan use csrc/gl_tile_rule.h; compiled here with the host compiler, it must give the same halo, tail
    frame, L_min, signal buffer and F as vocoder.tile_rule (the restatement test_tile_rule_exhaustive checks) for every supported
    (n_fft, hop)."""
    import subprocess
    from fastspeech2_amd.vocoder import tile_rule
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastspeech2_amd", "csrc")
    src = tmp_path / "probe.cpp"
    src.write_text('#include "gl_tile_rule.h"\n#include <cstdio>\nint main() {\n'
                   '    for (int n = 512; n <= 2048; n *= 2)\n'
                   '        for (int h = (n + 7) / 8; h <= n; ++h) {\n'
                   '            const int F = fs2::gl_tile_frames(n, h);\n'
                   '            std::printf("%d %d %d %d %d %d %d\\n", n, h, F, fs2::gl_halo(n, h), fs2::gl_tail(n, h), fs2::gl_lmin(n, h),\n'
                   '                        fs2::gl_sig_max(n, h, F));\n'
                   '        }\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", exe], check=True)
    rows = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {(r[0], r[1]): r[2:] for r in (tuple(int(x) for x in line.split()) for line in rows if line.strip())}
    want = {(n, h): None for n, h in _supported()}
    assert set(got) == set(want)
    for (n, h) in want:
        r = tile_rule(n, h)
        assert got[(n, h)] == (r["F"], r["halo"], r["tail"], r["lmin"], r["sig_max"]), (n, h)
