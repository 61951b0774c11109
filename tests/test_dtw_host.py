"""CPU: the float64 statement of the DTW validation numbers (tests/dtw_oracle.py) against what it must mean -- the minimum over
all monotone paths, the path its own choices trace back, the cases whose answer is known -- and the host half of
fastspeech2_amd.dtw (DtwTerms: per_utterance / evaluate / merge, fed with the oracle's records; the ctypes mirror of the argument
struct).  The kernels' code runs in tests/test_dtw_kernel_host.py (stand-in) and tests/test_gpu_dtw.py (MI355X)."""
import os

import numpy as np
import pytest

from tests import dtw_oracle as O


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_dp_equals_the_brute_force_minimum():
    rng = np.random.default_rng(0)
    for N in range(1, 6):
        for M in range(1, 6):
            a, b, e, p = O.warped_pair(rng, N, M, 3, noise=0.5)
            d = O.dist(a, b)
            r = O.record(a, b, e, p)
            want = O.brute_force_min(d)
            assert abs(r[O.COST] - want) <= 1e-14 * max(want, 1.0), (N, M)       # (the same terms, added in another order)
            assert r[O.N_] == N and r[O.M_] == M and max(N, M) <= r[O.STEPS] <= N + M - 1


def test_carried_record_equals_backtracking():
    rng = np.random.default_rng(1)
    for N, M in ((1, 1), (1, 9), (9, 1), (7, 12), (30, 22), (41, 41)):
        a, b, e, p = O.warped_pair(rng, N, M, 4)
        r, C, choice = O.record(a, b, e, p, want_choice=True)
        path = O.backtrack(choice)
        assert path[0] == (0, 0) and path[-1] == (N - 1, M - 1) and len(path) == r[O.STEPS]
        assert all((i1 - i0, j1 - j0) in ((1, 1), (1, 0), (0, 1)) for (i0, j0), (i1, j1) in zip(path, path[1:]))
        d = O.dist(a, b)
        cost = se = sp = spv = np.float64(0)
        nv = mis = 0
        for i, j in path:                                                   # the same sums in path order: the same bits
            cost = d[i, j] + cost
            se = se + abs(np.float64(e[0][i]) - np.float64(e[1][j]))
            dp = abs(np.float64(p[0][i]) - np.float64(p[1][j]))
            sp = sp + dp
            if p[0][i] != 0 and p[1][j] != 0:
                nv, spv = nv + 1, spv + dp
            elif (p[0][i] != 0) != (p[1][j] != 0):
                mis += 1
        assert _bits(r[2:9], [len(path), cost, se, sp, nv, spv, mis])
        assert r[O.COST] == C[N - 1, M - 1]


def test_the_two_statements_agree_bit_for_bit():
    rng = np.random.default_rng(2)
    for N, M, D in ((1, 1, 1), (1, 6, 2), (6, 1, 2), (13, 29, 1), (29, 13, 5), (40, 40, 80), (0, 3, 2), (3, 0, 2)):
        a, b, e, p = O.warped_pair(rng, N, M, D)
        assert _bits(O.record(a, b, e, p), O.record_fast(a, b, e, p)), (N, M, D)
        assert _bits(O.record(a, b), O.record_fast(a, b))                   # without tracks: their entries are 0
        assert np.all(O.record(a, b)[4:] == 0)
    a, b, e, p = O.warped_pair(rng, 12, 15, 3)
    a[4, 1] = np.nan                                                        # a NaN behaves alike in both
    r, f = O.record(a, b, e, p), O.record_fast(a, b, e, p)
    assert np.isnan(r[O.COST]) and _bits(r, f)
    a[4, 1], a[11, 0] = 0.0, np.nan                                         # the last frame: C(N-1, M-1) = d + ... is NaN whatever M
    assert np.isnan(O.record_fast(a, b[:1])[O.COST]) and np.isnan(O.record_fast(a, b)[O.COST])


def test_known_answers():
    rng = np.random.default_rng(3)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    x = f(37, 6)
    e, p = np.abs(f(37)), np.where(rng.random(37) < 0.3, 0, 100 + np.abs(f(37))).astype(np.float32)
    r = O.record_fast(x, x, (e, e), (p, p))                                 # identical: the diagonal
    assert r[O.COST] == 0 and r[O.STEPS] == 37 and r[O.ENERGY_L1] == 0 and r[O.PITCH_L1] == 0 and r[O.VUV] == 0 and r[O.VOICED] == (p != 0).sum()
    for rep in (2, 3):                                                      # every frame repeated: cost 0, steps max(N, M)
        xr, er, pr = np.repeat(x, rep, axis=0), np.repeat(e, rep), np.repeat(p, rep)
        for q in ((xr, x, (er, e), (pr, p)), (x, xr, (e, er), (p, pr))):
            r = O.record_fast(*q)
            assert r[O.COST] == 0 and r[O.STEPS] == 37 * rep and r[O.ENERGY_L1] == 0 and r[O.PITCH_L1] == 0 and r[O.VUV] == 0
    for N, M in ((5, 5), (9, 31), (31, 9), (1, 20)):                        # symmetric
        a, b, _, _ = O.warped_pair(rng, N, M, 7, noise=0.3)
        assert O.record_fast(a, b)[O.COST] == O.record_fast(b, a)[O.COST]
    z = np.zeros((9, 2), np.float32)                                        # all ties: the diagonal first, then what the rule says
    r, _, choice = O.record(z, z[:4], want_choice=True)
    assert r[O.STEPS] == 9 and O.backtrack(choice) == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 1), (7, 2), (8, 3)]
    assert O.record(np.zeros((0, 2), np.float32), z).tolist() == [0, 9] + [0] * 10
    assert O.min_gap(O.dist(z, z)) == 0 and O.min_gap(O.dist(z[:1], z)) == np.inf
    a, b, _, _ = O.warped_pair(rng, 40, 50, 8)
    assert 0 < O.min_gap(O.dist(a, b)) < 1 and O.min_gap(O.dist(a, b), nonzero=True) == (O.min_gap(O.dist(a, b)), 0)


def test_mcep_projection_is_orthonormal():
    B = O.dct_basis(80, 13)
    assert B.shape == (80, 13) and np.allclose(B.T @ B, np.eye(13), atol=1e-14)
    assert np.allclose(np.ones(80) @ B, 0, atol=1e-13)                      # coefficient 0 (the level) is left out
    import torch
    from fastspeech2_amd.dtw import dct_basis
    assert np.allclose(dct_basis(80, 13).numpy(), B, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="n_mcep"):
        dct_basis(13, 13)
    x = np.random.default_rng(4).normal(0, 1, (5, 80)).astype(np.float32)
    from fastspeech2_amd.dtw import mcep
    assert np.allclose(mcep(torch.from_numpy(x)).numpy(), O.mcep(x), rtol=0, atol=1e-6)


def _pairs(seed, shapes, D=6):
    rng = np.random.default_rng(seed)
    return [O.warped_pair(rng, N, M, D) for N, M in shapes]


def test_dtw_terms_algebra_and_merge():
    from fastspeech2_amd.dtw import DtwTerms
    rows, batch = O.records(_pairs(5, ((20, 25), (31, 17), (8, 8))))
    t = DtwTerms(rows, batch, "mel", 6)
    pu = t.per_utterance()
    assert pu["n_pred"].tolist() == [20, 31, 8] and pu["n_ref"].tolist() == [25, 17, 8] and pu["steps"].tolist() == rows[:, O.STEPS].astype(int).tolist()
    dist = rows[:, O.COST] / rows[:, O.STEPS]
    assert _bits(pu["distance"], dist) and np.allclose(pu["lsd_db"], 20 / np.log(10) * dist / np.sqrt(6), rtol=1e-15, atol=0) and "mcd_db" not in pu
    assert _bits(pu["energy_l1"], rows[:, 4] / rows[:, 2]) and _bits(pu["pitch_l1"], rows[:, 5] / rows[:, 2])
    assert _bits(pu["f0_l1_voiced"], rows[:, 7] / rows[:, 6]) and _bits(pu["vuv_error"], rows[:, 8] / rows[:, 2])
    assert _bits(pu["length_ratio"], rows[:, 0] / rows[:, 1])
    assert t.evaluate() == (float(np.mean(rows[:, 5] / rows[:, 2])), float(np.mean(rows[:, 4] / rows[:, 2])), float(np.mean(dist)))
    m = DtwTerms(rows, batch, "mcep", 6).per_utterance()
    assert np.allclose(m["mcd_db"], 10 * np.sqrt(2) / np.log(10) * dist, rtol=1e-15, atol=0) and "lsd_db" not in m
    merged = DtwTerms.empty("mel")
    for q in _pairs(5, ((20, 25), (31, 17), (8, 8))):
        r1, b1 = O.records([q])
        merged = merged.merge(DtwTerms(r1, b1, "mel", 6))
    assert len(merged) == 3 and merged.D == 6 and _bits(merged.terms, rows) and O.close(merged.batch, batch)
    assert merged.evaluate() == t.evaluate()
    with pytest.raises(ValueError, match="features"):
        t.merge(DtwTerms(rows, batch, "mcep", 6))
    with pytest.raises(ValueError, match="width"):
        t.merge(DtwTerms(rows, batch, "mel", 13))
    with pytest.raises(ValueError, match="features"):
        DtwTerms(rows, batch, "mfcc", 6)
    nothing = DtwTerms.empty()
    assert len(nothing) == 0 and np.all(nothing.batch == 0) and _bits(nothing.merge(t).batch, batch)
    zero = DtwTerms(*O.records(_pairs(6, ((0, 4),))), "mel", 6).per_utterance()          # no path: nothing to average
    assert np.isnan(zero["distance"][0]) and zero["length_ratio"][0] == 0


def test_cpu_tensors_raise():
    import torch
    from fastspeech2_amd import mel_dtw
    z = torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mel_dtw(z, [2], z, [2])
    from fastspeech2_amd import FeedForwardTransformer
    assert callable(FeedForwardTransformer.evaluate_free_running)


def test_ctypes_mirror_of_the_argument_struct_matches_the_compiled_header(tmp_path):
    """fs2_op_dtw_args as gcc sees include/fs2.h: sizeof and the offset of every field equal those of _lib.OpDtwArgs."""
    import ctypes
    import re
    import subprocess
    from fastspeech2_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in _lib.OpDtwArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fs2.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(fs2_op_dtw_args));', '  printf("FS2_DTW_TERMS %d\\n", FS2_DTW_TERMS);',
           '  printf("FS2_ABI_VERSION %d\\n", FS2_ABI_VERSION);']
    src += ['  printf("%s %%zu\\n", offsetof(fs2_op_dtw_args, %s));' % (f, f) for f in fields] + ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", exe], check=True)
    probe = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert probe["sizeof"] == ctypes.sizeof(_lib.OpDtwArgs) == _lib.OpDtwArgs().struct_size
    assert probe["FS2_DTW_TERMS"] == _lib.DTW_TERMS == O.TERMS
    assert probe["FS2_ABI_VERSION"] == _lib.ABI_VERSION == 4                # the addition is additive
    for f in fields:
        assert getattr(_lib.OpDtwArgs, f).offset == probe[f], f
    hdr = open(os.path.join(root, "include", "fs2.h")).read()
    body = hdr[hdr.index("struct fs2_op_dtw_args {"):hdr.index("typedef struct fs2_op_dtw_args")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[*\s,](\w+)\s*[,;]", body[body.index("{"):])
    assert declared == fields, (declared, fields)
