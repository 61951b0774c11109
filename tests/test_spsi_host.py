"""CPU: the numpy statement of the SPSI initial phase (tests/spsi_oracle.py) against a case done by hand and against a literal
transcription of the published sequential algorithm; what the phase is for (10 Griffin-Lim iterations from it beat 20 from the seeded
random phase, on the float64 oracle of tests/vocoder_oracle.py); the C ABI's new symbols; and the argument errors of the Python layer
that need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import spsi_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_case_done_by_hand():
    # 9 bins (n_fft 16, hop 4: hop / n_fft = 0.25).  Row 0: peaks at 2 and 5 share the valley 4, a plateau at 6-7.  Row 1: all zero.
    M = np.asarray([[0, 1, 3, 1, 0.5, 2, 1, 1, 0], [0] * 9], np.float32)
    own, half, right = S.owners(M[0])
    assert own.tolist() == [-1, 2, 2, 2, 5, 5, 5, -1, -1]                    # the valley 4 belongs to the right peak; 7 (plateau) to none
    assert half.tolist() == [False, True, False, True, True, False, True, False, False]
    assert not right[2] and right[5]
    # peak 2: a = c: p = 0, w = 8 / 16 = 0.5.  peak 5: den = (0.5 - 4) + 1 = -2.5, p = 0.5 (-0.5) / -2.5 = 0.1, w = 4 / 16 + 0.1 / 4 = 0.275
    assert S.peak_advance(M[0], 2, 16, 4) == np.float32(0.5)
    assert abs(float(S.peak_advance(M[0], 5, 16, 4)) - 0.275) < 1e-7
    t = S.spsi_turns(M, 16, 4)
    want = [0, 0.0, 0.5, 0.0, 0.775, 0.275, 0.775, 0, 0]                      # bins 1 and 3: 0.5 + 0.5 wraps to 0
    assert np.allclose(t[0], want, atol=1e-7) and t[0][1] == 0 and t[0][3] == 0
    assert np.array_equal(t[1], t[0])                                         # the zero row has no peak: every bin keeps its phase
    assert np.array_equal(S.spsi_phase(M, 16, 4), t * np.float32(6.28318548))
    # the chain: the same row twice advances the peak twice; right peak: d = -2 and +1 shifted, d = +2, +3 not
    M = np.asarray([[0, 0, 0, 1, 4, 2, 1, 0, 0]] * 2, np.float32)
    own, half, right = S.owners(M[0])
    assert own.tolist() == [-1, -1, 4, 4, 4, 4, 4, 4, -1] and right[4]
    assert half.tolist() == [False, False, True, True, False, True, False, False, False]
    t = S.spsi_turns(M, 16, 4)                                                # w = 0 + 0.1 / 4 = 0.025
    assert np.allclose(t[0], [0, 0, .525, .525, .025, .525, .025, .025, 0], atol=1e-7)
    assert np.allclose(t[1], [0, 0, .55, .55, .05, .55, .05, .05, 0], atol=1e-7)


@pytest.mark.parametrize("name", sorted(S.crafted_rows(513)))
def test_crafted_rows(name):
    NB = 513
    m = S.crafted_rows(NB)[name]
    own, half, right = S.owners(m)
    peaks = np.flatnonzero(own == np.arange(NB))
    assert own[0] == -1 and own[NB - 1] == -1
    if name == "peak_at_bin_1":
        assert 1 in peaks and own[2] == 1 and right[1] == (m[2] > m[0])
    if name == "peak_at_bin_NB-2":
        assert NB - 2 in peaks and own[NB - 3] == NB - 2 and half[NB - 3]           # not right (c > a), d = -1
    if name == "two_peaks_sharing_a_valley":
        assert peaks.tolist() == [11, 15] and own[10:17].tolist() == [11, 11, 11, 15, 15, 15, 15]
    if name == "plateau_next_to_a_peak":
        assert own[21:25].tolist() == [23] * 4 and own[20] != 23 and own[25] != 23 and own[26] != 23     # 20-21 and 24-25 are plateaus
    if name in ("monotone", "all_zero"):
        assert peaks.size == 0 and np.all(own == -1)
    if name == "nan_and_inf":
        assert 40 not in peaks and own[40] == -1 and 50 in peaks and 60 not in peaks and 61 not in peaks
        assert np.all(np.isfinite(S.spsi_turns(np.stack([m, m]), 1024, 256)))
    t = S.spsi_turns(np.stack([m, m, m]), 1024, 256)
    assert np.all((t >= 0) & (t <= 1))


@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (512, 128), (2048, 300), (16, 4)])
def test_closed_form_equals_the_published_sequential_algorithm(n_fft, hop):
    NB = n_fft // 2 + 1
    cases = [S.random_rows(12, NB, 7), np.random.RandomState(8).rand(12, NB).astype(np.float32)]
    if NB >= 257:
        c = S.crafted_rows(NB)
        cases.append(np.stack([c[k] for k in sorted(c) if k != "nan_and_inf"] * 2))
    for M in cases:
        got, want = S.spsi_turns(M, n_fft, hop), S.spsi_published(M, n_fft, hop)
        d = S.wrapped_diff(got, want)[:, 1:NB - 1]
        bound = 2.0 ** -20 * (np.arange(M.shape[0]) + 1)[:, None]
        assert np.all(d <= bound), float((d / bound).max())
        assert np.all(got[:, 0] == 0) and np.all(got[:, NB - 1] == 0)


@pytest.mark.parametrize("mel", [False, True], ids=["magnitudes", "mel_round_trip"])
@pytest.mark.parametrize("geom", [(1024, 256, 1024), (2048, 300, 1200)], ids=lambda g: "%d_%d_%d" % g)
def test_ten_iterations_from_spsi_beat_twenty_from_the_seeded_phase(geom, mel):
    """Seen with the hash seeds (seed_angles(0, L)) on the float64 oracle, SPSI + 10 iterations / seeded + 20 iterations:
    1024/256/1024 magnitudes 0.1010 / 0.1869, through 80 mels 0.1270 / 0.2255; 2048/300/1200 magnitudes 0.0845 / 0.2434,
    through 80 mels 0.1414 / 0.2570."""
    c = S.convergence_case(*geom, mel)
    print("sc spsi+10 %.4f seeded+20 %.4f" % (c["sc_spsi10"], c["sc_seed20"]))
    assert c["sc_spsi10"] < c["sc_seed20"], c


NEW = ["fs2_op_spsi_workspace_bytes_geom", "fs2_op_spsi_workspace_bytes_cap", "fs2_op_spsi_phase_geom", "fs2_op_spsi_phase_dev"]


def test_abi_declares_and_exports_the_new_symbols():
    from fastspeech2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fs2.h")).read()
    assert re.search(r"#define FS2_ABI_VERSION 4\b", hdr) and _lib.ABI_VERSION == 4
    for s in NEW:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        L = ctypes.CDLL(_lib.LIB_PATH)
        L.fs2_abi_version.restype = ctypes.c_int32
        assert L.fs2_abi_version() == 4
        for s in NEW:
            assert hasattr(L, s), s
        # host-only queries: sizes and refusals
        i32 = ctypes.c_int32
        for f in (L.fs2_op_spsi_workspace_bytes_geom, L.fs2_op_spsi_workspace_bytes_cap):
            f.restype = ctypes.c_size_t
        lens = (i32 * 3)(5, 0, 7)
        L.fs2_op_spsi_workspace_bytes_geom.argtypes = [i32] * 5 + [ctypes.POINTER(i32)]
        L.fs2_op_spsi_workspace_bytes_cap.argtypes = [i32] * 5 + [ctypes.c_int64]
        n = L.fs2_op_spsi_workspace_bytes_geom(1024, 256, 1024, 80, 3, lens)
        assert n >= 12 * 513 * 6 and n == L.fs2_op_spsi_workspace_bytes_cap(1024, 256, 1024, 80, 3, 12)
        assert L.fs2_op_spsi_workspace_bytes_geom(1000, 256, 1000, 80, 3, lens) == 0          # unsupported n_fft
        assert L.fs2_op_spsi_workspace_bytes_geom(1024, 256, 1024, 80, 3, (i32 * 3)(5, -1, 7)) == 0
        assert L.fs2_op_spsi_workspace_bytes_cap(1024, 256, 1024, 80, 0, 12) == 0
        assert L.fs2_op_spsi_workspace_bytes_cap(1024, 256, 1024, 80, 3, 2 ** 31) == 0


def test_argument_errors_that_need_no_gpu():
    from fastspeech2_amd import GriffinLim, spsi_phase
    gl = GriffinLim()
    mel = torch.zeros(6, 80)
    with pytest.raises(ValueError, match="init must be one of"):
        gl(mel, [6], init="random")
    with pytest.raises(ValueError, match="init must be one of"):
        gl(mel, torch.tensor([6]), init="random", sync=False)
    with pytest.raises(ValueError, match="not both"):
        gl(mel, [6], init="spsi", init_phase=torch.zeros(6, 513))
    with pytest.raises(ValueError, match="not both"):
        gl(mel, torch.tensor([6]), init="spsi", init_phase=torch.zeros(6, 513), sync=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gl(mel, [6], init="spsi")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spsi_phase(mel, [6])
    with pytest.raises(TypeError, match="torch.Tensor"):
        spsi_phase(np.zeros((6, 80), np.float32), [6])
    with pytest.raises(TypeError, match="CUDA int64"):
        spsi_phase(mel, [6], sync=False)
    with pytest.raises(TypeError, match="CUDA int64"):
        spsi_phase(mel, torch.tensor([6]), sync=False)
