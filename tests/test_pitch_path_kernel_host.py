"""CPU: the code of the pitch path kernels (csrc/pitch_path.h: pitch_path, records_combine<8, 1, 5> and their host side) compiled for the
host against the stand-in of the HIP constructs it uses (tests/kernel_standin: one thread per lane, one workgroup at a time) and run
on the edge batch of tests/pitch_path_oracle.py: synthetic_batch.  This checks the kernels' logic -- the chunks and what is carried
from one to the next, what is read after which barrier, the packed back pointers, the walk back and its counts -- and every index
they form without a GPU; what hipcc makes of the arithmetic only tests/test_gpu_pitch_path.py can see.

The bar: f0, state, strength and the integer entries of the records EQUAL the numpy float64 oracle's.  Both sides perform the same
IEEE double operations in the same order; the one term that may differ is log2 (libm's against numpy's), by an ulp of a value
below 16, that is 1.8e-15, and condition (b) of tests/test_pitch_path_host.py (no cell's two best predecessors closer than 1e-9 of
the cell) keeps that from flipping a choice on real candidates; the random candidates here are checked for the same.  So the score
D (a sum of at most 131 terms of order 1) is held to 1e-12 relative and the largest octave step (a difference of two log2) to
1e-12 absolute.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pitch_path_oracle as Q, standin_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_STEP = 256 / 22050
COSTS = {"default": dict(Q.DEFAULTS), "zero": dict(Q.DEFAULTS, octave_jump_cost=0.0, voiced_unvoiced_cost=0.0),
         "second": dict(Q.DEFAULTS, octave_jump_cost=0.7, voiced_unvoiced_cost=0.05, voicing_threshold=0.3, octave_cost=0.05, f0_floor=60.0)}
INTEGERS = [Q.N_FRAMES, Q.FLAGS, Q.VOICED, Q.SWITCHES, Q.CHANGED, 7]


def chunk():
    src = open(os.path.join(ROOT, "fastspeech2_amd", "csrc", "pitch_path.h")).read()
    return int(re.search(r"constexpr int kPathChunk = (\d+);", src).group(1))


def utts_per_launch():
    src = open(os.path.join(ROOT, "fastspeech2_amd", "csrc", "pitch_path.h")).read()
    return int(re.search(r"constexpr int kPathUttsPerLaunch = (\d+);", src).group(1))


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/pitch_path_main.cpp")


def pack(utts):
    """(cand_f0 [rows, K], cand_strength [rows, K], starts [B], lens [B]) of a list of (f, p)."""
    lens = np.asarray([len(f) for f, _ in utts], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    return np.concatenate([f for f, _ in utts]), np.concatenate([p for _, p in utts]), starts, lens


def _run(standin, tmp_path, utts, K, order, costs):
    """The utterances ``order`` of ``utts``, read in place from the packed arrays -> (rows [len(order), 8], batch, f0, state, strength)."""
    cf, cp, starts, lens = pack(utts)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([len(order), K, len(cf)], np.int32).tobytes())
        f.write(np.asarray([TIME_STEP] + [costs[k] for k in ("f0_floor", "voicing_threshold", "octave_cost", "octave_jump_cost", "voiced_unvoiced_cost")],
                           np.float64).tobytes())
        for x in (starts[order], lens[order], cf, cp):
            f.write(np.ascontiguousarray(x).tobytes())
    r = subprocess.run([standin, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    n, rows = (len(order) + 1) * Q.TERMS * 8, len(cf)
    out = np.frombuffer(raw[:n], np.float64).reshape(len(order) + 1, Q.TERMS)
    f0 = np.frombuffer(raw[n:n + 4 * rows], np.float32)
    state = np.frombuffer(raw[n + 4 * rows:n + 8 * rows], np.int32)
    strength = np.frombuffer(raw[n + 8 * rows:], np.float32)
    assert len(strength) == rows
    return out[:-1], out[-1], f0, state, strength


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def assert_records(got, want):
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert np.array_equal(got[:, INTEGERS], want[:, INTEGERS])
    assert np.all(np.abs(got[:, Q.SCORE] - want[:, Q.SCORE]) <= 1e-12 * np.abs(want[:, Q.SCORE]))
    assert np.all(np.abs(got[:, Q.MAX_STEP] - want[:, Q.MAX_STEP]) <= 1e-12)


def _assert_equal(utts, order, got, costs):
    rows, batch, f0, state, strength = got
    _, _, starts, lens = pack(utts)
    want = [Q.path(*utts[n], TIME_STEP, **costs) for n in order]
    assert_records(rows, Q.records(want)[0])
    assert_records(batch, Q.records(want)[1])
    untouched = np.ones(len(f0), bool)
    for n, w in zip(order, want):
        sl = slice(starts[n], starts[n] + lens[n])
        assert _bits(f0[sl], w.f0) and np.array_equal(state[sl], w.state) and _bits(strength[sl], w.strength), n
        untouched[sl] = False
    assert np.all(f0[untouched] == -777) and np.all(state[untouched] == -777) and np.all(strength[untouched] == -777)
    return want


def test_the_edge_batch_is_what_the_issue_asks_for():
    C = chunk()
    assert Q.edge_lens(C) == [0, 1, 2, C - 1, C, C + 1, 2 * C + 3]
    for K in (1, 3, 8):
        utts = Q.synthetic_batch(C, K)
        assert [len(f) for f, _ in utts] == Q.edge_lens(C) + [C + 1] * 3 and all(f.shape == (len(f), K) == p.shape for f, p in utts)
        assert not utts[-3][0].any() and (utts[-2][0] > 0).all() and np.isnan(utts[-1][0]).sum() == 1
        assert any((f > 0).any() and not (f > 0).any(axis=1).all() for f, _ in utts[:7])          # frames without a candidate beside frames with some
        for f, p in utts[:-1]:                                                                    # no choice hangs on the last bit of a log2
            assert Q.path(f, p, TIME_STEP).gap >= 1e-9


@pytest.mark.parametrize("K", [1, 3, 8])
def test_kernel_code_on_the_host_equals_the_oracle(standin, tmp_path, K):
    utts = Q.synthetic_batch(chunk(), K)
    everything = list(range(len(utts)))
    want = _assert_equal(utts, everything, _run(standin, tmp_path, utts, K, everything, COSTS["default"]), COSTS["default"])
    assert [int(w.record[Q.FLAGS]) for w in want] == [0] * 9 + [2]
    assert want[7].record[Q.VOICED] == 0 and not want[7].f0.any()                                   # no candidate anywhere: unvoiced throughout
    assert np.all(want[9].state == -1) and not want[9].f0.any() and np.all(want[9].record[2:] == 0)
    assert any(w.record[Q.CHANGED] > 0 for w in want) and any(w.record[Q.SWITCHES] > 0 for w in want)
    shuffled = [6, 9, 0, 3, 8, 1, 5, 7, 2, 4]
    got = _run(standin, tmp_path, utts, K, shuffled, COSTS["default"])
    again = _assert_equal(utts, shuffled, got, COSTS["default"])
    assert all(np.array_equal(again[i].record, want[n].record) for i, n in enumerate(shuffled))
    alone = _run(standin, tmp_path, utts, K, [6], COSTS["default"])                                 # without the NaN utterance beside it
    _assert_equal(utts, [6], alone, COSTS["default"])
    assert np.array_equal(alone[0][0].view(np.uint64), got[0][0].view(np.uint64))
    _assert_equal(utts, everything, _run(standin, tmp_path, utts, K, everything, COSTS["second"]), COSTS["second"])
    # both costs 0: the per-frame argmax of u, ties to unvoiced
    zero = _run(standin, tmp_path, utts, K, everything, COSTS["zero"])
    _assert_equal(utts, everything, zero, COSTS["zero"])
    _, _, starts, lens = pack(utts)
    for n in everything[:-1]:
        assert np.array_equal(zero[3][starts[n]:starts[n] + lens[n]], Q.frame_argmax(*utts[n]))
        assert zero[0][n, Q.CHANGED] == 0


def test_more_utterances_than_one_launch_holds(standin, tmp_path):
    """129 utterances at K = 2: the last one travels with a second launch, behind an utterance one frame longer than a chunk."""
    C, n = chunk(), utts_per_launch()
    utts = Q.boundary_batch(C, n)
    lens = [len(f) for f, _ in utts]
    assert len(utts) == n + 1 == 129 and lens[n - 1] == C + 1 == 65 and lens[n] > 0 and max(lens[:n - 1] + lens[n:]) == 3 and min(lens) == 0
    everything = list(range(n + 1))
    want = _assert_equal(utts, everything, _run(standin, tmp_path, utts, 2, everything, COSTS["default"]), COSTS["default"])
    assert all(w.gap >= 1e-9 for w in want) and not any(w.record[Q.FLAGS] for w in want)     # no choice hangs on the last bit of a log2


def test_host_side_argument_checks(standin):
    r = subprocess.run([standin, "--checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    got = dict(line.split() for line in r.stdout.splitlines())
    OK, ERR_ARG, ERR_WORKSPACE = "0", "-1", "-5"                       # include/fs2.h
    want = dict(ok=OK, ok_state="000_-1-1", ok_voiced="30", ok_batch_frames="5", struct_size=ERR_ARG, K_0=ERR_ARG, K_9=ERR_ARG, negative_B=ERR_ARG,
                null_lens=ERR_ARG, null_starts=ERR_ARG, negative_len=ERR_ARG, negative_start=ERR_ARG, time_step_0=ERR_ARG, time_step_negative=ERR_ARG,
                time_step_nan=ERR_ARG, time_step_inf=ERR_ARG, f0_floor_0=ERR_ARG, f0_floor_nan=ERR_ARG, threshold_nan=ERR_ARG, octave_cost_inf=ERR_ARG,
                octave_jump_cost_negative=ERR_ARG, octave_jump_cost_nan=ERR_ARG, voiced_unvoiced_cost_negative=ERR_ARG,
                voiced_unvoiced_cost_inf=ERR_ARG, zero_costs=OK, null_candidates=ERR_ARG, null_workspace=ERR_ARG,
                workspace_one_byte_short=ERR_WORKSPACE, no_outputs=OK, B0=OK, B0_batch_abs_sum="0", workspace_negative_B="0",
                workspace_null_lens="0", workspace_negative_len="0", workspace_B0="1", workspace_per_frame="8")
    assert got == want
    # the accepted call is the oracle's: the 200 Hz candidate throughout, and an utterance without candidates
    f = np.asarray([[200, 100], [200, 0], [201, 400]], np.float32)
    p = np.asarray([[0.9, 0.5], [0.8, 0], [0.9, 0.6]], np.float32)
    assert Q.path(f, p, 0.01).state.tolist() == [0, 0, 0]
