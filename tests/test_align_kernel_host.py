"""CPU: the code of the alignment kernels (csrc/align.h: align_sweep, records_combine<8, 2, -1> and their host side, with dtw_dist of csrc/dtw.h
on the swapped sides) compiled for the host against the stand-in of the HIP constructs it uses (tests/kernel_standin: one thread per
lane, one workgroup at a time) and run on the edge batch of tests/test_gpu_align.py.  This checks the kernels' logic -- the swapped
matrix, what is read after which barrier, the walk back and its counts, the grouping -- and every index they form without a GPU;
what hipcc makes of the arithmetic only tests/test_gpu_align.py can see.

The bar: EQUALITY of bits with the numpy float64 oracle, for the records, ``state`` and ``durations``.  Both sides perform the same
IEEE double operations in the same order (tests/test_dtw_kernel_host.py gives the reasons for d; Q adds one d per frame to the
chosen predecessor), so nothing is left to differ.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import align_oracle as A, standin_build
from tests.test_gpu_align import T, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 1 << 40


def test_W_and_T_are_the_kernels():
    csrc = os.path.join(ROOT, "fastspeech2_amd", "csrc")
    assert int(re.search(r"constexpr int kAlignThreads = (\d+);", open(os.path.join(csrc, "align.h")).read()).group(1)) == W
    assert int(re.search(r"constexpr int kDtwTile = (\d+);", open(os.path.join(csrc, "dtw.h")).read()).group(1)) == T
    unroll = int(re.search(r"constexpr int kAlignUnroll = (\d+);", open(os.path.join(csrc, "align.h")).read()).group(1))
    assert 2 * W < 2 * W + 3 <= unroll * W                      # the longest row of the edge batch: a third state for some threads, inside one pass
    assert A.edge_shapes(W, T) == [(1, 1), (1, 5), (2, 1), (3, 2), (5, 2), (2, 2), (T - 1, T + 1), (T + 1, T), (W - 1, W), (W, W + 1),
                                   (W + 1, W // 2 + 1), (2 * W + 3, W + 40), (40, 2 * W + 1), (0, 5), (5, 0)]


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/align_main.cpp")


_edges = {}


def edge(D):
    if D not in _edges:
        _edges[D] = A.Edge(W, T, D)
    return _edges[D]


def _run(standin, tmp_path, e, cap, S, labels, keep=None):
    """The pairs ``keep`` (default: all) of an A.Edge, read in place from its packed arrays through their row offsets
    -> (rows, batch, durations [len(keep), dur_stride], state [rows of b])."""
    keep = list(range(len(e.shapes))) if keep is None else keep
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int64(cap).tobytes())
        f.write(np.asarray([len(keep), e.D, e.D, e.D, len(e.a), len(e.b), S, int(labels), e.dur_stride], np.int32).tobytes())
        for x in (e.a_starts[keep], e.a_lens[keep], e.b_starts[keep], e.b_lens[keep], e.n_labels[keep], e.a, e.b):
            f.write(np.ascontiguousarray(x).tobytes())
        if labels:
            f.write(np.ascontiguousarray(e.labels).tobytes())
    r = subprocess.run([standin, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    n = (len(keep) + 1) * A.TERMS * 8
    out = np.frombuffer(raw[:n], np.float64).reshape(len(keep) + 1, A.TERMS)
    dur = np.frombuffer(raw[n:n + len(keep) * e.dur_stride * 8], np.int64).reshape(len(keep), e.dur_stride)
    state = np.frombuffer(raw[n + dur.nbytes:], np.int32)
    assert len(state) == len(e.b)
    return out[:-1], out[-1], dur, state


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _state_of(e, state, keep):
    """The frames of the pairs ``keep`` out of a state array over all rows of b (the others were never written: -777)."""
    return np.concatenate([state[e.b_starts[n]:e.b_starts[n] + e.b_lens[n]] for n in keep] + [np.zeros(0, np.int32)])


def _assert_equal(e, got, S, labels, keep=None):
    keep = list(range(len(e.shapes))) if keep is None else keep
    rows, batch, dur, state = got
    res, want_rows, _, want_dur, want_state = e.oracle(S, labels)
    assert _bits(rows, want_rows[keep])
    assert _bits(batch, A.records([res[n] for n in keep])[1])
    assert np.array_equal(dur, want_dur[keep])
    assert np.array_equal(_state_of(e, state, keep), _state_of(e, want_state, keep))
    untouched = np.ones(len(state), bool)
    for n in keep:
        untouched[e.b_starts[n]:e.b_starts[n] + e.b_lens[n]] = False
    assert np.all(state[untouched] == -777)                                 # nothing outside the pairs' own rows


@pytest.mark.parametrize("S", [1, 2])
def test_kernel_code_on_the_host_equals_the_oracle(standin, tmp_path, S):
    e = edge(3)
    want = e.oracle(S, False)[1]
    infeasible = [n for n, (N, M) in enumerate(e.shapes) if not A.feasible(N, M, S)]
    assert infeasible == ([2, 4, 13, 14] if S == 2 else [2, 3, 4, 7, 10, 11, 13, 14]) and np.all(want[infeasible, A.FLAGS] == 1)
    assert np.all(np.delete(want[:, A.FLAGS], infeasible) == 0)
    if S == 2:                                                              # the tight pairs: every frame advances by two states
        for n in (3, 10):
            assert want[n, A.STATES_USED] == e.shapes[n][1] and want[n, A.LONGEST_STAY] == 1
    for labels in (False, True):
        _assert_equal(e, _run(standin, tmp_path, e, ALL, S, labels), S, labels)
        res = e.oracle(S, labels)[0]
        assert all(r.durations.sum() == e.shapes[n][1] for n, r in enumerate(res) if r.record[A.FLAGS] == 0)
    assert any(r.record[A.EMPTY_LABELS] > 0 for r in e.oracle(S, True)[0])
    # a feature width beyond one staging pass of dtw_dist, on the pairs around the tile and the thread count
    e80 = edge(80)
    keep = [0, 3, 5, 6, 7, 8, 9, 10]
    _assert_equal(e80, _run(standin, tmp_path, e80, ALL, S, True, keep=keep), S, True, keep)


def test_groups_on_the_host(standin, tmp_path):
    e = edge(3)
    keep = [9, 12, 4, 0, 13, 14, 2, 11, 6, 3, 10]                # another order, the empty and the infeasible pairs in the middle
    one_per_group = _run(standin, tmp_path, e, 0, 2, True, keep=keep)
    _assert_equal(e, one_per_group, 2, True, keep)
    sizes = sorted(8 * N * M for N, M in (e.shapes[n] for n in keep))
    cap = sizes[-1] + sizes[-2] + 4096                            # the two largest matrices fit together, all of them do not: groups of several
    assert cap < sum(sizes)
    some = _run(standin, tmp_path, e, cap, 2, True, keep=keep)
    _assert_equal(e, some, 2, True, keep)
    assert _bits(some[0], one_per_group[0]) and _bits(some[1], one_per_group[1])


def test_host_side_argument_checks(standin):
    r = subprocess.run([standin, "--checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    got = dict(line.split() for line in r.stdout.splitlines())
    OK, ERR_ARG, ERR_WORKSPACE = "0", "-1", "-5"                       # include/fs2.h
    want = dict(ok=OK, ok_flags="10", ok_durations="00000_10300", ok_state="-1-1_0222", struct_size=ERR_ARG, negative_B=ERR_ARG, null_lens=ERR_ARG,
                null_starts=ERR_ARG, negative_len=ERR_ARG, negative_start=ERR_ARG, D_0=ERR_ARG, D_129=ERR_ARG, max_step_0=ERR_ARG, max_step_3=ERR_ARG,
                stride_below_D=ERR_ARG, n_labels_negative=ERR_ARG, n_labels_above_dur_stride=ERR_ARG, n_labels_at_dur_stride=OK,
                labels_without_n_labels=ERR_ARG, n_labels_without_labels=ERR_ARG, no_labels=OK, no_labels_dur_stride_below_N=ERR_ARG,
                null_a=ERR_ARG, null_workspace=ERR_ARG, workspace_one_byte_short=ERR_WORKSPACE, no_outputs=OK, bad_labels=OK,
                bad_labels_rows_written_whole="1", B0=OK, B0_batch_abs_sum="0", workspace_negative_B="0", workspace_null_lens="0",
                workspace_negative_len="0", workspace_too_many_cells="0", workspace_B0="1", workspace_cap_between="1")
    assert got == want
