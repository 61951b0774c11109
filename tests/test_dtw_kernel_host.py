"""CPU: the code of the DTW kernels (csrc/dtw.h: dtw_dist, dtw_sweep, records_combine<12, -1, -1> and their host side) compiled for the host against
the stand-in of the HIP constructs it uses (tests/kernel_standin: one thread per lane, one workgroup at a time) and run on the edge
batch of tests/test_gpu_dtw.py.  This checks the kernels' logic -- the skewed sweep, what travels through the rings and the edge
buffers after which barrier, the grouping -- and every index they form without a GPU; what hipcc makes of the arithmetic only
tests/test_gpu_dtw.py can see.

The bar: EQUALITY of bits with the numpy float64 oracle.  Both sides perform the same IEEE double operations in the same order (the
differences, one multiply and one add per feature in increasing order, a correctly rounded sqrt, the sums in path order); on the host
there is no fused multiply-add to contract into (x86-64 baseline) and libm's sqrt is correctly rounded, so nothing is left to differ.
The stand-in moves a cell's record to the next lane in one exchange (kernel_standin/hip_standin_record.h) where the device shuffles
its seven fields one by one: fourteen waits at a barrier of 64 host threads per step made this test take minutes.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dtw_oracle as O, standin_build
from tests.test_gpu_dtw import T, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 1 << 40


def test_W_and_T_are_the_kernels():
    src = open(os.path.join(ROOT, "fastspeech2_amd", "csrc", "dtw.h")).read()
    assert int(re.search(r"constexpr int kDtwCols = (\d+);", src).group(1)) == W
    assert int(re.search(r"constexpr int kDtwTile = (\d+);", src).group(1)) == T
    lag = int(re.search(r"constexpr int kDtwLag = (\d+);", src).group(1))
    assert 40 < (W - 1) + 3 * (lag - 1) < 2 * W + 1          # the edge batch's short sides end before, its long sides after the sweep's skew


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/dtw_main.cpp")


def _run(standin, tmp_path, e, cap, tracks=True, keep=None):
    """The pairs ``keep`` (default: all) of an O.Edge, read in place from its packed arrays through their row offsets."""
    keep = list(range(len(e.shapes))) if keep is None else keep
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int64(cap).tobytes())
        f.write(np.asarray([len(keep), e.D, e.D, e.D, len(e.a), len(e.b), int(tracks)], np.int32).tobytes())
        for x in (e.a_starts[keep], e.a_lens[keep], e.b_starts[keep], e.b_lens[keep], e.a, e.b):
            f.write(np.ascontiguousarray(x).tobytes())
        if tracks:
            for x in (e.e_a, e.e_b, e.p_a, e.p_b):
                f.write(np.ascontiguousarray(x).tobytes())
    r = subprocess.run([standin, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    out = np.frombuffer(open(dst, "rb").read(), np.float64).reshape(len(keep) + 1, O.TERMS)
    return out[:-1], out[-1]


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_kernel_code_on_the_host_equals_the_oracle(standin, tmp_path):
    e = O.Edge(W, T, 3)
    rows, batch = _run(standin, tmp_path, e, ALL)
    assert _bits(rows, e.rows) and _bits(batch, e.batch)
    # a feature width beyond one staging pass of dtw_dist, on the pairs around the tile and the column block
    e80 = O.Edge(W, T, 80)
    keep = [0, 3, 4, 5, 10, 11]
    rows80, batch80 = _run(standin, tmp_path, e80, ALL, keep=keep)
    assert _bits(rows80, e80.rows[keep])
    in_order = np.zeros(O.TERMS)
    for r in e80.rows[keep]:
        in_order = in_order + r
    assert _bits(batch80, in_order)


def test_groups_and_missing_tracks_on_the_host(standin, tmp_path):
    e = O.Edge(W, T, 3)
    keep = [4, 10, 0, 1, 11, 5, 3]                        # another order, the empty pairs in the middle; the short pairs, to stay quick
    one_per_group, batch = _run(standin, tmp_path, e, 0, keep=keep)
    assert _bits(one_per_group, e.rows[keep])
    some, batch2 = _run(standin, tmp_path, e, 40000, keep=keep)           # the two 32 KB matrices do not fit together: two groups of several
    assert _bits(some, e.rows[keep]) and _bits(batch2, batch)
    bare, _ = _run(standin, tmp_path, e, ALL, tracks=False, keep=keep)
    assert _bits(bare[:, :4], e.rows[keep, :4]) and np.all(bare[:, 4:] == 0)


def test_host_side_argument_checks(standin):
    r = subprocess.run([standin, "--checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    got = dict(line.split() for line in r.stdout.splitlines())
    OK, ERR_ARG, ERR_WORKSPACE = "0", "-1", "-5"                       # include/fs2.h
    want = dict(ok=OK, ok_steps="8", struct_size=ERR_ARG, negative_B=ERR_ARG, null_lens=ERR_ARG, null_starts=ERR_ARG, negative_len=ERR_ARG,
                negative_start=ERR_ARG, D_0=ERR_ARG, D_129=ERR_ARG, stride_below_D=ERR_ARG, e_a_without_e_b=ERR_ARG, p_b_without_p_a=ERR_ARG,
                null_a=ERR_ARG, null_workspace=ERR_ARG, workspace_one_byte_short=ERR_WORKSPACE, no_tracks=OK, nothing_asked=OK, B0=OK,
                B0_batch_abs_sum="0", workspace_negative_B="0", workspace_null_lens="0", workspace_negative_len="0",
                workspace_too_many_cells="0", workspace_B0="1", workspace_cap_between="1")
    assert got == want
