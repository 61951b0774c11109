"""CPU: the code of the loss-term kernels (csrc/losses.h: lt_terms, lt_combine and their host side) compiled for the host against the
stand-in of the HIP constructs it uses (tests/kernel_standin: one thread per lane, one workgroup at a time) and run on the edge batch
of tests/test_gpu_losses.py.  This checks the kernels' logic and every index they form without a GPU; what hipcc makes of the
arithmetic only tests/test_gpu_losses.py can see.

The bar: every sum within 1e-12 relative of the numpy float64 oracle (absolute floor 1e-300).  Derivation: both sides add the same
non-negative float64 terms (each difference is exact, |.| is exact, a square is rounded once on both sides), in different orders; a
reordered double sum of n non-negative terms moves by at most n 2^-53 relative.  The largest sum of the edge batch has
n = (6 (3 K + 9) - (6 K + 8)) 80 = 34,400 terms at K = 32 (the mel values of the pad frames), so n 2^-53 = 3.8e-12 is the worst case of
the bound -- but that is the bound for errors that all point the same way; the terms here are rounded to nearest, the expected
movement is sqrt(n) 2^-53 = 2e-14, and 1e-12 is held.  (log(ds + 1) may differ by an ulp between libm and numpy: 1e-16 relative of
a term, far below the bar.)

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import losses_oracle as O, standin_build
from tests.test_gpu_losses import K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_K_is_the_kernels_tile():
    src = open(os.path.join(ROOT, "fastspeech2_amd", "csrc", "losses.h")).read()
    assert int(re.search(r"constexpr int kLtFrames = (\d+);", src).group(1)) == K


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/losses_main.cpp")


@pytest.fixture(scope="module")
def edge():
    return O.Edge(K)


def _run(standin, tmp_path, e, pads, extra=()):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([e.B, e.odim, e.Tmax, e.Lmax, pads, e.psf, e.ysf, e.pst, e.dst, e.tsf], np.int32).tobytes())
        f.write(e.ilens.tobytes())
        f.write(e.olens.tobytes())
        for t in e.tensors():
            f.write(np.ascontiguousarray(t).tobytes())
    r = subprocess.run([standin, src, dst] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    out = np.frombuffer(open(dst, "rb").read(), np.float64).reshape(e.B + 1, O.TERMS)
    return out[:-1], out[-1]


def test_kernel_code_on_the_host_equals_the_oracle(standin, edge, tmp_path):
    assert edge.largest_n() == (6 * (3 * K + 9) - (6 * K + 8)) * 80          # the n of the docstring
    rows, batch = _run(standin, tmp_path, edge, 1)
    assert np.array_equal(rows[:, :4], edge.rows[:, :4]) and np.array_equal(batch[:4], edge.batch[:4])
    worst = np.max(np.abs(rows[:, 4:17] - edge.rows[:, 4:17]) / np.maximum(np.abs(edge.rows[:, 4:17]), 1e-300))
    print("worst relative difference of a sum: %.3g" % worst)
    assert O.close(rows, edge.rows) and O.close(batch, edge.batch)
    assert np.all(rows[:, 17:] == 0) and np.all(batch[17:] == 0)
    # pads = 0: the sums over [0, len) are the same bits, the pad sums are 0
    rows0, batch0 = _run(standin, tmp_path, edge, 0)
    assert np.array_equal(rows0[:, :12], rows[:, :12]) and np.all(rows0[:, 12:] == 0) and np.all(batch0[12:] == 0)
    assert np.array_equal(batch0[:12], batch[:12])
    # 4-byte loads (bases off a 16-byte boundary): the same values in the same order, so the same bits
    rows1, batch1 = _run(standin, tmp_path, edge, 1, ["misalign"])
    assert np.array_equal(rows1, rows) and np.array_equal(batch1, batch)


def test_host_side_argument_checks(standin):
    r = subprocess.run([standin, "--checks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    got = dict(line.split() for line in r.stdout.splitlines())
    OK, ERR_ARG, ERR_WORKSPACE = "0", "-1", "-5"                       # include/fs2.h
    want = dict(ok=OK, struct_size=ERR_ARG, negative_B=ERR_ARG, null_lens=ERR_ARG, negative_ilen=ERR_ARG, negative_olen=ERR_ARG,
                olen_above_Lmax=ERR_ARG, ilen_above_Tmax=ERR_ARG, Lmax_above_pred_stride=ERR_ARG, Lmax_above_y_stride=ERR_ARG,
                Lmax_above_tgt_stride=ERR_ARG, Tmax_above_pred_stride=ERR_ARG, Tmax_above_ds_stride=ERR_ARG, before_without_ys=ERR_ARG,
                d_outs_without_ds=ERR_ARG, es_without_e_outs=ERR_ARG, p_outs_without_ps=ERR_ARG, null_workspace=ERR_ARG,
                workspace_one_byte_short=ERR_WORKSPACE, all_groups_null=OK, nothing_asked=OK, B0=OK, B0_batch_abs_sum="0",
                workspace_negative_B="0", workspace_null_olens="0", workspace_negative_olen="0", workspace_B0="1")
    assert got == want
