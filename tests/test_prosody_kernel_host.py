"""CPU: the code of the prosody kernels (csrc/prosody.h: prosody_apply, label_means and the host side of fs2_op_label_means) compiled
for the host against the stand-in of the HIP constructs it uses (tests/kernel_standin: one thread per lane, one workgroup at a time)
and run on the cases of tests/prosody_oracle.py.  This checks the kernels' logic and every index they form without a GPU; what hipcc
makes of the arithmetic only tests/test_gpu_prosody.py can see.

The bar: EQUALITY of bits with the numpy statements.  label_means adds the float32 values of a run in frame order in a double and
divides once; prosody_apply rounds a float32 product and then a float32 sum: numpy performs the same IEEE operations in the same
order, so nothing is left to differ.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import subprocess

import numpy as np
import pytest

from tests import prosody_oracle as P, standin_build


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/prosody_main.cpp")


def _exec(standin, args):
    r = subprocess.run([standin] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _means(standin, tmp_path, c, positive_only):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([P.B, c.S, c.Tmax, int(positive_only)], np.int32).tobytes())
        for a in (c.lens, c.x, c.labels):
            f.write(np.ascontiguousarray(a).tobytes())
    _exec(standin, ["means", src, dst])
    raw = open(dst, "rb").read()
    n = P.B * c.Tmax * 4
    assert len(raw) == 2 * n
    return np.frombuffer(raw[:n], np.float32).reshape(P.B, c.Tmax), np.frombuffer(raw[n:], np.int32).reshape(P.B, c.Tmax)


@pytest.mark.parametrize("S", P.STRIDES)
@pytest.mark.parametrize("Tmax", P.TMAXES)
def test_label_means_on_the_host_equal_the_oracle(standin, tmp_path, Tmax, S):
    c = P.means_case(Tmax, S)
    P.check_means_case(c)
    for positive_only in (False, True):
        mean, count = _means(standin, tmp_path, c, positive_only)
        want_mean, want_count = c.want[positive_only]
        assert np.array_equal(count, want_count)
        assert P.same_bits(mean, want_mean)


def test_oracle_of_the_means_on_a_case_done_by_hand():
    x = np.asarray([[1, 2, 3, 4, 5], [6, -7, 0, 9, 10]], np.float32)
    labels = np.asarray([[0, 0, 2, 2, 2], [1, 1, 1, 2, -1]], np.int32)
    mean, count = P.label_means(x, labels, [5, 4], 3, positive_only=True)
    assert count.tolist() == [[2, 0, 3], [0, 1, 1]] and mean.tolist() == [[1.5, 0, 4], [0, 6, 9]]
    mean, count = P.label_means(x, labels, [5, 4], 3)
    assert count.tolist() == [[2, 0, 3], [0, 3, 1]] and mean.tolist() == [[1.5, 0, 4], [0, np.float32(-1.0 / 3.0), 9]]
    # the sum is a double: 2^24 + 1 + 1 is exact there and is not in float32
    big = np.asarray([[2 ** 24, 1, 1]], np.float32)
    assert P.label_means(big, np.zeros((1, 3), np.int32), [3], 1)[0][0, 0] == np.float32((2.0 ** 24 + 2) / 3)


def test_prosody_apply_on_the_host_equals_the_oracle(standin, tmp_path):
    c = P.ApplyCase()
    gap, none = c.row_pos < 0, c.no_phoneme
    assert gap.sum() > 100 and c.R > 256 and np.all(c.row_pos[none] >= 0)
    for name, ctl in c.controls.items():
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.asarray([c.R, c.B, c.Tmax] + [0 if t is None else t.shape[1] for t in ctl], np.int32).tobytes())
            for a in (c.row_pos, c.row_seq, c.lri, c.p, c.e) + tuple(t for t in ctl if t is not None):
                f.write(np.ascontiguousarray(a).tobytes())
        _exec(standin, ["apply", src, dst])
        got = np.frombuffer(open(dst, "rb").read(), np.float32).reshape(2, c.R)
        want_p, want_e = c.oracle(name)
        assert P.same_bits(got[0], want_p) and P.same_bits(got[1], want_e), name
        for got_v, base, given in ((got[0], c.p, ctl[0] is not None or ctl[1] is not None), (got[1], c.e, ctl[2] is not None or ctl[3] is not None)):
            assert P.same_bits(got_v[gap], base[gap]) and P.same_bits(got_v[none], base[none]), name      # gap rows, rows without a phoneme
            touched = ~gap & (c.lri >= 0)
            assert np.any(got_v[touched] != base[touched]) == given, name                                  # a track without control is not written
    # the two roundings: somewhere in the case a fused multiply-add would have given another float
    ps, ph, _, _ = c.controls["mixed_a"]
    rows = np.flatnonzero((c.row_pos >= 0) & (c.lri >= 0))
    fused = np.asarray([np.float32(np.float64(c.p[r]) * np.float64(ps[c.row_seq[r], 0]) + np.float64(ph[c.row_seq[r], c.lri[r]])) for r in rows])
    assert np.any(fused != c.oracle("mixed_a")[0][rows])


def test_host_side_argument_checks(standin):
    got = dict(line.split() for line in _exec(standin, ["--checks"]).splitlines())
    OK, ERR_ARG = "0", "-1"                                             # include/fs2.h
    want = dict(ok=OK, ok_counts="203_011", ok_means="3,0,4_0,6,9", negative_B=ERR_ARG, negative_x_stride=ERR_ARG, negative_n_labels=ERR_ARG,
                null_x=ERR_ARG, null_labels=ERR_ARG, null_lens=ERR_ARG, null_mean=ERR_ARG, null_count=ERR_ARG, too_many_cells=ERR_ARG,
                B0_all_null=OK, n_labels_0_null_outputs=OK, x_stride_0_null_inputs=OK, x_stride_0_writes_zeros="1", bad_labels=OK,
                bad_labels_counts_in_range="1")
    assert got == want
