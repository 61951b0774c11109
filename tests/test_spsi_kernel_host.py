"""CPU: the code of the SPSI kernels (csrc/gl_spsi.h: spsi_upload, spsi_plan, spsi_analyse, spsi_chain and the launch sequences behind
fs2_op_spsi_phase_geom / _dev) compiled for the host against the stand-in of the HIP constructs it uses (tests/kernel_standin: one
thread per lane, one workgroup at a time) and run on the cases of tests/spsi_oracle.py.  This checks the kernels' logic and every
index they form without a GPU; what hipcc makes of the arithmetic only tests/test_gpu_spsi.py can see.

The bar: EQUALITY of bits of the phase with the numpy statement (each float32 operation rounded on its own in both).

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import subprocess

import numpy as np
import pytest

from tests import spsi_oracle as S, standin_build


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/spsi_main.cpp", extra=("-ffp-contract=off",))


def run(standin, tmp_path, n_fft, hop, src, starts, lens, pinv=None, dev=False, stride=0, cap=0, expect=0):
    NB = n_fft // 2 + 1
    src = np.ascontiguousarray(src, np.float32)
    rows, width = src.shape
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(a, "wb") as f:
        f.write(np.asarray([n_fft, hop, width, len(lens), rows, int(dev), stride, cap], np.int32).tobytes())
        f.write(np.asarray(starts, np.int32).tobytes())
        f.write(np.asarray(lens, np.int32).tobytes())
        f.write(src.tobytes())
        if pinv is not None:
            f.write(np.ascontiguousarray(pinv, np.float32).tobytes())
    r = subprocess.run([standin, a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == expect and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    raw = open(b, "rb").read()
    n = rows * NB * 4
    assert len(raw) == 2 * n + 16
    return (np.frombuffer(raw[:n], np.float32).reshape(rows, NB), np.frombuffer(raw[n:2 * n], np.float32).reshape(rows, NB),
            np.frombuffer(raw[2 * n:], np.int32))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def covered(rows, starts, lens):
    m = np.zeros(rows, bool)
    for s, n in zip(starts, lens):
        m[s:s + n] = True
    return m


@pytest.mark.parametrize("padded", [False, True])
def test_batch_at_513_bins_equals_the_oracle(standin, tmp_path, padded):
    src, starts, lens = S.batch_case(513, padded=padded)
    want = S.spsi_batch(src, starts, lens, 1024, 256)
    phase, mag, hdr = run(standin, tmp_path, 1024, 256, src, starts, lens)
    cov = covered(src.shape[0], starts, lens)
    assert hdr[0] == sum(lens) and hdr[1] == 0
    assert same_bits(phase[cov], want[cov]) and np.all(phase[~cov] == -777.0)
    assert same_bits(mag[cov], src[cov]) and np.all(mag[~cov] == -777.0)
    # the device-driven sequence gives the same bits
    Lmax = max(lens)
    pd, md, hd = run(standin, tmp_path, 1024, 256, src, starts, lens, dev=True, stride=Lmax if padded else 0, cap=src.shape[0])
    assert hd[1] == 0 and same_bits(pd, phase) and same_bits(md, mag)


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (2048, 300)])
def test_one_utterance_of_each_at_the_other_geometries(standin, tmp_path, n_fft, hop):
    NB = n_fft // 2 + 1
    for L in S.BATCH_LENS:
        if L == 0:
            continue
        src, starts, lens = S.batch_case(NB, lens=(L,), seed=40 + L)
        if L >= 10:
            src[:10] = S.crafted_utterance(NB)
        phase, _, _ = run(standin, tmp_path, n_fft, hop, src, starts, lens)
        assert same_bits(phase, S.spsi_batch(src, starts, lens, n_fft, hop)), L


def test_mel_rows_give_the_magnitudes_and_their_phase(standin, tmp_path):
    rs = np.random.RandomState(3)
    n_fft, hop, nm, NB = 512, 128, 20, 257
    lens = [5, 0, 18]
    starts = [0, 5, 5]
    mel = (rs.randn(23, nm) * 1.5 - 2.0).astype(np.float32)
    pinv = (rs.randn(NB, nm) * 0.3 + 0.1).astype(np.float32)
    phase, mag, _ = run(standin, tmp_path, n_fft, hop, mel, starts, lens, pinv=pinv)
    want = np.maximum(np.exp(mel.astype(np.float64)) @ pinv.astype(np.float64).T, 0.0)
    bound = 1e-5 * (np.exp(mel.astype(np.float64)) @ np.abs(pinv.astype(np.float64)).T)
    assert np.all(np.abs(mag - want) <= bound)
    assert same_bits(phase, S.spsi_batch(mag, starts, lens, n_fft, hop))
    again, _, _ = run(standin, tmp_path, n_fft, hop, mag, starts, lens)
    assert same_bits(again, phase)


@pytest.mark.parametrize("lens,stride,cap,flag", [((4, -1, 3), 0, 16, 64), ((9, 9), 0, 17, 1), ((3, 7), 6, 12, 2), ((3, 2 ** 31 - 1), 0, 12, 1)])
def test_device_validation_writes_nothing(standin, tmp_path, lens, stride, cap, flag):
    src = S.random_rows(cap, 513, 2)
    phase, mag, hdr = run(standin, tmp_path, 1024, 256, src, [0] * len(lens), lens, dev=True, stride=stride, cap=cap)
    assert hdr[1] & flag and hdr[0] == 0
    assert np.all(phase == -777.0) and np.all(mag == -777.0)
