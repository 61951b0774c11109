"""CPU: the code of the excitation kernels (csrc/gl_excite.h: exc_upload, exc_plan, exc_prefix, exc_samples, exc_phase and the launch
sequences behind fs2_op_excitation_* / fs2_op_f0_phase_*) compiled for the host against the stand-in of the HIP constructs it uses
(tests/kernel_standin: one thread per lane, one workgroup at a time) and run on the cases of tests/excitation_oracle.py.  This checks the
kernels' logic and every index they form without a GPU; what hipcc makes of the arithmetic, and the float32 FFT of griffin_lim.h (the
stand-in's main transforms by the definition), only tests/test_gpu_excitation.py can see.

The bars come from the oracle's own float32 statement, never from the kernel (excitation_oracle.bars): 8 x its largest sample error
and 8 x its largest phasor error against the float64 statement; the factor allows the closed form the kernel evaluates the sum with.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import subprocess

import numpy as np
import pytest

from tests import excitation_oracle as E, standin_build

SR = E.SR


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/excitation_main.cpp", extra=("-ffp-contract=off",))


def run(standin, tmp_path, geom, f0, starts, lens, want, dev=False, stride=0, cap=0, seed=0, wav_stride=0, wav_cap=0, floor=71.0, ceil=800.0,
        expect=0):
    n_fft, hop, win = geom
    NB = n_fft // 2 + 1
    f0 = np.ascontiguousarray(f0, np.float32)
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(a, "wb") as f:
        f.write(np.asarray([n_fft, hop, win, len(lens), f0.size, int(dev), stride, cap, SR, seed, 2 if want == "phase" else 1, wav_stride, wav_cap,
                            0, 0, 0], np.int32).tobytes())
        f.write(np.asarray([floor, ceil], np.float64).tobytes())
        f.write(np.asarray(starts, np.int32).tobytes())
        f.write(np.asarray(lens, np.int32).tobytes())
        f.write(f0.tobytes())
    r = subprocess.run([standin, a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == expect and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    raw = np.frombuffer(open(b, "rb").read(), np.uint8)
    out = raw[:-16].view(np.float32)
    return (out.reshape(-1, NB) if want == "phase" else out), raw[-16:].view(np.int32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def utterances(f0, starts, lens):
    return [f0[s:s + n] for s, n in zip(starts, lens)]


def check_wav(wav, f0, starts, lens, hop, bar, seed=0):
    """max error of the packed waveform against the float64 statement; unvoiced samples are the hash's bits"""
    at, worst = 0, 0.0
    for u in utterances(f0, starts, lens):
        want = E.excitation(u, hop, SR, seed)
        got = wav[at:at + want.size]
        at += want.size
        if want.size:
            v = E.sample_phase(u, hop, SR)[3]
            assert same_bits(got[~v], want[~v].astype(np.float32))
            worst = max(worst, float(np.abs(got - want).max()))
    assert at == wav.size
    assert worst <= bar, (worst, bar)
    return worst


def check_phase(phase, f0, starts, lens, geom, bar):
    worst = 0.0
    cov = np.zeros(f0.size, bool)
    for s, n in zip(starts, lens):
        if n == 0:
            continue
        cov[s:s + n] = True
        want, X = E.f0_phase(f0[s:s + n], *geom, SR, return_stft=True)
        got = phase[s:s + n]
        assert np.all(np.isfinite(got)) and np.all(np.abs(got) <= np.float32(3.1415928))
        if n < geom[0] // (2 * geom[1]) + 2:
            assert np.all(got == 0.0)                   # N <= n_fft / 2: every row 0
        worst = max(worst, E.phasor_error(got, X, want))
    assert np.all(phase[~cov] == -777.0)
    assert worst <= bar, (worst, bar)
    return worst


@pytest.mark.parametrize("padded", [False, True])
def test_batch_at_the_default_geometry(standin, tmp_path, padded):
    geom = (1024, 256, 1024)
    f0, starts, lens = E.batch_case(padded=padded)
    ebar, pbar = E.bars(utterances(f0, starts, lens), *geom, SR)
    wav, hdr = run(standin, tmp_path, geom, f0, starts, lens, "wav")
    assert hdr[0] == sum(lens) and hdr[1] == 0 and hdr[2] == wav.size
    we = check_wav(wav, f0, starts, lens, geom[1], ebar)
    phase, _ = run(standin, tmp_path, geom, f0, starts, lens, "phase")
    wp = check_phase(phase, f0, starts, lens, geom, pbar)
    print("excitation: error %.3g, bar %.3g; phase: phasor error %.3g, bar %.3g" % (we, ebar, wp, pbar))
    # the device-driven sequence gives the same bits
    stride, cap = (max(lens) if padded else 0), f0.size
    wd, hd = run(standin, tmp_path, geom, f0, starts, lens, "wav", dev=True, stride=stride, cap=cap, wav_cap=wav.size)
    assert hd[1] == 0 and hd[0] == sum(lens) and same_bits(wd, wav)
    pd, hd = run(standin, tmp_path, geom, f0, starts, lens, "phase", dev=True, stride=stride, cap=cap)
    assert hd[1] == 0 and same_bits(pd, phase)
    # an utterance alone gives the bits it has in the batch
    b = lens.index(33)
    alone, _ = run(standin, tmp_path, geom, f0[starts[b]:starts[b] + 33], [0], [33], "phase")
    assert same_bits(alone, phase[starts[b]:starts[b] + 33])


@pytest.mark.parametrize("geom", [(512, 128, 512), (2048, 300, 1200)])
def test_the_other_geometries(standin, tmp_path, geom):
    f0, starts, lens = E.batch_case(lens=(1, 5, 33, 0, 9), seed=50)
    ebar, pbar = E.bars(utterances(f0, starts, lens), *geom, SR)
    wav, _ = run(standin, tmp_path, geom, f0, starts, lens, "wav", seed=7)
    we = check_wav(wav, f0, starts, lens, geom[1], ebar, seed=7)
    phase, _ = run(standin, tmp_path, geom, f0, starts, lens, "phase", seed=7)
    at, worst = 0, 0.0
    for s, n in zip(starts, lens):                      # (seed 7: the oracle's phase at that seed)
        if n:
            want, X = E.f0_phase(f0[s:s + n], *geom, SR, seed=7, return_stft=True)
            worst = max(worst, E.phasor_error(phase[s:s + n], X, want))
    assert worst <= pbar, (worst, pbar)
    print("%s excitation: error %.3g, bar %.3g; phase: phasor error %.3g, bar %.3g" % (geom, we, ebar, worst, pbar))


def test_padded_waveform_rows_and_the_seed(standin, tmp_path):
    geom = (512, 128, 512)
    f0, starts, lens = E.batch_case(lens=(5, 2, 33), padded=True, seed=60)
    ws = 128 * 32
    wav, hdr = run(standin, tmp_path, geom, f0, starts, lens, "wav", dev=True, stride=33, cap=99, wav_stride=ws, wav_cap=3 * ws)
    assert hdr[1] == 0
    for b, n in enumerate(lens):
        row = wav[b * ws:(b + 1) * ws]
        want = E.excitation(f0[starts[b]:starts[b] + n], 128, SR)
        assert np.abs(row[:want.size] - want).max() <= 1e-4 and np.all(row[want.size:] == -777.0)
    other, _ = run(standin, tmp_path, geom, f0, starts, lens, "wav", dev=True, stride=33, cap=99, wav_stride=ws, wav_cap=3 * ws, seed=1)
    v = np.concatenate([np.pad(E.sample_phase(f0[s:s + n], 128, SR)[3], (0, ws - 128 * (n - 1)), constant_values=True) for s, n in zip(starts, lens)])
    assert same_bits(other[v], wav[v]) and not np.any(other[~v] == wav[~v])          # the seed changes unvoiced samples only


@pytest.mark.parametrize("lens,stride,cap,wav_stride,wav_cap,flag",
                         [((4, -1, 3), 0, 16, 0, 4096, 64), ((9, 9), 0, 17, 0, 4352, 1), ((3, 7), 6, 12, 0, 3072, 2), ((3, 2 ** 31 - 1), 0, 12, 0, 3072, 1),
                          ((5, 6), 0, 12, 0, 2303, 128), ((5, 6), 0, 12, 1024, 2048, 128)])
def test_device_validation_writes_nothing(standin, tmp_path, lens, stride, cap, wav_stride, wav_cap, flag):
    f0 = np.full(cap, 200.0, np.float32)
    for want, kw in (("wav", dict(wav_stride=wav_stride, wav_cap=wav_cap)), ("phase", {})):
        if want == "phase" and flag == 128:
            continue
        out, hdr = run(standin, tmp_path, (1024, 256, 1024), f0, [0] * len(lens), lens, want, dev=True, stride=stride, cap=cap, **kw)
        assert hdr[1] & flag and hdr[0] == 0 and hdr[2] == 0
        assert np.all(out == -777.0)
