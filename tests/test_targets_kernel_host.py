"""CPU: the code of the target-cleaning kernels (csrc/targets.h: tg_clean, tg_combine and their host side) compiled for the host
against a stand-in of the HIP constructs it uses (tests/kernel_standin: one thread per lane, one workgroup at a time) and run on the
whole edge batch of tests/test_gpu_targets.py: every cleaned value, quartile and outlier count equals the oracle, out of place and in
place.  This checks the kernels' logic without a GPU; what hipcc makes of the arithmetic (contraction) only tests/test_gpu_targets.py
can see.  Built with -fsanitize=thread when FS2_STANDIN_TSAN=1 (slower; finds an LDS word reused without a barrier)."""
import struct
import subprocess

import numpy as np
import pytest

from fastspeech2_amd.targets import TargetStats
from tests import standin_build
from tests.test_gpu_targets import Edge, _many_utterances, _same, _stats_close


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/targets_main.cpp", tsan=True)


@pytest.fixture(scope="module")
def edge():
    return Edge()


def test_more_utterances_than_an_upload_chunk(standin, tmp_path):
    """501 utterances of 0 .. 3 values: record 500 travels alone in a second upload launch."""
    many = Edge(_many_utterances())
    assert len(many.utts) == 501 and many.lens[500] == 3 and max(many.lens) == 3
    _run_and_compare(standin, many, tmp_path, False)


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_kernel_code_on_the_host_equals_the_oracle(standin, edge, tmp_path, inplace):
    _run_and_compare(standin, edge, tmp_path, inplace)


def _run_and_compare(standin, edge, tmp_path, inplace):
    B, total = len(edge.utts), sum(edge.lens)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", B))
        f.write(np.asarray(edge.lens, np.int32).tobytes())
        f.write(np.concatenate(edge.utts).astype(np.float32).tobytes())
    r = subprocess.run([standin, src, dst] + (["inplace"] if inplace else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    y = np.frombuffer(raw[:4 * total], np.float32)
    q = np.frombuffer(raw[4 * total:4 * total + 8 * B], np.float32).reshape(B, 2)
    no = np.frombuffer(raw[4 * total + 8 * B:4 * total + 12 * B], np.int32)
    stats = TargetStats.from_record(np.frombuffer(raw[4 * total + 12 * B:], np.float64).tolist())
    off = np.concatenate([[0], np.cumsum(edge.lens)])
    for i, (name, c) in enumerate(zip(edge.names, edge.cleaned)):
        assert _same(y[off[i]:off[i + 1]], c.y), name
        assert _same(q[i], [c.p25, c.p75]), (name, q[i], c.p25, c.p75)
        assert no[i] == c.n_outliers, (name, no[i], c.n_outliers)
    _stats_close(stats, edge.stats)
