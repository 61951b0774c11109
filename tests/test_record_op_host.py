"""CPU: the scaffold the record operators share (csrc/record_op.h: the record upload, the plain combine, the workspace carve) on the
host stand-in, on hand-made data (tests/kernel_standin/record_op_main.cpp), apart from any operator.

The combine rule, stated here in numpy without looking at the header.  The batch record of B records of TERMS doubles, column by
column, the records taken in index order (so the sums are sequential, and equal a Python loop's bit for bit):
  no flag column (fs2_op_dtw):  batch[c] = sum_b recs[b, c];
  flag column F (fs2_op_align: 2; fs2_op_pitch_path: 1): a record is fine iff recs[b, F] == 0.0;  batch[F] = the number of records that
  are not;  batch[c] = sum over the fine records, or for the maximum column (fs2_op_pitch_path: 5) their maximum, starting from 0.0.
The copy of the records is the records.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program: the sanitizer never sees the GPU)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import record_ops_sweep as sweep
from tests import standin_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBINE = {"dtw": (2, 12, None, None), "align": (3, 8, 2, None), "pitch_path": (4, 8, 1, 5)}      # op code, TERMS, flag column, maximum column
LT_FRAMES = 32                          # kLtFrames (tests/test_losses_kernel_host.py holds it to the header)


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/record_op_main.cpp")


def _exec(standin, *args):
    r = subprocess.run([standin] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def records(op, B):
    """B records of small distinct doubles (sums of them round, so the order of the additions shows); with a flag column records 1
    and 3 are flagged, the second with a code other than 1, and for the pitch path record 3 holds the largest column-5 value."""
    _, terms, flag, mx = COMBINE[op]
    r = (np.arange(B * terms, dtype=np.float64).reshape(B, terms) * 0.37 + 0.1) * (1.0 + 1e-9 * np.arange(B)[:, None])
    if flag is not None:
        r[:, flag] = 0.0
        r[1::2, flag] = [1.0, 2.0][:len(r[1::2])]
    if mx is not None and B > 3:
        r[3, mx] = 1e6
        r[2, mx] = 77.0                 # the largest among the fine records, and not the last of them
    return r


def batch_rule(op, r):
    _, terms, flag, mx = COMBINE[op]
    out = np.zeros(terms)
    for c in range(terms):
        s = 0.0
        for b in range(len(r)):
            fine = flag is None or r[b, flag] == 0.0
            if c == flag:
                s += 0.0 if fine else 1.0
            elif fine and c == mx:
                s = r[b, c] if r[b, c] > s else s
            elif fine:
                s += r[b, c]
        out[c] = s
    return out


@pytest.mark.parametrize("B", [0, 1, 5])
@pytest.mark.parametrize("op", sorted(COMBINE))
def test_combine_equals_the_rule_bit_for_bit(standin, tmp_path, op, B):
    code, terms, flag, mx = COMBINE[op]
    r = records(op, B)
    assert len(np.unique(r[:, [c for c in range(terms) if c != flag]])) == B * (terms - (flag is not None))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([code, B], np.int32).tobytes() + r.tobytes())
    _exec(standin, "--combine", src, dst)
    got = np.frombuffer(open(dst, "rb").read(), np.float64).reshape(B + 1, terms)
    want = batch_rule(op, r)
    assert np.array_equal(got[:B].view(np.uint64), r.view(np.uint64))
    assert np.array_equal(got[B].view(np.uint64), want.view(np.uint64)), (got[B], want)
    if B == 5:
        if flag is None:
            assert np.all(want > 0)
        else:
            assert want[flag] == 2 and np.all(want[[c for c in range(terms) if c != flag]] > 0)      # the flag branch ran, and left something
            assert not np.array_equal(want, r.sum(axis=0))
        if mx is not None:
            assert want[mx] == 77.0 and r[:, mx].max() == 1e6          # the flagged record's larger value is not the maximum
    if B == 0:
        assert not want.any()


@pytest.mark.parametrize("kind,N", [(0, 4), (1, 96)], ids=["two_ints", "pair_record"])
def test_upload_lands_every_record_once_at_its_index(standin, kind, N):
    for B in (0, N - 1, N, N + 1, 2 * N + 1):
        lines = _exec(standin, "--upload", kind, B)
        chunks = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("chunk")]
        assert chunks == [(base, min(N, B - base)) for base in range(0, B, N)], (B, chunks)          # ceil(B / N) launches that partition [0, B)
        assert lines[-1] == "landed 1"


def _up(x):
    return (x + 255) // 256 * 256


def _region_sizes(op, B, al, bl):
    nb, al = max(B, 1), al or []
    if op == "targets":
        return [8 * nb, 12 * 8 * nb]
    if op == "losses":
        return [16 * nb, 16 * 8 * max(sum(max(1, -(-v // LT_FRAMES)) for v in al[:B]), 1)]
    if op == "pitch_path":
        return [8 * 8 * nb, 8 * max(sum(al[:B]), 1)]
    return [40 * nb, (12 if op == "dtw" else 8) * 8 * nb]


@pytest.fixture(scope="module")
def swept(standin, tmp_path_factory):
    src = str(tmp_path_factory.mktemp("sweep") / "in.bin")
    cases = sweep.cases()
    with open(src, "wb") as f:
        f.write(sweep.pack(cases))
    rows = [[int(x) for x in ln.split()] for ln in _exec(standin, "--workspace", src)]
    assert len(rows) == len(cases)
    return cases, rows


def test_workspace_queries_equal_the_recorded_ones(swept):
    cases, rows = swept
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "record_ops_workspace_parent.json")))
    got = {op: [row[0] for c, row in zip(cases, rows) if c[0] == op] for op in sweep.OPS}
    assert {op: len(v) for op, v in want.items()} == {op: len(v) for op, v in got.items()}
    for op in sweep.OPS:
        assert got[op] == want[op], op
        assert len(got[op]) >= 199 and got[op].count(0) >= 1 and len(set(got[op])) > 40
    for op in ("dtw", "align"):          # the sweep reaches the three regimes of the cap: below `largest`, between, above `all`
        by_batch = {}
        for c, row in zip(cases, rows):
            if c[0] == op and row[0]:
                by_batch.setdefault((c[1], tuple(c[2] or ()), tuple(c[3] or ())), {})[c[4]] = row[0]
        full = [(v, v[0], v[1 << 62]) for v in by_batch.values() if 0 in v and 1 << 62 in v]      # (cap 0: `largest`; cap 2^62: `all`)
        assert any(lo < v[cap] == cap < hi for v, lo, hi in full for cap in v)
        assert any(lo < hi and v[cap] == lo and 0 < cap < lo for v, lo, hi in full for cap in v)
        assert any(v[cap] == hi and hi < cap < 1 << 62 for v, lo, hi in full for cap in v)


def test_carve_offsets_are_aligned_and_end_at_the_query(swept):
    cases, rows = swept
    served = 0
    for (op, B, al, bl, cap), (query, o0, o1, end) in zip(cases, rows):
        if query == 0:
            assert (o0, o1, end) == (-1, -1, -1)
            continue
        s0, s1 = _region_sizes(op, B, al, bl)
        assert (o0, o1, end) == (0, _up(s0), _up(_up(s0) + s1)) and o1 % 256 == 0 and end % 256 == 0, (op, B)
        if op in ("dtw", "align"):
            assert end <= query                 # the groups' matrices follow the two regions
        else:
            assert end == query
        served += 1
    assert served > 1000
