"""CPU: the oracle of the forced alignment (tests/align_oracle.py) against a brute-force enumeration of every admissible state
sequence, its column-wise form against its cell-by-cell form (equality of bits), the tie rule on constructed exact ties, and the
properties every alignment has: the durations add up to the frames, the states are monotone with steps of at most max_step."""
import numpy as np
import pytest

from tests import align_oracle as A
from tests import dtw_oracle as O


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _same(x, y):
    return _bits(x.record, y.record) and np.array_equal(x.state, y.state) and np.array_equal(x.durations, y.durations)


@pytest.mark.parametrize("S", [1, 2])
def test_oracle_equals_brute_force(S):
    rng = np.random.default_rng(40 + S)
    for N in range(0, 6):
        for M in range(0, 7):
            a, b = O.warped_pair(rng, N, M, 3)[:2]
            got = A.align(a, b, max_step=S)
            ok = N >= 1 and M >= 1 and N - 1 <= S * (M - 1)
            assert A.feasible(N, M, S) == ok
            if N == 0 or M == 0:
                assert got.record[A.FLAGS] == 1 and np.all(got.record[3:] == 0) and np.all(got.state == -1) and not got.durations.any()
                continue
            best, arg = A.brute_force(O.dist(a, b), S)
            assert (best is not None) == ok, (N, M)                        # an admissible sequence exists exactly when the formula says so
            if not ok:
                assert got.record[A.FLAGS] == 1 and got.record[A.COST] == 0 and np.all(got.state == -1) and not got.durations.any()
                assert np.array_equal(got.record[:2], [N, M])
                continue
            assert got.record[A.FLAGS] == 0 and abs(got.record[A.COST] - best) <= 1e-12 * best, (N, M)
            assert np.array_equal(got.state, arg), (N, M)                   # (random data: the minimum is unique)
            assert _same(got, A.align_fast(a, b, max_step=S))


@pytest.mark.parametrize("S", [1, 2])
def test_column_form_equals_cell_form_and_properties(S):
    rng = np.random.default_rng(50 + S)
    for N, M, D in ((1, 1, 2), (1, 9, 2), (7, 7, 1), (12, 31, 5), (31, 17, 5), (33, 17, 3), (40, 64, 80), (64, 40, 13)):
        a, b = O.warped_pair(rng, N, M, D)[:2]
        labels, nl = A.random_labels(rng, N)
        for lab, n in ((None, None), (labels, nl)):
            slow, fast = A.align(a, b, lab, n, S), A.align_fast(a, b, lab, n, S)
            assert _same(slow, fast), (N, M, D)
            r = fast.record
            if not A.feasible(N, M, S):
                assert r[A.FLAGS] == 1 and not fast.durations.any()
                continue
            assert r[A.FLAGS] == 0 and fast.durations.sum() == M and len(fast.durations) == (N if lab is None else n)
            steps = np.diff(fast.state)
            assert fast.state[0] == 0 and fast.state[-1] == N - 1 and steps.min(initial=0) >= 0 and steps.max(initial=0) <= S
            cost = np.float64(0)
            d = O.dist(a, b)
            for j in range(M):                                             # the cost is the sum along the path, in frame order
                cost = cost + d[fast.state[j], j]
            assert cost == r[A.COST]
            used = len(np.unique(fast.state))
            assert r[A.STATES_USED] == used and r[A.EMPTY_LABELS] == (fast.durations == 0).sum()
            assert r[A.LONGEST_STAY] == np.bincount(fast.state).max()
            if lab is None:
                assert np.array_equal(fast.durations, np.bincount(fast.state, minlength=N)) and r[A.EMPTY_LABELS] == N - used
            else:
                assert np.array_equal(fast.durations, np.bincount(lab[fast.state], minlength=n))


def test_tie_rule():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (9, 4)).astype(np.float32)
    for S in (1, 2):
        same = A.align(x, x, max_step=S)                                   # a = b: the diagonal, cost 0 (a tie of zeros keeps k = 0
        assert np.array_equal(same.state, np.arange(9)) and same.record[A.COST] == 0      # only where the diagonal is not cheaper: d > 0 off it)
        assert np.all(same.durations == 1) and same.record[A.STATES_USED] == 9 and same.record[A.LONGEST_STAY] == 1 and same.record[A.EMPTY_LABELS] == 0
        rep = A.align(x, np.repeat(x, 3, axis=0), max_step=S)              # every frame three times: three frames per state
        assert np.all(rep.durations == 3) and rep.record[A.COST] == 0 and rep.record[A.LONGEST_STAY] == 3
    # constant features: every d is the same c, every finite Q(i, j) is (j + 1) c exactly (c = 3: small integers), so every
    # comparison between finite predecessors is a tie and keeps k = 0: walking back from (N-1, M-1) the state stays N-1 for as long
    # as a predecessor in the same state is finite, that is, down to frame ceil((N-1) / S); below that the forced advance
    a, b = np.full((5, 1), 1.0, np.float32), np.full((11, 1), 4.0, np.float32)
    one = A.align(a, b, max_step=1)
    assert np.array_equal(one.state, [0, 1, 2, 3] + [4] * 7) and one.record[A.COST] == 33 and one.record[A.LONGEST_STAY] == 7
    two = A.align(a, b, max_step=2)
    assert np.array_equal(two.state, [0, 2] + [4] * 9) and two.record[A.COST] == 33 and two.record[A.STATES_USED] == 3
    assert np.array_equal(two.durations, [1, 0, 1, 0, 9]) and two.record[A.EMPTY_LABELS] == 2
    assert _same(one, A.align_fast(a, b, max_step=1)) and _same(two, A.align_fast(a, b, max_step=2))


def test_non_finite_costs_and_records():
    rng = np.random.default_rng(4)
    a, b = O.warped_pair(rng, 6, 9, 3)[:2]
    bad = b.copy()
    bad[4, 1] = np.nan                                                     # a frame of the recording: every path passes through it
    for f in (A.align, A.align_fast):
        r = f(a, bad, max_step=2)
        assert r.record[A.FLAGS] == 2 and np.isnan(r.record[A.COST]) and np.all(r.state == -1) and not r.durations.any()
        assert np.all(r.record[4:] == 0) and np.array_equal(r.record[:2], [6, 9])
    res = [A.align_fast(a, b), A.align_fast(a, bad), A.align_fast(a, b[:2]), A.align_fast(b, a)]
    rows, batch = A.records(res)
    assert [int(r[A.FLAGS]) for r in rows] == [0, 2, 1, 0] and batch[A.FLAGS] == 2
    others = [i for i in range(A.TERMS) if i != A.FLAGS]
    assert _bits(batch[others], (rows[0] + rows[3])[others])
    assert A.min_gap(res[0].Q, 2) > 0 and A.min_gap(np.zeros((1, 4)), 2) == np.inf


def test_alignment_class_on_the_host():
    """fastspeech2_amd.align.Alignment from host arrays: the derived numbers and merge (no GPU, no library call)."""
    import torch
    from fastspeech2_amd import Alignment, monotonic_align, FeedForwardTransformer
    rng = np.random.default_rng(5)
    res = [A.align_fast(*O.warped_pair(rng, N, M, 4)[:2]) for N, M in ((6, 9), (9, 3), (5, 5))]
    rows, batch = A.records(res)
    dur = np.zeros((3, 9), np.int64)
    for n, r in enumerate(res):
        dur[n, :len(r.durations)] = r.durations
    al = Alignment(torch.from_numpy(dur), None, rows, batch, "mel", 4)
    assert len(al) == 3 and al.ok.tolist() == [True, False, True]
    pu = al.per_utterance()
    assert pu["flags"].tolist() == [0, 1, 0] and pu["longest_stay"].tolist() == [int(r.record[A.LONGEST_STAY]) for r in res]
    assert _bits(pu["cost_per_frame"][[0, 2]], rows[[0, 2], A.COST] / rows[[0, 2], A.M_]) and np.isnan(pu["cost_per_frame"][1])
    assert _bits(pu["length_ratio"], rows[:, 0] / rows[:, 1])
    assert pu["states_skipped"].tolist() == [6 - int(rows[0, A.STATES_USED]), 0, 5 - int(rows[2, A.STATES_USED])]
    assert pu["empty_labels"].tolist() == [int(r[A.EMPTY_LABELS]) for r in rows]
    both = al.merge(Alignment(torch.from_numpy(dur[:1, :7]), None, rows[:1], A.records(res[:1])[1], "mel", 4))
    assert len(both) == 4 and both.durations.shape == (4, 9) and torch.equal(both.durations[3], both.durations[0])
    assert both.batch[A.FLAGS] == 1 and _bits(both.batch[A.COST], batch[A.COST] + rows[0, A.COST])
    with pytest.raises(ValueError, match="features"):
        al.merge(Alignment(torch.from_numpy(dur), None, rows, batch, "mcep", 4))
    z = torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monotonic_align(z, [2], z, [2])
    assert callable(FeedForwardTransformer.align_durations)


def test_ctypes_mirror_of_the_argument_struct_matches_the_compiled_header(tmp_path):
    """fs2_op_align_args as gcc sees include/fs2.h: sizeof and the offset of every field equal those of _lib.OpAlignArgs."""
    import ctypes
    import os
    import re
    import subprocess
    from fastspeech2_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in _lib.OpAlignArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fs2.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(fs2_op_align_args));', '  printf("FS2_ALIGN_TERMS %d\\n", FS2_ALIGN_TERMS);',
           '  printf("FS2_ABI_VERSION %d\\n", FS2_ABI_VERSION);']
    src += ['  printf("%s %%zu\\n", offsetof(fs2_op_align_args, %s));' % (f, f) for f in fields] + ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", exe], check=True)
    probe = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert probe["sizeof"] == ctypes.sizeof(_lib.OpAlignArgs) == _lib.OpAlignArgs().struct_size
    assert probe["FS2_ALIGN_TERMS"] == _lib.ALIGN_TERMS == A.TERMS
    assert probe["FS2_ABI_VERSION"] == _lib.ABI_VERSION == 4                # the addition is additive
    for f in fields:
        assert getattr(_lib.OpAlignArgs, f).offset == probe[f], f
    hdr = open(os.path.join(root, "include", "fs2.h")).read()
    body = hdr[hdr.index("struct fs2_op_align_args {"):hdr.index("typedef struct fs2_op_align_args")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[*\s,](\w+)\s*[,;]", body[body.index("{"):])
    assert declared == fields, (declared, fields)
