"""Host-side checks of the pair plan (no GPU): csrc/pair_plan.h -- the layout, the records and the groups that fs2_op_dtw and
fs2_op_align launch from -- compiled with the host compiler (tests/pair_plan_probe.cpp runs the operators' checks and the plan on lengths
alone; nothing is allocated for the matrices, so a batch of terabytes is arithmetic).  The rule is stated here once more, in Python,
without looking at the header:

  bytes of a pair (N, M):  0 if N M = 0, else align_up(8 N M, 256), plus align_up(2 N 48, 256) for fs2_op_dtw when M > 256;
  tiles of a pair:         0 if N M = 0, else ceil(rows / 64) ceil(cols / 64) of the matrix as dtw_dist writes it: [N, M] for fs2_op_dtw,
                           [M, N] for fs2_op_align (the sides swapped);
  layout:                  off_terms = align_up(max(B, 1) 40, 256), off_group = align_up(off_terms + max(B, 1) TERMS 8, 256);
  workspace bytes:         min(off_group + all pairs, max(cap, off_group + the largest pair));
  groups:                  consecutive pairs; a pair opens a new group iff the group holds a pair already and with this one its bytes would
                           exceed workspace - off_group or its tiles INT32_MAX.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (a stand-alone host program)."""
import os
import re
import subprocess

import pytest

from tests import align_oracle, dtw_oracle, standin_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")
W, T = 256, 64                         # kDtwCols / kAlignThreads, kDtwTile (tests/test_gpu_dtw.py, tests/test_gpu_align.py)
TERMS = {"dtw": 12, "align": 8}        # include/fs2.h: FS2_DTW_TERMS, FS2_ALIGN_TERMS
REC, CELL, INT32_MAX, ALL = 40, 48, 2 ** 31 - 1, 1 << 40
SHAPES = {"dtw": dtw_oracle.edge_shapes(W, T), "align": align_oracle.edge_shapes(W, T)}
OPS = ("dtw", "align")


def align_up(x, a):
    return (x + a - 1) // a * a


def d_bytes(n, m):
    return align_up(8 * n * m, 256) if n and m else 0


def edge_bytes(op, n, m):
    return align_up(2 * n * CELL, 256) if op == "dtw" and n and m > W else 0


def pair_bytes(op, n, m):
    return d_bytes(n, m) + edge_bytes(op, n, m)


def pair_tiles(op, n, m):
    rows, cols = (m, n) if op == "align" else (n, m)
    return -(-rows // T) * -(-cols // T) if n and m else 0


def off_group(op, B):
    return align_up(align_up(max(B, 1) * REC, 256) + max(B, 1) * TERMS[op] * 8, 256)


def want_bytes(op, shapes, cap):
    per = [pair_bytes(op, n, m) for n, m in shapes]
    return min(off_group(op, len(shapes)) + sum(per), max(cap, off_group(op, len(shapes)) + max(per, default=0)))


def want_groups(op, shapes, ws_bytes):
    """[(first, count, tiles)] by the rule of the module docstring."""
    avail = ws_bytes - off_group(op, len(shapes))
    out, first, used, tiles = [], 0, 0, 0
    for i, (n, m) in enumerate(shapes):
        if i > first and (used + pair_bytes(op, n, m) > avail or tiles + pair_tiles(op, n, m) > INT32_MAX):
            out.append((first, i - first, tiles))
            first, used, tiles = i, 0, 0
        used, tiles = used + pair_bytes(op, n, m), tiles + pair_tiles(op, n, m)
    return out + ([(first, len(shapes) - first, tiles)] if shapes else [])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = standin_build.build(tmp_path_factory, "tests/pair_plan_probe.cpp", flags=("-std=c++17", "-Wall", "-Werror"))

    def run(op, mode, ws, shapes, *flags):
        r = subprocess.run([exe, op, mode, str(ws)] + list(flags) + ["%d:%d" % s for s in shapes], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def query(probe, op, shapes, cap, *flags):
    (line,) = probe(op, "bytes", cap, shapes, *flags)
    return int(line.split()[1])


def plan(probe, op, shapes, ws, *flags):
    """-> dict(rc, fail, layout, recs [(a0, n, b0, m, tile0, tcols, d_off, aux)], groups [(first, count, tiles)], chunks [(base, n, [(a0, b0)])])."""
    out = dict(rc=None, fail=None, layout=None, recs=[], groups=[], chunks=[], ngroups=None)
    for line in probe(op, "plan", ws, shapes, *flags):
        key, _, rest = line.partition(" ")
        if key == "fail":
            code, _, msg = rest.partition(" ")
            out["fail"] = (int(code), msg)
        elif key == "rc":
            out["rc"] = int(rest)
        elif key == "layout":
            out["layout"] = tuple(int(x) for x in rest.split())
        elif key == "rec":
            v = [int(x) for x in rest.split()]
            assert v[0] == len(out["recs"])
            out["recs"].append(tuple(v[1:]))
        elif key == "group":
            out["groups"].append(tuple(int(x) for x in rest.split()))
        elif key == "chunk":
            v = rest.split()
            out["chunks"].append((int(v[0]), int(v[1]), [tuple(int(x) for x in p.split(":")) for p in v[2:]]))
        elif key == "groups":
            out["ngroups"] = int(rest)
        else:
            raise AssertionError(line)
    return out


def check_plan(op, shapes, ws_bytes, got, labels=False):
    """Everything a plan promises, against the rule: the layout, the groups, every record."""
    B = len(shapes)
    og = off_group(op, B)
    assert got["rc"] == 0 and got["fail"] is None
    off_recs, off_terms, off_grp, everything, largest = got["layout"]
    per = [pair_bytes(op, n, m) for n, m in shapes]
    assert (off_recs, off_terms, off_grp) == (0, align_up(max(B, 1) * REC, 256), og)
    assert (everything, largest) == (og + sum(per), og + max(per, default=0))
    groups = got["groups"]
    assert groups == want_groups(op, shapes, ws_bytes) and got["ngroups"] == len(groups)        # (the walk for the launches sees the same groups)
    assert [f for f, _, _ in groups] == [sum(c for _, c, _ in groups[:k]) for k in range(len(groups))]      # consecutive runs ...
    assert sum(c for _, c, _ in groups) == B and all(c > 0 for _, c, _ in groups)                          # ... that partition [0, B)
    assert len(got["recs"]) == B
    a0 = b0 = 0
    for first, count, tiles in groups:
        ranges, tile0 = [], 0
        for i in range(first, first + count):
            n, m = shapes[i]
            ra0, rn, rb0, rm, rtile0, rtcols, d_off, aux = got["recs"][i]
            assert (ra0, rn, rb0, rm) == ((b0, m, a0, n) if op == "align" else (a0, n, b0, m))
            assert rtile0 == tile0 and rtcols == -(-rm // T)
            if n and m:
                assert rtile0 + -(-rn // T) * rtcols == tile0 + pair_tiles(op, n, m)
            tile0 += pair_tiles(op, n, m)
            ranges.append((d_off, d_off + d_bytes(n, m)))
            if op == "dtw":
                assert aux == d_off + d_bytes(n, m)
                ranges.append((aux, aux + edge_bytes(op, n, m)))
            else:
                assert aux == (n if labels else -1)
            a0, b0 = a0 + n, b0 + m
        assert tile0 == tiles <= INT32_MAX
        assert all(og <= lo <= hi <= ws_bytes for lo, hi in ranges)
        taken = sorted(r for r in ranges if r[1] > r[0])                 # (an empty pair takes no bytes and no tiles: its ranges are empty)
        assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))
        assert sum(hi - lo for lo, hi in taken) == sum(per[first:first + count])
    return groups


def test_pair_plan_header_is_plain_cpp():
    """No HIP construct in pair_plan.h, whose one include is record_op.h; none either, and no include, in the half of record_op.h that a
    plain host compiler sees (what stands ahead of its device half)."""
    hip = ("__global__", "__device__", "__shared__", "hipLaunch", "hipStream", "hipError", "threadIdx", "blockIdx")
    src = open(os.path.join(CSRC, "pair_plan.h")).read()
    assert re.findall(r"#\s*(?:include|import)\s*(\S+)", src) == ['"record_op.h"']
    plain, guard, device = open(os.path.join(CSRC, "record_op.h")).read().partition("#ifdef __global__")
    assert guard and device.rstrip().endswith("#endif") and device.count("#if") == 0 and not re.search(r"#\s*(?:include|import)", plain)
    for word in hip:
        assert word not in src and word not in plain, word


@pytest.mark.parametrize("op", OPS)
def test_workspace_bytes(probe, op):
    for shapes in (SHAPES[op], SHAPES[op][::-1], []):
        least, everything = want_bytes(op, shapes, 0), want_bytes(op, shapes, ALL)
        for cap in (0, (least + everything) // 2, ALL):
            assert query(probe, op, shapes, cap) == want_bytes(op, shapes, cap)
        if shapes:
            assert least < (least + everything) // 2 < everything
    assert query(probe, op, [], 0) == off_group(op, 0) > 0
    # the pinned terms, spelled out once for a pair with edge buffers (fs2_op_dtw) / without (fs2_op_align)
    want = 256 + 256 + align_up(8 * 40 * 513, 256) + (align_up(2 * 40 * 48, 256) if op == "dtw" else 0)
    assert query(probe, op, [(40, 513)], 0) == want
    assert query(probe, op, [(513, 40)], 0) == 256 + 256 + align_up(8 * 40 * 513, 256)
    assert query(probe, op, [(0, 5), (5, 0)], ALL) == off_group(op, 2)


@pytest.mark.parametrize("op,labels", [("dtw", False), ("align", False), ("align", True)])
def test_records_and_groups_under_the_byte_limit(probe, op, labels):
    flags = ("labels",) if labels else ()
    for shapes in (SHAPES[op], SHAPES[op][::-1]):
        sizes = sorted(8 * n * m for n, m in shapes)
        two = sizes[-1] + sizes[-2] + 4096                 # the two largest matrices fit together, all of them do not (the stand-in tests' cap)
        assert two < sum(sizes)
        seen = {}
        for cap in (0, two, ALL):
            ws = want_bytes(op, shapes, cap)
            seen[cap] = check_plan(op, shapes, ws, plan(probe, op, shapes, "cap:%d" % cap, *flags), labels)
        assert len(seen[ALL]) == 1
        assert 1 < len(seen[two]) < len(seen[0]) and any(sum(1 for n, m in shapes[f:f + c] if n and m) > 1 for f, c, _ in seen[two])
    # cap 0 leaves room for the largest pair alone.  Pairs of one size, with empty ones between: no two non-empty pairs fit together
    shapes = [(70, 300), (0, 5), (70, 300), (70, 300), (5, 0), (0, 0), (70, 300)]
    groups = check_plan(op, shapes, want_bytes(op, shapes, 0), plan(probe, op, shapes, "cap:0", *flags), labels)
    assert [sum(1 for n, m in shapes[f:f + c] if n and m) for f, c, _ in groups] == [1, 1, 1, 1]
    # one byte more or less than two pairs need decides whether the second joins the first
    two = off_group(op, 4) + 2 * pair_bytes(op, 70, 300)
    same = [(70, 300)] * 4
    assert [c for _, c, _ in check_plan(op, same, two, plan(probe, op, same, two, *flags), labels)] == [2, 2]
    assert [c for _, c, _ in check_plan(op, same, two - 1, plan(probe, op, same, two - 1, *flags), labels)] == [1, 1, 1, 1]
    check_plan(op, [], off_group(op, 0), plan(probe, op, [], "cap:0", *flags), labels)


@pytest.mark.parametrize("op", OPS)
def test_groups_under_the_tile_limit(probe, op):
    side = 1 << 20                                          # 2^40 cells (the most a pair may have), 2^28 tiles
    shapes = [(side, side)] * 12
    assert pair_tiles(op, side, side) == 1 << 28 and 7 * (1 << 28) <= INT32_MAX < 8 * (1 << 28)
    ws = want_bytes(op, shapes, 1 << 62)
    assert ws == off_group(op, 12) + 12 * pair_bytes(op, side, side)              # room for all: only the tiles can close a group
    groups = check_plan(op, shapes, ws, plan(probe, op, shapes, "cap:%d" % (1 << 62)))
    assert groups == [(0, 7, 7 << 28), (7, 5, 5 << 28)]
    # a pair whose 2^28 - 1 = 16383 x 16385 tiles just fit stays in the group; one tile more opens the next
    shapes = [(side, side)] * 7 + [(T * 16383, T * 16385), (1, 1)]
    groups = check_plan(op, shapes, want_bytes(op, shapes, 1 << 62), plan(probe, op, shapes, "cap:%d" % (1 << 62)))
    assert groups == [(0, 8, INT32_MAX), (8, 1, 1)]


@pytest.mark.parametrize("op", OPS)
def test_refusals(probe, op):
    who, side = "fs2_op_" + op, 1 << 20
    ERR_ARG, ERR_WORKSPACE = -1, -5                         # include/fs2.h
    cases = [([(side + 1, side)], (), "%s: a matrix of more than 2^40 cells" % who),
             ([(3, 4), (-1, 4)], (), "%s: negative length of pair 1" % who),
             ([(3, 4), (4, -2)], (), "%s: negative length of pair 1" % who),
             ([(3, 4)], ("nulllens",), "%s: bad batch (B = 1) or null a_starts / a_lens / b_starts / b_lens" % who)]
    for shapes, flags, msg in cases:
        assert query(probe, op, shapes, 0, *flags) == 0 and query(probe, op, shapes, ALL, *flags) == 0
        got = plan(probe, op, shapes, ALL, *flags)
        assert got["rc"] == ERR_ARG and got["fail"] == (ERR_ARG, msg) and not got["recs"] and not got["groups"] and not got["chunks"]
    assert query(probe, op, [(side, side)], 0) == off_group(op, 1) + pair_bytes(op, side, side)          # 2^40 cells exactly are served
    shapes = SHAPES[op]
    least = want_bytes(op, shapes, 0)
    got = plan(probe, op, shapes, least - 1)
    assert got["rc"] == ERR_WORKSPACE and got["fail"] == (ERR_WORKSPACE, "%s: workspace %d < %d bytes (the largest pair alone)" % (who, least - 1, least))
    assert plan(probe, op, shapes, least)["rc"] == 0


@pytest.mark.parametrize("op", OPS)
def test_many_pairs_upload_chunks(probe, op):
    shapes = [(i % 5 + 1, i % 3 + 1) for i in range(200)]
    got = plan(probe, op, shapes, "cap:%d" % ALL)
    check_plan(op, shapes, want_bytes(op, shapes, ALL), got)
    assert [(base, n) for base, n, _ in got["chunks"]] == [(0, 96), (96, 96), (192, 8)]
    rows = [(r[0], r[2]) for r in got["recs"]]                                      # (a0, b0): strictly increasing, so each names its pair
    assert len(set(rows)) == 200 and [p for _, _, part in got["chunks"] for p in part] == rows
    # and under a cap: the chunks carry the records of the grouped plan, whatever the groups
    ws = want_bytes(op, shapes, 0) + 1000
    got = plan(probe, op, shapes, ws)
    assert len(check_plan(op, shapes, ws, got)) > 3
    assert [p for _, _, part in got["chunks"] for p in part] == [(r[0], r[2]) for r in got["recs"]]
