"""Host-side checks of the packed-row layout (no GPU).

csrc/layout_rule.h -- the one statement of the gapped packed-row layout, the attention work list, the capacities and the offsets of the
`meta` block -- compiled with the host compiler (tests/layout_probe.cpp), and csrc/layout.h's kernels (frame_layout_dev,
build_row_meta) run on the host stand-in against build_layout (tests/kernel_standin/layout_main.cpp).  The rule is stated here once
more, in Python, in the form the runtime had before the header existed (explicit queues of items; the `meta` offsets as running
pointers), without looking at the header:

  lengths:    per utterance of v valid positions, longest of the batch m: (len, klen, vlen) = (v, v, v), or under padded-batch
              semantics (m, v if masked else m, v);
  rows:       row = gap; per utterance: start = row rounded up to 8, row = start + len + gap; R = row + 8, Rpad = R rounded up to 128;
  work list:  utterances by decreasing klen (stable), each to the shortest of eight queues (the lowest index on ties) as items
              (b, i), i 128 < len; depth = the longest queue; work[i 8 + j] = item i of queue j, (-1, 0) where the queue has ended.

Built with -fsanitize=address,undefined when FS2_STANDIN_ASAN=1 (stand-alone host programs: a sanitizer never sees the GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import standin_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")
INT32_MAX = 2 ** 31 - 1
MODES = ((0, 0), (1, 0), (1, 1))          # (compat, masked): per-utterance, compat, compat + masked
GAPS = (4, 8)
OVF_ROWS, OVF_LMAX, OVF_PE, OVF_EMPTY, OVF_BAD_ID = 1, 2, 4, 8, 16        # include/fs2.h


def up(x, a):
    return -(-x // a) * a


def lens_rule(valid, compat, masked):
    m = max(valid)
    return ([m if compat else v for v in valid], [(v if masked else m) if compat else v for v in valid], list(valid))


def parent_layout(valid, gap, compat, masked):
    """The module docstring's rule -> dict(start, len, klen, vlen, R, Rpad, work, depth)."""
    ln, klen, vlen = lens_rule(valid, compat, masked)
    row, start = gap, []
    for l in ln:
        row = up(row, 8)
        start.append(row)
        row += l + gap
    R = row + 8
    queues = [[] for _ in range(8)]
    for b in sorted(range(len(valid)), key=lambda b: -klen[b]):          # (sorted is stable)
        j = min(range(8), key=lambda t: len(queues[t]))                   # (min keeps the first of equals)
        queues[j] += [(b, i) for i in range(-(-ln[b] // 128))]
    depth = max(len(q) for q in queues)
    work = [(-1, 0)] * (depth * 8)
    for j, q in enumerate(queues):
        for i, item in enumerate(q):
            work[i * 8 + j] = item
    return dict(start=start, len=ln, klen=klen, vlen=vlen, R=R, Rpad=up(R, 128), work=work, depth=depth)


def batches():
    """B in {1, 2, 7, 8, 9, 17, 33, 100}: lengths around the 128-query block, runs of equal lengths, one utterance far longer than the rest."""
    out = [[1], [127], [128], [129], [1, 129], [128, 128]]
    rs = np.random.RandomState(5)
    for B in (7, 8, 9, 17, 33, 100):
        v = rs.randint(1, 300, size=B).tolist()
        v[:4] = [129, 1, 128, 127]
        v[B // 2: B // 2 + 3] = [77, 77, 77]             # a run of equal lengths: ties in batch order
        v[-1] = 2000
        out.append(v)
        out.append([130] * B)                            # all equal: the ninth utterance goes onto the first queue
    return out


BATCHES = batches()


def _checked(r):
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = standin_build.build(tmp_path_factory, "tests/layout_probe.cpp", flags=("-std=c++17", "-Wall", "-Werror"))

    def run(*args):
        out = {}
        for line in _checked(subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)):
            key, _, rest = line.partition(" ")
            out[key] = [tuple(int(x) for x in t.split(":")) if ":" in t else int(t) for t in rest.split()]
        return out
    return run


def test_rule_header_is_plain_cpp_and_owns_the_constants(probe):
    src = open(os.path.join(CSRC, "layout_rule.h")).read()
    for word in ("#include", "__global__", "__shared__", "hipLaunch", "hipStream", "hipError", "threadIdx", "blockIdx"):
        assert word not in src, word
    names = ("kGap", "kMinGap", "kTailRows", "kAttAlign", "kAttBlk", "kXcds")
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        for n in names:
            assert len(re.findall(r"constexpr\s+int\s+%s\s*=" % n, text)) == (1 if f == "layout_rule.h" else 0), (f, n)
    assert subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-include", os.path.join(CSRC, "layout_rule.h"), os.devnull]).returncode == 0
    assert probe("consts")["consts"] == [8, 4, 8, 8, 128, 8]


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("compat,masked", MODES)
def test_rule_equals_the_parents_algorithm(probe, compat, masked, gap):
    for valid in BATCHES:
        want = parent_layout(valid, gap, compat, masked)
        got = probe("layout", gap, compat, masked, *valid)
        assert got["start"] == want["start"] and got["len"] == want["len"] and got["klen"] == want["klen"] and got["vlen"] == want["vlen"], valid
        assert got["rows"] == [want["R"], want["Rpad"]] and got["depth"] == [want["depth"]], valid
        assert got["work"] == want["work"], valid


def parent_meta(B, Rpad, nwork, rf):
    """The offsets as the runtime formed them: running pointers, dims and row_pos rounded up to 16 bytes (4 ints) from a base that is."""
    host = [0, B, 2 * B, 3 * B, 4 * B]
    rest = up(4 * B + 2 * nwork, 4)
    host += [rest, rest + Rpad, rest + 2 * Rpad]
    dev = [0, B, 2 * B, 3 * B, 4 * B, 5 * B, 6 * B]
    dims = up(7 * B, 4)
    rest = up(dims + 16 + 2 * nwork, 4)
    dev += [dims, dims + 16, rest, rest + Rpad, rest + 2 * Rpad]
    dims2 = up(3 * B, 4)
    meta2 = [0, B, 2 * B, dims2, dims2 + 16, dims2 + 16 + Rpad * rf, dims2 + 16 + 2 * Rpad * rf]
    return host, dev, meta2


def _disjoint(offsets, sizes):
    spans = sorted(zip(offsets, sizes))
    return all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))


def test_meta_offsets(probe):
    for valid in BATCHES:
        B = len(valid)
        for compat, masked in MODES:
            lay = parent_layout(valid, 4, compat, masked)
            Rpad = lay["Rpad"]
            for nwork in (len(lay["work"]), 8 * ((Rpad // 128 + B + 7) // 8 + max(valid) // 128 + 2)):      # the host's list, a capacity
                for rf in (1, 2, 3):
                    got = probe("meta", B, Rpad, nwork, rf)
                    host, dev, meta2 = parent_meta(B, Rpad, nwork, rf)
                    assert got["host"] == host and got["dev"] == dev and got["meta2"] == meta2, (B, Rpad, nwork, rf)
                    assert _disjoint(host[:-1], [B, B, B, B, 2 * nwork, Rpad, Rpad]) and host[-1] == host[-2] + Rpad
                    assert _disjoint(dev[:-1], [B, B, B, B, B, B, B, 16, 2 * nwork, Rpad, Rpad]) and dev[-1] == dev[-2] + Rpad
                    assert _disjoint(meta2[:-1], [B, B, B, 16, Rpad * rf, Rpad * rf]) and meta2[-1] == meta2[-2] + Rpad * rf
                    assert got["ints"] == [7 * B + 2 * Rpad + 2 * nwork + 80, 4 * B + 2 * Rpad * rf + 64]
                    assert max(host[-1], dev[-1]) <= got["ints"][0] and meta2[-1] <= got["ints"][1]
                    assert all(x % 4 == 0 for x in (host[5], dev[7], dev[9], meta2[3], meta2[4]))             # row_pos, dims: 16-byte aligned


def test_row_bound_is_the_parents_expression(probe):
    for frames, utts in ((1, 1), (6000, 12), (8 * 4000, 64), (123456, 1024), (INT32_MAX - 300, 1), (INT32_MAX, 4096), (1 << 40, 7)):
        want = min(frames + utts * (8 + 8) + 8, INT32_MAX - 256)        # fs2_row_capacity rounds this up to 128; regime_rows_of takes it as it is
        assert probe("caps", frames, utts, 128, 1, 128)["row_bound"] == [want]


def test_capacity_bounds_the_work_list(probe):
    """Whenever the rows fit row_capacity and the longest utterance fits lmax_cap, the work list fits work_cap: checked at the tightest
    capacities (the rows and the longest utterance themselves) and at the ones a caller would name."""
    for valid in BATCHES:
        B = len(valid)
        for compat, masked in MODES:
            for gap in GAPS:
                lay = parent_layout(valid, gap, compat, masked)
                roomy = up(min(sum(lay["len"]) + B * 16 + 8, INT32_MAX - 256), 128)
                assert lay["R"] <= roomy
                for row_cap, lmax_cap in ((lay["R"], max(valid)), (roomy, max(valid)), (roomy, max(valid) + 500)):
                    cap = probe("caps", 1, 1, row_cap, B, lmax_cap)["work_capacity"][0]
                    assert cap == 8 * ((row_cap // 128 + B + 7) // 8 + lmax_cap // 128 + 2)
                    assert lay["depth"] * 8 <= cap, (valid, compat, masked, gap, row_cap, lmax_cap)


def test_overflow_flags(probe):
    ok = dict(rows=1000, depth=4, longest=300, smallest=5, row_cap=1000, work_cap=32, lmax_cap=300, pe_rows=300)
    order = ("rows", "depth", "longest", "smallest", "row_cap", "work_cap", "lmax_cap", "pe_rows")
    cases = [({}, 0), (dict(rows=1001), OVF_ROWS), (dict(depth=5), OVF_ROWS), (dict(lmax_cap=299), OVF_LMAX), (dict(pe_rows=299), OVF_PE),
             (dict(smallest=0), OVF_EMPTY), (dict(smallest=-1), OVF_BAD_ID), (dict(rows=1001, lmax_cap=1, pe_rows=1, smallest=-1), OVF_ROWS | OVF_LMAX | OVF_PE | OVF_BAD_ID)]
    for edit, want in cases:
        v = dict(ok, **edit)
        assert probe("flags", *[v[k] for k in order])["flags"] == [want], edit
    fs2_h = open(os.path.join(ROOT, "include", "fs2.h")).read()
    for name, val in (("ROWS", OVF_ROWS), ("LMAX", OVF_LMAX), ("PE", OVF_PE), ("EMPTY", OVF_EMPTY), ("BAD_ID", OVF_BAD_ID)):
        assert int(re.search(r"#define FS2_OVF_%s (\d+)" % name, fs2_h).group(1)) == val


# ---- the kernels' code on the host stand-in
@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return standin_build.build(tmp_path_factory, "tests/kernel_standin/layout_main.cpp")


def _launch(standin, tmp_path, counts, gap=4, compat=0, masked=0, row_cap=0, work_cap=0, lmax_cap=0, pe_rows=1 << 20, refused=False):
    """One launch of frame_layout_dev + build_row_meta (0 = a sufficient capacity) -> (dims, build_layout's answer or None)."""
    src = str(tmp_path / "in.txt")
    with open(src, "w") as f:
        f.write("%d %d %d %d %d %d %d %d\n%s\n" % (len(counts), gap, compat, masked, row_cap, work_cap, lmax_cap, pe_rows, " ".join(str(c) for c in counts)))
    r = subprocess.run([standin, src], capture_output=True, text=True, timeout=600)
    out = {}
    for line in _checked(r):
        key, _, rest = line.partition(" ")
        assert key != "mismatch", r.stdout[-2000:]
        out[key] = [tuple(int(x) for x in t.split(":")) if ":" in t else int(t) for t in rest.split()]
    assert out["mismatches"] == [0]            # the device's arrays against the host's: start, len, klen, vlen, work to work_cap, dims, pcum, row_pos, row_seq, status
    assert ("host_work" in out) == (not refused)
    return out["dims"], out


def _check_served(standin, tmp_path, counts, **kw):
    dims, out = _launch(standin, tmp_path, counts, **kw)
    want = parent_layout(counts, kw.get("gap", 4), kw.get("compat", 0), kw.get("masked", 0))
    assert dims == [want["R"], len(want["work"]), 0, max(counts), sum(counts), 0, 0, 0]
    assert out["host_start"] == want["start"] and out["host_len"] == want["len"] and out["host_klen"] == want["klen"] and out["host_vlen"] == want["vlen"]
    assert out["host_rows"] == [want["R"], want["Rpad"]] and out["host_work"] == want["work"]


RAGGED33 = [129, 1, 128, 127] + np.random.RandomState(9).randint(1, 300, size=25).tolist() + [77, 77, 77, 1500]


@pytest.mark.parametrize("name,counts,kw", [
    ("B1", [150], {}),
    ("B9_equal", [130] * 9, {}),
    ("B33_per_utterance", RAGGED33, dict(compat=0, masked=0)),
    ("B33_compat", RAGGED33, dict(compat=1, masked=0)),
    ("B33_compat_masked", RAGGED33, dict(compat=1, masked=1)),
    ("gap4", [5, 260, 3, 128, 40, 40, 9, 511, 64, 300], dict(gap=4)),
    ("gap8", [5, 260, 3, 128, 40, 40, 9, 511, 64, 300], dict(gap=8)),
    ("B4097_not_staged", np.random.RandomState(11).randint(1, 21, size=4097).tolist(), {}),
])
def test_kernel_code_on_the_host_equals_build_layout(standin, tmp_path, name, counts, kw):
    _check_served(standin, tmp_path, counts, **kw)


def test_kernel_refusals_on_the_host(standin, tmp_path):
    counts = [5, 260, 3, 128, 40, 40, 9, 511, 64, 300]
    lay = parent_layout(counts, 4, 0, 0)
    ok = dict(row_cap=lay["R"], work_cap=len(lay["work"]), lmax_cap=max(counts), pe_rows=max(counts))
    _check_served(standin, tmp_path, counts, **ok)                          # the tightest capacities serve the batch
    for edit, bad, flag in ((dict(row_cap=lay["R"] - 1), counts, OVF_ROWS), (dict(lmax_cap=max(counts) - 1), counts, OVF_LMAX),
                            (dict(pe_rows=max(counts) - 1), counts, OVF_PE), ({}, counts[:4] + [0] + counts[5:], OVF_EMPTY),
                            ({}, counts[:4] + [-1] + counts[5:], OVF_BAD_ID)):
        dims, _ = _launch(standin, tmp_path, bad, refused=True, **dict(ok, **edit))
        assert dims[2] == flag and dims[1] == 0 and dims[3] == max(bad) and dims[5:] == [0, 0, 0], (edit, dims)
