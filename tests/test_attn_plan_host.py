"""Host-side checks of the attention plan (no GPU): csrc/attn_plan.h -- the pure function launch_attention executes -- compiled with the host compiler
(tests/gemm_plan_probe.cpp, the driver of tests/test_gemm_plan_host.py).

(a) the kernel (family, head dim, MFMA terms) of the encoder's and the decoder's attention launch of the default model and the number of qkv_split passes, pinned
    for one utterance (c1) and for c3 in four precisions; the expected values are the `attn_*` / `qkv_split` dispatches of the committed kernel traces of the
    parent commit (profiles/gemm_plan_trace_parent_*.txt), not the plan's;
(b) the attn_w32 rule over regime rows on both sides of its threshold (a rule on 128-query blocks: 8064 rows are 63 of them, 8065 need 64), the FS2_ATTN_W32
    switch, the precisions, the four head dims and the distance of the lo planes;
(c) the grids, the refusals with their FS2_ERR_* code and text, and the softmax scales bit for bit."""
import os
import re

import numpy as np
import pytest

from tests.test_gemm_plan_host import ERR_UNSUPPORTED, MODES, REGIMES, ROOT, TRACED_CASE, probe  # noqa: F401  (probe: the fixture)

HEADS = 2      # of the default model (tests/gemm_plan_probe.cpp: Model)

# (workload, mode) -> (encoder launch, decoder launch, qkv_split dispatches); a launch is (family, head dim, MFMA terms: attn_bf16 only), from the parent's traces
_ENC, _DEC3, _DECW = ("attn_bf16", 128, 3), ("attn_bf16", 192, 3), ("attn_w32", 192, 0)
ATTN_PINNED = {
    ("c1", "fp32"): (("attn_f32", 128, 0), ("attn_f32", 192, 0), 0),
    ("c1", "bf16x3"): (_ENC, _DEC3, 0),
    ("c1", "mix_mx"): (_ENC, _DEC3, 0),
    ("c1", "mix_mx4"): (_ENC, _DEC3, 0),
    ("c3", "fp32"): (("attn_f32", 128, 0), ("attn_f32", 192, 0), 0),
    ("c3", "bf16x3"): (_ENC, _DECW, 0),
    ("c3", "mix_mx"): (_ENC, _DECW, 0),
    ("c3", "mix_mx4"): (_ENC, _DECW, 0),
}


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("mode", MODES)
def test_pinned_attention_plans(probe, regime, mode):
    got = {"enc.attn": [], "dec.attn": []}
    for line in probe("model", *REGIMES[regime], TRACED_CASE):
        f = line.split()
        if f[0] == mode and f[1] in got:
            got[f[1]].append((f[2], int(f[3]), int(f[4]), int(f[5])))
    print(regime, mode, got)
    assert all(len(v) == 4 and len(set(v)) == 1 for v in got.values()), "one attention launch per block, the four blocks of a stack alike"
    enc, dec = got["enc.attn"][0], got["dec.attn"][0]
    assert (enc[:3], dec[:3], 4 * enc[3] + 4 * dec[3]) == ATTN_PINNED[(regime, mode)]


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("mode", MODES)
def test_pinned_attention_table_is_the_parent_trace(regime, mode):
    """ATTN_PINNED is what the committed kernel trace of the parent commit says: the table cannot follow the plan without a trace file changing."""
    launches, splits = [], 0
    for l in open(os.path.join(ROOT, "profiles", "gemm_plan_trace_parent_%s_%s.txt" % (regime, mode))).read().split("\n"):
        m = re.match(r"(attn_\w+)<([^>]*)> grid=\d+,(\d+),\d+ wg=\d+,(\d+),\d+ ", l)
        if m:
            t = [int(x) for x in m.group(2).split(",")]
            assert int(m.group(3)) // int(m.group(4)) == HEADS, l      # grid.y in workgroups
            launches.append((m.group(1), t[0], t[1] if m.group(1) == "attn_bf16" else 0))
        splits += l.startswith("qkv_split ")
    assert len(launches) == 8 and len(set(launches[:4])) == 1 and len(set(launches[4:])) == 1, launches      # four encoder blocks, then four decoder blocks
    assert (launches[0], launches[4], splits) == ATTN_PINNED[(regime, mode)]


@pytest.fixture(scope="module")
def sweep(probe):
    out = {}
    for line in probe("attn_sweep"):
        what, kernel, dk, nsplit, gx, gy, split, scale, err, msg = line.split("|")
        assert what not in out
        out[what] = dict(kernel=kernel, dk=int(dk), nsplit=int(nsplit), grid=(int(gx), int(gy)), split=int(split), scale=int(scale, 16), err=int(err), msg=msg)
    return out


ROWS = (1, 8064, 8065, 8191, 8192, 8193, 37256)
W32_MIN_BLOCKS = 64      # csrc/attn_plan.h: kW32MinBlocks, in blocks of 128 queries


def test_w32_rule_over_the_threshold(sweep):
    n = 0
    for rows in ROWS:
        for w32 in (-1, 0, 1):
            for prec in ("fp32", "bf16x3", "bf16"):
                for dk in (64, 128, 192, 256):
                    given, by_R = (sweep["regime %d %d %s %d %d" % (rows, w32, prec, dk, k)] for k in (0, 1))
                    assert given == by_R, "regime_rows = 0 falls back to R"
                    n += 1
                    on = prec == "bf16x3" and dk in (128, 192) and (w32 == 1 or (w32 == -1 and (rows + 127) // 128 >= W32_MIN_BLOCKS))
                    want = "attn_f32" if prec == "fp32" else ("attn_w32" if on else "attn_bf16")
                    assert (given["kernel"], given["dk"], given["err"]) == (want, dk, 0), (rows, w32, prec, dk, given)
                    assert given["nsplit"] == ({"bf16x3": 3, "bf16": 1}[prec] if want == "attn_bf16" else 0)
                    assert given["grid"] == (8 if on else 16, HEADS) and not given["split"]      # 8 work items
    assert n == 7 * 3 * 3 * 4
    auto = lambda rows, dk: sweep["regime %d -1 bf16x3 %d 0" % (rows, dk)]["kernel"]
    for dk in (128, 192):      # 63 blocks end at 8064 rows: the rule is on blocks, not on rows
        assert [auto(r, dk) for r in ROWS] == ["attn_bf16"] * 2 + ["attn_w32"] * 5


def test_w32_needs_the_lo_planes_close_behind(sweep):
    for which in (0, 1):
        assert [sweep["dist %d %d" % (d, which)]["kernel"] for d in (0, -256, 2 ** 31 - 1, 2 ** 31)] == ["attn_bf16", "attn_bf16", "attn_w32", "attn_bf16"]


def test_attention_grids(sweep):
    for n in range(34):
        f32, b16, w32 = (sweep["grid %d %s" % (n, k)] for k in ("f32", "b16", "w32"))
        if n == 0:
            assert all(p["kernel"] == "none" and not p["split"] and p["err"] == 0 for p in (f32, b16, w32))
            continue
        assert (f32["kernel"], b16["kernel"], w32["kernel"]) == ("attn_f32", "attn_bf16", "attn_w32")
        assert f32["grid"] == b16["grid"] == (2 * ((n + 7) & ~7), HEADS) and w32["grid"] == (n, HEADS)
        assert (f32["split"], b16["split"], w32["split"]) == (0, 1, 0)      # fp32 reads the rows itself; the third case has its operands split already


def test_softmax_scales_bit_for_bit(sweep):
    bits = lambda x: int(np.float32(x).view(np.uint32))
    for dk_true in (64, 96, 128, 192):
        root = np.sqrt(np.float32(dk_true))
        assert root.dtype == np.float32
        padded = {64: 64, 96: 128, 128: 128, 192: 192}[dk_true]
        for prec in ("fp32", "bf16x3", "bf16"):
            p = sweep["scale %d %s" % (dk_true, prec)]
            assert p["dk"] == padded and p["split"] == (prec != "fp32")
            assert p["scale"] == bits((np.float32(1.0) if prec == "fp32" else np.float32(1.4426950408889634)) / root), (dk_true, prec)


HEAD_DIM = "attention head dim %d not in {64,128,192,256} (the model path pads other head dims)"
ATTN_REFUSALS = {
    "head_dim_fp32": ("none", ERR_UNSUPPORTED, HEAD_DIM % 96),
    "head_dim_bf16x3": ("none", ERR_UNSUPPORTED, HEAD_DIM % 96),
    "head_dim_no_work": ("none", 0, ""),                                   # nothing to launch is no error, whatever the shape
    "wide_split": ("none", ERR_UNSUPPORTED, "attention dim 1056 > 1024"),
    "wide_operands_given": ("none", ERR_UNSUPPORTED, HEAD_DIM % 264),      # D = 1056 with the operands given: the width is not refused, the head dim is (1056 is no multiple of one the kernels have)
    "wide_accepted": ("attn_bf16", 0, ""),                                 # D = 1152 with the operands already split
    "wide_fp32": ("attn_f32", 0, ""),
}


def test_attention_refusals_keep_their_codes(probe):
    got = {}
    for line in probe("attn_refusals"):
        f = line.split("|")
        got[f[0]] = (f[1], int(f[8]), f[9])
    assert got == ATTN_REFUSALS

