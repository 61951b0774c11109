"""Host-side checks of the GEMM plan (no GPU): csrc/gemm_plan.h -- the pure function launch_gemm executes -- and csrc/model_launches.h -- the forming of every
named launch of the model, which fs2_runtime.hip executes -- compiled with the host compiler (tests/gemm_plan_probe.cpp describes a model and walks the header's lists).

(a) the kernel family, tile height, split-K factor and ln_rows pass of every named launch of the default model, pinned for one utterance (c1) and
    for c3 in four precisions.  The expected values were read from kernel traces of the commit BEFORE the plan existed (rocprofv3 --kernel-trace of
    `bench.py --steps 1 --warmup 0 --streams 1 --no-overlap-encoder --workload c1|c3 --precision ...`; the condensed lists are
    profiles/gemm_plan_trace_parent_*.txt, profiles/gemm_plan_trace_names.md says how a traced kernel maps to a launch name), not from the plan;
(b) the planes-only decision of fs2_decode: the predicate it used to restate by hand equals "the decoder's three LayerNorm-fused launches, in planes-only
    form, all plan onto gemm_row4_bf16" over row counts on both sides of the threshold, the forcing switches, two precisions and two decoder widths;
(c) the plan of every frame-level launch is the same in every field for a row capacity of 1.0, 1.15 and 1.25 x the regime estimate (why the host- and
    the device-driven layout give equal bits);
(d) every refusal of launch_gemm keeps its FS2_ERR_* code and message;
(e) the pre-LN / concat_after block variants: the steps of a block, in order, are the launches run_stack_general made before the header existed, and every GEMM
    among them plans."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")
MODES = ("fp32", "bf16x3", "mix_mx", "mix_mx4")

# rows of the two workloads (bench.py's c1 and c3; synthetic.make_batch): token-level rows / regime estimate, frame-level rows / regime estimate.
# Token level: the host layout of the phoneme counts (80; 64 utterances, 4528 phonemes; the traces' embed_pe grids agree) and regime_rows_of = phonemes +
# 16 per utterance + 8.  Frame level: the rows of the traced run (4 x the workgroups of its lr_expand launch; c3 runs the device-driven layout, whose row
# count is a capacity) and fs2_runtime.hip's regime_rows_of = 8 x phonemes + 16 per utterance + 8.
REGIMES = {"c1": (100, 104, 896, 664), "c3": (5028, 5560, 46208, 37256)}

# The traces are older than FS2_TOKPROJ (multiply before expanding): they hold the frame-level launches var.conv0 / dec.in, which the default options no longer make.
# The probe's walk follows csrc/call_plan.h, so the pinned tables ask for the options of their traces explicitly.
TRACED_CASE = "tokproj=0"

# launch -> (kernel family, tile rows, ksplit, ln_rows pass), from the parent's traces
PINNED = {('c1', 'bf16x3'): {'dec.ffn1': ('pl_bf16', 64, 4, 1),
                    'dec.ffn2_ln': ('pl_bf16', 64, 4, 1),
                    'dec.in': ('pl_bf16', 64, 2, 1),
                    'dec.out_ln': ('pl_bf16', 64, 3, 1),
                    'dec.qkv': ('pl_bf16', 64, 1, 0),
                    'dur.conv0': ('pl_bf16', 64, 4, 1),
                    'dur.conv1': ('pl_bf16', 64, 4, 1),
                    'enc.ffn1': ('pl_bf16', 64, 4, 1),
                    'enc.ffn2_ln': ('pl_bf16', 64, 4, 1),
                    'enc.out_ln': ('pl_bf16', 64, 2, 1),
                    'enc.qkv': ('pl_bf16', 64, 1, 0),
                    'feat_out': ('pl_bf16', 64, 3, 1),
                    'postnet.0': ('pl_bf16', 64, 3, 1),
                    'postnet.1': ('pl_bf16', 64, 4, 1),
                    'postnet.2': ('pl_bf16', 64, 4, 1),
                    'postnet.3': ('pl_bf16', 64, 4, 1),
                    'postnet.4': ('pl_bf16', 64, 4, 1),
                    'var.conv0': ('pl_bf16', 64, 4, 1),
                    'var.conv1': ('pl_bf16', 64, 4, 1)},
 ('c1', 'fp32'): {'dec.ffn1': ('tile_f32', 0, 1, 0),
                  'dec.ffn2_ln': ('tile_rows_f32', 0, 1, 1),
                  'dec.in': ('tile_rows_f32', 0, 1, 1),
                  'dec.out_ln': ('tile_rows_f32', 0, 1, 1),
                  'dec.qkv': ('tile_f32', 0, 1, 0),
                  'dur.conv0': ('tile_rows_f32', 0, 1, 1),
                  'dur.conv1': ('tile_rows_f32', 0, 1, 1),
                  'enc.ffn1': ('tile_f32', 0, 1, 0),
                  'enc.ffn2_ln': ('tile_rows_f32', 0, 1, 1),
                  'enc.out_ln': ('tile_rows_f32', 0, 1, 1),
                  'enc.qkv': ('tile_f32', 0, 1, 0),
                  'energy.conv0': ('tile_rows_f32', 0, 1, 1),
                  'energy.conv1': ('tile_rows_f32', 0, 1, 1),
                  'feat_out': ('rows_f32', 0, 1, 0),
                  'pitch.conv0': ('tile_rows_f32', 0, 1, 1),
                  'pitch.conv1': ('tile_rows_f32', 0, 1, 1),
                  'postnet.0': ('tile_f32', 0, 1, 0),
                  'postnet.1': ('tile_f32', 0, 1, 0),
                  'postnet.2': ('tile_f32', 0, 1, 0),
                  'postnet.3': ('tile_f32', 0, 1, 0),
                  'postnet.4': ('rows_f32', 0, 1, 0)},
 ('c1', 'mix_mx'): {'dec.ffn1': ('pl_mx', 64, 4, 1),
                    'dec.ffn2_ln': ('pl_bf16', 64, 4, 1),
                    'dec.in': ('pl_bf16', 64, 2, 1),
                    'dec.out_ln': ('pl_bf16', 64, 3, 1),
                    'dec.qkv': ('pl_bf16', 64, 1, 0),
                    'dur.conv0': ('pl_bf16', 64, 4, 1),
                    'dur.conv1': ('pl_bf16', 64, 4, 1),
                    'enc.ffn1': ('pl_mx', 64, 4, 1),
                    'enc.ffn2_ln': ('pl_bf16', 64, 4, 1),
                    'enc.out_ln': ('pl_bf16', 64, 2, 1),
                    'enc.qkv': ('pl_bf16', 64, 1, 0),
                    'feat_out': ('pl_bf16', 64, 3, 1),
                    'postnet.0': ('pl_bf16', 64, 3, 1),
                    'postnet.1': ('pl_mx', 64, 4, 1),
                    'postnet.2': ('pl_mx', 64, 4, 1),
                    'postnet.3': ('pl_mx', 64, 4, 1),
                    'postnet.4': ('pl_bf16', 64, 4, 1),
                    'var.conv0': ('pl_bf16', 64, 4, 1),
                    'var.conv1': ('pl_bf16', 64, 4, 1)},
 ('c1', 'mix_mx4'): {'dec.ffn1': ('pl_mx', 64, 4, 1),
                     'dec.ffn2_ln': ('pl_bf16', 64, 4, 1),
                     'dec.in': ('pl_bf16', 64, 2, 1),
                     'dec.out_ln': ('pl_bf16', 64, 3, 1),
                     'dec.qkv': ('pl_bf16', 64, 1, 0),
                     'dur.conv0': ('pl_bf16', 64, 4, 1),
                     'dur.conv1': ('pl_bf16', 64, 4, 1),
                     'enc.ffn1': ('pl_mx', 64, 4, 1),
                     'enc.ffn2_ln': ('pl_bf16', 64, 4, 1),
                     'enc.out_ln': ('pl_bf16', 64, 2, 1),
                     'enc.qkv': ('pl_bf16', 64, 1, 0),
                     'feat_out': ('pl_bf16', 64, 3, 1),
                     'postnet.0': ('pl_bf16', 64, 3, 1),
                     'postnet.1': ('pl_mx', 64, 4, 1),
                     'postnet.2': ('pl_mx', 64, 4, 1),
                     'postnet.3': ('pl_mx', 64, 4, 1),
                     'postnet.4': ('pl_bf16', 64, 4, 1),
                     'var.conv0': ('pl_bf16', 64, 4, 1),
                     'var.conv1': ('pl_bf16', 64, 4, 1)},
 ('c3', 'bf16x3'): {'dec.ffn1': ('pl_bf16', 256, 1, 0),
                    'dec.ffn2_ln': ('row4', 160, 1, 0),
                    'dec.in': ('row4', 160, 1, 0),
                    'dec.out_ln': ('row4', 160, 1, 0),
                    'dec.qkv': ('qkv4', 160, 1, 0),
                    'dur.conv0': ('pl_bf16', 64, 4, 1),
                    'dur.conv1': ('pl_bf16', 64, 4, 1),
                    'enc.ffn1': ('pl_bf16', 64, 1, 0),
                    'enc.ffn2_ln': ('pl_bf16', 64, 4, 1),
                    'enc.out_ln': ('pl_bf16', 64, 2, 1),
                    'enc.qkv': ('pl_bf16', 64, 1, 0),
                    'energy.conv0': ('row8c', 192, 1, 0),
                    'feat_out': ('pl_bf16', 64, 1, 0),
                    'pitch.conv0': ('row8c', 192, 1, 0),
                    'postnet.0': ('pl_bf16', 128, 1, 0),
                    'postnet.1': ('pl_bf16', 128, 1, 0),
                    'postnet.2': ('pl_bf16', 128, 1, 0),
                    'postnet.3': ('pl_bf16', 128, 1, 0),
                    'postnet.4': ('pl_bf16', 64, 1, 0),
                    'var.conv1': ('row8c_grouped', 192, 1, 0)},
 ('c3', 'fp32'): {'dec.ffn1': ('tile_f32', 0, 1, 0),
                  'dec.ffn2_ln': ('tile_rows_f32', 0, 1, 1),
                  'dec.in': ('tile_rows_f32', 0, 1, 1),
                  'dec.out_ln': ('tile_rows_f32', 0, 1, 1),
                  'dec.qkv': ('tile_f32', 0, 1, 0),
                  'dur.conv0': ('tile_rows_f32', 0, 1, 1),
                  'dur.conv1': ('tile_rows_f32', 0, 1, 1),
                  'enc.ffn1': ('tile_f32', 0, 1, 0),
                  'enc.ffn2_ln': ('tile_rows_f32', 0, 1, 1),
                  'enc.out_ln': ('tile_rows_f32', 0, 1, 1),
                  'enc.qkv': ('tile_f32', 0, 1, 0),
                  'energy.conv0': ('tile_rows_f32', 0, 1, 1),
                  'energy.conv1': ('tile_rows_f32', 0, 1, 1),
                  'feat_out': ('rows_f32', 0, 1, 0),
                  'pitch.conv0': ('tile_rows_f32', 0, 1, 1),
                  'pitch.conv1': ('tile_rows_f32', 0, 1, 1),
                  'postnet.0': ('tile_f32', 0, 1, 0),
                  'postnet.1': ('tile_f32', 0, 1, 0),
                  'postnet.2': ('tile_f32', 0, 1, 0),
                  'postnet.3': ('tile_f32', 0, 1, 0),
                  'postnet.4': ('rows_f32', 0, 1, 0)},
 ('c3', 'mix_mx'): {'dec.ffn1': ('pl_mx', 256, 1, 0),
                    'dec.ffn2_ln': ('row4', 160, 1, 0),
                    'dec.in': ('row4', 160, 1, 0),
                    'dec.out_ln': ('row4', 160, 1, 0),
                    'dec.qkv': ('qkv4', 160, 1, 0),
                    'dur.conv0': ('pl_bf16', 64, 4, 1),
                    'dur.conv1': ('pl_bf16', 64, 4, 1),
                    'enc.ffn1': ('pl_mx', 64, 1, 0),
                    'enc.ffn2_ln': ('pl_bf16', 64, 4, 1),
                    'enc.out_ln': ('pl_bf16', 64, 2, 1),
                    'enc.qkv': ('pl_bf16', 64, 1, 0),
                    'energy.conv0': ('row8c', 192, 1, 0),
                    'feat_out': ('pl_bf16', 64, 1, 0),
                    'pitch.conv0': ('row8c', 192, 1, 0),
                    'postnet.0': ('pl_bf16', 128, 1, 0),
                    'postnet.1': ('pl_mx', 128, 1, 0),
                    'postnet.2': ('pl_mx', 128, 1, 0),
                    'postnet.3': ('pl_mx', 128, 1, 0),
                    'postnet.4': ('pl_bf16', 64, 1, 0),
                    'var.conv1': ('row8c_grouped', 192, 1, 0)},
 ('c3', 'mix_mx4'): {'dec.ffn1': ('pl_mx4', 256, 1, 0),
                     'dec.ffn2_ln': ('row4', 160, 1, 0),
                     'dec.in': ('row4', 160, 1, 0),
                     'dec.out_ln': ('row4', 160, 1, 0),
                     'dec.qkv': ('qkv4', 160, 1, 0),
                     'dur.conv0': ('pl_bf16', 64, 4, 1),
                     'dur.conv1': ('pl_bf16', 64, 4, 1),
                     'enc.ffn1': ('pl_mx', 64, 1, 0),
                     'enc.ffn2_ln': ('pl_bf16', 64, 4, 1),
                     'enc.out_ln': ('pl_bf16', 64, 2, 1),
                     'enc.qkv': ('pl_bf16', 64, 1, 0),
                     'energy.conv0': ('row8c', 192, 1, 0),
                     'feat_out': ('pl_bf16', 64, 1, 0),
                     'pitch.conv0': ('row8c', 192, 1, 0),
                     'postnet.0': ('pl_bf16', 128, 1, 0),
                     'postnet.1': ('pl_mx', 128, 1, 0),
                     'postnet.2': ('pl_mx', 128, 1, 0),
                     'postnet.3': ('pl_mx', 128, 1, 0),
                     'postnet.4': ('pl_bf16', 64, 1, 0),
                     'var.conv1': ('row8c_grouped', 192, 1, 0)}}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "gemm_plan_probe.cpp"), "-o", exe], check=True)
    return lambda *args: subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip().split("\n")


@pytest.fixture(scope="module")
def model_plans(probe):
    out = {}
    for regime, rows in REGIMES.items():
        for line in probe("model", *rows, TRACED_CASE):
            f = line.split()
            out[(regime, f[0], f[1])] = (f[2],) if f[1] == "capacity_independent" else (f[2], int(f[3]), int(f[4]), int(f[5]))
    return out


def test_gemm_plan_header_is_hip_free():
    for h in ("gemm_plan.h", "gemm_args.h", "model_launches.h", "attn_plan.h", "layout_rule.h", "call_plan.h", "weight_plan.h"):
        src = open(os.path.join(CSRC, h)).read()
        incl = [l.split()[1] for l in src.split("\n") if l.startswith("#include")]
        ours = ('"gemm_args.h"', '"gemm_plan.h"', '"layout_rule.h"', '"attn_plan.h"', '"model_launches.h"', '"../../include/fs2.h"')      # (fs2.h: plain C over stddef.h / stdint.h)
        assert all(i.startswith("<") and "hip" not in i or i in ours for i in incl), (h, incl)
    fs2_h = open(os.path.join(ROOT, "include", "fs2.h")).read()
    assert sorted(l.split()[1] for l in fs2_h.split("\n") if l.startswith("#include")) == ["<stddef.h>", "<stdint.h>"]


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("mode", MODES)
def test_pinned_plans(model_plans, regime, mode):
    want = PINNED[(regime, mode)]
    got = {k[2]: v for k, v in model_plans.items() if k[0] == regime and k[1] == mode and k[2] != "capacity_independent" and not k[2].endswith(".attn")}      # (test_attn_plan_host.py)
    for name in sorted(set(want) | set(got)):
        print("%s %s %-14s want %s got %s" % (regime, mode, name, want.get(name), got.get(name)))
    assert got == want


def _launches_of_trace(path):
    """(family, tile rows, ksplit, ln_rows pass) of every gemm_* dispatch of a condensed trace, in order (profiles/gemm_plan_trace_names.md)."""
    import re
    lines = open(path).read().split("\n")
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"(gemm_\w+)(?:<([^>]*)>)? grid=\d+,(\d+),(\d+) wg=\d+,(\d+),(\d+) ", l)
        if not m:
            continue
        k, t = m.group(1), (m.group(2) or "").split(",")
        gy, gz, rows = int(m.group(3)) // int(m.group(5)), int(m.group(4)) // int(m.group(6)), int(lines[i + 1].startswith("ln_rows"))
        if k == "gemm_pl_bf16":
            out.append((("pl_bf16", "pl_f16", "pl_mx", "pl_mx4")[int(t[3])], int(t[1]), gz, rows))
        elif k == "gemm_row4_bf16":
            out.append(("qkv4" if t[3] == "3" else "row4", 32 * int(t[2]), gz, rows))
        elif k == "gemm_row8c_bf16":
            out.append(("row8c_two_ln" if t[3] == "2" else ("row8c_grouped" if gy > 1 else "row8c"), 64 * int(t[2]), gz, rows))
        elif k in ("gemm_row8_bf16", "gemm_qkv8_bf16"):
            out.append((k[5:-5], 64 * int(t[2]), gz, rows))
        else:
            assert k in ("gemm_tile_f32", "gemm_rows_f32"), l
            out.append((("tile_rows_f32" if rows else "tile_f32") if k == "gemm_tile_f32" else "rows_f32", 0, 1, rows))
    return out


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("mode", MODES)
def test_pinned_table_is_the_parent_trace(regime, mode):
    """PINNED is what the committed kernel trace of the parent commit says, launch by launch: the table cannot follow the plan without the trace file changing."""
    got = _launches_of_trace(os.path.join(ROOT, "profiles", "gemm_plan_trace_parent_%s_%s.txt" % (regime, mode)))
    var = {4: ["energy.conv0", "energy.conv1", "pitch.conv0", "pitch.conv1"], 2: ["var.conv0", "var.conv1"], 3: ["energy.conv0", "pitch.conv0", "var.conv1"]}[len(got) - 41]
    block = ["qkv", "out_ln", "ffn1", "ffn2_ln"]
    names = (["enc." + b for _ in range(4) for b in block] + ["dur.conv0", "dur.conv1"] + var + ["dec.in"] + ["dec." + b for _ in range(4) for b in block] +
             ["feat_out"] + ["postnet.%d" % i for i in range(5)])
    table = {}
    for n, l in zip(names, got):
        assert table.setdefault(n, l) == l, (n, "the four blocks of a stack differ")
    assert table == PINNED[(regime, mode)]


def test_planes_only_agrees_with_the_old_predicate(probe):
    rows = [l.split() for l in probe("sweep")]
    assert len(rows) == 3 * 6 * 3 * 2 * 2 * 2
    assert {int(r[8]) for r in rows} == {0, 9, 10}      # plain, mx, mx4 FFN: the old predicate does not depend on the mode, nor may the answer
    assert {int(r[0]) for r in rows} == {1, 800, 16256, 16257, 36600, 78000}
    bad = [r for r in rows if not (r[5] == r[6] == r[7])]      # old predicate, plan at R = regime, plan at R = 1.25 x regime
    assert not bad, bad
    on = {(int(r[0]), int(r[1]), int(r[2]), r[3], int(r[4])) for r in rows if r[5] == "1"}
    assert all(sum(1 for r in rows if r[5] == "1" and (int(r[0]), int(r[1]), int(r[2]), r[3], int(r[4])) == k) == 3 for k in on)
    # the threshold (r + 127) / 128 >= 128 flips between 16256 and 16257 rows; the default configuration (ddim 384, bf16x3, no switch) is in the sweep
    assert (16257, -1, -1, "bf16x3", 384) in on and (16256, -1, -1, "bf16x3", 384) not in on
    assert (800, 1, -1, "bf16x3", 384) in on and (78000, 0, -1, "bf16x3", 384) not in on and (78000, -1, 0, "bf16x3", 384) not in on
    assert not any(k[3] == "bf16" or k[4] == 256 for k in on)


@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_plan_is_independent_of_the_capacity(model_plans, regime):
    for mode in MODES:
        assert model_plans[(regime, mode, "capacity_independent")] == ("1",), mode


ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -6      # include/fs2.h
REFUSALS = {
    "kernel_size": (ERR_UNSUPPORTED, "x: kernel size 18 > 17"),
    "channels": (ERR_UNSUPPORTED, "x: channels 258 / ld 256 must be multiples of 4"),
    "weight_image": (ERR_STATE, "x: no bf16 weight image"),
    "bf16_shape": (ERR_UNSUPPORTED, "x: bf16 path needs C % 8 == 0, N % 4 == 0 (N <= 1024 with a row epilogue)"),
    "no_planes": (ERR_STATE, "x: no activation planes and no scratch to build them"),
    "row_stride": (ERR_UNSUPPORTED, "x: bf16 path needs row strides that are multiples of 4"),
    "planes_only_off_row4": (ERR_STATE, "x: a planes-only launch (residual as planes / no fp32 rows) exists on gemm_row4_bf16 only and this one would not run there"),
    "col_off": (ERR_UNSUPPORTED, "x: a plane column offset exists in the row-complete conv kernel only"),
    "plane_slice": (ERR_UNSUPPORTED, "x: planes 2048 columns wide from a launch of 1024: filling a slice of a plane row exists in the row-complete conv kernel only"),
    "no_output": (ERR_ARG, "x: no output or scratch buffer"),
    "qkv_split": (ERR_UNSUPPORTED, "x: fused QKV split needs D % 128 == 0"),
    "f16_non_conv": (ERR_UNSUPPORTED, "x: the fp16 arithmetic exists for plain convolutions only"),
    "mx_shape": (ERR_UNSUPPORTED, "x: the mx arithmetic needs a convolution with C % 128 == 0 and N % 128 == 0"),
    "mx4_row_scales": (ERR_STATE, "x: the mx4 arithmetic needs mx4 planes with their row scales and the weight image's channel scales"),
    # these two were launchers returning hipErrorInvalidValue, which launch_gemm reported as "<name> launch: <hipGetErrorString>"
    "mx4_width": (ERR_HIP, "x launch: invalid argument"),
    "row4_mx_residual": (ERR_HIP, "x launch: invalid argument"),
    "f32_rows_width": (ERR_UNSUPPORTED, "x: row-epilogue GEMM needs N in {80,256,384}, got 100"),
    "accepted": (0, ""),
}


def test_refusals_keep_their_codes(probe):
    got = {}
    for line in probe("refusals"):
        what, err, msg = line.split("|")
        got[what] = (int(err), msg)
    assert got == REFUSALS
    import re
    hdr = open(os.path.join(ROOT, "include", "fs2.h")).read()
    for name, val in (("ARG", ERR_ARG), ("HIP", ERR_HIP), ("STATE", ERR_STATE), ("UNSUPPORTED", ERR_UNSUPPORTED)):
        assert int(re.search(r"#define FS2_ERR_%s \((-\d+)\)" % name, hdr).group(1)) == val


# The launches of one block in run_stack_general, written out by hand from the source of the commit before model_launches.h existed, in its order:
# pre-LN puts ln1 / ln2 in front of the sub-layers (and names the GEMMs out / ffn2: no LayerNorm follows them), concat_after replaces the out-projection's
# residual add by out, cat_x, cat_a.  (after_norm follows the last block of a pre-LN stack; the stack's runner launches it, it is no step of a block.)
_LN, _AT, _G = "layernorm", "attention", "gemm"
GENERAL_BLOCKS = {
    (True, False): [("ln1", _LN), ("qkv", _G), ("attn", _AT), ("out", _G), ("ln2", _LN), ("ffn1", _G), ("ffn2", _G)],
    (False, True): [("qkv", _G), ("attn", _AT), ("out", _G), ("cat_x", _G), ("cat_a", _G), ("ffn1", _G), ("ffn2", _G)],
    (True, True): [("ln1", _LN), ("qkv", _G), ("attn", _AT), ("out", _G), ("cat_x", _G), ("cat_a", _G), ("ln2", _LN), ("ffn1", _G), ("ffn2", _G)],
}
# tests/test_oracle_golden.py's variants: (pre_ln, concat_after) of the encoder and of the decoder
VARIANTS = {"pre_ln": ((True, False), (True, False)), "concat_after": ((False, True), (False, True)), "pre_ln_concat": ((True, True), (True, True)),
            "enc_pre_ln_dec_concat": ((True, False), (False, True))}


def test_block_variants_form_the_launches_of_run_stack_general(probe):
    got = {}
    for line in probe("variants", *REGIMES["c1"]):
        variant, mode, name, kind, err = line.split()
        got.setdefault((variant, mode), []).append((name, kind, int(err)))
    assert set(got) == {(v, m) for v in VARIANTS for m in MODES}
    for (variant, mode), steps in sorted(got.items()):
        enc, dec = VARIANTS[variant]
        want = [("enc." + n, k) for n, k in GENERAL_BLOCKS[enc]] + [("dec." + n, k) for n, k in GENERAL_BLOCKS[dec]]
        assert [(n, k) for n, k, _ in steps] == want, (variant, mode)
        assert all(err == 0 for _, _, err in steps), (variant, mode, steps)
