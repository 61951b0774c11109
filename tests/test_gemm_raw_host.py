"""CPU checks of tests/gemm_raw.py, the helper of the kernel-level GEMM tests (tests/test_gpu_row_kernels.py, ..._mx_kernels.py, ..._pred_kernels.py): all of them must pass before a block
is sent to a GPU.

(a) the ctypes mirror of fs2::GemmArgs against csrc/gemm_args.h as the host compiler lays it out (tests/gemm_raw_probe.cpp), and the kernel names
    against the enumerators of GemmKernel;
(b) the operand encoders / decoders: exact round trips, the in-chunk position a bijection and equal to csrc/common.h's plane_byte written out again
    byte by byte, the pair values equal to bf16 / fp16 / e4m3 arithmetic stated independently;
(c) the float64 reference against a plain F.linear + F.layer_norm fp32 statement;
(d) the plan of every argument block the GPU tests send, from csrc/gemm_plan.h compiled for the host on the block's own bytes: the expected kernel,
    epilogue, residual form and tile height, and no refusal;
(e) the formats of the mixed modes (tests/test_gpu_mx_kernels.py): the e2m1 codec, the scale rule against csrc/common.h compiled for the host, the byte positions
    of the mx4 planes, their scale record, both weight images and the scale image written out again element by element, the formulas near the ideal product,
    and DISCRIMINATION: every mutant of a formula -- what a kernel with one broken position rule would compute -- at 8 bars or more from it;
(f) the variance predictors' conv launches (tests/test_gpu_pred_kernels.py): the conv weight image against repack_weight_bf16's index arithmetic, the row pattern,
    ref_pred against F.conv1d + F.layer_norm utterance by utterance, the variants, the fp32 statement below an eighth of the bars, every mutant at 8 bars or more on
    the rows it concerns, and the refusal of a half launch where the row-complete conv kernel does not run."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_raw as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_raw")
    exe = str(d / "probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "gemm_raw_probe.cpp"), "-o", exe], check=True)
    return lambda *args: [l.split() for l in subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.strip().split("\n")]


def test_argument_block_mirror_matches_the_compiled_header(probe):
    lines = probe("layout")
    assert lines[0] == ["sizeof", str(ctypes.sizeof(G.GemmArgs))]
    assert [l[0] for l in lines[1:]] == [f[0] for f in G.GemmArgs._fields_]          # every field, in the header's order
    for name, off in lines[1:]:
        assert getattr(G.GemmArgs, name).offset == int(off), name
    # every byte of the struct is a field or padding the compiler also leaves: the last field ends within 8 bytes of the size
    last = G.GemmArgs._fields_[-1][0]
    assert ctypes.sizeof(G.GemmArgs) - getattr(G.GemmArgs, last).offset - getattr(G.GemmArgs, last).size < 8


def test_kernel_names_follow_the_enumerators(probe):
    assert [(int(v), n) for v, n in probe("kernels")] == list(enumerate(G.KERNELS))


def _plane_byte(row, nchunks, c):
    """csrc/common.h: plane_byte, written out again."""
    return (row * nchunks + (c >> 5)) * 128 + (((c & 15) >> 2) << 4) + (((c >> 4) & 1) << 3)


def _kperm(p):
    """csrc/gemm_bf16.h: kperm, the channel at k-position p of a chunk (repack_weight_bf16's order)."""
    slot, j = p >> 3, p & 7
    return 4 * slot + j if j < 4 else 16 + 4 * slot + (j - 4)


def test_in_chunk_position_is_the_bijection_of_the_kernels():
    pos = [G.chunk_pos(c) for c in range(32)]
    assert sorted(pos) == list(range(32))
    assert all(_kperm(G.chunk_pos(c)) == c for c in range(32))                        # the weight image's order
    assert all(2 * G.chunk_pos(c) == _plane_byte(0, 1, c & ~3) + 2 * (c & 3) for c in range(32))      # the planes' bytes


def test_split_bf16_planes_round_trip_and_byte_positions():
    rs = np.random.RandomState(0)
    rows, Cc = 5, 96
    x = torch.from_numpy(rs.uniform(-3, 3, size=(rows, Cc)).astype(np.float32))
    hi, lo = G.split_bf16(x)
    # bf16 arithmetic stated independently: round to nearest even on the upper 16 bits
    def bf16_bits(v):
        u = v.contiguous().view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF
        return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(hi.view(torch.int16).numpy().view(np.uint16), bf16_bits(x))
    assert np.array_equal(lo.view(torch.int16).numpy().view(np.uint16), bf16_bits(x - hi.float()))
    assert float((lo.float().abs() - 2.0 ** -8 * hi.float().abs()).max()) <= 0.0
    v = G.pair_value(hi, lo)
    assert bool((v.float().double() == v).all()) and float((v - x.double()).abs().max()) <= 2.0 ** -16 * 3
    img = G.encode_planes(hi, lo)
    assert img.shape == (rows, Cc * 2) and img.dtype == torch.bfloat16
    raw = img.view(torch.int16).numpy().view(np.uint16).reshape(-1)                  # the image as 16-bit words
    for r in range(rows):
        for c in range(Cc):
            b = _plane_byte(r, Cc // 32, c & ~3) + 2 * (c & 3)
            assert raw[b // 2] == hi.view(torch.int16).numpy().view(np.uint16)[r, c]
            assert raw[(b + 64) // 2] == lo.view(torch.int16).numpy().view(np.uint16)[r, c]
    h2, l2 = G.decode_planes(img, rows, Cc)
    assert torch.equal(h2.view(torch.int16), hi.view(torch.int16)) and torch.equal(l2.view(torch.int16), lo.view(torch.int16))
    # the decoder takes raw bytes with a tail behind them (the output buffers of the GPU tests)
    tail = torch.cat([img.view(torch.uint8).reshape(-1), torch.full((64,), 0xFF, dtype=torch.uint8)])
    assert torch.equal(G.decode_planes(tail, rows, Cc)[0].view(torch.int16), hi.view(torch.int16))


def _e4m3_value(b):
    """OCP e4m3 (finite-only variant), decoded by hand."""
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


def test_mx_planes_round_trip_and_value():
    rs = np.random.RandomState(1)
    rows, Cc, ka = 4, 128, G.KA_RES
    x = torch.from_numpy(rs.uniform(-1, 1, size=(rows, Cc)).astype(np.float32))
    h, e8 = G.split_mx(x, ka)
    img = G.encode_mx(h, e8, ka)
    assert img.shape == (rows, 4 * Cc) and img.dtype == torch.uint8
    raw = img.numpy()
    hb = h.view(torch.int16).numpy().view(np.uint16)
    for r in range(rows):
        for c in range(Cc):
            assert int(raw[r, 2 * c]) | (int(raw[r, 2 * c + 1]) << 8) == int(hb[r, c])
            assert raw[r, 2 * Cc + c] == e8[r, c]
    h2, e2, a2 = G.decode_mx(img, rows, Cc)
    assert torch.equal(h2.view(torch.int16), h.view(torch.int16)) and torch.equal(e2, e8)
    want = torch.tensor([[float(h[r, c]) + _e4m3_value(int(e8[r, c])) * 2.0 ** -(ka + 11) for c in range(Cc)] for r in range(rows)], dtype=torch.float64)
    v = G.mx_value(h, e8, ka)
    assert torch.equal(v, want)
    assert bool((v.float().double() == v).all())                                     # exact in fp32: what gemm_row8_bf16 gets as the reconstructed residual
    assert float((v - x.double()).abs().max()) <= 2.0 ** -14                         # fp16 + 2^-4 of half an fp16 ulp at |x| < 1
    # the third block: e4m3(fp16 2^ka), nearest
    a_val = torch.tensor([[_e4m3_value(int(a2[r, c])) for c in range(Cc)] for r in range(rows)], dtype=torch.float64)
    assert float((a_val - h.double() * 2.0 ** ka).abs().max()) <= 2.0 ** -4 * 8      # half a 3-bit-mantissa ulp below 16
    assert not bool(((img[:, 2 * Cc:] & 0x7F) == 0x7F).any())


def test_float64_reference_against_a_plain_fp32_statement():
    rs = np.random.RandomState(2)
    R, Cc, N = 50, 96, G.N_OUT
    u = lambda *s, scale=1.0: torch.from_numpy(rs.uniform(-scale, scale, size=s).astype(np.float32))
    x, w, b, r, g, bt, pe = u(R, Cc), u(N, Cc, scale=Cc ** -0.5), u(N, scale=0.5), u(R, N), 1 + u(N, scale=0.2), u(N, scale=0.2), u(16, N)
    pos = torch.arange(R).int() % 17 - 1                                              # some rows are gaps
    live = (pos >= 0).unsqueeze(1)
    got = G.ref_rows(x.double(), w.double(), b.double(), r.double(), g.double(), bt.double(), pos)
    want = F.layer_norm(F.linear(x, w, b) + r, (N,), g, bt, 1e-5) * live
    assert float((got - want.double()).abs().max()) < 1e-5
    got = G.ref_rows(x.double(), w.double(), b.double(), None, g.double(), bt.double(), pos, relu=True, x_scale=1.25, pe=pe.double(), alpha=0.9)
    want = (1.25 * torch.relu(F.layer_norm(F.linear(x, w, b), (N,), g, bt, 1e-5)) + 0.9 * pe[pos.clamp(min=0).long()]) * live
    assert float((got - want.double()).abs().max()) < 1e-5
    D = N // 3
    q, k, v = G.ref_qkv(x.double(), w.double(), b.double(), pos, D, 0.25)
    y = F.linear(x, w, b) * live
    assert max(float((q - 0.25 * y[:, :D].double()).abs().max()), float((k - y[:, D:2 * D].double()).abs().max()), float((v - y[:, 2 * D:].double()).abs().max())) < 1e-5


def test_operands_are_exact_pairs_on_the_tested_distributions():
    ops = G.LnOperands("epi0_res2", 128, 384)
    assert ops.ref.shape == (128, G.N_OUT) and bool(torch.isfinite(ops.ref).all())
    assert float(ops.ref[ops.pos[:128] < 0].abs().max()) == 0.0 and int((ops.pos[:128] < 0).sum()) == 8
    assert int(ops.pos.max()) < ops.pe.shape[0] and ops.pos.numel() == G.rpad(128) and bool((ops.pos[128:] == -1).all())
    G._exact_f32(ops.resid_value)
    assert ops.resid_planes.shape == (G.rpad(128), 4 * G.N_OUT)
    assert G.rpad(333) == 576 and G.rpad(128) == 384


def _plans(probe, tmp_path, launches):
    """The compiled plan of every (id, switches, block, expected) under its switches and its precision: {id: {field: value, "err": code}}."""
    path = tmp_path / "blocks.txt"
    with open(path, "w") as f:
        for name, opts, block, want in launches:
            f.write("%s %d %s %s\n" % (name, G.PREC_CODE[want.get("precision", "bf16x3")], ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "-", bytes(block).hex()))
    fields = ("kernel",) + G.Plan._fields[1:] + ("err",)
    return {l[0]: dict(zip(fields, [l[1]] + [int(v) for v in l[2:]])) for l in probe("plans", path)}


def test_every_block_the_gpu_tests_send_plans_onto_the_expected_kernel(probe, tmp_path):
    launches = G.all_launches()
    n_mixed = len(G.CONV_ARITHS) * len(G.CONV_CASES) * len(G.CONV_OUTS) + 2 * len(G.EPI4_CASES) + 3 * len(G.FFN2_CASES)
    n_pred = sum(len(G.pred_runs(c[0])) for c in G.PRED_CASES)
    assert len(launches) == 4 * len(G.LN_CASES) + sum(len(r) for r in G.QKV_RUNS.values()) + n_mixed + n_pred and len({l[0] for l in launches}) == len(launches)
    got = _plans(probe, tmp_path, launches)
    assert sorted(got) == sorted(l[0] for l in launches)
    for name, _, _, want in launches:
        want = {k: v for k, v in want.items() if k != "precision"}
        assert got[name]["err"] == 0, (name, got[name])
        assert {k: got[name][k] for k in want} == want, (name, got[name])
        # (the conv in the mx arithmetics has one MFMA term per unit kind: its plan says nsplit 1, and the block's expectation names it; the predictors' siblings
        #  name their split-K and their rows pass)
        assert got[name]["nsplit"] == want.get("nsplit", 3) and got[name]["ksplit"] == want.get("ksplit", 1), (name, got[name])
        assert got[name]["rows_pass"] == want.get("rows_pass", 0) and not got[name]["build_planes"], (name, got[name])
    # every instantiation family the issue names is reached: both heights of the four row4 forms, the QKV passes on it, gemm_qkv8_bf16 whole and apart
    reached = {(g["kernel"], g["epi"], g["res"], g["mt"], g["apart"]) for g in got.values()}
    for epi, res in ((0, 1), (0, 2), (1, 1), (2, 3), (4, 1)):
        assert {("row4", epi, res, 4, 0), ("row4", epi, res, 5, 0)} <= reached
    # ... and the launches of the mixed modes: the conv on mx and on mx4 operands, FFN2 + LN2 in the mx arithmetic at both heights
    assert {(g["kernel"], g["arith"], g["bm"]) for g in got.values() if g["kernel"].startswith("pl_mx")} == {("pl_mx4", 3, 256), ("pl_mx", 2, 64)}
    assert {("row4", 0, 2, 2, m) for m in (4, 5)} <= {(g["kernel"], g["epi"], g["arith"], g["res"], g["mt"]) for g in got.values()}
    assert {("qkv4", 3, 0, 4, 0), ("qkv4", 3, 0, 5, 0)} | {("qkv8", -1, 0, m, s) for m in (2, 3) for s in (0, 1)} | {("row8", -1, 0, 2, 0), ("row8", -1, 0, 3, 0)} <= reached


# ------------------------------------------------------------------ the mx / mx4 formats (tests/test_gpu_mx_kernels.py)
def test_bars_of_the_mixed_mode_launches_respect_the_ceiling():
    assert set(G.MX_BAR) == {"conv_mx4", "conv_mx", "ffn2_mx", "epi4"} and all(0 < b <= G.MX_CEILING for b in G.MX_BAR.values())


def test_e2m1_codec_rounds_to_nearest_even_and_saturates():
    codes = torch.arange(16, dtype=torch.uint8)
    vals = G.e2m1_decode(codes)
    assert vals.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    assert torch.equal(G.e2m1_encode(vals), codes)                                      # (the sign of a zero is kept: code 8)
    # nearest: a fine grid against the brute-force nearest code; the seven midpoints go to the code with the even mantissa bit
    x = torch.arange(-8.0, 8.0, 1.0 / 64, dtype=torch.float64)
    x = x[~G.e2m1_on_tie(x)]
    near = (x.unsqueeze(1) - vals[:8].unsqueeze(0) * torch.sign(x).unsqueeze(1)).abs().argmin(1)
    assert torch.equal((G.e2m1_encode(x) & 7).long(), near) and torch.equal(G.e2m1_encode(x) >> 3, (x < 0).to(torch.uint8))
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=torch.float64)
    assert G.e2m1_encode(ties).tolist() == [0, 2, 2, 4, 4, 6, 6] and G.e2m1_encode(-ties).tolist() == [8, 10, 10, 12, 12, 14, 14]
    assert G.e2m1_encode(torch.tensor([6.0, 7.0, 1e30, -1e30])).tolist() == [7, 7, 7, 15]
    assert int(G.e2m1_on_tie(ties).sum()) == 7 and not bool(G.e2m1_on_tie(vals).any())


def test_mx4_scale_rule_matches_the_compiled_header(tmp_path):
    """mx4_scale_byte / mx4_inv_scale of csrc/common.h, compiled for the host, on every binade edge, its neighbours, zero, denormals and the clamped ends."""
    exe = str(tmp_path / "mx_format_probe")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-host-only", "-std=c++17", "-I", CSRC,
                    os.path.join(ROOT, "tests", "mx_format_probe.cpp"), "-o", exe], check=True)
    bits = [0, 1, 0x007FFFFF, 0x7F7FFFFF]
    for e in list(range(1, 255, 7)) + [41, 42, 43, 201, 202, 203, 127]:
        bits += [(e << 23) - 1, e << 23, (e << 23) + 1, (e << 23) | 0x400000]
    out = subprocess.run([exe] + ["%08x" % b for b in bits], check=True, capture_output=True, text=True).stdout.split()
    got_byte, got_inv = [int(v) for v in out[1::3]], [int(v, 16) for v in out[2::3]]
    m = torch.tensor(np.array(bits, dtype=np.uint32).view(np.float32))
    eb = G.mx4_scale_byte(m)
    assert eb.tolist() == got_byte and int(eb.min()) == 40 and int(eb.max()) == 200
    assert G.mx4_inv_scale(eb).float().view(torch.int32).tolist() == got_inv
    # the rule: m / 2^(byte - 127) lies in [4, 8) wherever the clamp does not act
    free = (eb > 40) & (eb < 200)
    q = m.double()[free] * G.mx4_inv_scale(eb[free])
    assert bool(((q >= 4) & (q < 8)).all())
    assert G.fp8_scale_exponent(448.0) == 0 and G.fp8_scale_exponent(1.0) == 8 and G.fp8_scale_exponent(8.0) == 5 and G.fp8_scale_exponent(0.0) == 0
    assert G.scale_byte4(113) == 0x71717171 and G.scale_byte4(0) == 0x01010101


def test_mx4_planes_round_trip_and_byte_positions():
    rs = np.random.RandomState(3)
    rows, Cc, ka = 5, 384, 3
    x = torch.from_numpy(rs.uniform(-1, 1, size=(rows, Cc)).astype(np.float32)) * G._gain(rs, Cc)
    x[3] = 0.0                                                                            # a row of zeros: the clamped scale byte
    t = G.split_mx4(x, ka)
    planes, rec = G.encode_mx4(t, fill=0xEE)
    assert planes.shape == (rows, 4 * Cc) and rec.shape == (rows, 32) and planes.dtype == rec.dtype == torch.uint8
    hb = t.h.view(torch.int16).numpy().view(np.uint16)
    raw = planes.numpy()
    for r in range(rows):
        for c in range(Cc):
            assert int(raw[r, 2 * c]) | (int(raw[r, 2 * c + 1]) << 8) == int(hb[r, c])
            q, j = c & ~3, c & 3                                                          # the four channels c & ~3 .. + 3 own bytes 2 C + (c & ~3) .. + 3
            assert (int(raw[r, 2 * Cc + q + (j >> 1)]) >> (4 * (j & 1))) & 15 == int(t.r4[r, c])          # ra4 ra4 | ra4 ra4
            assert (int(raw[r, 2 * Cc + q + 2 + (j >> 1)]) >> (4 * (j & 1))) & 15 == int(t.h4[r, c])      # ah4 ah4 | ah4 ah4
            assert raw[r, 3 * Cc + c] == t.e8[r, c]
        for S in range(Cc // 16):
            u, sl = S // 8, S % 8
            assert int(rec[r, 8 * u + 2 * (sl & 3) + (sl >> 2)]) == int(t.sb[r, S]) - 11
    assert sorted(G.slot_pos(S) for S in range(24)) == list(range(24)) and bool((rec[:, 24:] == 0xEE).all())
    assert t.sb[3].tolist() == [40] * 24 and not bool(planes[3].any())
    back = G.decode_mx4(planes, rec, rows, Cc)
    for a, b in zip(t, back):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)
    # the parts: under the slot's scale the fp16 part lands in e2m1's range with the slot maximum in [4, 8) -> code 6 or 7; both parts within half a step
    inv = G.mx4_inv_scale(t.sb).repeat_interleave(16, dim=1)
    hs, rsd = t.h.double() * inv, (x - t.h.float()).double() * 2048.0 * inv
    live = torch.ones(rows, dtype=torch.bool)
    live[3] = False
    assert int((G.e2m1_decode(t.h4).abs().reshape(rows, -1, 16).amax(2)[live]).min()) >= 4
    for v, code in ((hs, t.h4), (rsd, t.r4)):
        err = (G.e2m1_decode(code) - v.clamp(-6, 6)).abs()
        assert bool((err <= torch.where(v.abs() >= 4, 1.0, torch.where(v.abs() >= 2, 0.5, 0.25))).all())
    assert float((x - t.h.float()).abs().max()) * 2.0 ** (ka + 11) <= 448.0


def test_weight_images_byte_positions_and_scale_image():
    rs = np.random.RandomState(4)
    N, Cc, k = 256, 384, 3
    w = G.repack_weights(N, Cc, k, 4)
    kw = G.fp8_scale_exponent(float(w.abs().max()))
    assert float(w.abs().max()) * 2.0 ** kw <= 448.0 < float(w.abs().max()) * 2.0 ** (kw + 1)
    t3, t4 = G.split_mx3(w, kw), G.split_mx4(w, 0, slot_dim=1)
    img3 = G.image_w_mx(t3).numpy()
    img4, sc = G.image_w_mx4(t4)
    img4, sc = img4.numpy(), sc.numpy()
    assert img3.shape == (N, Cc // 32, k, 128) and img4.shape == (N, Cc // 64 + Cc // 128, k, 128) and sc.shape == (N // 128, Cc // 128, k, 4, 128, 2)
    assert t4.sb.shape == (N, Cc // 16, k) and len(torch.unique(t4.sb)) > 4              # the blocks take different scale bytes
    hb = t3.h.view(torch.int16).numpy().view(np.uint16)
    nmain, ncross = Cc // 64, Cc // 128
    for n, c, tap in [(int(rs.randint(N)), int(rs.randint(Cc)), int(rs.randint(k))) for _ in range(3000)] + [(0, 0, 0), (N - 1, Cc - 1, k - 1), (128, 127, 1), (127, 128, 1)]:
        for img in (img3, img4):                                                          # fp16 channels: unit c / 64, two bytes at 2 (c % 64)
            assert int(img[n, c // 64, tap, 2 * (c % 64)]) | (int(img[n, c // 64, tap, 2 * (c % 64) + 1]) << 8) == int(hb[n, c, tap])
        assert img3[n, nmain + c // 128, tap, c % 128] == t3.a8[n, c, tap]                # wh8 meets ra8: the first C / 128 units behind the fp16 ones
        assert img3[n, nmain + ncross + c // 128, tap, c % 128] == t3.r8[n, c, tap]       # rw8 meets ah8
        q, j = (c % 128) & ~3, c & 3
        assert (int(img4[n, nmain + c // 128, tap, q + (j >> 1)]) >> (4 * (j & 1))) & 15 == int(t4.h4[n, c, tap])          # wh4 where the planes hold ra4
        assert (int(img4[n, nmain + c // 128, tap, q + 2 + (j >> 1)]) >> (4 * (j & 1))) & 15 == int(t4.r4[n, c, tap])      # rw4 where they hold ah4
        sl = (c % 128) // 16
        assert sc[n // 128, c // 128, tap, sl & 3, n % 128, sl >> 2] == int(t4.sb[n, c // 16, tap])
    # the value: fp16 + both reduced copies state w to the precision of their formats
    assert float((G.e4m3_value(t3.a8) * 2.0 ** -kw - t3.h.double()).abs().max()) <= 2.0 ** -4 * float(w.abs().max())
    assert float((G.e4m3_value(t3.r8) * 2.0 ** -(kw + 11) - (w - t3.h.float()).double()).abs().max()) <= 2.0 ** -4 * 2.0 ** -11 * float(w.abs().max())


def test_formulas_state_the_product_to_the_precision_of_the_formats():
    """The float64 formulas are the kernels', not the ideal product -- but they must be NEAR it: against F.conv1d / F.linear of the fp32 values in float64 the mx
    formula drops ra.rw (2^-22) and keeps 2^-4 of the cross terms (2^-15 per product), the mx4 formula keeps about a quarter of them (2^-13 per product)."""
    for arith, tol in (("mx", 2.0 ** -14), ("mx4", 2.0 ** -11)):
        o = G.ConvOperands(arith, 3, 256, 256, "model")
        a = o.x.h.double() + (G.e4m3_value(o.x.r8) * 2.0 ** -(o.ka + 11) if arith == "mx" else G.e4m3_value(o.x.e8) * 2.0 ** -(o.ka + 11))
        if arith == "mx":
            w = o.w.h.double() + G.e4m3_value(o.w.r8) * 2.0 ** -(o.kw + 11)
        else:
            w = o.w.h.double() + G.e2m1_decode(o.w.r4) * G.pow2(o.w.sb - 127).repeat_interleave(16, dim=1) * 2.0 ** -11
        want = torch.relu(F.conv1d(a[:o.R].t().unsqueeze(0), w, o.bias.double(), padding=1)[0].t()) * (o.pos[:o.R] >= 0).unsqueeze(1)
        scale = float(F.conv1d(a[:o.R].abs().t().unsqueeze(0), w.abs(), None, padding=1).max())      # Sum |a| |w|: what a relative error per product scales with
        assert float((o.ref - want).abs().max()) <= tol * scale, (arith, float((o.ref - want).abs().max()), scale)
        assert float(o.ref[o.pos[:o.R] < 0].abs().max()) == 0.0 and float(o.ref.min()) == 0.0 and float(o.ref.max()) > 0.5


def _discrimination(ops):
    worst = {}
    for m in ops.mutants():
        worst[m] = float((ops.mutant(m) - ops.ref).abs().max())
    return worst


@pytest.mark.parametrize("arith", G.CONV_ARITHS)
@pytest.mark.parametrize("case", G.CONV_CASES, ids=["k%d-N%d-R%d" % c for c in G.CONV_CASES])
def test_conv_formula_tells_every_mutant_apart(arith, case):
    """On the coherent operands every mutant of the formula -- cross terms dropped, the two scale bytes of a lane's pair swapped, the scale image's g index off by
    one, ra4 / ah4 nibble pairs swapped (mx: the ra8 and ah8 units swapped) -- lies at least 8 bars from the formula: a kernel that passes the bar is none of them."""
    ops = G.ConvOperands(arith, *case, "coherent")
    worst = _discrimination(ops)
    print(arith, case, worst)
    assert set(worst) == set(G.MX4_MUTANTS if arith == "mx4" else G.MX_MUTANTS)
    # (the bar the GPU test applies to this launch's fp32 rows; read back from mx planes an output carries 2^-14 |ref| of rounding on top: a mutant must clear that too)
    assert min(worst.values()) >= 8 * G.MX_BAR["conv_" + arith] and min(worst.values()) >= 2 * (G.MX_BAR["conv_" + arith] + 2.0 ** -14 * float(ops.ref.abs().max())), worst


@pytest.mark.parametrize("case", G.FFN2_CASES, ids=["C%d-R%d-rm%d" % c for c in G.FFN2_CASES])
def test_ffn2_formula_tells_every_mutant_apart(case):
    """... and for FFN2 + LN2 in the mx arithmetic; with the residual from mx4 planes also the residual bytes taken from 2 C (the cross units) instead of 3 C."""
    ops = G.Ffn2Operands(*case, "coherent")
    worst = _discrimination(ops)
    print(case, worst)
    assert ("resid_at_2c" in worst) == (case[2] == 2)
    assert min(worst.values()) >= 8 * G.MX_BAR["ffn2_mx"], worst


@pytest.mark.parametrize("case", G.EPI4_CASES, ids=["%s-R%d-C%d" % c for c in G.EPI4_CASES])
def test_epi4_operands_leave_few_slots_on_a_binade_edge(case):
    """From the reference alone: slots whose maximum lies within the bar of a power of two (where a kernel inside the bar may take either neighbouring scale byte) stay
    below 1 % of all slots; gamma spreads the slots of a row over several bytes."""
    ops = G.LnOperands(*case)
    bar = G.MX_BAR["epi4"] + 2.0 ** -14 * ops.ref.abs()
    lo, hi = G.epi4_scale_bounds(ops.ref, bar)
    assert bool((hi - lo >= 0).all()) and int((hi - lo).max()) <= 1
    print("edge slots: %d of %d" % (int((hi != lo).sum()), lo.numel()))
    assert int((hi != lo).sum()) < 0.01 * lo.numel()
    live = ops.pos[:ops.R] >= 0
    assert int((lo[live].max(1).values - lo[live].min(1).values).min()) >= 4              # 80-fold gamma: at least 2^4 between the slots of every live row
    assert bool((lo[~live] == 40).all()) and bool((hi[~live] == 40).all())
    assert float(ops.ref.abs().max()) * 2.0 ** -11 * 2.0 ** (G.KA_OUT + 11) <= 448.0       # the e4m3 residual under 2^ka stays finite


def test_e4m3_cells_contain_what_rounds_to_them():
    rs = np.random.RandomState(5)
    v = torch.from_numpy(rs.uniform(-300, 300, size=20000).astype(np.float32)) * torch.from_numpy(2.0 ** rs.randint(-12, 1, size=20000).astype(np.float32))
    b = G.e4m3_of(v)
    lo, hi = G.e4m3_cell(b)
    assert bool(((v.double() >= lo) & (v.double() <= hi)).all())
    assert bool((hi - lo <= 32.0).all()) and bool((lo <= G.e4m3_value(b)).all()) and bool((G.e4m3_value(b) <= hi).all())


# ------------------------------------------------------------------ the variance predictors' conv launches (tests/test_gpu_pred_kernels.py)
_pred_cache = {}


def _pred_ops(case):
    if case not in _pred_cache:
        _pred_cache[case] = G.PredOperands(*case)
    return _pred_cache[case]


def test_conv_weight_image_round_trip_and_byte_positions():
    """encode_w_conv against repack_weight_bf16's index arithmetic (csrc/gemm_bf16.h) written out again; at k = 1 the image is encode_planes'."""
    rs = np.random.RandomState(6)
    N, Cc, k = 6, 96, 3
    hi, lo = G.split_bf16(torch.from_numpy(rs.uniform(-1, 1, size=(N, Cc, k)).astype(np.float32)))
    img = G.encode_w_conv(hi, lo)
    assert img.shape == (N, Cc // 32, k, 64) and img.dtype == torch.bfloat16
    raw = img.view(torch.int16).numpy().view(np.uint16).reshape(-1)
    hb, lb = hi.view(torch.int16).numpy().view(np.uint16), lo.view(torch.int16).numpy().view(np.uint16)
    nchunks = Cc // 32
    seen = set()
    for n in range(N):
        for chunk in range(nchunks):
            for tap in range(k):
                for kk in range(32):
                    c = chunk * 32 + _kperm(kk)
                    base = ((n * nchunks + chunk) * k + tap) * 64
                    assert raw[base + kk] == hb[n, c, tap] and raw[base + 32 + kk] == lb[n, c, tap]
                    seen.add((n, c, tap))
    assert len(seen) == N * Cc * k
    # round trip: the positions are a bijection
    back_hi = img[:, :, :, G._POS].permute(0, 1, 3, 2).reshape(N, Cc, k)
    back_lo = img[:, :, :, 32 + G._POS].permute(0, 1, 3, 2).reshape(N, Cc, k)
    assert torch.equal(back_hi.view(torch.int16), hi.view(torch.int16)) and torch.equal(back_lo.view(torch.int16), lo.view(torch.int16))
    h1, l1 = hi[:, :, :1].contiguous(), lo[:, :, :1].contiguous()
    assert torch.equal(G.encode_w_conv(h1, l1).reshape(N, -1).view(torch.int16), G.encode_planes(h1[:, :, 0], l1[:, :, 0]).view(torch.int16))
    # a grouped layer: the image of the stacked weights is the groups' images stacked along N
    assert torch.equal(img[3:].view(torch.int16), G.encode_w_conv(hi[3:], lo[3:]).view(torch.int16))


def test_pred_row_pattern_keeps_every_boundary_row_live():
    for R in (333, 128):
        pos = G.pred_positions(R)
        live = pos >= 0
        assert pos.numel() == G.rpad(R) and bool((pos[R:] == -1).all()) and int(pos[0]) == 0
        for r in [0, R - 1] + [e + d for e in (128, 192, 256) for d in (-1, 0) if e < R]:
            assert bool(live[r]) and (r == 0 or bool(live[r - 1])) and (r == R - 1 or bool(live[r + 1])), (R, r)
        gaps = [r for r in range(R) if not bool(live[r])]
        assert gaps == [r for r in range(R) if (r + 4) % 109 < 4] and len(gaps) == (12 if R == 333 else 4)
        # positions count up inside an utterance
        assert all(int(pos[r]) == int(pos[r - 1]) + 1 for r in range(1, R) if bool(live[r]) and bool(live[r - 1]))
    assert sorted({c[3] for c in G.PRED_CASES}) == [128, 333] and len(G.PRED_IDS) == len(set(G.PRED_IDS)) == len(G.PRED_CASES) == 25


@pytest.mark.parametrize("case", [("mid", 256, 3, 333, ""), ("head", 256, 5, 128, ""), ("two_ln", 256, 3, 333, ""), ("grouped", 384, 3, 333, ""), ("grouped", 256, 3, 128, "quiet"),
                                  ("head", 256, 3, 128, "dead_window")], ids=lambda c: "-".join(str(v) for v in c if v != ""))
def test_pred_reference_against_conv1d_and_layer_norm(case):
    """ref_pred against F.conv1d + F.layer_norm in float64, utterance by utterance (each on its own: what the zero gap rows of the packed layout stand for)."""
    o = _pred_ops(case)
    R, k, P, Ng, Nl = o.R, o.k, o.P, o.N // o.kg, o.N // o.lg
    live = (o.pos[:R] >= 0)
    starts = [r for r in range(R) if bool(live[r]) and (r == 0 or not bool(live[r - 1]))]
    assert len(starts) == (4 if R == 333 else 2)
    want_v, want_h = torch.zeros(R, o.N, dtype=torch.float64), torch.zeros(R, o.lg, dtype=torch.float64)
    for s in starts:
        e = s
        while e < R and bool(live[e]):
            e += 1
        xu = o.xv[s:e].t().unsqueeze(0)                                                    # [1, Cx, L]
        y = torch.cat([F.conv1d(xu[:, g * o.Cg:(g + 1) * o.Cg], o.wv[g * Ng:(g + 1) * Ng], o.bias.double()[g * Ng:(g + 1) * Ng], padding=P) for g in range(o.kg)], dim=1)[0].t()
        y = torch.relu(y)
        for g in range(o.lg):
            cs = slice(g * Nl, (g + 1) * Nl)
            v = F.layer_norm(y[:, cs], (Nl,), o.gamma.double()[cs], o.beta.double()[cs], 1e-12)
            want_v[s:e, cs] = v
            want_h[s:e, g] = v @ o.dot_w.double()[cs] + o.dot_b.double()[g]
    assert float((o.ref.v - want_v).abs().max()) < 1e-9 * max(1.0, float(o.ref.rstd.max()) * o.s)
    assert float(o.ref.v[~live].abs().max()) == 0.0
    if o.has_head:
        assert float((o.ref.head - want_h).abs().max()) < 1e-8 * max(1.0, float(o.ref.rstd.max()) * o.s) and float(o.ref.head[~live].abs().max()) == 0.0
    else:
        assert o.ref.head is None
    assert o.ref.rstd.shape == (R, o.lg) and o.ref.yhat.shape == (R, o.N)
    assert float((o.ref.yhat.reshape(R, o.lg, -1).mean(2)).abs().max()) < 1e-9


def test_pred_operands_are_exact_pairs_and_the_variants_what_they_claim():
    loud, quiet = _pred_ops(("grouped", 256, 3, 128, "")), _pred_ops(("grouped", 256, 3, 128, "quiet"))
    for o in (loud, quiet):
        G._exact_f32(G.pair_value(*o.x))
        G._exact_f32(o.wv)
        assert float((o.x[1].float().abs() - 2.0 ** -8 * o.x[0].float().abs()).max()) <= 0.0
        gap = o.pos < 0
        assert not bool(G.encode_planes(*o.x).view(torch.int16)[gap].any())               # zero BYTES in gap rows and behind R
    # quiet: the pairs and the bias are the loud ones x 2^-10 exactly, so every fp32 product and sum of the kernel is the loud one's x 2^-10
    assert torch.equal(quiet.x[0].float() * 1024.0, loud.x[0].float()) and torch.equal(quiet.x[1].float() * 1024.0, loud.x[1].float())
    assert torch.equal(quiet.bias * 1024.0, loud.bias) and torch.equal(quiet.w[0].view(torch.int16), loud.w[0].view(torch.int16))
    assert torch.equal(quiet.conv() * 1024.0, loud.conv())
    var = 1.0 / quiet.ref.rstd[quiet.pos[:128] >= 0] ** 2
    assert 1e-9 < float(var.min()) and float(var.max()) < 1e-6                            # far above 1e-12, far below 1e-5
    assert float((quiet.ceiling - loud.ceiling).abs().max()) < 1e-3 * float(loud.ceiling.max())
    # dead_window: the rows whose whole window is zero
    for form in ("mid", "head"):
        o = _pred_ops((form, 256, 3, 128, "dead_window"))
        assert o.dead == [41, 42, 43] and bool((o.pos[38:48] >= 0).all()) and float(o.xv[40:45].abs().max()) == 0.0 and float(o.xv[39].abs().min()) > 0.0
        y = o.conv()
        assert float(y[o.dead].max()) <= -0.5 and bool((o.ref.rstd[o.dead] == 1e6).all()) and float(o.ref.yhat[o.dead].abs().max()) == 0.0
        assert torch.equal(o.ref.v[o.dead], o.beta.double().unsqueeze(0).expand(3, -1))
        ordinary = (y.max(1).values > 0.0) & (o.pos[:128] >= 0)                            # (most other rows keep some outputs behind the ReLU)
        assert int(ordinary.sum()) > 100 and not bool(ordinary[o.dead].any()) and bool(torch.isfinite(o.ref.v).all())
    o = _pred_ops(("two_ln", 256, 3, 333, "hi_only"))
    assert not bool(o.x[1].view(torch.int16).any()) and not bool(o.w[1].view(torch.int16).any()) and G.pred_precision("hi_only") == "bf16"


@pytest.mark.parametrize("case", G.PRED_CASES, ids=G.PRED_IDS)
def test_pred_fp32_statement_stays_below_an_eighth_of_the_bar(case):
    """The kernels' arithmetic stated in fp32 on the CPU (the figure the shares are 8 x the worst of), case by case."""
    from tests.test_gpu_ops import GEMM_TOL
    assert G.PRED_TOL == GEMM_TOL["bf16x3"] and G.PRED_BAR_SHARE == min(1.0, 8 * G.PRED_FP32_RATIO[0]) and G.PRED_HEAD_SHARE == min(1.0, 8 * G.PRED_FP32_RATIO[1])
    o = _pred_ops(case)
    v, head = G.pred_fp32(o)
    bar_v, bar_h = o.bars()
    rv = float(((v - o.ref.v).abs() / o.ceiling).max())
    rh = float(((head - o.ref.head).abs() / o.head_ceiling).max()) if o.has_head else 0.0
    print("%s: fp32 statement / ceiling: planes %.4g, heads %.4g" % (case, rv, rh))
    assert bool(torch.isfinite(v).all()) and float(o.ceiling.min()) >= G.PRED_TOL
    assert bool(((v - o.ref.v).abs() <= bar_v / 8).all()), rv
    if o.has_head:
        assert bool(((head - o.ref.head).abs() <= bar_h / 8).all()), rh
    for r in o.dead:                                                                       # exactly beta, as the planes round it
        assert torch.equal(v[r], G.pair_value(*G.split_bf16(o.beta)))


@pytest.mark.parametrize("case", G.PRED_CASES, ids=G.PRED_IDS)
def test_pred_reference_tells_every_mutant_apart(case):
    """Taps reversed, the halo tap behind a tile edge missing, the tap in front of row 0 reading a row, groups crossed, one LayerNorm over all columns, eps = 1e-5
    (quiet variant), no ReLU, ReLU per split-K partial, dot_b[0] for dot_b[g], the heads swapped: each at 8 bars or more on some element of the rows it concerns."""
    o = _pred_ops(case)
    form, _, _, R, variant = case
    want = {"taps_reversed", "row0_front", "no_relu", "relu_per_partial"} | ({"edge_plus_tap"} if R == 333 else set()) | ({"eps_1e-5"} if variant == "quiet" else set())
    want |= ({"one_ln"} if form in ("two_ln", "grouped") else set()) | ({"groups_crossed", "head_bias0", "head_swapped"} if form == "grouped" else set())
    assert set(o.mutants()) == want and o.ksplit() > 1
    worst = {}
    for m in o.mutants():
        r, rows = o.mutant(m)
        assert rows is None or (len(rows) > 0 and all(0 <= q < R and int(o.pos[q]) >= 0 for q in rows)), (m, rows)
        assert {"row0_front": list(range(o.P)), "edge_plus_tap": [127, 191, 255]}.get(m) == rows
        worst[m] = o.distance(r, rows)
    print(case, {m: "%.3g" % d for m, d in worst.items()})
    assert min(worst.values()) >= 8.0, worst
    assert o.distance(o.ref) == 0.0


def test_pred_half_blocks_are_refused_without_the_row_kernel_and_every_family_is_reached(probe, tmp_path):
    fs2_h = open(os.path.join(ROOT, "include", "fs2.h")).read()
    assert "#define FS2_ERR_UNSUPPORTED (-6)" in fs2_h and "#define FS2_PREC_BF16X3 1 " in fs2_h and "#define FS2_PREC_BF16 2 " in fs2_h
    assert G.PLAN_ERR_UNSUPPORTED == -6 and G.PREC_CODE == {"bf16x3": 1, "bf16": 2}
    p = collections.defaultdict(lambda: 0x1000)
    refused = [("%s-R%d-split%d" % (h, R, s), {"FS2_ROW8": 0}, G.pred_block(h, 256, 3, R, p, split=bool(s)), {}) for h in ("half0", "half1") for R in (333, 128) for s in (0, 1)]
    got = _plans(probe, tmp_path, refused)
    assert len(got) == 8 and all(g["err"] == G.PLAN_ERR_UNSUPPORTED and g["kernel"] == "none" for g in got.values()), got
    launches = G.pred_launches(p)
    got = _plans(probe, tmp_path, launches)
    assert all(g["err"] == 0 for g in got.values())
    reached = {(g["kernel"], g["nsplit"], g["nb"], g["mt"]) for g in got.values()}
    assert {("row8c", 3, nb, mt) for nb in (2, 3) for mt in (2, 3)} | {("row8c_grouped", 3, nb, mt) for nb in (2, 3) for mt in (2, 3)} <= reached
    assert {("row8c_two_ln", 3, 4, 2), ("row8c_two_ln", 1, 4, 2), ("row8c", 1, 2, 2), ("row8c", 1, 2, 3), ("row8c_grouped", 1, 2, 3)} <= reached
    sib = [g for n, g in got.items() if "-sib" in n]
    assert all(g["kernel"] == "pl_bf16" and g["bm"] == 64 and g["rows_pass"] == 1 for g in sib)
    assert all((g["ksplit"] > 1) == ("-sibk-" in n) for n, g in got.items()) and {g["ksplit"] for g in sib} == {1, 4}
    # a block differs from its sibling's in nothing but the switches; from its split-K form in the three fields call_defaults sets
    for form in ("mid", "head", "two_ln", "grouped"):
        a, b = G.pred_block(form, 256, 3, 333, p), G.pred_block(form, 256, 3, 333, p, split=True)
        diff = {f for f, _ in G.GemmArgs._fields_ if getattr(a, f) != getattr(b, f)}
        assert diff == {"kpart", "kpart_cap", "ksplit"} and a.relu_pre == 1 and a.x_scale == 1.0 and abs(a.ln_eps - 1e-12) < 1e-19 and not a.Y and a.scratch and a.Xp
