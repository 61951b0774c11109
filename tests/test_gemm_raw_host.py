"""CPU checks of tests/gemm_raw.py, the helper of the kernel-level GEMM tests (tests/test_gpu_row_kernels.py): all of them must pass before a block
is sent to a GPU.

(a) the ctypes mirror of fs2::GemmArgs against csrc/gemm_args.h as the host compiler lays it out (tests/gemm_raw_probe.cpp), and the kernel names
    against the enumerators of GemmKernel;
(b) the operand encoders / decoders: exact round trips, the in-chunk position a bijection and equal to csrc/common.h's plane_byte written out again
    byte by byte, the pair values equal to bf16 / fp16 / e4m3 arithmetic stated independently;
(c) the float64 reference against a plain F.linear + F.layer_norm fp32 statement;
(d) the plan of every argument block the GPU tests send, from csrc/gemm_plan.h compiled for the host on the block's own bytes: the expected kernel,
    epilogue, residual form and tile height, and no refusal."""
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


def test_every_block_the_gpu_tests_send_plans_onto_the_expected_kernel(probe, tmp_path):
    launches = G.all_launches()
    assert len(launches) == 4 * len(G.LN_CASES) + sum(len(r) for r in G.QKV_RUNS.values()) and len({l[0] for l in launches}) == len(launches)
    path = tmp_path / "blocks.txt"
    with open(path, "w") as f:
        for name, opts, block, _ in launches:
            f.write("%s 1 %s %s\n" % (name, ",".join("%s=%d" % kv for kv in sorted(opts.items())), bytes(block).hex()))
    fields = ("kernel",) + G.Plan._fields[1:] + ("err",)
    got = {l[0]: dict(zip(fields, [l[1]] + [int(v) for v in l[2:]])) for l in probe("plans", path)}
    assert sorted(got) == sorted(l[0] for l in launches)
    for name, _, _, want in launches:
        assert got[name]["err"] == 0, (name, got[name])
        assert {k: got[name][k] for k in want} == want, (name, got[name])
        assert got[name]["nsplit"] == 3 and got[name]["ksplit"] == 1 and not got[name]["rows_pass"] and not got[name]["build_planes"], (name, got[name])
    # every instantiation family the issue names is reached: both heights of the four row4 forms, the QKV passes on it, gemm_qkv8_bf16 whole and apart
    reached = {(g["kernel"], g["epi"], g["res"], g["mt"], g["apart"]) for g in got.values()}
    for epi, res in ((0, 1), (0, 2), (1, 1), (2, 3)):
        assert {("row4", epi, res, 4, 0), ("row4", epi, res, 5, 0)} <= reached
    assert {("qkv4", 3, 0, 4, 0), ("qkv4", 3, 0, 5, 0)} | {("qkv8", -1, 0, m, s) for m in (2, 3) for s in (0, 1)} | {("row8", -1, 0, 2, 0), ("row8", -1, 0, 3, 0)} <= reached
