"""Test-side access to single GEMM launches of libfs2_hip through fs2_op_launch_gemm (include/fs2.h): the argument-block mirror, the operand
encoders / decoders, the launches the kernel-level tests send, and the float64 reference.

Nothing here trusts a converter of the library: operands are PAIRS the kernels read as they are -- a bf16 hi and a bf16 lo (|lo| <= 2^-8 |hi|), or an
fp16 value and a finite e4m3 byte -- so the value a kernel sees is known exactly (hi + lo, fp16 + e4m3 2^-(ka+11)) and the float64 reference carries no
conversion error.  A wrong mirror of the in-chunk channel position cannot make a test pass: A and W only need the same order for the GEMM to be right,
but the residual and the outputs would come out permuted.

CPU-only parts (tests/test_gemm_raw_host.py): the mirror against the compiled header, the encoders, the reference, and the plan of every block of
`all_launches()` -- built there with placeholder pointers, which plan_gemm never follows.  GPU parts (tests/test_gpu_row_kernels.py): `LnCase` / `QkvCase`."""
import collections
import ctypes as C

import numpy as np
import torch

N_OUT = 384                    # the decoder width: the only N gemm_row4_bf16 is built for
Q_SCALE = float(np.float32(0.104))
KA_RES = 3                     # static scale 2^ka of mx residual planes (|x| < 1 here; the model's comes from the LayerNorm bound)
KA_OUT = 3                     # ... of mx planes a launch writes: yp_scale = 8
GUARD = 4096                   # sentinel bytes behind every output buffer

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t


class GemmArgs(C.Structure):
    """fs2::GemmArgs (fastspeech2_amd/csrc/gemm_args.h), field for field."""
    _fields_ = [("X", _vp), ("ldx", _i), ("C", _i), ("W", _vp), ("Cpad", _i), ("ktaps", _i), ("N", _i), ("R", _i), ("row_pos", _vp), ("bias", _vp),
                ("resid", _vp), ("ldr", _i), ("relu_pre", _i), ("ln_g", _vp), ("ln_b", _vp), ("ln_eps", _f), ("act_post", _i),
                ("pe", _vp), ("pe_ld", _i), ("pe_alpha", _vp), ("x_scale", _f), ("dot_w", _vp), ("dot_b", _vp), ("dot_out", _vp),
                ("Y", _vp), ("ldy", _i), ("Ysrc", _vp), ("ldsrc", _i), ("Wb", _vp),
                ("qk_hi", _vp), ("qk_lo", _vp), ("vt_hi", _vp), ("vt_lo", _vp), ("att_D", _i), ("Rvt", _i), ("q_scale", _f), ("scratch", _vp),
                ("Xp", _vp), ("xp_scratch", _vp), ("Yp", _vp), ("yp_chunks", _i), ("yp_f16", _i), ("f16_terms", _i),
                ("yp_scale", _f), ("mx", _i), ("mx_scale", _i), ("mx_scale_b", _i),
                ("ksplit", _i), ("kpart", _vp), ("kpart_stride", _sz), ("kpart_cap", _sz), ("regime_rows", _i),
                ("xp_row_chunks", _i), ("k_groups", _i), ("ln_groups", _i), ("dot_gstride", _i), ("yp_col_off", _i), ("Rp", _vp),
                ("residp", _vp), ("residp_chunks", _i), ("residp_mx", _i), ("residp_scale", _f),
                ("yp_rowscale", _vp), ("x_rowscale", _vp), ("w_rowscale", _vp)]


# GemmKernel (csrc/gemm_plan.h) in enumerator order: plan_out[0] of fs2_op_launch_gemm indexes this list (checked against the compiled header on the CPU)
KERNELS = ["none", "rows_f32", "tile_f32", "tile_rows_f32", "pl_bf16", "pl_f16", "pl_mx", "pl_mx4", "row8", "row8c", "row8c_grouped", "row8c_two_ln",
           "row4", "qkv8", "qkv4"]
Plan = collections.namedtuple("Plan", "kernel nsplit nb bm mt apart epi arith res ksplit rows_pass build_planes")


def rpad(R):
    """Rows of every row-indexed buffer: whole tiles of every height (128, 160, 192) behind the last row."""
    return (R + 191) // 192 * 192 + 192


# ------------------------------------------------------------------ encoders / decoders (CPU)
def chunk_pos(c):
    """Position (in bf16 elements) of channel c & 31 inside the hi half of its 32-channel chunk (csrc/common.h: plane_byte; gemm_bf16.h: kperm)."""
    c &= 31
    return ((c & 15) >> 2) * 8 + ((c >> 4) & 1) * 4 + (c & 3)


_POS = torch.tensor([chunk_pos(c) for c in range(32)])


def split_bf16(x):
    """fp32 -> (hi, lo) bf16 with hi + lo exact in fp32."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi, lo


def encode_planes(hi, lo):
    """(hi, lo) bf16 [rows, C] -> the plane / weight image [rows, C / 32 * 64] bf16: per 32-channel chunk [hi 32 | lo 32]."""
    rows, Cc = hi.shape
    out = torch.empty(rows, Cc // 32, 64, dtype=torch.bfloat16)
    out[:, :, _POS] = hi.reshape(rows, Cc // 32, 32)
    out[:, :, 32 + _POS] = lo.reshape(rows, Cc // 32, 32)
    return out.reshape(rows, Cc // 32 * 64)


def decode_planes(buf, rows, Cc):
    """Bytes of split-bf16 planes -> (hi, lo) bf16 [rows, C]."""
    b = buf.contiguous().view(torch.uint8).reshape(-1)[:rows * Cc * 4].view(torch.bfloat16).reshape(rows, Cc // 32, 64)
    return b[:, :, _POS].reshape(rows, Cc), b[:, :, 32 + _POS].reshape(rows, Cc)


def pair_value(hi, lo):
    return hi.double() + lo.double()


def split_mx(x, ka):
    """fp32 -> (fp16, e4m3 byte of the residual x 2^(ka+11))."""
    h = x.half()
    e8 = ((x - h.float()) * 2.0 ** (ka + 11)).to(torch.float8_e4m3fn).view(torch.uint8)
    assert not bool(((e8 & 0x7F) == 0x7F).any()), "a non-finite e4m3 byte"
    return h, e8


def e4m3_of(v):
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


def encode_mx(h, e8, ka):
    """(fp16, e4m3 residual byte) [rows, C] -> mx planes, a row of 4 C bytes: fp16 at 2 c | residual at 2 C + c | e4m3(fp16 2^ka) at 3 C + c."""
    rows, Cc = h.shape
    out = torch.empty(rows, 4 * Cc, dtype=torch.uint8)
    out[:, :2 * Cc] = h.contiguous().view(torch.uint8)
    out[:, 2 * Cc:3 * Cc] = e8
    out[:, 3 * Cc:] = e4m3_of(h.float() * 2.0 ** ka)
    return out


def decode_mx(buf, rows, Cc):
    """Bytes of mx planes -> (fp16, residual byte, ah8 byte) [rows, C]."""
    b = buf.contiguous().view(torch.uint8).reshape(-1)[:rows * Cc * 4].reshape(rows, 4 * Cc)
    return b[:, :2 * Cc].contiguous().view(torch.float16), b[:, 2 * Cc:3 * Cc].contiguous(), b[:, 3 * Cc:].contiguous()


def mx_value(h, e8, ka):
    return h.double() + e8.contiguous().view(torch.float8_e4m3fn).float().double() * 2.0 ** -(ka + 11)


# ------------------------------------------------------------------ float64 reference
def ref_rows(x, w, bias, resid, gamma, beta, pos, relu=False, x_scale=1.0, pe=None, alpha=1.0, eps=1e-5):
    """LayerNorm(x w^T + bias + resid) -> optional ReLU -> x_scale v + alpha pe[pos]; rows with pos < 0 are zeros.  Everything float64; pos [rows]."""
    y = x @ w.t() + bias
    if resid is not None:
        y = y + resid
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    v = (y - mu) / torch.sqrt(var + eps) * gamma + beta
    if relu:
        v = v.clamp(min=0.0)
    if pe is not None:
        v = x_scale * v + alpha * pe[pos.clamp(min=0).long()]
    return v * (pos >= 0).unsqueeze(1)


def ref_qkv(x, w, bias, pos, D, q_scale):
    """(Q q_scale, K, V) of x w^T + bias, rows with pos < 0 zero.  float64."""
    y = (x @ w.t() + bias) * (pos >= 0).unsqueeze(1)
    return y[:, :D] * q_scale, y[:, D:2 * D], y[:, 2 * D:]


# ------------------------------------------------------------------ the launches
# the LayerNorm-fused forms gemm_row4_bf16 has (csrc/gemm_row4.h: EPI / RES); gemm_row8_bf16 runs the same launch with fp32 rows in and out
LN_FORMS = collections.OrderedDict([
    ("epi0_res1", dict(epi=0, res=1)),      # residual from split-bf16 planes, split-bf16 planes out
    ("epi0_res2", dict(epi=0, res=2)),      # residual from mx planes
    ("epi1_res1", dict(epi=1, res=1)),      # mx planes out
    ("epi2_res3", dict(epi=2, res=3)),      # decoder input layer: no residual, ReLU, x_scale, positional encoding
])
LN_RUNS = [("row8", 2), ("row8", 3), ("row4", 4), ("row4", 5)]
# (form, R, C): 333 rows = several tiles of every height with a ragged last one; 128 = exactly one tile of 128 rows, a partial one of 160
LN_CASES = [(f, 333, 384) for f in LN_FORMS] + [("epi0_res1", 333, 1024)] + [(f, 128, 384) for f in LN_FORMS]
QKV_RUNS = {384: [("qkv8", 2, 0), ("qkv8", 2, 1), ("qkv8", 3, 0), ("qkv8", 3, 1), ("qkv4", 4, 0), ("qkv4", 5, 0), ("pl", 0, 0)],
            256: [("qkv8", 2, 0), ("qkv8", 2, 1), ("qkv8", 3, 0), ("qkv8", 3, 1), ("pl", 0, 0)]}
QKV_R = 333


def ln_options(side, mt):
    o = {"FS2_ROW8": 1, "FS2_QKV8": 1, "FS2_ROW4": 1 if side == "row4" else 0}
    o["FS2_MT4" if side == "row4" else "FS2_MT8"] = mt
    return o


def ln_expected(form, side, mt):
    """(kernel, epi, res, mt) of the plan."""
    f = LN_FORMS[form]
    return ("row4", f["epi"], f["res"], mt) if side == "row4" else ("row8", -1, 0, mt)


def ln_block(form, R, Cc, side, p):
    """The argument block of one LayerNorm-fused launch; p: name -> pointer (int)."""
    f = LN_FORMS[form]
    a = GemmArgs()
    a.C = a.Cpad = Cc
    a.ktaps, a.N, a.R = 1, N_OUT, R
    a.W = a.Wb = p["w"]
    a.Xp, a.row_pos, a.bias = p["x"], p["pos"], p["bias"]
    a.ldr, a.ldy = N_OUT, N_OUT
    a.ln_g, a.ln_b, a.ln_eps = p["gamma"], p["beta"], 1e-5
    a.Yp, a.yp_chunks, a.x_scale = p["yp"], N_OUT // 32, 1.0
    if f["epi"] == 1:
        a.yp_f16, a.yp_scale = 2, 2.0 ** KA_OUT
    if f["epi"] == 2:
        a.act_post, a.pe, a.pe_ld, a.pe_alpha, a.x_scale = 1, p["pe"], N_OUT, p["alpha"], 1.25
    if side == "row8":          # fp32 rows in and out (the residual reconstructed from the planes: exact in fp32)
        a.Y = p["y"]
        if f["res"] != 3:
            a.resid = p["resid32"]
    elif f["res"] != 3:         # planes only
        a.residp, a.residp_chunks = p["residp"], N_OUT // 32
        a.residp_mx, a.residp_scale = (1, 2.0 ** -(KA_RES + 11)) if f["res"] == 2 else (0, 1.0)
    return a


def qkv_options(kind, mt, split):
    if kind == "pl":
        return {"FS2_ROW8": 1, "FS2_QKV8": 0}
    if kind == "qkv4":
        return {"FS2_ROW8": 1, "FS2_QKV8": 1, "FS2_ROW4": 1, "FS2_QKV4": 1, "FS2_MT4": mt}
    return {"FS2_ROW8": 1, "FS2_QKV8": 1, "FS2_QKV4": 0, "FS2_MT8": mt, "FS2_QKV_SPLIT": split}


def qkv_expected(kind, mt, split):
    """(kernel, epi, res, mt, apart, bm)."""
    return {"pl": ("pl_bf16", -1, 0, 0, 0, 64), "qkv4": ("qkv4", 3, 0, mt, 0, 0), "qkv8": ("qkv8", -1, 0, mt, split, 0)}[kind]


def qkv_block(D, R, p):
    a = GemmArgs()
    a.C = a.Cpad = D
    a.ktaps, a.N, a.R = 1, 3 * D, R
    a.W = a.Wb = p["w"]
    a.Xp, a.row_pos, a.bias = p["x"], p["pos"], p["bias"]
    a.qk_hi, a.qk_lo, a.vt_hi, a.vt_lo = p["qk_hi"], p["qk_lo"], p["vt_hi"], p["vt_lo"]
    a.att_D, a.Rvt, a.q_scale, a.x_scale = D, rpad(R), Q_SCALE, 1.0
    return a


def all_launches(p=None):
    """[(id, switches, block, expected plan fields)] of every launch the GPU tests send; p: pointers (default: placeholders)."""
    p = p if p is not None else collections.defaultdict(lambda: 0x1000)
    out = []
    for form, R, Cc in LN_CASES:
        for side, mt in LN_RUNS:
            out.append(("%s-R%d-C%d-%s-mt%d" % (form, R, Cc, side, mt), ln_options(side, mt), ln_block(form, R, Cc, side, p),
                        dict(zip(("kernel", "epi", "res", "mt"), ln_expected(form, side, mt)))))
    for D, runs in QKV_RUNS.items():
        for kind, mt, split in runs:
            out.append(("qkv-D%d-%s-mt%d-split%d" % (D, kind, mt, split), qkv_options(kind, mt, split), qkv_block(D, QKV_R, p),
                        dict(zip(("kernel", "epi", "res", "mt", "apart", "bm"), qkv_expected(kind, mt, split)))))
    return out


# ------------------------------------------------------------------ operands
def _uni(rs, *shape, scale=1.0):
    return torch.from_numpy(rs.uniform(-scale, scale, size=shape).astype(np.float32))


def row_positions(R):
    """The probe's pattern: 4 gap rows in front of every 105-row "utterance"; rows >= R are gaps too."""
    r = torch.arange(rpad(R))
    return torch.where((r % 109 < 4) | (r >= R), torch.full_like(r, -1), r % 109 - 4).int()


def _exact_f32(v):
    assert bool((v.float().double() == v).all()), "an operand pair whose sum is not an fp32 value"
    return v.float()


class LnOperands:
    """Operands of one LayerNorm-fused case on the CPU (the distributions of test_conv_gemm), the exact values the kernels see, and the float64 result."""

    def __init__(self, form, R, Cc):
        f = LN_FORMS[form]
        self.form, self.R, self.C, self.epi, self.res = form, R, Cc, f["epi"], f["res"]
        rs = np.random.RandomState(1000 * f["epi"] + 100 * f["res"] + R + Cc)
        Rp = rpad(R)
        self.x = split_bf16(_uni(rs, Rp, Cc))
        self.w = split_bf16(_uni(rs, N_OUT, Cc, scale=1.0 / np.sqrt(Cc)))
        self.bias, self.gamma, self.beta = _uni(rs, N_OUT, scale=0.5), 1.0 + _uni(rs, N_OUT, scale=0.2), _uni(rs, N_OUT, scale=0.2)
        self.pos = row_positions(R)
        self.pe, self.alpha = _uni(rs, 128, N_OUT), torch.tensor([0.9], dtype=torch.float32)
        r = _uni(rs, Rp, N_OUT)
        self.resid_planes = self.resid_value = None
        if self.res == 1:
            hi, lo = split_bf16(r)
            self.resid_planes, self.resid_value = encode_planes(hi, lo), pair_value(hi, lo)
        elif self.res == 2:
            h, e8 = split_mx(r, KA_RES)
            self.resid_planes, self.resid_value = encode_mx(h, e8, KA_RES), mx_value(h, e8, KA_RES)
        pe = self.epi == 2
        self.ref = ref_rows(pair_value(*self.x)[:R], pair_value(*self.w), self.bias.double(), None if self.resid_value is None else self.resid_value[:R],
                            self.gamma.double(), self.beta.double(), self.pos[:R], relu=pe, x_scale=1.25 if pe else 1.0, pe=self.pe.double() if pe else None,
                            alpha=float(self.alpha[0]) if pe else 1.0)

    def decode(self, yp_bytes):
        """Output planes -> float64 [R, N] (and, for mx planes, the three decoded blocks)."""
        if self.epi == 1:
            h, e8, a8 = decode_mx(yp_bytes, self.R, N_OUT)
            return mx_value(h, e8, KA_OUT), (h, e8, a8)
        return pair_value(*decode_planes(yp_bytes, self.R, N_OUT)), None


class QkvOperands:
    def __init__(self, D, R=QKV_R):
        self.D, self.R = D, R
        rs = np.random.RandomState(7 * D + R)
        self.x = split_bf16(_uni(rs, rpad(R), D))
        self.w = split_bf16(_uni(rs, 3 * D, D, scale=1.0 / np.sqrt(D)))
        self.bias = _uni(rs, 3 * D, scale=0.5)
        self.pos = row_positions(R)
        self.ref = ref_qkv(pair_value(*self.x)[:R], pair_value(*self.w), self.bias.double(), self.pos[:R], D, Q_SCALE)


# ------------------------------------------------------------------ device side
def _dev():
    return torch.device("cuda:0")


def sentinel(nbytes):
    """An output buffer of nbytes + GUARD bytes of 0xFF (NaN in bf16, fp16 and fp32)."""
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())


def untouched(buf, start):
    """Every byte of buf from `start` on still holds the sentinel."""
    return bool((buf[start:] == 0xFF).all())


def launch(block, precision="bf16x3"):
    """fs2_op_launch_gemm on the current stream; returns the plan it ran."""
    from fastspeech2_amd import _lib
    L = _lib.lib()
    plan = (C.c_int32 * _lib.GEMM_PLAN_FIELDS)()
    with torch.cuda.device(_dev()):
        _lib.check(L.fs2_op_launch_gemm(C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream), C.byref(block), C.sizeof(block),
                                        _lib.PRECISIONS[precision], plan, _lib.GEMM_PLAN_FIELDS))
    torch.cuda.synchronize()
    v = list(plan)
    return Plan(KERNELS[v[0]], *v[1:])


class LnCase:
    """One LayerNorm-fused case on the GPU: the operands uploaded once, one run per (kernel, tile height) into fresh sentinel buffers."""

    def __init__(self, ops):
        self.ops = ops
        d = _dev()
        Rp = rpad(ops.R)
        self.keep = dict(x=encode_planes(*ops.x).to(d), w=encode_planes(*ops.w).to(d), pos=ops.pos.to(d), bias=ops.bias.to(d), gamma=ops.gamma.to(d),
                         beta=ops.beta.to(d), pe=ops.pe.to(d), alpha=ops.alpha.to(d))
        if ops.resid_planes is not None:
            self.keep["residp"] = ops.resid_planes.to(d)
            self.keep["resid32"] = _exact_f32(ops.resid_value).to(d)
        self.out_bytes = Rp * N_OUT * 4           # fp32 rows, split-bf16 planes and mx planes all take 4 bytes per element

    def run(self, side, mt, set_option):
        """-> (plan, yp bytes (CPU, with guard), y fp32 rows bytes or None)."""
        for k, v in ln_options(side, mt).items():
            set_option(k, v)
        yp, y = sentinel(self.out_bytes), sentinel(self.out_bytes)
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p.update(yp=yp.data_ptr(), y=y.data_ptr())
        a = ln_block(self.ops.form, self.ops.R, self.ops.C, side, p)
        plan = launch(a)
        return plan, yp.cpu(), y.cpu()


class QkvCase:
    def __init__(self, ops):
        self.ops = ops
        d = _dev()
        self.keep = dict(x=encode_planes(*ops.x).to(d), w=encode_planes(*ops.w).to(d), pos=ops.pos.to(d), bias=ops.bias.to(d))
        self.Rvt = rpad(ops.R)
        self.qk_bytes, self.vt_bytes = self.Rvt * 2 * ops.D * 2, ops.D * self.Rvt * 2

    def run(self, kind, mt, split, set_option):
        """-> (plan, {qk_hi, qk_lo, vt_hi, vt_lo: bytes on the CPU, with guard})."""
        for k, v in qkv_options(kind, mt, split).items():
            set_option(k, v)
        out = dict(qk_hi=sentinel(self.qk_bytes), qk_lo=sentinel(self.qk_bytes), vt_hi=sentinel(self.vt_bytes), vt_lo=sentinel(self.vt_bytes))
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p.update({k: t.data_ptr() for k, t in out.items()})
        plan = launch(qkv_block(self.ops.D, self.ops.R, p))
        return plan, {k: t.cpu() for k, t in out.items()}

    def decode(self, out):
        """-> (Q, K, V) float64 [Rvt, D] as hi + lo."""
        D, Rvt = self.ops.D, self.Rvt
        bf = lambda k, n: out[k][:n].view(torch.bfloat16)
        qk = pair_value(bf("qk_hi", self.qk_bytes), bf("qk_lo", self.qk_bytes)).reshape(Rvt, 2 * D)
        vt = pair_value(bf("vt_hi", self.vt_bytes), bf("vt_lo", self.vt_bytes)).reshape(D, Rvt)
        return qk[:, :D], qk[:, D:], vt.t()


def canon_zero16(b):
    """Bytes as 16-bit words with -0 turned into +0 (rows that are padding leave the QKV kernels as v x 0 = +-0 with the sign of a value nobody defined)."""
    w = b.contiguous().view(torch.int16).clone()
    w[(w & 0x7FFF) == 0] = 0
    return w
