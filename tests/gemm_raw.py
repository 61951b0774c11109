"""Test-side access to single GEMM launches of libfs2_hip through fs2_op_launch_gemm (include/fs2.h): the argument-block mirror, the operand
encoders / decoders, the launches the kernel-level tests send, and the float64 reference.

Nothing here trusts a converter of the library: operands are PAIRS the kernels read as they are -- a bf16 hi and a bf16 lo (|lo| <= 2^-8 |hi|), or an
fp16 value and a finite e4m3 byte -- so the value a kernel sees is known exactly (hi + lo, fp16 + e4m3 2^-(ka+11)) and the float64 reference carries no
conversion error.  A wrong mirror of the in-chunk channel position cannot make a test pass: A and W only need the same order for the GEMM to be right,
but the residual and the outputs would come out permuted.

The mixed modes' formats (mx: fp16 + two e4m3 copies under static scales; mx4: fp16 + two e2m1 copies under one E8M0 byte per 16-channel slot) are stated here
once, as TUPLES per element with encoders that put them where the kernels read them, and the float64 references of those launches state each kernel's own
formula on the tuples, with the mutants a broken position rule would compute.

CPU-only parts (tests/test_gemm_raw_host.py): the mirror against the compiled header, the encoders, the references, the mutants, and the plan of every block of
`all_launches()` -- built there with placeholder pointers, which plan_gemm never follows.  GPU parts: `LnCase` / `QkvCase` (tests/test_gpu_row_kernels.py),
`ConvCase` / `Ffn2Case` / `repack_weight` (tests/test_gpu_mx_kernels.py), `PredCase` (tests/test_gpu_pred_kernels.py).

The LayerNorm-terminated convolutions of the variance predictors (`PRED_CASES`) have their conv weight image (`encode_w_conv`), a row pattern in which row 0 and every
tile edge are live, their float64 reference (`ref_pred`), the kernels' arithmetic stated in fp32 (`pred_fp32`, from which alone the bars are set) and their mutants here."""
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
PREC_CODE = {"bf16x3": 1, "bf16": 2}      # FS2_PREC_BF16X3 / FS2_PREC_BF16 (include/fs2.h): what the plan is asked under
PLAN_ERR_UNSUPPORTED = -6                 # FS2_ERR_UNSUPPORTED = kPlanErrUnsupported


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


def encode_w_conv(hi, lo):
    """(hi, lo) bf16 [N, C, k] -> the split-bf16 conv weight image [N, C / 32, k, 64] bf16: per (output row, 32-channel chunk, tap) [hi 32 | lo 32], the k-step
    order chunk * k + tap of repack_weight_bf16 (csrc/gemm_bf16.h).  A grouped layer's image is its groups stacked along N, each over its own C."""
    N, Cc, k = hi.shape
    out = torch.empty(N, Cc // 32, k, 64, dtype=torch.bfloat16)
    out[:, :, :, _POS] = hi.reshape(N, Cc // 32, 32, k).permute(0, 1, 3, 2)
    out[:, :, :, 32 + _POS] = lo.reshape(N, Cc // 32, 32, k).permute(0, 1, 3, 2)
    return out


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


# ------------------------------------------------------------------ the mx / mx4 formats as exact tuples (CPU)
# THE statement of the formats on the CPU (csrc/gemm_mx.h, csrc/common.h: store_planes4_mx4, csrc/gemm_planes.h ARITH = 2 / 3, csrc/gemm_row4.h EPI 4): operands are
# the tuples the kernels read -- (fp16, e4m3 byte, e4m3 byte) per element in the mx arithmetic, (fp16, e2m1 nibble, e2m1 nibble) per element + one E8M0 byte per
# 16-channel slot in the mx4 arithmetic -- and the encoders below put those tuples at the byte positions the kernels read them from.
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
_E2M1_EDGE = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]          # the midpoint between code i and code i + 1


def e2m1_encode(x):
    """-> the 4-bit code (bit 3 = sign) of x: round to nearest, ties to the even code, saturating at +-6; the sign of a zero is kept."""
    x = x.double()
    mag = x.abs()
    code = torch.zeros(mag.shape, dtype=torch.uint8)
    for i, e in enumerate(_E2M1_EDGE):
        code += ((mag >= e) if (i & 1) else (mag > e)).to(torch.uint8)       # a tie goes to code i + 1 where that is the even one
    return code | (torch.signbit(x).to(torch.uint8) << 3)


def e2m1_decode(code):
    """the 16 codes -> float64."""
    return E2M1[(code & 7).long()] * (1.0 - 2.0 * (code >> 3).double())


def e4m3_value(b):
    return b.contiguous().view(torch.float8_e4m3fn).float().double()


def mx4_scale_byte(m):
    """csrc/common.h: mx4_scale_byte -- the E8M0 byte of a slot whose largest magnitude is the fp32 m: its exponent field - 2, clamped to [40, 200]."""
    bits = m.float().contiguous().view(torch.int32).long()
    return (((bits >> 23) & 0xFF) - 2).clamp(40, 200)


def mx4_inv_scale(eb):
    """csrc/common.h: mx4_inv_scale -- 2^(127 - byte), exact."""
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (127 - eb).double())


def pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def fp8_scale_exponent(bound):
    """csrc/fs2_runtime.hip: fp8_scale_exponent -- the largest k with bound 2^k <= 448."""
    return int(np.floor(np.log2(448.0 / float(bound)))) if bound > 0 else 0


def scale_byte4(e):
    """csrc/model_launches.h: scale_byte4 -- the E8M0 byte of 2^(e - 127) in all four bytes of the scaled MFMA's scale operand."""
    return min(max(int(e), 1), 254) * 0x01010101


def slot_pos(S):
    """Position of slot S = 8 u + s (slot s of cross unit u) in a row's 32-byte scale record: 8 u + 2 (s & 3) + (s >> 2) (csrc/gemm_row4.h, EPI 4)."""
    u, sl = S >> 3, S & 7
    return 8 * u + 2 * (sl & 3) + (sl >> 2)


Mx = collections.namedtuple("Mx", "h r8 a8")                   # mx activation / weight tuples: fp16, e4m3(residual 2^(k+11)), e4m3(fp16 2^k)
Mx4 = collections.namedtuple("Mx4", "h r4 h4 e8 sb")           # mx4: fp16, e2m1(residual 2^11 / s), e2m1(fp16 / s), e4m3(residual 2^(ka+11)) (activations), sb: byte of s per slot


def split_mx3(x, k):
    """fp32 [.., C] -> Mx under the static scale 2^k (the clamp to +-448 as the kernels apply it)."""
    h = x.half()
    r8 = e4m3_of(((x - h.float()) * 2.0 ** (k + 11)).clamp(-448.0, 448.0))
    a8 = e4m3_of((h.float() * 2.0 ** k).clamp(-448.0, 448.0))
    assert not bool(((r8 & 0x7F) == 0x7F).any() or ((a8 & 0x7F) == 0x7F).any()), "a non-finite e4m3 byte"
    return Mx(h, r8, a8)


def split_mx4(x, ka, slot_dim=-1):
    """fp32 -> Mx4: the scale byte of every 16-element slot along `slot_dim` by the OCP rule from the slot's largest |fp16 value| (csrc/gemm_mx.h: the weights;
    EPI 4 applies the rule to the fp32 values, which names another byte only where the rounding to fp16 crosses a binade), e2m1 of both parts under it."""
    x = x.movedim(slot_dim, -1)
    h = x.half()
    r = x - h.float()
    m = h.float().abs().reshape(x.shape[:-1] + (x.shape[-1] // 16, 16)).amax(-1)
    sb = mx4_scale_byte(m)
    inv = mx4_inv_scale(sb).repeat_interleave(16, dim=-1)
    h4, r4 = e2m1_encode(h.double() * inv), e2m1_encode(r.double() * 2048.0 * inv)
    e8 = e4m3_of((r * 2.0 ** (ka + 11)).clamp(-448.0, 448.0))
    back = lambda t: t.movedim(-1, slot_dim).contiguous()
    return Mx4(back(h), back(r4), back(h4), back(e8), back(sb))


def _nib(lo, hi):
    return lo | (hi << 4)


def _cross_bytes(first, second):
    """e2m1 codes [.., C] of the two terms -> the cross units' bytes [.., C]: per 4 channels (first first | first first | second second | second second), the
    lower channel of a pair in the low nibble."""
    f, g = first.reshape(first.shape[:-1] + (-1, 4)), second.reshape(second.shape[:-1] + (-1, 4))
    return torch.stack([_nib(f[..., 0], f[..., 1]), _nib(f[..., 2], f[..., 3]), _nib(g[..., 0], g[..., 1]), _nib(g[..., 2], g[..., 3])], dim=-1).reshape(first.shape)


def _uncross_bytes(b):
    q = b.reshape(b.shape[:-1] + (-1, 4))
    lo, hi = q & 0xF, q >> 4
    first = torch.stack([lo[..., 0], hi[..., 0], lo[..., 1], hi[..., 1]], dim=-1).reshape(b.shape)
    second = torch.stack([lo[..., 2], hi[..., 2], lo[..., 3], hi[..., 3]], dim=-1).reshape(b.shape)
    return first, second


def encode_mx3(t):
    """Mx [rows, C] -> mx planes [rows, 4 C] bytes: fp16 at 2 c | residual byte at 2 C + c | e4m3(fp16 2^ka) at 3 C + c."""
    rows, Cc = t.h.shape
    out = torch.empty(rows, 4 * Cc, dtype=torch.uint8)
    out[:, :2 * Cc] = t.h.contiguous().view(torch.uint8)
    out[:, 2 * Cc:3 * Cc] = t.r8
    out[:, 3 * Cc:] = t.a8
    return out


def encode_mx4(t, fill=0):
    """Mx4 [rows, C] (sb [rows, C / 16]) -> (mx4 planes [rows, 4 C] bytes: fp16 at 2 c | cross units at 2 C + c | e4m3 residual at 3 C + c,
    the scale record [rows, 32]: byte slot_pos(S) = sb - 11 (2^-11 of the residuals' pre-scale folded in); bytes no slot owns hold `fill`)."""
    rows, Cc = t.h.shape
    out = torch.empty(rows, 4 * Cc, dtype=torch.uint8)
    out[:, :2 * Cc] = t.h.contiguous().view(torch.uint8)
    out[:, 2 * Cc:3 * Cc] = _cross_bytes(t.r4, t.h4)
    out[:, 3 * Cc:] = t.e8
    rec = torch.full((rows, 32), fill, dtype=torch.uint8)
    rec[:, [slot_pos(S) for S in range(Cc // 16)]] = (t.sb - 11).to(torch.uint8)
    return out, rec


def decode_mx4(buf, rec, rows, Cc):
    """Bytes of mx4 planes and of their scale record -> Mx4 (sb: the byte of s itself, record + 11)."""
    b = buf.contiguous().view(torch.uint8).reshape(-1)[:rows * Cc * 4].reshape(rows, 4 * Cc)
    r4, h4 = _uncross_bytes(b[:, 2 * Cc:3 * Cc].contiguous())
    sb = rec.contiguous().view(torch.uint8).reshape(-1)[:rows * 32].reshape(rows, 32)[:, [slot_pos(S) for S in range(Cc // 16)]].long() + 11
    return Mx4(b[:, :2 * Cc].contiguous().view(torch.float16), r4, h4, b[:, 3 * Cc:].contiguous(), sb)


def image_w_mx(t):
    """Mx [N, C, k] -> the mx weight image [N][C / 32 units][tap][128 B]: C / 64 units of fp16 channels, C / 128 of wh8, C / 128 of rw8 (csrc/gemm_mx.h)."""
    N, Cc, k = t.h.shape
    units = lambda x, per: x.reshape(N, Cc // per, per, k).permute(0, 1, 3, 2).contiguous()
    main = units(t.h, 64).view(torch.uint8).reshape(N, Cc // 64, k, 128)
    return torch.cat([main, units(t.a8, 128), units(t.r8, 128)], dim=1).contiguous()


def image_w_mx4(t):
    """Mx4 [N, C, k] (sb [N, C / 16, k]) -> (the mx4 weight image [N][C / 64 + C / 128 units][tap][128 B]: wh4 where the planes hold ra4, rw4 where they hold ah4,
    its scale image [N / 128][cross unit][tap][g 0..3][n 0..127][2]: byte 0 = slot g, byte 1 = slot 4 + g of that weight row's cross unit)."""
    N, Cc, k = t.h.shape
    units = lambda x, per: x.reshape(N, Cc // per, per, k).permute(0, 1, 3, 2).contiguous()
    main = units(t.h, 64).view(torch.uint8).reshape(N, Cc // 64, k, 128)
    cross = _cross_bytes(units(t.h4, 128), units(t.r4, 128))
    sc = t.sb.to(torch.uint8).reshape(N // 128, 128, Cc // 128, 2, 4, k).permute(0, 2, 5, 4, 1, 3).contiguous()      # (tile, n, u, s >> 2, s & 3, tap) -> (tile, u, tap, g, n, half)
    return torch.cat([main, cross], dim=1).contiguous(), sc


def mx_cross_scale(ms_a, ms_b):
    """The factor of the cross terms of the mx arithmetic: the static E8M0 bytes of both sides (byte 0 of mx_scale / mx_scale_b)."""
    return 2.0 ** ((ms_a & 0xFF) - 127) * 2.0 ** ((ms_b & 0xFF) - 127)


def mx_terms(a, w, ms_a, ms_b):
    """The three operand pairs of the mx formula a.w ~ ah.wh + 2^.. (ra8.wh8 + ah8.rw8) as float64 (A parts [rows, C], W parts [N, C, k]): concatenated along the
    channels, one product of the concatenations is the formula."""
    f = mx_cross_scale(ms_a, ms_b)
    return (torch.cat([a.h.double(), e4m3_value(a.r8) * f, e4m3_value(a.a8) * f], dim=1),
            torch.cat([w.h.double(), e4m3_value(w.a8), e4m3_value(w.r8)], dim=1))


def mx4_terms(a, w):
    """... of the mx4 formula: Sum ah.wh + Sum_slot 2^(sa - 127) 2^(sw - 127) Sum_(c in slot) (ra4.wh4 + ah4.rw4); sa = the record's byte (a.sb - 11), sw = w.sb.
    The powers of two are exact in float64, so scaling the operands slot by slot states the same sum."""
    fa = pow2(a.sb - 11 - 127).repeat_interleave(16, dim=1)
    fw = pow2(w.sb - 127).repeat_interleave(16, dim=1)
    return (torch.cat([a.h.double(), e2m1_decode(a.r4) * fa, e2m1_decode(a.h4) * fa], dim=1),
            torch.cat([w.h.double(), e2m1_decode(w.h4) * fw, e2m1_decode(w.r4) * fw], dim=1))


def ref_conv(ta, tw, bias, pos, R, relu=True):
    """bias + Sum_tap A[row + tap - P] . W[:, :, tap] over the term concatenations (mx_terms / mx4_terms), rows outside [0, R) zeros, -> ReLU; rows with
    pos < 0 are zeros.  float64 [R, N]."""
    k = tw.shape[2]
    P = (k - 1) // 2
    pad = torch.zeros(P, ta.shape[1], dtype=torch.float64)
    x = torch.cat([pad, ta[:R], pad])
    y = bias.double().unsqueeze(0).expand(R, -1).clone()
    for tap in range(k):
        y += x[tap:tap + R] @ tw[:, :, tap].t()
    if relu:
        y = y.clamp(min=0.0)
    return y * (pos[:R] >= 0).unsqueeze(1)


# the mutants of the formulas: what a kernel that broke one position rule would compute (tests/test_gemm_raw_host.py holds every one of them at >= 8 bars from
# the formula on the coherent operands, so a bar that passes the kernel tells them apart)
def mutant_mx4(a, w, which):
    if which == "no_cross":
        z = torch.zeros_like(a.r4)
        return a._replace(r4=z, h4=z), w
    if which == "pair_swapped":            # the two scale bytes of a lane's pair: slots lg and 4 + lg of a cross unit
        return a._replace(sb=a.sb[:, [S ^ 4 for S in range(a.sb.shape[1])]]), w
    if which == "g_off_by_one":            # the weight scale image read at g + 1
        return a, w._replace(sb=w.sb[:, [(S & ~3) | ((S + 1) & 3) for S in range(w.sb.shape[1])]])
    if which == "nibbles_swapped":         # ra4 and ah4 nibble pairs of the planes
        return a._replace(r4=a.h4, h4=a.r4), w
    raise KeyError(which)


def mutant_mx(a, w, which):
    if which == "no_cross":
        z = torch.zeros_like(a.r8)
        return a._replace(r8=z, a8=z), w
    if which == "units_swapped":           # the ra8 and the ah8 units of the planes
        return a._replace(r8=a.a8, a8=a.r8), w
    raise KeyError(which)


MX4_MUTANTS = ("no_cross", "pair_swapped", "g_off_by_one", "nibbles_swapped")
MX_MUTANTS = ("no_cross", "units_swapped")

# The bars of tests/test_gpu_mx_kernels.py, kernel against the float64 value of its own formula: 5 x the worst max-abs measured on the MI355X, none above the
# ceiling GEMM_TOL["bf16x3"] = 1.5e-4 (tests/test_gpu_ops.py).  tests/test_gemm_raw_host.py holds every mutant of the formulas at 8 bars or more on the CPU.
#   conv_mx4  fp32 rows of the mx4 conv: measured 8.44e-6 (k = 9, coherent operands, max |y| 5.8)            -> 4.2e-5; the hand-off case runs the same launch
#   conv_mx   fp32 rows of the mx conv: measured 9.68e-6                                                     -> 4.8e-5
#   ffn2_mx   split-bf16 planes of FFN2 + LN2 in the mx arithmetic: measured 3.08e-5 (5 x = 1.54e-4)          -> the ceiling
#   epi4      the value of the mx4 planes: the bar of the mx-planes form (tests/test_gpu_row_kernels.py), the ceiling + 2^-14 |ref| (measured 6.33e-5 at |ref| <= 7.4)
# Outputs read back from mx planes carry the planes' rounding, 2^-14 |ref| per element, on top of the launch's bar.
MX_CEILING = 1.5e-4
MX_BAR = {"conv_mx4": 4.2e-5, "conv_mx": 4.8e-5, "ffn2_mx": MX_CEILING, "epi4": MX_CEILING}


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
    # out-proj + LN1 of mix_mx4: mx4 planes + the scale record out.  gemm_row4_bf16 only (gemm_row8_bf16 has no such output); gamma spread 80-fold across the
    # 16-channel slots (2 .. 1 / 40), so that the slots of a row take different scale bytes
    ("epi4_res1", dict(epi=4, res=1, row4_only=True, gamma_spread=80.0)),
])
LN_RUNS = [("row8", 2), ("row8", 3), ("row4", 4), ("row4", 5)]
# (form, R, C): 333 rows = several tiles of every height with a ragged last one; 128 = exactly one tile of 128 rows, a partial one of 160
_LN_BOTH = [f for f in LN_FORMS if not LN_FORMS[f].get("row4_only")]
LN_CASES = [(f, 333, 384) for f in _LN_BOTH] + [("epi0_res1", 333, 1024)] + [(f, 128, 384) for f in _LN_BOTH]
EPI4_CASES = [("epi4_res1", 333, 384), ("epi4_res1", 128, 384)]
ROW4_RUNS = [("row4", 4), ("row4", 5)]
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


def ln_block(form, R, Cc, side, p, rm=None):
    """The argument block of one LayerNorm-fused launch; p: name -> pointer (int); rm: the format of the residual planes of a RES 2 form (1 mx, 2 mx4)."""
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
    if f["epi"] == 4:
        a.yp_f16, a.yp_scale, a.yp_rowscale = 3, 2.0 ** KA_OUT, p["rowscale"]
    if f["epi"] == 2:
        a.act_post, a.pe, a.pe_ld, a.pe_alpha, a.x_scale = 1, p["pe"], N_OUT, p["alpha"], 1.25
    if side == "row8":          # fp32 rows in and out (the residual reconstructed from the planes: exact in fp32)
        a.Y = p["y"]
        if f["res"] != 3:
            a.resid = p["resid32"]
    elif f["res"] != 3:         # planes only
        a.residp, a.residp_chunks = p["residp"], N_OUT // 32
        a.residp_mx, a.residp_scale = (rm or 1, 2.0 ** -(KA_RES + 11)) if f["res"] == 2 else (0, 1.0)
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


# ---- the launches of the mixed modes (tests/test_gpu_mx_kernels.py).  The FFN conv runs at C = 384, the only width gemm_pl_bf16<.., ARITH = 3> is built for:
# (k, N, R): N = 256 reads the scale image of N tile 1, one case at N = 1024; R = 333 is two 256-row tiles with a ragged last one, 256 a single exact tile
CONV_C = 384
CONV_CASES = [(3, 256, 333), (9, 256, 333), (3, 256, 256), (9, 256, 256), (9, 1024, 333)]
CONV_ARITHS = ("mx4", "mx")
CONV_OUTS = ("yp", "y_yp")             # mx planes out only (the model's form) / fp32 rows as well
DISTS = ("model", "coherent")
# FFN2 + LN2 in the mx arithmetic (C, R, residp_mx): the residual from mx planes (1) or from mx4 planes (2: the e4m3 residual at byte 3 C)
FFN2_CASES = [(Cc, R, rm) for Cc in (256, 1024) for R in (333, 128) for rm in (1, 2)]


def conv_expected(arith):
    return dict(kernel="pl_mx4", arith=3, bm=256, ksplit=1, nsplit=1) if arith == "mx4" else dict(kernel="pl_mx", arith=2, ksplit=1, nsplit=1)


def conv_block(arith, k, N, R, out, p, ka=0, kw=0, kh=0):
    """The FFN conv (k taps, ReLU) on mx4 planes + row scales + the mx4 weight image with its scale image, or on mx planes + the mx weight image under the static
    scales 2^ka / 2^kw; mx planes out under 2^kh."""
    a = GemmArgs()
    a.C = a.Cpad = CONV_C
    a.ktaps, a.N, a.R = k, N, R
    a.W = a.Wb = p["w"]
    a.Xp, a.row_pos, a.bias = p["x"], p["pos"], p["bias"]
    a.ldy, a.ln_eps, a.x_scale, a.act_post = N, 1e-5, 1.0, 1
    a.Yp, a.yp_chunks, a.yp_f16, a.yp_scale = p["yp"], N // 32, 2, 2.0 ** kh
    if out == "y_yp":
        a.Y = p["y"]
    if arith == "mx4":
        a.mx, a.x_rowscale, a.w_rowscale = 2, p["x_rowscale"], p["w_rowscale"]
    else:
        a.mx, a.mx_scale, a.mx_scale_b = 1, scale_byte4(127 - ka - 11), scale_byte4(127 - kw)
    return a


def ffn2_block(Cc, R, rm, p, ka=0, kw=0):
    """FFN2 + LN2 in the mx arithmetic: k = 1, A as mx planes, the mx weight image, the residual from mx (rm 1) or mx4 (rm 2) planes, split-bf16 planes out."""
    a = GemmArgs()
    a.C = a.Cpad = Cc
    a.ktaps, a.N, a.R = 1, N_OUT, R
    a.W = a.Wb = p["w"]
    a.Xp, a.row_pos, a.bias = p["x"], p["pos"], p["bias"]
    a.ldr, a.ldy = N_OUT, N_OUT
    a.ln_g, a.ln_b, a.ln_eps = p["gamma"], p["beta"], 1e-5
    a.Yp, a.yp_chunks, a.x_scale = p["yp"], N_OUT // 32, 1.0
    a.mx, a.mx_scale, a.mx_scale_b = 1, scale_byte4(127 - ka - 11), scale_byte4(127 - kw)
    a.residp, a.residp_chunks, a.residp_mx, a.residp_scale = p["residp"], N_OUT // 32, rm, 2.0 ** -(KA_RES + 11)
    return a


# ---- the LayerNorm-terminated convolutions of the variance predictors (tests/test_gpu_pred_kernels.py), formed as predictor_step / fused_predictor_steps
# (csrc/model_launches.h) form them: relu_pre, ln_eps = 1e-12, planes in, a scratch buffer, no fp32 rows out.
#   mid      a hidden layer: planes out                                                      gemm_row8c_bf16<.., nb, mt, 1>
#   head     the last layer: the scalar head, nothing but dot_out leaves                      the same
#   half0/1  energy.conv0 / pitch.conv0: N = 256 into its half of a 512-column plane row     the same, yp_col_off
#   two_ln   var.conv0: both layers stacked, N = 512, one LayerNorm per 256 columns          gemm_row8c_bf16<.., 4, 2, 2>
#   grouped  var.conv1: group g contracts channels [g C, (g + 1) C) of the stacked row with its own weights, LayerNorm and head; as in the model it writes
#            no planes: its two heads are all that leaves                                    gemm_row8c_bf16<.., nb, mt, 1>, grid.y = group
# and, where the row kernels are switched off, gemm_pl_bf16's conv form + ln_rows, with and without split-K.
PRED_EPS = 1e-12
PRED_TOL = MX_CEILING                  # GEMM_TOL["bf16x3"]: the pre-LayerNorm error of the split-bf16 arithmetic on these distributions
PRED_QUIET = 2.0 ** -10                # the scale of x and bias in the `quiet` variant
PRED_FORMS = ("mid", "head", "half0", "half1", "two_ln", "grouped")
# (form, chans, k, R, variant).  R = 333: three 128-row tiles, two of 192 rows, each with a ragged last one; 128: exactly one 128-row tile, a partial one of 192.
# chans 384: nb = 3.  k = 5: P = 2, the other parity of the A tile's instruction count.  The halves ride on the two_ln cases: the same stacked operands.
PRED_CASES = ([(f, 256, 3, R, "") for R in (333, 128) for f in ("mid", "head", "two_ln", "grouped")] +
              [(f, 384, 3, R, "") for R in (333, 128) for f in ("mid", "head", "grouped")] +
              [(f, 256, 5, R, "") for R in (333, 128) for f in ("mid", "head")] +
              [(f, 256, 3, 128, "quiet") for f in ("head", "grouped")] +
              [(f, 256, 3, 128, "dead_window") for f in ("mid", "head")] +
              [(f, 256, 3, 333, "hi_only") for f in ("mid", "two_ln", "grouped")])
PRED_IDS = ["%s-c%d-k%d-R%d%s" % (c[:4] + ("-" + c[4] if c[4] else "",)) for c in PRED_CASES]
# The bars: a share of the ceiling
#     ceiling(row, col) = PRED_TOL max(1, s rstd |gamma| (2 + |yhat|)),      head: Sum_col ceiling |dot_w| + PRED_TOL
# (a pre-LayerNorm error d moves LN(y)_i by at most rstd |gamma_i| (2 + |yhat_i|) max |d| to first order, mean |yhat| <= 1; s = 2^-10 in the quiet variant, else 1).
# The shares come from the reference side alone: 8 x the worst error-to-ceiling ratio of the kernels' arithmetic stated in fp32 on the CPU (pred_fp32: hi.hi + hi.lo +
# lo.hi, fp32 accumulation, fp32 ReLU / LayerNorm / head, the planes' rounding) over all PRED_CASES -- 8 x because the MFMA and wave-reduction orders differ from
# torch's -- capped at 1.  Measured (tests/test_gemm_raw_host.py prints them per case): planes 0.01281 (grouped, chans 256, R = 128; every case lies in
# 0.0065 .. 0.0128), heads 3.64e-4 (head, chans 256, k = 3, R = 333; 2.2e-5 .. 3.6e-4), rounded up.  The GPU's figures do not enter; for the record, its worst
# error-to-ceiling ratios per form on the MI355X (tests/test_gpu_pred_kernels.py records them): planes mid 0.01132, two_ln 0.01124, the halves 0.01120 (share 0.1026);
# heads head 3.55e-4, grouped 3.94e-4 (share 2.92e-3).  The planes' figure is mostly the planes' own rounding (2^-17 |v|), the same on both sides.
PRED_FP32_RATIO = (0.01282, 3.65e-4)
PRED_BAR_SHARE = min(1.0, 8 * PRED_FP32_RATIO[0])
PRED_HEAD_SHARE = min(1.0, 8 * PRED_FP32_RATIO[1])


def pred_geometry(form, chans):
    """(C a group contracts, channels of an x row, N of the launch, columns of an output plane row, k_groups, ln_groups)."""
    if form == "grouped":
        return chans, 2 * chans, 2 * chans, 2 * chans, 2, 2
    if form == "two_ln":
        return chans, chans, 512, 512, 1, 2
    if form in ("half0", "half1"):
        return chans, chans, 256, 512, 1, 1
    return chans, chans, chans, chans, 1, 1


def pred_has_planes(form):
    return form in ("mid", "half0", "half1", "two_ln")


def pred_gstride(R):
    """Floats between the two groups' head arrays: more than R, so that there is a gap between them that must stay untouched."""
    return rpad(R) + 64


def pred_kpart_cap(form, chans, R):
    return 4 * rpad(R) * pred_geometry(form, chans)[2]


def pred_ksplit(Cpad, k, N, R, allowed=3):
    """csrc/gemm_plan.h: pick_ksplit with an ample kpart_cap (the CPU test holds it against the compiled plan of every split-K block)."""
    nch, wgs = Cpad // 32, (N + 127) // 128 * ((R + 63) // 64)
    for cand in (4, 3, 2):
        if nch % cand == 0 and (nch // cand) * k >= 4 and wgs * cand <= 1024 and cand - 1 <= allowed:
            return cand
    return 1


def pred_runs(form):
    """[(run, mt)]: the row kernel at both heights (two_ln exists at 128 rows only), the sibling without and with split-K; with two_ln the two half launches, in
    the order they are sent: half0 then half1 into one buffer at 128 rows, half1 then half0 into another at 192."""
    runs = ([("row", 2)] if form == "two_ln" else [("row", 2), ("row", 3)]) + [("sib", 0), ("sibk", 0)]
    return runs + ([("half0", 2), ("half1", 2), ("half1", 3), ("half0", 3)] if form == "two_ln" else [])


def pred_options(run, mt):
    return {"FS2_ROW8": 0} if run in ("sib", "sibk") else {"FS2_ROW8": 1, "FS2_MT8": mt}


def pred_precision(variant):
    return "bf16" if variant == "hi_only" else "bf16x3"


def pred_expected(form, chans, k, R, variant, run, mt):
    """The plan of one run: every field the GPU test asserts."""
    f = form if run in ("row", "sib", "sibk") else run
    Cg, _, N, _, kg, _ = pred_geometry(f, chans)
    ns = 1 if variant == "hi_only" else 3
    if run in ("sib", "sibk"):
        return dict(kernel="pl_bf16", bm=64, nsplit=ns, ksplit=pred_ksplit(Cg, k, N, R) if run == "sibk" else 1, rows_pass=1, build_planes=0)
    kernel = {"two_ln": "row8c_two_ln", "grouped": "row8c_grouped"}.get(f, "row8c")
    return dict(kernel=kernel, nb=4 if f == "two_ln" else (3 if N // kg == 384 else 2), mt=mt, nsplit=ns, ksplit=1, rows_pass=0, build_planes=0)


def pred_block(form, chans, k, R, p, split=False):
    """The argument block of one predictor conv launch; p: name -> pointer (int) of the case's buffers (the halves take their slices of the stacked ones);
    split: the call's split-K scratch named, three partial buffers allowed (call_defaults)."""
    Cg, Cx, N, Nrow, kg, lg = pred_geometry(form, chans)
    half = 1 if form == "half1" else 0
    a = GemmArgs()
    a.C = a.Cpad = Cg
    a.ldx, a.ktaps, a.N, a.R, a.ldy = Cx, k, N, R, N
    a.W = a.Wb = p["w"] + half * 256 * (Cg // 32) * k * 128
    a.Xp, a.row_pos = p["x"], p["pos"]
    a.bias, a.ln_g, a.ln_b = p["bias"] + half * 1024, p["gamma"] + half * 1024, p["beta"] + half * 1024
    a.relu_pre, a.ln_eps, a.x_scale = 1, PRED_EPS, 1.0
    a.scratch = p["scratch"]
    if pred_has_planes(form):
        a.Yp, a.yp_chunks, a.yp_col_off = p["yp"], Nrow // 32, half * 256
    else:
        a.dot_w, a.dot_b, a.dot_out = p["dot_w"], p["dot_b"], p["dot_out"]
    if lg > 1:
        a.ln_groups = lg
    if kg > 1:
        a.k_groups, a.xp_row_chunks, a.dot_gstride = kg, Cx // 32, pred_gstride(R)
    if split:
        a.kpart, a.kpart_cap, a.ksplit = p["kpart"], pred_kpart_cap(form, chans, R), 3
    return a


def pred_launches(p):
    out = []
    for (form, chans, k, R, variant), cid in zip(PRED_CASES, PRED_IDS):
        for run, mt in pred_runs(form):
            want = pred_expected(form, chans, k, R, variant, run, mt)
            want["precision"] = pred_precision(variant)
            out.append(("pred-%s-%s-mt%d" % (cid, run, mt), pred_options(run, mt), pred_block(form if run in ("row", "sib", "sibk") else run, chans, k, R, p, split=run == "sibk"), want))
    return out


def all_launches(p=None):
    """[(id, switches, block, expected plan fields)] of every launch the GPU tests send; p: pointers (default: placeholders).  Expected fields: those of `Plan`;
    "precision" (default "bf16x3") is the precision the launch is sent with, not a field of the plan."""
    p = p if p is not None else collections.defaultdict(lambda: 0x1000)
    out = pred_launches(p)
    for arith in CONV_ARITHS:
        for k, N, R in CONV_CASES:
            for o in CONV_OUTS:
                out.append(("conv-%s-k%d-N%d-R%d-%s" % (arith, k, N, R, o), {}, conv_block(arith, k, N, R, o, p), conv_expected(arith)))
    for form, R, Cc in EPI4_CASES:
        for side, mt in ROW4_RUNS:
            out.append(("%s-R%d-C%d-%s-mt%d" % (form, R, Cc, side, mt), ln_options(side, mt), ln_block(form, R, Cc, side, p),
                        dict(zip(("kernel", "epi", "res", "mt"), ln_expected(form, side, mt)))))
    for Cc, R, rm in FFN2_CASES:
        for side, mt in ROW4_RUNS:
            out.append(("ffn2mx-C%d-R%d-rm%d-mt%d" % (Cc, R, rm, mt), ln_options(side, mt), ffn2_block(Cc, R, rm, p), dict(kernel="row4", epi=0, arith=2, res=2, mt=mt)))
        # (its sibling on split-bf16 operands: the same values, the same residual planes)
        out.append(("ffn2bf-C%d-R%d-rm%d-mt4" % (Cc, R, rm), ln_options("row4", 4), ln_block("epi0_res2", R, Cc, "row4", p, rm=rm), dict(kernel="row4", epi=0, arith=0, res=2, mt=4)))
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
        if f.get("gamma_spread"):      # one gain per 16-channel slot, 2 .. 2 / spread in a shuffled order
            g = 2.0 * f["gamma_spread"] ** -(rs.permutation(N_OUT // 16) / (N_OUT // 16 - 1.0))
            self.gamma = self.gamma * torch.from_numpy(np.repeat(g, 16).astype(np.float32))
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
        if self.epi == 4:      # (the value the residual reader sees: fp16 + the e4m3 residual at 3 C; the cross units need the scale record: decode_mx4)
            b = yp_bytes.contiguous().view(torch.uint8).reshape(-1)[:self.R * N_OUT * 4].reshape(self.R, 4 * N_OUT)
            return mx_value(b[:, :2 * N_OUT].contiguous().view(torch.float16), b[:, 3 * N_OUT:].contiguous(), KA_OUT), None
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


def e2m1_on_tie(v):
    """Elements of v that sit exactly on the midpoint of two e2m1 codes."""
    mag = v.double().abs()
    t = torch.zeros(mag.shape, dtype=torch.bool)
    for e in _E2M1_EDGE:
        t |= mag == e
    return t


def repack_weights(N, Cc, k, seed):
    """fp32 [N, C, k] for the repack comparison: the model-like distribution (every 16-channel block its own gain), with no element whose fp16 part or residual
    lands on a rounding tie of e2m1 under its block's scale -- there the byte depends on the tie rule of the hardware conversion alone (one fp16 value in 1024 per
    binade is such a midpoint, so random weights do hit them); elements that would are moved by 2^-7 of themselves until none is left."""
    rs = np.random.RandomState(seed)
    w = _uni(rs, N, Cc, k) * _gain(rs, N, Cc // 16).repeat_interleave(16, dim=1).unsqueeze(2) / np.sqrt(Cc * k)
    for _ in range(8):
        h = w.half()
        inv = mx4_inv_scale(mx4_scale_byte(h.float().abs().reshape(N, Cc // 16, 16, k).amax(2))).repeat_interleave(16, dim=1)
        tie = e2m1_on_tie(h.double() * inv) | e2m1_on_tie((w - h.float()).double() * 2048.0 * inv)
        if not bool(tie.any()):
            return w
        w = torch.where(tie, w * (1.0 + 2.0 ** -7), w)
    raise AssertionError("ties left")


def epi4_scale_bounds(ref, bar):
    """The scale byte (of s itself) of every slot of the float64 LayerNorm output ref [R, N] by the rule of csrc/common.h: (lowest, highest) byte a kernel whose
    values lie within `bar` [R, N] of ref may write: they differ only for a slot whose maximum lies within the bar of a binade edge."""
    R = ref.shape[0]
    lo = (ref.abs() - bar).clamp(min=0.0).reshape(R, -1, 16).amax(2)
    hi = (ref.abs() + bar).reshape(R, -1, 16).amax(2) * (ref.abs().reshape(R, -1, 16).amax(2) > 0)
    return mx4_scale_byte(lo.float()), mx4_scale_byte(hi.float())


_E4M3_SORTED = None


def e4m3_cell(b):
    """The interval of reals that round to the e4m3 byte b (round to nearest; the ends included, whichever way ties go): (lo, hi) float64, signed."""
    global _E4M3_SORTED
    if _E4M3_SORTED is None:
        mags = e4m3_value(torch.arange(0, 0x7F, dtype=torch.uint8))           # 0 .. 448, ascending
        mid = (mags[1:] + mags[:-1]) / 2
        _E4M3_SORTED = (torch.cat([torch.zeros(1, dtype=torch.float64), mid]), torch.cat([mid, torch.tensor([float("inf")], dtype=torch.float64)]))      # (the kernels clamp to 448)
    m = (b & 0x7F).long()
    lo, hi = _E4M3_SORTED[0][m], _E4M3_SORTED[1][m]
    neg = (b >> 7).bool()
    return torch.where(neg, -hi, torch.where(m == 0, -hi, lo)), torch.where(neg, torch.where(m == 0, hi, -lo), hi)


def _fp16_ulp(h):
    """The spacing of fp16 at h (normal values)."""
    return torch.pow(torch.tensor(2.0), torch.floor(torch.log2(h.float().abs())) - 10.0)


def _gain(rs, *shape):
    return torch.from_numpy((2.0 ** rs.uniform(-3.0, 3.0, size=shape)).astype(np.float32))


def mixed_operands(rs, dist, rows, Cc, N, k, wnorm):
    """(a [rows, C], w [N, C, k]) fp32 of one of the two distributions of the mixed-mode launches.
    model:    uniform values with per-channel gains spread over 2^+-3 (activations) and per 16-channel block and output channel (weights): the slots of a
              row, and the blocks of a weight row, take different scale bytes.
    coherent: every a lies 0.45 fp16 ulp above its fp16 value, sign(a) is one sign per channel, every wh is positive and rw = sign(a) 0.45 ulp: all ra.wh
              and ah.rw terms of an output add up -- about 1e-2 of the output instead of about 1e-4."""
    ga, gw = _gain(rs, Cc), _gain(rs, N, Cc // 16).repeat_interleave(16, dim=1).unsqueeze(2)
    if dist == "model":
        return _uni(rs, rows, Cc) * ga, _uni(rs, N, Cc, k) * gw * wnorm
    sgn = torch.from_numpy(rs.choice([-1.0, 1.0], size=Cc).astype(np.float32))
    ah = (torch.from_numpy(rs.uniform(0.25, 1.0, size=(rows, Cc)).astype(np.float32)) * ga * sgn).half()
    wh = (torch.from_numpy(rs.uniform(0.25, 1.0, size=(N, Cc, k)).astype(np.float32)) * gw * wnorm).half()
    def above(h, s):      # (towards zero from a power of two the spacing halves: 0.45 of the smaller one there)
        v = h.float() + 0.45 * _fp16_ulp(h) * s
        return torch.where(v.half() == h, v, h.float() + 0.225 * _fp16_ulp(h) * s)
    a, w = above(ah, torch.ones(1)), above(wh, sgn.reshape(1, Cc, 1))
    assert torch.equal(a.half(), ah) and torch.equal(w.half(), wh)
    return a, w


class ConvOperands:
    """Operands of one FFN-conv case as the tuples the kernel reads, their images, and the float64 value of the kernel's formula on them."""

    def __init__(self, arith, k, N, R, dist, x_tuples=None):
        self.arith, self.k, self.N, self.R, self.dist, self.C = arith, k, N, R, dist, CONV_C
        rs = np.random.RandomState(10000 * CONV_ARITHS.index(arith) + 1000 * DISTS.index(dist) + 100 * k + N + R)
        Rp = rpad(R)
        self.pos = row_positions(R)
        a, w = mixed_operands(rs, dist, Rp, CONV_C, N, k, 1.0 / (8.0 * np.sqrt(CONV_C * k)))
        a = a * (self.pos >= 0).unsqueeze(1)                 # gap rows and the rows behind R are zeros, as their producer leaves them
        self.bias = _uni(rs, N, scale=0.1)
        self.ka, self.kw = fp8_scale_exponent(float(a.abs().max())), fp8_scale_exponent(float(w.abs().max()))
        if arith == "mx4":
            self.x = x_tuples if x_tuples is not None else split_mx4(a, self.ka)
            self.w = split_mx4(w, 0, slot_dim=1)
            self.x_planes, self.x_rowscale = encode_mx4(self.x)
            self.w_image, self.w_scales = image_w_mx4(self.w)
        else:
            self.x, self.w = split_mx3(a, self.ka), split_mx3(w, self.kw)
            self.x_planes, self.x_rowscale = encode_mx3(self.x), None
            self.w_image, self.w_scales = image_w_mx(self.w), None
        self.ref = self.formula(self.x, self.w)
        self.kh = fp8_scale_exponent(max(1.01 * float(self.ref.abs().max()), 1.0))

    def terms(self, x, w):
        return mx4_terms(x, w) if self.arith == "mx4" else mx_terms(x, w, scale_byte4(127 - self.ka - 11), scale_byte4(127 - self.kw))

    def formula(self, x, w):
        return ref_conv(*self.terms(x, w), self.bias, self.pos, self.R)

    def mutant(self, which):
        return self.formula(*(mutant_mx4 if self.arith == "mx4" else mutant_mx)(self.x, self.w, which))

    def mutants(self):
        return MX4_MUTANTS if self.arith == "mx4" else MX_MUTANTS


class Ffn2Operands:
    """Operands of one FFN2 + LN2 case in the mx arithmetic (A as mx planes, the mx weight image at k = 1, the residual as mx or mx4 planes) and the float64
    value of the kernel's formula -> LayerNorm."""

    def __init__(self, Cc, R, rm, dist):
        self.C, self.R, self.rm, self.dist = Cc, R, rm, dist
        rs = np.random.RandomState(1000 * DISTS.index(dist) + 100 * rm + Cc + R)
        Rp = rpad(R)
        self.pos = row_positions(R)
        a, w = mixed_operands(rs, dist, Rp, Cc, N_OUT, 1, 1.0 / (4.0 * np.sqrt(Cc)))
        self.a32, self.w32 = a, w[:, :, 0]
        self.bias, self.gamma, self.beta = _uni(rs, N_OUT, scale=0.5), 1.0 + _uni(rs, N_OUT, scale=0.2), _uni(rs, N_OUT, scale=0.2)
        self.ka, self.kw = fp8_scale_exponent(float(a.abs().max())), fp8_scale_exponent(float(w.abs().max()))
        self.x, self.w = split_mx3(a, self.ka), split_mx3(w, self.kw)
        self.x_planes, self.w_image = encode_mx3(self.x), image_w_mx(self.w)
        r = _uni(rs, Rp, N_OUT)
        if rm == 1:
            h, e8 = split_mx(r, KA_RES)
            self.resid_planes, self.resid_value, self.resid_2c = encode_mx(h, e8, KA_RES), mx_value(h, e8, KA_RES), None
        else:
            t = split_mx4(r, KA_RES)
            self.resid_planes, _ = encode_mx4(t)
            self.resid_value = mx_value(t.h, t.e8, KA_RES)
            at2c = self.resid_planes[:, 2 * N_OUT:3 * N_OUT].contiguous()          # what a reader of the mx planes' position would take for the residual bytes
            self.resid_2c = t.h.double() + torch.nan_to_num(e4m3_value(at2c), nan=448.0) * 2.0 ** -(KA_RES + 11)
        self.ref = self.formula(self.x, self.w, self.resid_value)

    def formula(self, x, w, resid):
        ta, tw = mx_terms(x, w, scale_byte4(127 - self.ka - 11), scale_byte4(127 - self.kw))
        return ref_rows(ta[:self.R], tw[:, :, 0], self.bias.double(), resid[:self.R], self.gamma.double(), self.beta.double(), self.pos[:self.R])

    def mutants(self):
        return MX_MUTANTS + (("resid_at_2c",) if self.rm == 2 else ())

    def mutant(self, which):
        if which == "resid_at_2c":
            return self.formula(self.x, self.w, self.resid_2c)
        return self.formula(*mutant_mx(self.x, self.w, which), self.resid_value)


# ---- the predictors' conv launches: operands, the float64 reference, the fp32 statement, the mutants
def pred_positions(R):
    """Row 0 is live, so that the tap at row -1 lies in front of the buffer: 105-row "utterances" with 4 gap rows behind each ((r + 4) % 109 < 4); rows >= R
    are gaps.  The rows on both sides of the tile edges 127 / 128, 191 / 192, 255 / 256 and the last row (R = 333, 128) are live with live neighbours: every
    halo tap at a tile edge and at R - 1 counts."""
    r = torch.arange(rpad(R))
    return torch.where(((r + 4) % 109 < 4) | (r >= R), torch.full_like(r, -1), (r + 4) % 109 - 4).int()


PredRef = collections.namedtuple("PredRef", "v head rstd yhat")      # [R, N], [R, G] or None, [R, G], [R, N]


def pred_conv(x, w, bias, k_groups=1, front=None):
    """y = bias + Sum_tap Sum_c w[n, c, tap] x[r + tap - P, c] with zeros outside [0, R); group g of a grouped layer contracts channels [g C, (g + 1) C) of the
    row.  float64 [R, N].  front: P rows that stand in front of row 0 instead of zeros (a mutant)."""
    R, (N, Cg, k) = x.shape[0], w.shape
    P = (k - 1) // 2
    pad = torch.zeros(P, x.shape[1], dtype=torch.float64)
    xx = torch.cat([pad if front is None else front, x, pad])
    Ng = N // k_groups
    y = bias.unsqueeze(0).expand(R, N).clone()
    for g in range(k_groups):
        for tap in range(k):
            y[:, g * Ng:(g + 1) * Ng] += xx[tap:tap + R, g * Cg:(g + 1) * Cg] @ w[g * Ng:(g + 1) * Ng, :, tap].t()
    return y


def pred_rows(y, gamma, beta, pos, ln_groups=1, dot_w=None, dot_b=None, eps=PRED_EPS, relu=True, head_groups=None):
    """ReLU -> LayerNorm over each group's N / G columns -> gamma, beta; gap rows zero; the head of group g = v . dot_w[g] + dot_b[g].  Also rstd and the
    normalised rows: the bars need them."""
    R, N = y.shape
    G = ln_groups
    if relu:
        y = y.clamp(min=0.0)
    yg = y.reshape(R, G, N // G)
    mu = yg.mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(((yg - mu) ** 2).mean(2, keepdim=True) + eps)
    yhat = ((yg - mu) * rstd).reshape(R, N)
    live = (pos >= 0).unsqueeze(1)
    v = (yhat * gamma + beta) * live
    head = None
    if dot_w is not None:
        H = head_groups or G
        head = ((v * dot_w).reshape(R, H, N // H).sum(2) + dot_b[:H]) * live
    return PredRef(v, head, rstd.reshape(R, G), yhat)


def ref_pred(x, w, bias, gamma, beta, pos, k_groups=1, ln_groups=1, dot_w=None, dot_b=None):
    """The predictors' conv layer in float64 on the values the kernels see."""
    return pred_rows(pred_conv(x, w, bias, k_groups), gamma, beta, pos, ln_groups, dot_w, dot_b)


class PredOperands:
    """Operands of one predictor conv case on the CPU: x and w as exact bf16 pairs (the `_uni` distributions, w at 1 / sqrt(C k), dot_w at 1 / sqrt(N)), x zero in
    gap rows (the contract of the packed layout), the float64 result, the ceilings of the bars.  The halves of a two_ln case are slices of these.
    quiet: x and bias x 2^-10 exactly (every product and sum scales exactly in fp32, the row variance is ~5e-8: far below 1e-5, far above 1e-12).
    dead_window: bias = -0.5 - |u| and 2 P + 3 zero x rows inside the first utterance: the rows whose whole window is zero (`dead`) have every output <= 0 in front
    of the ReLU, variance exactly 0, rstd = 1e6, and the result exactly beta.   hi_only: every lo half zero (the one-term kernels are exact on such operands)."""

    def __init__(self, form, chans, k, R, variant=""):
        assert form in ("mid", "head", "two_ln", "grouped") and variant in ("", "quiet", "dead_window", "hi_only") and (form != "two_ln" or chans == 256)
        self.form, self.chans, self.k, self.R, self.variant = form, chans, k, R, variant
        self.Cg, self.Cx, self.N, self.Nrow, self.kg, self.lg = pred_geometry(form, chans)
        self.P = P = (k - 1) // 2
        rs = np.random.RandomState(7000 + 1000 * PRED_FORMS.index(form) + 10 * chans + 100 * k + R)      # (a variant changes the loud case's operands)
        Rp, N = rpad(R), self.N
        self.pos = pred_positions(R)
        x = _uni(rs, Rp, self.Cx)
        x = torch.where((self.pos >= 0).unsqueeze(1), x, torch.zeros_like(x))
        w = _uni(rs, N, self.Cg, k, scale=1.0 / np.sqrt(self.Cg * k))
        self.bias, self.gamma, self.beta = _uni(rs, N, scale=0.5), 1.0 + _uni(rs, N, scale=0.2), _uni(rs, N, scale=0.2)
        self.dot_w, self.dot_b = _uni(rs, N, scale=1.0 / np.sqrt(N // self.lg)), _uni(rs, 2, scale=0.5)
        self.s, self.dead = 1.0, []
        if variant == "dead_window":
            self.bias = -0.5 - self.bias.abs()
            x[40:40 + 2 * P + 3] = 0.0
            self.dead = list(range(40 + P, 40 + P + 3))
        if variant == "quiet":
            self.s = PRED_QUIET
            x, self.bias = x * PRED_QUIET, self.bias * PRED_QUIET
        self.x, self.w = split_bf16(x), split_bf16(w)
        if variant == "hi_only":
            self.x, self.w = (self.x[0], torch.zeros_like(self.x[1])), (self.w[0], torch.zeros_like(self.w[1]))
        self.xv, self.wv = pair_value(*self.x)[:R], pair_value(*self.w)
        self.has_head = not pred_has_planes(form)
        self.ref = self.rows(self.conv())
        # the ceilings (see PRED_BAR_SHARE)
        rstd = self.ref.rstd.repeat_interleave(N // self.lg, dim=1)
        self.ceiling = PRED_TOL * (self.s * rstd * self.gamma.double().abs() * (2.0 + self.ref.yhat.abs())).clamp(min=1.0)
        self.head_ceiling = (self.ceiling * self.dot_w.double().abs()).reshape(R, self.lg, -1).sum(2) + PRED_TOL

    def conv(self, x=None, w=None, bias=None, **kw):
        return pred_conv(self.xv if x is None else x, self.wv if w is None else w, self.bias.double() if bias is None else bias, self.kg, **kw)

    def rows(self, y, **kw):
        args = dict(ln_groups=self.lg, dot_w=self.dot_w.double() if self.has_head else None, dot_b=self.dot_b.double() if self.has_head else None)
        args.update(kw)
        return pred_rows(y, self.gamma.double(), self.beta.double(), self.pos[:self.R], **args)

    def bars(self):
        """(the planes' bar [R, N], the heads' [R, G])."""
        return PRED_BAR_SHARE * self.ceiling, PRED_HEAD_SHARE * self.head_ceiling

    def ksplit(self):
        return pred_ksplit(self.Cg, self.k, self.N, self.R)

    # what a kernel with one broken rule would compute (tests/test_gemm_raw_host.py holds every one at >= 8 bars on the rows it concerns)
    def mutants(self):
        m = ["taps_reversed", "row0_front", "no_relu", "relu_per_partial"] + (["edge_plus_tap"] if self.R > 256 else []) + (["eps_1e-5"] if self.variant == "quiet" else [])
        return m + (["one_ln"] if self.lg > 1 else []) + (["groups_crossed", "head_bias0", "head_swapped"] if self.kg > 1 else [])

    def mutant(self, which):
        """-> (PredRef of the mutant, the rows it concerns or None for all)."""
        R, P, k = self.R, self.P, self.k
        if which == "taps_reversed":
            return self.rows(self.conv(w=self.wv.flip(2))), None
        if which == "row0_front":              # the taps in front of row 0 read rows that are not zero
            return self.rows(self.conv(front=self.xv[P + 1:2 * P + 1])), list(range(P))
        if which == "edge_plus_tap":           # the taps behind the row just below a tile edge (128, 192, 256 rows) are missing: the halo rows of the A tile
            edge = [e - 1 for e in (128, 192, 256) if e < R]
            w0 = self.wv.clone()
            w0[:, :, P + 1:] = 0.0
            y = self.conv()
            y[edge] = self.conv(w=w0)[edge]
            return self.rows(y), edge
        if which == "groups_crossed":          # the groups contract each other's channels
            return self.rows(self.conv(x=torch.cat([self.xv[:, self.Cg:], self.xv[:, :self.Cg]], dim=1))), None
        if which == "one_ln":                  # one LayerNorm over all the columns of a row
            return self.rows(self.conv(), ln_groups=1, head_groups=self.lg), None
        if which == "eps_1e-5":
            return self.rows(self.conv(), eps=1e-5), None
        if which == "no_relu":
            return self.rows(self.conv(), relu=False), None
        if which == "relu_per_partial":        # ReLU on each split-K partial sum (the chunks split as pick_ksplit splits them; bias with the first) before they are added
            cand = self.ksplit()
            assert cand > 1
            per = self.Cg // cand
            y = torch.zeros(R, self.N, dtype=torch.float64)
            for z in range(cand):
                keep = torch.zeros(self.Cx, dtype=torch.bool)
                for g in range(self.kg):
                    keep[g * self.Cg + z * per:g * self.Cg + (z + 1) * per] = True
                y += self.conv(x=self.xv * keep, bias=self.bias.double() * (z == 0)).clamp(min=0.0)
            return self.rows(y), None
        if which == "head_bias0":              # dot_b[0] for dot_b[g]
            return self.rows(self.conv(), dot_b=self.dot_b.double()[[0, 0]]), None
        if which == "head_swapped":            # each head written to the other group's array
            r = self.rows(self.conv())
            return r._replace(head=r.head.flip(1)), None
        raise KeyError(which)

    def distance(self, other, rows=None):
        """The worst |other - ref| in bars over `rows`: of the planes where the form writes planes, else of the heads."""
        bar_v, bar_h = self.bars()
        q = ((other.head - self.ref.head).abs() / bar_h) if self.has_head else ((other.v - self.ref.v).abs() / bar_v)
        return float((q if rows is None else q[rows]).max())


def pred_fp32(ops):
    """The kernels' arithmetic stated in fp32 on the CPU: hi.hi + hi.lo + lo.hi with fp32 accumulation, fp32 ReLU / LayerNorm (two passes) / head; the values as
    the planes hold them (hi + lo of the fp32 result).  -> (v float64 [R, N], head float64 [R, G] or None)."""
    R, N, Cg, k, P = ops.R, ops.N, ops.Cg, ops.k, ops.P
    pad = torch.zeros(P, ops.Cx)
    xh, xl = (torch.cat([pad, t[:R].float(), pad]) for t in ops.x)
    wh, wl = ops.w[0].float(), ops.w[1].float()
    Ng = N // ops.kg
    y = ops.bias.unsqueeze(0).expand(R, N).clone()
    for g in range(ops.kg):
        cs, ns = slice(g * Cg, (g + 1) * Cg), slice(g * Ng, (g + 1) * Ng)
        for tap in range(k):
            ah, al = xh[tap:tap + R, cs], xl[tap:tap + R, cs]
            y[:, ns] += al @ wh[ns, :, tap].t() + ah @ wl[ns, :, tap].t() + ah @ wh[ns, :, tap].t()
    y = y.clamp(min=0.0).reshape(R, ops.lg, N // ops.lg)
    mu = y.mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mu) ** 2).mean(2, keepdim=True) + torch.tensor(PRED_EPS, dtype=torch.float32))
    live = (ops.pos[:R] >= 0).unsqueeze(1)
    zero = torch.zeros(1)
    v = torch.where(live, ((y - mu) * rstd).reshape(R, N) * ops.gamma + ops.beta, zero)                   # (+0.0 in gap rows, as the kernels write it)
    head = torch.where(live, (v * ops.dot_w).reshape(R, ops.lg, -1).sum(2) + ops.dot_b[:ops.lg], zero) if ops.has_head else None
    return pair_value(*split_bf16(v)), (None if head is None else head.double())


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
        rowscale = sentinel(rpad(self.ops.R) * 32)          # (handed over by the EPI 4 form only)
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p.update(yp=yp.data_ptr(), y=y.data_ptr(), rowscale=rowscale.data_ptr())
        a = ln_block(self.ops.form, self.ops.R, self.ops.C, side, p)
        plan = launch(a)
        self.rowscale = rowscale.cpu()
        return plan, yp.cpu(), y.cpu()


class ConvCase:
    """One FFN-conv case on the GPU.  Behind row R the planes and the scale records hold 0xFF (NaN in fp16 and e4m3, a scale of 2^128): the kernel has to take
    the rows outside [0, R) for zeros without reading them."""

    def __init__(self, ops, x_planes=None, x_rowscale=None):
        self.ops = ops
        d = _dev()
        xp = (ops.x_planes if x_planes is None else x_planes).clone()
        xp[ops.R:] = 0xFF
        self.keep = dict(x=xp.to(d), w=ops.w_image.to(d), pos=ops.pos.to(d), bias=ops.bias.to(d))
        if ops.arith == "mx4":
            rec = (ops.x_rowscale if x_rowscale is None else x_rowscale).clone()
            rec[ops.R:] = 0xFF
            self.keep.update(x_rowscale=rec.to(d), w_rowscale=ops.w_scales.to(d))
        self.out_bytes = rpad(ops.R) * ops.N * 4      # (fp32 rows and mx planes: 4 bytes per element; whole tiles of rows behind R, all of which must stay untouched)

    def run(self, out):
        """-> (plan, yp bytes (mx planes, CPU, with guard), y bytes)."""
        yp, y = sentinel(self.out_bytes), sentinel(self.out_bytes)
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p.update(yp=yp.data_ptr(), y=y.data_ptr())
        o = self.ops
        plan = launch(conv_block(o.arith, o.k, o.N, o.R, out, p, ka=o.ka, kw=o.kw, kh=o.kh))
        return plan, yp.cpu(), y.cpu()


class Ffn2Case:
    def __init__(self, ops):
        self.ops = ops
        d = _dev()
        self.keep = dict(x=ops.x_planes.to(d), w=ops.w_image.to(d), pos=ops.pos.to(d), bias=ops.bias.to(d), gamma=ops.gamma.to(d), beta=ops.beta.to(d),
                         residp=ops.resid_planes.to(d))
        self.out_bytes = rpad(ops.R) * N_OUT * 4

    def run(self, mt, set_option):
        """-> (plan, yp bytes: split-bf16 planes)."""
        for k, v in ln_options("row4", mt).items():
            set_option(k, v)
        yp = sentinel(self.out_bytes)
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p["yp"] = yp.data_ptr()
        o = self.ops
        plan = launch(ffn2_block(o.C, o.R, o.rm, p, ka=o.ka, kw=o.kw))
        return plan, yp.cpu()

    def run_split_bf16(self, set_option):
        """The same values and residual planes through the split-bf16 arithmetic (ARITH = 0, the epi0_res2 form) -> (plan, yp bytes)."""
        for k, v in ln_options("row4", 4).items():
            set_option(k, v)
        o, d = self.ops, _dev()
        x, w = encode_planes(*split_bf16(o.a32)).to(d), encode_planes(*split_bf16(o.w32)).to(d)
        yp = sentinel(self.out_bytes)
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p.update(x=x.data_ptr(), w=w.data_ptr(), yp=yp.data_ptr())
        plan = launch(ln_block("epi0_res2", o.R, o.C, "row4", p, rm=o.rm))
        return plan, yp.cpu()


class PredCase:
    """One predictor conv case on the GPU: the operands uploaded once, one run per entry of pred_runs into fresh sentinel buffers (the second half launch of a pair
    into the buffer of the first).  Behind row R the x planes hold 0xFF (NaN): the kernels have to take the rows outside [0, R) for zeros without reading them."""

    def __init__(self, ops):
        self.ops = o = ops
        d = _dev()
        xp = encode_planes(*o.x).contiguous()
        xp.view(torch.uint8)[o.R:] = 0xFF
        self.keep = dict(x=xp.to(d), w=encode_w_conv(*o.w).to(d), pos=o.pos.to(d), bias=o.bias.to(d), gamma=o.gamma.to(d), beta=o.beta.to(d),
                         dot_w=o.dot_w.to(d), dot_b=o.dot_b.to(d))
        Rp = rpad(o.R)
        self.gstride = pred_gstride(o.R)
        self.yp_bytes, self.dot_bytes, self.scratch_bytes = Rp * o.Nrow * 4, 2 * self.gstride * 4, Rp * o.N * 4
        self.kpart_bytes = pred_kpart_cap(o.form, o.chans, o.R) * 4

    def run(self, run, mt, set_option, yp=None):
        """-> (plan, {yp, dot, scratch, kpart: bytes on the CPU, with guard}, the planes buffer on the device)."""
        o = self.ops
        for k, v in pred_options(run, mt).items():
            set_option(k, v)
        yp = sentinel(self.yp_bytes) if yp is None else yp
        out = dict(yp=yp, dot=sentinel(self.dot_bytes), scratch=sentinel(self.scratch_bytes), kpart=sentinel(self.kpart_bytes))
        p = {k: t.data_ptr() for k, t in self.keep.items()}
        p.update(yp=yp.data_ptr(), dot_out=out["dot"].data_ptr(), scratch=out["scratch"].data_ptr(), kpart=out["kpart"].data_ptr())
        form = o.form if run in ("row", "sib", "sibk") else run
        plan = launch(pred_block(form, o.chans, o.k, o.R, p, split=run == "sibk"), pred_precision(o.variant))
        return plan, {k: t.cpu() for k, t in out.items()}, yp

    def heads(self, dot):
        """The bytes of the dot_out buffer -> fp32 [2, gstride]: group g's array in row g."""
        return dot[:self.dot_bytes].view(torch.float32).reshape(2, self.gstride)


def repack_weight(w, fmt):
    """fs2_op_repack_weight on fp32 [N, C, k] -> (image bytes, scale image bytes or None, kw), on the CPU."""
    from fastspeech2_amd import _lib
    L = _lib.lib()
    N, Cc, k = w.shape
    nimg = N * (Cc // 32 if fmt == "mx" else Cc // 64 + Cc // 128) * k * 128
    nsc = (N // 128) * (Cc // 128) * k * 1024 if fmt == "mx4" else 0
    wd = w.contiguous().to(_dev())
    img, sc = sentinel(nimg), sentinel(nsc)
    kw = C.c_int32(-999)
    with torch.cuda.device(_dev()):
        _lib.check(L.fs2_op_repack_weight(C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream), C.c_void_p(wd.data_ptr()), N, Cc, k,
                                          _lib.REPACK_MX4 if fmt == "mx4" else _lib.REPACK_MX, C.c_void_p(img.data_ptr()), nimg,
                                          C.c_void_p(sc.data_ptr()) if nsc else None, nsc, C.byref(kw)))
    torch.cuda.synchronize()
    assert untouched(img, nimg) and untouched(sc, nsc), "the repack wrote behind an image"
    return img[:nimg].cpu(), (sc[:nsc].cpu() if nsc else None), kw.value


class QkvCase:
    def __init__(self, ops):
        self.ops = ops
        d = _dev()
        self.keep = dict(x=encode_planes(*ops.x).to(d), w=encode_planes(*ops.w).to(d), pos=ops.pos.to(d), bias=ops.bias.to(d))
        self.Rvt = rpad(ops.R)
        self.qk_bytes, self.vt_bytes = self.Rvt * 2 * ops.D * 2, ops.D * self.Rvt * 2

    def run(self, kind, mt, split, set_option, out=None):
        """-> (plan, {qk_hi, qk_lo, vt_hi, vt_lo: bytes on the CPU, with guard}).  out: the caller's device buffers of the four planes (a consumer then reads what the
        launch left: tests/test_gpu_attn_kernels.py)."""
        for k, v in qkv_options(kind, mt, split).items():
            set_option(k, v)
        if out is None:
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
