"""Test-side statement of the row steps between the GEMMs of libfs2_hip (csrc/elementwise.h, csrc/varshort.h), launched one at a time through
fs2_op_launch_row_step (include/fs2.h): the ctypes mirrors of the library's argument blocks (csrc/row_step_args.h), the packed-row layout, operands whose values are
known exactly, the float64 reference of every step in plain numpy, the arithmetic of the two LayerNorm kernels stated in float32 (from which alone their bars are
set), the mutants, and the device side of the kernel-level tests.  The plane decoders and the sentinel helpers are tests/gemm_raw.py's.

Layout.  layout_rule.h's walk (row = gap; start = row rounded up to 8; row = start + len + gap; rows = row + 8) over five utterances: the frame rows (R = 285, no
multiple of 4, utterance 1 crosses row 128) and the token rows (103).  Utterance 0 stores three rows more than it has frames (padded-batch semantics: frame rows with
no token), utterance 2 has only zero durations (becomes all ones) and products that the ReLU of var_gather0 kills, utterance 3 is the low-variance one.

NaN stands wherever nothing may be read: the rows of P / hs of zero-duration tokens and of token gap rows, pe rows beyond the longest utterance, es / ps beyond
their stride and behind an utterance's end, e_rows / p_rows of gap rows, the table rows and bins no case selects.  Behind R, lri[R] and row_pos[R] / row_seq[R] hold
plausible live values that point at NaN rows.

CPU-only parts: tests/test_rowstep_host.py.  GPU parts (`Dev`): tests/test_gpu_rowstep_kernels.py."""
import ctypes as C

import numpy as np
import torch

from tests import gemm_raw as G
from tests.test_varshort_host import row_bound, short_dur, short_offset, up

VP, I32, F32 = C.c_void_p, C.c_int32, C.c_float
STEPS = ("embed", "dur_post", "lr_index", "lr_index_short", "lr_expand", "var_gather0", "var_embed", "dec_in_gather", "to_planes", "planes_to_rows")      # FS2_ROW_STEP_*


def _fields(spec):
    kinds = {"p": VP, "i": I32, "f": F32}
    return [(name, kinds[k]) for k, names in spec for name in names.split()]


class TokGatherArgs(C.Structure):
    """fs2::TokGatherArgs (csrc/row_step_args.h), field for field; tests/test_rowstep_host.py holds it against the compiled header."""
    _fields_ = _fields([("p", "P"), ("i", "ldp"), ("p", "tok_start lri row_pos row_seq"), ("i", "R chans"), ("p", "bias ln_g ln_b vp"), ("i", "col0 D"), ("p", "es ps"),
                        ("i", "es_stride ps_stride"), ("p", "e_rows p_rows ebins pbins"), ("i", "nb"), ("p", "TE TP qe_rows qp_rows f2s sqe sqp ln_g2 ln_b2 pe pe_alpha"),
                        ("f", "x_scale"), ("p", "x0 x0p srow_pos"), ("i", "Rs")])


class ShortLayoutArgs(C.Structure):
    _fields_ = _fields([("p", "cum scum"), ("i", "Tmax"), ("p", "ilen so32 row_pos row_seq vlen"), ("i", "R"), ("p", "ovf"), ("i", "B gap K Rs Rs_pad"),
                        ("p", "lri f2s sstart slen sdims srow_pos srow_seq slri")])


class RowStepArgs(C.Structure):
    _fields_ = _fields([("p", "row_pos row_seq"), ("i", "R"), ("p", "start vlen"), ("i", "B Tmax D"), ("p", "rows planes xs E"), ("i", "idim"), ("p", "pe pe_alpha"),
                        ("f", "x_scale"), ("p", "dlog_rows d_log d_int d_int2 ds cum olens olens32"), ("f", "alpha"), ("p", "scum so32"), ("i", "K"),
                        ("p", "src_rows tok_start ilen cum_in index_rows es ps"), ("i", "es_stride ps_stride"), ("p", "e_rows p_rows ebins pbins"), ("i", "nb"),
                        ("p", "Te Tp qe_rows qp_rows")])


BLOCK_OF = {"var_gather0": TokGatherArgs, "dec_in_gather": TokGatherArgs, "lr_index_short": ShortLayoutArgs}      # every other step: RowStepArgs

GAP, ALIGN, TAIL, ROW_TILE = 4, 8, 8, 128      # layout_rule.h: kMinGap, kAttAlign, kTailRows, kRowTile
K_SHORT = 5                                    # vs_window(2, 3)
NAN = float("nan")
F = np.float32
WIDTHS = [(128, 128), (256, 256), (1024, 384)]      # (chans of var_gather0, D of dec_in_gather) sharing one P: ldp = 6 chans + D
D_WIDTHS = (128, 256, 384)
EPS_VAR, EPS_DEC = 1e-12, 1e-5
X_SCALE, PE_ALPHA = 1.5, 0.75
NB = 15                                        # bin edges; the tables have NB + 1 rows
PRED_TOL = G.PRED_TOL                          # the model-level bar of the predictors: 1.5e-4 x max |reference|
PLANES_ROUNDING = 2.0 ** -16                   # attn_raw.PLANES_ROUNDING
U24 = 2.0 ** -24

# The CPU figures: the worst max-abs error, over the rows < R, of the float32 statement of the kernel's arithmetic (var_gather0_fp32 / dec_in_gather_fp32) against the
# float64 reference, per step and width; the bar is 8 x the figure (attn_raw.BAR's margin: the device's division, square root and contraction differ from numpy's).
# tests/test_rowstep_host.py recomputes them and requires recorded >= computed and <= 1.25 x computed; the GPU's figures never enter.
# Computed: var_gather0 1.178e-6 / 1.231e-6 / 1.462e-6 at 128 / 256 / 1024 channels; dec_in_gather 1.056e-6 / 1.211e-6 / 1.246e-6 at D = 128 / 256 / 384 (the worse of the
# per-frame and the teacher-forced route); max |reference| is 6.5 .. 7.5 throughout, so every bar is about 1e-5 against the model-level 1.5e-4 x 7 = 1e-3.
# For the record, the MI355X's figures (they enter nothing): dec_in_gather's fp32 rows 8.72e-7 / 1.08e-6 / 1.18e-6, 0.097 / 0.106 / 0.112 of the bar -- at D = 128 and 256
# the CPU statement's own max-abs to three digits; its planes 0.41 .. 0.43 of the bar with the planes' rounding; var_gather0, which leaves planes only, 0.40 / 0.42 / 0.41
# of that bar: its max-abs 3.1e-5 is the planes' rounding of |y| up to 7 (2^-17 |y|), 2.5 .. 3.1 x the fp32 bar alone, so through its only output the kernel is seen to
# about 3e-5, not 1e-5 -- still 30 x finer than the model-level bar.  embed_pe 0.49 .. 0.55 and bucket_embed 0.61 .. 0.62 of their derived bars.
CPU_FIGURE = {("var_gather0", 128): 1.25e-6, ("var_gather0", 256): 1.3e-6, ("var_gather0", 1024): 1.55e-6,
              ("dec_in_gather", 128): 1.12e-6, ("dec_in_gather", 256): 1.28e-6, ("dec_in_gather", 384): 1.32e-6}
BAR = {k: 8 * v for k, v in CPU_FIGURE.items()}


def walk(lens, gap=GAP):
    """layout_rule.h's row walk -> (starts, rows used)."""
    starts, row = [], gap
    for n in lens:
        s = up(row, ALIGN)
        starts.append(s)
        row = s + n + gap
    return starts, row + TAIL


def row_meta(starts, lens, R, extra=0):
    """row_pos / row_seq of R (+ extra) rows: -1 on every row that is no utterance's."""
    pos, seq = np.full(R + extra, -1, np.int32), np.full(R + extra, -1, np.int32)
    for b, (s, n) in enumerate(zip(starts, lens)):
        pos[s:s + n] = np.arange(n)
        seq[s:s + n] = b
    return pos, seq


# ------------------------------------------------------------------ durations (dur.post)
DUR_MAX = 2 ** 31 - 1      # elementwise.h: kDurMax -- a duration, and an utterance's frame count, beyond the int range saturates there


def scaled_duration(d, alpha):
    """elementwise.h: scaled_duration -- round_half_even(float(d) * alpha) in fp32 when alpha != 1, negatives are zero, the int range saturates."""
    if d <= 0:
        return 0
    if F(alpha) == F(1):
        return min(int(d), DUR_MAX)
    f = np.rint(F(d) * F(alpha))
    return min(int(f), DUR_MAX) if f > 0 else 0


def ref_scan(ds, ilens, alpha, K=K_SHORT):
    """length_regulator.py:57-60,85-88 per utterance -> (used durations, cum, scum, frame counts, short frame counts); an all-zero utterance becomes all ones."""
    used, cum, scum, olens, so = [], [], [], [], []
    for b, T in enumerate(ilens):
        d = [scaled_duration(int(ds[b][t]), alpha) for t in range(T)]
        if sum(d) == 0:
            d = [1] * T
        c, sc, run, run2 = [], [], 0, 0
        for t in range(T):
            run += d[t]
            run2 += short_dur(d[t], K)
            c.append(run)
            sc.append(run2)
        used.append(d); cum.append(c); scum.append(sc); olens.append(min(run, DUR_MAX)); so.append(run2)
    return used, cum, scum, olens, so


def ref_duration(y):
    """duration_predictor.py:77-81 in float64: clamp(round_half_even(exp(y) - 1), 0)."""
    return int(max(np.rint(np.exp(np.float64(y)) - 1.0), 0.0))


class DurOperands:
    """dur.post: token counts around the 256-token passes of dur_scan, Tmax = 300."""
    Tmax, idim = 300, 40
    ilens = [1, 255, 256, 257, 300, 40, 7, 30, 20, 20]
    ALPHAS = (1.0, 0.5, 1.3)
    POISON = 1000                                  # durations behind an utterance's end: never scanned

    def __init__(self):
        rs = np.random.RandomState(41)
        B, T = len(self.ilens), self.Tmax
        self.B = B
        ds = np.full((B, T), self.POISON, np.int64)
        for b, n in enumerate(self.ilens):
            ds[b, :n] = rs.randint(0, 10, size=n)
        ds[5, :40] = rs.randint(1, 10, size=40)
        ds[5, [0, 1, 17, 18, 19, 38, 39]] = 0      # zeros at both edges and adjacent
        ds[5, 7] = 12                              # longer than K
        ds[6, :7] = 0                              # all zero: becomes all ones
        ds[7, 3] = -4                              # a negative duration counts as zero
        ds[4, 255] = 0; ds[4, 256] = 9             # around the carry between the passes
        self.ds = ds
        xs = rs.randint(0, self.idim, size=(B, T)).astype(np.int64)
        xs[8, 5] = self.idim                       # an id outside [0, idim) inside the utterance
        xs[9, 250] = -1                            # ... and in the padding only
        self.xs, self.bad = xs, [b in (8, 9) for b in range(B)]
        self.start, self.Rtok = walk(self.ilens)
        # log-durations whose exp(y) - 1 = n + delta stays 0.2 from a half-integer; a few far below zero
        dlog = np.full(self.Rtok + 8, NAN, np.float32)
        self.y = []
        for b, n in enumerate(self.ilens):
            val = rs.randint(0, 10, size=n) + rs.uniform(-0.3, 0.3, size=n)
            y = np.log(np.maximum(1.0 + val, 1e-3)).astype(np.float32)
            y[::11] = F(-3.0)
            dlog[self.start[b]:self.start[b] + n] = y
            self.y.append(y)
        self.dlog_rows = dlog
        self.d_log = np.zeros((B, T), np.float32)
        self.d_int = np.zeros((B, T), np.int64)
        for b, n in enumerate(self.ilens):
            self.d_log[b, :n] = self.y[b]
            self.d_int[b, :n] = [ref_duration(v) for v in self.y[b]]

    def expected(self, ds, alpha):
        """-> dict of the scan's outputs; cum / scum hold None where nothing is written (t >= ilen)."""
        used, cum, scum, olens, so = ref_scan(ds, self.ilens, alpha)
        return dict(used=used, cum=cum, scum=scum, olens=[-1 if bad else n for bad, n in zip(self.bad, olens)], so=so)


# ------------------------------------------------------------------ the frame-level batch
def bucket(x, bins):
    """torch.bucketize(x, bins, right=False): the first i with x <= bins[i]; NaN -> len(bins)."""
    for i in range(len(bins)):
        if x <= bins[i]:
            return i
    return len(bins)


def bucket_right(x, bins):
    """the mutant: right=True, the first i with x < bins[i]."""
    for i in range(len(bins)):
        if x < bins[i]:
            return i
    return len(bins)


class Batch:
    """Five utterances: durations, both layouts, the scan, the index, the short layout -- integers only, shared by every width."""
    Tmax = 24
    ilens = [9, 20, 3, 14, 11]
    EXTRA = [3, 0, 0, 0, 0]                      # rows stored beyond the frames (padded-batch semantics)
    KILLED, QUIET = 2, 3                         # the utterance the ReLU kills; the low-variance one

    def __init__(self):
        rs = np.random.RandomState(7)
        B, T = len(self.ilens), self.Tmax
        self.B = B
        ds = np.full((B, T), 1000, np.int64)
        ds[0, :9] = [0, 0, 3, 5, 0, 0, 12, 6, 0]
        ds[1, :20] = [4, 7, 0, 9, 2, 5, 5, 0, 0, 8, 3, 6, 1, 9, 4, 7, 2, 6, 5, 4]
        ds[2, :3] = 0
        ds[3, :14] = [3, 0, 6, 2, 8, 1, 1, 4, 0, 5, 7, 2, 3, 6]
        ds[4, :11] = [2, 40, 1, 0, 3, 5, 0, 2, 6, 1, 5]
        self.ds = ds
        self.used, self.cum, self.scum, self.vlen, self.so = ref_scan(ds, self.ilens, 1.0)
        self.len = [v + e for v, e in zip(self.vlen, self.EXTRA)]
        self.start, self.R = walk(self.len)
        self.tok_start, self.Rtok = walk(self.ilens)
        assert self.R % 4 != 0 and self.Rtok % 4 != 0
        assert any(s < 128 < s + n for s, n in zip(self.start, self.len)), "no utterance crosses row 128"
        self.TRAP = 8                                # entries behind R
        self.row_pos, self.row_seq = row_meta(self.start, self.len, self.R, self.TRAP)
        self.tok_pos, self.tok_seq = row_meta(self.tok_start, self.ilens, self.Rtok, self.TRAP)
        # tokens nothing may read: zero duration (except where the whole utterance became ones)
        self.dead_tok = np.ones(self.Rtok, bool)
        for b in range(B):
            for t in range(self.ilens[b]):
                self.dead_tok[self.tok_start[b] + t] = self.used[b][t] == 0
        self.lri = self.ref_lri()
        # the trap behind R: a live-looking row of utterance 1 whose token (index 2, duration 0) is a NaN row
        self.row_pos[self.R], self.row_seq[self.R] = 2, 1
        self.lri_in = np.concatenate([self.lri, np.full(self.TRAP, -1, np.int32)])
        self.lri_in[self.R] = 2
        assert self.dead_tok[self.tok_start[1] + 2]
        self.short = self.ref_short()
        self.Lmax = max(self.len)

    def cum_padded(self, which):
        out = np.full((self.B, self.Tmax), 10 ** 6, np.int32)      # behind ilen: never searched
        for b, c in enumerate(which):
            out[b, :len(c)] = c
        return out

    def ref_lri(self):
        """The token of every frame row: the first i with cum[b, i] > j; -1 for gap rows and for rows beyond the utterance's frames."""
        lri = np.full(self.R, -1, np.int32)
        for row in range(self.R):
            b, j = self.row_seq[row], self.row_pos[row]
            if b < 0 or j < 0 or j >= self.vlen[b]:
                continue
            lri[row] = next(i for i in range(self.ilens[b]) if self.cum[b][i] > j)
        return lri

    def ref_short(self):
        """layout_rule.h's short layout as tests/test_varshort_host.py states it: the row walk over the short lengths, the token of every short row, the short row of
        every frame."""
        K = K_SHORT
        sstart, rows = walk(self.so)
        Rs = min(row_bound(min(self.R, K * sum(self.ilens)), self.B), self.R)
        Rs_pad = up(Rs, ROW_TILE)
        assert rows <= Rs
        spos, sseq = row_meta(sstart, self.so, Rs_pad)
        slri = np.full(Rs_pad, -1, np.int32)
        for row in range(Rs_pad):
            if spos[row] >= 0:
                b = sseq[row]
                slri[row] = next(i for i in range(self.ilens[b]) if self.scum[b][i] > spos[row])
        f2s = np.full(self.R, -1, np.int32)
        for row in range(self.R):
            tk = self.lri[row]
            if tk >= 0:
                b, j = self.row_seq[row], self.row_pos[row]
                c0 = self.cum[b][tk - 1] if tk else 0
                s0 = self.scum[b][tk - 1] if tk else 0
                f2s[row] = sstart[b] + s0 + short_offset(j - c0, self.cum[b][tk] - c0, K)
        return dict(sstart=sstart, slen=list(self.so), rows=rows, Rs=Rs, Rs_pad=Rs_pad, srow_pos=spos, srow_seq=sseq, slri=slri, f2s=f2s)


_batch = None


def batch():
    global _batch
    if _batch is None:
        _batch = Batch()
    return _batch


def _u(rs, *shape, scale=1.0):
    return rs.uniform(-scale, scale, size=shape).astype(np.float32)


class Operands:
    """The float operands of one (chans, D) pair over the batch."""

    def __init__(self, chans, D):
        bt = self.bt = batch()
        self.chans, self.D = chans, D
        rs = np.random.RandomState(chans * 7 + D)
        N, R, Rtok = chans, bt.R, bt.Rtok
        self.ldp, self.col0 = 6 * N + D, 6 * N
        P = _u(rs, Rtok, self.ldp)
        q0, q1 = bt.tok_start[Batch.QUIET], bt.tok_start[Batch.QUIET] + bt.ilens[Batch.QUIET]
        P[q0:q1] *= F(0.1)                                         # the low-variance utterance
        k0, k1 = bt.tok_start[Batch.KILLED], bt.tok_start[Batch.KILLED] + bt.ilens[Batch.KILLED]
        P[k0:k1, :6 * N] = -(np.abs(P[k0:k1, :6 * N]) + F(1))      # every tap sum below -3 + |bias|: the ReLU kills the rows
        P[bt.dead_tok] = NAN
        self.P = P
        self.bias, self.ln_g, self.ln_b = _u(rs, 2 * N, scale=0.1), (F(1) + _u(rs, 2 * N, scale=0.5)), _u(rs, 2 * N, scale=0.5)
        self.ln_g2, self.ln_b2 = (F(1) + _u(rs, D, scale=0.5)), _u(rs, D, scale=0.5)
        # bins: exact quarters for energy (0.0 is an edge), fifths rounded to fp32 for pitch
        self.ebins = (np.arange(NB) * 0.25 - 1.75).astype(np.float32)
        self.pbins = (np.arange(NB) * 0.2 - 1.4).astype(np.float32)
        TE, TP = _u(rs, NB + 1, D), _u(rs, NB + 1, D)
        TE[:4] *= F(0.1); TP[:4] *= F(0.1)                         # the bins the low-variance utterance lands in
        # the predictions per SHORT row (the FS2_VARSHORT route); a frame takes its short row's
        sh = bt.short
        se, sp = np.full(sh["Rs_pad"], NAN, np.float32), np.full(sh["Rs_pad"], NAN, np.float32)
        live = np.nonzero(sh["srow_pos"] >= 0)[0]
        se[live], sp[live] = _u(rs, len(live), scale=2.0), _u(rs, len(live), scale=2.0)
        se[(se > self.ebins[9]) & (se <= self.ebins[10])] -= F(0.25)      # nobody selects energy bin 10 or pitch bin 12: those table rows are NaN
        sp[(sp > self.pbins[11]) & (sp <= self.pbins[12])] -= F(0.25)
        quiet = live[sh["srow_seq"][live] == Batch.QUIET]
        se[quiet], sp[quiet] = rs.uniform(-2.5, -1.01, len(quiet)).astype(np.float32), rs.uniform(-2.0, -0.81, len(quiet)).astype(np.float32)
        other = [r for r in live if sh["srow_seq"][r] in (1, 4)]
        e3, p5 = self.ebins[3], self.pbins[5]
        specials = [(e3, p5), (np.nextafter(e3, F(9)), np.nextafter(p5, F(9))), (np.nextafter(e3, F(-9)), np.nextafter(p5, F(-9))), (F(-9.0), F(9.0)), (F(9.0), F(-9.0)),
                    (F(-0.0), F(0.0)), (F(np.inf), F(-np.inf)), (F(-np.inf), F(np.inf)), (F(NAN), F(0.3)), (F(0.3), F(NAN)), (self.ebins[0], self.pbins[NB - 1]),
                    (self.ebins[NB - 1], self.pbins[0])]
        self.special_rows = other[3:3 + 4 * len(specials):4]
        for r, (e, p) in zip(self.special_rows, specials):
            se[r], sp[r] = e, p
        self.se, self.sp = se, sp
        # ... per frame: the short row's value; a live frame without a short row reads 0 (dec_in_gather's rule under FS2_VARSHORT)
        self.f2s = sh["f2s"].copy()
        self.forced = bt.start[1] + 30                             # a live frame whose short row the test takes away
        self.f2s[self.forced] = -1
        e_rows, p_rows = np.full(R + bt.TRAP, NAN, np.float32), np.full(R + bt.TRAP, NAN, np.float32)
        for row in range(R):
            if bt.row_pos[row] >= 0:
                s = self.f2s[row]
                e_rows[row], p_rows[row] = (se[s], sp[s]) if s >= 0 else (F(0), F(0))
        self.e_rows, self.p_rows = e_rows, p_rows
        # teacher forcing: es shorter than the longest utterance (positions behind the stride read 0), ps longer; NaN behind every utterance's end and behind the array
        self.es_stride, self.ps_stride = 60, 120
        self.es, self.ps = np.full(bt.B * 60 + 64, NAN, np.float32), np.full(bt.B * 120 + 64, NAN, np.float32)
        for b in range(bt.B):
            n = bt.len[b]
            rows = slice(bt.start[b], bt.start[b] + n)
            self.es[b * 60:b * 60 + min(n, 60)] = e_rows[rows][:60]
            self.ps[b * 120:b * 120 + n] = p_rows[rows]
        self.e_teacher, self.p_teacher = e_rows.copy(), p_rows.copy()
        for row in range(R):
            if bt.row_pos[row] >= 60:
                self.e_teacher[row] = 0.0
        # the searched indices per route, and NaN in every table row no case selects
        self.q = {"rows": self.search(e_rows, p_rows), "teacher": self.search(self.e_teacher, p_rows)}
        used_e = set(self.q["rows"][0][self.q["rows"][0] >= 0]) | set(self.q["teacher"][0][self.q["teacher"][0] >= 0])
        used_p = set(self.q["rows"][1][self.q["rows"][1] >= 0])
        for i in range(NB + 1):
            if i not in used_e:
                TE[i] = NAN
            if i not in used_p:
                TP[i] = NAN
        self.TE, self.TP = TE, TP
        # positional table: the oracle's, NaN beyond the longest utterance
        from oracle import fs2_oracle as O
        pe = np.full((bt.Lmax + 8, D), NAN, np.float32)
        pe[:bt.Lmax] = O.positional_table(bt.Lmax, D).numpy()
        self.pe = pe

    def search(self, e_rows, p_rows, right=False):
        bt, fn = self.bt, (bucket_right if right else bucket)
        qe, qp = np.full(bt.R, -1, np.int32), np.full(bt.R, -1, np.int32)
        for row in range(bt.R):
            if bt.row_pos[row] >= 0:
                qe[row], qp[row] = fn(e_rows[row], self.ebins), fn(p_rows[row], self.pbins)
        return qe, qp

    def short_search(self):
        """var_bucket_short: the indices per short row, -1 on gap rows (rows < Rs)."""
        sh = self.bt.short
        sqe, sqp = np.full(sh["Rs"], -1, np.int32), np.full(sh["Rs"], -1, np.int32)
        for r in range(sh["Rs"]):
            if sh["srow_pos"][r] >= 0:
                sqe[r], sqp[r] = bucket(self.se[r], self.ebins), bucket(self.sp[r], self.pbins)
        return sqe, sqp


_ops = {}


def operands(chans, D):
    if (chans, D) not in _ops:
        _ops[(chans, D)] = Operands(chans, D)
    return _ops[(chans, D)]


def padded_width(N):
    """What the 64 lanes x 4 channels passes of the two LayerNorm kernels cover."""
    return up(N, 256)


# ------------------------------------------------------------------ float64 references (and mutants: one changed line each)
MUTANTS = {"var_gather0": ("eps_swapped", "mean_over_padded_width", "bias_after_relu", "taps_reversed", "neighbour_across_gap", "lo_plane_dropped"),
           "dec_in_gather": ("eps_swapped", "mean_over_padded_width", "tp_te_swapped", "scale_before_relu", "pe_of_row_not_position", "lo_plane_dropped", "bucket_right_true")}


def _hi_only(v):
    return torch.from_numpy(np.ascontiguousarray(v)).float().bfloat16().double().numpy()


def _neighbour_token_row(bt, r, d):
    """P row the frame row r contributes as a neighbour; mutant neighbour_across_gap (d = -1 / +1: the side): a gap row hands on the adjacent utterance's token."""
    while 0 <= r < bt.R and bt.row_pos[r] < 0:
        r += d
    if not (0 <= r < bt.R) or bt.lri[r] < 0:
        return -1
    return bt.tok_start[bt.row_seq[r]] + bt.lri[r]


def ref_var_gather0(ops, mutant=None):
    """y[row, g N + c] = LayerNorm_1e-12(relu(sum_d P[tok(row + d - 1), d 2N + g N + c] + bias[g N + c])) per predictor g, a neighbour without token contributing
    zero; rows that are no frame are zero.  -> float64 [R, 2 N]"""
    bt, N, P = ops.bt, ops.chans, ops.P.astype(np.float64)
    bias, g, b = ops.bias.astype(np.float64), ops.ln_g.astype(np.float64), ops.ln_b.astype(np.float64)
    eps = EPS_DEC if mutant == "eps_swapped" else EPS_VAR
    out = np.zeros((bt.R, 2 * N))
    for row in range(bt.R):
        if bt.row_pos[row] < 0:
            continue
        t0 = bt.tok_start[bt.row_seq[row]]
        for grp in range(2):
            ch = slice(grp * N, (grp + 1) * N)                    # (for c in range(N): one slice statement per channel loop)
            y = np.zeros(N)
            for d in range(3):
                r = row + d - 1
                tk = bt.lri_in[r] if 0 <= r < bt.R else -1
                src = t0 + tk if tk >= 0 else -1
                if mutant == "neighbour_across_gap" and d != 1 and 0 <= r < bt.R and bt.row_pos[r] < 0:
                    src = _neighbour_token_row(bt, r, d - 1)
                tap = 2 - d if mutant == "taps_reversed" else d
                if src >= 0:
                    y = y + P[src, tap * 2 * N + grp * N:tap * 2 * N + (grp + 1) * N]
            y = np.maximum(y, 0.0) + bias[ch] if mutant == "bias_after_relu" else np.maximum(y + bias[ch], 0.0)
            mean = y.sum() / (padded_width(N) if mutant == "mean_over_padded_width" else N)
            var = ((y - mean) ** 2).sum() / N
            out[row, ch] = (y - mean) / np.sqrt(var + eps) * g[ch] + b[ch]
    return _hi_only(out) if mutant == "lo_plane_dropped" else out


def ref_dec_in_gather(ops, route="rows", mutant=None):
    """x[row, c] = relu(LayerNorm_1e-5((P[tok(row), col0 + c] + TP[qp, c]) + TE[qe, c])) x_scale + alpha pe[pos(row), c]; a frame row without token has a zero first
    term; rows that are no frame are zero.  -> (float64 [R, D], qe, qp)"""
    bt, D, P = ops.bt, ops.D, ops.P.astype(np.float64)
    TE, TP, pe = ops.TE.astype(np.float64), ops.TP.astype(np.float64), ops.pe.astype(np.float64)
    g, b = ops.ln_g2.astype(np.float64), ops.ln_b2.astype(np.float64)
    e_rows = ops.e_teacher if route == "teacher" else ops.e_rows
    qe, qp = ops.search(e_rows, ops.p_rows, right=mutant == "bucket_right_true")
    eps = EPS_VAR if mutant == "eps_swapped" else EPS_DEC
    out = np.zeros((bt.R, D))
    for row in range(bt.R):
        pos = bt.row_pos[row]
        if pos < 0:
            continue
        tk = bt.lri_in[row]
        first = P[bt.tok_start[bt.row_seq[row]] + tk, ops.col0:ops.col0 + D] if tk >= 0 else np.zeros(D)
        ie, ip = (qp[row], qe[row]) if mutant == "tp_te_swapped" else (qe[row], qp[row])
        y = (first + TP[ip]) + TE[ie]                                 # (for c in range(D))
        mean = y.sum() / (padded_width(D) if mutant == "mean_over_padded_width" else D)
        var = ((y - mean) ** 2).sum() / D
        ln = (y - mean) / np.sqrt(var + eps) * g + b
        prow = row if mutant == "pe_of_row_not_position" else pos
        pv = pe[prow] if prow < pe.shape[0] else np.full(D, NAN)
        out[row] = np.maximum(ln * X_SCALE + PE_ALPHA * pv, 0.0) if mutant == "scale_before_relu" else np.maximum(ln, 0.0) * X_SCALE + PE_ALPHA * pv
    return (_hi_only(out) if mutant == "lo_plane_dropped" else out), qe, qp


def ref_lr_expand(bt, hs):
    """out[row, c] = hs[tok_start[b] + index[row], c]; rows without token are zero."""
    out = np.zeros((bt.R, hs.shape[1]), hs.dtype)
    for row in range(bt.R):
        if bt.lri[row] >= 0:
            out[row] = hs[bt.tok_start[bt.row_seq[row]] + bt.lri[row]]      # (for c in range(D))
    return out


def ref_embed(bt, xs, E, pe, idim, x_scale=X_SCALE, alpha=PE_ALPHA):
    """h[row, c] = E[xs[b, t], c] x_scale + alpha pe[t, c] over the TOKEN rows; an id outside [0, idim) reads row 0.  -> (float64 [Rtok, D], the two terms' magnitudes)"""
    D = E.shape[1]
    out, mag = np.zeros((bt.Rtok, D)), np.zeros((bt.Rtok, D))
    for row in range(bt.Rtok):
        t = bt.tok_pos[row]
        if t < 0:
            continue
        i = int(xs[bt.tok_seq[row], t])
        i = i if 0 <= i < idim else 0
        a, p = E[i].astype(np.float64) * x_scale, alpha * pe[t].astype(np.float64)      # (for c in range(D))
        out[row], mag[row] = a + p, np.abs(a) + np.abs(p)
    return out, mag


def ref_bucket_embed(ops, h, Te, Tp, route="rows"):
    """h[row, c] = (h[row, c] + Tp[qp, c]) + Te[qe, c] on the frame rows; every other row stays.  -> (float64 [R, D], magnitudes, qe, qp)"""
    bt = ops.bt
    qe, qp = ops.q[route]
    out, mag = h.astype(np.float64).copy(), np.zeros(h.shape)
    for row in range(bt.R):
        if bt.row_pos[row] >= 0:
            a, p, e = h[row].astype(np.float64), Tp[qp[row]].astype(np.float64), Te[qe[row]].astype(np.float64)      # (for c in range(D))
            out[row], mag[row] = (a + p) + e, np.abs(a) + np.abs(p) + np.abs(e)
    return out, mag, qe, qp


# ------------------------------------------------------------------ the LayerNorm kernels' arithmetic in float32
def _lane_sum(v4):
    """[rows, 4 passes, 64 lanes, 4] fp32 -> the wave's sum as the kernels form it: per lane ((x + y) + (z + w)) pass after pass, then the xor butterfly 32 .. 1."""
    s = np.zeros(v4.shape[:1] + (64,), np.float32)
    for j in range(4):
        s = s + ((v4[:, j, :, 0] + v4[:, j, :, 1]) + (v4[:, j, :, 2] + v4[:, j, :, 3]))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def ln_fp32(v, eps):
    """v [rows, N] fp32 (N <= 1024) -> ((v - mean) rstd, fp32) with the kernels' sums: channel c = 256 j + 4 lane + k, channels >= N absent."""
    rows, N = v.shape
    pad = np.zeros((rows, 1024), np.float32)
    pad[:, :N] = v
    mean = _lane_sum(pad.reshape(rows, 4, 64, 4)) / F(N)
    dx = np.zeros((rows, 1024), np.float32)
    dx[:, :N] = v - mean[:, None]
    q = _lane_sum((dx * dx).reshape(rows, 4, 64, 4))
    rstd = F(1) / np.sqrt(q / F(N) + F(eps))
    return (v - mean[:, None]) * rstd[:, None]


def var_gather0_fp32(ops):
    """var_gather0 in fp32, operation for operation (no contraction) -> float64 [R, 2 N] of the fp32 values the planes split."""
    bt, N, P = ops.bt, ops.chans, ops.P
    live = np.nonzero(bt.row_pos[:bt.R] >= 0)[0]
    out = np.zeros((bt.R, 2 * N), np.float32)
    for grp in range(2):
        v = np.zeros((len(live), N), np.float32)
        for d in range(3):
            for i, row in enumerate(live):
                r = row + d - 1
                tk = bt.lri_in[r] if 0 <= r < bt.R else -1
                if tk >= 0:
                    v[i] = v[i] + P[bt.tok_start[bt.row_seq[row]] + tk, d * 2 * N + grp * N:d * 2 * N + (grp + 1) * N]
        v = np.maximum(v + ops.bias[grp * N:(grp + 1) * N], F(0))
        out[live, grp * N:(grp + 1) * N] = ln_fp32(v, EPS_VAR) * ops.ln_g[grp * N:(grp + 1) * N] + ops.ln_b[grp * N:(grp + 1) * N]
    return out.astype(np.float64)


def dec_in_gather_fp32(ops, route="rows"):
    bt, D = ops.bt, ops.D
    qe, qp = ops.q[route]
    live = np.nonzero(bt.row_pos[:bt.R] >= 0)[0]
    v = np.zeros((len(live), D), np.float32)
    for i, row in enumerate(live):
        tk = bt.lri_in[row]
        if tk >= 0:
            v[i] = ops.P[bt.tok_start[bt.row_seq[row]] + tk, ops.col0:ops.col0 + D]
        v[i] = (v[i] + ops.TP[qp[row]]) + ops.TE[qe[row]]
    ln = ln_fp32(v, EPS_DEC) * ops.ln_g2 + ops.ln_b2
    out = np.zeros((bt.R, D), np.float32)
    out[live] = np.maximum(ln, F(0)) * F(X_SCALE) + F(PE_ALPHA) * ops.pe[bt.row_pos[live]]
    return out.astype(np.float64)


def planes_bar(key, ref):
    """The bar where the output is planes: the step's bar plus the planes' own rounding of the value (attn_raw.planes_bar)."""
    return BAR[key] + PLANES_ROUNDING * (np.abs(ref) + BAR[key])


def split_planes(rows32):
    """fp32 [rows, C] -> the (hi, lo) bf16 bit patterns (int16) the kernels' store_planes4 writes: hi = bf16(v), lo = bf16(v - hi), round to nearest even."""
    hi, lo = G.split_bf16(torch.from_numpy(np.ascontiguousarray(rows32)).float())
    return hi.view(torch.int16).numpy(), lo.view(torch.int16).numpy()


# ------------------------------------------------------------------ device side
class Dev:
    """Uploads, sentinel outputs and launches of one test module; every output buffer carries gemm_raw.GUARD sentinel bytes behind it."""

    def __init__(self):
        from fastspeech2_amd import _lib
        self._lib, self.keep = _lib, []

    def up(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(G._dev())
        self.keep.append(t)
        return t

    @staticmethod
    def out(nbytes):
        return G.sentinel(nbytes)

    def launch(self, step, block, size=None):
        L = self._lib.lib()
        with torch.cuda.device(G._dev()):
            rc = L.fs2_op_launch_row_step(C.c_void_p(torch.cuda.current_stream(G._dev()).cuda_stream), STEPS.index(step) if isinstance(step, str) else step,
                                          C.byref(block) if block is not None else None, C.sizeof(block) if size is None else size)
        torch.cuda.synchronize()
        return rc


def ptr(t):
    return t.data_ptr() if t is not None else None


def view(buf, dtype, n):
    """The first n elements of a sentinel buffer's bytes (CPU) as dtype."""
    t = buf.cpu()
    size = torch.empty(0, dtype=dtype).element_size()
    return t[:n * size].view(dtype).numpy().copy()
