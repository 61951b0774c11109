"""The fixed sweep of inputs behind tests/golden/record_ops_workspace_parent.json: what the five fs2_op_*_workspace_bytes queries of the
record operators (csrc/record_op.h) are asked in tests/test_record_op_host.py.  The answers in the golden file were recorded, through
the stand-in, from the commit before the operators shared their workspace carve; the walk that replaced the four hand-written layouts
has to give the same number for every input, the 0 of a refused one included.

A case is (op, B, a_lens, b_lens, cap): lens None = a null pointer; b_lens and cap are the pair operators' only."""
import struct

import numpy as np

OPS = ("targets", "losses", "dtw", "align", "pitch_path")
LENS = (0, 1, 31, 32, 33, 255, 256, 257, 5000)
BS = (0, 1, 2, 3, 95, 96, 97, 128, 129, 250, 251, 257, 499, 500, 501, 600)
PAIR_BS = (0, 1, 2, 5, 96, 97, 200, 600)
CAPS = (0, 1 << 12, 1 << 20, 1 << 26, 1 << 32, 1 << 62)      # below `largest`, between `largest` and `all`, above `all`, batch by batch
INT32_MAX = 2 ** 31 - 1


def _mixes(B, seed, n):
    rng = np.random.RandomState(seed)
    return [[int(v) for v in rng.choice(LENS, size=B)] for _ in range(n)]


def cases():
    out = [("targets", B, None, None, 0) for B in list(range(-3, 600, 3)) + [500, 501, 600]]
    for op in ("losses", "pitch_path"):
        for B in BS:
            for lens in [[v] * B for v in LENS] + _mixes(B, 7 * B + 1, 3):
                out.append((op, B, lens, None, 0))
        out += [(op, -1, [1], None, 0), (op, 1, None, None, 0), (op, 1, [-1], None, 0), (op, 3, [5, -2, 5], None, 0), (op, 0, None, None, 0),
                (op, 600, [5000] * 599 + [-1], None, 0), (op, 2, [INT32_MAX, INT32_MAX], None, 0)]
    for op in ("dtw", "align"):
        for B in PAIR_BS:
            for k, (al, bl) in enumerate([([257] * B, [33] * B), ([33] * B, [257] * B), ([5000] * B, [5000] * B), ([0] * B, [256] * B)]
                                         + list(zip(_mixes(B, 11 * B + 2, 2), _mixes(B, 13 * B + 3, 2)))):
                for cap in CAPS:
                    out.append((op, B, al, bl, cap))
        out += [(op, -1, [1], [1], 0), (op, 1, None, [1], 0), (op, 1, [1], None, 0), (op, 1, [-1], [1], 0), (op, 1, [1], [-1], 1 << 62),
                (op, 1, [INT32_MAX], [INT32_MAX], 0), (op, 0, None, None, 0), (op, 0, None, None, 1 << 62), (op, 2, [1 << 20, 3], [1 << 20, 3], 0),
                (op, 2, [(1 << 20) + 1, 3], [1 << 20, 3], 0)]
    return out


def pack(cs):
    """The stand-in's input (record_op_main --workspace IN): int32 count; per case int32 op, B, nulls (bit 0: a_lens, bit 1: b_lens),
    n (lengths per side), uint64 cap, int32 a_lens[n], b_lens[n]."""
    raw = [struct.pack("i", len(cs))]
    for op, B, al, bl, cap in cs:
        pair = op in ("dtw", "align")
        nulls = (al is None) | ((bl is None and pair) << 1)
        n = max(len(al or []), len(bl or []))
        a = list(al or []) + [0] * (n - len(al or []))
        b = list(bl or []) + [0] * (n - len(bl or []))
        raw.append(struct.pack("iiiiQ", OPS.index(op), B, nulls, n, cap))
        raw.append(np.asarray(a + b, np.int32).tobytes())
    return b"".join(raw)
