"""Every vocoder entry point (include/fs2.h: 10 calls, 10 workspace queries) keeps, for the calls that end before a launch, its return
code AND the text of fs2_last_error: the record profiles/vocoder_refusals_parent.json was taken with this case list from the library
before the host path was folded into one call description (csrc/griffin_lim_host.h), so a check that moved, merged or changed its
wording shows here by name.  Needs no GPU: every call passes a workspace below what it needs (or none), the last thing each path
checks, so one that slipped past the check it is here for ends with FS2_ERR_WORKSPACE and launches nothing.

``python tests/test_vocoder_refusals_host.py --record`` rewrites the record from the library it finds (for a look at what changed;
the committed record stays the parent's)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_mel_gl_host as M              # noqa: E402
from tests import test_vocoder_async_host as A       # noqa: E402

RECORD = os.path.join(ROOT, "profiles", "vocoder_refusals_parent.json")
PTR, DEFAULT_G = A.PTR, A.DEFAULT_G
BAD_G = (1000, 256, 1000, 80)
SENTINEL = "fs2_op_bucketize: bad arguments"          # left by _mark(): the text of a case that failed without a message of its own


@pytest.fixture(scope="module")
def lib():
    from fastspeech2_amd import _lib
    _lib.build()
    return _lib.lib()


def _i32s(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def _spsi_host(g=DEFAULT_G, src=PTR, width=80, pinv=PTR, B=None, lens=(10, 5), ws=PTR, ws_bytes=0, phase=PTR):
    B = (0 if lens is None else len(lens)) if B is None else B
    starts = None if lens is None else np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    return "fs2_op_spsi_phase_geom", (None,) + tuple(g) + (src, width, pinv, B, _i32s(starts), _i32s(lens), ws, ws_bytes, phase, None)


def _spsi_dev(g=DEFAULT_G, src=PTR, width=80, pinv=PTR, B=2, lens_dev=PTR, src_stride=0, frame_capacity=15, ws=PTR, ws_bytes=0, phase=PTR):
    return "fs2_op_spsi_phase_dev", (None,) + tuple(g) + (src, width, pinv, B, lens_dev, src_stride, frame_capacity, None, ws, ws_bytes, phase, None)


def _spsi_cases(lib):
    """Both forms of fs2_op_spsi_phase_* with the faults of the synthesis lists (those that exist for a call without iterations, a wav
    or a status)."""
    h, d = _spsi_host, _spsi_dev
    need = int(lib.fs2_op_spsi_workspace_bytes_geom(*DEFAULT_G, 2, _i32s((10, 5))))
    need_d = int(lib.fs2_op_spsi_workspace_bytes_cap(*DEFAULT_G, 2, 15))
    for e, c, nd in (("spsi host", h, need), ("spsi dev", d, need_d)):
        yield ("src_width", e) + c(width=100)
        yield ("src_width of another geometry's bins", e) + c(width=1025)
        yield ("mel without pinv", e) + c(pinv=None)
        yield ("null src", e) + c(src=None)
        yield ("null phase", e) + c(phase=None)
        yield ("null workspace", e) + c(ws=None)
        yield ("workspace one byte short", e) + c(ws_bytes=nd - 1)
        yield ("linear input needs no pinv", e) + c(width=513, pinv=None)
        for bad in ((1000, 256, 1000, 80), (1024, 100, 1024, 80), (1024, 512, 256, 80), (1024, 256, 2048, 80), (1024, 256, 1024, 129)):
            yield ("geometry %s" % (bad,), e) + c(g=bad, src=None, pinv=None, ws=None)
    yield ("null starts / lens", "spsi host") + h(lens=None, B=2)
    yield ("negative length", "spsi host") + h(lens=(10, -1))
    yield ("B < 0", "spsi host") + h(lens=None, B=-1)
    yield ("B = 0", "spsi host") + h(lens=None, src=None, phase=None, ws=None)
    yield ("no frames", "spsi host") + h(lens=(0, 0), src=None, phase=None, ws=None)
    yield ("B = 0", "spsi dev") + d(B=0)
    yield ("frame_capacity 0", "spsi dev") + d(frame_capacity=0)
    yield ("negative stride", "spsi dev") + d(src_stride=-1)
    yield ("frame_capacity * bins >= 2^31", "spsi dev") + d(frame_capacity=2 ** 31 // 513 + 1)
    yield ("rows * bins >= 2^31", "spsi dev") + d(B=4, src_stride=2 ** 31 // 513 // 4 + 1)
    yield ("null lens_dev", "spsi dev") + d(lens_dev=None)


def _pitch_call(g=DEFAULT_G, lens=(3000, 700), ws=PTR, ws_bytes=0, sr=22050, floor=71.0, ceil=800.0, thr=0.45, oc=0.02, f0=PTR, wav=PTR, mag=None,
                logmel=None):
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    return "fs2_op_stft_pitch_geom", (None,) + tuple(g) + (wav, len(lens), _i32s(starts), _i32s(lens), ws, ws_bytes, mag, None, logmel, None, sr, floor,
                                                          ceil, thr, oc, f0, None)


def _pitch_cases(lib):
    """fs2_op_stft_pitch_geom with the faults of test_pitch_host.test_c_entry_point_refuses_before_any_launch (none of them with a
    workspace that would do), and what tells its order: the pitch options are looked at first, and without f0 it is the plain analysis."""
    p, e = _pitch_call, "pitch"
    need = int(lib.fs2_op_stft_pitch_workspace_bytes_geom(*DEFAULT_G, 2, _i32s((3000, 700))))
    plain = int(lib.fs2_op_stft_workspace_bytes_geom(*DEFAULT_G, 2, _i32s((3000, 700))))
    yield ("workspace one byte short", e) + p(ws_bytes=need - 1)
    yield ("the plain analysis' workspace is too small", e) + p(ws_bytes=plain)
    yield ("floor below 2 sr / win", e) + p(g=(512, 160, 400, 80))
    yield ("ceil above sr / 2", e) + p(ceil=20000.0)
    yield ("floor just usable", e) + p(g=(512, 160, 400, 80), floor=110.4)
    yield ("floor 0", e) + p(floor=0.0)
    yield ("floor above ceil", e) + p(floor=900.0)
    yield ("sample_rate 0", e) + p(sr=0)
    yield ("threshold nan", e) + p(thr=float("nan"))
    yield ("octave cost inf", e) + p(oc=float("inf"))
    yield ("null wav", e) + p(wav=None)
    yield ("null workspace", e) + p(ws=None)
    yield ("no waveform", e) + p(lens=(), wav=None, ws=None)
    yield ("negative length", e) + p(lens=(3000, -1))
    yield ("logmel without basis", e) + p(logmel=PTR)
    yield ("options before the batch", e) + p(floor=0.0, lens=(3000, -1), logmel=PTR)
    yield ("geometry before the options", e) + p(g=BAD_G, floor=0.0)
    yield ("without f0: nothing asked for", e) + p(f0=None, wav=None, ws=None)
    yield ("without f0: options still first", e) + p(f0=None, floor=0.0, wav=None, ws=None)
    yield ("without f0: the plain analysis, one byte short", e) + p(f0=None, mag=PTR, ws_bytes=plain - 1)
    yield ("without f0: the plain analysis, null wav", e) + p(f0=None, mag=PTR, wav=None)


QUERIES_LENS = ("fs2_op_vocode_workspace_bytes_geom", "fs2_op_vocode_mel_workspace_bytes_geom", "fs2_op_spsi_workspace_bytes_geom",
                "fs2_op_stft_workspace_bytes_geom", "fs2_op_stft_pitch_workspace_bytes_geom")
QUERIES_FIXED = ("fs2_op_vocode_workspace_bytes", "fs2_op_stft_workspace_bytes")
QUERIES_CAP = ("fs2_op_vocode_workspace_bytes_cap", "fs2_op_vocode_mel_workspace_bytes_cap", "fs2_op_spsi_workspace_bytes_cap")


def _query_cases(lib):
    """Each of the 10 queries: a good batch (the size itself is recorded), then a bad geometry, a negative length, B = -1, null lens,
    B = 0 and, for _cap, an over-large capacity.  A query answers 0 on every failure."""
    lens = (3000, 700)
    for q in QUERIES_LENS:
        for g in A.GEOMS:
            yield ("size at %s" % (g,), q) + (q, tuple(g) + (80, 2, _i32s(lens)))
        yield ("bad geometry", q) + (q, BAD_G + (2, _i32s(lens)))
        yield ("n_mels 129", q) + (q, (1024, 256, 1024, 129, 2, _i32s(lens)))
        yield ("negative length", q) + (q, DEFAULT_G + (2, _i32s((3000, -1))))
        yield ("B = -1", q) + (q, DEFAULT_G + (-1, _i32s(lens)))
        yield ("null lens", q) + (q, DEFAULT_G + (2, None))
        yield ("B = 0", q) + (q, DEFAULT_G + (0, None))
        yield ("batch too large", q) + (q, DEFAULT_G + (3, _i32s((2 ** 31 - 1,) * 3)))
    for q in QUERIES_FIXED:
        yield ("size", q) + (q, (2, _i32s(lens)))
        yield ("negative length", q) + (q, (2, _i32s((3000, -1))))
        yield ("B = -1", q) + (q, (-1, _i32s(lens)))
        yield ("B = 0", q) + (q, (0, None))
    for q in QUERIES_CAP:
        for g in A.GEOMS:
            yield ("size at %s" % (g,), q) + (q, tuple(g) + (80, 2, 15))
        yield ("bad geometry", q) + (q, BAD_G + (2, 15))
        yield ("negative capacity", q) + (q, DEFAULT_G + (2, -1))
        yield ("B = -1", q) + (q, DEFAULT_G + (-1, 15))
        yield ("B = 0, capacity 0", q) + (q, DEFAULT_G + (0, 0))
        yield ("B = 0", q) + (q, DEFAULT_G + (0, 15))
        yield ("capacity 0", q) + (q, DEFAULT_G + (2, 0))
        yield ("over-large capacity", q) + (q, DEFAULT_G + (4, 2 ** 31 // 513 + 1))


def _cases(lib):
    """(label, where, function, arguments) of every case, in the order of the record."""
    for label, where, fn, args, _ in A._refused_or_empty_calls(lib):
        yield label, where, fn, args
    for label, where, fn, args, _ in M._calls(lib):
        yield label, where, fn, args
    yield from _spsi_cases(lib)
    yield from _pitch_cases(lib)
    yield from _query_cases(lib)


def _mark(lib):
    """Leave a known text in fs2_last_error, so that a case which fails without a message of its own is told from its neighbour."""
    assert lib.fs2_op_bucketize(None, None, 0, None, 0, None) != 0


def _observe(lib):
    out = []
    for label, where, fn, args in _cases(lib):
        _mark(lib)
        code = int(getattr(lib, fn)(*args))
        text = lib.fs2_last_error(None)
        out.append(dict(case="%s | %s | %s" % (fn, where, label), code=code, message=(text or b"").decode()))
    return out


def test_the_case_list_is_what_the_record_was_taken_with(lib):
    got = [c["case"] for c in _observe(lib)]
    want = [c["case"] for c in json.load(open(RECORD))["cases"]]
    assert got == want
    assert len(got) == len(set(got)), "every case has a name of its own"
    n_old = len(list(A._refused_or_empty_calls(lib))) + len(list(M._calls(lib)))
    assert n_old == 119
    called = {c.split(" | ")[0] for c in got}
    assert set(QUERIES_LENS + QUERIES_FIXED + QUERIES_CAP) <= called and len(QUERIES_LENS + QUERIES_FIXED + QUERIES_CAP) == 10
    assert {"fs2_op_griffin_lim", "fs2_op_griffin_lim_geom", "fs2_op_griffin_lim_dev", "fs2_op_griffin_lim_mel_geom", "fs2_op_griffin_lim_mel_dev",
            "fs2_op_spsi_phase_geom", "fs2_op_spsi_phase_dev", "fs2_op_stft", "fs2_op_stft_geom", "fs2_op_stft_pitch_geom"} <= called


def test_every_refusal_keeps_its_code_and_its_message(lib):
    want = json.load(open(RECORD))["cases"]
    got = _observe(lib)
    assert len(got) == len(want)
    wrong = [(g["case"], (g["code"], g["message"]), (w["code"], w["message"])) for g, w in zip(got, want)
             if (g["code"], g["message"]) != (w["code"], w["message"])]
    assert not wrong, "%d of %d cases differ from the record (case, got, recorded): %s" % (len(wrong), len(got), wrong[:5])
    assert _observe(lib) == got, "two passes over the cases agree"


def test_no_call_case_gets_as_far_as_a_launch(lib):
    """A call that returns FS2_OK here is an empty one; every other one was refused with a message of its own, at the workspace at the latest."""
    queries = set(QUERIES_LENS + QUERIES_FIXED + QUERIES_CAP)
    for c in json.load(open(RECORD))["cases"]:
        if c["case"].split(" | ")[0] in queries:
            assert c["code"] >= 0, c
        elif c["code"] != A.OK:
            assert c["code"] in (A.ERR_ARG, A.ERR_WORKSPACE, A.ERR_UNSUPPORTED) and c["message"] != SENTINEL, c


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_vocoder_refusals_host.py --record")
    from fastspeech2_amd import _lib as _L
    _L.build()
    cases = _observe(_L.lib())
    with open(RECORD, "w") as f:
        json.dump(dict(source="include/fs2.h ABI %d, the library before csrc/griffin_lim_host.h took one call description" % _L.lib().fs2_abi_version(),
                       cases=cases), f, indent=1)
        f.write("\n")
    print("wrote %d cases (%d distinct messages) to %s" % (len(cases), len({c["message"] for c in cases}), RECORD))
