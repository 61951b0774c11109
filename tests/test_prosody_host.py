"""CPU: the host side of pitch / energy control (fastspeech2_amd/prosody.py, _lib.Prosody): the ctypes mirror against the header as gcc
compiles it, the normaliser's accepted and rejected forms, semitones, the fields of ProsodyPrediction and the signatures that carry
the four keywords.  No GPU, no launch."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTROLS = ["pitch_scale", "pitch_shift", "energy_scale", "energy_shift"]


def test_ctypes_mirror_of_fs2_prosody_matches_the_compiled_header(tmp_path):
    """fs2_prosody as gcc sees include/fs2.h: sizeof and the offset of every field equal those of _lib.Prosody; the revision stays 4."""
    from fastspeech2_amd import _lib
    fields = [f[0] for f in _lib.Prosody._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fs2.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(fs2_prosody));', '  printf("FS2_ABI_VERSION %d\\n", FS2_ABI_VERSION);']
    src += ['  printf("%s %%zu\\n", offsetof(fs2_prosody, %s));' % (f, f) for f in fields] + ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", exe], check=True)
    probe = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert probe["sizeof"] == ctypes.sizeof(_lib.Prosody) == _lib.Prosody().struct_size
    assert probe["FS2_ABI_VERSION"] == _lib.ABI_VERSION == 4                # the addition is additive
    for f in fields:
        assert getattr(_lib.Prosody, f).offset == probe[f], f
    hdr = open(os.path.join(ROOT, "include", "fs2.h")).read()
    body = hdr[hdr.index("struct fs2_prosody {"):hdr.index("typedef struct fs2_prosody")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[*\s,](\w+)\s*[,;]", body[body.index("{"):])
    assert declared == fields, (declared, fields)
    assert fields == ["struct_size"] + CONTROLS + [c + "_cols" for c in CONTROLS]
    assert "fs2_decode_ctl" in _lib.EXPORTS and "fs2_op_label_means" in _lib.EXPORTS


def test_library_exports_the_entry_points_and_refuses_bad_label_means_arguments():
    """The built library (hipcc cross-compiles gfx950 without a GPU): the two symbols exist, and fs2_op_label_means answers its
    argument errors on the host, before any launch."""
    from fastspeech2_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert hasattr(L, "fs2_decode_ctl") and hasattr(L, "fs2_op_label_means")
    assert L.fs2_op_label_means(None, None, None, None, 0, 5, 3, 0, None, None) == 0                   # B = 0: nothing to do
    assert L.fs2_op_label_means(None, None, None, None, -1, 5, 3, 0, None, None) == -1 and b"fs2_op_label_means" in L.fs2_last_error(None)
    assert L.fs2_op_label_means(None, None, None, None, 2, 5, 3, 0, None, None) == -1 and b"null" in L.fs2_last_error(None)
    assert L.fs2_op_label_means(None, None, None, None, 2, -5, 3, 0, None, None) == -1
    assert L.fs2_op_label_means(None, None, None, None, 2, 5, -3, 0, None, None) == -1
    # fs2_decode_ctl checks the handle before anything else
    assert L.fs2_decode_ctl(None, None, None, None) == -1


def test_normaliser_accepts_none_numbers_and_the_two_shapes():
    from fastspeech2_amd.prosody import CONTROLS as names, normalize_controls, prosody_struct
    assert list(names) == CONTROLS
    B, T = 3, 9
    none = normalize_controls(B, T, "cpu")
    assert list(none) == CONTROLS and all(v is None for v in none.values()) and prosody_struct(none) is None and prosody_struct(None) is None
    per_tok = torch.rand(B, T)
    wide = torch.rand(B, 2 * T)[:, ::2]                                     # a strided view: made contiguous
    assert not wide.is_contiguous()
    got = normalize_controls(B, T, "cpu", pitch_scale=2, pitch_shift=per_tok, energy_scale=torch.full((B, 1), 0.5), energy_shift=wide)
    assert got["pitch_scale"].shape == (B, 1) and got["pitch_scale"].dtype == torch.float32 and torch.all(got["pitch_scale"] == 2.0)
    assert got["pitch_shift"].data_ptr() == per_tok.data_ptr()             # already in the form: used as it is
    assert got["energy_scale"].shape == (B, 1) and got["energy_shift"].is_contiguous() and torch.equal(got["energy_shift"], wide)
    st = prosody_struct(got)
    assert st.struct_size == ctypes.sizeof(st)
    assert [getattr(st, c + "_cols") for c in CONTROLS] == [1, T, 1, T]
    assert [getattr(st, c) for c in CONTROLS] == [got[c].data_ptr() for c in CONTROLS]
    one = prosody_struct(normalize_controls(B, T, "cpu", energy_shift=-0.25))
    assert [getattr(one, c) for c in CONTROLS[:3]] == [None] * 3 and one.energy_shift and one.energy_shift_cols == 1
    # what ShardedSynthesizer does with a tensor keyword: rows of the shard, columns up to the shard's longest utterance
    sel, T_loc = torch.tensor([2, 0]), 4
    cut = lambda v: v[sel][:, :T_loc]
    shard = normalize_controls(2, T_loc, "cpu", pitch_shift=cut(per_tok), energy_scale=cut(got["energy_scale"]))
    assert shard["pitch_shift"].shape == (2, T_loc) and torch.equal(shard["pitch_shift"], per_tok[[2, 0], :4]) and shard["energy_scale"].shape == (2, 1)
    # Tmax = 1: [B, 1] is both forms
    assert normalize_controls(B, 1, "cpu", pitch_scale=torch.ones(B, 1))["pitch_scale"].shape == (B, 1)


@pytest.mark.parametrize("name", CONTROLS)
def test_normaliser_rejects_everything_else_naming_the_argument(name):
    from fastspeech2_amd.prosody import normalize_controls
    B, T = 3, 9
    bad = [torch.ones(B), torch.ones(B, T + 1), torch.ones(B + 1, T), torch.ones(B, T, 1), torch.ones(T, B), torch.ones(B, T, dtype=torch.float64),
           torch.ones(B, 1, dtype=torch.int64), torch.ones(B, T, device="meta"), "loud", [1.0] * B, True]
    for v in bad:
        with pytest.raises(ValueError, match=name):
            normalize_controls(B, T, "cpu", **{name: v})
    with pytest.raises(TypeError):
        normalize_controls(B, T, "cpu", duration_scale=1.0)


def test_semitones():
    from fastspeech2_amd import semitones
    assert semitones(12) == 2.0 and semitones(0) == 1.0 and semitones(-12) == 0.5 and semitones(24) == 4.0
    assert abs(semitones(2) - 1.122462048309373) < 1e-15 and semitones(+2) * semitones(-2) == pytest.approx(1.0, abs=1e-15)


def test_prosody_prediction_fields_and_the_public_signatures():
    from fastspeech2_amd import FeedForwardTransformer, ProsodyPrediction, label_means
    assert ProsodyPrediction._fields == ("durations", "olens", "pitch", "energy", "lr_index", "pitch_tok", "energy_tok", "voiced_tok")
    p = ProsodyPrediction(*range(8))
    assert p.durations == 0 and p.voiced_tok == 7 and isinstance(p, tuple)
    params = lambda f: list(inspect.signature(f).parameters)
    # every earlier positional order and default stays; the four keywords come behind them
    assert params(FeedForwardTransformer.inference) == ["self", "x", "alpha"] + CONTROLS
    assert params(FeedForwardTransformer.inference_batch) == ["self", "xs", "ilens", "d_override", "packed", "sync", "capacity", "alpha", "packed_out", "regime",
                                                              "inputs_ready"] + CONTROLS
    assert params(FeedForwardTransformer.capture_graph) == ["self", "xs", "ilens", "d_override", "vocoder"] + CONTROLS + ["vocoder_args"]
    assert params(FeedForwardTransformer.predict_prosody) == ["self", "xs", "ilens", "alpha", "d_override", "controls"]
    assert params(FeedForwardTransformer._run)[-1] == "prosody"
    for f in (FeedForwardTransformer.inference, FeedForwardTransformer.inference_batch, FeedForwardTransformer.capture_graph):
        sig = inspect.signature(f).parameters
        assert all(sig[c].default is None for c in CONTROLS)
    assert inspect.signature(FeedForwardTransformer.inference_batch).parameters["sync"].default is True
    assert params(label_means) == ["x", "labels", "lens", "n_labels", "positive_only"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label_means(torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int32), [2], 1)


def test_control_errors_are_raised_on_the_host_before_anything_runs():
    """No GPU here: each of these must fail in the argument checks, not at the missing device."""
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    hp = default_hparams()
    m = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    xs = torch.ones(2, 5, dtype=torch.int64)
    m.batch_semantics = "padded_compat"
    with pytest.raises(ValueError, match="per-utterance"):
        m.inference_batch(xs, [5, 5], pitch_scale=1.5)
    with pytest.raises(ValueError, match="per-utterance"):
        m.predict_prosody(xs, [5, 5], energy_shift=0.1)
    m.batch_semantics = "per_utterance"
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # (and without control the call reaches the device check as before)
        m.inference_batch(xs, [5, 5])
    with pytest.raises(TypeError):
        m.predict_prosody(xs, [5, 5], duration_scale=2.0)
