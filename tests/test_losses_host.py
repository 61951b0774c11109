"""CPU: the float64 restatement of the loss terms (tests/losses_oracle.py) and the host half of fastspeech2_amd.losses (LossTerms:
report / evaluate / per_utterance / merge, fed with the oracle's records) against the reference's own recordings.

The reference's report values are float32 means of <= 11,280 terms (3 x 47 x 80 mel values), so they carry a few 1e-7 of relative
error themselves; the float64 algebra is held to them at 1e-6 relative.  Measured on this CPU: 1.6e-7 (G2, masked, worst of the
seven) and 9.9e-8 (G9, unmasked + weighted)."""
import os

import numpy as np
import pytest

from tests import losses_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-6


@pytest.fixture(scope="module")
def g2():
    return dict(np.load(os.path.join(GOLD, "g2_teacher_padded_b3.npz")))


@pytest.fixture(scope="module")
def g9():
    return dict(np.load(os.path.join(GOLD, "g9_weighted_masking_b3.npz")))


def _tensors(g):
    return tuple(g[k] for k in ("before", "after", "ys", "d_outs", "ds", "e_outs", "es", "p_outs", "ps"))


def _worst(pairs, want):
    got = np.asarray([v for _, v in pairs])
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _loss_terms(rows, batch, pads=True, odim=80):
    from fastspeech2_amd.losses import LossTerms
    return LossTerms(rows, batch, pads, odim)


def test_oracle_and_report_equal_the_reference_recordings(g2, g9):
    assert list(g2["report_names"]) == list(O.REPORT_NAMES) == list(g9["report_names"])
    for k in ("xs", "ilens", "olens", "ds", "es", "ps", "ys"):          # G9 is the same batch under the other switches
        assert np.array_equal(g2[k], g9[k]), k
    rows, batch = O.records(*_tensors(g2), g2["ilens"], g2["olens"])
    masked = O.report(batch, 80, True, False)
    weighted = O.report(batch, 80, False, True)
    w2, w9 = _worst(masked, g2["report_values"]), _worst(weighted, g9["report_values"])
    print("worst relative difference: G2 masked %.3g, G9 unmasked + weighted %.3g" % (w2, w9))
    assert w2 <= REL and w9 <= REL
    lt = _loss_terms(rows, batch)
    assert lt.report() == [(n, float(v)) for n, v in masked]
    assert lt.report(use_masking=False, use_weighted_masking=True) == [(n, float(v)) for n, v in weighted]
    assert [n for n, _ in lt.report()] == list(O.REPORT_NAMES)
    plain = dict(lt.report(use_masking=False))                         # unmasked, unweighted: only l1_loss and loss differ from G9's
    assert abs(plain["l1_loss"] - (plain["before_loss"] + plain["after_loss"])) == 0.0
    for n in ("before_loss", "after_loss", "duration_loss", "energy_loss", "pitch_loss"):
        assert plain[n] == dict(weighted)[n]


def test_evaluate_on_one_utterance_is_the_plain_mean():
    g = dict(np.load(os.path.join(GOLD, "g1_teacher_b1.npz")))
    ys = np.zeros_like(g["before"])
    rows, batch = O.records(g["before"], g["after"], ys, g["d_outs"], g["ds"], g["e_outs"], g["es"], g["p_outs"], g["ps"], g["ilens"], g["olens"])
    D = np.float64
    want = (np.abs(g["p_outs"].astype(D) - g["ps"]).mean(), np.abs(g["e_outs"].astype(D) - g["es"]).mean(),
            np.abs(g["d_outs"].astype(D) - g["ds"]).mean())
    for got in (O.evaluate(rows), _loss_terms(rows, batch).evaluate()):
        assert np.allclose(got, want, rtol=1e-12, atol=0.0), (got, want)
    pu = _loss_terms(rows, batch).per_utterance()
    assert pu["ilen"].tolist() == [24] and pu["olen"].tolist() == [113]
    assert np.allclose([pu["pitch_l1"][0], pu["energy_l1"][0], pu["duration_l1"][0]], want, rtol=1e-12, atol=0.0)
    assert np.isclose(pu["energy_mse"][0], ((g["e_outs"].astype(D) - g["es"]) ** 2).mean(), rtol=1e-12, atol=0.0)


def test_merge_of_single_utterances_is_the_batch(g2):
    t = _tensors(g2)
    rows, batch = O.records(*t, g2["ilens"], g2["olens"])
    merged = None
    for b in range(3):
        r1, b1 = O.records(*[x[b:b + 1] for x in t], g2["ilens"][b:b + 1], g2["olens"][b:b + 1])
        one = _loss_terms(r1, b1)
        merged = one if merged is None else merged.merge(one)
    additive = [0, 1] + list(range(4, 12))                             # lengths and the sums over [0, len): no Tmax / Lmax in them
    assert len(merged) == 3
    assert np.array_equal(merged.terms[:, additive], rows[:, additive])
    assert O.close(merged.batch[additive], batch[additive])
    assert merged.batch[2] == 0 and merged.batch[3] == 0               # an utterance alone has no pads
    whole = _loss_terms(rows, batch)
    assert np.allclose([v for _, v in merged.report()], [v for _, v in whole.report()], rtol=1e-12, atol=0.0)
    assert merged.evaluate() == pytest.approx(whole.evaluate(), rel=1e-12)
    from fastspeech2_amd.losses import LossTerms
    assert np.array_equal(LossTerms.empty().merge(whole).batch, batch)
    with pytest.raises(ValueError, match="pads"):
        whole.merge(_loss_terms(rows, batch, pads=False))
    with pytest.raises(ValueError, match="pads=False"):
        _loss_terms(rows, batch, pads=False).report(use_masking=False)


def test_masking_with_weighted_masking_raises_the_reference_error(g2):
    rows, batch = O.records(*_tensors(g2), g2["ilens"], g2["olens"])
    with pytest.raises(IndexError, match="Dimension out of range"):
        O.report(batch, 80, True, True)
    with pytest.raises(IndexError, match="Dimension out of range"):
        _loss_terms(rows, batch).report(use_masking=True, use_weighted_masking=True)


def test_cpu_tensors_raise():
    import torch
    from fastspeech2_amd.losses import loss_terms
    z = torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_terms(z, z, z, None, None, None, None, None, None, [1], [2])


def test_ctypes_mirror_of_the_argument_struct_matches_the_compiled_header(tmp_path):
    """fs2_op_loss_args as gcc sees include/fs2.h: sizeof and the offset of every field equal those of _lib.OpLossArgs."""
    import ctypes
    import subprocess
    from fastspeech2_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in _lib.OpLossArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fs2.h"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(fs2_op_loss_args));', '  printf("FS2_LOSS_TERMS %d\\n", FS2_LOSS_TERMS);']
    src += ['  printf("%s %%zu\\n", offsetof(fs2_op_loss_args, %s));' % (f, f) for f in fields] + ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(src))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", exe], check=True)
    probe = {k: int(v) for k, v in (line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert probe["sizeof"] == ctypes.sizeof(_lib.OpLossArgs) == _lib.OpLossArgs().struct_size
    assert probe["FS2_LOSS_TERMS"] == _lib.LOSS_TERMS == O.TERMS
    for f in fields:
        assert getattr(_lib.OpLossArgs, f).offset == probe[f], f
    hdr = open(os.path.join(root, "include", "fs2.h")).read()
    body = hdr[hdr.index("struct fs2_op_loss_args {"):hdr.index("typedef struct fs2_op_loss_args")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"[*\s,](\w+)\s*[,;]", body[body.index("{"):])
    assert declared == fields, (declared, fields)
