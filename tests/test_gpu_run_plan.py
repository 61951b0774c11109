"""``FeedForwardTransformer._run`` behind the run plan, on the GPU (fastspeech2_amd/_run_plan.py): the plan's refusals
come before anything exists or runs, the retry after a grown decoder positional table repeats the call it was, and the two frame
layouts give the same mels.  Default hparams, synthetic weights, tools/forward_digest.py's batch (3 utterances of 5, 17 and 33
phonemes), fp32."""
import pytest
import torch

from tools import forward_digest as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# The loads of the weights one call makes when the decoder's positional table was replaced by one of 16 rows, measured in the same way
# on the commit before the plan existed: one in front of the encoder (the table is another tensor) and one in front of its second
# pass (the table grew to the longest utterance).
RELOADS_AFTER_SHRUNK_TABLE = 2


@pytest.fixture(scope="module")
def batch():
    return D.make_inputs()


@pytest.fixture(scope="module")
def model():
    return D.make_model("default")


def refusals(model, b):
    """(number, text, call) of the refusals 4 - 11 of the plan, each through ``_run`` or ``inference_batch``."""
    xs, il, ol, ds, es, ps = b["xs"], b["ilens"], b["olens"], b["ds"], b["es"], b["ps"]
    cap = D.device_capacity(b)
    small = torch.empty(1, model.odim, device=DEV)
    return [
        (4, "must both be positive", lambda: model._run(xs, il, is_inference=True, regime=(0, 3))),
        (5, "regime applies to per-utterance", lambda: model._run(xs, il, is_inference=True, compat=True, regime=(55, 3))),
        (6, "needs ds, es and ps", lambda: model._run(xs, il, ol, ds, es, None, is_inference=False)),
        (7, r"ds must be \[B, Tmax\]", lambda: model.inference_batch(xs, il, d_override=ds[:, :-1])),
        (7, r"ds must be \[B, Tmax\]", lambda: model._run(xs, il, ol, ds[:, :-1], es, ps, is_inference=False)),
        (8, "serves free-running synthesis", lambda: model._run(xs, il, ol, ds, es, ps, is_inference=False, capacity=cap)),
        (9, "packed_out must be a contiguous float32", lambda: model.inference_batch(xs, il, sync=False, packed=True, packed_out=small, capacity=cap)),
        (10, "'after' or 'after_packed' must be requested", lambda: model._run(xs, il, is_inference=True, want=("before",), capacity=cap)),
        (11, "'after' must be requested", lambda: model._run(xs, il, is_inference=True, want=("before", "after_packed"))),
    ]


def test_refusals_come_before_any_launch(batch):
    model = D.make_model("default")          # its own: the handle must not exist yet
    state = lambda: (model._handle, model.last_olens, model._weights_generation)
    assert state() == (None, None, 0)
    with torch.no_grad():
        for number, text, call in refusals(model, batch):
            with pytest.raises(ValueError, match=text):
                call()
            assert state() == (None, None, 0), number
        model._run(batch["xs"], batch["ilens"], is_inference=True, d_override=batch["ds"])
        torch.cuda.synchronize()
        model.set_profiling(True)
        try:
            listed = model.get_profile()
            held = (model._handle, model._weights_generation)
            for number, text, call in refusals(model, batch):
                with pytest.raises(ValueError, match=text):
                    call()
                torch.cuda.synchronize()
                assert model.get_profile() == listed and (model._handle, model._weights_generation) == held, number
        finally:
            model.set_profiling(False)


def shrink_decoder_table(model):
    from fastspeech2_amd.fastspeech import sinusoid_table
    pos = model.decoder.embed[-1]
    pos.pe = sinusoid_table(16, pos.d_model).to(DEV)
    return pos


def test_retry_after_a_grown_table_repeats_the_call(model, batch):
    model.precision = "fp32"
    xs, il, ds = batch["xs"], batch["ilens"], batch["ds"]
    want = ("before", "after", "e_outs", "p_outs", "lr_index")
    call = lambda: model._run(xs, il, is_inference=True, d_override=ds, alpha=1.0, regime=(55, 3), prosody={"pitch_scale": 1.1}, want=want)
    packed = lambda: model.inference_batch(xs, il, d_override=ds, sync=True, packed=True)
    Lmax = int(batch["olens"].max())
    assert Lmax > 16
    with torch.no_grad():
        # the result dict carries the keys the plan names, in its order
        from fastspeech2_amd._run_plan import plan_run
        plan = plan_run(xs.shape[0], xs.shape[1], len(il), 1, model.odim, model._cfg["adim"], model._cfg["ddim"], True, False, want, has_d_override=True,
                        durations_shape=tuple(ds.shape), regime=(55, 3), controlled=True)
        assert tuple(call()) == plan.keys == want + ("olens", "d_int")
        for run, outputs in ((call, lambda r: [r[k] for k in want + ("olens", "d_int")]), (packed, list)):
            first = outputs(run())
            pos, generation = shrink_decoder_table(model), model._weights_generation
            again = outputs(run())
            assert pos.pe.shape[1] >= Lmax
            assert model._weights_generation == generation + RELOADS_AFTER_SHRUNK_TABLE
            assert len(first) == len(again)
            for a, b in zip(first, again):
                assert a.dtype == b.dtype and torch.equal(a, b)


def test_both_layouts_give_the_same_mels(model, batch):
    from fastspeech2_amd.parallel import row_capacity
    model.precision = "fp32"
    xs, il, ds = batch["xs"], batch["ilens"], batch["ds"]
    with torch.no_grad():
        mels, ol = model.inference_batch(xs, il, d_override=ds, sync=True, packed=True)
        total, longest = int(ol.sum()), int(ol.max())
        buf = torch.full((row_capacity(len(il), total) + 8, model.odim), float("nan"), device=DEV)
        res = model.inference_batch(xs, il, d_override=ds, sync=False, packed=True, packed_out=buf, capacity=(total, longest))
        assert res.ok()
    assert torch.equal(res[1].cpu(), ol) and mels.shape[0] == total
    assert res[0].data_ptr() == buf.data_ptr()                       # the caller's buffer, written in place
    assert torch.equal(res[0][:total], mels) and torch.equal(buf[:total], mels)
    assert torch.isnan(buf[-8:]).all()                               # nothing behind the rows of the capacity
