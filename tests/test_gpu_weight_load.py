"""fs2_load_weights on a broken tensor list (the default model): one tensor per kind of layer of csrc/weight_plan.h's ask constructors removed, one per kind given a
wrong shape.  The load returns FS2_ERR_WEIGHT with the message naming that tensor, leaves the handle unloaded, and a correct load afterwards succeeds and
computes what it computed before.

The expected strings are the formats of the Loader of commit 07673c6, the parent of the weight plan (fs2_runtime.hip:705 and :710 there): "missing tensor %s" and
"tensor %s has the wrong shape"."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

FS2_ERR_WEIGHT, FS2_ERR_STATE = -4, -3
MISSING, WRONG_SHAPE = "missing tensor %s", "tensor %s has the wrong shape"

# kind of layer -> a tensor of it (the fused predictors and tok.proj read the predictors' and the input layer's tensors: those are named by their first reader)
TENSORS = {
    "qkv": "encoder.encoders_.0.self_attn.linear_k.weight",
    "qkv bias": "decoder.encoders_.1.self_attn.linear_v.bias",
    "attention out": "encoder.encoders_.1.self_attn.linear_out.weight",
    "ffn w_1": "decoder.encoders_.0.feed_forward.w_1.weight",
    "ffn w_1 bias": "decoder.encoders_.2.feed_forward.w_1.bias",
    "ffn w_2": "decoder.encoders_.3.feed_forward.w_2.weight",
    "duration predictor conv": "duration_predictor.conv.1.0.weight",
    "variance predictor conv": "energy_predictor.predictor.conv.0.0.weight",
    "variance predictor conv bias": "pitch_predictor.predictor.conv.1.0.bias",
    "dec.in": "decoder.embed.0.weight",
    "feat_out": "feat_out.weight",
    "postnet": "postnet.postnet.2.0.weight",
    "postnet batch norm": "postnet.postnet.1.1.running_var",
    "postnet last": "postnet.postnet.4.0.weight",
}
_state = {}


def _setup():
    """The default model with a loaded handle, its tensor list, one small batch and the mel of that batch (once per session)."""
    if _state:
        return _state
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from fastspeech2_amd import FeedForwardTransformer, default_hparams, N_PHONEME_SYMBOLS
    from fastspeech2_amd.synthetic import portable_state_dict, make_batch
    hp = default_hparams()
    model = FeedForwardTransformer(N_PHONEME_SYMBOLS, hp.audio.num_mels, hp).eval()
    model.load_state_dict(portable_state_dict(model.state_dict(), seed=3))
    model = model.to("cuda:0")
    b = make_batch("c2", seed=11, B=2, tlens=[9, 17])
    run = lambda: model._run(b["xs"].cuda(), b["ilens"], b["olens"], b["ds"].cuda(), b["es"].cuda(), b["ps"].cuda(), is_inference=False, want=("after",))["after"].clone()
    with torch.no_grad():
        model.precision = "mix_mx4"      # (every image of the default model is read)
        after = run()
    tensors = [(n, t.detach().contiguous()) for n, t in model.state_dict().items() if t.dtype == torch.float32]
    assert set(TENSORS.values()) <= {n for n, _ in tensors}
    _state.update(model=model, run=run, after=after, tensors=tensors)
    return _state


def _load(st, edit):
    """fs2_load_weights on the model's handle with edit(name, shape) -> None (leave the tensor out) or the shape to declare.  Returns (code, message)."""
    from fastspeech2_amd import _lib
    L = _lib.lib()
    descs = []
    for name, t in st["tensors"]:
        shape = edit(name, list(t.shape))
        if shape is not None:
            descs.append(_lib.TensorDesc(name.encode(), t.data_ptr(), len(shape), (C.c_int64 * 4)(*(shape + [0] * (4 - len(shape))))))
    arr = (_lib.TensorDesc * len(descs))(*descs)
    h = st["model"]._handle
    code = L.fs2_load_weights(h, arr, len(descs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return code, L.fs2_last_error(h).decode()


def _refused_then_loads(st, edit, want):
    code, msg = _load(st, edit)
    print("fs2_load_weights -> %d %r" % (code, msg))
    assert (code, msg) == (FS2_ERR_WEIGHT, want)
    # the handle holds no weights now: a forward is refused, not run on freed memory
    from fastspeech2_amd import _lib
    with pytest.raises(_lib.Fs2Error) as e, torch.no_grad():
        st["run"]()
    assert e.value.code == FS2_ERR_STATE and "weights not loaded" in str(e.value)
    assert _load(st, lambda name, shape: shape)[0] == 0
    with torch.no_grad():
        assert torch.equal(st["run"](), st["after"])


@pytest.mark.parametrize("kind", sorted(TENSORS))
def test_missing_tensor_is_named(kind):
    st = _setup()
    gone = TENSORS[kind]
    _refused_then_loads(st, lambda name, shape: None if name == gone else shape, MISSING % gone)


@pytest.mark.parametrize("kind", sorted(TENSORS))
def test_wrong_shape_is_named(kind):
    st = _setup()
    odd = TENSORS[kind]
    _refused_then_loads(st, lambda name, shape: shape[:-1] + [shape[-1] + 1] if name == odd else shape, WRONG_SHAPE % odd)


def test_transposed_and_flattened_shapes_are_refused():
    """The number of dimensions counts, and so does their order: a Conv1d weight declared [N, C k], a Linear weight declared [C, N]."""
    st = _setup()
    conv, lin = TENSORS["ffn w_1"], TENSORS["feat_out"]
    _refused_then_loads(st, lambda name, shape: [shape[0], shape[1] * shape[2]] if name == conv else shape, WRONG_SHAPE % conv)
    _refused_then_loads(st, lambda name, shape: shape[::-1] if name == lin else shape, WRONG_SHAPE % lin)
