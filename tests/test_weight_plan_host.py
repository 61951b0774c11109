"""Host-side checks of the weight plan (no GPU): csrc/weight_plan.h -- which images a weight gets at load time -- compiled with the host compiler
(tests/gemm_plan_probe.cpp, modes `weights` and `weight_sweep`; the probe forms its asks with the constructors the loader calls).

The reference of every comparison is the Loader of commit 07673c6, the parent of the weight plan: `parent_images` restates the body of its `Loader::gemm`
(fs2_runtime.hip:743-840 there) expression by expression, `parent_layers` the call sites of `load_stack`, `load_predictor`, `load_tok_proj` and `fs2_load_weights`
with their positional arguments, and `parent_ffn_pointers` the three `ly.w2.wm = nullptr` branches of `load_stack` (:881-891).  Nothing is read back from the tree.

(a) the default model: every layer with its images and byte sizes, pinned, and the bytes of all of them together against what the parent allocates for them;
(b) a sweep over asks, field by field against the parent's conditions; and over FFN shapes, the w_1 / w_2 image pointers a successful load leaves;
(c) the configurations of tests/test_gpu_parity.py's VARIANTS: which layers hold wf / wm / wm4.

The parent's one flag `f16_image` asked for three things (the fp16 image, the mx image of a convolution, the mx4 image with it).  The ask names them apart
(f16, mx_conv, mx4; fs2_op_conv_gemm asks for the mx image alone, as it did by hand); where the sweep sets them apart, the parent's expression is read with the
flag that stands for that use, and mx4 is the parent's `k > 1` inside its mx branch."""
import re

import pytest

from tests.test_gemm_plan_host import CSRC, ROOT, probe  # noqa: F401  (probe: the fixture)

IMAGES = ("w", "wb", "wf", "wm", "wm4", "ws4", "bias")


def round_up(x, a):
    return (x + a - 1) // a * a


# ------------------------------------------------------------------ the parent, restated
def parent_images(parts, Neach, C, k, linear, bias=True, bn=False, f16_image=False, col_off=0, src_cols=0, mx_k1=False, mx_conv=None, mx4=None):
    """Loader::gemm of the parent: the bytes it allocates per image (0: none), the source of the mx image and the shapes it asks of the tensors."""
    mx_conv = f16_image if mx_conv is None else mx_conv
    mx4 = mx_conv if mx4 is None else mx4
    out = dict.fromkeys(IMAGES, 0)
    N = Neach * parts
    Cpad = round_up(C, 32)                                  # g.Cpad = round_up(C, kBK), kBK = 32
    Npad = round_up(N, 128)
    out["w"] = max(Npad * k * Cpad, 1) * 4                  # dalloc((size_t)Npad * k * g.Cpad): max(n, 1) floats
    nchunks = Cpad // 32
    wb_elems = Npad * k * nchunks * 64
    out["wb"] = wb_elems * 2
    src = "none"
    if ((mx_conv and k > 1 and not linear) or (mx_k1 and k == 1 and not src_cols)) and parts == 1 and N % 128 == 0 and C % 128 == 0 and not bn:
        out["wm"] = Npad * (C // 32) * k * 128                                  # mx_image_bytes(Npad, C, k)
        src = "tensor"
        if k > 1 and mx4:
            out["wm4"] = Npad * (C // 64 + C // 128) * k * 128                  # mx4_image_bytes
            out["ws4"] = (Npad // 128) * (C // 128) * k * 1024                  # mx4_scale_image_bytes
    if f16_image:
        out["wf"] = wb_elems * 2
    if bn and k > 1 and parts == 1 and N % 128 == 0 and C % 128 == 0:
        out["wm"] = Npad * (C // 32) * k * 128
        src = "folded"
    if bias or bn:                                          # !bnames.empty(), else if (bg): dalloc(g.N)
        out["bias"] = max(N, 1) * 4
    shape = (Neach, src_cols) if src_cols else ((Neach, C) if linear else (Neach, C, k))
    return dict(out, N=N, Npad=Npad, Cpad=Cpad, nchunks=nchunks, mx_src=src, shape=shape, vec=Neach)


def padded_head_dim(dk):
    return 64 if dk <= 64 else 128 if dk <= 128 else 192 if dk <= 192 else 256


DEFAULT = dict(adim=256, ddim=384, aheads=2, elayers=4, eunits=1024, dlayers=4, dunits=1024, ffn_kernel=9, linear_ffn=False, postnet_layers=5, postnet_filts=5,
               postnet_chans=256, use_batch_norm=True, dur_layers=2, dur_chans=256, dur_kernel=3, var_layers=2, var_chans=256, var_kernel=3, odim=80, reduction_factor=1,
               enc_concat=False, dec_concat=False)


def parent_layers(c):
    """The L.gemm calls of the parent's fs2_load_weights in its order: (name, arguments of parent_images)."""
    out = []

    def stack(tag, layers, D, units, concat):
        k = c["ffn_kernel"]
        Dp = c["aheads"] * padded_head_dim(D // c["aheads"])
        for i in range(layers):
            p = "%s.%d." % (tag, i)
            out.append((p + "qkv", dict(parts=3, Neach=Dp, C=D, k=1, linear=True)))             # (padded heads: L.gemm(wn, bn, st.Dp, D, 1, true))
            out.append((p + "out", dict(parts=1, Neach=D, C=Dp, k=1, linear=True)))
            out.append((p + "w1", dict(parts=1, Neach=units, C=D, k=k, linear=k == 1 and c["linear_ffn"], f16_image=k > 1)))
            out.append((p + "w2", dict(parts=1, Neach=D, C=units, k=1, linear=c["linear_ffn"], mx_k1=k > 1 and D == 384)))
            if concat:
                out.append((p + "cat_x", dict(parts=1, Neach=D, C=D, k=1, linear=True, col_off=0, src_cols=2 * D)))
                out.append((p + "cat_a", dict(parts=1, Neach=D, C=D, k=1, linear=True, bias=False, col_off=D, src_cols=2 * D)))

    def predictor(tag, layers, chans, k):
        for l in range(layers):
            out.append(("%s.conv%d" % (tag, l), dict(parts=1, Neach=chans, C=c["adim"] if l == 0 else chans, k=k, linear=False)))

    stack("enc", c["elayers"], c["adim"], c["eunits"], c["enc_concat"])
    stack("dec", c["dlayers"], c["ddim"], c["dunits"], c["dec_concat"])
    predictor("dur", c["dur_layers"], c["dur_chans"], c["dur_kernel"])
    predictor("energy", c["var_layers"], c["var_chans"], c["var_kernel"])
    predictor("pitch", c["var_layers"], c["var_chans"], c["var_kernel"])
    fused = c["var_layers"] == 2 and c["var_chans"] % 128 == 0 and c["adim"] % 32 == 0
    if fused:
        out.append(("var.c0", dict(parts=2, Neach=c["var_chans"], C=c["adim"], k=c["var_kernel"], linear=False)))
        out.append(("var.c1", dict(parts=2, Neach=c["var_chans"], C=c["var_chans"], k=c["var_kernel"], linear=False)))
    out.append(("dec_in", dict(parts=1, Neach=c["ddim"], C=c["adim"], k=1, linear=True)))
    if fused and c["var_kernel"] == 3 and c["var_chans"] <= 1024 and c["ddim"] % 32 == 0 and c["ddim"] <= 1024:      # tok_proj_cols
        out.append(("tokw", dict(parts=1, Neach=6 * c["var_chans"] + c["ddim"], C=c["adim"], k=1, linear=True, bias=False)))
    out.append(("feat", dict(parts=1, Neach=c["odim"] * max(c["reduction_factor"], 1), C=c["ddim"], k=1, linear=True)))
    for l in range(c["postnet_layers"]):
        ic = c["odim"] if l == 0 else c["postnet_chans"]
        oc = c["odim"] if l == c["postnet_layers"] - 1 else c["postnet_chans"]
        out.append(("post.%d" % l, dict(parts=1, Neach=oc, C=ic, k=c["postnet_filts"], linear=False, bias=False, bn=c["use_batch_norm"])))
    return out


def parent_ffn_pointers(c, D, units):
    """(w1.wm, w2.wm) as load_stack of the parent leaves them after a successful load: w2.wm is set to nullptr again unless w1.wm exists."""
    k = c["ffn_kernel"]
    w1 = parent_images(1, units, D, k, k == 1 and c["linear_ffn"], f16_image=k > 1)
    w2 = parent_images(1, D, units, 1, c["linear_ffn"], mx_k1=k > 1 and D == 384)
    w1_wm, w2_wm = w1["wm"] != 0, w2["wm"] != 0
    if not w1_wm:      # `else ly.w2.wm = nullptr;` (ln1g, ln1b and the scratch exist after a successful load; so does w_1's tensor)
        w2_wm = False
    return w1_wm, w2_wm


# ------------------------------------------------------------------ the probe's lines
def parse_plan(text):
    f = dict(kv.split("=") for kv in text.split())
    ndim, dims = f.pop("shape").split(":")
    out = {k: int(f[k]) for k in IMAGES + ("N", "Npad", "Cpad", "nchunks", "vec")}
    out["mx_src"] = f["mx_src"]
    out["shape"] = tuple(int(d) for d in dims.split(",")[: int(ndim)])
    return out


def probe_model(probe, case):
    lines = probe("weights", case)
    layers = []
    for line in lines[:-1]:
        head, plan = line.split(" | ")
        layers.append((head.split()[0], parse_plan(plan)))
    assert lines[-1].startswith("total ")
    return layers, int(lines[-1].split()[1])


def case_of(c):
    """The probe's case of a configuration (DEFAULT's keys)."""
    keys = dict(adim="adim", ddim="ddim", aheads="aheads", elayers="elayers", eunits="eunits", dlayers="dlayers", dunits="dunits", ffn_kernel="kffn", postnet_layers="post",
                postnet_chans="post_chans", dur_layers="dur_layers", var_chans="var_chans", reduction_factor="rf")
    flags = dict(linear_ffn="linear_ffn", use_batch_norm="bn", enc_concat="enc_concat", dec_concat="dec_concat")
    parts = ["%s=%d" % (keys[k], c[k]) for k in keys if c[k] != DEFAULT[k]] + ["%s=%d" % (flags[k], c[k]) for k in flags if c[k] != DEFAULT[k]]
    assert all(k in keys or k in flags or c[k] == DEFAULT[k] for k in c)
    return ",".join(parts) or "-"


# ------------------------------------------------------------------ (a) the default model
MB = 1 << 20
# kind of layer -> (w, wb, wf, wm, wm4, ws4, bias, mx source); the sizes follow from the formats: fp32 and split-bf16 4 B per padded weight, mx the same,
# mx4 three quarters of it plus 1 KB of scales per (128 output channels, 128 input channels, tap)
PINNED = {
    "enc.qkv": (768 * 256 * 4, 768 * 256 * 4, 0, 0, 0, 0, 768 * 4, "none"),
    "enc.out": (256 * 256 * 4, 256 * 256 * 4, 0, 0, 0, 0, 256 * 4, "none"),
    "enc.w1": (9 * MB, 9 * MB, 9 * MB, 9 * MB, 9 * MB * 3 // 4, 8 * 2 * 9 * 1024, 1024 * 4, "tensor"),
    "enc.w2": (MB, MB, 0, 0, 0, 0, 256 * 4, "none"),                                                   # no row kernel for N = 256: no mx image
    "dec.qkv": (1152 * 384 * 4, 1152 * 384 * 4, 0, 0, 0, 0, 1152 * 4, "none"),
    "dec.out": (384 * 384 * 4, 384 * 384 * 4, 0, 0, 0, 0, 384 * 4, "none"),
    "dec.w1": (13 * MB + MB // 2, 13 * MB + MB // 2, 13 * MB + MB // 2, 13 * MB + MB // 2, (13 * MB + MB // 2) * 3 // 4, 8 * 3 * 9 * 1024, 1024 * 4, "tensor"),
    "dec.w2": (MB + MB // 2, MB + MB // 2, 0, MB + MB // 2, 0, 0, 384 * 4, "tensor"),
    "dur.conv0": (256 * 3 * 256 * 4, 256 * 3 * 256 * 4, 0, 0, 0, 0, 1024, "none"), "dur.conv1": (256 * 3 * 256 * 4, 256 * 3 * 256 * 4, 0, 0, 0, 0, 1024, "none"),
    "energy.conv0": (256 * 3 * 256 * 4, 256 * 3 * 256 * 4, 0, 0, 0, 0, 1024, "none"), "energy.conv1": (256 * 3 * 256 * 4, 256 * 3 * 256 * 4, 0, 0, 0, 0, 1024, "none"),
    "pitch.conv0": (256 * 3 * 256 * 4, 256 * 3 * 256 * 4, 0, 0, 0, 0, 1024, "none"), "pitch.conv1": (256 * 3 * 256 * 4, 256 * 3 * 256 * 4, 0, 0, 0, 0, 1024, "none"),
    "var.c0": (512 * 3 * 256 * 4, 512 * 3 * 256 * 4, 0, 0, 0, 0, 2048, "none"), "var.c1": (512 * 3 * 256 * 4, 512 * 3 * 256 * 4, 0, 0, 0, 0, 2048, "none"),
    "dec_in": (384 * 256 * 4, 384 * 256 * 4, 0, 0, 0, 0, 384 * 4, "none"),
    "tokw": (1920 * 256 * 4, 1920 * 256 * 4, 0, 0, 0, 0, 0, "none"),
    "feat": (128 * 384 * 4, 128 * 384 * 4, 0, 0, 0, 0, 320, "none"),                                   # 80 rows padded to 128
    "post.0": (256 * 5 * 96 * 4, 256 * 5 * 96 * 4, 0, 0, 0, 0, 1024, "none"),                         # 80 channels padded to 96: no mx image
    "post.1": (256 * 5 * 256 * 4, 256 * 5 * 256 * 4, 0, 256 * 5 * 256 * 4, 0, 0, 1024, "folded"),
    "post.2": (256 * 5 * 256 * 4, 256 * 5 * 256 * 4, 0, 256 * 5 * 256 * 4, 0, 0, 1024, "folded"),
    "post.3": (256 * 5 * 256 * 4, 256 * 5 * 256 * 4, 0, 256 * 5 * 256 * 4, 0, 0, 1024, "folded"),
    "post.4": (128 * 5 * 256 * 4, 128 * 5 * 256 * 4, 0, 0, 0, 0, 320, "none"),
}
DEFAULT_TOTAL = 539297920      # bytes of all images of the default model: the plan's figure and the parent's (test_default_model_total)


def _kind(name):
    return re.sub(r"^(enc|dec)\.\d+\.", r"\1.", name)


def test_default_model_is_pinned(probe):
    layers, _ = probe_model(probe, "-")
    assert len(layers) == 2 * 4 * 4 + 6 + 2 + 3 + 5
    assert {_kind(n) for n, _ in layers} == set(PINNED)
    for name, p in layers:
        assert tuple(p[i] for i in IMAGES) + (p["mx_src"],) == PINNED[_kind(name)], name


def test_default_model_total(probe):
    layers, total = probe_model(probe, "-")
    parent = parent_layers(DEFAULT)
    assert [n for n, _ in layers] == [n for n, _ in parent]
    parent_total = sum(sum(parent_images(**a)[i] for i in IMAGES) for _, a in parent)
    print("bytes of the default model's weight images: plan %d, parent's Loader %d" % (total, parent_total))
    assert total == sum(sum(p[i] for i in IMAGES) for _, p in layers)
    assert total == parent_total == DEFAULT_TOTAL


def test_default_model_is_the_parents(probe):
    layers, _ = probe_model(probe, "-")
    for (name, got), (pname, args) in zip(layers, parent_layers(DEFAULT)):
        assert name == pname and got == parent_images(**args), name


# ------------------------------------------------------------------ (b) the sweep
def test_sweep_equals_the_parents_conditions(probe):
    lines = probe("weight_sweep")
    assert len(lines) == 2 * 7 * 8 * 3 * 2 * 2 * 2 * 2 * 8
    seen = set()
    built = dict.fromkeys(("wf", "wm", "wm4", "ws4", "bias"), 0)
    for line in lines:
        head, plan = line.split(" | ")
        a = {k: int(v) for k, v in (kv.split("=") for kv in head.split())}
        want = parent_images(a["parts"], a["Neach"], a["C"], a["k"], bool(a["linear"]), bias=bool(a["bias"]), bn=bool(a["bn"]), f16_image=bool(a["f16"]),
                             col_off=a["col_off"], src_cols=a["src_cols"], mx_k1=bool(a["mx_k1"]), mx_conv=bool(a["mx_conv"]), mx4=bool(a["mx4"]))
        got = parse_plan(plan)
        assert got == want, head
        seen.add(head)
        for i in built:
            built[i] += got[i] != 0
    assert len(seen) == len(lines)
    assert all(built.values()), built      # every optional image is built somewhere in the sweep, so every condition is met from both sides
    cover = lambda key: {int(re.search(r"\b%s=(\d+)" % key, h).group(1)) for h in seen}
    assert cover("parts") == {1, 3} and cover("k") == {1, 3, 9} and cover("linear") == cover("bn") == cover("bias") == {0, 1}
    assert cover("Neach") == {31, 32, 33, 127, 128, 129, 256} and cover("C") == {31, 32, 33, 127, 128, 129, 256, 384}
    assert all(cover(f) == {0, 1} for f in ("f16", "mx_conv", "mx4", "mx_k1")) and len(cover("src_cols")) > 2


@pytest.mark.parametrize("k", [1, 3, 9])
@pytest.mark.parametrize("units", [1000, 1024, 1536])
@pytest.mark.parametrize("D", [256, 320, 384, 512])
def test_ffn_pointers_are_the_parents(probe, D, units, k):
    """w_2's mx image is decided before anything is allocated: the pointers equal what the parent leaves after building the image and taking it back."""
    c = dict(DEFAULT, ddim=D, dunits=units, ffn_kernel=k)
    layers = dict(probe_model(probe, case_of(c))[0])
    got = layers["dec.0.w1"]["wm"] != 0, layers["dec.0.w2"]["wm"] != 0
    assert got == parent_ffn_pointers(c, D, units)
    assert got[1] == (k > 1 and D == 384 and units % 128 == 0)


# ------------------------------------------------------------------ (c) the variants of tests/test_gpu_parity.py
HP_KEYS = dict(positionwise_conv_kernel_size="ffn_kernel", use_batch_norm="use_batch_norm", postnet_layers="postnet_layers", ddim="ddim", dunits="dunits", elayers="elayers",
               dlayers="dlayers", duration_predictor_layers="dur_layers", aheads="aheads", decoder_concat_after="dec_concat")
NO_WEIGHT_KEYS = ("use_scaled_pos_enc", "decoder_normalize_before")      # (a parameter vector more or less: no Linear / Conv1d weight)
POST_MX = {"post.1", "post.2", "post.3"}
FFN = lambda tag, n, what: {"%s.%d.%s" % (tag, i, what) for i in range(n)}
# variant -> (layers with wf, with wm, with wm4)
VARIANT_IMAGES = {
    "linear_ffn": (set(), POST_MX, set()),
    "plain_posenc": (FFN("enc", 4, "w1") | FFN("dec", 4, "w1"), FFN("enc", 4, "w1") | FFN("dec", 4, "w1") | FFN("dec", 4, "w2") | POST_MX, FFN("enc", 4, "w1") | FFN("dec", 4, "w1")),
    "no_batchnorm": (FFN("enc", 4, "w1") | FFN("dec", 4, "w1"), FFN("enc", 4, "w1") | FFN("dec", 4, "w1") | FFN("dec", 4, "w2"), FFN("enc", 4, "w1") | FFN("dec", 4, "w1")),
    "no_postnet": (FFN("enc", 4, "w1") | FFN("dec", 4, "w1"), FFN("enc", 4, "w1") | FFN("dec", 4, "w1") | FFN("dec", 4, "w2"), FFN("enc", 4, "w1") | FFN("dec", 4, "w1")),
    "ddim256_arch": (FFN("enc", 2, "w1") | FFN("dec", 3, "w1"), FFN("enc", 2, "w1") | FFN("dec", 3, "w1") | {"post.1"}, FFN("enc", 2, "w1") | FFN("dec", 3, "w1")),
}
for _v in ("conv_k3_ffn", "aheads4", "aheads8", "aheads4_pre_ln_concat"):
    VARIANT_IMAGES[_v] = VARIANT_IMAGES["plain_posenc"]
VARIANT_IMAGES["aheads1_ddim256"] = (FFN("enc", 4, "w1") | FFN("dec", 4, "w1"), FFN("enc", 4, "w1") | FFN("dec", 4, "w1") | POST_MX, FFN("enc", 4, "w1") | FFN("dec", 4, "w1"))


def _variant_config(hp):
    c = dict(DEFAULT)
    for k, v in hp.items():
        if k == "positionwise_layer_type":
            c["linear_ffn"] = v == "linear"
        elif k not in NO_WEIGHT_KEYS:
            c[HP_KEYS[k]] = v
    return c


def test_variants_are_the_parity_tests():
    from tests.test_gpu_parity import VARIANTS
    from tests.test_call_plan_host import _forward_digest
    assert set(VARIANTS) == set(VARIANT_IMAGES)
    fd = _forward_digest()      # the digest's load cases run the same configurations
    assert all(VARIANTS[k] == v for k, v in fd.LOAD_VARIANTS.items())
    assert set(fd.LOAD_VARIANTS) == {"linear_ffn", "no_batchnorm", "conv_k3_ffn", "aheads8", "aheads4_pre_ln_concat", "ddim256_arch"}


@pytest.mark.parametrize("name", sorted(VARIANT_IMAGES))
def test_variant_images(probe, name):
    from tests.test_gpu_parity import VARIANTS
    c = _variant_config(VARIANTS[name])
    layers, _ = probe_model(probe, case_of(c))
    parent = parent_layers(c)
    assert [n for n, _ in layers] == [n for n, _ in parent]
    for (n, got), (_, args) in zip(layers, parent):
        want = parent_images(**args)
        if n.endswith(".w2"):      # the pointer the parent leaves, not the allocation it made
            tag = n.split(".")[0]
            want["wm"] = want["wm"] if parent_ffn_pointers(c, c["adim" if tag == "enc" else "ddim"], c["eunits" if tag == "enc" else "dunits"])[1] else 0
            want["mx_src"] = "tensor" if want["wm"] else "none"
        assert got == want, n
    for i, image in enumerate(("wf", "wm", "wm4")):
        assert {n for n, p in layers if p[image]} == VARIANT_IMAGES[name][i], image
    assert {n for n, p in layers if p["ws4"]} == VARIANT_IMAGES[name][2]


def test_weight_plan_header_is_hip_free():
    import os
    src = open(os.path.join(CSRC, "weight_plan.h")).read()
    assert sorted(l.split()[1] for l in src.split("\n") if l.startswith("#include")) == ["<cstddef>", "<cstdint>"]
    # the runtime decides no image: the conditions live in the plan
    rt = open(os.path.join(CSRC, "fs2_runtime.hip")).read()
    for kernel in ("repack_weight", "repack_weight_bf16", "repack_weight_mx", "repack_weight_mx4"):
        assert len(re.findall(r"hipLaunchKernelGGL\(%s," % kernel, rt)) == 1, kernel
    assert "D == 384" not in rt
