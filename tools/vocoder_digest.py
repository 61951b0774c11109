"""Digest of the vocoder's outputs per call-forming case: what a change of the host code behind the vocoder's entry points
(csrc/griffin_lim_host.h, fastspeech2_amd/vocoder.py) must leave alone, bit for bit.

    python tools/vocoder_digest.py [--root TREE]

prints `<case> <sha256 over the outputs>`.  --root runs another checkout's package (built there) with this file's cases: run it on the
parent commit twice and on the tree under test, in one session on one machine; where the parent equals itself the tree must equal the
parent (profiles/vocoder_call_digest.txt).

Cases, at the four geometries that take the four branches of gl_dispatch: a batch of (0, 1, L_min - 1, L_min, F, F + 1, 2 F + 5) frames
(nobody owns a sample / too short / the first real one / the tile edge / three tiles) through every form of the synthesis -- n_iter 0
and 3 against momentum 0 and 0.99, constraint magnitude and mel, init seeded / init_phase / spsi, a magnitude source, host-planned
packed and padded, device-driven packed, padded and padded_out -- spsi_phase with its magnitudes in both forms, init="f0" in the same
forms (padded_out also at n_iter 0), f0_phase host and device, packed and padded, the excitation, the analysis with and without pitch, 125 utterances of L_min frames (more tile records than one upload chunk) and 245 of one frame (more than one SPSI
chunk), and the two fixed-geometry entry points called directly.  The largest case has under 600 frames."""
import argparse
import ctypes as C
import hashlib
import os
import sys

GEOMS = [(1024, 256, 1024), (1024, 200, 800), (2048, 300, 1200), (512, 160, 400)]


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy()
        h.update(("%s%s" % (a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def hp_of(geom):
    from fastspeech2_amd.hparams import DotDict
    n_fft, hop, win = geom
    return DotDict({"audio": {"n_fft": n_fft, "hop_length": hop, "win_length": win, "n_mels": 80, "sample_rate": 22050}})


def pad(x, lens, width):
    """packed [sum lens, width] -> padded [B, max lens, width], zeros behind every utterance"""
    import torch
    out = torch.zeros(len(lens), max(max(lens), 1), width, dtype=x.dtype, device=x.device)
    row = 0
    for b, n in enumerate(lens):
        out[b, :n] = x[row:row + n]
        row += n
    return out


def synthesis_cases(gl, name, lens, iters=((0, 0.0), (0, 0.99), (3, 0.0), (3, 0.99)), forms=True):
    """(case, outputs) of the batch ``lens`` through GriffinLim.__call__ in every form (forms=False: host- and device-driven packed only)"""
    import torch
    g = gl.geometry
    gen = torch.Generator().manual_seed(7)
    N = sum(lens)
    mels = (torch.randn(N, g.n_mels, generator=gen) - 3.0).cuda()
    mags = torch.randn(N, g.n_bins, generator=gen).abs().cuda()
    phase = ((torch.rand(N, g.n_bins, generator=gen) * 2 - 1) * 3.14159).cuda()
    olens = torch.tensor(lens, dtype=torch.int64)
    for n_iter, mom in iters:
        for con in ("magnitude", "mel"):
            kw = dict(n_iter=n_iter, momentum=mom, seed=5, constraint=con)
            tag = "%s/%s/it%d/m%g" % (name, con, n_iter, mom)
            yield tag + "/host/packed", gl(mels, olens, **kw)
            w = gl(mels, olens.cuda(), sync=False, **kw)
            yield tag + "/dev/packed", (w.wav, w.sample_lens, w.status)
    if not forms:
        return
    pm, pp, Lmax = pad(mels, lens, g.n_mels), pad(phase, lens, g.n_bins), max(lens)
    for con in ("magnitude", "mel"):
        kw = dict(n_iter=3, momentum=0.99, constraint=con)
        tag = "%s/%s" % (name, con)
        yield tag + "/host/padded", gl(pm, olens, seed=9, **kw)
        yield tag + "/host/init_phase", gl(mels, olens, init_phase=phase, **kw)
        yield tag + "/host/padded/init_phase", gl(pm, olens, init_phase=pp, **kw)
        yield tag + "/host/spsi", gl(mels, olens, init="spsi", **kw)
        for label, extra in (("padded", {}), ("padded_out", dict(padded_out=True)), ("padded/capacity", dict(capacity=sum(lens))),
                             ("padded/init_phase", dict(init_phase=pp)), ("padded/spsi", dict(init="spsi"))):
            w = gl(pm, olens.cuda(), sync=False, seed=9, **kw, **extra)
            yield "%s/dev/%s" % (tag, label), (w.wav, w.sample_lens, w.status)
        w = gl(mels, olens.cuda(), sync=False, init="spsi", **kw)
        yield tag + "/dev/packed/spsi", (w.wav, w.sample_lens, w.status)
    yield name + "/magnitudes/host", gl(mags, olens, n_iter=3, magnitudes=True)
    yield name + "/magnitudes/host/spsi", gl(mags, olens, n_iter=3, magnitudes=True, init="spsi")
    w = gl(mags, olens.cuda(), n_iter=3, magnitudes=True, sync=False)
    yield name + "/magnitudes/dev", (w.wav, w.sample_lens, w.status)
    for label, src, mg in (("mel", mels, False), ("magnitudes", mags, True)):
        yield "%s/spsi_phase/%s/host/packed" % (name, label), gl.spsi_phase(src, olens, magnitudes=mg, return_magnitudes=True)
        yield "%s/spsi_phase/%s/dev/packed" % (name, label), gl.spsi_phase(src, olens.cuda(), magnitudes=mg, return_magnitudes=True, sync=False)
    yield name + "/spsi_phase/mel/host/padded", gl.spsi_phase(pm, olens, return_magnitudes=True)
    yield name + "/spsi_phase/mel/dev/padded", gl.spsi_phase(pm, olens.cuda(), return_magnitudes=True, sync=False)
    yield name + "/spsi_phase/mel/host/phase only", (gl.spsi_phase(mels, olens),)
    yield from f0_cases(gl, name, lens, mels, pm, olens, gen)


def f0_cases(gl, name, lens, mels, pm, olens, gen):
    """init="f0" in every form of the synthesis, f0_phase host and device, packed and padded, and the excitation"""
    import torch
    f0 = 120.0 + 100.0 * torch.rand(sum(lens), generator=gen)
    f0[::5] = 0.0
    f0 = f0.cuda()
    pf = pad(f0[:, None], lens, 1)[:, :, 0].contiguous()
    dev = lambda w: (w.wav, w.sample_lens, w.status)
    for con in ("magnitude", "mel"):
        kw = dict(n_iter=3, momentum=0.99, seed=9, init="f0", constraint=con)
        tag = "%s/%s/f0" % (name, con)
        yield tag + "/host/packed", gl(mels, olens, f0=f0, **kw)
        yield tag + "/host/padded", gl(pm, olens, f0=pf, **kw)
        yield tag + "/dev/packed", dev(gl(mels, olens.cuda(), f0=f0, sync=False, **kw))
        yield tag + "/dev/padded", dev(gl(pm, olens.cuda(), f0=pf, sync=False, **kw))
        yield tag + "/dev/padded_out", dev(gl(pm, olens.cuda(), f0=pf, sync=False, padded_out=True, **kw))
        yield tag + "/dev/padded_out/it0", dev(gl(pm, olens.cuda(), f0=pf, sync=False, padded_out=True, **dict(kw, n_iter=0)))
    yield name + "/f0_phase/host/packed", (gl.f0_phase(f0, olens, seed=9),)
    yield name + "/f0_phase/host/padded", (gl.f0_phase(pf, olens, seed=9),)
    yield name + "/f0_phase/dev/packed", (gl.f0_phase(f0, olens.cuda(), seed=9, sync=False),)
    yield name + "/f0_phase/dev/padded", (gl.f0_phase(pf, olens.cuda(), seed=9, sync=False),)
    yield name + "/excitation", gl.excitation(f0, olens, seed=9)
    yield name + "/excitation/padded", gl.excitation(pf, olens, seed=9)


def analysis_cases(fs, hp, name, g, F):
    import torch
    n_fft, hop, win = g
    T = [0, 100, n_fft // 2, n_fft // 2 + 1, 3000, hop * F, hop * (2 * F + 5) - 1]
    gen = torch.Generator().manual_seed(11)
    t = torch.arange(sum(T), dtype=torch.float32)
    x = (0.4 * torch.sin(2 * 3.14159265 * 180.0 / 22050 * t) + 0.05 * torch.randn(sum(T), generator=gen)).cuda()
    floor = max(71.0, 2.1 * 22050 / win)
    yield name + "/stft_magnitude", (fs.stft_magnitude(x, T, hp=hp),)
    yield name + "/stft_magnitude/mel", (fs.stft_magnitude(x, T, mel=True, hp=hp),)
    yield name + "/mel_energy", fs.mel_energy(x, T, hp=hp)
    yield name + "/wav_features", fs.wav_features(x, T, hp=hp, f0_floor=floor)
    yield name + "/pitch", fs.pitch(x, T, hp=hp, f0_floor=floor, return_strength=True)


def fixed_entry_cases(fs):
    """fs2_op_griffin_lim and fs2_op_stft (no geometry arguments), called as the library exports them"""
    import numpy as np
    import torch
    from fastspeech2_amd import _lib
    lib = _lib.lib()
    gl = fs.GriffinLim()
    lens = np.array([1, 4, 33, 69], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    mels = (torch.randn(int(lens.sum()), 80, generator=torch.Generator().manual_seed(3)) - 3.0).cuda()
    pinv, basis = gl.constants(mels.device)
    wav = torch.zeros(int((256 * np.maximum(lens - 1, 0)).sum()), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.fs2_op_vocode_workspace_bytes(len(lens), p32(lens))), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.fs2_op_griffin_lim(stream, mels.data_ptr(), 80, pinv.data_ptr(), len(lens), p32(starts), p32(lens), 3, 0.99, 5, None, ws.data_ptr(),
                                      ws.numel(), wav.data_ptr()))
    yield "fixed/fs2_op_griffin_lim", (wav,)
    T = (256 * np.maximum(lens - 1, 0)).astype(np.int32)
    t0 = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int32)
    frames = int((T // 256 + 1).sum())
    mag = torch.zeros(frames, 513, dtype=torch.float32, device="cuda")
    lm = torch.zeros(frames, 80, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.fs2_op_stft_workspace_bytes(len(T), p32(T))), dtype=torch.uint8, device="cuda")
    _lib.check(lib.fs2_op_stft(stream, wav.data_ptr(), len(T), p32(t0), p32(T), ws.data_ptr(), ws.numel(), mag.data_ptr(), basis.data_ptr(), lm.data_ptr()))
    yield "fixed/fs2_op_stft", (mag, lm)


def all_cases():
    import torch
    import fastspeech2_amd as fs
    from fastspeech2_amd import vocoder as V
    for g in GEOMS:
        hp, name = hp_of(g), "%d-%d-%d" % g
        gl = V.GriffinLim(hp)
        F, lmin = V.tile_rule(g[0], g[1])["F"], gl.geometry.l_min
        yield from synthesis_cases(gl, name + "/edges", [0, 1, lmin - 1, lmin, F, F + 1, 2 * F + 5])
        yield from synthesis_cases(gl, name + "/125 x L_min", [lmin] * 125, iters=((1, 0.0),), forms=False)
        ones = [1] * 245
        src = (torch.randn(245, 80, generator=torch.Generator().manual_seed(13)) - 3.0).cuda()
        yield name + "/245 x 1/spsi_phase/host", gl.spsi_phase(src, ones, return_magnitudes=True)
        yield name + "/245 x 1/spsi_phase/dev", gl.spsi_phase(src, torch.tensor(ones).cuda(), return_magnitudes=True, sync=False)
        yield from analysis_cases(fs, hp, name, g, F)
    yield from fixed_entry_cases(fs)


def trace_cases():
    """The few cases whose kernel trace is compared (--trace-subset): a host-planned, a device-driven, a mel-constrained, an SPSI, a
    device-driven init="f0" and a pitch call at the default geometry and at one other."""
    import torch
    import fastspeech2_amd as fs
    from fastspeech2_amd import vocoder as V
    for g in GEOMS[:2]:
        hp, name = hp_of(g), "%d-%d-%d" % g
        gl = V.GriffinLim(hp)
        lens = [1, gl.geometry.l_min, 2 * V.tile_rule(g[0], g[1])["F"] + 5]
        mels = (torch.randn(sum(lens), 80, generator=torch.Generator().manual_seed(7)) - 3.0).cuda()
        olens = torch.tensor(lens, dtype=torch.int64)
        yield name + "/host", gl(mels, olens, n_iter=3, momentum=0.99)
        w = gl(mels, olens.cuda(), n_iter=3, sync=False)
        yield name + "/dev", (w.wav, w.sample_lens, w.status)
        yield name + "/mel", gl(mels, olens, n_iter=3, momentum=0.99, constraint="mel")
        yield name + "/spsi", gl(mels, olens, n_iter=3, init="spsi")
        f0 = torch.full((sum(lens),), 150.0).cuda()
        w = gl(mels, olens.cuda(), n_iter=3, init="f0", f0=f0, sync=False)
        yield name + "/f0", (w.wav, w.sample_lens, w.status)
        x =gl(mels, olens, n_iter=0).wav
        yield name + "/pitch", fs.wav_features(x, [x.numel()], hp=hp)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose (built) package runs the cases")
    ap.add_argument("--trace-subset", action="store_true", help="only the cases of trace_cases(), for a kernel trace of their launches")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    assert torch.cuda.is_available(), "vocoder_digest.py needs a GPU"
    import fastspeech2_amd
    print("# package: %s" % os.path.dirname(fastspeech2_amd.__file__), file=sys.stderr)
    n = 0
    for case, out in (trace_cases() if args.trace_subset else all_cases()):
        torch.cuda.synchronize()
        print(case.replace(" ", "_"), digest(*[t for t in out if t is not None]), flush=True)
        n += 1
    print("# %d cases" % n, file=sys.stderr)


if __name__ == "__main__":
    main()
