"""Golden vectors of the reference's STFT and Griffin-Lim at other transform geometries (tests/golden/g11_stft_geometries.npz):
imports the REFERENCE's own STFT class and griffin_lim with the stubs of tools/gen_golden_vocoder.py and records, per geometry
n_fft / hop / win_length, a synthetic harmonic signal of 43 hops (44 frames), its magnitudes from STFT.transform, the angles the
reference's griffin_lim draws after np.random.seed(1234), its waveforms after 0, 1 and 30 iterations, and the frame energy
torch.norm(magnitudes, dim=0) of the reference's preprocessing (nvidia_preprocessing.py).  Keys are prefixed "<n_fft>_<hop>_<win>/".
It prints the float64 oracle's distance (tests/vocoder_oracle.py) to each, relative to the peak.

TEST INFRASTRUCTURE ONLY.  Usage (in the build container, with the reference checked out):
    python tools/gen_golden_stft_geometries.py [--all] [REFERENCE_DIR]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (n_fft, hop, win, sample rate of the recipe's signal).  Between them: n_fft 2048 and 512, a window shorter than n_fft and a hop
# that does not divide n_fft.  512 / 128 / 512 and 2048 / 512 / 2048 would take the file past 1 MiB (the random angles do not
# compress); pass --all to print their figures without writing them.
GEOMETRIES = [(2048, 300, 1200, 24000), (512, 160, 400, 22050), (1024, 200, 800, 22050)]
EXTRA = [(512, 128, 512, 22050), (2048, 512, 2048, 22050)]


def key(n_fft, hop, win):
    return "%d_%d_%d" % (n_fft, hop, win)


def main():
    from tests import vocoder_oracle as O           # (before the reference's directory joins sys.path: it has a tests package too)
    from tools.gen_golden_vocoder import import_reference
    args = [a for a in sys.argv[1:] if a != "--all"]
    ref = args[0] if args else os.environ.get("FS2_REFERENCE", "../reference")
    extra = EXTRA if "--all" in sys.argv[1:] else []
    STFT, griffin_lim = import_reference(ref)
    out = {}
    for n_fft, hop, win, sr in GEOMETRIES + extra:
        k = key(n_fft, hop, win) + "/"
        stft = STFT(filter_length=n_fft, hop_length=hop, win_length=win)
        sig = O.harmonic_signal(43 * hop, seed=3, noise=0.01, sr=sr).astype(np.float32)
        mag, _ = stft.transform(torch.from_numpy(sig)[None])                            # [1, bins, L]
        out[k + "signal"] = sig
        out[k + "magnitudes"] = mag[0].numpy().T.copy()                                  # [L, bins]
        out[k + "energy"] = torch.norm(mag[0], dim=0).numpy().astype(np.float32)         # [L]
        np.random.seed(1234)
        angles = np.angle(np.exp(2j * np.pi * np.random.rand(*mag.size()))).astype(np.float32)
        out[k + "angles"] = angles[0].T.copy()
        o = O.Stft(n_fft, hop, win)
        row = []
        for n in (0, 1, 30):
            np.random.seed(1234)
            y = griffin_lim(mag, stft, n).numpy()[0].astype(np.float32)
            out[k + "wav_iter%d" % n] = y
            g = o.griffin_lim(out[k + "magnitudes"], out[k + "angles"], n)
            row.append(np.abs(g - y).max() / np.abs(y).max())
        e = o.energy(sig)
        row.append(np.abs(e - out[k + "energy"]).max() / np.abs(e).max())
        print("%4d/%3d/%4d: %d frames, oracle vs reference GL 0 / 1 / 30: %.2e / %.2e / %.2e, energy %.2e"
              % (n_fft, hop, win, mag.shape[-1], *row))
    path = os.path.join(ROOT, "tests", "golden", "g11_stft_geometries.npz")
    keep = {key(n, h, w) for n, h, w, _ in GEOMETRIES}
    np.savez_compressed(path, **{a: b for a, b in out.items() if a.split("/")[0] in keep})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
