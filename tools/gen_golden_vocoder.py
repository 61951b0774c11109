"""Golden vectors of the reference's Griffin-Lim (tests/golden/g10_griffin_lim.npz): imports the REFERENCE's own STFT and
griffin_lim (utils/stft.py, dataset/audio_processing.py) in the build container and records their outputs for one ~0.5 s synthetic
harmonic signal's magnitudes, with recorded initial angles, at n_iters 0, 1 and 30.

TEST INFRASTRUCTURE ONLY, like oracle/gen_golden.py: the reference's third-party imports the path never uses are stubbed
(librosa.util gets numpy pad_center / tiny, librosa.filters.mel a dummy, pyworld an empty module), and torch.Tensor.cuda is patched
to the identity because the reference hard-codes .cuda() (stft.py:96-99, audio_processing.py:235).  The fixture holds data only:
the magnitudes, the angles and the reference's signals (float32).  It also prints the float64 oracle's distance to them.

Usage (in the build container, with the reference checked out):  python tools/gen_golden_vocoder.py [REFERENCE_DIR]
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def import_reference(ref):
    def stub(n, **a):
        m = types.ModuleType(n)
        m.__dict__.update(a)
        sys.modules[n] = m
        return m

    def pad_center(data, size, axis=-1, **kw):
        n = data.shape[axis]
        lpad = int((size - n) // 2)
        widths = [(0, 0)] * data.ndim
        widths[axis] = (lpad, int(size - n - lpad))
        return np.pad(data, widths, **kw)

    def normalize(S, norm=None, **kw):
        assert norm is None
        return S

    util = stub("librosa.util", pad_center=pad_center, tiny=lambda x: np.finfo(np.asarray(x).dtype).tiny, normalize=normalize)
    filters = stub("librosa.filters", mel=lambda *a, **k: np.zeros((80, 513), np.float32))
    stub("librosa", util=util, filters=filters)
    stub("pyworld")
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, ref)
    from utils.stft import STFT
    from dataset.audio_processing import griffin_lim
    return STFT, griffin_lim


def main():
    from tests import vocoder_oracle as O           # (before the reference's directory joins sys.path: it has a tests package too)
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FS2_REFERENCE", "../reference")
    STFT, griffin_lim = import_reference(ref)
    stft = STFT(filter_length=1024, hop_length=256, win_length=1024)
    sig = O.harmonic_signal(11008, seed=3, noise=0.01).astype(np.float32)          # 0.5 s -> 44 frames
    mag, _ = stft.transform(torch.from_numpy(sig)[None])                            # [1, 513, L]
    out = dict(signal=sig, magnitudes=mag[0].numpy().T.copy())                       # [L, 513]
    np.random.seed(1234)
    angles = np.angle(np.exp(2j * np.pi * np.random.rand(*mag.size()))).astype(np.float32)   # what griffin_lim draws
    out["angles"] = angles[0].T.copy()
    for n in (0, 1, 30):
        np.random.seed(1234)
        y = griffin_lim(mag, stft, n).numpy()[0]
        out["wav_iter%d" % n] = y.astype(np.float32)
        o = O.griffin_lim(out["magnitudes"], out["angles"], n)
        print("n_iters %2d: %d samples, oracle max-abs diff %.3e (peak %.3f), SC ref %.5f oracle %.5f"
              % (n, y.size, np.abs(o - y).max(), np.abs(y).max(), O.spectral_convergence(out["magnitudes"], y),
                 O.spectral_convergence(out["magnitudes"], o)))
    path = os.path.join(ROOT, "tests", "golden", "g10_griffin_lim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
