"""Golden vectors of the reference's target cleaning (tests/golden/g12_targets.npz): imports the REFERENCE's own
utils.util.remove_outlier and records its outputs for seeded synthetic float32 arrays, 16 utterances of each of three kinds (lengths
1 .. 400; tests/targets_oracle.py: energy-like, F0-like with zeros and spikes, tie-heavy integers), together with what the reference's
compute_statistics.py itself prints and saves for those arrays.

compute_statistics.py is RUN, not restated: runpy executes the reference's file as __main__ in a temporary tree whose
configs/default.yaml points hp.data.data_dir at temporary energy / pitch / mels .npy files; its printed minima and maxima are parsed
from its output and e_mean.npy, e_std.npy, f0_mean.npy, f0_std.npy are read back.  Nothing of that tree is kept.  Two runs: the
energy-like arrays as energy with the F0-like arrays as pitch ("energy/", "f0/"), and the same energy with the tie-heavy arrays as
pitch ("ties/").  The script's energy loop has no guard for an utterance without a positive cleaned value (``e[e > 0].min()``
raises), so the energy directory holds only the energy-like utterances that keep one (every one but those whose quartiles coincide,
such as a single value); "energy/stats_index" lists them.  Its pitch loop has the guard (its bad_pitch list), so all pitch-like
utterances go in; "<kind>/stats_bad" is the length of that list.

The reference's third-party imports the path never uses are stubbed (librosa, tqdm as the identity).  The fixture holds arrays and
short key strings only.  It pins the FLOAT32 behaviour under the numpy that recorded it (printed below and stored as "numpy_version";
2.2.6 for the committed file): the reference's DIO pitch is float64 where ours is float32, and under numpy 1.x the scalar
``1.5 * (p75 - p25)`` of a float32 array was evaluated in float64, so other numpy generations may flag threshold ties differently.

TEST INFRASTRUCTURE ONLY.  Usage (in the build container, with the reference checked out):  python tools/gen_golden_targets.py [REFERENCE_DIR]
"""
import contextlib
import io
import os
import re
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PER_KIND, MAX_LEN, SEED = 16, 400, 12


def import_reference(ref):
    def stub(n, **a):
        m = types.ModuleType(n)
        m.__dict__.update(a)
        sys.modules[n] = m
        return m

    stub("librosa")
    stub("tqdm", tqdm=lambda it, *a, **k: it)
    sys.path.insert(0, ref)
    from utils.util import remove_outlier
    return remove_outlier


def run_compute_statistics(ref, energy, pitch):
    """What the reference's compute_statistics.py prints and saves for these energy and pitch arrays (lists of float32 arrays)."""
    with tempfile.TemporaryDirectory(prefix="g12_") as td:
        data = os.path.join(td, "data")
        os.makedirs(os.path.join(td, "configs"))
        for sub, arrs in (("energy", energy), ("pitch", pitch), ("mels", [np.zeros(1, np.float32)] * len(energy))):
            os.makedirs(os.path.join(data, sub))
            for i, a in enumerate(arrs):
                np.save(os.path.join(data, sub, "%04d.npy" % i), a)
        with open(os.path.join(td, "configs", "default.yaml"), "w") as f:
            f.write("data:\n  data_dir: '%s'\n" % data)
        cwd, out = os.getcwd(), io.StringIO()
        os.chdir(td)
        try:
            with contextlib.redirect_stdout(out):
                runpy.run_path(os.path.join(ref, "compute_statistics.py"), run_name="__main__")
        finally:
            os.chdir(cwd)
        printed = {k.strip(): float(v) for k, v in re.findall(r"^([A-Za-z ]+?)\s*:\s*([-+0-9.einfa]+)\s*$", out.getvalue(), re.M)}
        bad = int(re.search(r"bad Pitch Vectors is\s+(\d+)", out.getvalue()).group(1))
        saved = {k: np.load(os.path.join(data, k + ".npy")) for k in ("e_mean", "e_std", "f0_mean", "f0_std")}
    return printed, saved, bad


def main():
    from tests import targets_oracle as O           # (before the reference's directory joins sys.path: it has a tests package too)
    ref = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FS2_REFERENCE", "../reference"))
    remove_outlier = import_reference(ref)
    print("numpy", np.__version__)
    rng = np.random.default_rng(SEED)
    out = {"numpy_version": np.array(np.__version__)}
    inputs = {}
    for kind, make in O.KINDS:
        lens = [1, 2, 3, 4, 5, MAX_LEN] + [int(v) for v in rng.integers(6, MAX_LEN, N_PER_KIND - 6)]
        xs = [make(rng, n) for n in lens]
        ys = [remove_outlier(x.copy()) for x in xs]
        assert all(y.dtype == np.float32 for y in ys)
        inputs[kind] = xs
        out[kind + "/lens"] = np.asarray(lens, np.int32)
        out[kind + "/x"] = np.concatenate(xs)
        out[kind + "/y"] = np.concatenate(ys)
        out[kind + "/p25"] = np.asarray([np.percentile(x, 25) for x in xs], np.float32)
        out[kind + "/p75"] = np.asarray([np.percentile(x, 75) for x in xs], np.float32)
        mism = sum(not np.array_equal(O.clean(x).y, y) for x, y in zip(xs, ys))
        print("%-6s %d utterances, %d values, %d changed by the reference, oracle mismatches %d"
              % (kind, len(xs), out[kind + "/x"].size, int((out[kind + "/x"] != out[kind + "/y"]).sum()), mism))
    keep = [i for i, x in enumerate(inputs["energy"]) if (remove_outlier(x.copy()) > 0).any()]
    out["energy/stats_index"] = np.asarray(keep, np.int32)
    energy = [inputs["energy"][i] for i in keep]
    for kind in ("f0", "ties"):
        # (the script wants as many pitch files as energy files: the pitch-like kinds are cut or cycled to that number)
        pitch = [inputs[kind][i % len(inputs[kind])] for i in range(len(energy))]
        out[kind + "/stats_index"] = np.asarray([i % len(inputs[kind]) for i in range(len(energy))], np.int32)
        printed, saved, bad = run_compute_statistics(ref, energy, pitch)
        print(kind, printed, {k: float(v) for k, v in saved.items()}, "bad", bad)
        if kind == "f0":
            out["energy/stats_nonzero_min"] = np.float32(printed["Non zero Min Energy"])
            out["energy/stats_max"] = np.float32(printed["Max Energy"])
            out["energy/stats_mean"] = saved["e_mean"]
            out["energy/stats_std"] = saved["e_std"]
        out[kind + "/stats_min"] = np.float32(printed["Min Pitch"])
        out[kind + "/stats_nonzero_min"] = np.float32(printed["Non zero Min Pitch"])
        out[kind + "/stats_max"] = np.float32(printed["Max Pitch"])
        out[kind + "/stats_mean"] = saved["f0_mean"]
        out[kind + "/stats_std"] = saved["f0_std"]
        out[kind + "/stats_bad"] = np.int32(bad)
    path = os.path.join(ROOT, "tests", "golden", "g12_targets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
