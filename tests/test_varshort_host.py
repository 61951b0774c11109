"""Host-side checks of the variance predictors on short rows (FS2_VARSHORT; no GPU).

csrc/layout_rule.h -- K, the short duration of a phoneme, the map from a frame's offset to its short offset, the bound on the short rows --
compiled with the host compiler (tests/varshort_probe.cpp) and compared with the rule restated here, in Python, without looking at the header:

  K           1 + the sum over the predictor's layers of (kernel - 1): 5 for two k = 3 layers;
  short       min(d, K) frames of a phoneme of d;
  map         d <= K: o -> o.  d > K, K = 5: o -> o for o < 2, o -> K - (d - o) for o >= d - 2, o -> 2 otherwise (general K: 2 is (K - 1) / 2);
  bound       row_bound(min(frame bound, K x phonemes), utterances), row_bound(f, u) = min(f + 16 u + 8, 2^31 - 1 - 256);
  layout      the gapped-row walk over the short lengths: row = gap; start = row rounded up to 8; row = start + len + gap; rows = row + 8.

And the property everything rests on, in numpy float64: a stack of two k = 3 convolutions, each followed by ReLU and LayerNorm, run on the length
regulator's output with every duration clipped to K gives, at the mapped frames, the values the full sequence gives."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")
EDGE_D = (0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 20, 40)


def up(x, a):
    return -(-x // a) * a


def window(kernels):
    return 1 + sum(k - 1 for k in kernels)


def short_dur(d, K):
    return min(d, K)


def short_offset(o, d, K):
    h = (K - 1) // 2
    if d <= K or o < h:
        return o
    return K - (d - o) if o >= d - h else h


def row_bound(frames, utts):
    return min(frames + utts * 16 + 8, 2 ** 31 - 1 - 256)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("varshort") / "probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "varshort_probe.cpp"), "-o", exe], check=True)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (args, r.stdout[-500:], r.stderr[-500:])
        return [line.split() for line in r.stdout.splitlines()]
    return run


def test_rule_header_is_plain_cpp():
    src = open(os.path.join(CSRC, "layout_rule.h")).read()
    for word in ("__global__", "__shared__", "hipLaunch", "hipStream", "hipError", "threadIdx", "blockIdx"):
        assert word not in src, word
    assert subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", CSRC, "-include", os.path.join(CSRC, "layout_rule.h"), os.devnull]).returncode == 0


def test_window(probe):
    assert probe("window", 2, 3) == [["window", "5"]]
    for layers in (1, 2, 3, 5):
        for k in (1, 3, 5, 9):
            assert int(probe("window", layers, k)[0][1]) == window([k] * layers)


def test_the_map_as_the_issue_states_it_for_k5(probe):
    """K = 5, written out with the literal 2s: first two frames, last two frames, everything between them the interior frame."""
    K = 5
    for line in probe("map", K, *range(0, 48)):
        d, s, offs = int(line[1]), int(line[3]), [int(x) for x in line[5:]]
        assert s == min(d, 5) and len(offs) == d
        for o, got in enumerate(offs):
            want = o if d <= K else (o if o < 2 else (K - (d - o) if o >= d - 2 else 2))
            assert got == want, (d, o, got, want)
        assert sorted(set(offs)) == list(range(s))                  # every short frame is some frame's image, none beyond
        assert offs == sorted(offs)                                 # and the map is monotone


@pytest.mark.parametrize("K", [1, 3, 5, 7, 9])
def test_short_durations_and_map_random_and_edges(probe, K):
    rs = np.random.RandomState(K)
    ds = list(EDGE_D) + rs.randint(0, 60, size=40).tolist() + [K - 1, K, K + 1, 2 * K, 1000]
    for line, d in zip(probe("map", K, *ds), ds):
        assert int(line[1]) == d and int(line[3]) == short_dur(max(d, 0), K)
        assert [int(x) for x in line[5:]] == [short_offset(o, d, K) for o in range(d)], (K, d)


def test_row_bound(probe):
    rs = np.random.RandomState(3)
    cases = [(1, 1, 1, 5), (100, 10, 2, 5), (40, 10, 2, 5), (50, 10, 2, 5), (2 ** 31 - 1, 2 ** 28, 64, 5), (10 ** 12, 10 ** 12, 4096, 5)]
    cases += [(int(f), int(p), int(u), int(k)) for f, p, u, k in zip(rs.randint(1, 10 ** 6, 30), rs.randint(1, 10 ** 5, 30), rs.randint(1, 300, 30), rs.choice([1, 3, 5, 9], 30))]
    for frames, phon, utts, K in cases:
        assert int(probe("bound", frames, phon, utts, K)[0][1]) == row_bound(min(frames, K * phon), utts), (frames, phon, utts, K)


def _random_utterances(rs, B):
    return [[int(rs.choice(EDGE_D)) for _ in range(int(rs.randint(1, 12)))] for _ in range(B)]


@pytest.mark.parametrize("gap", [4, 8])
def test_short_layout_and_frame_map(probe, gap):
    """The short layout -- layout_rule.h's row walk over the short lengths -- and the short row of every frame, against the docstring's rule;
    the short rows never exceed the bound, nor the rows the frames themselves take."""
    K = 5
    rs = np.random.RandomState(17 + gap)
    batches = [[[0, 40, 0]], [[1]], [[1] * 9, [40] * 3, [0, 12, 0, 7, 0]], [[0, 0, 0]]] + [_random_utterances(rs, B) for B in (1, 2, 3, 4, 9, 33)]
    for utts in batches:
        args = []
        for i, u in enumerate(utts):
            args += (["/"] if i else []) + u
        out = probe("layout", gap, K, *args)
        row, frow, start, ln = gap, gap, [], []
        for u in utts:
            row, frow = up(row, 8), up(frow, 8)
            start.append(row)
            ln.append(sum(min(d, K) for d in u))
            row += ln[-1] + gap
            frow += sum(u) + gap
        assert [int(x) for x in out[0][1:]] == start and [int(x) for x in out[1][1:]] == ln, utts
        assert int(out[2][1]) == row + 8
        assert row + 8 <= row_bound(min(sum(map(sum, utts)), K * sum(map(len, utts))), len(utts)) and row <= frow
        for b, u in enumerate(utts):
            want, s0 = [], 0
            for d in u:
                want += [start[b] + s0 + short_offset(o, d, K) for o in range(d)]
                s0 += min(d, K)
            assert [int(x) for x in out[3 + b][1:]] == want, (utts, b)
            assert all(start[b] <= r < start[b] + ln[b] for r in want)


def _conv_relu_ln(x, w, b, g, beta):
    """x [L, C] -> LayerNorm(ReLU(conv1d(x, w [N, C, 3], zero padding 1) + b)) over the channels, eps 1e-12: one layer of the predictor."""
    L = x.shape[0]
    xp = np.concatenate([np.zeros((1, x.shape[1])), x, np.zeros((1, x.shape[1]))])
    y = sum(xp[t:t + L] @ w[:, :, t].T for t in range(3)) + b
    y = np.maximum(y, 0.0)
    mu = y.mean(1, keepdims=True)
    var = ((y - mu) ** 2).mean(1, keepdims=True)
    return (y - mu) / np.sqrt(var + 1e-12) * g + beta


def test_two_layer_stack_on_clipped_durations_equals_the_full_one_at_the_mapped_frames(probe):
    """200 random cases in float64: tokens [T, 8], two k = 3 layers 8 -> 6 -> 6, durations from {0, .., 7, 9, 20}.  The frame-to-short map is the
    header's (the probe's), so the property is checked for the rule the kernels apply."""
    rs = np.random.RandomState(0)
    K, worst = 5, 0.0
    for case in range(200):
        T = int(rs.randint(1, 10))
        d = rs.choice([0, 1, 2, 3, 4, 5, 6, 7, 9, 20], size=T)
        if d.sum() == 0:
            d[int(rs.randint(T))] = int(rs.choice([1, 6, 20]))
        tok = rs.randn(T, 8)
        w0, b0, w1, b1 = rs.randn(6, 8, 3), rs.randn(6), rs.randn(6, 6, 3), rs.randn(6)
        g0, be0, g1, be1 = rs.randn(6), rs.randn(6), rs.randn(6), rs.randn(6)
        stack = lambda x: _conv_relu_ln(_conv_relu_ln(x, w0, b0, g0, be0), w1, b1, g1, be1)      # noqa: E731
        full = stack(np.repeat(tok, d, axis=0))
        short = stack(np.repeat(tok, np.minimum(d, K), axis=0))
        out = probe("layout", 0, K, *d.tolist())
        start, f2s = int(out[0][1]), [int(x) for x in out[3][1:]]
        assert len(f2s) == full.shape[0] and short.shape[0] == int(out[1][1])
        err = float(np.abs(full - short[np.asarray(f2s) - start]).max())
        worst = max(worst, err)
        assert err <= 1e-12, (case, d.tolist(), err)
    print("two-layer stack, clipped against full at the mapped frames: worst max-abs %.2e over 200 cases" % worst)
