"""CPU, world_size 2 (and 3), gloo: the N>1 path -- cost-balanced utterance sharding (LPT: shards of UNEQUAL size, possibly
empty), the one-collective sync-free gather of capacity packs (`gather_shards`), the host-driven gathers, order restoration --
with a stand-in per-utterance compute function that honours the real `inference_batch` contract.  The exact same code runs
over RCCL/xGMI on the GPU box (backend "nccl"); sharded == unsharded must hold bit-for-bit."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ODIM = 8


def _fake_run_local(xs, ilens, **kw):
    """Deterministic per-utterance 'mel': depends only on that utterance's ids (like the real path)."""
    B = xs.shape[0]
    ol = torch.tensor([int(xs[b, : int(ilens[b])].sum() % 37) + 5 for b in range(B)], dtype=torch.int64)
    Lmax = int(ol.max()) if B else 1
    mel = torch.zeros(B, Lmax, ODIM)
    for b in range(B):
        L = int(ol[b])
        base = xs[b, : int(ilens[b])].float().mean()
        mel[b, :L] = base + torch.arange(L * ODIM, dtype=torch.float32).view(L, ODIM) * 0.01
    return mel, ol


class _Async(tuple):
    def ok(self):
        return True


class FakeModel:
    """`FeedForwardTransformer.inference_batch` contract on the CPU: sync form -> (packed [sum L, odim], olens host);
    sync=False form -> ([row_capacity, odim] pack with the valid frames first and garbage behind, olens 'device' tensor)."""
    odim = ODIM
    _frames_per_token = None
    _overflow_seen = False
    overflow_next = False        # test hook: the next sync-free call behaves like a capacity overflow (NaN pack, flagged)
    regimes = None               # every `regime` a call was given (ShardedSynthesizer names the WHOLE batch on every rank)

    def async_ok(self):
        ok = not self._overflow_seen
        self._overflow_seen = False
        return ok

    def inference_batch(self, xs, ilens, packed=False, sync=True, capacity=None, alpha=1.0, regime=None):
        from fastspeech2_amd.parallel import row_capacity
        assert packed and xs.shape[0] == len(ilens) > 0, "the synthesizer must not call the model with an empty shard"
        self.regimes = (self.regimes or []) + [regime]
        mel, ol = _fake_run_local(xs, ilens)
        if alpha != 1.0:         # duration scale: every utterance gets round(L * alpha) frames (its first frame repeated behind)
            ol2 = torch.round(ol.float() * alpha).long()
            m2 = torch.zeros(mel.shape[0], int(ol2.max()), ODIM)
            for b in range(len(ol)):
                n = min(int(ol[b]), int(ol2[b]))
                m2[b, :n] = mel[b, :n]
                m2[b, n:int(ol2[b])] = mel[b, 0]
            mel, ol = m2, ol2
        valid = torch.cat([mel[i, : int(ol[i])] for i in range(len(ol))])
        il = torch.as_tensor(ilens)
        if sync:
            self._frames_per_token = (float(ol.sum()) / float(il.sum()), float((ol.float() / il.float()).max()))
            return valid, ol
        rows = row_capacity(len(ol), capacity[0])
        assert valid.shape[0] <= rows and int(ol.max()) <= capacity[1], "capacities from ShardedSynthesizer.capacities() too small"
        pk = torch.full((rows, ODIM), float("nan"))          # rows beyond the valid frames must never be read
        if self.overflow_next:
            self.overflow_next, self._overflow_seen = False, True
            return _Async((pk, ol.clone()))
        pk[: valid.shape[0]] = valid
        return _Async((pk, ol.clone()))


class FakeModelR2(FakeModel):
    """The same contract at reduction_factor = 2: every decoder frame yields two (identical) mel frames; `olens` and the packs count
    MEL frames, the capacities handed in by ShardedSynthesizer and the learned frames-per-phoneme ratio count DECODER frames."""
    reduction_factor = 2

    def inference_batch(self, xs, ilens, packed=False, sync=True, capacity=None, alpha=1.0, regime=None):
        from fastspeech2_amd.parallel import row_capacity
        assert packed and alpha == 1.0 and regime is not None and regime[1] >= len(ilens) and regime[0] >= int(torch.as_tensor(ilens).sum())
        mel, ol = _fake_run_local(xs, ilens)
        valid = torch.cat([mel[i, : int(ol[i])].repeat_interleave(2, dim=0) for i in range(len(ol))])
        il = torch.as_tensor(ilens)
        if sync:
            self._frames_per_token = (float(ol.sum()) / float(il.sum()), float((ol.float() / il.float()).max()))
            return valid, 2 * ol
        rows = 2 * row_capacity(len(ol), capacity[0])
        assert valid.shape[0] <= rows and int(ol.max()) <= capacity[1], "capacities (decoder frames) too small"
        pk = torch.full((rows, ODIM), float("nan"))
        pk[: valid.shape[0]] = valid
        return _Async((pk, 2 * ol))


def _make_inputs(B=11):
    g = torch.Generator().manual_seed(7)
    il = torch.randint(3, 40, (B,), generator=g)
    xs = torch.zeros(B, int(il.max()), dtype=torch.int64)
    for b in range(B):
        xs[b, : il[b]] = torch.randint(1, 68, (int(il[b]),), generator=g)
    return xs, il


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastspeech2_amd.parallel import ShardedSynthesizer, shard_indices, gather_packed
    xs, il = _make_inputs()
    want_mel, want_ol = _fake_run_local(xs, il)
    L = want_mel.shape[1]
    # (1) generic callable form: ragged padded batches, host-driven gather
    mel, ol = ShardedSynthesizer(_fake_run_local)(xs, il)
    assert torch.equal(ol, want_ol) and torch.equal(mel, want_mel)
    # (2) packed host-driven form
    parts = shard_indices(il.tolist(), world)
    assert len({len(p) for p in parts}) > 1 or world == 1, "the test batch should give shards of unequal size: %s" % parts
    mine = parts[rank]
    sel = torch.as_tensor(mine, dtype=torch.int64)
    m_loc, ol_loc = _fake_run_local(xs[sel][:, : int(il[sel].max())], il[sel])
    packed = torch.cat([m_loc[i, : int(ol_loc[i])] for i in range(len(mine))])
    mel2, ol2 = gather_packed(packed, ol_loc, mine, xs.shape[0])
    assert torch.equal(ol2, want_ol) and torch.equal(mel2, want_mel[:, : mel2.shape[1]])
    # (3) the production form: model object, first call synchronous (learns + agrees on the ratio), second call sync-free
    #     with ONE collective (gather_shards) over LPT shards of unequal size
    synth = ShardedSynthesizer(FakeModel())
    mel3, ol3 = synth(xs, il)
    assert torch.equal(ol3, want_ol) and torch.equal(mel3[:, :L], want_mel)
    mel4, ol4 = synth(xs, il)
    assert synth.ok()
    assert torch.equal(ol4, want_ol) and torch.equal(mel4[:, :L], want_mel) and float(mel4[:, L:].abs().sum()) == 0.0
    assert not torch.isnan(mel4).any()
    # every call named the WHOLE batch as the basis of the kernel-variant choice (sharded == unsharded bit for bit on the real model)
    if mine:
        assert synth.model.regimes == [(int(il.sum()), int(il.numel()))] * 2, synth.model.regimes
    local = ShardedSynthesizer(FakeModel(), global_regime=False)
    local(xs, il)
    assert not mine or local.model.regimes == [None]
    # (3b) packed return form: no padded [B, Lcap, odim] tensor, frames are read in place from the gathered packs
    recv, starts, ol5 = synth(xs, il, packed=True)
    assert torch.equal(ol5, want_ol)
    for g in range(xs.shape[0]):
        s0, n = int(starts[g]), int(ol5[g])
        assert torch.equal(recv[s0:s0 + n], want_mel[g, :n])
    # (3c) ok() is cumulative: an overflow on ONE rank in an EARLIER call is still reported after a later good call, once
    if rank == world - 1:
        synth.model.overflow_next = True
    synth(xs, il)
    synth(xs, il)
    assert not synth.ok() and synth.ok()
    # (3d) duration scale: the capacities follow alpha (1.6x the frames would overflow capacities sized for alpha = 1)
    m6, o6 = synth(xs, il, alpha=1.6)
    assert synth.ok() and torch.equal(o6, torch.round(want_ol.float() * 1.6).long()) and not torch.isnan(m6).any()
    try:
        synth(xs, il, alpha=0.0)
        raise AssertionError("alpha = 0 must be rejected")
    except ValueError:
        pass
    # (3e) reduction_factor = 2: capacities in decoder frames, packs / results / olens in mel frames (two per decoder frame)
    synth2 = ShardedSynthesizer(FakeModelR2())
    want2 = want_mel.repeat_interleave(2, dim=1)
    for _ in range(2):          # synchronous first call, then the sync-free one
        m7, o7 = synth2(xs, il)
        assert synth2.ok() and torch.equal(o7, 2 * want_ol) and torch.equal(m7[:, : 2 * L], want2) and not torch.isnan(m7).any()
    recv7, st7, o7p = synth2(xs, il, packed=True)
    for g in range(xs.shape[0]):
        s0, n = int(st7[g]), int(o7p[g])
        assert n == 2 * int(want_ol[g]) and torch.equal(recv7[s0:s0 + n], want2[g, :n])
    # (4) fewer utterances than ranks: some rank has an EMPTY shard and still takes part in the collectives
    for form in (ShardedSynthesizer(_fake_run_local), synth):
        for _ in range(2):
            m1, o1 = form(xs[:1], il[:1])
            assert torch.equal(o1, want_ol[:1]) and torch.equal(m1[:, : int(want_ol[0])], want_mel[:1, : int(want_ol[0])])
    # (numpy, not torch tensors: a tensor on an mp.Queue travels as a file descriptor the RECEIVER fetches from the sender's resource
    #  sharer -- if this process has exited by then the parent's q.get() fails with FileNotFoundError, which it did once in ~30 runs)
    q.put((rank, mel4[:, :L].numpy().copy(), ol4.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def _run_world(world):
    xs, il = _make_inputs()
    want_mel, want_ol = _fake_run_local(xs, il)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, mel, ol in got:
        assert torch.equal(torch.from_numpy(ol), want_ol) and torch.equal(torch.from_numpy(mel), want_mel)


def test_sharded_equals_unsharded_gloo():
    from fastspeech2_amd.parallel import shard_indices
    _run_world(2)
    xs, il = _make_inputs()
    parts = shard_indices(il.tolist(), 2)
    assert sorted(parts[0] + parts[1]) == list(range(xs.shape[0])) and parts[0] and parts[1]


def test_sharded_equals_unsharded_gloo_three_ranks():
    _run_world(3)


def test_meta_rows_hold_int64_counts_for_any_width():
    from fastspeech2_amd.parallel import meta_rows
    for odim in (1, 3, 7, 8, 80, 81):
        for bmax in (1, 2, 5, 128):
            r = meta_rows(bmax, odim)
            assert r * odim * 4 >= 8 * bmax and (r * odim) % 2 == 0, (odim, bmax, r)
    assert meta_rows(128, 80) == 4


def test_shard_balance():
    from fastspeech2_amd.parallel import shard_indices, utterance_cost
    il = [16 + (i * 37) % 160 for i in range(128)]
    parts = shard_indices(il, 8)
    loads = [sum(utterance_cost(il[i]) for i in p) for p in parts]
    assert max(loads) / (sum(loads) / 8) < 1.05      # LPT keeps the heaviest rank within 5 % of the mean


def test_c5_partition_is_balanced():
    """BASELINE config c5: 1024 LJSpeech-shape utterances over 8 ranks -> every rank within 1 % of the mean cost."""
    from fastspeech2_amd.parallel import shard_indices, utterance_cost
    from fastspeech2_amd.synthetic import make_batch
    il = make_batch("c5")["ilens"].tolist()
    parts = shard_indices(il, 8)
    assert sorted(sum(parts, [])) == list(range(1024))
    loads = [sum(utterance_cost(il[i]) for i in p) for p in parts]
    assert max(loads) / (sum(loads) / 8) < 1.01


def test_bench_self_launches_its_ranks_when_started_as_a_plain_command():
    """`python bench.py --gpus 2` with no launcher (no WORLD_SIZE): the script re-launches itself under torch.distributed.run with two
    ranks on 127.0.0.1 and a free port, and exactly ONE JSON line comes back on stdout (the only unmeasured row of the
    survey depended on a launch convention).  FS2_BENCH_FAKE=1 swaps the GPU model for the stand-in of this file over gloo; the
    launch, sharding, collective and printing code is the real one."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["FS2_BENCH_FAKE"] = "1"
    for extra in ([], ["--padded"]):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"] + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        rec = json.loads(lines[0])
        assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["value"] > 0
        assert rec["config"]["gather"] == ("padded" if extra else "packed")


def test_bench_relaunch_command_shape():
    import bench
    cmd = bench.relaunch_command(["--gpus", "8", "--steps", "3"], 8)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"] and cmd[-5].endswith("bench.py")


def _fake_bench(args, out_dir):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["FS2_BENCH_FAKE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dump-outputs", str(out_dir)] + args,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_hold_the_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR` writes what the timed path's caller received from its last step: `olens` and the packed gather's valid
    frames in utterance order (`mel_packed`; the capacity rows behind them are cut) or, with --padded, the padded mels cut at the longest
    utterance; float32 / float64 only.  The inputs depend on the arguments alone, so runs with other step counts dump the same arrays, and the
    two gather forms hold the same frames.  The line carries `ms_per_step` and `steps` as given."""
    import numpy as np
    rec = _fake_bench(["--steps", "3", "--warmup", "1"], tmp_path / "a")
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    _fake_bench(["--steps", "1", "--warmup", "2"], tmp_path / "b")
    _fake_bench(["--steps", "2", "--warmup", "1", "--padded"], tmp_path / "p")
    assert sorted(os.listdir(tmp_path / "a")) == ["mel_packed.npy", "olens.npy"]
    assert sorted(os.listdir(tmp_path / "p")) == ["mel.npy", "olens.npy"]
    ol, packed = np.load(tmp_path / "a" / "olens.npy"), np.load(tmp_path / "a" / "mel_packed.npy")
    assert ol.dtype == np.float64 and packed.dtype == np.float32
    assert packed.shape == (int(ol.sum()), ODIM) and np.isfinite(packed).all()
    for name in ("olens.npy", "mel_packed.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
    padded = np.load(tmp_path / "p" / "mel.npy")
    assert np.array_equal(np.load(tmp_path / "p" / "olens.npy"), ol) and padded.shape == (len(ol), int(ol.max()), ODIM)
    assert np.array_equal(np.concatenate([padded[b, : int(n)] for b, n in enumerate(ol)]), packed)
    xs, il = _make_inputs(B=4 * 2 + 3)                  # (fake_main's batch at world size 2)
    mel, ol_ref = _fake_run_local(xs, il)
    assert np.array_equal(ol, ol_ref.double().numpy()) and np.array_equal(padded, mel.numpy())


def test_bench_dump_outputs_keep_to_the_budget(tmp_path):
    """An output beyond the 64 MB budget is cut to a fixed sample of its rows (the same rows on every call), whose row numbers are written
    beside it; what fits is written whole; integer arrays become float64."""
    import numpy as np
    import bench
    big = torch.arange(300 * 1000 * 80, dtype=torch.float32).view(300, 1000, 80)          # 96 MB
    small = torch.arange(300, dtype=torch.int64)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"mel": big, "olens": small})
    files = sorted(os.listdir(tmp_path / "x"))
    assert files == ["mel.npy", "mel_rows.npy", "olens.npy"]
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in files) <= bench.DUMP_BUDGET_BYTES
    for f in files:
        assert np.array_equal(np.load(tmp_path / "x" / f), np.load(tmp_path / "y" / f)), f
    rows, mel = np.load(tmp_path / "x" / "mel_rows.npy"), np.load(tmp_path / "x" / "mel.npy")
    assert rows.dtype == np.float64 and mel.dtype == np.float32 and mel.shape == (len(rows), 80) and len(rows) > 100000
    assert np.array_equal(mel, big.view(-1, 80).numpy()[rows.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "x" / "olens.npy"), small.double().numpy())
