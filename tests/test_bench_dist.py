"""The N > 1 path of bench.py on CPU: two ranks over gloo run the same barrier / max-over-ranks
timing and whole-job aggregation that the GPU replicas use (inference shards nothing between
ranks: "replicas only")."""

import json
import os
import socket
import sys
import time
from pathlib import Path

import torch
import torch.distributed as dist
import pytest
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = {"n": 0}

    def step():
        calls["n"] += 1
        time.sleep(0.01 * (rank + 1))  # rank 1 is the slow one: the max over ranks must win

    def max_reduce(x):
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    elapsed = bench.timed_region(step, steps=5, warmup=2, sync_fn=lambda: None, barrier_fn=dist.barrier, max_reduce_fn=max_reduce)
    samples = 1000
    value = world * samples * 5 / elapsed
    Path(out_dir, f"rank{rank}.json").write_text(json.dumps({"elapsed": elapsed, "calls": calls["n"], "value": value}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_timing_and_aggregation(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [json.loads(Path(tmp_path, f"rank{i}.json").read_text()) for i in range(world)]
    assert r[0]["calls"] == r[1]["calls"] == 7  # W warm-up + exactly K timed steps
    assert r[0]["elapsed"] == r[1]["elapsed"]  # every rank reports the max over ranks
    assert r[0]["elapsed"] >= 5 * 0.02 * 0.9  # the slow rank (20 ms / step) sets the time
    assert abs(r[0]["value"] - 2 * 1000 * 5 / r[0]["elapsed"]) < 1e-6  # whole-job aggregate, not per-GPU


def _allreduce_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from everyvoice_amd.train.hifigan import allreduce_mean_

    flat = torch.arange(10, dtype=torch.float32) * (rank + 1)  # the optimiser's flat gradient buffer of this rank
    allreduce_mean_(flat, None, lambda t, s: t.mul_(s))        # CPU stand-in for the device scaling kernel
    torch.save(flat, Path(out_dir, f"g{rank}.pt"))
    dist.destroy_process_group()


def test_gradient_allreduce_is_a_mean_over_ranks(tmp_path):
    """The data-parallel exchange of the training step (one all-reduce per optimiser's flat gradient buffer)."""
    world = 2
    mp.spawn(_allreduce_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    g0, g1 = (torch.load(Path(tmp_path, f"g{i}.pt")) for i in range(world))
    want = torch.arange(10, dtype=torch.float32) * 1.5
    assert torch.equal(g0, g1) and torch.allclose(g0, want)


def _bucket_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from everyvoice_amd.train.hifigan import BucketReducer

    flat = torch.arange(23, dtype=torch.float32) * (rank + 1)
    red = BucketReducer(flat, None, lambda t, s: t.mul_(s))
    hi = flat.numel()
    for lo in (17, 9, 4):  # backward finishes the buffer suffix-first, bucket by bucket
        red.launch(lo, hi)
        hi = lo
    red.launch(0, hi)      # what is left in front of the first bucket
    red.launch(0, 0)       # empty ranges are ignored
    red.finish()
    torch.save(flat, Path(out_dir, f"b{rank}.pt"))
    dist.destroy_process_group()


def test_bucketed_overlapped_allreduce_is_a_mean_over_ranks(tmp_path):
    """The exchange the training step uses on N > 1 GPUs: asynchronous all-reduces of contiguous buckets launched during
    backward, one wait + 1/world scaling at the end (gloo stands in for RCCL; the side stream is GPU-only)."""
    world = 2
    mp.spawn(_bucket_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    b0, b1 = (torch.load(Path(tmp_path, f"b{i}.pt")) for i in range(world))
    assert torch.equal(b0, b1) and torch.allclose(b0, torch.arange(23, dtype=torch.float32) * 1.5)


class _RecordingReducer:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def launch(self, lo, hi):
        self.log.append((self.name, "launch", lo, hi))

    def finish(self):
        self.log.append((self.name, "finish"))


class _ScheduleHost:
    """What HiFiGANTrainer._data_parallel_schedule needs of a trainer, with phases that only write down that they ran."""

    MIN_G_BUCKET = 5

    def __init__(self, log):
        from types import SimpleNamespace

        self.log = log
        self._dp_reducers = (_RecordingReducer("d", log), _RecordingReducer("g", log))
        self.pg = True
        self.keep_grads = False
        self.d_params = SimpleNamespace(names=lambda: ["p"], offset_of=lambda n: 2)
        self.g_params = SimpleNamespace(grad=torch.zeros(20))

    def d_bucket_groups(self):
        return [[0, 1], [2]]

    def discriminators(self):
        from types import SimpleNamespace

        return [SimpleNamespace(layers=lambda i=i: [i]) for i in range(3)]

    @staticmethod
    def _bucket_range(group, layers):
        return 10 * min(layers) + 2, 10 * max(layers) + 12

    def _phase_generator_forward(self, step, mel, audio, d_step=True):
        self.log.append(("phase", "generator forward"))

    def _phase_d_prelude(self, step):
        self.log.append(("phase", "d prelude"))

    def _phase_d_group(self, step, idxs):
        self.log.append(("phase", "d group", tuple(idxs)))

    def _phase_d_epilogue(self, step):
        self.log.append(("phase", "d epilogue"))

    def _phase_d_update(self, step):
        self.log.append(("phase", "d update"))

    def _phase_g_backward(self, step, adversarial=True):
        self.log.append(("phase", "g backward"))
        stop = step.g_stop

        def segments():  # gradient ranges becoming final from the end of the buffer downwards; the schedule cuts where `stop` says so
            for lo, hi in ((17, 20), (14, 17), (8, 14), (6, 8), (3, 6)):
                if stop((lo, hi)):
                    yield (lo, hi)

        step.g_segments = segments()

    def _phase_g_update(self, step):
        self.log.append(("phase", "g update"))


def test_eager_and_captured_data_parallel_steps_issue_the_same_collectives():
    """VERDICT r04 item 5 / ADVICE r03: one collective schedule.  `HiFiGANTrainer._data_parallel_schedule` is what BOTH modes run -- the
    eager step calls every stretch and every exchange at once, the capture stores the exchanges and the replay loop calls them between
    the graphs -- so a rank that runs eagerly (new shape, failed capture) pairs its all-reduces with a replaying rank's one for one
    (the reference: every rank, the same DDP buckets: everyvoice/base_cli/helpers.py:252-270).  Host logic only: phases are stubs."""
    from everyvoice_amd.train.hifigan import HiFiGANTrainer, _Step

    for warm in (False, True):
        eager_log, cap_log = [], []
        host = _ScheduleHost(eager_log)
        HiFiGANTrainer._data_parallel_schedule(host, lambda fn: fn(), lambda then: then(), _Step(), None, None, warm)
        host = _ScheduleHost(cap_log)
        stored = []
        HiFiGANTrainer._data_parallel_schedule(host, lambda fn: (fn(), stored.append(None)), lambda then: stored.__setitem__(-1, then), _Step(), None, None, warm)
        n_capture_time = len(cap_log)
        assert not [e for e in cap_log if e[0] != "phase"], "a capture must not issue collectives"
        for then in stored:  # the replay loop: graph i, then its exchange
            if then is not None:
                then()
        collectives = lambda log: [e for e in log if e[0] != "phase"]  # noqa: E731
        assert collectives(eager_log) == collectives(cap_log[n_capture_time:]) and collectives(eager_log)
        assert [e for e in eager_log if e[0] == "phase"] == cap_log[:n_capture_time]
        if not warm:  # both discriminator groups, the front padding, then generator buckets of >= MIN_G_BUCKET gradients
            assert collectives(eager_log)[:4] == [("d", "launch", 2, 22), ("d", "launch", 22, 32), ("d", "launch", 0, 2), ("d", "finish")]
            assert collectives(eager_log)[4:] == [("g", "launch", 14, 20), ("g", "launch", 8, 14), ("g", "launch", 3, 8), ("g", "launch", 0, 3), ("g", "finish")]


def test_dist_env_and_roofline_aggregation(monkeypatch):
    monkeypatch.setenv("RANK", "3")
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "4")
    assert bench.dist_env() == (3, 1, 4)
    recs = [
        dict(kernel="a", layer="l0", ms=1.0, flops=2e9, bytes=1e6),
        dict(kernel="a", layer="l1", ms=3.0, flops=2e9, bytes=1e6),
        dict(kernel="b", layer="l2", ms=1.0, flops=1e9, bytes=4e6),
    ]
    roof = bench.roofline_from_records([recs, recs])
    assert roof["kernel"] == "a" and roof["launches_per_forward"] == 2
    assert abs(roof["avg_launch_ms"] - 2.0) < 1e-9  # median of (1, 3, 1, 3)
    assert abs(roof["achieved"] - 2e9 / 2e-3 / 1e12) < 1e-2  # algorithmic FLOP per launch / median duration
    assert roof["peak"] == 2500.0 and roof["bound"] == "mfma"
    assert abs(roof["frac"] - roof["achieved"] / 2500.0) < 1e-3
    assert abs(roof["whole_forward"]["event_ms"] - 5.0) < 1e-9


def test_roofline_block_survives_one_stretched_launch():
    """one launch of a small kernel read 21 ms on the driver's box and the 3-pass MEAN named it the dominant kernel at
    8x its rocprof time.  Medians over launches and passes do not move, and `measured_roofline` rejects the pass outright (its events
    do not add up to the timed step) and measures again."""
    def recs(stretch=1.0):
        return [dict(kernel="big", layer=f"l{i}", ms=0.56, flops=567e9, bytes=1e9) for i in range(6)] + \
               [dict(kernel="small", layer=f"s{i}", ms=0.34 * (stretch if i == 1 else 1.0), flops=50e9, bytes=1e8) for i in range(3)]
    clean = bench.roofline_from_records([recs()] * 5)
    dirty = bench.roofline_from_records([recs(), recs(60.0), recs(), recs(), recs()])
    for k in ("kernel", "avg_launch_ms", "frac", "launches_per_forward"):
        assert clean[k] == dirty[k], k
    assert clean["kernel"] == "big" and abs(clean["avg_launch_ms"] - 0.56) < 1e-9
    assert dirty["whole_forward"]["event_ms"] == clean["whole_forward"]["event_ms"]

    class Gen:
        def __init__(self, seq):
            self.seq = list(seq)

        def forward_profiled(self, mel):
            return None, recs(self.seq.pop(0))

    timed = 6 * 0.56 + 3 * 0.34
    roof = bench.measured_roofline(Gen([1.0, 60.0, 1.0, 1.0, 1.0, 1.0]), None, timed, 5)
    assert roof["check"] == {"event_ms": round(timed, 3), "timed_ms": round(timed, 3), "passes": 5, "rejected": 1, "tolerance": 0.1, "consistent": True}
    assert roof["kernel"] == "big"
    # a box that never agrees with its own timed region: the block says so instead of posing as evidence
    bad = bench.measured_roofline(Gen([60.0] * 40), None, timed, 5)
    assert bad["check"]["consistent"] is False and bad["check"]["rejected"] == 20


def test_bare_multi_gpu_command_launches_its_own_ranks(monkeypatch, capfd):
    """`python bench.py --gpus 2` with no launcher in the environment: the parent starts two ranks through
    torch.distributed.run, relays rank 0's JSON line and returns the children's exit code (--selftest-cpu replaces the GPU
    legs by a sleep and RCCL by gloo; the launcher path is the one the GPU run takes)."""
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    rc = bench.main(["--gpus", "2", "--steps", "3", "--warmup", "1", "--selftest-cpu"])
    out = capfd.readouterr().out
    assert rc == 0, out
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["steps"] == 3
    assert line["ms_per_step"] >= 4.0 * 0.9  # the slower rank (2 x 2 ms) sets the time


def test_rank_count_mismatch_is_a_hard_error(monkeypatch, capfd):
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    assert bench.main(["--gpus", "8", "--selftest-cpu"]) == 2
    assert "WORLD_SIZE=4" in capfd.readouterr().err


def test_plain_run_and_full_run_options():
    """A plain run measures the headline alone; --full adds the other legs; --steps is the exact count of timed steps (at least 1)."""
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_writes_float32_within_the_size_cap(tmp_path, monkeypatch):
    """--dump-outputs: DIR/<name>.npy in float32; a tensor past its share of the cap is written as a fixed strided sample."""
    import numpy as np

    small = torch.randn(2, 1, 300, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"wav": small})
    got = np.load(tmp_path / "d" / "wav.npy")
    assert got.dtype == np.float32 and got.shape == (2, 1, 300) and np.array_equal(got, small.float().numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 2 * 1000)
    big = torch.arange(3000, dtype=torch.float32).reshape(3, 1000)
    bench.dump_outputs(str(tmp_path / "e"), {"a": big, "b": big[:1, :10]})
    a, b = np.load(tmp_path / "e" / "a.npy"), np.load(tmp_path / "e" / "b.npy")
    assert a.nbytes + b.nbytes <= 2 * 1000 and a.dtype == np.float32
    assert np.array_equal(a, big.reshape(-1)[::12].numpy())  # 12000 bytes into a 1000-byte share: every 12th element
    assert np.array_equal(b, big[:1, :10].numpy())


def test_train_base_command_devices_2_over_gloo(tmp_path, monkeypatch):
    """``train_base_command(..., devices=2)`` outside a launcher starts one rank per device running the same command
    (base_cli/interfaces.py:84-97 -> Lightning's DDP launcher).  With CPU stand-ins for the three classes (tests/ddp_stub.py) over
    gloo this checks the driver's own part: the classes travel by qualified name (nested ones too), ``model_kwargs`` and the
    accelerator reach the ranks, every rank writes into ONE log directory, rank shards are disjoint and cover the data,
    validation is sharded and its mean agreed between ranks, and only rank 0 writes checkpoints."""
    import json
    import os
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    monkeypatch.chdir(root)
    monkeypatch.setenv("PYTHONPATH", str(root) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "EVMI_LOG_SUB_DIR"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, str(root))
    from everyvoice_amd.lightning import train_base_command
    from tests.ddp_stub import Outer, StubData, StubModel

    cfg = Outer.StubConfig(training=dict(batch_size=2, max_epochs=1, max_steps=100, val_check_interval=None, check_val_every_n_epoch=1, save_top_k_ckpts=1,
                                         logger=dict(save_dir=tmp_path / "logs", name="ddp")))
    (tmp_path / "cfg.json").write_text(json.dumps(cfg.model_dump(mode="json")))
    rc = train_base_command(Outer.StubConfig, StubData, StubModel, "validation/stub", [], tmp_path / "cfg.json", accelerator="cpu", devices=2,
                            model_kwargs={"scale": 3.0, "tag": "from-the-parent"})
    assert rc == 0
    runs = list((tmp_path / "logs" / "ddp" / "base").iterdir())
    assert len(runs) == 1 and (runs[0] / "hparams.yaml").exists()  # one <sub_dir> for both ranks
    rec = json.loads((tmp_path / "logs" / "rank0.json").read_text())
    assert not (tmp_path / "logs" / "rank1.json").exists()  # rank 0 alone saves checkpoints
    assert rec["world"] == 2 and rec["scale"] == 3.0 and rec["tag"] == "from-the-parent" and rec["process_group"] and rec["sub_dir"] == runs[0].name
    assert rec["seen"] == [0, 2, 4, 6] and rec["val_seen"] == [0, 2, 4]  # rank 0's shard of the data / of the validation batches
    assert rec["monitor"]["validation/stub"] == pytest.approx(3.0 * (0 + 1 + 2 + 3 + 4) / 5)  # mean over BOTH ranks' batches
    assert (runs[0] / "checkpoints" / "last.ckpt").exists() and (tmp_path / "logs" / "prepared.txt").read_text() == "rank 0\n"
    # a class defined inside a function cannot be found by the children: refused with a message, not a crash in N processes
    from everyvoice_amd.lightning import _resolve_class

    assert _resolve_class("tests.ddp_stub:Outer.StubConfig") is Outer.StubConfig
    with pytest.raises(ValueError, match="module level"):
        _resolve_class("tests.ddp_stub:f.<locals>.C")
    with pytest.raises(TypeError, match="JSON"):
        train_base_command(Outer.StubConfig, StubData, StubModel, "validation/stub", [], tmp_path / "cfg.json", accelerator="cpu", devices=2,
                           model_kwargs={"process_group": object()})
