"""GPU: bench.py contract (one JSON line; with --full also roofline + cpu_baseline) and the RCCL code path exercised on
a single GPU (1-rank nccl group, launched exactly as the driver launches N > 1)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only():
    """a plain run sets up, warms up, times the steps and prints the line: none of what --full adds"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"] == "utterances/sec per GAN train step, IEMOCAP tri-modal" and d["unit"] == "utterances/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 3 and d["value"] > 0
    for k in ("roofline", "roofline_families", "roofline_worst", "cpu_baseline", "profile"):
        assert k not in d, k
    assert "median_ms_per_step_synchronised" not in d["config"] and "gpu_over_cpu" not in d["config"]
    assert "cpu_baseline" not in r.stderr


def test_bench_default_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                        "--cpu-sample-batch", "2"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "f32" and d["vs_baseline"] is None
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    assert d["value"] > 50 * d["cpu_baseline"]["value"]          # north_star: >= 50x the host CPU
    assert d["config"]["synchronised_iterations"] == 20 and d["config"]["median_ms_per_step_synchronised"] > 0


def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """--dump-outputs writes what the last timed step computed (12 sub-step losses, the six networks' parameters) as float32
    within 64 MB; warm-up and timed steps start from the seeded initial state whatever the timing-dependent pre-roll ran,
    so two runs with the same arguments dump the same bits"""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--batch", "4",
                            "--seq", "20", "--no-cpu-baseline", "--step-only", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        assert _last_json(r.stdout)["steps"] == 3
        dumps.append({p.stem: np.load(str(p)) for p in sorted(out.glob("*.npy"))})
    a, b = dumps
    assert set(a) == {"losses"} | {"params_%s_%s" % (k, m) for k in "GD" for m in ("acoustic", "visual", "text")}
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["losses"].shape == (12,) and np.isfinite(a["losses"]).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_bench_rccl_path_on_one_rank():
    env = dict(os.environ, GANFFN_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", _free_port(), os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["config"]["launch"] == "eager" and d["config"]["parallelism"] == "dp1"
    assert all(0.1 < v < 5 for v in d["config"]["last_losses"].values())


@pytest.mark.parametrize("config", ["meld", "drnn"])
def test_bench_other_configs_on_the_rccl_path(config):
    """configs[2] (MELD widths) and configs[4] (GAN-FFN + DialogueRNN) through the same launcher and the 1-rank nccl
    group: the line keeps the contract's keys and, with --full, a roofline object"""
    env = dict(os.environ, GANFFN_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", _free_port(),
                        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--config", config], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step", "scaling", "dtype", "config", "roofline"):
        assert k in d, k
    assert d["value"] > 0 and d["config"]["parallelism"] == "dp1" and 0 < d["roofline"]["frac"] < 1


def test_data_parallel_path_costs_nothing_at_one_rank():
    """the N = 1 point of the scaling curve: the data-parallel code path (1-rank RCCL group: in-line all-reduce of every
    sub-step's gradient slab on the sub-step's own stream, one communicator per stream) against the plain engine, 3 streams,
    step only, best of two interleaved runs each.  Rounds 1-3 issued 4-5 asynchronous all-reduces per sub-step on the process
    group's internal stream: 18-75 % slower at one rank.  This is a correctness suite, so the gate here is COARSE (15 %: it
    catches that regression, not box noise); the precise A/B (-0.07 ... +0.35 % over ten boxes) is the recorded artefact
    profiles/r05_bench_dist1.json, written by tools/dist1_ab.sh."""
    def run(dist):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        if dist:
            env.update(GANFFN_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--step-only", "--steps", "10"],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return _last_json(r.stdout)["ms_per_step"]
    plain, dist1 = [], []
    for i in range(2):
        plain.append(run(False))
        dist1.append(run(True))
    assert min(dist1) <= 1.15 * min(plain), (plain, dist1)


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment must start N ranks ITSELF (replaces
    /root/reference/train_IEMOCAP.py:587-593).  One GPU here, so N = 1 through the very same path (--launcher spawn): the parent
    spawns the rank, the rank joins a 1-rank RCCL group, the parent relays ONE JSON line that records what ran."""
    env = dict(os.environ, GANFFN_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GANFFN_DP_MODE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--launcher", "spawn", "--gpus", "1", "--steps", "10", "--warmup", "2",
                        "--no-cpu-baseline", "--step-only"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    c = d["config"]
    assert c["launcher"]["spawned_ranks"] == 1 and c["launcher"]["rung"] == "inline-3streams" and c["launcher"]["fallback_from"] is None
    assert c["rccl_ranks"] == 1 and c["dp_mode"] == "inline" and c["communicators"] == 3 and c["streams"] == 3
    assert c["ms_per_step_min_max_over_ranks"][0] <= d["ms_per_step"] + 1e-3
    # and against the plain in-process line on the same box: the launcher path must not cost the step anything (coarse gate;
    # the recorded A/B is in profiles/r05_bench_dist1.json)
    env2 = {k: v for k, v in env.items() if k != "GANFFN_FORCE_DIST"}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "2", "--no-cpu-baseline", "--step-only"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env2)
    assert p.returncode == 0, p.stderr[-3000:]
    assert d["ms_per_step"] <= 1.15 * _last_json(p.stdout)["ms_per_step"]


def test_launcher_second_rung_runs_on_one_stream_and_one_communicator():
    """the fallback rungs are real configurations: rung 2 of the ladder (in-line all-reduce, ONE stream, ONE communicator) and
    rung 3 (bucket mode) on the 1-rank RCCL group — each must deliver a line and say what it was"""
    for rung, dp, comms, streams in (("1", "inline", 1, 1), ("2", "buckets", 1, 3)):
        env = dict(os.environ, GANFFN_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0", GANFFN_LAUNCH_RUNGS=rung)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GANFFN_DP_MODE"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--launcher", "spawn", "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--no-cpu-baseline", "--step-only"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        c = _last_json(r.stdout)["config"]
        assert c["dp_mode"] == dp and c["communicators"] == comms and c["streams"] == streams and c["rccl_ranks"] == 1, c


def test_two_rank_rehearsal_through_the_launcher():
    """every world > 1 line of bench.py end to end on a one-GPU box: `python bench.py --gpus 2` (no WORLD_SIZE) spawns two
    ranks that SHARE the GPU and reduce over gloo (GANFFN_DIST_BACKEND=gloo; RCCL refuses two ranks on one device) — the
    launcher, the rank-0 relay, the slab broadcast, the pre-roll's collective stop flag, the in-line all-reduce on three
    streams, MAX-over-ranks timing and the per-rank spread.  A rehearsal of the plumbing, not a measurement (the line says
    dist_backend = gloo)."""
    env = dict(os.environ, GANFFN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GANFFN_DP_MODE", "GANFFN_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--seq", "20", "--no-cpu-baseline", "--step-only"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    c = d["config"]
    assert d["n_gpus"] == 2 and c["launcher"]["spawned_ranks"] == 2 and c["launcher"]["rung"] == "inline-3streams"
    assert c["rccl_ranks"] == 2 and c["dist_backend"] == "gloo" and c["dp_mode"] == "inline" and c["streams"] == 3
    lo, hi = c["ms_per_step_min_max_over_ranks"]
    assert 0 < lo <= hi <= d["ms_per_step"] + 1e-3          # the line's time is the MAX over the ranks
    assert "[rank 1]" in r.stderr                             # the second rank really ran (its stderr is relayed)


def test_two_rank_rehearsal_under_torch_distributed_run():
    """the way the DRIVER starts N > 1: `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`.  Every rank
    torchrun starts becomes a supervisor that makes no GPU call and runs the real rank as its child (bench.supervise): the
    watchdog and the fallback ladder work here too.  Two ranks sharing the GPU over gloo (rehearsal backend); ONE JSON line, from
    rank 0, saying how it was launched."""
    env = dict(os.environ, GANFFN_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "GANFFN_DP_MODE", "GANFFN_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "4", "--seq", "20", "--no-cpu-baseline", "--step-only"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    c = d["config"]
    assert d["n_gpus"] == 2 and c["rccl_ranks"] == 2 and c["dist_backend"] == "gloo"
    assert c["launcher"]["rung"] == "inline-3streams" and c["launcher"]["spawned_ranks"] == 2 and "supervises" in c["launcher"]["how"]
