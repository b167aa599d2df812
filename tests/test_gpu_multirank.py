"""Multi-rank rehearsals of bench.py on the ONE GPU of the box.  This module sorts before test_gpu_parity.py on purpose: its tests start
child processes that each open the GPU, the box admits at most six such processes at a time, and this pytest process has not touched
the GPU yet when they run (nothing here does).  Eight GPU processes (BASELINE configs[4] as stated) are therefore out of reach of any test
that runs on this pool: the eight-rank SHAPE is covered by tests/test_distributed_cpu.py::test_eight_rank_shape_of_configs4 (gloo, CPU)
and by test_gpu_parity.py::test_configs4_eight_shards_on_one_gpu (the eight slabs through the HIP engine one after the other); here the
10 M-ballot batch is split over FOUR ranks."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _env(env_extra=None):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return env


def _run(nproc, extra, env_extra=None, timeout=1100, script="bench.py"):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(29900 + os.getpid() % 90), str(ROOT / script), "--gpus", str(nproc), *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=_env(env_extra), cwd=str(ROOT))


def _run_bare(extra, env_extra=None, timeout=900):
    """bench.py started the way the driver starts it at N = 1 (`python3 bench.py --gpus N ...`, no launcher)."""
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *extra], capture_output=True, text=True, timeout=timeout,
                          env=_env(env_extra), cwd=str(ROOT))


def test_bench_started_bare_launches_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` with no launcher and no WORLD_SIZE: bench.py starts the two ranks itself as a child
    torch.distributed.run (before it has touched the GPU), the child's one JSON line is the last line of stdout, exit code 0
    (VERDICT r4 task 1; the loop over voters of examples/voting.rs:199-203 cut into N slabs)."""
    r = _run_bare(["--full", "--gpus", "2", "--rehearse-one-gpu", "--steps", "1", "--warmup", "0", "--ballots", "20000", "--cpu-seconds", "1",
                   "--selfbench-seconds", "0.5"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().splitlines()
    lines = [l for l in out if l.startswith("{")]
    assert len(lines) == 1 and out[-1] == lines[0], out[-5:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 1 and line["warmup"] == 0 and line["scaling"] == "weak"
    assert line["config"]["tally_exchange_ok"] is True and line["config"]["parallelism"] == "shard2"
    assert line["config"]["accepted"] == 40000 and line["value"] > 1e4
    assert "starting the ranks as a child" in r.stderr
    # the line explains itself (VERDICT r5 task 1): one entry per rank, the exchange timed on its own, the CPU path in the same run, and the
    # host-staging legs run on both ranks at the same time
    assert [p["rank"] for p in line["per_rank"]] == [0, 1] and all(p["accepted"] == 20000 and p["ms_per_step"] > 0 for p in line["per_rank"])
    assert line["exchange"]["us_per_step"] > 0 and line["exchange"]["bytes_per_rank"] == 320 and line["slowest_rank"] in (0, 1)
    assert line["cpu_baseline"]["verdicts_match_gpu"] is True
    assert line["host_inclusive"]["all_ranks"]["ranks"] == 2 and line["host_inclusive"]["all_ranks"]["verdicts_match_device_path"] is True
    assert line["json_inclusive"]["all_ranks"]["ranks"] == 2 and line["json_inclusive"]["all_ranks"]["verdicts_match_device_path"] is True


def test_bench_started_bare_refuses_more_gpus_than_the_node_has():
    """Without --rehearse-one-gpu the bare form asks for N real devices: on this one-GPU box `--gpus 2` ends with a message and exit
    code 2 before any rank is started (torch.cuda.device_count() does not initialise the runtime)."""
    r = _run_bare(["--gpus", "2", "--steps", "1", "--warmup", "0", "--ballots", "20000"], timeout=300)
    assert r.returncode == 2 and "FATAL" in r.stderr and "GPU(s)" in r.stderr
    assert not [l for l in r.stdout.strip().splitlines() if l.startswith("{")]


def test_bench_spawned_single_rank_goes_through_the_bare_launch_path_over_rccl():
    """VERDICT r5 task 5: the NON-rehearsed launch path on hardware, every round - `python3 bench.py --gpus 1 --force-dist --spawn`: the
    parent counts the GPUs from the KFD topology in sysfs (no HIP call before the spawn), starts the rank as a child
    `python -m torch.distributed.run`, the rank initialises RCCL (backend nccl, world size 1), runs the preflight all-gather and the
    steps, and prints ONE line with tally_exchange_ok (examples/voting.rs:199-203 is the loop the slabs stand in for).  A second
    invocation asks for one GPU more than HIP_VISIBLE_DEVICES leaves visible: refused with exit code 2 before any rank starts."""
    r = _run_bare(["--full", "--gpus", "1", "--force-dist", "--spawn", "--steps", "1", "--warmup", "0", "--ballots", "20000",
                   "--selfbench-seconds", "0.5", "--cpu-seconds", "1", "--no-extra-configs"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().splitlines()
    lines = [l for l in out if l.startswith("{")]
    assert len(lines) == 1 and out[-1] == lines[0], out[-5:]
    line = json.loads(lines[0])
    assert "starting the ranks as a child" in r.stderr and "cannot count" not in r.stderr
    assert line["n_gpus"] == 1 and line["config"]["tally_exchange_ok"] is True and line["config"]["accepted"] == 20000
    assert len(line["per_rank"]) == 1 and line["per_rank"][0]["accepted"] == 20000 and line["exchange"]["us_per_step"] > 0
    assert line["cpu_baseline"]["verdicts_match_gpu"] is True
    r = _run_bare(["--gpus", "2", "--steps", "1", "--warmup", "0", "--ballots", "20000"], {"HIP_VISIBLE_DEVICES": "0"}, timeout=300)
    assert r.returncode == 2 and "FATAL" in r.stderr and "shows 1 GPU(s)" in r.stderr


def test_bench_in_process_devices_rehearsed():
    """`bench.py --in-process-devices 3`: the step of the ranked path through ONE process - three contexts (all on device 0 here), one
    resident slab and one stream each, eg_verify_*_batch_multi_device, the running tallies merged by eg_*_tally_encode_multi; the merged
    tally is also the running tally of one engine that verified every slab (VERDICT r4 task 6c; examples/voting.rs:179-213 is one
    process).  Weak (3 x 30 000, 1 % tampered) and strong (100 001 ballots cut in three)."""
    for extra, total, tampered in ((["--ballots", "30000", "--tampered-percent", "1"], 90000, 900),
                                   (["--total-ballots", "100001", "--workload", "qv"], 100001, 0)):
        r = _run_bare(["--full", "--in-process-devices", "3", "--rehearse-one-gpu", "--steps", "2", "--warmup", "1", *extra],
                      {"EG_CHUNK": "32768", "EG_COMB_BIG_BITS": "0"})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        cfg = line["config"]
        assert line["n_gpus"] == 3 and cfg["parallelism"] == "in-process3-on-one-gpu" and cfg["devices"] == [0, 0, 0]
        assert cfg["total_ballots"] == total and cfg["tampered"] == tampered and cfg["accepted"] == total - tampered
        assert cfg["tally_exchange_ok"] is True and cfg["tally_checked_against_one_engine"] is True
        assert line["scaling"] == ("weak" if total == 90000 else "strong") and line["value"] > 1e4 and line["steps"] == 2
        assert cfg["input"] == "hbm"
        js = line["json_inclusive"]                     # the JSON text of the batch through eg_verify_*_json_multi (one parser, three lanes)
        assert js["devices"] == 3 and js["verdicts_match_device_path"] is True and js["value"] > 1e4, js
    # the same through ONE pinned host buffer (--from-host: eg_verify_*_batch_multi; VERDICT r5 task 1): the entry a one-process host
    # with its ballots in host memory calls had no timing anywhere
    r = _run_bare(["--full", "--in-process-devices", "3", "--rehearse-one-gpu", "--from-host", "--steps", "2", "--warmup", "1", "--ballots", "30000",
                   "--tampered-percent", "1"], {"EG_CHUNK": "32768", "EG_COMB_BIG_BITS": "0"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    cfg = line["config"]
    assert cfg["input"] == "host" and cfg["accepted"] == 90000 - 900 and cfg["tally_exchange_ok"] is True
    assert line["host_inclusive"]["bytes_h2d"] == 90000 * 736 and line["host_inclusive"]["value"] == line["value"] > 1e4


def test_bench_four_ranks_ten_million_ballots_rehearsed():
    """BASELINE configs[4] - 10 M single-choice ballots, sharded, 1 % tampered, ONE tally exchange - with four ranks time-sharing the
    GPU (gloo for the exchange), per-rank memory bounded (chunks of 65 536 ballots, narrow comb tables): shards of 2.5 M each,
    9 900 000 accepted, the exchanged tally identical on every rank, one JSON line from rank 0 (examples/voting.rs:199-203)."""
    r = _run(4, ["--full", "--steps", "1", "--warmup", "0", "--rehearse-one-gpu", "--total-ballots", "10000000", "--tampered-percent", "1",
                 "--no-isolated"], {"EG_CHUNK": "65536", "EG_COMB_BIG_BITS": "0"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    cfg = line["config"]
    assert line["n_gpus"] == 4 and line["scaling"] == "strong" and cfg["total_ballots"] == 10_000_000
    assert cfg["ballots_per_gpu"] == 2_500_000 and cfg["parallelism"] == "shard4"
    assert cfg["tampered"] == 100_000 and cfg["accepted"] == 9_900_000
    assert cfg["tally_exchange_ok"] is True
    assert line["value"] > 1e5 and line["steps"] == 1 and line["warmup"] == 0


def test_bench_multi_rank_failures_are_loud_and_early():
    """A rank that cannot take part must end the job with a non-zero exit code BEFORE any timed step, as a failure of a fresh process
    (VERDICT r3 task 2).  (a) an exchange that returns wrong bytes - the rank script tests/bench_rank_corrupt_gather.py wraps
    gather_tallies so that rank 1's gathered tallies differ (the shipped module has no such switch): the preflight check stops every
    rank, no JSON line is printed; (b) a wrong --gpus / WORLD_SIZE pairing under the launcher."""
    r = _run(2, ["--steps", "1", "--warmup", "0", "--rehearse-one-gpu", "--ballots", "20000"], timeout=600,
             script="tests/bench_rank_corrupt_gather.py")
    assert r.returncode != 0
    assert "FATAL" in r.stderr and "preflight" in r.stderr
    assert not [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, timeout=300,
                       env=_env({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}), cwd=str(ROOT))
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)
