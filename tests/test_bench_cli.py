"""bench.py's command line: a plain run times the headline alone and can
write what its last timed step returned (--dump-outputs); every other leg of
the line sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("configs1", "replica_sweep", "annotations", "annotations_configs2", "per_cycle", "per_cycle_launch",
             "per_cycle_hinted", "per_cycle_configs2", "configs2", "kubelet_memory", "cpu_baseline")


def test_options_present_and_steps_checked():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--nodes", "300", "--pods", "400"]


def _run(args, dump):
    return subprocess.run([sys.executable, BENCH] + SMALL + ["--dump-outputs", str(dump)] + args,
                          capture_output=True, text=True, timeout=180)


@pytest.fixture(scope="module")
def plain_run(built, tmp_path_factory):
    """One plain run at 300 nodes x 400 pods, shared: (process, dump folder)."""
    dump = tmp_path_factory.mktemp("plain") / "dump"
    return _run([], dump), dump


@pytest.mark.gpu
def test_plain_run_dumps_last_step(plain_run):
    """300 nodes x 400 pods, 2 timed steps: the line holds the headline fields
    and no --full leg; placements.npy is the last step's placement vector."""
    n_pods = 400
    r, dump = plain_run
    assert r.returncode == 0, r.stderr[-2000:]
    # the result line is the last line of stdout (RCCL may print its version banner before it)
    lines = r.stdout.strip().splitlines()
    assert len([ln for ln in lines if ln.startswith("{")]) == 1
    d = json.loads(lines[-1])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "pods/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - n_pods / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert r.stderr.count("step wall") == 2
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(dump)) == ["placements.npy", "replica_placements.npy"]
    pl = np.load(dump / "placements.npy")
    rp = np.load(dump / "replica_placements.npy")
    assert pl.dtype == np.float64 and pl.shape == (n_pods,)
    assert rp.dtype == np.float64 and rp.shape == (1, n_pods) and np.array_equal(rp[0], pl)
    assert np.array_equal(pl, np.round(pl)) and pl.min() >= -1 and pl.max() < 300
    assert int((pl >= 0).sum()) == d["config"]["pods_scheduled_per_step"]
    # the same queue through the CPU oracle
    import binding
    G, E = pkg("generator"), pkg("encoder")
    nodes, pods, prof = G.config1(n_nodes=300, n_pods=n_pods)
    enc = E.Encoder(nodes, pods, prof)
    ora = binding.Oracle(nthreads=4)
    ora.load(enc, E.encode_profile(prof, enc.cluster.res_names))
    want, _ = ora.run_queue(0, n_pods, results=False)
    ora.close()
    assert np.array_equal(pl, np.asarray(want, dtype=np.float64))


@pytest.mark.gpu
def test_full_run_carries_every_leg(plain_run, tmp_path):
    """--full at the same headline size with every leg cut down to a few
    hundred pods: each moved key is in the line again, the headline agrees
    with the oracle, and a second run with the same arguments for the headline
    dumps the same arrays as the plain one."""
    r = _run(["--full", "--cpu-budget", "1", "--configs1-pods", "400", "--sweep-replicas", "8", "--sweep-pods", "64",
              "--annotate-pods", "64", "--annotate-long-pods", "0", "--cycle-pods", "32", "--cycle-warm", "16",
              "--kubelet-pods", "400", "--topo-nodes", "300", "--topo-cycle-pods", "16", "--topo-queue-pods", "300",
              "--topo-annotate-pods", "16", "--topo-annotate-long-pods", "0"], tmp_path / "dump")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "unavailable" not in r.stderr, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert not [k for k in FULL_ONLY if k not in d]
    assert d["roofline"].get("kernel") and d["placements_equal_oracle"] is True
    assert d["steps"] == 2 and r.stderr.count("step wall") == 2   # the per-kernel timing pass is not a timed step
    for k in ("per_cycle", "per_cycle_launch", "per_cycle_hinted", "per_cycle_configs2"):
        assert d[k]["placements_equal_run_queue"] is True
    for k in ("annotations", "annotations_configs2"):
        assert d[k]["device_serialiser"]["bytes_equal_host"] is True
    _, plain_dump = plain_run
    for name in ("placements.npy", "replica_placements.npy"):
        assert np.array_equal(np.load(tmp_path / "dump" / name), np.load(plain_dump / name))
