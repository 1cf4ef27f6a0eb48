"""bench.py's command line on one GPU: a plain run prints the headline line and nothing that
takes a run of its own; --dump-outputs writes the last timed step's outputs, identical from run
to run and equal to the CPU restatement's over the same seeded reports; --full adds the roofline
pass, the CPU baseline with its parity checks and (unless --no-secondary) the secondary lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VK = bytes.fromhex("4a414e55532d414d442d42454e434821")  # bench.py's verify key
SEED = 0x4A414E5553000001                                # bench.py's report seed
N = 4096 + 37  # more than one block, not a multiple of the wave
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FILES = ("sample_index", "prep_msgs", "status", "aggregate_share", "count", "checksum", "interval")


def _bench(*argv):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reports", str(N),
           *argv]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       timeout=240)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out + p.stderr.decode(errors="replace")[-4000:]
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in FILES}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """One plain run, shared: its result line and the directory it dumped into."""
    a = str(tmp_path_factory.mktemp("plain"))
    return _bench("--steps", "3", "--warmup", "1", "--dump-outputs", a), a


def test_plain_run_dumps_the_timed_steps_outputs(plain):
    import torch
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle, batch_metadata
    line, a = plain
    for k in HEADLINE:
        assert k in line
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] / 1e3))
    # three timed steps, and no pass after them, on the engine's launch counters
    launches = {v["launches"] for v in line["kernels_timed_region"].values()}
    assert launches and all(x % 3 == 0 for x in launches)
    moved = [k for k in line if k in ("roofline", "kernels", "cpu_baseline", "speedup_vs_cpu")
             or k.startswith("secondary_")]
    assert not moved, moved
    assert line["checks"] == dict(finished=N, generator_flags=0, agg_count=N)
    got = _load(a)
    assert sorted(os.listdir(a)) == sorted(k + ".npy" for k in FILES)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20

    # they are what the CPU restatement computes from the same seeded reports
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), VK, device=0)
    d = eng.generate_reports_device(N, seed=SEED, first_index=0)
    h = {k: d[k].cpu().numpy() for k in
         ("nonces", "public_shares", "helper_shares", "leader_prep_shares")}
    g = torch.Generator(device=d["nonces"].device).manual_seed(0x4A414E55)
    times = (1_700_000_000 + torch.randint(0, 3600, (N,), generator=g, device=d["nonces"].device,
                                           dtype=torch.int64)).cpu().numpy()
    rm, rs, ra, rc = Oracle("histogram", length=256, chunk_length=16).helper_batch(
        VK, h["nonces"], h["public_shares"], h["helper_shares"], h["leader_prep_shares"],
        n_threads=4, job_size=500)
    ck, iv = batch_metadata(h["nonces"], times, rs, None, None, 1)
    np.testing.assert_array_equal(got["sample_index"], np.arange(N))
    np.testing.assert_array_equal(got["status"], rs)
    np.testing.assert_array_equal(got["prep_msgs"], rm)
    np.testing.assert_array_equal(got["aggregate_share"].reshape(-1), np.asarray(ra).reshape(-1))
    np.testing.assert_array_equal(got["count"].reshape(-1), np.asarray(rc).reshape(-1))
    np.testing.assert_array_equal(got["checksum"], ck)
    np.testing.assert_array_equal(got["interval"], iv.view(np.int64))
    eng.close()


def test_full_run_adds_roofline_and_cpu_baseline(plain, tmp_path):
    line = _bench("--full", "--no-secondary", "--cpu-seconds", "0.2", "--steps", "2",
                  "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k in HEADLINE + ("roofline", "kernels", "cpu_baseline", "speedup_vs_cpu"):
        assert k in line
    assert line["steps"] == 2 and line["roofline"]["frac"] > 0
    assert line["checks"]["cpu_gpu_parity_on_sample"] is True
    assert line["checks"]["batch_metadata_parity"] is True
    assert not [k for k in line if k.startswith("secondary_")]
    # the same reports again: the same outputs, whatever runs after the timed steps
    first, again = _load(plain[1]), _load(str(tmp_path))
    for k in FILES:
        np.testing.assert_array_equal(first[k], again[k])
