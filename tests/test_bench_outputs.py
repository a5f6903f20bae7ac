"""bench.py's plain run and --dump-outputs.

A plain run (no --full) prints the headline line alone: no oracle check, no
side leg.  --dump-outputs DIR writes what the last timed step computed, each
partition's sum as the caller reads it, as DIR/sums.npy: float64, a fixed
seeded sample of every partition when the whole exceeds bench.DUMP_CAP_BYTES.
The choice of elements is checked on the CPU; on the GPU one run of config B
(16 x 1M x 8: the smallest config, already past the cap, so the sample is
taken) per input format, its dumped sums bit for bit against the oracle's
fixed-order fold of the same synthetic buckets."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

SIDE_KEYS = ("round", "publish", "per_arrival", "host_inclusive", "middleware_socket", "jni_heap", "cpu_baseline",
             "other_configs", "few_partitions")


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, str(ROOT))
    import bench as b
    return b


def test_sample_is_fixed_sorted_and_keeps_both_ends(bench):
    P, L = 16, 4194304
    idx = bench.dump_sample_index(P, L)
    assert idx.dtype == np.int64 and idx[0] == 0 and idx[-1] == L - 1
    assert np.all(np.diff(idx) > 0)                                  # sorted, no element twice
    assert 8 * P * idx.size <= bench.DUMP_CAP_BYTES < 64 * 10**6
    assert np.array_equal(idx, bench.dump_sample_index(P, L))        # the same elements in every run
    assert bench.dump_sample_index(3, 1000) is None                  # fits: everything is kept


def test_dump_writes_float64_whole_or_sampled(bench, tmp_path):
    info = bench.dump_outputs(str(tmp_path / "d"), "sums", lambda q: np.arange(1000.0) + q, 3, 1000)
    got = np.load(tmp_path / "d" / "sums.npy")
    assert got.dtype == np.float64 and got.shape == (3, 1000) and info["sampled"] is False
    assert np.array_equal(got[2], np.arange(1000.0) + 2)
    P, L = 4, 4194304
    info = bench.dump_outputs(str(tmp_path / "d"), "big", lambda q: np.arange(float(L)) * (q + 1), P, L)
    got = np.load(tmp_path / "d" / "big.npy")
    idx = bench.dump_sample_index(P, L)
    assert info["sampled"] is True and info["shape"] == [P, idx.size] and got.nbytes <= bench.DUMP_CAP_BYTES
    assert np.array_equal(got[3], idx.astype(np.float64) * 4)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("be", [False, True], ids=["f64", "be"])
def test_plain_run_dumps_the_timed_sums(bench, tmp_path, be):
    from oracle import oracle as O   # checker only
    P, L, K = bench.CONFIGS["B"]
    steps = 3
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--config", "B", "--dump-outputs", str(tmp_path)] + (["--be"] if be else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1                                           # stdout is the one JSON line
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "GB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["metric"] == bench.METRIC
    # value is the algorithmic bytes of the timed steps over their wall time
    assert line["value"] == pytest.approx(P * (K + 1) * L * 8 / line["ms_per_step"] / 1e6, rel=1e-3)
    assert not [k for k in SIDE_KEYS if k in line] and line["verified"] is None
    got = np.load(tmp_path / "sums.npy")
    idx = bench.dump_sample_index(P, L)
    assert got.dtype == np.float64 and got.shape == (P, idx.size) == tuple(line["outputs"]["shape"])
    for p in (0, P - 1):
        want = O.c_reduce([O.c_synth_bucket(L, p, k) for k in range(K)], L, O.START_ZERO)
        assert_bits_equal(got[p], want[idx], f"partition {p}")
