"""bench.py honours --gpus (a plain `--gpus 8` used to run one rank
and report n_gpus 1).  Under a launcher WORLD_SIZE must equal --gpus; the check
runs before anything touches a GPU, so it is testable here."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def test_world_size_mismatch_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert "WORLD_SIZE=2" in line["error"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline
    line without the --full legs; --dump-outputs writes the last step's CRCs and
    digests as float64 .npy (32-bit values, exact), and a second run with the
    same arguments writes the same arrays: the pool is seeded."""
    import numpy as np
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    chunks, steps = 16, 2
    dumps = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--chunks", str(chunks),
                            "--steps", str(steps), "--warmup", "1", "--clock-warm-ms", "0", "--dump-outputs", str(d)],
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and len(line["roofline"]["kernel_ms_each"]) == steps
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "GiB/s"
        assert abs(line["value"] - chunks * (16 << 20) / (1 << 30) / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
        for leg in ("verify", "cpu_baseline", "partial_write", "read_verify", "wal_replay", "stream", "files",
                    "scan_op", "digest_check_cpu"):
            assert leg not in line, leg
        arrays = {f: np.load(str(d / f)) for f in sorted(os.listdir(d))}
        assert {f: a.shape for f, a in arrays.items()} == {
            "digest.npy": (min(64, chunks),), "file_crcs.npy": (chunks,), "meta_crcs.npy": (chunks,),
            "page_crcs.npy": (chunks * 4096,), "slice_crcs.npy": (chunks * 4,)}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64_000_000
        dumps.append(arrays)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
    # not all zero, and every value a 32-bit integer
    pages = dumps[0]["page_crcs.npy"]
    assert len(np.unique(pages)) > pages.size // 2
    assert (pages == np.floor(pages)).all() and pages.min() >= 0 and pages.max() < 2**32


def test_numa_binding_helpers_never_fail():
    """bench.bind_to_gpu_numa parses sysfs cpulists and never fails the run: with
    no GPU (here) it reports why it did not bind and leaves the affinity alone."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench._cpulist("0-3,8,10-11\n") == {0, 1, 2, 3, 8, 10, 11}
    assert bench._cpulist("5") == {5}
    assert bench._cpulist("\n") == set()
    before = os.sched_getaffinity(0)
    r = bench.bind_to_gpu_numa(0)
    assert r["bound"] is False and r["why"]
    assert os.sched_getaffinity(0) == before


def test_stream_distinct_bounded_by_free_host_memory():
    """The C3 stream leg pins up to --stream-distinct 16 MiB chunks (156 GiB for
    all 10,000 distinct): _host_chunk_budget keeps that under MemAvailable /
    the cgroup limit less a margin, never below 64 chunks, never above the ask."""
    sys.path.insert(0, ROOT)
    import bench
    want = 10000
    got = bench._host_chunk_budget(want)
    assert 64 <= got <= want
    free = None
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            free = int(line.split()[1]) * 1024
    if free is not None:
        assert got == want or got == 64 or got * (16 << 20) <= free
    assert bench._host_chunk_budget(10) == 10
    assert bench._host_chunk_budget(want, margin=1 << 62) == 64  # nothing to spare: the floor
