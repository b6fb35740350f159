"""bench.py's launcher logic (no GPU needed): `--gpus N` starts N ranks itself through
torch.distributed.run on 127.0.0.1, and a launcher whose WORLD_SIZE disagrees with --gpus is refused
before anything touches the GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_launcher_cmd_one_process_per_gpu():
    cmd = bench.launcher_cmd(["--gpus", "8", "--steps", "3"], 8, 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd and "--master-port=29555" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"] and cmd[-5].endswith("bench.py")


def test_bench_import_does_not_load_the_library():
    assert bench.ppo_amd is None


def test_dump_rows_are_a_fixed_sorted_sample_within_the_caps():
    """--dump-outputs: every row below the caps, above them the same sorted sample in every run, and
    the caps keep a dump of the eight storage buffers (O=17, A=6) below 64 MB."""
    import numpy as np
    rows, wide = bench.dump_rows(8192)
    assert np.array_equal(rows, np.arange(8192)) and np.array_equal(wide, rows)
    rows, wide = bench.dump_rows(4096 * 128)  # the metric config: scalars whole, obs / actions sampled
    assert np.array_equal(rows, np.arange(4096 * 128)) and wide.size == bench.DUMP_MAX_WIDE_ROWS
    B = 3 * bench.DUMP_MAX_ROWS + 5
    rows, wide = bench.dump_rows(B)
    assert rows.size == bench.DUMP_MAX_ROWS and wide.size == bench.DUMP_MAX_WIDE_ROWS
    for a in (rows, wide):
        assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < B
    assert np.isin(wide, rows).all()
    again = bench.dump_rows(B)
    assert np.array_equal(rows, again[0]) and np.array_equal(wide, again[1])
    assert 4 * (6 * bench.DUMP_MAX_ROWS + (17 + 6) * bench.DUMP_MAX_WIDE_ROWS) < 40e6


def test_world_size_mismatch_fails_loudly():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in r.stderr
