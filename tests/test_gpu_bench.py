"""GPU tests of the bench.py driver contract — single rank and a
2-process gloo rendezvous sharing one GPU (the multi-GPU launch shape
on a 1-GPU box)."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

SMALL = ["--msg-bytes", "4194304", "--region-bytes", "67108864",
         "--steps", "3", "--warmup", "1"]


def _env(extra=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    if extra:
        env.update(extra)
    return env


@pytest.mark.timeout(600)
def test_bench_single_rank_gpu():
    out = subprocess.run([sys.executable, BENCH, "--full"] + SMALL,
                         capture_output=True, text=True, env=_env(),
                         cwd=ROOT, timeout=480)
    assert out.returncode == 0, out.stderr
    r = json.loads([l for l in out.stdout.splitlines()
                    if l.startswith("{")][0])
    assert r["config"]["transport"] == "sdma"
    assert r["config"]["integrity"] == "ok"
    assert r["value"] > 5  # GB/s; PCIe path


@pytest.mark.timeout(600)
def test_bench_plain_run_dumps_the_written_region(tmp_path):
    """A plain run (no --full) skips the integrity pass and the extra
    sizes; --dump-outputs holds the HBM region the last step wrote —
    64 MiB, so a seeded sample of 4 KiB chunks — byte for byte the
    staged splitmix64 payloads (16 messages of 4 MiB, one slot each)."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from rocnrdma_amd.utils import pattern

    out = subprocess.run(
        [sys.executable, BENCH, "--dump-outputs", str(tmp_path)] + SMALL,
        capture_output=True, text=True, env=_env(), cwd=ROOT, timeout=480)
    assert out.returncode == 0, out.stderr
    r = json.loads([l for l in out.stdout.splitlines()
                    if l.startswith("{")][0])
    assert r["config"]["transport"] == "sdma"
    assert r["config"]["integrity"] == "skipped"
    assert r["config"]["msg_sweep_gbps"] is None
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert r["value"] > 5  # GB/s; PCIe path

    assert os.listdir(tmp_path) == ["region.npy"]
    got = np.load(tmp_path / "region.npy")
    idx = bench.dump_sample_chunks(67108864)
    assert got.dtype == np.float32 and got.shape == (len(idx), 4096)
    msg = 4194304
    want = np.empty((len(idx), 4096), dtype=np.uint8)
    for k, off in enumerate(idx * 4096):
        slot = off // msg  # 16 messages, 16 staging slots
        want[k] = pattern.splitmix64_words(
            0xDA7A, slot * 8192 + (off % msg) // 8, 512).view(np.uint8)
    assert np.array_equal(got, want.astype(np.float32))


@pytest.mark.timeout(600)
def test_bench_step_refills_the_ring(tmp_path):
    """bench's step shape end to end: --inflight 6 under 16 messages of
    4 MiB, so every post_many(base, 16) refills the ring twice and the
    slot of a message is not its region message.  The last of the 3 steps
    posts indices 32..47: region message j holds the splitmix64 payload
    of slot (32 + j) % 6."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from rocnrdma_amd.utils import pattern

    out = subprocess.run(
        [sys.executable, BENCH, "--dump-outputs", str(tmp_path),
         "--inflight", "6"] + SMALL,
        capture_output=True, text=True, env=_env(), cwd=ROOT, timeout=480)
    assert out.returncode == 0, out.stderr
    r = json.loads([l for l in out.stdout.splitlines()
                    if l.startswith("{")][0])
    assert r["config"]["transport"] == "sdma"
    assert r["config"]["inflight"] == 6
    assert r["steps"] == 3

    got = np.load(tmp_path / "region.npy")
    idx = bench.dump_sample_chunks(67108864)
    assert got.dtype == np.float32 and got.shape == (len(idx), 4096)
    msg = 4194304
    want = np.empty((len(idx), 4096), dtype=np.uint8)
    for k, off in enumerate(idx * 4096):
        slot = (32 + off // msg) % 6
        want[k] = pattern.splitmix64_words(
            0xDA7A, slot * 8192 + (off % msg) // 8, 512).view(np.uint8)
    assert np.array_equal(got, want.astype(np.float32))
    # the sample tells the slots apart: it touches messages of several
    assert len({(32 + off // msg) % 6 for off in idx * 4096}) > 1


@pytest.mark.timeout(600)
def test_bench_two_ranks_one_gpu():
    """Two ranks rendezvous over gloo at 127.0.0.1, both on cuda:0 —
    validates the distributed launch path the driver uses for N>1."""
    procs = []
    for rank in range(2):
        env = _env({"RANK": str(rank), "WORLD_SIZE": "2",
                    "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": "29612"})
        procs.append(subprocess.Popen(
            [sys.executable, BENCH, "--gpus", "2", "--full"] + SMALL,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
            env=env, cwd=ROOT))
    outs = [p.communicate(timeout=480) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se
    r = json.loads([l for l in outs[0][0].splitlines()
                    if l.startswith("{")][0])
    assert r["n_gpus"] == 2
    assert r["config"]["integrity"] == "ok"
