"""bench.py's multi-rank launcher on CPU (no HIP): `bench.py --gpus N` without WORLD_SIZE starts
N rank processes with the torch.distributed environment and passes rank 0's JSON line through;
it refuses (non-zero status) to run fewer ranks than asked for. The driver's scaling run uses
`torch.distributed.run ... bench.py --gpus N`, which sets WORLD_SIZE itself."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=180):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    if env:
        e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("n", [2, 3])
def test_launcher_forms_n_ranks(n):
    r = _run(["--gpus", str(n), "--selftest", "--batch", "1000"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout  # rank 0's JSON line and nothing else
    out = json.loads(lines[0])
    assert out["n_gpus"] == n
    assert out["max_over_ranks"] == float(n)  # every rank took part in the MAX reduction
    # the node figure: one 1000-check request shared by the n ranks in contiguous slices, in rank
    # order, covering it exactly (strong scaling); weak scaling checks n x 1000 per step
    assert out["global_batch"] == 1000
    sl = out["slices"]
    assert len(sl) == n and sl[0][0] == 0 and sl[-1][1] == 1000
    assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    assert max(e - b for b, e in sl) - min(e - b for b, e in sl) <= 1
    assert out["slice"] == sl[0]
    assert out["checks_per_step"] == {"strong": 1000, "weak": 1000 * n}


def test_launcher_refuses_missing_gpus():
    # this container has no GPU: asking for 2 must fail loudly rather than run one rank
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("enough GPUs visible")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "refusing" in r.stderr


def test_full_and_dump_outputs_options_parse():
    # --full and --dump-outputs are options of every run (the selftest writes nothing)
    r = _run(["--gpus", "1", "--selftest", "--batch", "1000", "--full", "--dump-outputs", "unused"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1
    assert not os.path.exists(os.path.join(ROOT, "unused"))
    # the loop trace is of the host-buffer region, which only --full runs
    r = _run(["--gpus", "1", "--selftest", "--trace-loop"])
    assert r.returncode != 0 and "--full" in r.stderr


def test_dump_outputs_writes_float32_and_samples_reproducibly(tmp_path, monkeypatch):
    import numpy as np
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    perm = np.arange(1000, dtype=np.uint8) % 4
    err = np.arange(1000, dtype=np.int32) - 500
    bench.dump_outputs(str(tmp_path / "a"), {"perm": perm, "err": err})
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("perm", "err")}
    assert got["perm"].dtype == np.float32 and got["err"].dtype == np.float32
    assert (got["perm"] == perm).all() and (got["err"] == err).all()
    # over the size limit: a fixed sample, the same elements every time, within the limit in all
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 100)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"perm": perm, "err": err})
    b, c = (np.load(tmp_path / d / "err.npy") for d in ("b", "c"))
    assert b.shape == (100,) and (b == c).all() and np.isin(b, err).all() and (np.diff(b) > 0).all()
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 8 * 100 + 2 * 128
    # rank r > 0 of several writes beside rank 0
    bench.dump_outputs(str(tmp_path / "a"), {"perm": perm}, rank=1, world=2)
    assert (tmp_path / "a" / "perm.rank1.npy").exists()


def test_world_size_mismatch_refused():
    r = _run(["--gpus", "2", "--steps", "1"], env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr
