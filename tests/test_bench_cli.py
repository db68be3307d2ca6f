"""CPU: bench.py's command line.  A plain run times exactly --steps steps and
carries nothing but the headline (the cfg3 line and the CPU baseline sit
behind --full); --dump-outputs writes the last step's outputs as float .npy
files, the same elements from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _bench(args):
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                          capture_output=True, text=True, env=env,
                          timeout=300, cwd=ROOT)


def test_plain_run_carries_the_headline_only(tmp_path):
    d = str(tmp_path / "out")
    r = _bench(["--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1",
                "--dump-outputs", d])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    assert out["unit"] == "GB/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u16"
    assert out["cpu_baseline"] is None and "secondary" not in out
    a = np.load(os.path.join(d, "data.npy"))
    assert a.dtype == np.float64 and a.size > 0


def test_steps_must_be_positive():
    r = _bench(["--gpus", "1", "--dry-run", "--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr


def _buffers(S, n_out, k, P, cap, seed):
    g = torch.Generator().manual_seed(seed)
    coded = torch.randint(-32768, 32768, (S, n_out, P), dtype=torch.int16, generator=g)
    dec = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, generator=g)
    counts = torch.randint(0, cap + 1, (S * n_out,), dtype=torch.int32, generator=g)
    entries = torch.randint(0, P, (S * n_out * cap,), dtype=torch.int32, generator=g)
    return coded, dec, counts, entries


def test_dump_outputs_whole_arrays(tmp_path):
    S, n_out, k, P, cap = 3, 8, 4, 32, 4
    coded, dec, counts, entries = _buffers(S, n_out, k, P, cap, 1)
    bench.dump_outputs(str(tmp_path), coded, dec, counts, entries, cap)
    got = {n: np.load(tmp_path / f"{n}.npy")
           for n in ("coded", "decoded", "oor_counts", "oor_entries")}
    assert got["coded"].dtype == got["decoded"].dtype == np.float32
    assert got["oor_counts"].dtype == np.float32
    assert got["oor_entries"].dtype == np.float64
    # u16 values, not the int16 the buffers hold them as
    assert (got["coded"] == coded.numpy().view(np.uint16).ravel()).all()
    assert (got["decoded"] == dec.numpy().view(np.uint16).ravel()).all()
    assert (got["oor_counts"] == counts.numpy()).all()
    ent = entries.numpy().reshape(-1, cap)
    for b, c in enumerate(counts.numpy()):
        # a bucket is the set of its first `count` entries: the order the
        # kernels appended them in and what lies behind them do not show
        assert got["oor_entries"][b, :c].tolist() == sorted(ent[b, :c].tolist())
        assert (got["oor_entries"][b, c:] == -1).all()
    shuffled = ent.copy()
    for b, c in enumerate(counts.numpy()):
        shuffled[b, :c] = shuffled[b, :c][::-1]
        shuffled[b, c:] = 7
    other = tmp_path / "other"
    bench.dump_outputs(str(other), coded, dec, counts,
                       torch.from_numpy(shuffled).reshape(-1), cap)
    assert (np.load(other / "oor_entries.npy") == got["oor_entries"]).all()


def test_dump_outputs_samples_the_same_elements(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CODED", 100)
    monkeypatch.setattr(bench, "DUMP_DECODED", 50)
    monkeypatch.setattr(bench, "DUMP_COUNTS", 10)
    monkeypatch.setattr(bench, "DUMP_ENTRIES", 5 * 4)
    S, n_out, k, P, cap = 3, 8, 4, 32, 4
    a = _buffers(S, n_out, k, P, cap, 1)
    bench.dump_outputs(str(tmp_path / "a"), *a, cap)
    bench.dump_outputs(str(tmp_path / "a2"), *a, cap)
    shapes = {"coded": (100,), "decoded": (50,), "oor_counts": (10,),
              "oor_entries": (5, cap)}
    for n, shp in shapes.items():
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "a2" / f"{n}.npy")
        assert x.shape == shp and (x == y).all()
    # the sample follows the buffers' contents, not only their shapes
    b = _buffers(S, n_out, k, P, cap, 2)
    bench.dump_outputs(str(tmp_path / "b"), *b, cap)
    assert (np.load(tmp_path / "a" / "coded.npy")
            != np.load(tmp_path / "b" / "coded.npy")).any()
