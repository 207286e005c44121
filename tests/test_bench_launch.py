"""bench.py --gpus N from a plain shell (no torchrun around it): the parent starts the ranks itself, relays rank 0's JSON line and the
worst exit code.  Runs here without a GPU through --dry-run, which exercises everything of the N-rank path except the kernels: the
rendezvous (gloo, 127.0.0.1), block-cyclic ownership, the double-buffered gather into rank 0, the assembly, and the per-phase clocks
the N > 1 line carries (render_ms_max, gather_ms, assemble_ms, gather_bytes)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.parametrize("n,extra", [(2, []), (3, ["--block-cols", "32"])])
def test_plain_shell_launch_of_n_ranks(n, extra):
    W, H, B = 256, 136, 3
    r = _run("--gpus", str(n), "--backend", "gloo", "--steps", "2", "--warmup", "1", "--dry-run", "--width", str(W), "--height", str(H), "--frames", str(B), *extra)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["steps"] == 2 and d["value"] is None and "dry_run" in d
    assert d["assembled_frames_ok"] is True
    for k in ("render_ms_max", "gather_ms", "assemble_ms"):
        assert d[k] > 0.0, k
    assert d["gather_bytes"] > 0 and d["gather_bytes"] % (n - 1) == 0
    assert d["gather_bytes"] // (n - 1) >= B * (H // n) * W * 3 * 0.9          # one padded tile set per peer


def test_dump_outputs_is_small_fixed_and_exact(tmp_path):
    """--dump-outputs: finite float32 / float64 files under 64 MB in all (+inf / NaN written as -1).  A 1920x1080 step's arrays keep
    one fixed, seeded pixel sample (the same in every array and every run, pixel_index.npy says which); a small frame is written
    whole.  Values are exact."""
    import importlib.util
    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    B, H, W, NB = 8, 1080, 1920, 4
    g = torch.Generator().manual_seed(1)
    outs = {"rgb8": torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g),
            "hit_id": torch.randint(-1, 1 << 20, (NB, H, W), dtype=torch.int32, generator=g),
            "t": torch.rand((NB, H, W), generator=g), "rgb_linear": torch.rand((NB, H, W, 3), generator=g)}
    outs["t"][outs["hit_id"] < 0] = float("inf")                 # the library's t where no surface was hit
    outs["rgb_linear"][:, ::7, ::5, 1] = float("nan")            # shading of a mesh without normals
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["hit_id.npy", "pixel_index.npy", "rgb8.npy", "rgb_linear.npy", "t.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < 64e6
    for f in files:
        x = np.load(tmp_path / "a" / f)
        assert x.dtype in (np.float32, np.float64), f
        assert np.isfinite(x).all(), f
        assert np.array_equal(x, np.load(tmp_path / "b" / f)), f
    idx = np.load(tmp_path / "a" / "pixel_index.npy").astype(np.int64)
    assert 0 < idx.size < H * W and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rgb8.npy"), outs["rgb8"].reshape(B, -1, 3).numpy()[:, idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "hit_id.npy"), outs["hit_id"].reshape(NB, -1).numpy()[:, idx].astype(np.float64))
    lin = outs["rgb_linear"].reshape(NB, -1, 3).numpy()[:, idx]
    assert np.isnan(lin).any() and np.array_equal(np.load(tmp_path / "a" / "rgb_linear.npy"), np.where(np.isnan(lin), np.float32(-1), lin))
    t = outs["t"].reshape(NB, -1).numpy()[:, idx]
    assert np.isinf(t).any() and np.array_equal(np.load(tmp_path / "a" / "t.npy"), np.where(np.isinf(t), np.float32(-1), t))
    small = outs["rgb8"][:2, :96, :128]
    b.dump_outputs(str(tmp_path / "s"), {"rgb8": small})
    assert os.listdir(tmp_path / "s") == ["rgb8.npy"]
    assert np.array_equal(np.load(tmp_path / "s" / "rgb8.npy"), small.numpy().astype(np.float32))


def test_a_failing_rank_fails_the_launch():
    """Without --dry-run the ranks need a GPU; here they exit with an error, and the parent must report it (not hang, not return 0)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the ranks would run")
    r = _run("--gpus", "2", "--backend", "gloo", "--steps", "1", "--no-pmc", "--no-cpu-baseline", timeout=300)
    assert r.returncode != 0
    assert "needs a GPU" in r.stderr
