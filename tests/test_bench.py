"""bench.py's driver contract on CPU: ``--gpus N`` launches N ranks itself (gloo rehearsal here),
prints exactly one JSON line, and a failing rank fails the whole command."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["MS_DIST_BACKEND"] = "gloo"
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          env=env, timeout=timeout, cwd=ROOT)


def _json_lines(out: str) -> list[dict]:
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{\"metric\"")]


def test_bench_gpus_two_self_launches_two_ranks():
    p = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--map-size", "64", "--cells", "200")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    out = lines[0]
    assert out["ranks"] == 2 and out["config"]["ranks"] == 2
    assert out["config"]["parallelism"] == "spatial2"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert len(out["devices"]) == 2


def test_bench_single_rank_unchanged():
    p = _run("--steps", "2", "--warmup", "1", "--map-size", "64", "--cells", "200")
    assert p.returncode == 0, p.stderr[-3000:]
    (out,) = _json_lines(p.stdout)
    assert out["ranks"] == 1 and out["config"]["parallelism"] == "single"
    assert "ranks" not in out["config"]


def test_bench_dump_outputs_is_reproducible(tmp_path):
    """``--dump-outputs DIR``: the last timed step's world state as float32 / float64 ``.npy`` files
    below 64 MB, the same from run to run with the same arguments (same seeds, same inputs);
    ``--steps`` sets the timed steps and ``ms_per_step`` is their mean wall time; ``--full`` runs."""
    import numpy as np

    args = ("--steps", "2", "--warmup", "0", "--map-size", "64", "--cells", "200")
    dumps = []
    for name, extra in (("a", ("--full",)), ("b", ())):
        d = tmp_path / name
        p = _run(*args, *extra, "--dump-outputs", str(d))
        assert p.returncode == 0, p.stderr[-3000:]
        (out,) = _json_lines(p.stdout)
        assert out["steps"] == 2 and out["warmup"] == 0
        assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1.0  # value = steps/s of the same window
        arrays = {f.name: np.load(f) for f in sorted(d.iterdir())}
        assert all(f.endswith(".npy") for f in arrays)
        assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
        n = int(arrays["n_cells.npy"][0])
        assert n == out["config"]["cells_at_end"] > 0
        assert arrays["molecule_map.npy"].shape[1:] == (64, 64)
        assert arrays["cell_molecules.npy"].shape == (n, arrays["molecule_map.npy"].shape[0])
        assert arrays["cell_positions.npy"].shape == (n, 2)
        assert np.isfinite(arrays["molecule_map.npy"]).all() and np.isfinite(arrays["cell_molecules.npy"]).all()
        np.testing.assert_allclose(arrays["molecule_map_totals.npy"],
                                   arrays["molecule_map.npy"].astype(np.float64).sum(axis=(1, 2)), rtol=1e-12)
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        np.testing.assert_array_equal(dumps[0][f], dumps[1][f], err_msg=f)


def test_bench_failing_rank_fails_the_command():
    # an impossible config on every rank: the launcher reports the failure with a non-zero code
    p = _run("--gpus", "2", "--steps", "1", "--warmup", "0", "--map-size", "64", "--cells", "200",
             "--chemistry", "synthetic:0:0")
    assert p.returncode != 0
    assert not _json_lines(p.stdout)
