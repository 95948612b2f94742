"""Cost of the kill / replicate step by selection route, on one world in one process.

Three routes over the same loop (top-up, activity, selection, recombination, mutation, degradation,
diffusion), in alternating blocks of steps so that drift of the population or of the machine hits
all three alike:

* ``where``: ``World.kill_divide_where`` (hard thresholds, what ``bench.py`` runs);
* ``prob``:  ``World.kill_divide_prob`` with all three terms (Hill curves around the same
  thresholds plus a genome-size term);
* ``torch``: the README-style route -- ``torch.bernoulli`` masks of the same probabilities,
  ``kill_cells`` (one blocking read-back), ``divide_cells_t(lazy=True)``.

Every route runs inside the benchmark's own step (``bench.step``), whose chemostat sets the same
``kill_fraction`` rule for all three to hold the population at the target. Per block it prints one
JSON line: the selection's device time per step from ``World.step_timings()`` (HIP events) and the
wall time of a whole step.

    python performance/selection_prob.py [--map-size 4096] [--cells 50000] [--rounds 5] [--steps 40]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
import magicsoup_amd as ms  # noqa: E402
from magicsoup_amd.examples.wood_ljungdahl import CHEMISTRY  # noqa: E402

KILL_K, DIVIDE_K, GENOME_K, N_HILL, COST = 1.0, 5.0, 2000.0, 7, 4.0


def _hill_up(v, k, n):
    return 1.0 / (1.0 + (k / v) ** n)


def select(world, route: str, atp: int, frac: float) -> None:
    if route == "where":
        type(world).kill_divide_where(world, atp, KILL_K, DIVIDE_K, COST, kill_fraction=frac)
    elif route == "prob":
        world.kill_divide_prob(atp, kill_k=KILL_K, kill_n=N_HILL, divide_k=DIVIDE_K, divide_n=N_HILL, divide_cost=COST,
                               genome_k=GENOME_K, genome_n=N_HILL, kill_fraction=frac)
    else:
        x = world.cell_molecules[:, atp].clamp(min=1e-30)
        g = world._genomes.lens[: world.n_cells].float().clamp(min=1e-30)
        p_kill = 1.0 - (1.0 - frac) * _hill_up(x, KILL_K, N_HILL) * (1.0 - _hill_up(g, GENOME_K, N_HILL))
        world.kill_cells(torch.bernoulli(p_kill).bool())
        world.__dict__["_kill_n"] = world.n_cells
        x = world.cell_molecules[:, atp].clamp(min=1e-30)
        div = torch.bernoulli(_hill_up(x, DIVIDE_K, N_HILL)).bool()
        world.cell_molecules[:, atp] -= COST * div
        world.divide_cells_t(div, lazy=True)


def block(world, route: str, steps: int, target: int, size: int, atp: int) -> dict:
    """``steps`` steps of the benchmark's loop (bench.step: top-up, chemostat dilution rate, the
    genome operations, degradation, diffusion) with its selection call routed through ``route``."""

    def routed(mol, kill_below, divide_above, divide_cost, kill_fraction=0.0):
        n = world.n_cells
        select(world, route, mol, kill_fraction)
        if route == "torch":  # (the chemostat reads the kill's counts from last_kill)
            world.__dict__["last_kill"] = (n, world.__dict__["_kill_n"])

    world.kill_divide_where = routed  # (instance attribute: bench.step calls it)
    torch.cuda.synchronize()
    world.step_timings()  # reset
    t0 = time.perf_counter()
    try:
        for _ in range(steps):
            bench.step(world, target, size, atp)
        torch.cuda.synchronize()
    finally:
        del world.kill_divide_where
    wall = (time.perf_counter() - t0) / steps * 1e3
    t = world.step_timings()
    ops = ("kill_divide",) if route != "torch" else ("kill_cells", "divide_cells_t", "divide_cells")
    sel = sum(t[o]["ms_total"] for o in ops if o in t) / steps
    return {"route": route, "steps": steps, "selection_ms": round(sel, 4), "step_ms": round(wall, 4),
            "n_cells": world.n_cells, "last_kill": list(world.last_kill)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-size", type=int, default=4096)
    ap.add_argument("--cells", type=int, default=50_000)
    ap.add_argument("--genome-size", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    ms.set_seed(0)
    torch.manual_seed(0)
    world = ms.World(chemistry=CHEMISTRY, map_size=a.map_size, device="cuda", seed=0)
    world.spawn_cells(bench.random_genomes(a.cells, a.genome_size, "cuda"))
    atp = CHEMISTRY.molname_2_idx["ATP"]
    world.enable_timings(sync=False)
    routes = ("where", "prob", "torch")
    for r in routes:
        block(world, r, a.warmup, a.cells, a.genome_size, atp)
    for rnd in range(a.rounds):
        for r in routes:
            print(json.dumps({"round": rnd, **block(world, r, a.steps, a.cells, a.genome_size, atp)}), flush=True)


if __name__ == "__main__":
    main()
