"""Probabilistic (Hill-curve) kill / divide selection on the GPU: the mask kernels against the host
core's masks, ``World.kill_divide_prob`` against explicit masks + ``kill_divide_t``, on plain worlds
and on a decomposed world's strip."""
import copy

import numpy as np
import pytest
import torch

import magicsoup_amd as ms
from magicsoup_amd.examples.wood_ljungdahl import CHEMISTRY
from magicsoup_amd.ops import native
from tests.conftest import gen_genomes
from tests.dist_utils import run_ranks
from tests.test_selection_prob import (KILL_K, DIVIDE_K, SATURATED, STATE, host_masks, rule_cases,
                                       saturated_world, selection_inputs)

pytestmark = pytest.mark.gpu

MASK_KEY = 0xBB67AE8584CAA73B  # (models/world.py _PROB_MASK_KEY)
RULE = dict(kill_k=KILL_K, kill_n=2, divide_k=DIVIDE_K, divide_n=3, genome_k=320.0, genome_n=7, kill_fraction=0.05)


def _bits(t: torch.Tensor) -> torch.Tensor:
    """Bit pattern of a float tensor (NaN-safe equality)."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _rule_args(rule):
    a = []
    for t, n0 in (("kill", 1), ("divide", 3), ("genome", 7)):
        k = rule.get(f"{t}_k")
        a += [k is not None, 1.0 if k is None else float(k), int(rule.get(f"{t}_n", n0))]
    return a


def _next_call(seed):
    """The (seed, call) the next native call draws under ms.set_seed(seed), which is set again."""
    from magicsoup_amd.ops import hip_ops

    ms.set_seed(seed)
    sc = hip_ops._rng()
    ms.set_seed(seed)
    return sc


def _oracle_masks(w, mol, rule, seed, call):
    """_host.prob_masks over the world's molecules and genome lengths (bool tensors on its device)."""
    n = w.n_cells
    kill, div = host_masks(w.cell_molecules.cpu().numpy(), mol, w._genomes.lens[:n].cpu().numpy(), rule, seed, call)
    return torch.from_numpy(kill).to(w.device), torch.from_numpy(div).to(w.device)


def _mask_worlds(chem, n, dtype):
    """Two equal worlds of n cells (a deep copy materialises pending map state, so the copy is made
    first); reduced-precision maps carry a pending degradation and correction."""
    ms.set_seed(5)
    torch.manual_seed(5)
    size = 16 if n < 20 else 32 if n < 300 else 128
    w = ms.World(chemistry=chem, map_size=size, device="cuda", seed=5, map_dtype=dtype)
    w.spawn_cells(gen_genomes(n, 300))
    assert w.n_cells == n
    ws = [w, copy.deepcopy(w)]
    if dtype != torch.float32:
        for v in ws:
            v.degrade_molecules()
            v.diffuse_molecules()
            v.degrade_molecules()  # a pending scale on top of the pending correction
            assert v.__dict__.get("_pending_scale") is not None and v.__dict__.get("_pending_corr") is not None
    return ws


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("chem,n", [("wl", 1), ("wl", 19), ("wl", 257), ("wl", 4096), ("syn300", 5)])
def test_mask_kernels_match_host_masks(chem, n, dtype):
    """prob_masks_kernel (fast_prob_masks) over the inputs of the host test -- special molecule
    values, genome lengths 0, 1, 500, 2^31 - 1 written to the length column for the launch -- and the
    masks prob_spill_kernel leaves behind a World.kill_divide_prob equal _host.prob_masks bit for
    bit, with the paid column; the fused launch's spill leaves the map (fp32, and bf16 with a pending
    degradation and correction) as the torch masks + kill_divide_t of a deep copy do. The world-level
    leg decides on the world's own genome lengths (its genomes are read afterwards). One cell, a
    partial last workgroup, many workgroups, and more molecules than threads (one cell per
    workgroup)."""
    from magicsoup_amd.ops import hip_ops

    if chem == "wl":
        chemistry, mol = CHEMISTRY, CHEMISTRY.molname_2_idx["ATP"]
    else:
        from magicsoup_amd.examples.synthetic import make_chemistry

        chemistry, mol = make_chemistry(300, 600, seed=3), 7
        assert len(chemistry.molecules) > 256
    w, ref = _mask_worlds(chemistry, n, dtype)
    x, g = selection_inputs(n)
    for v in (w, ref):
        v.cell_molecules[:, mol] = torch.from_numpy(x).cuda()
    m_ = native.hip()

    # --- the mask kernel alone, on the test's genome lengths
    fw = w._fast_world(2 * n)
    col, lens = w.cell_molecules[:, mol].clone(), w._genomes.lens[:n].clone()
    w._genomes.lens[:n] = torch.from_numpy(g).cuda()
    mols_h = w.cell_molecules.cpu().numpy()
    kill, div = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    cost = 1.5
    try:
        for rule in rule_cases():
            kill.fill_(7), div.fill_(7)
            m_.fast_prob_masks(fw, n, mol, *_rule_args(rule), cost, float(rule.get("kill_fraction", 0.0)), 99, 12,
                               kill.data_ptr(), div.data_ptr(), hip_ops._stream())
            hk, hd = host_masks(mols_h, mol, g, rule, 99, 12)
            assert np.array_equal(kill.cpu().numpy(), hk.astype(np.uint8)), rule
            assert np.array_equal(div.cpu().numpy(), hd.astype(np.uint8)), rule
            paid = torch.from_numpy(x) - cost * torch.from_numpy(hd)
            assert torch.equal(_bits(w.cell_molecules[:, mol].cpu()), _bits(paid)), rule
            w.cell_molecules[:, mol] = col
    finally:
        w._genomes.lens[:n] = lens
    assert torch.equal(_bits(w.cell_molecules[:, mol]), _bits(col))

    # --- the fused launch, through the world
    assert (w.__dict__.get("_pending_scale") is not None) == (dtype != torch.float32)
    seed, call = _next_call(17)
    w.kill_divide_prob(mol, divide_cost=cost, **RULE)
    hk, hd = _oracle_masks(ref, mol, RULE, seed ^ MASK_KEY, call)
    bufs = w.__dict__["_fw_bufs"]
    assert torch.equal(bufs["kmask"][:n].bool(), hk) and torch.equal(bufs["dvmask"][:n].bool(), hd)
    ms.set_seed(17)
    ref.cell_molecules[:, mol] -= cost * hd
    ref.kill_divide_t(hk, hd)
    assert w.n_cells == ref.n_cells and w.last_kill == ref.last_kill
    assert w.molecule_map.dtype == dtype
    assert torch.equal(_bits(w.molecule_map), _bits(ref.molecule_map))
    assert torch.equal(_bits(w.cell_molecules), _bits(ref.cell_molecules))
    assert torch.equal(w.cell_map, ref.cell_map) and torch.equal(w.cell_positions, ref.cell_positions)
    if n >= 19:
        assert 0 < int(hk.sum()) < n


def test_kill_divide_prob_matches_masks_on_gpu():
    """The fused probabilistic kill / replicate (one native call: masks, payment, kill, division)
    leaves the world bit for bit as the host core's masks at the key-separated seed + kill_divide_t
    do, over 3 steps with the activity in between."""
    from tests.test_gpu_kernels import _world

    base = _world("cuda", map_size=64, n=1500, s=400, seed=12)
    base.synchronize()
    atp = CHEMISTRY.molname_2_idx["ATP"]
    rule = dict(kill_k=1.0, kill_n=2, divide_k=4.0, divide_n=3, genome_k=450.0, genome_n=7, kill_fraction=0.02)
    w1, w2 = copy.deepcopy(base), copy.deepcopy(base)
    for step in range(3):
        w1.enzymatic_activity()
        w2.enzymatic_activity()
        seed, call = _next_call(20 + step)
        n = w1.n_cells
        w1.kill_divide_prob(atp, divide_cost=2.0, **rule)
        assert w1.__dict__.get("_count_pending") is not None
        ms.set_seed(20 + step)
        kill, div = _oracle_masks(w2, atp, rule, seed ^ MASK_KEY, call)
        assert 0 < int(kill.sum()) < n and 0 < int(div.sum()) < n
        w2.cell_molecules[:, atp] -= 2.0 * div
        w2.kill_divide_t(kill, div)
        for k in STATE:
            assert torch.equal(getattr(w1, k), getattr(w2, k)), (step, k)
        assert list(w1.cell_genomes) == list(w2.cell_genomes) and w1.last_kill == w2.last_kill
    w1.check_invariants()


def test_saturated_rule_equals_threshold_call_on_gpu():
    base, atp = saturated_world("cuda")
    base.synchronize()
    n = base.n_cells
    w1, w2 = copy.deepcopy(base), copy.deepcopy(base)
    ms.set_seed(4)
    w1.kill_divide_prob(atp, **SATURATED)
    ms.set_seed(4)
    w2.kill_divide_where(atp, 1.0, 1e6, 2.0)
    assert w1.n_cells == w2.n_cells
    for k in STATE:
        assert torch.equal(getattr(w1, k), getattr(w2, k)), k
    assert list(w1.cell_genomes) == list(w2.cell_genomes)
    assert w1.last_kill == w2.last_kill == (n, n - (n + 2) // 3)
    w1.check_invariants()


def _body_strip_kill_divide_prob(rank, ws):
    """A strip world's kill_divide_prob (native masks, kill, division mask compacted on the device,
    lazy strip division) evolves the strip exactly as one burned call + the host core's masks +
    kill_cells + divide_cells_t(lazy=True) do."""
    from magicsoup_amd.ops import hip_ops
    from magicsoup_amd.parallel import DistributedWorld

    ms.set_seed(41)
    torch.manual_seed(41)
    w = ms.World(chemistry=CHEMISTRY, map_size=64, seed=41, device="cpu")
    w.spawn_cells(gen_genomes(1200, 300))
    atp = CHEMISTRY.molname_2_idx["ATP"]
    rule = dict(kill_k=0.5, kill_n=2, divide_k=2.0, divide_n=3, genome_k=400.0, genome_n=7, kill_fraction=0.02)
    out, kills = {}, {}
    for mode in ("masks", "prob"):
        dw = DistributedWorld(chemistry=CHEMISTRY, map_size=64, seed=42, device="cuda", strips=True)
        dw.adopt_maps(w)
        dw.scatter_from(w, maps=False)
        ms.set_seed(43)
        for it in range(3):
            dw.enzymatic_activity()
            if mode == "prob":
                dw.kill_divide_prob(atp, divide_cost=1.0, **rule)
            else:
                seed, call = hip_ops._rng()
                n = dw.n_cells
                hk, hd = host_masks(dw.cell_molecules.cpu().numpy(), atp, dw._genomes.lens[:n].cpu().numpy(), rule,
                                    seed ^ MASK_KEY, call)
                kill, repl = torch.from_numpy(hk).cuda(), torch.from_numpy(hd).cuda()
                assert 0 < int(kill.sum()) < n and 0 < int(repl.sum()) < n
                dw.cell_molecules[:, atp] -= 1.0 * repl
                dw.kill_cells(kill)
                kills.setdefault(mode, []).append((n, dw.n_cells))
                dw.divide_cells_t(repl[~kill], lazy=True)
            dw.degrade_molecules()
            dw.diffuse_molecules()
            dw.increment_cell_lifetimes()
            if mode == "prob":  # (the diffusion completed the lazy division: the counts are in)
                kills.setdefault(mode, []).append(tuple(dw.last_kill))
        dw.synchronize()
        dw.check_invariants("strip kill_divide_prob")
        out[mode] = (dw.cell_positions.cpu(), dw.cell_molecules.cpu(), dw.cell_divisions.cpu(), list(dw.cell_genomes))
        dw.close()
    a, b = out["masks"], out["prob"]
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert kills["masks"] == kills["prob"]


def test_strip_kill_divide_prob_matches_masks():
    run_ranks(_body_strip_kill_divide_prob, 1, timeout=300, backend="nccl")


def test_kill_divide_prob_does_not_wait_for_the_device():
    """With timings that do not drain the device, kill_divide_prob on a plain GPU world returns with
    both counts pending (behind an event) and the host's cell count not yet adopted."""
    from tests.test_gpu_kernels import _world

    w = _world("cuda", map_size=64, n=1500, s=400, seed=8)
    w.enzymatic_activity()
    w.synchronize()
    atp = CHEMISTRY.molname_2_idx["ATP"]
    w.enable_timings(sync=False)
    n = w.n_cells
    w.kill_divide_prob(atp, kill_k=1.0, divide_k=4.0, divide_cost=2.0, genome_k=450.0, kill_fraction=0.05)
    d = w.__dict__
    assert d.get("_count_pending") is not None and d["_count_pending"][0] == n and d["n_cells"] == n
    w.degrade_molecules()  # (count-safe: still pending)
    assert d.get("_count_pending") is not None
    n_new = w.n_cells  # adopts the counts
    assert d.get("_count_pending") is None and n_new >= w.last_kill[1] and w.last_kill[0] == n and w.last_kill[1] < n
    assert "kill_divide" in w.step_timings()
    w.check_invariants()
