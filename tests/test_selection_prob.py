"""Probabilistic (Hill-curve) kill / divide selection on the host: the Philox block, the masks of
``_host.prob_masks`` against a numpy float32 oracle, and ``World.kill_divide_prob`` on CPU worlds."""
import copy

import numpy as np
import pytest
import torch

import magicsoup_amd as ms
from magicsoup_amd.examples.wood_ljungdahl import CHEMISTRY
from magicsoup_amd.ops import native
from tests.conftest import gen_genomes
from tests.dist_utils import run_ranks
from tests.genome_oracle import M32, philox4x32_10

F = np.float32


# ------------------------------------------------------------------------------------ oracles
def oracle_words(seed, call, item):
    return philox4x32_10((item & M32, call & M32, (call >> 32) & M32, 0), (seed & M32, (seed >> 32) & M32))


def oracle_uniforms(n, seed, call, first=0):
    w = np.array([oracle_words(seed, call, first + i) for i in range(n)], dtype=np.uint64)
    return ((w >> np.uint64(8)).astype(F) * F(2.0 ** -24)).astype(F)


def _ipow(x, n):
    """ms::ipow: square and multiply from the low bit, fp32 products in that order."""
    r, b, e = np.ones_like(x), x.copy(), n
    while e:
        if e & 1:
            r = r * b
        b = b * b
        e >>= 1
    return r


def _rise(v, k, n):
    with np.errstate(all="ignore"):
        return np.where(v > 0, F(1) / (F(1) + _ipow(F(k) / v, n)), F(0)).astype(F)


def _fall(v, k, n):
    with np.errstate(all="ignore"):
        return np.where(v > 0, F(1) / (F(1) + _ipow(v / F(k), n)), F(1)).astype(F)


def oracle_masks(x, g, u, rule):
    """The normative decision in numpy float32: x (n,) molecule, g (n,) int genome lengths, u (n, 4)."""
    kill = u[:, 0] < F(rule.get("kill_fraction", 0.0))
    if rule.get("kill_k") is not None:
        kill |= u[:, 1] < _fall(x, rule["kill_k"], rule["kill_n"])
    if rule.get("genome_k") is not None:
        kill |= u[:, 2] < _rise(g.astype(F), rule["genome_k"], rule["genome_n"])
    div = np.zeros_like(kill)
    if rule.get("divide_k") is not None:
        div = ~kill & (u[:, 3] < _rise(x, rule["divide_k"], rule["divide_n"]))
    return kill, div


def host_masks(mols, mol, g, rule, seed, call):
    """_host.prob_masks with a rule dict (None / missing k: the term is off)."""
    a = []
    for t, n0 in (("kill", 1), ("divide", 3), ("genome", 7)):
        k = rule.get(f"{t}_k")
        a += [k is not None, 1.0 if k is None else float(k), int(rule.get(f"{t}_n", n0))]
    kill, div = native.host().prob_masks(mols, mol, g, *a, float(rule.get("kill_fraction", 0.0)), seed, call)
    return np.asarray(kill).astype(bool), np.asarray(div).astype(bool)


# ------------------------------------------------------------------------------------ inputs
KILL_K, DIVIDE_K, GENOME_K = 0.5, 20.0, 450.0
# (value, killed by an enabled molecule term for sure, divides for sure when divide_k is set)
SPECIALS = [(0.0, True, False), (-1.0, True, False), (float("nan"), True, False), (float("inf"), False, True),
            (1e-45, True, False), (1e-30, None, None), (1e30, None, None), (KILL_K, None, None), (DIVIDE_K, None, None)]
GENOME_SPECIALS = [0, 1, 500, 2 ** 31 - 1]


def selection_inputs(n, seed=11):
    """x (n,) float32 log-uniform over 1e-6..1e6 with the special values at fixed places (as many as
    fit), g (n,) int32 genome lengths around GENOME_K with 0, 1, 500 and 2^31 - 1 among them."""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-6, 6, n)).astype(F)
    g = rng.integers(100, 1000, n).astype(np.int32)
    for j, (v, _, _) in enumerate(SPECIALS[: max(0, n - 1)]):
        x[1 + j] = F(v)
    for j, v in enumerate(GENOME_SPECIALS):
        if 11 + j < n:
            g[11 + j] = v
    return x, g


def rule_cases():
    full = dict(kill_k=KILL_K, divide_k=DIVIDE_K, genome_k=GENOME_K, kill_fraction=0.05)
    cases = []
    for e in (1, 2, 3, 5, 15):
        cases.append(dict(full, kill_n=e, divide_n=e, genome_n=e))
    base = dict(full, kill_n=1, divide_n=3, genome_n=7)
    for off in ("kill_k", "divide_k", "genome_k"):
        cases.append(dict(base, **{off: None}))
    cases.append(dict(base, kill_fraction=0.0))
    cases.append(dict(kill_fraction=0.25))  # a pure dilution
    cases.append(dict(base, kill_k=None, genome_k=None, kill_fraction=0.0))  # division only
    return cases


SEED, CALL = 0x1234_5678_9ABC_DEF0, 0x0000_0003_0000_0007


# ------------------------------------------------------------------------------------ 1. Philox
def test_philox_oracle_reproduces_random123_vectors():
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_selection_uniforms_known_answers():
    h = native.host()
    u = np.asarray(h.selection_uniforms(1, 0, 0))
    assert u.dtype == np.float32 and u.shape == (1, 4)
    words = np.array([0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], dtype=np.uint64) >> np.uint64(8)
    assert np.array_equal(u[0], words.astype(F) * F(2.0 ** -24))
    top = 0xFFFFFFFFFFFFFFFF
    u = np.asarray(h.selection_uniforms(1, top, top, M32))  # counter (ffffffff, ffffffff, ffffffff, 0)
    assert np.array_equal(u, oracle_uniforms(1, top, top, M32))
    for seed, call in ((SEED, CALL), (0xDEADBEEF_00000001, 0x8000_0000_0000_0000)):
        u = np.asarray(h.selection_uniforms(257, seed, call))
        assert np.array_equal(u, oracle_uniforms(257, seed, call))
        assert (u >= 0).all() and (u < 1).all()


# ------------------------------------------------------------------------------------ 2. masks
@pytest.fixture(scope="module")
def inputs():
    x, g = selection_inputs(4096)
    mols = np.zeros((4096, 5), dtype=F)
    mols[:, 0] = 1e3  # (other columns must not matter)
    mols[:, 2] = x
    return mols, g, oracle_uniforms(4096, SEED, CALL)


@pytest.mark.parametrize("rule", rule_cases(), ids=[f"rule{i}" for i in range(len(rule_cases()))])
def test_prob_masks_match_numpy_oracle(inputs, rule):
    mols, g, u = inputs
    kill, div = host_masks(mols, 2, g, rule, SEED, CALL)
    ok, od = oracle_masks(mols[:, 2], g, u, rule)
    assert np.array_equal(kill, ok) and np.array_equal(div, od)
    assert not (kill & div).any()
    assert 0 < (kill | div).sum() < 4096  # (a rule that decides nothing checks nothing)


def test_prob_masks_special_values(inputs):
    mols, g, _ = inputs
    rule = dict(kill_k=KILL_K, kill_n=3, divide_k=DIVIDE_K, divide_n=3)  # (no dilution, no genome term)
    kill, div = host_masks(mols, 2, g, rule, SEED, CALL)
    for j, (v, killed, divides) in enumerate(SPECIALS):
        if killed is not None:
            assert kill[1 + j] == killed and div[1 + j] == divides, v
    # +inf survives the molecule term whatever the division rule
    kill, _ = host_masks(mols, 2, g, dict(kill_k=KILL_K, kill_n=1), SEED, CALL)
    assert not kill[1 + 3]
    # the genome term alone never kills an empty genome, and kills a 2^31 - 1 one for sure
    kill, div = host_masks(mols, 2, g, dict(genome_k=GENOME_K, genome_n=7), SEED, CALL)
    assert not kill[11] and kill[11 + 3] and not div.any()
    assert 0 < kill.sum() < 4096


# ------------------------------------------------------------------------------------ 3. properties
def test_prob_masks_nesting_and_independent_draws(inputs):
    mols, g, _ = inputs
    base = dict(kill_k=KILL_K, kill_n=2, divide_k=DIVIDE_K, divide_n=3, kill_fraction=0.1)
    k0, d0 = host_masks(mols, 2, g, base, SEED, CALL)
    k1, d1 = host_masks(mols, 2, g, base, SEED, CALL)
    assert np.array_equal(k0, k1) and np.array_equal(d0, d1)  # same arguments, same masks
    prev = None
    for f in (0.0, 0.1, 0.5, 1.0):
        k, _ = host_masks(mols, 2, g, dict(base, kill_fraction=f), SEED, CALL)
        if prev is not None:
            assert not (prev & ~k).any() and k.sum() > prev.sum()
        prev = k
    assert prev.all()  # kill_fraction 1 kills every cell
    prev = None
    for kk in (1e-3, KILL_K, 50.0, 1e5):  # a larger kill_k kills at higher concentrations
        k, _ = host_masks(mols, 2, g, dict(base, kill_k=kk), SEED, CALL)
        if prev is not None:
            assert not (prev & ~k).any() and k.sum() > prev.sum()
        prev = k
    kg, dg = host_masks(mols, 2, g, dict(base, genome_k=GENOME_K, genome_n=7), SEED, CALL)
    assert not (k0 & ~kg).any() and kg.sum() > k0.sum()  # the genome term only adds kills
    alive = ~k0 & ~kg
    assert np.array_equal(d0[alive], dg[alive]) and d0[alive].any()
    # another call or seed is another set of draws
    k2, _ = host_masks(mols, 2, g, base, SEED, CALL + 1)
    k3, _ = host_masks(mols, 2, g, base, SEED + 1, CALL)
    assert not np.array_equal(k0, k2) and not np.array_equal(k0, k3)


# ------------------------------------------------------------------------------------ 4. statistics
def test_prob_masks_frequencies():
    """65,536 cells at one concentration: each term fires on 0.3 n cells within 5 binomial standard
    deviations. x / k = 7 / 3 makes the fp32 probability 0.3 to within an ulp (asserted on the
    oracle), which moves the expected count by less than 0.01 cells."""
    n = 65536
    sd = (n * 0.3 * 0.7) ** 0.5
    g = np.full(n, 3, dtype=np.int32)
    assert abs(float(_fall(np.array([7], F), 3.0, 1)[0]) - 0.3) < 1e-6
    assert abs(float(_rise(np.array([3], F), 7.0, 1)[0]) - 0.3) < 1e-6
    mols = np.full((n, 1), 7.0, dtype=F)
    kill, div = host_masks(mols, 0, g, dict(kill_k=3.0, kill_n=1), 2024, 5)
    assert abs(int(kill.sum()) - 0.3 * n) < 5 * sd and not div.any()
    mols[:] = 3.0
    kill, div = host_masks(mols, 0, g, dict(divide_k=7.0, divide_n=1), 2024, 5)
    assert abs(int(div.sum()) - 0.3 * n) < 5 * sd and not kill.any()
    kill, _ = host_masks(mols, 0, g, dict(genome_k=7.0, genome_n=1), 2024, 5)  # g = 3
    assert abs(int(kill.sum()) - 0.3 * n) < 5 * sd
    kill, _ = host_masks(mols, 0, g, dict(kill_fraction=0.3), 2024, 5)
    assert abs(int(kill.sum()) - 0.3 * n) < 5 * sd


# ------------------------------------------------------------------------------------ 5. world level
STATE = ("cell_molecules", "cell_positions", "cell_divisions", "cell_lifetimes", "molecule_map", "cell_map")
SATURATED = dict(kill_k=1.0, kill_n=15, divide_k=1e6, divide_n=15, divide_cost=2.0)


def saturated_world(device, map_size=32, n=300, seed=7):
    """A world whose ATP is 1e-3 / 1e3 / 1e9 by thirds: under SATURATED the kill probabilities are
    exactly 1, 0, 0 and the division probabilities 0, 0, 1 in fp32."""
    ms.set_seed(seed)
    torch.manual_seed(seed)
    w = ms.World(chemistry=CHEMISTRY, map_size=map_size, seed=seed, device=device)
    w.spawn_cells(gen_genomes(n, 300))
    atp = CHEMISTRY.molname_2_idx["ATP"]
    vals = torch.tensor([1e-3, 1e3, 1e9], device=w.device)
    w.cell_molecules[:, atp] = vals[torch.arange(w.n_cells, device=w.device) % 3]
    return w, atp


def assert_same_world(w1, w2):
    assert w1.n_cells == w2.n_cells
    for k in STATE:
        assert torch.equal(getattr(w1, k), getattr(w2, k)), k
    assert list(w1.cell_genomes) == list(w2.cell_genomes) and w1.last_kill == w2.last_kill


def test_saturated_rule_equals_threshold_call():
    base, atp = saturated_world("cpu")
    n = base.n_cells
    w1, w2 = copy.deepcopy(base), copy.deepcopy(base)
    ms.set_seed(4)
    w1.kill_divide_prob(atp, **SATURATED)
    ms.set_seed(4)
    w2.kill_divide_where(atp, 1.0, 1e6, 2.0)
    assert_same_world(w1, w2)
    assert w1.last_kill == (n, n - (n + 2) // 3) and w1.n_cells > w1.last_kill[1]
    w1.check_invariants()


def test_world_kill_divide_prob_uses_molecule_name_and_genome_term():
    base, atp = saturated_world("cpu")
    w = copy.deepcopy(base)
    n = w.n_cells
    torch.manual_seed(1)
    w.kill_divide_prob("ATP", genome_k=1.0, genome_n=15)  # every genome is far longer than 1 nt
    assert w.n_cells == 0 and w.last_kill == (n, 0)
    w = copy.deepcopy(base)
    torch.manual_seed(1)
    w.kill_divide_prob("ATP", kill_fraction=0.5)  # a pure dilution
    assert 0.35 * n < w.n_cells < 0.65 * n  # (300 fair coins: 5 sd = 43 cells)
    w.check_invariants()


# ------------------------------------------------------------------------------------ 6. arguments
@pytest.mark.parametrize("kw", [
    dict(kill_n=0), dict(kill_n=16), dict(divide_n=2.0), dict(genome_n=-1), dict(genome_n=True),
    dict(kill_k=0.0), dict(kill_k=-1.0), dict(divide_k=float("inf")), dict(genome_k=float("nan")),
    dict(kill_fraction=-0.1), dict(kill_fraction=1.5), dict(kill_fraction=float("nan")),
], ids=str)
def test_kill_divide_prob_rejects_bad_arguments(kw):
    w, atp = saturated_world("cpu", map_size=16, n=10)
    before = w.cell_molecules.clone()
    with pytest.raises(ValueError):
        w.kill_divide_prob(atp, **{"kill_k": 1.0, "divide_k": 5.0, **kw})
    with pytest.raises(ValueError):
        w.kill_divide_prob(len(CHEMISTRY.molecules), kill_k=1.0)
    assert w.n_cells == 10 and torch.equal(w.cell_molecules, before)


def test_kill_divide_prob_without_cells_is_a_no_op():
    w = ms.World(chemistry=CHEMISTRY, map_size=16, seed=1)
    mm = w.molecule_map.clone()
    w.kill_divide_prob("ATP", kill_k=1.0, divide_k=5.0, genome_k=500.0, kill_fraction=0.1)
    assert w.n_cells == 0 and torch.equal(w.molecule_map, mm)


# ------------------------------------------------------------------------------------ 7. gloo strips
def _body_empty_strip_prob(rank, ws):
    """2 strips, every cell on rank 0: the saturated rule leaves the population of the threshold
    call, and a strip the kill empties (or that never had cells) still joins the division."""
    from magicsoup_amd.parallel import DistributedWorld

    atp = CHEMISTRY.molname_2_idx["ATP"]

    def world():
        ms.set_seed(3)
        torch.manual_seed(3)
        g = ms.World(chemistry=CHEMISTRY, map_size=16, seed=3)
        genomes = gen_genomes(21, 300)
        pos = torch.tensor([[i // 8, 2 * (i % 8)] for i in range(21)], dtype=torch.int32)
        g._grow(21)
        g._genomes.append_strings(genomes)
        g._labels.append_strings([f"c{i}" for i in range(21)])
        g._place(torch.arange(21), pos)
        g._update_params_rows(torch.arange(21))
        dw = DistributedWorld(chemistry=CHEMISTRY, map_size=16, seed=5, device="cpu")
        dw.scatter_from(g)
        assert dw.n_cells == (21 if rank == 0 else 0)
        n = dw.n_cells
        dw.cell_molecules[:, atp] = torch.tensor([1e-3, 1e3, 1e9])[torch.arange(n) % 3]
        return dw

    a, b = world(), world()
    ms.set_seed(9)
    a.kill_divide_prob(atp, **SATURATED)  # rank 0 kills 7 and divides 7, rank 1 is empty
    ms.set_seed(9)
    b.kill_divide_where(atp, 1.0, 1e6, 2.0)
    assert a.last_kill == b.last_kill == ((21, 14) if rank == 0 else (0, 0))
    assert a.n_cells == b.n_cells and torch.equal(a.cell_positions, b.cell_positions)
    assert torch.equal(a.cell_molecules, b.cell_molecules) and list(a.cell_genomes) == list(b.cell_genomes)
    # everything dies on rank 0 (its strip empties) and still completes; rank 1 keeps its arrivals
    n1 = a.n_cells
    a.cell_molecules[:, atp] = 1e-3 if rank == 0 else 1e3
    a.kill_divide_prob(atp, **SATURATED)
    assert a.n_cells == (0 if rank == 0 else n1) and a.last_kill == ((n1, 0) if rank == 0 else (n1, n1))
    a.kill_divide_prob(atp, **SATURATED)
    pos = a.cell_positions.long()
    assert int(a.owned_cell_map().sum()) == a.n_cells and bool(a.cell_map[pos[:, 0], pos[:, 1]].all())


def test_distributed_empty_strip_joins_kill_divide_prob():
    run_ranks(_body_empty_strip_prob, 2, timeout=120.0)
