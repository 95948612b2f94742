"""The register integrator's entry loops (kinetics.hip integrate_item_fast): wave-uniform exponent
classes (all exponents <= 1, <= 2, < 8, general), one or two powers per entry, entries in groups of
four. Every variant must give the bits of the LDS path (mode 8) and of the host core, and the same
iteration masks (GPU only)."""
import copy
import functools

import pytest
import torch

import magicsoup_amd as ms
from magicsoup_amd.examples.wood_ljungdahl import CHEMISTRY
from magicsoup_amd.ops import kinetics_ops, native
from tests.conftest import gen_genomes

pytestmark = pytest.mark.gpu

TRIMS = (0.7, 0.2, 0.1)
N_ITERS = 4


@functools.lru_cache(maxsize=None)
def _base_world(n):
    ms.set_seed(3)
    torch.manual_seed(3)
    w = ms.World(chemistry=CHEMISTRY, map_size=32 if n < 100 else 64, device="cpu", seed=3)
    w.spawn_cells(gen_genomes(n, 500))
    return w


def _world(n):
    return copy.deepcopy(_base_world(n))  # (the cached world itself stays unchanged)


def _state(w):
    pos = w.cell_positions.long()
    return torch.cat([w.cell_molecules, w.molecule_map[:, pos[:, 0], pos[:, 1]].T], dim=1).contiguous()


def _params(w):
    kin = w.kinetics
    return {k: getattr(kin, k).clone() for k in ("N", "Nf", "Nb", "A")}


def _set_params(w, p):
    p["N"] = p["Nb"] - p["Nf"]
    for k, t in p.items():
        setattr(w.kinetics, k, t)


def _clamp_exponents(p, cells, top):
    for k in ("Nf", "Nb"):
        p[k][cells] = p[k][cells].clamp(max=top)


def _max_exponent(p):
    return torch.maximum(p["Nf"], p["Nb"]).amax(dim=(1, 2))


def _integrate_all(wc, X):
    """X integrated by the host core, the register path (mode 0) and the LDS path (mode 8)."""
    wg = copy.deepcopy(wc).to("cuda")
    Xh = X.clone()
    res = {"host": (Xh, kinetics_ops.integrate(wc.kinetics, Xh, TRIMS, N_ITERS))}
    try:
        for mode in (0, 8):
            native.hip().set_integrate_mode(mode)
            Xk = X.cuda()
            masks = kinetics_ops.integrate(wg.kinetics, Xk, TRIMS, N_ITERS)
            res[mode] = (Xk.cpu(), masks)
    finally:
        native.hip().set_integrate_mode(0)
    return res


def _assert_identical(res, X):
    reg, reg_masks = res[0]
    assert not torch.equal(reg.nan_to_num(-1.0), X.nan_to_num(-1.0))  # (something was integrated)
    for ref in (8, "host"):
        out, masks = res[ref]
        assert torch.equal(torch.isnan(reg), torch.isnan(out)), ref
        assert torch.equal(reg.nan_to_num(-1.0), out.nan_to_num(-1.0)), ref
        assert list(reg_masks) == list(masks), ref
    return reg


@pytest.mark.parametrize("n", [2, 9, 300])
def test_population_sizes(n):
    """One wave with both halves; a full block of 8 groups plus a block with one live group; 300."""
    w = _world(n)
    assert w.n_cells == n
    X = _state(w)
    _assert_identical(_integrate_all(w, X), X)


@functools.lru_cache(maxsize=None)
def _all_ones_result():
    w = _world(300)
    p = _params(w)
    _clamp_exponents(p, slice(None), 1)
    assert int(_max_exponent(p).max()) == 1  # class 1 in every wave
    _set_params(w, p)
    X = _state(w)
    return _assert_identical(_integrate_all(w, X), X)


def test_class_one_population():
    _all_ones_result()


def test_class_two_population():
    w = _world(300)
    p = _params(w)
    _clamp_exponents(p, slice(None), 2)
    mx = _max_exponent(p)
    assert int(mx.max()) == 2 and int((mx == 2).sum()) >= 10 and int((mx == 1).sum()) >= 10
    _set_params(w, p)
    X = _state(w)
    _assert_identical(_integrate_all(w, X), X)


@pytest.mark.parametrize("top", [2, 3, 7, 8, 17])
def test_class_boundary_inside_a_wave(top):
    """Even cells carry exponents 1 only, odd cells a largest exponent of `top`: the class is a
    wave-wide decision, and an exponent-1 cell gives the same bits whatever its neighbour's class."""
    w = _world(300)
    p = _params(w)
    _clamp_exponents(p, slice(None), 1)
    odd = torch.arange(1, 300, 2)
    for k in ("Nf", "Nb"):
        cols = p[k][odd, :, ::3]
        p[k][odd, :, ::3] = torch.where(cols > 0, top, cols)
    mx = _max_exponent(p)
    assert int(mx[::2].max()) == 1
    assert int(mx[1::2].max()) == top and int((mx[1::2] == top).sum()) >= 100
    _set_params(w, p)
    X = _state(w)
    reg = _assert_identical(_integrate_all(w, X), X)
    assert torch.equal(reg[::2], _all_ones_result()[::2])


@pytest.mark.parametrize("top", [1, 2])
def test_entries_with_both_exponents(top):
    """A signal consumed and produced by one protein (two powers per entry) in every third cell."""
    w = _world(300)
    p = _params(w)
    _clamp_exponents(p, slice(None), 2)
    col = 1
    third = torch.arange(0, 300, 3)
    nf = p["Nf"][third, :, col].clamp(max=top)
    nf[::2] = torch.where(nf[::2] > 0, top, nf[::2])
    p["Nf"][third, :, col] = nf
    p["Nb"][third, :, col] = nf
    both = (p["Nf"] > 0) & (p["Nb"] > 0)
    assert int(both[third].sum()) >= 20
    assert int((p["Nf"][both] == top).sum()) >= 5 and int((p["Nb"][both] == top).sum()) >= 5
    if top == 2:
        assert int((p["Nf"][both] == 1).sum()) >= 1
    _set_params(w, p)
    X = _state(w)
    _assert_identical(_integrate_all(w, X), X)


@pytest.mark.parametrize("top", [1, 2])
def test_allosteric_entries(top):
    """Allosteric entries in some proteins of a wave and none in others, with classes 1 and 2."""
    w = _world(300)
    p = _params(w)
    _clamp_exponents(p, slice(None), top)
    has = (p["A"] != 0).any(dim=2)
    assert int(has.sum()) >= 50 and int(has.any(dim=1).sum()) >= 50  # proteins / cells with one
    assert int((~has.any(dim=1)).sum()) >= 50  # cells without any
    assert int(_max_exponent(p).max()) == top
    _set_params(w, p)
    X = _state(w)
    _assert_identical(_integrate_all(w, X), X)


def test_entry_count_boundaries():
    """Proteins with exactly 1, 4, 5, 8, 15, 16 non-zero signals (the groups of four), and 17 (which
    leaves the narrow register path through the overflow list)."""
    counts = (1, 4, 5, 8, 15, 16, 17)
    w = _world(64)
    p = _params(w)
    vmax = w.kinetics.Vmax
    cells = []
    for i, k in enumerate(counts):
        for cell in (2 * i, 2 * i + 33):  # (twice each: an even and an odd cell)
            prot = int(torch.nonzero(vmax[cell] > 0)[0])
            for name in ("Nf", "Nb", "A"):
                p[name][cell, prot] = 0
            p["Nf"][cell, prot, :k] = 1 + (i % 2)
            cells.append((cell, prot, k))
    _set_params(w, p)
    kin = w.kinetics
    nz = ((kin.N != 0) | (kin.Nf != 0) | (kin.Nb != 0) | (kin.A != 0)).sum(dim=2)
    for cell, prot, k in cells:
        assert int(nz[cell, prot]) == k
    assert sorted({int(nz[c, q]) for c, q, _ in cells}) == list(counts)
    X = _state(w)
    _assert_identical(_integrate_all(w, X), X)


@pytest.mark.parametrize("top", [1, 2])
def test_special_values(top):
    """0, a denormal, a value whose square overflows, Inf and NaN in signals that class-1 / class-2
    entries read."""
    values = (0.0, 1e-40, 1e30, float("inf"), float("nan"))
    w = _world(300)
    p = _params(w)
    _clamp_exponents(p, slice(None), top)
    X = _state(w)
    placed = 0
    for r, val in enumerate(values):
        for cell in range(r, 300, 10):
            used = ((p["Nf"][cell] > 0) | (p["Nb"][cell] > 0)).any(dim=0)
            if not used.any():
                continue
            j = int(torch.nonzero(used)[0])
            for k in ("Nf", "Nb"):
                p[k][cell, :, j] = torch.where(p[k][cell, :, j] > 0, top, p[k][cell, :, j])
            X[cell, j] = val
            placed += 1
    assert placed >= 100
    assert int(_max_exponent(p).max()) == top
    _set_params(w, p)
    reg = _assert_identical(_integrate_all(w, X), X)
    assert torch.isnan(reg).any()  # (the NaN inputs reach the results: the NaN masks are compared)
