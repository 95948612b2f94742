"""The CPU replay oracle of the genome kernels (``tests/genome_oracle.py``) against things that are not
the kernels: the host's Philox uniforms, the defining properties of its samplers, plans and assembly,
and the requirement that no count of the shared count table depends on the last bit of a device
``exp`` / ``log`` / ``cos`` (the GPU tests compare those counts with ``==``)."""
import numpy as np
import pytest

from magicsoup_amd.ops import native
from tests import genome_oracle as go

SEED, CALL = 0xDEADBEEF_1234_5678, 0x0000_0009_8000_0003


def _genome(n: int, salt: int) -> bytes:
    return bytes(b"TCGA"[(i * 2654435761 + salt * 40503 >> 7) & 3] for i in range(n))


# ------------------------------------------------------------------------------------ stream
@pytest.mark.parametrize("seed,call", [(SEED, CALL), (go.COUNT_SEED, go.COUNT_CALL), (1, 0), (2 ** 64 - 1, 2 ** 64 - 1)])
def test_device_rng_layout_matches_host_uniforms(seed, call):
    """counter = (item, call_lo, call_hi, block), key = (seed_lo, seed_hi), words handed out x, y, z, w"""
    first = 0xFFFF_FF00
    u = np.asarray(native.host().selection_uniforms(300, seed, call, first))
    for i in (0, 1, 2, 63, 255, 299):
        rng = go.DeviceRng(seed, call, first + i)  # (items wrap at 2^32 as the uint32 counter word does)
        assert [np.float32(rng.uniform()) for _ in range(4)] == list(u[i])


def test_device_rng_blocks_and_derived_draws():
    rng = go.DeviceRng(SEED, CALL, 5)
    words = [rng.u32() for _ in range(8)]
    key = (SEED & go.M32, SEED >> 32)
    assert tuple(words[:4]) == go.philox4x32_10((5, CALL & go.M32, CALL >> 32, 0), key)
    assert tuple(words[4:]) == go.philox4x32_10((5, CALL & go.M32, CALL >> 32, 1), key)
    a, b = go.DeviceRng(SEED, CALL, 5), go.DeviceRng(SEED, CALL, 5)
    assert a.uniform_d() == ((words[0] << 21) ^ (words[1] >> 11)) / 2.0 ** 53
    assert [b.below(n) for n in (1, 4, 1000)] == [0, (words[1] * 4) >> 32, (words[2] * 1000) >> 32]
    assert 0.0 <= a.uniform_d() < 1.0


# ------------------------------------------------------------------------------------ samplers
@pytest.mark.parametrize("k", list(range(1, go.FLOYD_MAX + 1)))
def test_floyd_sorted_gives_k_distinct_sorted_positions(k):
    for n in (k, k + 1, 2 * k + 3, 4097):
        pos = go.floyd_sorted(go.DeviceRng(SEED, CALL, 100 * k + n), n, k)
        assert len(pos) == k and pos == sorted(set(pos)) and 0 <= pos[0] and pos[-1] < n
    assert go.floyd_sorted(go.DeviceRng(SEED, CALL, k), k, k) == list(range(k))


@pytest.mark.parametrize("n,k", [(33, 33), (40, 33), (64, 40), (513, 40), (4097, 33), (4097, 4097), (50, 49)])
def test_serial_sampling_selects_exactly_k(n, k):
    pos = go.serial_positions(go.DeviceRng(SEED, CALL, n + k), n, k)
    assert len(pos) == k and pos == sorted(set(pos)) and 0 <= pos[0] and pos[-1] < n


def test_poisson_branches():
    assert go.poisson(go.DeviceRng(1, 2, 3), 0.0) == (0, False)
    assert go.poisson(go.DeviceRng(1, 2, 3), float("nan")) == (0, False)
    for lam in (1e-4, 1.0, 29.9, 30.1, 1000.0):
        ks = [go.poisson(go.DeviceRng(SEED, CALL, i), lam)[0] for i in range(400)]
        sd = (lam / 400) ** 0.5
        assert abs(np.mean(ks) - lam) < 5 * sd + 1e-3, lam  # (a sanity bound on the oracle itself)
    rng = go.DeviceRng(SEED, CALL, 0)
    go.poisson(rng, 29.9)
    assert (rng.block, rng.have) == (1, 2)  # one uniform_d below 30 ...
    rng = go.DeviceRng(SEED, CALL, 0)
    go.poisson(rng, 30.1)
    assert (rng.block, rng.have) == (1, 0)  # ... two above


# ------------------------------------------------------------------------------------ plans + assembly
MUT_SHAPES = [(L, k) for L in (1, 2, 63, 64, 65, 513) for k in (1, 2, 31, 32, 33, 40, L) if k <= L]


@pytest.mark.parametrize("p_indel,p_del", [(0.4, 0.66), (1.0, 0.0), (1.0, 1.0), (0.0, 0.5)])
def test_edit_lists_have_k_positions_and_assemble(p_indel, p_del):
    for item, (L, k) in enumerate(MUT_SHAPES):
        g = _genome(L, item)
        edits = go.mut_plan(SEED, CALL, item, L, k, p_indel, p_del)
        pos = [e[0] for e in edits]
        assert len(pos) == k and pos == sorted(set(pos)) and 0 <= pos[0] and pos[-1] < L
        kinds = [e[1] for e in edits]
        assert all((nt is None) == (kind == go.DEL) and (nt is None or nt in go.NTS) for _, kind, nt in edits)
        if p_indel == 0.0:
            assert set(kinds) == {go.SUB}
        if p_indel == 1.0:
            assert set(kinds) == {go.DEL if p_del == 1.0 else go.INS}
        new = go.apply_edits(g, edits)
        assert len(new) == L + kinds.count(go.INS) - kinds.count(go.DEL)
        # base by base, without slicing
        by, want = {t: (kind, nt) for t, kind, nt in edits}, bytearray()
        for t in range(L):
            kind, nt = by.get(t, (None, None))
            want += {None: g[t:t + 1], go.SUB: bytes([nt or 0]), go.INS: bytes([nt or 0]) + g[t:t + 1], go.DEL: b""}[kind]
        assert new == bytes(want)


def test_apply_edits_semantics_by_hand():
    g = b"TTCCGGAA"
    a = ord("A")
    assert go.apply_edits(g, [(0, go.DEL, None)]) == b"TCCGGAA"
    assert go.apply_edits(g, [(7, go.DEL, None)]) == b"TTCCGGA"
    assert go.apply_edits(g, [(2, go.INS, a)]) == b"TTACCGGAA"  # before the base
    assert go.apply_edits(g, [(2, go.SUB, a)]) == b"TTACGGAA"
    assert go.apply_edits(g, [(0, go.INS, a), (1, go.DEL, None), (7, go.SUB, ord("C"))]) == b"ATCCGGAC"
    assert go.clip(b"ACGT", 3) == (b"ACG", 3) and go.clip(b"ACGT", 9) == (b"ACGT", 4)


REC_SHAPES = [(n0, n1, k) for n0, n1 in ((0, 5), (5, 0), (1, 1), (64, 64), (511, 513), (1000, 37))
              for k in (1, 2, 31, 32, 33, 40, n0 + n1) if k <= n0 + n1]


def test_recombination_parts_partition_both_strands():
    seen_empty = 0
    for item, (n0, n1, k) in enumerate(REC_SHAPES):
        a, b = _genome(n0, item), _genome(n1, item + 1000)
        cuts, parts, shuffled, split = go.rec_plan(SEED, CALL, item, n0, n1, k)
        assert len(cuts) == k and cuts == sorted(set(cuts)) and 0 <= cuts[0] and cuts[-1] < n0 + n1
        assert len(parts) == k + 2 and sorted(parts) == sorted(shuffled) and 0 <= split < k + 2
        for strand, n, own in ((0, n0, [c for c in cuts if c < n0]), (1, n1, [c - n0 for c in cuts if c >= n0])):
            mine = [p for p in parts if p[0] == strand]
            # consecutive [a0, a1) from 0 to n, broken exactly at the strand's cuts
            assert [p[1] for p in mine] == [0] + own and [p[2] for p in mine] == own + [n]
            seen_empty += sum(p[1] == p[2] for p in mine)
        r0, r1 = go.rec_assemble(a, b, shuffled, split)
        assert len(r0) + len(r1) == n0 + n1
        piece = [(a, b)[s][a0:a1] for s, a0, a1 in shuffled]
        assert r0 + r1 == b"".join(piece) and len(r0) == sum(len(x) for x in piece[:split])
        assert sorted(piece) == sorted((a, b)[s][a0:a1] for s, a0, a1 in parts)
    assert seen_empty > 0  # (cuts at 0 / n0 and the empty strands are among the cases)


def test_rec_assemble_by_hand():
    a, b = b"AAAA", b"CCGG"
    shuffled = [(1, 2, 4), (0, 0, 1), (1, 0, 2), (0, 1, 4)]
    assert go.rec_assemble(a, b, shuffled, 0) == (b"", b"GGACCAAA")
    assert go.rec_assemble(a, b, shuffled, 1) == (b"GG", b"ACCAAA")
    assert go.rec_assemble(a, b, shuffled, 3) == (b"GGACC", b"AAA")


# ------------------------------------------------------------------------------------ the count table
@pytest.mark.parametrize("name", [c[0] for c in go.MUT_COUNT_CASES])
def test_mut_count_table_has_no_ambiguous_count(name):
    _, n, rows, p, kcap, gflags = next(c for c in go.MUT_COUNT_CASES if c[0] == name)
    k, amb, op = go.mut_count_case(name)
    assert int(amb.sum()) == 0
    lens = go.count_lens()[go.count_rows(n)] if rows else go.count_lens()[:n]
    assert (k >= 0).all() and (k <= lens).all() and (kcap == 0 or (k <= kcap).all())
    if gflags is not None and gflags & go.GP_WIDTH:
        assert not k.any() and op == go.GP_SKIPPED
    else:
        assert op == 0 and (n < 255 or k.any())


def test_count_table_lengths_reach_every_branch():
    lens, lam = go.count_lens(), 0.1 * go.count_lens()
    assert {0, 1, 2, 299, 301, 10_000} <= set(lens.tolist())
    assert 0.1 * 299 < 30.0 < 0.1 * 301 and (lam[lens > 0] < 1.0).any()
    k, _, _ = go.mut_count_case("n5000-all-p5.0-cap0")
    for L in (1, 2):  # lambda 5 and 10: clamped to the length (P(draw < L) is 0.7 % and 0.05 %)
        at = k[:5000][lens[:5000] == L]
        assert at.max() == L and (at == L).mean() > 0.95
    k3, _, _ = go.mut_count_case("n5000-all-p0.1-cap3")
    k0, _, _ = go.mut_count_case("n5000-all-p0.1-cap0")
    assert np.array_equal(k3, np.minimum(k0, 3)) and (k0 > 3).any()
    kr, _, _ = go.mut_count_case("n5000-rows-p0.1-cap0")
    assert not np.array_equal(kr, k0)
    assert len(set(go.count_rows(5000).tolist())) < 5000  # (rows repeat)


@pytest.mark.parametrize("name", [c[0] for c in go.REC_COUNT_CASES])
def test_rec_count_table_has_no_ambiguous_count(name):
    k, amb = go.rec_count_case(name)
    assert int(amb.sum()) == 0 and (len(k) < 200 or k.any())


@pytest.mark.parametrize("name", [c[0] for c in go.REC_KEYS_CASES])
def test_rec_keys_table_has_no_ambiguous_count(name):
    _, n, p, kcap, gflags, longest = next(c for c in go.REC_KEYS_CASES if c[0] == name)
    k, tot, amb, op = go.rec_keys_case(name)
    assert int(amb.sum()) == 0
    keys = go.count_keys(n)
    assert (keys < 0).any() and not k[keys < 0].any() and not tot[keys < 0].any()
    if gflags is not None and gflags & go.GP_WIDTH:
        assert not k.any() and not tot.any() and op == go.GP_SKIPPED
    else:
        assert op == 0 and k.any() and (k <= tot).all() and (kcap == 0 or (k <= kcap).all())
        assert tot[keys >= 0].any()
