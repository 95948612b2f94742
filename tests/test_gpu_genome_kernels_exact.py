"""The genome arena kernels against their exact CPU replay (GPU).

``mut_count`` / ``mut_apply`` / ``rec_count`` / ``rec_count_keys`` / ``rec_apply`` (``csrc/hip/mutations.hip``,
``csrc/hip/rec_common.h``) draw everything from ``Philox(seed, stream, item)``, so ``tests/genome_oracle.py``
replays a launch draw for draw and assembles the results independently. Every output byte, length and
count is compared with ``==``: there is no tolerance in this file. Genomes sit in one byte pool at ragged
offsets (16-aligned and odd), seeds and calls have non-zero high words, item indices are sparse and
large, and output buffers are prefilled with a sentinel that must survive past every ``out_len`` and in
a guard region behind the last row. ``arena_scatter`` allocates by atomics, so its tests assert the
properties of a commit instead of offsets.
"""
import numpy as np
import pytest
import torch

from tests import genome_oracle as go

pytestmark = pytest.mark.gpu

SEED, CALL = 0xC0FFEE12_3456_789A, 0x0000_0007_0000_0005
SENT, GUARD, FILL = 0xEE, 4096, ord("N")  # output sentinel, guard bytes, pool bytes between genomes
NK = 70_000  # entries of the k arrays: the items of a launch are a sparse few of them


def _m():
    from magicsoup_amd.ops import native

    return native.hip()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None) -> torch.Tensor:
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()  # (a writable copy)


def _p(t) -> int:
    return 0 if t is None else t.data_ptr()


def _genomes(lengths, seed: int) -> list:
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"TCGA", dtype=np.uint8)
    return [lut[rng.integers(0, 4, int(n))].tobytes() for n in lengths]


class Arena:
    """Genomes in one byte pool at ragged offsets: even genomes 16-aligned, odd ones at an odd byte,
    filler bytes between them (a kernel that reads past a genome emits a byte outside the alphabet).
    ``at``: the arena row of each genome (default: its index) among ``nrows`` rows."""

    def __init__(self, genomes, at=None, nrows=None):
        at = list(range(len(genomes))) if at is None else list(at)
        nrows = len(genomes) if nrows is None else nrows
        off, lens = np.zeros(nrows, dtype=np.int64), np.zeros(nrows, dtype=np.int32)
        chunks, cur = [], 0
        for j, g in enumerate(genomes):
            start = (cur + 15) // 16 * 16 if j % 2 == 0 else cur | 1
            chunks.append(bytes([FILL]) * (start - cur) + g + bytes([FILL]) * (j % 3))
            off[at[j]], lens[at[j]] = start, len(g)
            cur = start + len(g) + j % 3
        self.data = _dev(np.frombuffer(b"".join(chunks) + bytes([FILL]) * 64, dtype=np.uint8))
        self.off, self.lens = _dev(off), _dev(lens)
        assert (off[at][0::2] % 16 == 0).all() and (off[at][1::2] % 2 == 1).all()


def _sparse(items, values, dtype, fill=0) -> torch.Tensor:
    a = np.full((NK,) + np.shape(values)[1:], fill, dtype=dtype)
    a[np.asarray(items)] = values
    return _dev(a)


def _check_rows(out, out_len, want, out_width, extra_rows=0):
    """Rows of ``out`` (flat, with the guard behind) == the oracle's results clipped to out_width; the
    sentinel survives behind every row's length, in ``extra_rows`` further rows and in the guard."""
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    n = len(want)
    rows = out[: (n + extra_rows) * out_width].reshape(n + extra_rows, out_width)
    for j, w in enumerate(want):
        seq, ln = go.clip(w, out_width)
        assert out_len[j] == ln, (j, int(out_len[j]), ln)
        assert rows[j, :ln].tobytes() == seq, j
        assert (rows[j, ln:] == SENT).all(), j
    assert (rows[n:] == SENT).all() and (out_len[n:] == -7).all()
    assert out[(n + extra_rows) * out_width:].size == GUARD and (out[(n + extra_rows) * out_width:] == SENT).all()


def _out(nrows: int, out_width: int):
    return (torch.full((nrows * out_width + GUARD,), SENT, dtype=torch.uint8, device="cuda"),
            torch.full((nrows,), -7, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------ mut_apply
MUT_LENGTHS = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1025, 4097)
MUT_COUNTS = (1, 2, 31, 32, 33, 40, None)  # None: every position
MUT_TABLE = [(L, min(c or L, L)) for L in MUT_LENGTHS for c in MUT_COUNTS]
MUT_ITEMS = [11 + 907 * j for j in range(len(MUT_TABLE))]
MUT_RATES = [(0.4, 0.66), (1.0, 0.0), (1.0, 1.0), (0.0, 0.5)]


@pytest.fixture(scope="module")
def mut_genomes():
    return _genomes([L for L, _ in MUT_TABLE], seed=5)


def _mut_apply(arena, sel, k, rows, p_indel, p_del, out_width, dn=None):
    nsel = len(sel)
    out, out_len = _out(nsel, out_width)
    sel_d = _dev(sel, np.int64)
    _m().mut_apply(nsel, _p(dn), sel_d.data_ptr(), _p(rows), arena.data.data_ptr(), arena.off.data_ptr(),
                   arena.lens.data_ptr(), k.data_ptr(), p_indel, p_del, SEED, CALL, out.data_ptr(), out_width,
                   out_len.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out, out_len


@pytest.mark.parametrize("via_rows", [False, True], ids=["direct", "rows"])
@pytest.mark.parametrize("p_indel,p_del", MUT_RATES)
def test_mut_apply_table_matches_oracle(mut_genomes, p_indel, p_del, via_rows):
    n = len(MUT_TABLE)
    if via_rows:  # item j works on arena row perm[j]: a permutation with one row twice
        perm = [(30 * j + 7) % n for j in range(n)]
        perm[9] = perm[5]
        arena = Arena(mut_genomes)
        rows = _sparse(MUT_ITEMS, perm, np.int64)
    else:  # item i works on arena row i
        perm = list(range(n))
        arena = Arena(mut_genomes, at=MUT_ITEMS, nrows=NK)
        rows = None
    k = _sparse(MUT_ITEMS, [MUT_TABLE[g][1] for g in perm], np.int32)
    out_width = max(MUT_LENGTHS) + 40 + 16
    out, out_len = _mut_apply(arena, MUT_ITEMS, k, rows, p_indel, p_del, out_width)
    want = [go.mutate(mut_genomes[g], SEED, CALL, i, MUT_TABLE[g][1], p_indel, p_del) for g, i in zip(perm, MUT_ITEMS)]
    assert sum(w != mut_genomes[g] for w, g in zip(want, perm)) > n // 2
    _check_rows(out, out_len, want, out_width)


def _layout(L, edits):
    """Output offsets of a mutated genome's pieces: copied segments (start, length), literals (start, n)."""
    segs, lits, w, prev = [], [], 0, 0
    for t, kind, _ in edits:
        segs.append((w, t - prev))
        w += t - prev
        nl = {go.SUB: 1, go.INS: 2, go.DEL: 0}[kind]
        lits.append((w, nl))
        w += nl
        prev = t + 1
    segs.append((w, L - prev))
    return segs, lits, w + L - prev


@pytest.mark.parametrize("L,k,item", [(4097, 2, 12_345), (513, 40, 54_321)], ids=["floyd", "serial"])
def test_mut_apply_clips_at_out_width(L, k, item):
    """One item per launch, so a byte written past the row lands in the guard. Pure insertions: the
    result is L + k long, the cuts are W, W - 1, inside a copied segment of more than 512 bytes (first
    case) and between the two bytes of an insertion's literal."""
    (g,) = _genomes([L], seed=L)
    arena = Arena([b"ACGT", g], at=[0, item], nrows=NK)  # (the genome sits at an odd offset)
    kd = _sparse([item], [k], np.int32)
    edits = go.mut_plan(SEED, CALL, item, L, k, 1.0, 0.0)
    want = go.apply_edits(g, edits)
    segs, lits, W = _layout(L, edits)
    assert W == len(want) == L + k and all(nl == 2 for _, nl in lits)
    widths = [W, W - 1, lits[0][0] + 1, lits[-1][0] + 1]
    if L > 4000:
        s0, sl = max(segs, key=lambda s: s[1])
        assert sl > 1100
        widths += [s0 + 512 + 70, s0 + sl - 3]  # in the unrolled part and in the remainder of the copy
    for out_width in widths:
        out, out_len = _mut_apply(arena, [item], kd, None, 1.0, 0.0, out_width)
        _check_rows(out, out_len, [want], out_width)


def test_mut_apply_device_count_and_grid_stride():
    """A capacity of 3000 items with 2500 live: more items than blocks (the grid is capped at 2048), so
    blocks reuse their LDS plan; rows past the live count stay untouched. Then a live count of 0."""
    cap, live, out_width = 3000, 2500, 64
    lengths = [33 + (7 * j) % 15 for j in range(cap)]
    items = [3 * j + 1 for j in range(cap)]
    ks = [1 + j % 3 for j in range(cap)]
    genomes = _genomes(lengths, seed=6)
    arena = Arena(genomes, at=items, nrows=NK)
    k = _sparse(items, ks, np.int32)
    dn = _dev([live], np.int32)
    out, out_len = _mut_apply(arena, items, k, None, 0.4, 0.66, out_width, dn=dn)
    want = [go.mutate(genomes[j], SEED, CALL, items[j], ks[j], 0.4, 0.66) for j in range(live)]
    _check_rows(out, out_len, want, out_width, extra_rows=cap - live)
    out, out_len = _mut_apply(arena, items, k, None, 0.4, 0.66, out_width, dn=_dev([0], np.int32))
    _check_rows(out, out_len, [], out_width, extra_rows=cap)


# ------------------------------------------------------------------------------------ rec_apply
REC_PAIRS = ((0, 5), (5, 0), (1, 1), (64, 64), (511, 513), (1000, 37), (2048, 2048))
REC_COUNTS = (1, 2, 31, 32, 33, 40, None)  # None: a break at every position
REC_TABLE = [(n0, n1, min(c or n0 + n1, n0 + n1)) for n0, n1 in REC_PAIRS for c in REC_COUNTS]
REC_ITEMS = [23 + 1409 * j for j in range(len(REC_TABLE))]
REC_WIDTH = 4096


class RecSetup:
    def __init__(self):
        self.genomes = _genomes([n for n0, n1, _ in REC_TABLE for n in (n0, n1)], seed=7)
        # genome 2j / 2j+1 are strands a / b of pair j; their arena rows are swapped for odd j (a > b)
        at = [r for j in range(len(REC_TABLE)) for r in ((2 * j, 2 * j + 1) if j % 2 == 0 else (2 * j + 1, 2 * j))]
        self.cells = np.array(at, dtype=np.int64).reshape(-1, 2)
        self.arena = Arena(self.genomes, at=at)
        self.pairs = _sparse(REC_ITEMS, self.cells, np.int32)
        self.keys = _sparse(REC_ITEMS, (self.cells[:, 0] << 32) | self.cells[:, 1], np.int64, fill=-1)
        self.ks = [k for _, _, k in REC_TABLE]
        self.k = _sparse(REC_ITEMS, self.ks, np.int32)
        self.parts_cap = max(self.ks) + 2
        self._want = None

    def want(self, j):
        if self._want is None:
            self._want = [go.recombine(self.genomes[2 * q], self.genomes[2 * q + 1], SEED, CALL, REC_ITEMS[q], self.ks[q])
                          for q in range(len(REC_TABLE))]
        return self._want[j]

    def apply(self, sel, out_width, use_keys, dn=None):
        nsel = len(sel)
        out, out_len = _out(2 * nsel, out_width)
        out_rows = torch.full((2 * nsel,), -3, dtype=torch.int64, device="cuda")
        parts = torch.full((nsel * self.parts_cap * 3,), -1, dtype=torch.int32, device="cuda")
        sel_d = _dev(sel, np.int64)
        _m().rec_apply(nsel, _p(dn), sel_d.data_ptr(), 0 if use_keys else self.pairs.data_ptr(),
                       self.keys.data_ptr() if use_keys else 0, self.arena.data.data_ptr(), self.arena.off.data_ptr(),
                       self.arena.lens.data_ptr(), self.k.data_ptr(), SEED, CALL, parts.data_ptr(), self.parts_cap,
                       out.data_ptr(), out_width, out_len.data_ptr(), out_rows.data_ptr(), _stream())
        torch.cuda.synchronize()
        return out, out_len, out_rows.cpu().numpy()


@pytest.fixture(scope="module")
def rec():
    return RecSetup()


def test_rec_apply_table_matches_oracle_with_pairs_and_keys(rec):
    n = len(REC_TABLE)
    want = [r for j in range(n) for r in rec.want(j)]
    assert sum(rec.want(j) != (rec.genomes[2 * j], rec.genomes[2 * j + 1]) for j in range(n)) > n // 2
    res = []
    for use_keys in (False, True):
        out, out_len, out_rows = rec.apply(REC_ITEMS, REC_WIDTH, use_keys)
        _check_rows(out, out_len, want, REC_WIDTH)
        assert np.array_equal(out_rows, rec.cells.reshape(-1))
        res.append((out.cpu().numpy(), out_len.cpu().numpy(), out_rows))
    assert all(np.array_equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("j", [REC_TABLE.index((1000, 37, 2)), REC_TABLE.index((511, 513, 40))], ids=["floyd", "serial"])
def test_rec_apply_clips_at_out_width(rec, j):
    r0, r1 = rec.want(j)
    for out_width in (max(len(r0), len(r1)) - 3, max(min(len(r0), len(r1)) - 1, 1)):
        out, out_len, out_rows = rec.apply([REC_ITEMS[j]], out_width, use_keys=False)
        _check_rows(out, out_len, [r0, r1], out_width)
        assert out_rows.tolist() == rec.cells[j].tolist()


def test_rec_apply_device_count(rec):
    n, cap = len(REC_TABLE), len(REC_TABLE) + 11
    sel = REC_ITEMS + [REC_ITEMS[0]] * (cap - n)
    out, out_len, out_rows = rec.apply(sel, REC_WIDTH, use_keys=True, dn=_dev([n], np.int32))
    _check_rows(out, out_len, [r for j in range(n) for r in rec.want(j)], REC_WIDTH, extra_rows=2 * (cap - n))
    assert np.array_equal(out_rows[: 2 * n], rec.cells.reshape(-1)) and (out_rows[2 * n:] == -3).all()


# ------------------------------------------------------------------------------------ counts
def _count_buffers(n):
    k = torch.full((n + 64,), -9, dtype=torch.int32, device="cuda")
    return k, torch.zeros(1, dtype=torch.int32, device="cuda")


def _flag_word(gflags):
    return None if gflags is None else _dev([gflags], np.int32)


@pytest.mark.parametrize("name", [c[0] for c in go.MUT_COUNT_CASES])
def test_mut_count_matches_oracle(name):
    _, n, rows, p, kcap, gflags = next(c for c in go.MUT_COUNT_CASES if c[0] == name)
    want, amb, op = go.mut_count_case(name)
    assert not amb.any()
    lens, rows_d, gf = _dev(go.count_lens()), _dev(go.count_rows(n)) if rows else None, _flag_word(gflags)
    k, opflags = _count_buffers(n)
    _m().mut_count(n, _p(rows_d), lens.data_ptr(), p, go.COUNT_SEED, go.COUNT_CALL, k.data_ptr(), kcap, _p(gf),
                   opflags.data_ptr(), _stream())
    k = k.cpu().numpy()
    assert np.array_equal(k[:n], want) and (k[n:] == -9).all()
    assert int(opflags.item()) == op and (gf is None or int(gf.item()) == gflags)


@pytest.mark.parametrize("name", [c[0] for c in go.REC_COUNT_CASES])
def test_rec_count_matches_oracle(name):
    _, n, p = next(c for c in go.REC_COUNT_CASES if c[0] == name)
    want, amb = go.rec_count_case(name)
    assert not amb.any()
    lens, pairs = _dev(go.count_lens()), _dev(go.count_pairs(n))
    k, _ = _count_buffers(n)
    _m().rec_count(n, pairs.data_ptr(), lens.data_ptr(), p, go.COUNT_SEED, go.COUNT_CALL, k.data_ptr(), _stream())
    k = k.cpu().numpy()
    assert np.array_equal(k[:n], want) and (k[n:] == -9).all()


@pytest.mark.parametrize("name", [c[0] for c in go.REC_KEYS_CASES])
def test_rec_count_keys_matches_oracle(name):
    _, n, p, kcap, gflags, longest = next(c for c in go.REC_KEYS_CASES if c[0] == name)
    want, want_tot, amb, op = go.rec_keys_case(name)
    assert not amb.any()
    lens, keys, gf = _dev(go.count_lens()), _dev(go.count_keys(n)), _flag_word(gflags)
    lw = None if longest is None else _dev([(77 << 32) | longest], np.int64)  # (generation << 32) | longest
    for with_tot in (True, False):
        k, opflags = _count_buffers(n)
        tot, _ = _count_buffers(n)
        _m().rec_count_keys(n, keys.data_ptr(), lens.data_ptr(), p, go.COUNT_SEED, go.COUNT_CALL, k.data_ptr(),
                            tot.data_ptr() if with_tot else 0, kcap, _p(gf), opflags.data_ptr(), _stream(), _p(lw))
        k, tot = k.cpu().numpy(), tot.cpu().numpy()
        assert np.array_equal(k[:n], want) and (k[n:] == -9).all()
        assert np.array_equal(tot[:n], want_tot) if with_tot else (tot == -9).all()
        assert (tot[n:] == -9).all() and int(opflags.item()) == op


# ------------------------------------------------------------------------------------ arena_scatter
TOP0, OFF0, LEN0 = 48, -5, -6  # pool bytes in use before the call, untouched off / lens cells


def _r16(n: int) -> int:
    return (max(n, 1) + 15) // 16 * 16


class Scatter:
    """One arena_scatter call on fresh buffers (or on ``prev``'s arena, for a second generation)."""

    def __init__(self, rows, src_len, src_width, width, *, ncell=64, pool_cap=1 << 16, mark=False, gen=1, flags=False,
                 gflags=False, dn=None, dn_mul=1, src_shift=0, prev=None, data_seed=9):
        k = len(rows)
        rng = np.random.default_rng(data_seed)
        lut = np.frombuffer(b"TCGA", dtype=np.uint8)
        maxw = max(max(src_len), 1)
        self.full = lut[rng.integers(0, 4, (k, maxw))]  # (the same data whatever the row pitch)
        assert src_width >= maxw
        src = np.full((k, src_width), FILL, dtype=np.uint8)
        for q in range(k):
            src[q, : src_len[q]] = self.full[q, : src_len[q]]
        buf = torch.full((k * src_width + 32,), FILL, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[src_shift: src_shift + k * src_width] = _dev(src.reshape(-1))
        self.rows, self.src_len, self.width, self.pool_cap, self.k = list(rows), list(src_len), width, pool_cap, k
        if prev is None:
            self.pool = torch.full((pool_cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
            self.off = torch.full((ncell,), OFF0, dtype=torch.int64, device="cuda")
            self.lens = torch.full((ncell,), LEN0, dtype=torch.int32, device="cuda")
            self.top = torch.full((1,), TOP0, dtype=torch.int64, device="cuda")
            self.mark = torch.zeros(ncell, dtype=torch.int64, device="cuda") if mark else None
        else:
            self.pool, self.off, self.lens, self.top, self.mark = prev.pool, prev.off, prev.lens, prev.top, prev.mark
        self.before = (self.off.cpu().numpy().copy(), self.lens.cpu().numpy().copy(), int(self.top.item()))
        self.flags = torch.full((k,), 7, dtype=torch.uint8, device="cuda") if flags else None
        self.gflags = torch.zeros(1, dtype=torch.int32, device="cuda") if gflags else None
        self.opflags = torch.zeros(1, dtype=torch.int32, device="cuda") if gflags else None
        rows_d, len_d = _dev(rows, np.int64), _dev(src_len, np.int32)
        dn_d = None if dn is None else _dev([dn], np.int32)
        _m().arena_scatter(k, _p(dn_d), dn_mul, rows_d.data_ptr(), buf.data_ptr() + src_shift, src_width, len_d.data_ptr(),
                           self.pool.data_ptr(), self.off.data_ptr(), self.top.data_ptr(), pool_cap, width,
                           self.lens.data_ptr(), _p(self.mark), gen, _p(self.flags), _p(self.gflags), _p(self.opflags),
                           _stream())
        torch.cuda.synchronize()

    def check(self, winners: dict, left: set = frozenset(), n_commit=None):
        """``winners``: cell -> result row that must be committed to it (unless the cell is in ``left``:
        then it must be unchanged, as every other cell). Returns the committed cells."""
        pool, off, lens = self.pool.cpu().numpy(), self.off.cpu().numpy(), self.lens.cpu().numpy()
        off0, lens0, top0 = self.before
        top, spans, allocated = int(self.top.item()), [], 0
        for cell, q in winners.items():
            L = min(self.src_len[q], self.width)
            if cell in left:
                continue
            o = int(off[cell])
            assert lens[cell] == L and o % 16 == 0 and o >= top0 and o + _r16(L) <= min(top, self.pool_cap), (cell, q, o)
            assert pool[o: o + L].tobytes() == self.full[q, :L].tobytes(), (cell, q)
            spans.append((o, o + _r16(L)))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # pairwise disjoint
        same = [c for c in range(len(off)) if c not in winners or c in left]
        assert np.array_equal(off[same], off0[same]) and np.array_equal(lens[same], lens0[same])
        assert (pool[:TOP0] == SENT).all() and (pool[self.pool_cap:] == SENT).all()
        return top - top0, sum(b - a for a, b in spans)


SCATTER_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 299, 7, 255, 256, 257, 100, 2, 48, 200]


@pytest.mark.parametrize("src_width,shift", [(304, 0), (301, 0), (304, 1)], ids=["vector", "odd-pitch", "odd-base"])
def test_arena_scatter_commits_rows_on_vector_and_byte_paths(src_width, shift):
    k = len(SCATTER_LENS)
    rows = [(11 * q + 3) % 64 for q in range(k)]
    assert len(set(rows)) == k
    s = Scatter(rows, SCATTER_LENS, src_width, width=512, src_shift=shift)
    grew, used = s.check({r: q for q, r in enumerate(rows)})
    assert grew == used == sum(_r16(n) for n in SCATTER_LENS)
    # the same data gives the same genomes on every path
    ref = Scatter(rows, SCATTER_LENS, 304, width=512)
    off, roff, pool, rpool = s.off.cpu().numpy(), ref.off.cpu().numpy(), s.pool.cpu().numpy(), ref.pool.cpu().numpy()
    assert torch.equal(s.lens, ref.lens) and torch.equal(s.top, ref.top)
    for q, r in enumerate(rows):
        n = SCATTER_LENS[q]
        assert pool[off[r]: off[r] + n].tobytes() == rpool[roff[r]: roff[r] + n].tobytes()


def _winners(rows):
    return {r: q for q, r in enumerate(rows)}  # the highest q of a cell


def test_arena_scatter_last_writer_wins_across_generations():
    lens1 = [(37 * q) % 300 for q in range(40)]
    rows1 = [(5 * q) % 13 for q in range(40)]
    a = Scatter(rows1, lens1, 304, width=512, mark=True, gen=5, flags=True)
    win = _winners(rows1)
    grew, used = a.check(win)
    assert grew == used == sum(_r16(min(lens1[q], 512)) for q in win.values())
    assert a.flags.cpu().tolist() == [int(win[r] == q) for q, r in enumerate(rows1)]
    # the next generation on the uncleared marks: fewer rows, so every old mark has a higher q
    lens2 = [(53 * q + 1) % 300 for q in range(30)]
    rows2 = [(3 * q) % 11 for q in range(30)]
    b = Scatter(rows2, lens2, 301, width=512, mark=True, gen=6, flags=True, prev=a, data_seed=10)
    win = _winners(rows2)
    grew, used = b.check(win)
    assert grew == used == sum(_r16(lens2[q]) for q in win.values())
    assert b.flags.cpu().tolist() == [int(win[r] == q) for q, r in enumerate(rows2)]


def test_arena_scatter_too_long_results():
    lens = [100, 101, 99, 250, 0, 100, 300, 16]
    rows = [9, 2, 7, 4, 1, 6, 3, 8]
    long = {r for r, n in zip(rows, lens) if n > 100}
    s = Scatter(rows, lens, 304, width=100, gflags=True, flags=True)  # left for the host
    grew, used = s.check(_winners(rows), left=long)
    assert grew == used == sum(_r16(n) for n in lens if n <= 100)
    assert int(s.gflags.item()) == go.GP_WIDTH and int(s.opflags.item()) == go.GP_WIDTH
    assert s.flags.cpu().tolist() == [1] * len(rows)
    s = Scatter(rows, lens, 304, width=100)  # no flag word: committed truncated
    grew, used = s.check(_winners(rows))
    assert grew == used == sum(_r16(min(n, 100)) for n in lens) and int(s.lens.max().item()) == 100


def test_arena_scatter_pool_full():
    k, fit = 12, 5
    rows = [(7 * q + 2) % 64 for q in range(k)]
    s = Scatter(rows, [64] * k, 64, width=512, pool_cap=TOP0 + 64 * fit + 20, gflags=True)
    off = s.off.cpu().numpy()
    failed = {r for r in rows if off[r] == OFF0}
    assert len(failed) == k - fit  # equal sizes: exactly the allocations below the cap succeed
    grew, used = s.check(_winners(rows), left=failed)
    assert grew == 64 * k and used == 64 * fit
    assert int(s.gflags.item()) == go.GP_WIDTH and int(s.opflags.item()) == go.GP_WIDTH


def test_arena_scatter_device_count():
    cap, dn = 40, 13  # two result rows per item: 26 live rows
    rows = [(11 * q + 3) % 64 for q in range(cap)]
    lens = [(29 * q + 5) % 200 for q in range(cap)]
    s = Scatter(rows, lens, 208, width=512, mark=True, gen=3, flags=True, dn=dn, dn_mul=2)
    grew, used = s.check({r: q for q, r in enumerate(rows[: 2 * dn])})
    assert grew == used == sum(_r16(n) for n in lens[: 2 * dn])
    assert s.flags.cpu().tolist() == [1] * (2 * dn) + [0] * (cap - 2 * dn)


# ------------------------------------------------------------------------------------ end to end
def _world():
    import magicsoup_amd as ms
    from magicsoup_amd.examples.wood_ljungdahl import CHEMISTRY

    ms.set_seed(3)
    torch.manual_seed(3)
    w = ms.World(chemistry=CHEMISTRY, map_size=32, device="cuda", seed=3)
    w.spawn_cells([ms.random_genome(200 + (37 * i) % 401) for i in range(200)])
    return w


def _cell_genomes(w) -> list:
    return [g.encode() for g in w.cell_genomes]


def _oracle_point_mutations(before, rows, p, p_indel, p_del, seed, call):
    lens = [len(g) for g in before]
    n = len(before) if rows is None else len(rows)
    k, amb, _ = go.mut_count(n, rows, lens, p, seed, call)
    assert not amb.any()
    after, hit = list(before), []
    for i in np.nonzero(k)[0].tolist():  # in item order: the last mutated copy of a cell wins
        r = i if rows is None else rows[i]
        after[r] = go.mutate(before[r], seed, call, i, int(k[i]), p_indel, p_del)
        hit.append(r)
    return after, hit, k


def test_world_point_mutations_match_oracle():
    from magicsoup_amd.ops import hip_ops

    w = _world()
    before = _cell_genomes(w)
    assert len(before) == w.n_cells >= 150 and len({len(g) for g in before}) > 50
    changed = hip_ops.point_mutations(w, None, 1e-3, 0.4, 0.66, rng=(SEED, CALL))
    want, hit, _ = _oracle_point_mutations(before, None, 1e-3, 0.4, 0.66, SEED, CALL)
    assert len(hit) >= 20 and sorted(changed.tolist()) == hit
    assert _cell_genomes(w) == want
    # explicit rows with a cell three times
    before = want
    rows = [(13 * i + 5) % w.n_cells for i in range(60)]
    rows[40], rows[57] = rows[2], rows[2]
    changed = hip_ops.point_mutations(w, torch.tensor(rows, device="cuda"), 1e-2, 0.4, 0.66, rng=(SEED + 1, CALL + (1 << 32)))
    want, hit, k = _oracle_point_mutations(before, rows, 1e-2, 0.4, 0.66, SEED + 1, CALL + (1 << 32))
    assert k[2] > 0 and k[40] > 0 and k[57] > 0 and len(set(hit)) >= 20  # (every copy of the cell mutates)
    assert sorted(changed.tolist()) == sorted(set(hit))
    assert _cell_genomes(w) == want


def test_world_recombinations_match_oracle():
    from magicsoup_amd.ops import hip_ops

    w = _world()
    before = _cell_genomes(w)
    n, p = w.n_cells, 3e-4
    keys = hip_ops.neighbor_slot_keys(w)[: 8 * n].cpu().numpy().copy()
    lens = [len(g) for g in before]
    k, tot, amb, _ = go.rec_count_keys(8 * n, keys, lens, p, SEED, CALL, longest=max(lens))
    assert not amb.any()
    want, pairs = list(before), 0
    for i in np.nonzero(k)[0].tolist():  # in slot order: a cell keeps the result of its last slot
        a, b = int(keys[i]) >> 32, int(keys[i]) & go.M32
        want[a], want[b] = go.recombine(before[a], before[b], SEED, CALL, i, int(k[i]))
        pairs += 1
    assert pairs >= 10
    changed = hip_ops.recombinate_all(w, p, rng=(SEED, CALL))
    hit = {int(keys[i]) >> 32 for i in np.nonzero(k)[0]} | {int(keys[i]) & go.M32 for i in np.nonzero(k)[0]}
    assert sorted(changed.tolist()) == sorted(hit)
    assert _cell_genomes(w) == want
