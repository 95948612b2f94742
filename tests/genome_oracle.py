"""Exact CPU replay of the device genome kernels (``csrc/hip/mutations.hip``, ``csrc/hip/rec_common.h``).

Every random draw of ``mut_count`` / ``mut_apply`` / ``rec_count`` / ``rec_count_keys`` / ``rec_apply`` comes
from ``msd::Philox(seed, stream, item)`` (``csrc/hip/hip_common.h``), a counter RNG, so a launch can be
replayed draw for draw in Python ints and float64. The module has three layers:

* the stream (:class:`DeviceRng`) and the counts (:func:`poisson` and the count kernels), which mirror the
  kernels' arithmetic; a count carries an ``ambiguous`` flag where a last-bit difference of the device's
  ``exp`` / ``log`` / ``cos`` could change it;
* the plans (:func:`mut_plan`, :func:`rec_plan`), which mirror the kernels' order of draws and return an
  explicit edit list / part list;
* the assembly (:func:`apply_edits`, :func:`rec_assemble`, :func:`clip`), which knows nothing of the kernels:
  it applies the lists with plain slicing under the reference's semantics (``rust/mutations.rs``: a deletion
  removes the base, an insertion goes before it, a substitution replaces it; recombined parts are
  concatenated unaltered, those before the split into result 0 and the rest into result 1).

Pure Python and numpy; nothing here touches a GPU. The table of count cases at the end is shared by
``tests/test_genome_oracle.py`` (which asserts that none of its counts is ambiguous) and
``tests/test_gpu_genome_kernels_exact.py`` (which compares the kernels' counts with it).
"""
import functools
import math

import numpy as np

M32 = 0xFFFFFFFF
APPLY_STREAM = 0x6A09E667F3BCC909  # rec_common.h kApplyStream
FLOYD_MAX = 32  # rec_common.h kFloydMax
GP_WIDTH, GP_SKIPPED = 8, 16  # mutations.hip kGpWidth, kGpSkipped
NTS = b"ACTG"  # mutations.hip rand_nt
SUB, INS, DEL = "sub", "ins", "del"


# ------------------------------------------------------------------------------------ stream
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., Random123) on Python ints: counter (4 words), key (2 words)."""
    x0, x1, x2, x3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ k0, p1 & M32, (p0 >> 32) ^ x3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return x0, x1, x2, x3


class DeviceRng:
    """``msd::Philox(seed, stream, item)``: counter (item, stream_lo, stream_hi, block), key (seed_lo,
    seed_hi); the four words of a block are handed out in the order x, y, z, w."""

    def __init__(self, seed: int, stream: int, item: int):
        self.c0, self.c1, self.c2, self.block = item & M32, stream & M32, (stream >> 32) & M32, 0
        self.key = (seed & M32, (seed >> 32) & M32)
        self.buf: tuple = ()
        self.have = 0

    def u32(self) -> int:
        if self.have == 0:
            self.buf = philox4x32_10((self.c0, self.c1, self.c2, self.block), self.key)
            self.block = (self.block + 1) & M32
            self.have = 4
        self.have -= 1
        return self.buf[3 - self.have]

    def uniform(self) -> float:
        return (self.u32() >> 8) / 2.0 ** 24  # (exact in float32 and float64)

    def uniform_d(self) -> float:
        hi, lo = self.u32(), self.u32()
        return ((hi << 21) ^ (lo >> 11)) / 2.0 ** 53

    def below(self, n: int) -> int:
        return (self.u32() * n) >> 32


# ------------------------------------------------------------------------------------ counts
U_TOL, ROUND_TOL = 1e-12, 1e-6  # distances below which a count is called ambiguous


def poisson(rng: DeviceRng, lam: float):
    """``msd::poisson`` in float64: (k, ambiguous)."""
    if not lam > 0.0:
        return 0, False
    if lam < 30.0:
        u = rng.uniform_d()
        if u <= (1.0 - lam) - 1e-15:
            return 0, False
        p = math.exp(-lam)
        cum, k = p, 0
        amb = abs(u - cum) <= U_TOL
        while u > cum and k < 1000:
            k += 1
            p *= lam / float(k)
            cum += p
            amb = amb or abs(u - cum) <= U_TOL
        return k, amb
    u1, u2 = max(rng.uniform_d(), 1e-300), rng.uniform_d()
    z = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
    x = lam + math.sqrt(lam) * z + 0.5
    k = math.floor(x)
    return max(k, 0), abs(x - round(x)) <= ROUND_TOL


def _skipped(gflags):
    return gflags is not None and bool(gflags & GP_WIDTH)


def mut_count(n, rows, lens, p, seed, call, kcap=0, gflags=None):
    """``mut_count_kernel``: (k int32 (n,), ambiguous bool (n,), bits or-ed into opflags)."""
    k, amb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    if _skipped(gflags):
        return k, amb, GP_SKIPPED if n > 0 else 0
    for i in range(n):
        L = int(lens[i if rows is None else int(rows[i])])
        if L < 1:
            continue
        kk, amb[i] = poisson(DeviceRng(seed, call, i), p * float(L))
        if kcap > 0 and kk > kcap:
            kk = kcap
        k[i] = min(kk, L)
    return k, amb, 0


def rec_count(n, pairs, lens, p, seed, call):
    """``rec_count_kernel`` over int32 pairs (n, 2): (k, ambiguous)."""
    k, amb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    for i in range(n):
        nb = int(lens[int(pairs[i][0])]) + int(lens[int(pairs[i][1])])
        if nb < 1:
            continue
        kk, amb[i] = poisson(DeviceRng(seed, call, i), p * float(nb))
        k[i] = min(kk, nb)
    return k, amb


def rec_count_keys(n, keys, lens, p, seed, call, kcap=0, gflags=None, longest=None):
    """``rec_count_keys_kernel`` over int64 slot keys (a << 32) | b, -1 = empty: (k, tot, ambiguous, opflags
    bits). ``longest``: the low word of ``lw_word`` (thinned draw against len(a) + longest), None: direct."""
    k, tot, amb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    if _skipped(gflags):
        return k, tot, amb, GP_SKIPPED if n > 0 else 0
    for i in range(n):
        key = int(keys[i])
        if key < 0:
            continue
        la = int(lens[key >> 32])
        nb = la + int(lens[key & M32])
        tot[i] = nb
        kk = 0
        if longest is not None:
            lb = float(la) + float(longest)
            if lb >= 1.0:
                rng = DeviceRng(seed, call, i)
                nev, amb[i] = poisson(rng, p * lb)
                for _ in range(nev):
                    kk += 1 if rng.uniform_d() * lb < float(nb) else 0
        else:
            if nb < 1:
                continue
            kk, amb[i] = poisson(DeviceRng(seed, call, i), p * float(nb))
        if kcap > 0 and kk > kcap:
            kk = kcap
        k[i] = min(kk, nb)
    return k, tot, amb, 0


# ------------------------------------------------------------------------------------ plans
def floyd_sorted(rng: DeviceRng, n: int, k: int) -> list:
    """``floyd_sorted``: k distinct positions in [0, n), sorted (Floyd's sampling; k <= n)."""
    pos: list = []
    for j in range(n - k, n):
        t = rng.below(j + 1)
        if t in pos:
            t = j
        pos.append(t)
    return sorted(pos)


def mutate_at(rng: DeviceRng, p_indel: float, p_del: float):
    """``mutate_at``: the kind of one event and its drawn nucleotide (None for a deletion)."""
    if rng.uniform_d() < p_indel:
        if rng.uniform_d() < p_del:
            return DEL, None
        return INS, NTS[rng.below(4)]
    return SUB, NTS[rng.below(4)]


def serial_positions(rng: DeviceRng, n: int, k: int, on_pick=None) -> list:
    """Selection sampling as in the kernels' paths for k > kFloydMax: position t is chosen with chance
    need / (n - t), no draw once need is 0; ``on_pick(t)`` runs right after a pick (its draws interleave)."""
    need, pos = k, []
    for t in range(n):
        if need > 0 and rng.below(n - t) < need:
            need -= 1
            pos.append(t)
            if on_pick is not None:
                on_pick(t)
    return pos


def mut_plan(seed, call, item, L, k, p_indel, p_del) -> list:
    """``mut_apply_item``'s draws for a genome of L nt with k events: edits (position, kind, nucleotide)
    in position order."""
    rng = DeviceRng(seed, call ^ APPLY_STREAM, item)
    if k > FLOYD_MAX:
        edits: list = []
        serial_positions(rng, L, k, lambda t: edits.append((t, *mutate_at(rng, p_indel, p_del))))
        return edits
    return [(t, *mutate_at(rng, p_indel, p_del)) for t in floyd_sorted(rng, L, k)]


def rec_plan(seed, call, item, n0, n1, k):
    """``rec_pair_apply``'s draws: (cuts, parts in push order, shuffled parts, split index). A part is
    (strand, a0, a1); a cut at 0 or n0 and an empty strand give empty parts."""
    nb = n0 + n1
    rng = DeviceRng(seed, call ^ APPLY_STREAM, item)
    cuts = floyd_sorted(rng, nb, k) if k <= FLOYD_MAX else serial_positions(rng, nb, k)
    parts, start = [], 0
    for c in (c for c in cuts if c < n0):
        parts.append((0, start, c))
        start = c
    parts.append((0, start, n0))
    start = 0
    for c in (c for c in cuts if c >= n0):
        parts.append((1, start, c - n0))
        start = c - n0
    parts.append((1, start, n1))
    shuffled = list(parts)
    for q in range(len(shuffled) - 1, 0, -1):
        r = rng.below(q + 1)
        shuffled[q], shuffled[r] = shuffled[r], shuffled[q]
    return cuts, parts, shuffled, rng.below(len(shuffled))


# ------------------------------------------------------------------------------------ assembly
def apply_edits(genome: bytes, edits) -> bytes:
    out, prev = bytearray(), 0
    for pos, kind, nt in edits:
        out += genome[prev:pos]
        if kind == SUB:
            out.append(nt)
        elif kind == INS:
            out.append(nt)
            out.append(genome[pos])
        else:
            assert kind == DEL
        prev = pos + 1
    return bytes(out + genome[prev:])


def rec_assemble(a: bytes, b: bytes, shuffled, split: int):
    piece = [(a, b)[s][a0:a1] for s, a0, a1 in shuffled]
    return b"".join(piece[:split]), b"".join(piece[split:])


def clip(seq: bytes, out_width: int):
    """What an apply kernel leaves of a result in a row of out_width bytes: (bytes, out_len)."""
    return seq[:out_width], min(len(seq), out_width)


def mutate(genome: bytes, seed, call, item, k, p_indel, p_del) -> bytes:
    return apply_edits(genome, mut_plan(seed, call, item, len(genome), k, p_indel, p_del))


def recombine(a: bytes, b: bytes, seed, call, item, k):
    _, _, shuffled, split = rec_plan(seed, call, item, len(a), len(b), k)
    return rec_assemble(a, b, shuffled, split)


# ------------------------------------------------------------------------------------ count cases
# The fixed table of count launches that the GPU tests compare with the kernels. Everything is a
# constant: lengths come from the formulas below, never from a library RNG.
COUNT_SEED, COUNT_CALL = 0x9E3779B9_7F4A7C15, 0x0000_0005_0000_000B
POOL_ROWS = 6000
_LEN_CYCLE = (0, 1, 2, 299, 301, 10_000, 37, 1000, 513, 64, 5, 120)  # p = 0.1: lambda 29.9, 30.1, 1000


def count_lens() -> np.ndarray:
    """Genome lengths of the count cases' arena rows (int32 (POOL_ROWS,))."""
    r = np.arange(POOL_ROWS, dtype=np.int64)
    lens = np.array(_LEN_CYCLE, dtype=np.int64)[r % len(_LEN_CYCLE)]
    odd = (r // len(_LEN_CYCLE)) % 3 == 1  # every third cycle: other short lengths instead of the fixed ones
    return np.where(odd & (lens > 2), (r * 2654435761 >> 9) % 700, lens).astype(np.int32)


def count_rows(n: int) -> np.ndarray:
    """Row indirection of a count case: spread over the arena, with repeats (int64 (n,))."""
    i = np.arange(n, dtype=np.int64)
    r = (i * 7919 + 13) % POOL_ROWS
    dup = np.nonzero(i % 50 == 7)[0]
    r[dup] = r[dup - 3]
    return r


def count_pairs(n: int) -> np.ndarray:
    i = np.arange(n, dtype=np.int64)
    return np.stack([(i * 7919 + 13) % POOL_ROWS, (i * 104729 + 7) % POOL_ROWS], axis=1).astype(np.int32)


def count_keys(n: int) -> np.ndarray:
    """Slot keys (a << 32) | b of count_pairs with every fifth slot empty (int64 (n,))."""
    pr = count_pairs(n).astype(np.int64)
    keys = (pr[:, 0] << 32) | pr[:, 1]
    keys[np.arange(n) % 5 == 3] = -1
    return keys


# (name, n, rows given, p, kcap, gflags word or None)
MUT_COUNT_CASES = [(f"n{n}-{'rows' if rows else 'all'}-p{p}-cap{kcap}", n, rows, p, kcap, None)
                   for n in (1, 255, 256, 257, 5000) for rows in (False, True)
                   for p, kcap in ((0.1, 0), (0.1, 3), (5.0, 0))]
MUT_COUNT_CASES += [("n257-all-skipped", 257, False, 0.1, 0, GP_WIDTH), ("n257-rows-other-flag", 257, True, 0.1, 0, 4)]
# (name, n, p)
REC_COUNT_CASES = [("n1", 1, 1e-3), ("n257", 257, 1e-3), ("n3000", 3000, 4e-3), ("n256-dense", 256, 0.05)]
# (name, n, p, kcap, gflags word or None, longest or None)
REC_KEYS_CASES = [("n257-direct", 257, 1e-3, 0, None, None), ("n1000-direct-cap3", 1000, 4e-3, 3, None, None),
                  ("n257-thinned", 257, 1e-3, 0, None, 10_000), ("n1000-thinned-cap3", 1000, 4e-4, 3, None, 10_000),
                  ("n64-thinned-dense", 64, 0.05, 0, None, 10_000), ("n300-thinned-flag", 300, 1e-3, 0, 4, 10_000),
                  ("n257-skipped", 257, 1e-3, 0, GP_WIDTH, 10_000)]


@functools.lru_cache(maxsize=None)
def mut_count_case(name: str):
    _, n, rows, p, kcap, gflags = next(c for c in MUT_COUNT_CASES if c[0] == name)
    return mut_count(n, count_rows(n) if rows else None, count_lens(), p, COUNT_SEED, COUNT_CALL, kcap, gflags)


@functools.lru_cache(maxsize=None)
def rec_count_case(name: str):
    _, n, p = next(c for c in REC_COUNT_CASES if c[0] == name)
    return rec_count(n, count_pairs(n), count_lens(), p, COUNT_SEED, COUNT_CALL)


@functools.lru_cache(maxsize=None)
def rec_keys_case(name: str):
    _, n, p, kcap, gflags, longest = next(c for c in REC_KEYS_CASES if c[0] == name)
    return rec_count_keys(n, count_keys(n), count_lens(), p, COUNT_SEED, COUNT_CALL, kcap, gflags, longest)
