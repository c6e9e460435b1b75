"""The generic-alphabet engine (dbg_generic.h: packed keys, k <= 11; dbg_genref.h: tables keyed by reference into the
reads, 12 <= k <= 63; the GGen accessor of the shared prune / tips / pull-reads / walk kernels) where the rest of the
suite never runs it: every k in 1..63 on ragged reads, bytes >= 0x80, heavy repeats, table sizes at the capacity steps,
the ABI's [n][32] arrays compared directly, final mode and thresholds 1, 3, 5 above vector size, both walks, the
index-only walk, and dbg_take_reads.

The tables are compared with `table_reference` below: a numpy restatement of the definitions in include/dbg.h that
takes raw bytes and offsets.  It shares nothing with oracle/dbg_oracle.py (strings, dicts) or oracle/dbg_oracle.c, so
the three are separate witnesses; `test_table_reference_*` ties it to the C one on the CPU."""
import contextlib
import functools
import io
import time

import numpy as np
import pytest

import _dbg
from oracle import orc_c

gpu = pytest.mark.gpu

D = 32                       # successor slots per node of the generic layout (dbg_sizes_t.max_degree)
NONE = np.int64(1) << 62     # "no first occurrence" in the reference's first-seen arrays

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
AA20 = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
# 32 symbols: the most the 5-bit codes hold, with the bytes on both sides of the sign bit (0x7F / 0x80), the extremes
# 0x01 and 0xFF, and no byte 0
SYM32 = np.array([0x01, 0x7F, 0x80, 0xFF] + list(range(0x41, 0x41 + 14)) + list(range(0xC0, 0xC0 + 14)), dtype=np.uint8)
assert np.unique(SYM32).size == 32 and SYM32.min() > 0


# ---------------------------------------------------------------------------------------------------------------
# 1. the table reference
# ---------------------------------------------------------------------------------------------------------------
def window_ids(codes, n):
    """ids[p] for p in 0 .. len - n: equal exactly where the windows codes[p:p+n] are equal.  Windows of length 1, 2,
    4, ... are numbered by np.unique over (id of the left half, id of the right half) pairs and joined along the bits
    of n, so nothing of size len x n is ever held."""
    def join(a, la, b, lb):
        m = codes.size - (la + lb) + 1
        if m <= 0:
            return np.zeros(0, dtype=np.int64)
        pair = a[:m] * (int(b.max()) + 1) + b[la:la + m]   # both factors are below len(codes): no overflow
        return np.unique(pair, return_inverse=True)[1].astype(np.int64).reshape(-1)
    cur, cur_len = codes.astype(np.int64), 1
    out, out_len = None, 0
    while True:
        if n & cur_len:
            out = cur if out is None else join(out, out_len, cur, cur_len)
            out_len += cur_len
        if cur_len * 2 > n:
            return out
        cur, cur_len = join(cur, cur_len, cur, cur_len), cur_len * 2


def table_reference(bases, offsets, k):
    """include/dbg.h, literally.  -> dict:
    alphabet   the distinct bytes in byte order (code = rank: dbg_get_alphabet)
    kmers      uint8[n][k]: the distinct k-mers of the reads with len > k, in ascending stamp order
    stamps     (offset of the first occurrence << 1) | (that occurrence is not at position 0 of its read)
    counts     int64[n][32] per successor code; first[n][32]: offset of the first instance of that (k+1)-mer (NONE if none)
    succ       int64[n][32]: row of the successor k-mer (-1 if none)
    n_kmer_instances / n_edge_instances: N_k, N_e"""
    b = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
    off = np.asarray(offsets, dtype=np.int64)
    n = b.size
    alphabet = np.unique(b)
    codes = np.searchsorted(alphabet, b).astype(np.int64)
    pos = np.arange(n, dtype=np.int64)
    read = np.searchsorted(off, pos, side="right") - 1        # the (non-empty) read that holds byte p
    beg, end = off[read], off[read + 1]
    has_kmer = ((end - beg) > k) & (end - pos >= k)             # a k-mer window of a read with len > k starts at p
    has_edge = end - pos >= k + 1                               # ... and a (k+1)-mer window
    pk, pe = np.nonzero(has_kmer)[0], np.nonzero(has_edge)[0]
    out = {"alphabet": alphabet, "k": k, "n_kmer_instances": int(pk.size), "n_edge_instances": int(pe.size)}
    if pk.size == 0:
        out.update(kmers=np.zeros((0, k), np.uint8), stamps=np.zeros(0, np.uint64), counts=np.zeros((0, D), np.int64),
                   first=np.zeros((0, D), np.int64), succ=np.zeros((0, D), np.int64))
        return out
    ids = window_ids(codes, k)
    uniq, first_idx = np.unique(ids[pk], return_index=True)     # pk ascends: the first index is the first occurrence
    fp = pk[first_idx]
    rank = np.argsort(fp)                                        # ascending stamp == ascending first offset
    fp = fp[rank]
    row_of = np.full(int(ids.max()) + 1, -1, dtype=np.int64)
    row_of[uniq[rank]] = np.arange(fp.size)
    nn = fp.size
    counts = np.zeros((nn, D), dtype=np.int64)
    first = np.full((nn, D), NONE, dtype=np.int64)
    succ = np.full((nn, D), -1, dtype=np.int64)
    if pe.size:
        src, code, dst = row_of[ids[pe]], codes[pe + k], row_of[ids[pe + 1]]
        assert src.min() >= 0 and dst.min() >= 0
        np.add.at(counts, (src, code), 1)
        np.minimum.at(first, (src, code), pe)
        succ[src, code] = dst
    out.update(kmers=b[fp[:, None] + np.arange(k)[None, :]], stamps=((fp << 1) | (fp != beg[fp])).astype(np.uint64),
               counts=counts, first=first, succ=succ)
    return out


def table_reference_plain(bases, offsets, k):
    """The same by one Python loop over the reads and dicts of bytes (slow: small inputs only) -> (k-mer bytes in
    stamp order, stamps, {(k+1)-mer bytes: (count, first offset)}, N_k, N_e)."""
    b = bytes(np.asarray(bases, dtype=np.uint8))
    nodes, edges, n_k, n_e = {}, {}, 0, 0
    for r in range(len(offsets) - 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        if hi - lo <= k:
            continue
        for p in range(lo, hi - k + 1):
            nodes.setdefault(b[p:p + k], (p << 1) | (p != lo))
            n_k += 1
            if p + k < hi:
                c, f = edges.get(b[p:p + k + 1], (0, p))
                edges[b[p:p + k + 1]] = (c + 1, f)
                n_e += 1
    return list(nodes), list(nodes.values()), edges, n_k, n_e


def rank_bytes(counts, first):
    """dbg_export_orders of the generic layout: successor codes by (count descending, first seen) and by first seen
    alone, 0xFF beyond the out-degree."""
    deg = (counts != 0).sum(axis=1)
    beyond = np.arange(D)[None, :] >= deg[:, None]
    big = np.int64(1) << 21
    assert not counts.any() or (counts.max() < big and first[counts != 0].max() < (np.int64(1) << 41))
    mc_key = np.where(counts != 0, ((big - counts) << 41) + np.minimum(first, (np.int64(1) << 41) - 1), np.iinfo(np.int64).max)
    fs_key = np.where(counts != 0, first, np.iinfo(np.int64).max)
    mc = np.argsort(mc_key, axis=1, kind="stable").astype(np.uint8)
    fs = np.argsort(fs_key, axis=1, kind="stable").astype(np.uint8)
    mc[beyond] = 0xFF
    fs[beyond] = 0xFF
    return mc, fs


def pack(reads):
    """list of uint8 arrays -> (bases, offsets) as dbg_set_reads takes them"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([r.size for r in reads], out=off[1:])
    return (np.concatenate(reads) if reads else np.zeros(0, np.uint8)).astype(np.uint8), off


def build_graph(bases, offsets, k, g=None):
    g = g or _dbg.Graph()
    g.set_reads(bases, offsets)
    g.build(k)
    return g


def check_tables(g, ref, bases, offsets):
    """Everything dbg_build leaves behind on a generic alphabet against `table_reference`, array by array."""
    k, n = ref["k"], ref["stamps"].size
    sz = g.sizes()
    n_edges = int((ref["counts"] != 0).sum())
    assert (sz["k"], sz["n_reads"], sz["n_bytes"]) == (k, len(offsets) - 1, int(offsets[-1]))
    assert sz["n_nodes"] == n and sz["n_edges"] == n_edges
    assert sz["n_kmer_instances"] == ref["n_kmer_instances"] and sz["n_edge_instances"] == ref["n_edge_instances"]
    assert sz["max_degree"] == D
    assert g.alphabet() == (ref["alphabet"].tobytes(), 5)
    keys, stamps, counts, flags = g.export_nodes()
    assert counts.shape == (n, D)
    o = np.argsort(stamps, kind="stable")
    assert np.array_equal(stamps[o], ref["stamps"])
    assert np.array_equal(flags[o] & 1, (ref["stamps"] & np.uint64(1)).astype(np.uint8))
    assert np.array_equal(counts[o], ref["counts"])
    assert np.array_equal(g.export_dict_order(), o)
    # keys: 5 bits per character in one word up to k = 11, zeros above (the k-mer is the text at the stamp)
    kcodes = np.searchsorted(ref["alphabet"], ref["kmers"]).astype(np.uint64)
    if k <= 11:
        want = (kcodes << (np.uint64(5) * (k - 1 - np.arange(k)).astype(np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
        assert np.array_equal(keys[o], want)
    else:
        assert not keys.any()
        dev_bases, dev_off = g.copy_reads()
        assert np.array_equal(dev_off, np.asarray(offsets, dtype=np.uint64))
        at = (stamps[o] >> np.uint64(1)).astype(np.int64)
        assert np.array_equal(dev_bases[at[:, None] + np.arange(k)[None, :]], ref["kmers"])
    # succ: a value exactly where the count is nonzero; the successor's k-mer is the node's shifted by that byte
    succ = g.export_succ()
    has = counts != 0
    assert np.all(succ[~has] == _dbg.NO_NODE) and np.all(succ[has] < n)
    inv = np.empty(n, dtype=np.int64)
    inv[o] = np.arange(n)
    rows, code = np.nonzero(has)
    src, dst = ref["kmers"][inv[rows]], ref["kmers"][inv[succ[rows, code]]]
    assert np.array_equal(dst[:, :-1], src[:, 1:]) and np.array_equal(dst[:, -1], ref["alphabet"][code])
    assert np.array_equal(inv[succ[rows, code]], ref["succ"][inv[rows], code])
    # CSR: the nonzero entries in code order
    rp, col, cnt = g.export_csr()
    assert int(rp[0]) == 0 and np.array_equal(np.diff(rp.astype(np.int64)), has.sum(axis=1))
    assert np.array_equal(col, succ[has]) and np.array_equal(cnt, counts[has])
    # successor ranks
    mc, fs = g.export_orders()
    want_mc, want_fs = rank_bytes(ref["counts"], ref["first"])
    assert np.array_equal(mc[o], want_mc) and np.array_equal(fs[o], want_fs)
    return o


def against_c_oracle(ref, want, alphabet_2bit=b"ACTG"):
    """`table_reference` of reads over ACGT == orc_c.build (2-bit codes A=0, C=1, T=2, G=3)."""
    k = ref["k"]
    assert ref["n_kmer_instances"] == want["n_kmer_instances"] and ref["n_edge_instances"] == want["n_edge_instances"]
    assert ref["stamps"].size == want["n_nodes"] and np.array_equal(ref["stamps"], want["stamps"])
    lut = np.zeros(256, dtype=np.int64)
    lut[np.frombuffer(alphabet_2bit, dtype=np.uint8)] = np.arange(4)
    c2 = lut[ref["kmers"]]
    v = [0] * ref["stamps"].size
    for i in range(k):                                     # 2k-bit numbers: Python ints
        col = c2[:, i].tolist()
        v = [(a << 2) | c for a, c in zip(v, col)]
    assert [x & orc_c.M64 for x in v] == want["keys"].tolist() and [x >> 64 for x in v] == want["keys_hi"].tolist()
    cols = np.searchsorted(ref["alphabet"], np.frombuffer(alphabet_2bit, dtype=np.uint8))   # 2-bit code -> reference code
    present = np.isin(np.frombuffer(alphabet_2bit, dtype=np.uint8), ref["alphabet"])
    counts4 = np.zeros((ref["stamps"].size, 4), dtype=np.int64)
    counts4[:, present] = ref["counts"][:, cols[present]]
    assert np.array_equal(counts4, want["counts"])
    assert int(ref["counts"].sum()) == int(counts4.sum())  # nothing outside the four columns


def ragged_reads(alphabet, k, seed, n_reads=1500, genome_len=9000, noise=None):
    """The recipe of test_every_window_width_both_extraction_kernels: reads of 0..159 symbols cut from one random
    sequence (k-mers repeat), every fifth of length 0, k - 1, k, k + 1 or 3k, every third with one substitution;
    `noise` (byte, rate): that byte replaces symbols of the genome at that rate."""
    rng = np.random.default_rng(seed)
    genome = alphabet[rng.integers(0, alphabet.size, size=genome_len)]
    if noise:
        genome[rng.random(genome_len) < noise[1]] = noise[0]
    reads = []
    for i in range(n_reads):
        L = int(rng.integers(0, 160)) if i % 5 else int(rng.choice([0, k - 1, k, k + 1, 3 * k]))
        s = int(rng.integers(0, genome_len - 200))
        r = genome[s:s + L].copy()
        if L > 3 and i % 3 == 0:
            r[int(rng.integers(0, L))] = alphabet[int(rng.integers(0, alphabet.size))]
        reads.append(r)
    return reads


ALPHABETS = {"acgtn": (ACGT, (ord("N"), 0.01)), "aa20": (AA20, None), "sym32": (SYM32, None)}


def test_table_reference_equals_plain_loop_and_c_oracle():
    """No GPU: the vectorised reference against the dict loop (three alphabets) and against orc_c.build (ACGT), on the
    reads of the per-k rows at a size the loop can take, for k on every side of a word or key-layout border."""
    for k in (1, 2, 3, 7, 11, 12, 16, 31, 32, 33, 47, 63):
        for name, (alphabet, noise) in ALPHABETS.items():
            bases, off = pack(ragged_reads(alphabet, k, 7 * k + len(name), n_reads=300, genome_len=1500, noise=noise))
            ref = table_reference(bases, off, k)
            kmers, stamps, edges, n_k, n_e = table_reference_plain(bases, off, k)
            assert (ref["n_kmer_instances"], ref["n_edge_instances"]) == (n_k, n_e)
            assert [bytes(r) for r in ref["kmers"]] == kmers and ref["stamps"].tolist() == stamps
            rows, code = np.nonzero(ref["counts"])
            got = {bytes(ref["kmers"][r]) + bytes([ref["alphabet"][c]]): (int(ref["counts"][r, c]), int(ref["first"][r, c]))
                   for r, c in zip(rows.tolist(), code.tolist())}
            assert got == edges and np.all(ref["first"][ref["counts"] == 0] == NONE)
            assert np.array_equal(ref["succ"] >= 0, ref["counts"] != 0)
        bases, off = pack(ragged_reads(ACGT, k, 11 * k, n_reads=600, genome_len=3000))
        against_c_oracle(table_reference(bases, off, k), orc_c.build(bases, off, k))


@pytest.mark.parametrize("k", [5, 21, 40, 63])
def test_table_reference_equals_c_oracle_at_row_size(k):
    """No GPU: the reference at the size of the per-k rows (1500 reads, 120 kB) against orc_c.build."""
    bases, off = pack(ragged_reads(ACGT, k, 300 + k))
    against_c_oracle(table_reference(bases, off, k), orc_c.build(bases, off, k))


# ---------------------------------------------------------------------------------------------------------------
# 2. every k, three alphabets, ragged reads
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", list(range(1, 64)))
@pytest.mark.parametrize("name", ["aa20", "sym32"])
def test_every_k_tables(name, k):
    """About 120 kB behind a start bitmap of thousands of words: read borders at every shift of the 64-bit window
    of gr_startwin64, reads of length 0, k - 1, k, k + 1, k-mers that repeat; sym32 feeds bytes >= 0x80."""
    alphabet, noise = ALPHABETS[name]
    bases, off = pack(ragged_reads(alphabet, k, 1000 + 64 * len(name) + k, noise=noise))
    g = build_graph(bases, off, k)
    check_tables(g, table_reference(bases, off, k), bases, off)
    g.close()


@gpu
@pytest.mark.parametrize("k", list(range(1, 64)))
def test_every_k_tables_acgtn_and_two_bit_path(k):
    """ACGT with about 1 % N through the generic engine; then the reads without an N three ways: the 2-bit engines,
    the generic engine (the same reads followed by the one-symbol read "N": it is no longer than any k, adds no k-mer
    and moves no stamp, but takes the build off the 2-bit path), and orc_c.build -- one graph."""
    alphabet, noise = ALPHABETS["acgtn"]
    reads = ragged_reads(alphabet, k, 5000 + k, noise=noise)
    bases, off = pack(reads)
    assert (bases == ord("N")).any()
    g = build_graph(bases, off, k)
    check_tables(g, table_reference(bases, off, k), bases, off)
    g.close()

    clean = [r for r in reads if not (r == ord("N")).any()]
    assert len(clean) > len(reads) // 3
    cb, coff = pack(clean)
    want = orc_c.build(cb, coff, k)
    g2 = build_graph(cb, coff, k)                                 # 2-bit path
    assert g2.sizes()["max_degree"] == 4
    keys, stamps, counts, flags = g2.export_nodes()
    o = np.argsort(stamps, kind="stable")
    assert g2.sizes()["n_kmer_instances"] == want["n_kmer_instances"] and g2.sizes()["n_edge_instances"] == want["n_edge_instances"]
    assert np.array_equal(keys[o], want["keys"]) and np.array_equal(g2.export_keys_hi()[o], want["keys_hi"])
    assert np.array_equal(stamps[o], want["stamps"]) and np.array_equal(counts[o], want["counts"])
    g2.close()
    gb, goff = pack(clean + [np.frombuffer(b"N", dtype=np.uint8)])
    ref = table_reference(gb, goff, k)
    against_c_oracle(ref, want)
    g3 = build_graph(gb, goff, k)                                 # generic path, same graph
    check_tables(g3, ref, gb, goff)
    g3.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. contention and degenerate structure
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [5, 11, 12, 31])
def test_first_occurrence_under_contention(k):
    """gr_insert / k_g_insert keep the first occurrence of a k-mer by racing atomicMin's on one slot: 20 000 copies of
    one 40-symbol peptide, 5 000 homopolymer reads (a self-loop: the node is its own successor), 3 000 copies of a
    period-2 read and 2 000 ordinary reads, shuffled.  The homopolymer reads are 160 - 3k symbols long, the shortest
    whose one edge is seen 5 000 x (160 - 4k) = 20 000 x (40 - k) times, the load the largest count is held to."""
    rng = np.random.default_rng(40 + k)
    while True:                                                    # its 5-mers (so its k-mers) are distinct: each edge
        peptide = AA20[rng.integers(0, 20, size=40)]               # of the peptide is seen exactly 20 000 times there
        if np.unique(window_ids(np.searchsorted(AA20, peptide), 5)).size == 36:
            break
    homo = np.full(160 - 3 * k, ord("W"), dtype=np.uint8)
    period2 = np.tile(np.frombuffer(b"KR", dtype=np.uint8), 20)
    reads = [peptide] * 20000 + [homo] * 5000 + [period2] * 3000 + ragged_reads(AA20, k, 900 + k, n_reads=2000)
    reads = [reads[i] for i in rng.permutation(len(reads)).tolist()]
    bases, off = pack(reads)
    ref = table_reference(bases, off, k)
    g = build_graph(bases, off, k)
    o = check_tables(g, ref, bases, off)
    counts = g.export_nodes(keys=False, stamps=False, flags=False)[2][o]
    assert int(counts.max()) >= 20000 * (40 - k)
    w = int(np.searchsorted(ref["alphabet"], ord("W")))
    loop = int(np.nonzero((ref["kmers"] == ord("W")).all(axis=1))[0][0])
    assert int(counts[loop, w]) >= 5000 * (160 - 4 * k) and inv_succ(g, o)[loop, w] == loop     # the self-loop
    pep_rows = [int(np.nonzero((ref["kmers"] == peptide[i:i + k]).all(axis=1))[0][0]) for i in range(40 - k)]
    pep_cnt = counts[pep_rows, np.searchsorted(ref["alphabet"], peptide[k:])]
    assert int(pep_cnt.min()) >= 20000
    g.close()


def inv_succ(g, o):
    """successor rows in stamp order (-1: none)"""
    succ = g.export_succ()[o].astype(np.int64)
    inv = np.empty(o.size, dtype=np.int64)
    inv[o] = np.arange(o.size)
    return np.where(succ == _dbg.NO_NODE, -1, inv[np.minimum(succ, o.size - 1)])


# ---------------------------------------------------------------------------------------------------------------
# 4. table sizing and alphabet limits
# ---------------------------------------------------------------------------------------------------------------
def all_distinct_sequence(rng, n, width=3):
    """n symbols over SYM32 whose windows of `width` are all different (so are all longer ones)."""
    seq, seen = [int(x) for x in rng.integers(0, 32, size=width - 1)], set()
    while len(seq) < n:
        c = int(rng.integers(0, 32))
        w = tuple(seq[len(seq) - width + 1:]) + (c,)
        if w not in seen:
            seen.add(w)
            seq.append(c)
    return SYM32[np.array(seq)]


@gpu
@pytest.mark.parametrize("k", [3, 12])
@pytest.mark.parametrize("n_bytes", [511, 512, 1023, 1024])
def test_table_capacity_steps_with_every_window_distinct(n_bytes, k):
    """The tables hold the power of two >= 2 * (n_bytes + 1) slots (1024 at least): 511 bytes are the most 1024 slots
    take, 512 and 1023 go to 2048, 1024 to 4096.  Three reads with no repeated window fill them as far as they go."""
    rng = np.random.default_rng(n_bytes + k)
    seq = all_distinct_sequence(rng, n_bytes)
    cuts = (n_bytes // 3, 2 * n_bytes // 3 + 1)
    bases, off = pack([seq[:cuts[0]], seq[cuts[0]:cuts[1]], seq[cuts[1]:]])
    assert bases.size == n_bytes
    ref = table_reference(bases, off, k)
    assert ref["stamps"].size == ref["n_kmer_instances"] == n_bytes - 3 * (k - 1)      # every window its own node
    g = build_graph(bases, off, k)
    check_tables(g, ref, bases, off)
    g.close()


@gpu
@pytest.mark.parametrize("k", [11, 12, 63])
def test_32_symbols_build_and_33_do_not(k):
    rng = np.random.default_rng(k)
    reads = [SYM32[rng.permutation(32)]] + [SYM32[rng.integers(0, 32, size=100)] for _ in range(40)]
    bases, off = pack(reads)
    g = build_graph(bases, off, k)
    check_tables(g, table_reference(bases, off, k), bases, off)
    assert g.alphabet()[0] == np.sort(SYM32).tobytes()
    bases33, off33 = pack(reads + [np.full(70, 0x30, dtype=np.uint8)])
    g.set_reads(bases33, off33)
    with pytest.raises(_dbg.AlphabetError) as e:
        g.build(k)
    assert e.value.code == _dbg.DBG_E_ALPHABET
    g.set_reads(bases, off)                                       # the handle is still good
    g.build(k)
    check_tables(g, table_reference(bases, off, k), bases, off)
    g.close()


@gpu
def test_k_64_fails_on_a_generic_alphabet():
    rng = np.random.default_rng(64)
    bases, off = pack([AA20[rng.integers(0, 20, size=150)] for _ in range(20)])
    g = _dbg.Graph()
    g.set_reads(bases, off)
    with pytest.raises(_dbg.DbgError) as e:
        g.build(64)
    assert e.value.code in (_dbg.DBG_E_ARG, _dbg.DBG_E_ALPHABET)
    g.build(63)
    check_tables(g, table_reference(bases, off, 63), bases, off)
    g.close()


def stage_arrays(g):
    """what a build left on the handle, in stamp order, successors as stamp-order rows"""
    keys, stamps, counts, flags = g.export_nodes()
    o = np.argsort(stamps, kind="stable")
    sz = g.sizes()
    g.refine_edge_order()          # the 2-bit path ranks its successors here; the generic engine already has
    mc, fs = g.export_orders()
    out = {"sizes": {f: sz[f] for f in ("k", "n_reads", "n_bytes", "n_kmer_instances", "n_edge_instances", "n_nodes",
                                        "n_edges", "max_degree", "n_starts")},
           "alphabet": g.alphabet(), "keys": keys[o], "keys_hi": g.export_keys_hi()[o], "stamps": stamps[o],
           "counts": counts[o], "flags": flags[o], "succ": inv_succ(g, o), "mc": mc[o], "fs": fs[o]}
    rp, col, cnt = g.export_csr()
    out["deg"] = np.diff(rp.astype(np.int64))[o]
    out["cnt_sum"] = int(cnt.sum())
    return out


def assert_same_stage(a, b):
    assert a.keys() == b.keys()
    for f in a:
        same = np.array_equal(a[f], b[f]) if isinstance(a[f], np.ndarray) else a[f] == b[f]
        assert same, f


@gpu
def test_one_handle_across_alphabets_and_key_layouts():
    """DNA at k = 21, peptides at k = 12 (no packed keys) and k = 8 (packed keys again), DNA at k = 21 again, all on one
    handle: every stage is what a fresh handle gives, and the peptide stages are what the table reference gives."""
    import synth
    dna = synth.reads_ascii(12, 8000, 600, 100, 0.01)
    dna_b, dna_off = dna.reshape(-1), np.arange(0, dna.size + 1, 100, dtype=np.uint64)
    pep_b, pep_off = pack(ragged_reads(AA20, 12, 77, n_reads=800, genome_len=4000))
    g = _dbg.Graph()
    want_dna = orc_c.build(dna_b, dna_off, 21)
    for bases, off, ks in ((dna_b, dna_off, (21,)), (pep_b, pep_off, (12, 8)), (dna_b, dna_off, (21,))):
        g.set_reads(bases, off)
        for k in ks:
            g.build(k)
            got = stage_arrays(g)
            fresh = build_graph(bases, off, k)
            assert_same_stage(got, stage_arrays(fresh))
            fresh.close()
            if bases is pep_b:
                check_tables(g, table_reference(bases, off, k), bases, off)
                assert bool(got["keys"].any()) == (k <= 11)
            else:
                assert got["sizes"]["max_degree"] == 4
                assert np.array_equal(got["keys"], want_dna["keys"]) and np.array_equal(got["stamps"], want_dna["stamps"])
                assert np.array_equal(got["counts"], want_dna["counts"])
    g.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. dbg_take_reads
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_take_reads_equals_numpy_gather():
    rng = np.random.default_rng(6)
    reads = ragged_reads(SYM32, 9, 66, n_reads=700, genome_len=3000)
    reads[0] = reads[0][:0]                                        # empty reads at both ends and in the middle
    reads[-1] = reads[-1][:0]
    bases, off = pack(reads)
    lens = np.diff(off.astype(np.int64))
    empty = np.nonzero(lens == 0)[0]
    assert empty.size >= 10 and lens.max() > 64
    g = _dbg.Graph()
    g.set_reads(bases, off)
    n = len(reads)
    takes = {"none": np.zeros(0, np.int64), "all": np.arange(n), "reversed": np.arange(n)[::-1],
             "repeats": rng.integers(0, n, size=2 * n), "one_empty": empty[3:4], "first_last_empty": np.array([0, n - 1]),
             "same_read_many_times": np.full(300, int(np.argmax(lens)))}

    def check(idx):
        chars, o = g.take_reads(idx)
        want_off = np.zeros(idx.size + 1, dtype=np.uint64)
        np.cumsum(lens[idx], out=want_off[1:])
        assert np.array_equal(o, want_off)
        want = np.concatenate([reads[i] for i in idx.tolist()]) if idx.size else np.zeros(0, np.uint8)
        assert np.array_equal(chars, want)

    for name, idx in takes.items():
        check(np.asarray(idx, dtype=np.int64))
    for bad in ([n], [0, 5, n + 7, 2], [2 ** 40]):
        with pytest.raises(_dbg.DbgError) as e:
            g.take_reads(np.array(bad, dtype=np.uint64))
        assert e.value.code == _dbg.DBG_E_ARG and not isinstance(e.value, _dbg.AlphabetError)
        check(np.asarray(takes["repeats"], dtype=np.int64))       # the handle stays usable
    g.build(9)                                                     # ... and builds what it would have built
    check_tables(g, table_reference(bases, off, 9), bases, off)
    check(np.asarray(takes["reversed"], dtype=np.int64))
    g.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the whole path in the modes never run above vector size
# ---------------------------------------------------------------------------------------------------------------
def traversal_reads(name, seed, genome_len, err, n_reads):
    """Ragged reads of 0..160 symbols cut from one random sequence, `err` substitutions per symbol; "acgtn": ACGT
    with 1 % N in the sequence, "aa20": the 20 amino acids."""
    rng = np.random.default_rng(seed)
    alphabet = ACGT if name == "acgtn" else AA20
    genome = alphabet[rng.integers(0, alphabet.size, size=genome_len)]
    if name == "acgtn":
        genome[rng.random(genome_len) < 0.01] = ord("N")
    lens = rng.integers(0, 161, size=n_reads)
    starts = (rng.random(n_reads) * (genome_len - lens + 1)).astype(np.int64)
    out = []
    for s, L in zip(starts.tolist(), lens.tolist()):
        r = genome[s:s + L].copy()
        flip = rng.random(L) < err
        r[flip] = alphabet[rng.integers(0, alphabet.size, size=int(flip.sum()))]
        out.append(r.tobytes().decode("latin-1"))
    return out


# (alphabet, k, threshold, final) -> (sequence length, substitution rate, reads).  Chosen on the CPU from the oracle
# alone so that every row has at least 20 branch k-mers, 10 pulled nodes, (non-final) 10 pull-out reads and a contig,
# and so that the final-mode DFS -- which enumerates every path: it doubles at every bubble a start can reach -- ends
# within seconds: 5-10x coverage or 3-8 % substitutions for the branches, and for final mode below k = 41 a sequence
# of 1000-3000 symbols under fewer reads, so that a path has few bubbles ahead of it.  No (k, alphabet) pair had to
# give up its (2, True) row for a second (1, True) one.  Never more than the 3000 reads / 240 kB of the k-series.
TRAVERSAL_ROWS = {
    ("acgtn", 8, 1, False): (6000, 0.01, 3000), ("acgtn", 8, 3, False): (6000, 0.01, 3000),
    ("acgtn", 8, 5, False): (6000, 0.01, 3000), ("acgtn", 8, 1, True): (1500, 0.05, 750),
    ("acgtn", 8, 2, True): (1000, 0.05, 500),
    ("acgtn", 11, 1, False): (48000, 0.05, 3000), ("acgtn", 11, 3, False): (24000, 0.01, 3000),
    ("acgtn", 11, 5, False): (24000, 0.01, 3000), ("acgtn", 11, 1, True): (1000, 0.05, 500),
    ("acgtn", 11, 2, True): (1500, 0.05, 750),
    ("acgtn", 12, 1, False): (48000, 0.03, 3000), ("acgtn", 12, 3, False): (24000, 0.03, 3000),
    ("acgtn", 12, 5, False): (24000, 0.01, 3000), ("acgtn", 12, 1, True): (1500, 0.05, 750),
    ("acgtn", 12, 2, True): (1500, 0.05, 750),
    ("acgtn", 21, 1, False): (48000, 0.03, 3000), ("acgtn", 21, 3, False): (48000, 0.05, 3000),
    ("acgtn", 21, 5, False): (24000, 0.01, 3000), ("acgtn", 21, 1, True): (2000, 0.05, 1000),
    ("acgtn", 21, 2, True): (1500, 0.05, 750),
    ("acgtn", 41, 1, False): (48000, 0.03, 3000), ("acgtn", 41, 3, False): (24000, 0.01, 3000),
    ("acgtn", 41, 5, False): (24000, 0.01, 3000), ("acgtn", 41, 1, True): (48000, 0.03, 3000),
    ("acgtn", 41, 2, True): (48000, 0.05, 3000),
    ("acgtn", 63, 1, False): (24000, 0.01, 3000), ("acgtn", 63, 3, False): (6000, 0.03, 3000),
    ("acgtn", 63, 5, False): (24000, 0.01, 3000), ("acgtn", 63, 1, True): (48000, 0.03, 3000),
    ("acgtn", 63, 2, True): (24000, 0.05, 3000),
    ("aa20", 8, 1, False): (48000, 0.03, 3000), ("aa20", 8, 3, False): (48000, 0.03, 3000),
    ("aa20", 8, 5, False): (24000, 0.01, 3000), ("aa20", 8, 1, True): (2000, 0.08, 1000),
    ("aa20", 8, 2, True): (1500, 0.08, 750),
    ("aa20", 11, 1, False): (48000, 0.05, 3000), ("aa20", 11, 3, False): (48000, 0.05, 3000),
    ("aa20", 11, 5, False): (24000, 0.01, 3000), ("aa20", 11, 1, True): (1500, 0.08, 750),
    ("aa20", 11, 2, True): (1500, 0.05, 750),
    ("aa20", 12, 1, False): (48000, 0.05, 3000), ("aa20", 12, 3, False): (24000, 0.05, 3000),
    ("aa20", 12, 5, False): (24000, 0.01, 3000), ("aa20", 12, 1, True): (1000, 0.08, 500),
    ("aa20", 12, 2, True): (2000, 0.05, 1000),
    ("aa20", 21, 1, False): (48000, 0.05, 3000), ("aa20", 21, 3, False): (24000, 0.03, 3000),
    ("aa20", 21, 5, False): (24000, 0.01, 3000), ("aa20", 21, 1, True): (2000, 0.05, 500),
    ("aa20", 21, 2, True): (3000, 0.03, 1500),
    ("aa20", 41, 1, False): (24000, 0.01, 3000), ("aa20", 41, 3, False): (24000, 0.01, 3000),
    ("aa20", 41, 5, False): (24000, 0.01, 3000), ("aa20", 41, 1, True): (48000, 0.03, 3000),
    ("aa20", 41, 2, True): (24000, 0.05, 3000),
    ("aa20", 63, 1, False): (24000, 0.01, 3000), ("aa20", 63, 3, False): (24000, 0.01, 3000),
    ("aa20", 63, 5, False): (24000, 0.01, 3000), ("aa20", 63, 1, True): (24000, 0.01, 3000),
    ("aa20", 63, 2, True): (6000, 0.05, 3000),
}
assert len(TRAVERSAL_ROWS) == 2 * 6 * 5


@functools.lru_cache(maxsize=None)
def oracle_row(name, k, thr, final):
    """The Python oracle's canonical result of one row (+ stdout, scores, seconds), computed once."""
    from golden_util import canonical
    from oracle import dbg_oracle as orc
    genome_len, err, n_reads = TRAVERSAL_ROWS[(name, k, thr, final)]
    reads = traversal_reads(name, 1000 * k + thr + 7 * final, genome_len, err, n_reads)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        g, pull, branch, pulled, ect = orc.construct_graph(list(reads), k, threshold=thr, final=final)
        contigs = orc.output_contigs(g, branch, pulled)
    secs = time.perf_counter() - t0
    r = canonical(g, pull, branch, pulled, ect, contigs)
    r["stdout"] = buf.getvalue()
    r["scores"] = [orc.get_score(ect, c, k) for c in contigs]
    return reads, r, secs


def device_row(reads, k, thr, final):
    import debruijn as prod
    from golden_util import canonical
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        g, pull, branch, pulled, ect = prod.construct_graph(list(reads), k, threshold=thr, final=final)
        contigs = prod.output_contigs(g, branch, pulled)
    r = canonical(g, pull, branch, pulled, ect, contigs)
    r["stdout"] = buf.getvalue()
    r["scores"] = list(contigs.scores)
    return r, (g, branch, pulled, contigs)


@gpu
@pytest.mark.parametrize("name,k,thr,final", list(TRAVERSAL_ROWS), ids=lambda x: str(x))
def test_traversal_modes_equal_python_oracle(name, k, thr, final):
    """construct_graph + output_contigs against oracle/dbg_oracle.py: vertices, edges, pull-out reads, branch list, pulled
    nodes, edge counts, contigs, stdout and scores, at thresholds 1, 3, 5 and in final mode, on both key layouts.

    The oracle alone on the CPU, per row: branch k-mers / pulled nodes / pull-out reads / oracle seconds
    alph.  k            (1, False)            (3, False)            (5, False)             (1, True)             (2, True)
    acgtn  8       548/62/1145/1.0       768/70/2580/0.9       835/74/2580/0.9          602/76/-/0.4          346/43/-/0.4
    acgtn 11     1368/321/1540/1.2        117/14/616/0.9       379/36/1424/0.8          108/31/-/0.3          169/21/-/0.4
    acgtn 12        525/98/801/1.5        492/57/981/1.1       328/38/1006/0.6          145/28/-/0.6          145/26/-/0.6
    acgtn 21       603/172/898/1.6     2165/446/2086/1.6       447/54/1157/0.8          137/47/-/0.9          104/25/-/0.8
    acgtn 41       429/109/728/1.2        291/55/732/0.9      585/123/1337/0.6         414/173/-/1.5         472/154/-/1.4
    acgtn 63        102/37/200/0.7        265/81/498/1.0        350/99/821/1.2          143/47/-/0.8           87/20/-/1.1
    aa20   8       498/124/691/1.9     2300/375/2124/1.4        325/40/881/0.8          139/21/-/1.6          101/16/-/0.6
    aa20  11     1165/337/1374/1.9     3795/651/2463/1.6        371/65/955/0.9           96/28/-/0.8           43/23/-/1.0
    aa20  12     1237/279/1431/1.3     1680/307/1823/1.1       414/65/1043/0.8           75/28/-/1.1           54/24/-/0.8
    aa20  21     1119/308/1418/1.4     1162/178/1536/1.1      591/104/1362/0.7           28/15/-/0.6           31/20/-/1.0
    aa20  41         86/29/169/1.1        390/54/882/0.6      631/140/1374/0.8         408/162/-/1.4          401/91/-/1.3
    aa20  63        115/40/220/0.6        369/95/778/0.5        381/88/842/0.7          121/56/-/0.6           93/47/-/0.9
    (contigs: 163 .. 3655 per row, 5 k .. 2.5 M contig characters; the slowest oracle run took 1.9 s)"""
    reads, o, secs = oracle_row(name, k, thr, final)
    n_branch = int(o["stdout"].split("branch number: ")[1].split()[0])
    print(f"\n[{name} k={k} threshold={thr} final={final}] nodes {len(o['vertices'])} branch {n_branch} "
          f"pulled {len(o['already_pull_out'])} pull_reads {len(o['pull_out_read'])} contigs {len(o['contigs'])} "
          f"contig_chars {sum(map(len, o['contigs']))} oracle {secs:.1f}s")
    # the reference's own result: a row that would pass with the tip removal or the pull-out reads broken is no row
    assert n_branch >= 20 and len(o["already_pull_out"]) >= 10 and len(o["contigs"]) >= 1
    if final:
        assert secs < 10.0 and o["branch_kmer"] == [] and o["pull_out_read"] == []
    else:
        assert len(o["branch_kmer"]) == n_branch and len(o["pull_out_read"]) >= 10
    d, _ = device_row(reads, k, thr, final)
    for field in o:
        assert d[field] == o[field], field


@gpu
@pytest.mark.parametrize("k", [11, 12])
def test_both_walks_index_only_walk_and_sorted_fasta(k):
    """Peptides on both sides of the key switch (GGen with packed keys / with keys == nullptr), non-final: the
    node-by-node walk and the pointer-jumping walk against the oracle's contigs and scores, the walk that keeps the
    index only (text fetched per contig), and the device's sorted FASTA."""
    import debruijn as prod
    thr = 3
    reads, o, _ = oracle_row("aa20", k, thr, False)
    with contextlib.redirect_stdout(io.StringIO()):
        g, pull, branch, pulled, ect = prod.construct_graph(list(reads), k, threshold=thr, final=False)
        gh = g[0]._graph
        assert (gh.export_nodes(stamps=False, counts=False, flags=False)[0].any()) == (k <= 11)
        walks = {}
        for mode, jump_min in (("jump", 0), ("node_by_node", 2 ** 31)):
            gh.set_option("walk_jump_min_nodes", jump_min)
            contigs = prod.output_contigs(g, branch, pulled)
            assert gh.sizes()["contigs_materialised"] == 1
            assert list(contigs) == o["contigs"] and list(contigs.scores) == o["scores"], mode
            off, score, stamp, seq = gh.export_contig_index()
            order = np.lexsort((seq, stamp))
            walks[mode] = (np.diff(off.astype(np.int64))[order], score[order], stamp[order], seq[order])
            # the driver's sort: by score, descending, stable
            by_score = sorted(range(len(contigs)), key=lambda i: -o["scores"][i])
            want = "".join(">SEQUENCE_{}_{}mer\n{}\n".format(i, k, o["contigs"][j]) for i, j in enumerate(by_score))
            assert contigs.sorted_fasta() == want, mode
        for a, b in zip(walks["jump"], walks["node_by_node"]):
            assert np.array_equal(a, b)
        # index only: max_chars too small for the text
        gh.set_option("walk_jump_min_nodes", 0)
        gh.walk(False, 0)
        m_off, m_chars, m_score, m_stamp, m_seq = gh.export_contigs()
        gh.walk(False, 16)
        sz = gh.sizes()
        assert sz["contigs_materialised"] == 0 and sz["n_contigs"] == len(o["contigs"]) and sz["contig_chars"] == m_chars.size
        off, score, stamp, seq = gh.export_contig_index()
        for a, b in ((off, m_off), (score, m_score), (stamp, m_stamp), (seq, m_seq)):
            assert np.array_equal(a, b)
        with pytest.raises(_dbg.DbgError):
            gh.export_contigs()                                    # there is no text to export
        text = m_chars.tobytes()
        for i in range(off.size - 1):
            lo, hi = int(off[i]), int(off[i + 1])
            assert gh.export_contig_text(i, hi - lo) == text[lo:hi], i
        order = np.lexsort((seq, stamp))
        assert [text[int(off[i]):int(off[i + 1])].decode("latin-1") for i in order] == o["contigs"]
    gh.close()


# Two 12-mers and two 13-mers over the amino acids that differ in their last byte only and agree in everything the
# by-reference tables look at before they compare bytes: the 16-bit fingerprint and the home slot of a 1024-slot table
# (found by a search over 8 million random windows with the hash of gr_hash: FNV-1a over the bytes, then mix64).  Among
# the 54 000 pairs of k-mers and (k+1)-mers of the per-k rows that differ in the last byte only, one shares its
# fingerprint and none its slot as well, so gr_bytes_eq could drop its last byte there unnoticed.
COLLIDING_12MERS = (b"CCVFLLSDDPSF", b"CCVFLLSDDPSR")
COLLIDING_13MERS = (b"RNTATTYVTPHMC", b"RNTATTYVTPHMY")


def colliding_reads():
    rng = np.random.default_rng(12)
    fill = lambda: AA20[rng.integers(0, 20, size=25)]  # noqa: E731
    reads = [np.concatenate([fill(), np.frombuffer(w, dtype=np.uint8), fill()])
             for w in COLLIDING_12MERS + COLLIDING_13MERS for _ in range(2)]
    return pack(reads)


@gpu
def test_equal_fingerprint_and_slot_are_told_apart_by_the_bytes():
    """k = 12, 500 bytes, 1024 slots: the node table meets the colliding 12-mers, the edge table the colliding
    13-mers (one node, two successors), each twice.  Only the comparison of all k (k + 1) bytes keeps them apart."""
    bases, off = colliding_reads()
    assert bases.size <= 511                                      # 1024 slots: the slot the vectors collide in
    ref = table_reference(bases, off, 12)
    kmers = [bytes(r) for r in ref["kmers"]]
    assert len({kmers.index(w) for w in COLLIDING_12MERS}) == 2    # two nodes
    src = kmers.index(COLLIDING_13MERS[0][:12])
    assert (ref["counts"][src] == 2).sum() == 2                   # one node, successors C and Y, twice each
    g = build_graph(bases, off, 12)
    check_tables(g, ref, bases, off)
    g.close()
