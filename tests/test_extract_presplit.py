"""Option "extract_presplit": dbg_build's extraction writes its records pre-split by the top f0 bits of the bucket hash and
hands level 1 of the multisplit its count matrix.  The graph must not depend on f0: every comparison here is independent
of the order in which the table holds its nodes (nodes sorted by k-mer, successors as the successor's stamp)."""
import numpy as np
import pytest

import _dbg
import synth
from oracle import orc_c

pytestmark = pytest.mark.gpu

READ_LEN = 100
SEED = 5


def graph_of(g):
    """(keys, stamps, counts, successor stamps) by ascending k-mer, sizes() and the record count of the last build."""
    keys, stamps, counts, _ = g.export_nodes()
    succ = g.export_succ()
    o = np.argsort(keys, kind="stable")
    present = succ != np.uint32(0xFFFFFFFF)
    succ_stamps = np.where(present, stamps[np.where(present, succ, 0)].astype(np.int64), np.int64(-1))
    return {"keys": keys[o], "stamps": stamps[o], "counts": counts[o], "succ_stamps": succ_stamps[o], "sizes": g.sizes(),
            "n_records": g.stats()["n_records"]}


def assert_same_graph(a, b):
    assert a["sizes"] == b["sizes"]
    assert a["n_records"] == b["n_records"]
    for f in ("keys", "stamps", "counts", "succ_stamps"):
        assert np.array_equal(a[f], b[f]), f


def node_digest(gr):
    """bench.py's node_digest_gpu (= oracle/orc_c.digest), restated: sum over the nodes of
    mix(key ^ mix(stamp) ^ mix(c0 + 3 c1 + 5 c2 + 7 c3 + 1)) modulo 2^64, mix = the 64-bit murmur3 finaliser."""
    def mix(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
        return x
    with np.errstate(over="ignore"):
        c = gr["counts"].astype(np.uint64)
        w = c[:, 0] + np.uint64(3) * c[:, 1] + np.uint64(5) * c[:, 2] + np.uint64(7) * c[:, 3] + np.uint64(1)
        return int(mix(gr["keys"] ^ mix(gr["stamps"]) ^ mix(w)).sum(dtype=np.uint64))


def assert_equals_oracle(gr, bases, offsets, k):
    mt = orc_c.build_mt(bases, offsets, k, 4)
    sz = gr["sizes"]
    for f in ("n_nodes", "n_edges", "n_kmer_instances", "n_edge_instances"):
        assert sz[f] == mt[f], f
    assert node_digest(gr) == mt["digest"]


def build(bases, offsets, k, f0=None, stamp64=False):
    g = _dbg.Graph()
    try:
        g.set_reads(bases, offsets)
        if stamp64:
            g.set_option("stamp64", 1)
        if f0 is not None:
            g.set_option("extract_presplit", f0)
        g.build(k)
        gr = graph_of(g)
        gr["n_buckets"] = g.stats()["n_buckets"]
        gr["fallbacks"] = g.stats()["extract_presplit_fallbacks"]
        return gr
    finally:
        g.close()


@pytest.fixture(scope="module")
def synth_set():
    """20 000 reads x 100 bp of a 200 kbp genome, 1 % errors: 2 MB, about 245 extraction tiles."""
    reads = synth.reads_ascii(SEED, 200_000, 20_000, READ_LEN, 0.01)
    bases = np.ascontiguousarray(reads.reshape(-1))
    bases.setflags(write=False)
    return bases, np.arange(0, bases.size + 1, READ_LEN, dtype=np.uint64)


_unsplit = {}


def unsplit(synth_set, k, stamp64=False):
    """The f0 = 0 graph of the synthetic set, built once per (k, stamp width)."""
    if (k, stamp64) not in _unsplit:
        _unsplit[(k, stamp64)] = build(*synth_set, k, 0, stamp64)
    return _unsplit[(k, stamp64)]


@pytest.mark.parametrize("f0", [1, 4, 6])
@pytest.mark.parametrize("k", [13, 21, 31])  # W = 1, 9, 19
def test_same_graph_as_without_the_split(synth_set, k, f0):
    ref = unsplit(synth_set, k)
    got = build(*synth_set, k, f0)
    assert_same_graph(got, ref)
    assert got["fallbacks"] == 0 and ref["fallbacks"] == 0
    if f0 == 4:
        assert got["n_buckets"] == ref["n_buckets"]


def test_default_equals_the_c_oracle(synth_set):
    assert_equals_oracle(build(*synth_set, 31), *synth_set, 31)


@pytest.mark.parametrize("f0", [1, 4, 6])
def test_same_graph_with_64_bit_stamps(synth_set, f0):
    ref = unsplit(synth_set, 31, True)
    got = build(*synth_set, 31, f0, True)
    assert_same_graph(got, ref)
    assert_same_graph(got, unsplit(synth_set, 31))  # the stamp width changes nothing a caller sees
    if f0 == 4:
        assert got["n_buckets"] == ref["n_buckets"]


def awkward_reads(k):
    """Reads of exactly k bases (no successor), reads shorter than k, one read longer than a tile, a read that ends on a
    tile border (byte 16 384 of 8 192-byte tiles) and, behind it, a tail tile of 8 bases that holds no k-mer."""
    rng = np.random.default_rng(11)

    def rnd(n):
        return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))
    reads = [rnd(k), rnd(k - 1), rnd(9000), rnd(5), rnd(k), rnd(77), rnd(k + 1), rnd(1)]
    reads.append(rnd(16384 - sum(len(r) for r in reads)))
    reads.append(rnd(8))
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    assert int(offsets[-2]) == 16384 and int(offsets[-1]) == 16392
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets


@pytest.mark.parametrize("k", [13, 31])
def test_awkward_reads(k):
    bases, offsets = awkward_reads(k)
    ref = build(bases, offsets, k, 0)
    assert_equals_oracle(ref, bases, offsets, k)
    for f0 in (1, 4, 6, None):
        assert_same_graph(build(bases, offsets, k, f0), ref)


def test_total_bytes_a_multiple_of_the_tile():
    """Two reads of 8 192 bases each: both end on a tile border and no tile is partial."""
    k = 31
    rng = np.random.default_rng(12)
    bases = np.frombuffer(bytes(b"ACGT"[c] for c in rng.integers(0, 4, 16384)), dtype=np.uint8).copy()
    offsets = np.array([0, 8192, 16384], dtype=np.uint64)
    ref = build(bases, offsets, k, 0)
    assert_equals_oracle(ref, bases, offsets, k)
    for f0 in (4, 6):
        assert_same_graph(build(bases, offsets, k, f0), ref)


# ---- the fallback -----------------------------------------------------------------------------------------------------
M = 13
CODE = {65: 0, 67: 1, 84: 2, 71: 3}  # the library's 2-bit codes: ACTG


def records_per_child(read, k, f0):
    """The super-k-mer records of one read by the top f0 bits of their bucket hash: a numpy restatement of the
    extraction (minimizer = the 13-mer of the window with the least 16-bit hash, leftmost on ties; a record = a run of
    k-mers that share one minimizer occurrence; bucket hash = 22 bits of fmix32)."""
    u32 = np.uint32
    codes = np.array([CODE[c] for c in read], dtype=np.uint64)
    n_m = codes.size - M + 1
    mm = np.zeros(n_m, dtype=np.uint64)
    for i in range(M):
        mm = (mm << np.uint64(2)) | codes[i:i + n_m]
    mm = mm.astype(u32)
    with np.errstate(over="ignore"):
        h16 = ((mm ^ (mm >> u32(9)) ^ u32(0x3C6EF372)) * u32(0x9E3779B1)) >> u32(16)
        x = mm * u32(0x9E3779B1) + u32(0x7F4A7C15)
        x ^= x >> u32(16); x *= u32(0x85EBCA6B)
        x ^= x >> u32(13); x *= u32(0xC2B2AE35)
        x ^= x >> u32(16)
    bh = x >> u32(10)
    w = k - M + 1
    out = np.zeros(1 << f0, dtype=np.int64)
    prev = -1
    for q in range(codes.size - k + 1):
        at = q + int(np.argmin(h16[q:q + w]))  # argmin: the first of equal minima
        if at != prev:
            out[int(bh[at]) >> (22 - f0)] += 1
        prev = at
    return out


def test_overflow_falls_back_to_the_unsplit_extraction():
    """Low-complexity reads: 20 000 copies of one read and 2 000 reads of A only.  Every record of a copy goes to the few
    children its few minimizers hash to, and every k-mer of an all-A read is a record of its own in ONE child, so that
    child outgrows its sub-segment (1.5 x a sixteenth of the workgroup's records) and the build extracts again unsplit."""
    k = 31
    rng = np.random.default_rng(13)
    one = bytes(b"ACGT"[c] for c in rng.integers(0, 4, READ_LEN))
    poly_a = b"A" * READ_LEN
    per_child = 20_000 * records_per_child(one, k, 4) + 2_000 * records_per_child(poly_a, k, 4)
    assert per_child.max() > 1.5 / 16 * per_child.sum(), per_child  # the input does what the case needs
    bases = np.frombuffer(one * 20_000 + poly_a * 2_000, dtype=np.uint8).copy()
    offsets = np.arange(0, bases.size + 1, READ_LEN, dtype=np.uint64)
    ref = build(bases, offsets, k, 0)
    assert ref["fallbacks"] == 0
    got = build(bases, offsets, k, 4)
    assert got["fallbacks"] == 1
    assert_same_graph(got, ref)
    assert_equals_oracle(got, bases, offsets, k)


@pytest.mark.parametrize("value", [7, -1])
def test_option_range(value):
    g = _dbg.Graph()
    try:
        with pytest.raises(_dbg.DbgError) as e:
            g.set_option("extract_presplit", value)
        assert e.value.code == _dbg.DBG_E_ARG
        g.set_option("extract_presplit", 6)
        g.set_option("extract_presplit", 0)
    finally:
        g.close()
