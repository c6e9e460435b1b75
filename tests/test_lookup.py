"""The query side of a built graph through the C ABI (run with -m gpu on an MI355X): dbg_lookup_nodes on both of its paths
(the build's directory, the sorted index), dbg_gather_nodes, dbg_score_sequences, and the lazy views / score_sequences of
debruijn.py on top of them.

Expected values come from export_nodes / export_keys_hi / export_orders / export_keepmask / export_contigs of the same
graph -- pinned elsewhere against the reference's vectors -- and from plain Python over them, never from the calls under test.
"""
import contextlib
import io

import numpy as np
import pytest

import _dbg
import debruijn
import inproc_dist
import synth
from conftest import case_reads, load_golden

pytestmark = pytest.mark.gpu

NO_NODE = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
READ_LEN = 100
AA20 = b"ACDEFGHIKLMNPQRSTVWY"


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def dna_reads(seed=3, genome_len=20_000, n_reads=3000):
    """The 3 000-read case: 100 bp reads with 1 % errors."""
    return synth.reads_ascii(seed, genome_len, n_reads, READ_LEN, 0.01)


def peptide_reads(seed=9, n_reads=600, genome_len=4000, read_len=40):
    """A 20-letter synthetic set: reads of a random protein 'genome' with 1 % substitutions."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(AA20, dtype=np.uint8)
    genome = alpha[rng.integers(0, 20, genome_len)]
    starts = rng.integers(0, genome_len - read_len, n_reads)
    reads = genome[starts[:, None] + np.arange(read_len)[None, :]].copy()
    err = rng.random(reads.shape) < 0.01
    reads[err] = alpha[rng.integers(0, 20, int(err.sum()))]
    return reads


def set_rows(g, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    g.set_reads(rows.reshape(-1), np.arange(0, rows.size + 1, rows.shape[1], dtype=np.uint64))


def set_strings(g, reads):
    blob = "".join(reads).encode("latin-1")
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    g.set_reads(blob, off)


def build(rows, k, **opts):
    g = _dbg.Graph()
    for name, v in opts.items():
        g.set_option(name, v)
    set_rows(g, rows)
    g.build(k)
    return g


def counters(g):
    s = g.stats()
    return {n: s[n] for n in ("lookup_index_builds", "lookup_dir_calls", "lookup_index_calls")}


class Exported:
    """The node table of a graph as the whole-graph exports give it, with a host dict from k-mer to row."""

    def __init__(self, g):
        self.k = g.sizes()["k"]
        self.alphabet, self.bits = g.alphabet()
        self.keys, self.stamps, self.counts, self.flags = g.export_nodes()
        self.hi = g.export_keys_hi()
        self.n = self.keys.size
        self.width = self.bits * self.k
        self.row_of = {hl: i for i, hl in enumerate(zip(self.hi.tolist(), self.keys.tolist()))}  # the Python set of the nodes
        assert len(self.row_of) == self.n
        self.code_of = {ch: c for c, ch in enumerate(self.alphabet)}

    def mask_words(self):
        m = (1 << self.width) - 1
        return m >> 64, m & U64_MAX

    def expected(self, qhi, qlo):
        return np.array([self.row_of.get(hl, NO_NODE) for hl in zip(qhi.tolist(), qlo.tolist())], dtype=np.uint32)

    def one_base_changed(self, seed=1):
        """Every node's k-mer with one character changed (position and new code drawn per node)."""
        rng = np.random.default_rng(seed)
        pos = rng.integers(0, self.k, self.n)
        delta = rng.integers(1, 1 << self.bits, self.n).astype(np.uint64)
        shift = self.bits * (self.k - 1 - pos)
        in_lo = shift < 64
        lo = self.keys ^ np.where(in_lo, delta << np.where(in_lo, shift, 0).astype(np.uint64), np.uint64(0))
        hi = self.hi ^ np.where(~in_lo, delta << np.where(~in_lo, shift - 64, 0).astype(np.uint64), np.uint64(0))
        return hi, lo

    def encode(self, s):
        """(hi, lo) of a k-character byte string, None if a character is outside the alphabet."""
        v = 0
        for ch in s:
            c = self.code_of.get(ch)
            if c is None:
                return None
            v = (v << self.bits) | c
        return v >> 64, v & U64_MAX

    def host_score(self, seq):
        """(sum of the counts of the (k+1)-mers of seq that are edges, index of the first one that is not or U64_MAX)."""
        total, miss = 0, U64_MAX
        for i in range(len(seq) - self.k):
            e = self.encode(seq[i:i + self.k])
            c = self.code_of.get(seq[i + self.k])
            row = self.row_of.get(e) if e is not None else None
            n = int(self.counts[row, c]) if row is not None and c is not None else 0
            if n:
                total += n
            elif miss == U64_MAX:
                miss = i
        return total, miss


def check_lookups(g, ex, want_path):
    """Present, absent, random, out-of-range, duplicated and empty queries against the export; -> calls made."""
    before = counters(g)
    calls = 0

    def ask(hi, lo, with_hi=True):
        nonlocal calls
        calls += 1 if lo.size else 0
        return g.lookup_nodes(lo, hi if with_hi else None)

    # every node's own key returns its own row
    assert np.array_equal(ask(ex.hi, ex.keys), np.arange(ex.n, dtype=np.uint32))
    if ex.width <= 64:
        assert np.array_equal(ask(None, ex.keys, with_hi=False), np.arange(ex.n, dtype=np.uint32))
    # one base changed, minus those that are nodes: absent
    vh, vl = ex.one_base_changed()
    absent = np.fromiter((hl not in ex.row_of for hl in zip(vh.tolist(), vl.tolist())), dtype=bool, count=ex.n)
    assert absent.sum() > 0 or ex.width <= 24  # (at k = 5 every 5-mer may be a node)
    got = ask(vh[absent], vl[absent])
    assert got.size == absent.sum() and (got == NO_NODE).all()
    # 10 000 random keys of the k-mer's width (small k: many of them are nodes)
    rng = np.random.default_rng(ex.k)
    mh, ml = ex.mask_words()
    rh = rng.integers(0, 1 << 64, 10_000, dtype=np.uint64) & np.uint64(mh)
    rl = rng.integers(0, 1 << 64, 10_000, dtype=np.uint64) & np.uint64(ml)
    assert np.array_equal(ask(rh, rl), ex.expected(rh, rl))
    # bits above the k-mer's width mean "absent"
    if ex.width < 64:
        assert (ask(np.zeros(ex.n, np.uint64), ex.keys | np.uint64(1 << ex.width)) == NO_NODE).all()
    if ex.width <= 64:
        assert (ask(np.ones(ex.n, np.uint64), ex.keys) == NO_NODE).all()      # present keys with keys_hi = 1
    elif ex.width < 128:
        assert (ask(ex.hi | np.uint64(1 << (ex.width - 64)), ex.keys) == NO_NODE).all()
    # duplicated queries, present and absent mixed
    pick = rng.integers(0, ex.n, 5000)
    dh = np.concatenate([ex.hi[pick], ex.hi[pick], vh[absent][:100], vh[absent][:100]])
    dl = np.concatenate([ex.keys[pick], ex.keys[pick], vl[absent][:100], vl[absent][:100]])
    assert np.array_equal(ask(dh, dl), ex.expected(dh, dl))
    # n = 0
    assert ask(np.zeros(0, np.uint64), np.zeros(0, np.uint64)).size == 0
    after = counters(g)
    if want_path == "dir":
        assert after["lookup_dir_calls"] - before["lookup_dir_calls"] == calls
        assert after["lookup_index_calls"] == before["lookup_index_calls"]
        assert after["lookup_index_builds"] == before["lookup_index_builds"]
    else:
        assert after["lookup_index_calls"] - before["lookup_index_calls"] == calls
        assert after["lookup_dir_calls"] == before["lookup_dir_calls"]
        assert after["lookup_index_builds"] - before["lookup_index_builds"] <= 1  # once per graph, not once per call
    return calls


# ---- lookup, both paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,opts", [(5, {}), (13, {}), (21, {}), (31, {}), (32, {}), (40, {}), (63, {}), (21, {"engine": 1}),
                                    (40, {"wide_engine": 0})], ids=lambda v: str(v).replace(" ", ""))
def test_lookup_on_both_paths(k, opts):
    g = build(dna_reads(), k, **opts)
    ex = Exported(g)
    has_dir = not opts  # the LDS engines of a single-GPU build leave their directory behind
    builds0 = counters(g)["lookup_index_builds"]
    check_lookups(g, ex, "dir" if has_dir else "index")
    assert counters(g)["lookup_index_builds"] == builds0 + (0 if has_dir else 1)
    g.set_option("lookup_index", 1)
    check_lookups(g, ex, "index")
    check_lookups(g, ex, "index")
    assert counters(g)["lookup_index_builds"] == builds0 + 1
    if has_dir:
        g.set_option("lookup_index", 0)
        check_lookups(g, ex, "dir")
    g.close()


def test_lookup_through_hash_sub_ranges():
    """bucket_bits 9 on 60 000 reads: buckets overflow their LDS table and are counted in hash sub-ranges, whose
    directories hang off the bucket's chain of ranges (the geometry of test_multipass_with_forced_geometry_...)."""
    reads = synth.reads_ascii(12, 400_000, 60_000, 100, 0.01)
    g = build(reads, 31, bucket_bits=9)
    assert g.stats()["n_buckets"] == 512
    ex = Exported(g)
    assert ex.n > 512 * 2800  # a bucket is counted in sub-ranges from ~3300 distinct k-mers: the MEAN bucket is close to that
    check_lookups(g, ex, "dir")
    g.close()


def test_lookup_device_form():
    import torch
    g = build(dna_reads(), 40)
    ex = Exported(g)
    dev = torch.device("cuda", g.sizes_device())
    lo = torch.from_numpy(ex.keys.view(np.int64)).to(dev)
    hi = torch.from_numpy(ex.hi.view(np.int64)).to(dev)
    ids = g.lookup_nodes(lo, hi)
    assert ids.is_cuda and np.array_equal(ids.cpu().numpy().view(np.uint32), np.arange(ex.n, dtype=np.uint32))
    g.close()


# ---- graphs without a directory ---------------------------------------------------------------------------------------------
def walked(rows_or_strings, k, strings=False, **opts):
    g = _dbg.Graph()
    for name, v in opts.items():
        g.set_option(name, v)
    (set_strings if strings else set_rows)(g, rows_or_strings)
    g.build(k)
    g.refine_edge_order()
    g.prune(2)
    g.remove_tips()
    g.mark_pull_reads()
    g.walk(False)
    assert g.sizes()["contigs_materialised"] == 1
    return g


@pytest.mark.parametrize("k", [21, 31, 40])
def test_lookup_on_a_graph_built_from_a_walk(k):
    src = walked(dna_reads(), k)
    order = np.arange(src.sizes()["n_contigs"], dtype=np.uint64)
    g = _dbg.Graph()
    g.build_from_walk(src, k + 1, order, b"", np.zeros(1, dtype=np.uint64))
    ex = Exported(g)
    assert ex.k == k + 1 and ex.n > 0
    check_lookups(g, ex, "index")
    assert counters(g)["lookup_index_builds"] == 1
    g.close()
    src.close()


@pytest.mark.parametrize("k", [21, 40])
def test_lookup_on_an_imported_graph_and_refusal_on_a_shard(k):
    import multi_gpu
    from test_multi_gpu import rank_reads

    def one(dist, rank):
        reads = rank_reads(2, rank, 3000, READ_LEN)
        g = _dbg.Graph(device=0)
        set_rows(g, reads)
        multi_gpu.sharded_build(g, k, dist)
        with pytest.raises(_dbg.DbgError, match="gather"):  # one shard of two: its successors live in another handle
            g.lookup_nodes(g.export_nodes()[0][:4])
        with pytest.raises(_dbg.DbgError):
            g.score_sequences(b"ACGT" * 20, [0, 80])
        merged = multi_gpu.gather_graph(g, k, dist, dst=0)
        dist.barrier()
        return g, merged

    res = inproc_dist.run_ranks(2, one)
    merged = res[0][1]
    ex = Exported(merged)
    assert ex.n == sum(r[0].sizes()["n_nodes"] for r in res)
    check_lookups(merged, ex, "index")
    assert counters(merged)["lookup_index_builds"] == 1
    merged.close()
    for g, _ in res:
        g.close()


def peptide_golden():
    return case_reads(load_golden("peptide_k4_nonfinal"))


def test_lookup_on_the_peptide_example():
    g = _dbg.Graph()
    set_strings(g, peptide_golden())
    g.build(4)
    ex = Exported(g)
    assert ex.bits == 5 and ex.n == load_golden("peptide_k4_nonfinal")["summary"]["n_vertices"]
    check_lookups(g, ex, "index")
    g.close()


@pytest.mark.parametrize("k", [5, 8, 11])
def test_lookup_on_a_20_letter_alphabet(k):
    g = build(peptide_reads(), k)
    ex = Exported(g)
    assert ex.bits == 5 and ex.alphabet == AA20
    check_lookups(g, ex, "index")
    assert counters(g)["lookup_index_builds"] == 1
    g.close()


def test_graphs_the_calls_refuse():
    g = _dbg.Graph()
    with pytest.raises(_dbg.DbgError):  # no graph
        g.lookup_nodes(np.zeros(3, np.uint64))
    with pytest.raises(_dbg.DbgError):
        g.gather_nodes([0])
    with pytest.raises(_dbg.DbgError):
        g.score_sequences(b"ACGTACGT", [0, 8])
    assert g.lookup_nodes(np.zeros(0, np.uint64)).size == 0  # n = 0 touches nothing
    # the generic by-reference path: no packed keys
    set_rows(g, peptide_reads())
    g.build(12)
    with pytest.raises(_dbg.DbgError, match="packed key"):
        g.lookup_nodes(np.zeros(3, np.uint64))
    with pytest.raises(_dbg.DbgError, match="packed key"):
        g.score_sequences(AA20 * 2, [0, 40])
    # a graph in parts
    set_rows(g, dna_reads())
    g.build_multipass(21, 2)
    with pytest.raises(_dbg.DbgError, match="part"):
        g.lookup_nodes(np.zeros(3, np.uint64))
    with pytest.raises(_dbg.DbgError, match="part"):
        g.gather_nodes([0])
    with pytest.raises(_dbg.DbgError, match="part"):
        g.score_sequences(b"ACGT" * 20, [0, 80])
    # ... and the handle answers again after a plain build
    g.build(21)
    check_lookups(g, Exported(g), "dir")
    g.close()


def test_one_handle_over_time():
    """Every lookup answers for the graph that is current: the directory of an earlier build is not trusted, the index of
    an earlier graph is gone."""
    g = _dbg.Graph()
    set_rows(g, dna_reads())
    g.build(21)
    ex21 = Exported(g)
    check_lookups(g, ex21, "dir")
    g.set_option("lookup_index", 1)
    check_lookups(g, ex21, "index")
    g.build(40)
    ex40 = Exported(g)
    check_lookups(g, ex40, "index")
    g.set_option("lookup_index", 0)
    check_lookups(g, ex40, "dir")
    g.set_option("wide_engine", 0)  # the global-table engine leaves no directory: the one of the k = 40 build above is stale
    g.build(40)
    check_lookups(g, Exported(g), "index")
    g.set_option("wide_engine", 1)
    set_rows(g, dna_reads(seed=4))
    with pytest.raises(_dbg.DbgError):  # the reads changed: no graph
        g.lookup_nodes(ex21.keys[:4])
    g.build(21)
    other = Exported(g)
    assert not np.array_equal(other.keys, ex21.keys)
    check_lookups(g, other, "dir")
    g.set_option("engine", 1)
    g.build(21)
    check_lookups(g, Exported(g), "index")
    assert counters(g)["lookup_index_builds"] == 4
    g.close()


# ---- gather -----------------------------------------------------------------------------------------------------------------
def check_gather(g):
    ex = Exported(g)
    mc, fs = g.export_orders()
    keep = g.export_keepmask()
    rng = np.random.default_rng(5)
    for ids in (rng.integers(0, ex.n, 4000), np.arange(ex.n), np.array([ex.n - 1, 0, 0, ex.n - 1])):
        r = g.gather_nodes(ids)
        assert set(r) == set(_dbg.Graph.GATHER_COLUMNS)
        for name, want in (("keys", ex.keys), ("keys_hi", ex.hi), ("stamps", ex.stamps), ("counts", ex.counts), ("flags", ex.flags),
                           ("keepmask", keep), ("order", mc), ("fsorder", fs)):
            assert r[name].dtype == want.dtype and np.array_equal(r[name], want[ids]), name
    one = g.gather_nodes([3], what=("counts",))
    assert set(one) == {"counts"} and np.array_equal(one["counts"], ex.counts[[3]])
    assert g.gather_nodes([], what=("keys",))["keys"].size == 0
    assert g.gather_nodes([0, ex.n - 1], what=()) == {}          # all outputs NULL
    for bad in ([ex.n], [0, ex.n, 1], [NO_NODE]):
        with pytest.raises(_dbg.DbgError, match="n_nodes"):
            g.gather_nodes(bad)
        with pytest.raises(_dbg.DbgError, match="n_nodes"):
            g.gather_nodes(bad, what=())
    return ex


@pytest.mark.parametrize("k", [21, 40])
def test_gather_rows_of_a_dna_graph(k):
    g = _dbg.Graph()
    set_rows(g, dna_reads())
    g.build(k)
    with pytest.raises(_dbg.DbgError, match="prune"):     # the preconditions of dbg_export_keepmask / dbg_export_orders
        g.gather_nodes([0], what=("keepmask",))
    with pytest.raises(_dbg.DbgError, match="refine"):
        g.gather_nodes([0], what=("fsorder",))
    assert g.gather_nodes([0], what=("keys", "counts", "order"))["keys"].size == 1
    g.refine_edge_order()
    g.prune(2)
    g.remove_tips()
    ex = check_gather(g)
    assert (ex.flags & _dbg.F_PULLED).any() and (ex.flags & _dbg.F_BRANCH).any()
    g.close()


def test_gather_rows_of_a_generic_graph():
    g = build(peptide_reads(), 5)
    g.refine_edge_order()
    g.prune(2)
    g.remove_tips()
    ex = check_gather(g)
    assert ex.counts.shape[1] == 32
    g.close()


# ---- score ------------------------------------------------------------------------------------------------------------------
def pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return b"".join(seqs), off


def check_scores(g, ex, seqs):
    want = [ex.host_score(s) for s in seqs]
    for index in (0, 1):
        g.set_option("lookup_index", index)
        before = counters(g)
        scores, miss = g.score_sequences(*pack(seqs))
        after = counters(g)
        assert after["lookup_dir_calls"] + after["lookup_index_calls"] == before["lookup_dir_calls"] + before["lookup_index_calls"] + 1
        assert miss.tolist() == [w[1] for w in want]
        assert [int(s) for s, w in zip(scores, want) if w[1] == U64_MAX] == [w[0] for w in want if w[1] == U64_MAX]
    g.set_option("lookup_index", 0)
    return want


def score_inputs(ex, reads, foreign):
    """500 substrings of reads of lengths 1..100, the same with one character changed, and the edge cases."""
    rng = np.random.default_rng(ex.k)
    k = ex.k
    subs = []
    for _ in range(500):
        r = reads[int(rng.integers(0, len(reads)))]
        n = int(rng.integers(1, min(100, len(r)) + 1))
        a = int(rng.integers(0, len(r) - n + 1))
        subs.append(r[a:a + n])
    changed = []
    for s in subs:
        p = int(rng.integers(0, len(s)))
        other = [c for c in ex.alphabet if c != s[p]]
        changed.append(s[:p] + bytes([other[int(rng.integers(0, len(other)))]]) + s[p + 1:])
    long_read = max(reads, key=len)
    edge = [long_read[:40] + foreign + long_read[41:], long_read[:k], long_read[:k + 1], b"", long_read, foreign * (k + 3),
            foreign + long_read[1:], long_read[:-1] + foreign, b"", long_read[:1]]
    return subs, changed, edge


@pytest.mark.parametrize("k", [21, 40])
def test_scores_of_a_dna_graph(k):
    rows = dna_reads()
    g = walked(rows, k)
    ex = Exported(g)
    off, chars, score, _, _ = g.export_contigs()
    text = chars.tobytes()
    contigs = [text[int(off[i]):int(off[i + 1])] for i in range(off.size - 1)]
    assert len(contigs) > 10
    for index in (0, 1):
        g.set_option("lookup_index", index)
        got, miss = g.score_sequences(chars, off)
        assert np.array_equal(got, score) and (miss == U64_MAX).all()   # the walk's own getScore
    g.set_option("lookup_index", 0)
    reads = [r.tobytes() for r in rows]
    subs, changed, edge = score_inputs(ex, reads, b"N")
    want = check_scores(g, ex, subs)
    assert sum(w[1] == U64_MAX for w in want) > 400
    want = check_scores(g, ex, changed)
    assert sum(w[1] != U64_MAX for w in want) > 100
    want = check_scores(g, ex, edge)
    assert want[0][1] == 40 - k and want[1] == (0, U64_MAX) and want[3] == (0, U64_MAX) and want[5][1] == 0
    scores, miss = g.score_sequences(b"", [0])                            # n_seq = 0
    assert scores.size == 0 and miss.size == 0
    scores, miss = g.score_sequences(b"", [0, 0, 0])                      # empty sequences only
    assert scores.tolist() == [0, 0] and miss.tolist() == [U64_MAX] * 2
    g.close()


@pytest.mark.parametrize("k", [21, 40])
def test_scores_are_balanced_over_windows(k):
    """One 50 000-character walk (ten times around a circular genome) among 1 000 short sequences."""
    rng = np.random.default_rng(k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, 5000)]
    starts = rng.integers(0, 5000, 3000)
    rows = genome[(starts[:, None] + np.arange(READ_LEN)[None, :]) % 5000].copy()
    err = rng.random(rows.shape) < 0.01
    rows[err] = acgt[rng.integers(0, 4, int(err.sum()))]
    g = build(rows, k)
    ex = Exported(g)
    around = np.tile(genome, 11)[:50_000].tobytes()
    shorts = [rows[i % 3000, (i % 7):(i % 7) + 30 + (i % 60)].tobytes() for i in range(1000)]
    seqs = shorts[:500] + [around] + shorts[500:]
    want = check_scores(g, ex, seqs)
    assert want[500][1] == U64_MAX and want[500][0] > 50_000 - k
    g.close()


def test_scores_of_the_peptide_example_and_a_20_letter_graph():
    reads = peptide_golden()
    g = walked(reads, 4, strings=True)
    ex = Exported(g)
    off, chars, score, _, _ = g.export_contigs()
    got, miss = g.score_sequences(chars, off)
    assert off.size > 1 and np.array_equal(got, score) and (miss == U64_MAX).all()
    subs, changed, edge = score_inputs(ex, [r.encode() for r in reads], b"X")
    check_scores(g, ex, subs)
    check_scores(g, ex, changed)
    check_scores(g, ex, [r.encode() for r in reads] + [b"", b"EVQLX", b"XXXXXXXX", b"EVQ"])
    g.close()
    rows = peptide_reads()
    g = walked(rows, 8)
    ex = Exported(g)
    off, chars, score, _, _ = g.export_contigs()
    got, miss = g.score_sequences(chars, off)
    assert np.array_equal(got, score) and (miss == U64_MAX).all()
    subs, changed, edge = score_inputs(ex, [r.tobytes() for r in rows], b"X")
    check_scores(g, ex, subs)
    check_scores(g, ex, changed)
    check_scores(g, ex, edge)
    g.close()


# ---- the views of debruijn.py -----------------------------------------------------------------------------------------------
def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def get_score(table, contig, k):
    """II_assembleFromReads.py:14-18"""
    return sum(table[contig[i:i + k + 1]] for i in range(len(contig) - k))


@pytest.mark.parametrize("name", ["dna_small_k5_e1_t2", "dna_small_k9_e1_t1", "dna_small_k33_e1_t2", "peptide_k4_nonfinal"])
def test_lazy_views_answer_point_queries_on_the_device(name, monkeypatch):
    import II_assembleFromReads as driver
    case = load_golden(name)
    reads, inp = case_reads(case), case["inputs"]
    k, thr = inp["k"], inp["threshold"]
    (eV, eE), _, ebranch, epulled, eect = quiet(debruijn.construct_graph, list(reads), k, threshold=thr, final=inp["final"])
    assert isinstance(eV, dict) and isinstance(eE, dict) and isinstance(eect, dict)
    monkeypatch.setattr(debruijn, "LAZY_MIN_NODES", 0)
    (V, E), _, branch, pulled, ect = quiet(debruijn.construct_graph, list(reads), k, threshold=thr, final=inp["final"])
    assert type(V) is debruijn._LazyVertices and type(E) is debruijn._LazyEdges and type(ect) is debruijn._LazyEdgeCounts
    for lab, node in eV.items():
        assert lab in V
        got = V[lab]
        assert (got.label, got.indegree, got.outdegree) == (node.label, node.indegree, node.outdegree)
        assert (lab in E) == (lab in eE)
        if lab in eE:
            assert E[lab] == eE[lab]
        else:  # a pulled node
            with pytest.raises(KeyError):
                E[lab]
    for name_, n in eect.items():
        assert name_ in ect and ect[name_] == n
    some = next(iter(eV))
    foreign = "N" if "N" not in V._s.code_of else "#"
    absent_nodes = ["", some[:-1], some + some[-1], foreign * k, some[:-1] + foreign, None, 7, ("A",) * k]
    absent_nodes += [lab[:-1] + ch for lab in list(eV)[:40] for ch in V._s.chars if lab[:-1] + ch not in eV]
    for lab in absent_nodes:
        assert lab not in V and lab not in E
        with pytest.raises(KeyError):
            V[lab]
        with pytest.raises(KeyError):
            E[lab]
    absent_edges = ["", some, some + foreign, foreign * (k + 1), None, 7]
    absent_edges += [lab + ch for lab in list(eV)[:40] for ch in V._s.chars if lab + ch not in eect]
    for name_ in absent_edges:
        assert name_ not in ect
        with pytest.raises(KeyError):
            ect[name_]
    assert V._s._arrays is None  # nothing of size n_nodes left the device for any of the above

    # getScore over the lazy table: one device call, the reference's values
    contigs = quiet(debruijn.output_contigs, (V, E), branch, pulled)
    assert len(contigs) > 0
    want = [get_score(eect, c, k) for c in contigs]
    assert debruijn.score_sequences(ect, list(contigs), k) == want == list(contigs.scores)
    assert [driver.getScore(ect, c, k) for c in list(contigs)[:5]] == want[:5]
    assert debruijn.score_sequences(eect, list(contigs), k) == want      # a plain dict: the reference's loop
    longest = max(contigs, key=len)
    bad = longest[:len(longest) // 2] + foreign + longest[len(longest) // 2 + 1:]
    mixed = list(contigs)[:2] + [bad] + list(contigs)[2:] + [foreign * (k + 1)]
    with pytest.raises(KeyError) as host:
        [get_score(eect, c, k) for c in mixed]
    with pytest.raises(KeyError) as dev:
        debruijn.score_sequences(ect, mixed, k)
    assert dev.value.args == host.value.args and foreign in dev.value.args[0]
    with pytest.raises(KeyError):
        driver.getScore(ect, bad, k)
    assert V._s._arrays is None

    # materialised, the views still answer -- now from the host arrays
    assert dict(V).keys() == eV.keys()
    assert V._s._arrays is not None
    for lab in list(eV)[:200]:
        assert lab in V and V[lab].outdegree == eV[lab].outdegree and (lab in E) == (lab in eE)
    for name_ in list(eect)[:200]:
        assert ect[name_] == eect[name_]
    assert foreign * k not in V and foreign * (k + 1) not in ect
    assert debruijn.score_sequences(ect, list(contigs), k) == want


def test_views_of_a_replaced_graph_raise(monkeypatch, tmp_path):
    monkeypatch.setattr(debruijn, "LAZY_MIN_NODES", 0)
    reads = synth.reads_list(3, 4000, 600, 100, 0.01)
    path = str(tmp_path / "reads.fasta")
    synth.write_fasta(path, reads)
    dr = debruijn.read_reads_device(path)
    (V, E), _, _, _, ect = quiet(debruijn.construct_graph, dr, 21, threshold=2)
    lab = reads[0][:21]
    assert lab in V and reads[0][:22] in ect and V._s._arrays is None
    (V2, E2), _, _, _, ect2 = quiet(debruijn.construct_graph, dr, 25, threshold=2)
    for fn in (lambda: lab in V, lambda: V[lab], lambda: lab in E, lambda: E[lab], lambda: ect[reads[0][:22]],
               lambda: debruijn.score_sequences(ect, [reads[0]], 21), lambda: len(E)):
        with pytest.raises(RuntimeError, match="later build"):
            fn()
    assert reads[0][:25] in V2 and reads[0][:26] in ect2 and V2._s._arrays is None
