"""Point queries on a graph in parts through the C ABI (run with -m gpu on an MI355X): dbg_part_lookup_nodes[_device] and
dbg_part_score_sequences on a multi-pass build, on the ranks of ranks x passes, and PartTraversal.lookup / .score_sequences
on top of them.

Expected values come only from export_part of every part -- a host dict from (hi, lo) to (virtual shard, local id), the
counts of the CSR as a dense table -- and from plain Python over them, never from the calls under test.
"""
import numpy as np
import pytest

import _dbg
import inproc_dist
import multi_gpu
import part_traversal
import synth

pytestmark = pytest.mark.gpu

NO_NODE = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
CODE_OF = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3}  # (ascii >> 1) & 3


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def dna_reads(seed=3, genome_len=20_000, n_reads=3000, read_len=100, first_read=0):
    """The 3 000-read case (or a rank's share of it): 100 bp reads with 1 % errors on a 20 kb genome."""
    return synth.reads_ascii(seed, genome_len, n_reads, read_len, 0.01, first_read=first_read)


def set_rows(g, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    g.set_reads(rows.reshape(-1), np.arange(0, rows.size + 1, rows.shape[1] if rows.size else 1, dtype=np.uint64))


def multipass(rows, k, n_passes, **opts):
    g = _dbg.Graph()
    for name, v in opts.items():
        g.set_option(name, v)
    set_rows(g, rows)
    g.build_multipass(k, n_passes)
    assert g.part_count() == n_passes
    return g


def dense_counts(d):
    """[n, 4] counts by base code from a part's CSR: the columns of a row follow the base codes set in flags."""
    n = d["keys"].size
    counts = np.zeros((n, 4), dtype=np.uint32)
    e = d["row_ptr"][:-1].astype(np.int64).copy()
    for code in range(4):
        has = ((d["flags"] >> (1 + code)) & 1).astype(bool)
        counts[has, code] = d["cnt"][e[has]]
        e[has] += 1
    assert np.array_equal(e, d["row_ptr"][1:].astype(np.int64))
    return counts


class Whole:
    """The whole graph from the exports of all its parts (index = virtual shard), with the host dict of its nodes."""

    def __init__(self, parts, k):
        self.k, self.parts, self.nv = k, parts, len(parts)
        self.counts = [dense_counts(d) for d in parts]
        self.lo = np.concatenate([d["keys"] for d in parts])
        self.hi = np.concatenate([d["keys_hi"] for d in parts])
        self.v = np.concatenate([np.full(d["keys"].size, v, dtype=np.int64) for v, d in enumerate(parts)])
        self.local = np.concatenate([np.arange(d["keys"].size, dtype=np.int64) for d in parts])
        self.n = self.lo.size
        self.node_of = {hl: vl for hl, vl in zip(zip(self.hi.tolist(), self.lo.tolist()), zip(self.v.tolist(), self.local.tolist()))}
        assert len(self.node_of) == self.n  # no k-mer is a node of two parts
        self._changed = {}

    def mask_words(self):
        m = (1 << (2 * self.k)) - 1
        return m >> 64, m & U64_MAX

    def changed(self, seed=1):
        """Every node's k-mer with one base changed, minus those that are nodes: (hi, lo) of k-mers the graph does not hold."""
        if seed in self._changed:
            return self._changed[seed]
        rng = np.random.default_rng(seed)
        pos = rng.integers(0, self.k, self.n)
        delta = rng.integers(1, 4, self.n).astype(np.uint64)
        shift = 2 * (self.k - 1 - pos)
        in_lo = shift < 64
        lo = self.lo ^ np.where(in_lo, delta << np.where(in_lo, shift, 0).astype(np.uint64), np.uint64(0))
        hi = self.hi ^ np.where(~in_lo, delta << np.where(~in_lo, shift - 64, 0).astype(np.uint64), np.uint64(0))
        absent = np.fromiter((hl not in self.node_of for hl in zip(hi.tolist(), lo.tolist())), dtype=bool, count=self.n)
        self._changed[seed] = hi[absent], lo[absent]
        return self._changed[seed]

    def expected(self, qhi, qlo, v_first, n_parts):
        """(owner or -1 where the export cannot tell, local) a handle with the parts [v_first, v_first + n_parts) answers."""
        owner, local = np.full(qlo.size, -1, dtype=np.int64), np.full(qlo.size, NO_NODE, dtype=np.int64)
        for i, hl in enumerate(zip(qhi.tolist(), qlo.tolist())):
            vl = self.node_of.get(hl)
            if vl is not None:
                owner[i] = vl[0]
                if v_first <= vl[0] < v_first + n_parts:
                    local[i] = vl[1]
        return owner, local

    def gids(self, qhi, qlo):
        return np.array([(vl[0] << 32) | vl[1] if vl is not None else -1
                         for vl in (self.node_of.get(hl) for hl in zip(qhi.tolist(), qlo.tolist()))], dtype=np.int64)

    def host_score(self, seq):
        """test_lookup.py's host_score over the union of the part exports: (sum of the counts of the (k+1)-mers of seq that
        are edges, index of the first one that is not or U64_MAX).  The k-mer of window i is spelled from its own k characters
        (kept as a running number; `good` = characters since the last one outside ACGT)."""
        k, total, miss = self.k, 0, U64_MAX
        full = (1 << (2 * k)) - 1
        v, good = 0, 0
        for j, ch in enumerate(seq):
            i = j - k  # seq[j] is the character behind the k-mer seq[i:j]
            c = CODE_OF.get(ch)
            if i >= 0:
                vl = self.node_of.get((v >> 64, v & U64_MAX)) if good >= k else None
                n = int(self.counts[vl[0]][vl[1], c]) if vl is not None and c is not None else 0
                if n:
                    total += n
                elif miss == U64_MAX:
                    miss = i
            v = ((v << 2) | (c or 0)) & full
            good = good + 1 if c is not None else 0
        return total, miss


def whole_of(g, k):
    return Whole([g.export_part(p) for p in range(g.part_count())], k)


def check_answer(w, got, qhi, qlo, v_first, n_parts):
    owner, local = got
    assert owner.dtype == np.uint8 and local.dtype == np.uint32 and owner.size == local.size == qlo.size
    want_owner, want_local = w.expected(qhi, qlo, v_first, n_parts)
    assert np.array_equal(local.astype(np.int64), want_local)
    known = want_owner >= 0
    assert np.array_equal(owner.astype(np.int64)[known], want_owner[known])
    assert (owner[~known] < w.nv).all()  # an absent k-mer still has an owner: a function of the key alone


def check_nodes_and_changed(g, w, v_first=0, n_parts=None):
    """Every node's own key returns its own (part, local); the changed keys are absent."""
    n_parts = w.nv if n_parts is None else n_parts
    owner, local = g.part_lookup_nodes(w.lo, w.hi)
    assert np.array_equal(owner.astype(np.int64), w.v)
    mine = (w.v >= v_first) & (w.v < v_first + n_parts)
    assert np.array_equal(local.astype(np.int64), np.where(mine, w.local, NO_NODE))
    ch, cl = w.changed()
    assert cl.size > 0
    owner, local = g.part_lookup_nodes(cl, ch)
    assert (local == NO_NODE).all() and (owner < w.nv).all()
    return ch, cl


def check_lookups(g, w):
    """The cases of test_lookup.check_lookups on a handle that holds every part."""
    calls0 = g.stats()["part_lookup_calls"]
    ch, cl = check_nodes_and_changed(g, w)
    if 2 * w.k <= 64:
        owner, local = g.part_lookup_nodes(w.lo)  # keys_hi None: zeros
        assert np.array_equal(owner.astype(np.int64), w.v) and np.array_equal(local.astype(np.int64), w.local)
    rng = np.random.default_rng(w.k)
    mh, ml = w.mask_words()
    rh = rng.integers(0, 1 << 64, 10_000, dtype=np.uint64) & np.uint64(mh)
    rl = rng.integers(0, 1 << 64, 10_000, dtype=np.uint64) & np.uint64(ml)
    check_answer(w, g.part_lookup_nodes(rl, rh), rh, rl, 0, w.nv)
    # bits above 2k: no k-mer at all
    if 2 * w.k < 64:
        owner, local = g.part_lookup_nodes(w.lo | np.uint64(1 << (2 * w.k)), np.zeros(w.n, np.uint64))
        assert (owner == 0xFF).all() and (local == NO_NODE).all()
    if 2 * w.k <= 64:
        owner, local = g.part_lookup_nodes(w.lo, np.ones(w.n, np.uint64))
    else:
        owner, local = g.part_lookup_nodes(w.lo, w.hi | np.uint64(1 << (2 * w.k - 64)))
    assert (owner == 0xFF).all() and (local == NO_NODE).all()
    # duplicated queries, present and absent mixed
    pick = rng.integers(0, w.n, 5000)
    dh = np.concatenate([w.hi[pick], w.hi[pick], ch[:100], ch[:100]])
    dl = np.concatenate([w.lo[pick], w.lo[pick], cl[:100], cl[:100]])
    check_answer(w, g.part_lookup_nodes(dl, dh), dh, dl, 0, w.nv)
    # n = 0 touches nothing
    calls = g.stats()["part_lookup_calls"]
    owner, local = g.part_lookup_nodes(np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    assert owner.size == 0 and local.size == 0 and g.stats()["part_lookup_calls"] == calls > calls0
    # the device-tensor form
    import torch
    dev = torch.device("cuda", g.sizes_device())
    t_lo, t_hi = torch.from_numpy(dl.view(np.int64)).to(dev), torch.from_numpy(dh.view(np.int64)).to(dev)
    owner, local = g.part_lookup_nodes(t_lo, t_hi)
    assert owner.is_cuda and local.is_cuda and owner.dtype == torch.uint8 and local.dtype == torch.int32
    check_answer(w, (owner.cpu().numpy(), local.cpu().numpy().view(np.uint32)), dh, dl, 0, w.nv)
    owner, local = g.part_lookup_nodes(t_lo[:0], t_hi[:0])
    assert owner.numel() == 0 and local.numel() == 0


# ---- 1. one handle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_passes", [(21, 1), (21, 4), (31, 2), (31, 64), (40, 1), (40, 64), (63, 2), (63, 4)])
def test_lookup_on_one_handle(k, n_passes):
    g = multipass(dna_reads(), k, n_passes)
    w = whole_of(g, k)
    assert w.n > 20_000
    check_lookups(g, w)
    g.close()


# ---- 2. hash sub-ranges -----------------------------------------------------------------------------------------------------
def test_lookup_through_hash_sub_ranges():
    """bucket_bits 9 on 60 000 reads (the geometry of test_multipass_with_forced_geometry_and_overflowing_buckets): buckets
    overflow their LDS table and are counted in hash sub-ranges, whose directories hang off the bucket's chain of ranges."""
    g = multipass(synth.reads_ascii(12, 400_000, 60_000, 100, 0.01), 31, 4, bucket_bits=9)
    w = whole_of(g, 31)
    assert w.n > 512 * 2800  # a bucket is counted in sub-ranges from ~3300 distinct k-mers: the MEAN bucket is close to that
    check_nodes_and_changed(g, w)
    g.close()


# ---- 3. empty parts ---------------------------------------------------------------------------------------------------------
def test_lookup_with_empty_parts():
    g = multipass(synth.reads_ascii(13, 2000, 40, 60, 0.0), 31, 64)
    assert any(g.part_sizes(p)["n_nodes"] == 0 for p in range(64))
    w = whole_of(g, 31)
    assert w.n > 0
    check_nodes_and_changed(g, w)
    scores, miss = g.part_score_sequences(b"ACGT" * 20, [0, 80])
    assert scores.tolist() == [0] and miss.tolist() == [0]
    g.close()


def test_lookup_on_a_graph_without_reads():
    g = _dbg.Graph()
    g.set_reads(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    g.build_multipass(31, 4)
    assert g.sizes()["n_nodes"] == 0
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 1 << 62, 5000, dtype=np.uint64)
    owner, local = g.part_lookup_nodes(keys)
    assert (local == NO_NODE).all() and (owner < 4).all()
    scores, miss = g.part_score_sequences(b"ACGT" * 20 + b"AC", [0, 80, 82])
    assert scores.tolist() == [0, 0] and miss.tolist() == [0, U64_MAX]
    g.close()


# ---- 4. ranks x passes in process -------------------------------------------------------------------------------------------
def build_ranks(ranks, n_passes, k):
    """-> (the handles of the ranks, the whole graph from everybody's exports); rank r holds reads [r * per, (r + 1) * per)."""
    per = 3000 // ranks

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        set_rows(g, dna_reads(n_reads=per, first_read=rank * per))
        multi_gpu.sharded_build_multipass(g, k, dist, n_passes)
        assert g.part_count() == n_passes
        return g, [g.export_part(p) for p in range(n_passes)]

    got = inproc_dist.run_ranks(ranks, one)
    return [g for g, _ in got], Whole([d for _, ps in got for d in ps], k)


@pytest.mark.parametrize("ranks,n_passes,k", [(2, 2, 31), (4, 1, 63), (8, 1, 31), (2, 4, 40)])
def test_lookup_on_ranks_times_passes(ranks, n_passes, k):
    gs, w = build_ranks(ranks, n_passes, k)
    assert w.nv == ranks * n_passes and w.n > 20_000
    ch, cl = w.changed()
    assert cl.size > 0

    def one(dist, rank):
        g = gs[rank]
        # the keys of all nodes of the whole graph: local ids for the own parts, the owner byte for everybody's
        check_nodes_and_changed(g, w, rank * n_passes, n_passes)
        # PartTraversal.lookup: different queries on every rank, nodes and changed keys mixed, in query order
        rng = np.random.default_rng(100 + rank)
        pick = rng.permutation(w.n)[:4000 + 500 * rank]
        miss = rng.permutation(cl.size)[:300 + 10 * rank]
        qh, ql = np.concatenate([w.hi[pick], ch[miss]]), np.concatenate([w.lo[pick], cl[miss]])
        o = rng.permutation(ql.size)
        qh, ql = qh[o], ql[o]
        t = part_traversal.PartTraversal(g, k, dist)
        gid = t.lookup(ql, qh)
        assert gid.dtype == np.int64 and np.array_equal(gid, w.gids(qh, ql))
        assert int((gid < 0).sum()) == miss.size
        if 2 * k <= 64:
            assert np.array_equal(t.lookup(ql), gid)
        return True

    assert all(inproc_dist.run_ranks(ranks, one))
    for g in gs:
        g.close()


def test_traversal_lookup_on_one_process():
    g = multipass(dna_reads(), 31, 4)
    w = whole_of(g, 31)
    t = part_traversal.PartTraversal(g, 31)
    ch, cl = w.changed()
    qh, ql = np.concatenate([w.hi, ch[:500]]), np.concatenate([w.lo, cl[:500]])
    gid = t.lookup(ql, qh)
    assert np.array_equal(gid, w.gids(qh, ql)) and int((gid < 0).sum()) == 500
    import torch
    dev = torch.device("cuda", g.sizes_device())
    gid_t = t.lookup(torch.from_numpy(ql.view(np.int64)).to(dev), torch.from_numpy(qh.view(np.int64)).to(dev))
    assert gid_t.is_cuda and np.array_equal(gid_t.cpu().numpy(), gid)
    g.close()


# ---- 5. scores --------------------------------------------------------------------------------------------------------------
def pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return b"".join(seqs), off


_sequences = {}


def score_sequences_for(k):
    """200 reads, the contigs of a single-GPU build + prune(2) + walk of the same reads, the genome itself (five tiles), an N in
    the middle, lengths k and k + 1, an empty one, a foreign random sequence."""
    if k not in _sequences:
        rows = dna_reads()
        g = _dbg.Graph()
        set_rows(g, rows)
        g.build(k)
        g.refine_edge_order()
        g.prune(2)
        g.remove_tips()
        g.mark_pull_reads()
        g.walk(False)
        off, chars, _, _, _ = g.export_contigs()
        g.close()
        text = chars.tobytes()
        contigs = [text[int(off[i]):int(off[i + 1])] for i in range(off.size - 1)]
        assert len(contigs) > 10
        genome = synth.ALPHABET[synth.genome_codes(3, 0, 20_000)].tobytes()
        reads = [r.tobytes() for r in rows[::15]]
        assert len(reads) == 200
        foreign = synth.ALPHABET[np.random.default_rng(k).integers(0, 4, 3000)].tobytes()
        edge = [reads[0][:40] + b"N" + reads[0][41:], reads[1][:k], reads[1][:k + 1], b"", foreign]
        _sequences[k] = reads + contigs + [genome] + edge
    return _sequences[k]


def check_expected_scores(want):
    """The inputs really cover what they are meant to: sequences that score without a miss, and the edge cases."""
    assert sum(m == U64_MAX and s > 0 for s, m in want) > 100
    n_in_middle, len_k, len_k1, empty, foreign = want[-5:]
    assert n_in_middle[1] != U64_MAX and len_k == (0, U64_MAX) and len_k1[1] == U64_MAX and len_k1[0] > 0
    assert empty == (0, U64_MAX) and foreign[1] == 0


@pytest.mark.parametrize("k,n_passes", [(21, 4), (40, 2)])
def test_scores_on_one_handle(k, n_passes):
    g = multipass(dna_reads(), k, n_passes)
    w = whole_of(g, k)
    seqs = score_sequences_for(k)
    want = [w.host_score(s) for s in seqs]
    check_expected_scores(want)
    calls = g.stats()["part_lookup_calls"]
    scores, miss = g.part_score_sequences(*pack(seqs))
    assert g.stats()["part_lookup_calls"] == calls + 1
    assert miss.tolist() == [m for _, m in want] and [int(s) for s in scores] == [s for s, _ in want]
    t = part_traversal.PartTraversal(g, k)
    scores, miss = t.score_sequences(*pack(seqs))
    assert miss.tolist() == [m for _, m in want] and [int(s) for s in scores] == [s for s, _ in want]
    scores, miss = g.part_score_sequences(b"", [0])                       # n_seq = 0
    assert scores.size == 0 and miss.size == 0
    scores, miss = g.part_score_sequences(b"", [0, 0, 0])                 # empty sequences only
    assert scores.tolist() == [0, 0] and miss.tolist() == [U64_MAX] * 2
    g.close()


@pytest.mark.parametrize("ranks,n_passes,k", [(2, 2, 31), (4, 1, 63)])
def test_scores_on_ranks_times_passes(ranks, n_passes, k):
    gs, w = build_ranks(ranks, n_passes, k)
    seqs = score_sequences_for(k)
    want = [w.host_score(s) for s in seqs]
    check_expected_scores(want)
    chars, off = pack(seqs)

    def one(dist, rank):
        partial = gs[rank].part_score_sequences(chars, off)
        both = part_traversal.PartTraversal(gs[rank], k, dist).score_sequences(chars, off)
        return partial, both

    got = inproc_dist.run_ranks(ranks, one)
    total = np.sum([p[0] for p, _ in got], axis=0, dtype=np.uint64)
    first = np.min([p[1] for p, _ in got], axis=0)
    assert [int(s) for s in total] == [s for s, _ in want] and first.tolist() == [m for _, m in want]
    assert sum(int(p[0].sum()) > 0 for p, _ in got) == ranks  # every rank owns some of the windows
    for _, (scores, miss) in got:
        assert [int(s) for s in scores] == [s for s, _ in want] and miss.tolist() == [m for _, m in want]
    for g in gs:
        g.close()


def test_score_sequences_refuses_different_sequences_on_the_ranks():
    gs, _ = build_ranks(2, 1, 31)

    def one(dist, rank):
        seq = b"ACGT" * 20 if rank == 0 else b"ACGA" * 20  # the same sizes, another text
        with pytest.raises(RuntimeError, match="different sequences"):
            part_traversal.PartTraversal(gs[rank], 31, dist).score_sequences(seq, [0, 80])
        return True

    assert all(inproc_dist.run_ranks(2, one))
    for g in gs:
        g.close()


# ---- 6. against the walk in parts -------------------------------------------------------------------------------------------
def test_scores_of_the_contigs_of_the_walk_in_parts():
    k = 31
    g = multipass(dna_reads(), k, 4)
    w = whole_of(g, k)
    before = g.part_lookup_nodes(w.lo, w.hi)
    res = part_traversal.traverse(g, k, 2)
    t, _, _, _ = part_traversal.construct_graph(g, k, 2)          # the same traversal, keeping the skeleton for the texts
    ctg = part_traversal.output_contigs(t)
    assert len(ctg) > 10 and np.array_equal(ctg.scores, res["contigs"]["score"])
    texts = [s.encode("ascii") for s in ctg.texts(range(len(ctg)))]
    scores, miss = t.score_sequences(*pack(texts))
    assert np.array_equal(scores.astype(np.int64), np.asarray(ctg.scores, dtype=np.int64))
    assert (miss == np.uint64(U64_MAX)).all()
    # prune, tips and segments left the directories alone
    after = g.part_lookup_nodes(w.lo, w.hi)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    check_nodes_and_changed(g, w)
    g.close()


# ---- 7. one handle over time ------------------------------------------------------------------------------------------------
def test_one_handle_over_time():
    """Every answer is for the graph that is current: the descriptor table of an earlier graph in parts is not trusted."""
    rows = dna_reads()
    g = multipass(rows, 21, 2)
    old = whole_of(g, 21)
    check_nodes_and_changed(g, old)
    g.build(21)
    with pytest.raises(_dbg.DbgError, match="parts"):
        g.part_lookup_nodes(old.lo[:4])
    with pytest.raises(_dbg.DbgError, match="parts"):
        g.part_score_sequences(b"ACGT" * 20, [0, 80])
    keys, _, _, _ = g.export_nodes()
    assert np.array_equal(g.lookup_nodes(keys), np.arange(keys.size, dtype=np.uint32))
    # other reads; 200 of them start with ten A's and a 21-mer of the old graph, so that the packed 31-mer IS the old 21-mer's key
    other = dna_reads(seed=4).copy()
    other[:200, :10] = ord("A")
    other[:200, 10:31] = rows[:200, :21]
    set_rows(g, other)
    g.build_multipass(31, 4)
    new = whole_of(g, 31)
    check_nodes_and_changed(g, new)
    both = [hl for hl in old.node_of if hl in new.node_of]
    assert len(both) >= 100
    assert any(old.node_of[hl] != new.node_of[hl] for hl in both)
    lo = np.array([hl[1] for hl in both], dtype=np.uint64)
    owner, local = g.part_lookup_nodes(lo)
    assert [(int(o), int(x)) for o, x in zip(owner, local)] == [new.node_of[hl] for hl in both]
    g.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_what_the_calls_refuse():
    import torch
    g = _dbg.Graph()
    for _ in range(2):  # a fresh handle, then a plain build
        with pytest.raises(_dbg.DbgError, match="parts"):
            g.part_lookup_nodes(np.zeros(3, np.uint64))
        with pytest.raises(_dbg.DbgError, match="parts"):
            g.part_lookup_nodes(torch.zeros(3, dtype=torch.int64, device=torch.device("cuda", g.sizes_device())))
        with pytest.raises(_dbg.DbgError, match="parts"):
            g.part_score_sequences(b"ACGT" * 20, [0, 80])
        owner, local = g.part_lookup_nodes(np.zeros(0, np.uint64))  # n = 0 touches nothing
        assert owner.size == 0 and local.size == 0
        set_rows(g, dna_reads(n_reads=300))
        g.build(21)
    g.build_multipass(21, 2)
    with pytest.raises(_dbg.DbgError, match=r"offsets\[0\]"):
        g.part_score_sequences(b"ACGT" * 20, [1, 80])
    with pytest.raises(_dbg.DbgError, match="non-decreasing"):
        g.part_score_sequences(b"ACGT" * 20, [0, 60, 40, 80])
    with pytest.raises(_dbg.DbgError, match="tensor on"):
        g.part_lookup_nodes(torch.zeros(3, dtype=torch.int64))      # a host tensor
    dev = torch.device("cuda", g.sizes_device())
    with pytest.raises(_dbg.DbgError, match="tensor on"):
        g.part_lookup_nodes(torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64))
    owner, local = g.part_lookup_nodes(np.zeros(3, np.uint64))      # ... and the handle still answers
    assert owner.size == 3 and (owner < 2).all()
    g.close()
