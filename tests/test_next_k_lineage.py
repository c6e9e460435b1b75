"""The driver's steps from the third k on (dbg_build_from_walks): the reads are the contigs of the previous walk, blocks of
pulled contigs of earlier walks and a few real reads.  Every block stays on the device as references into the graph that
holds it; the graph built from the chains equals the text path's on the spelled-out reads."""
import numpy as np
import pytest

import _dbg
import debruijn
import synth
from conftest import load_golden
from test_next_k_from_walk import _graph_view, _quiet

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _index_only_walks(monkeypatch):
    """Forced-lazy contigs: the list-ranking walk also for small graphs, and no contig text kept by a walk."""
    monkeypatch.setenv("DBG_WALK_JUMP_MIN", "1")
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)


def _no_text(m):
    m.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("contig text left the device")))


def _count_calls(m):
    calls = []
    real = _dbg.Graph.build_from_walk
    m.setattr(_dbg.Graph, "build_from_walk", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def _virtual_blocks(lazy):
    return [t for t in lazy._tail if type(t) is debruijn._ContigBlock]


def _driver_step(seqs, k, thr):
    """II_assembleFromReads.py:57-74 for one non-final k -> (result of construct_graph, the next step's reads)."""
    res = _quiet(debruijn.construct_graph, seqs, k, threshold=thr)
    lazy = _quiet(debruijn.output_contigs, res[0], res[2], res[3])
    assert isinstance(lazy, debruijn.LazyContigs)
    lazy.sort(reverse=True)
    lazy.extend(res[1])
    return res, lazy


def test_no_text_leaves_the_device_over_the_driver(monkeypatch):
    seqs = synth.reads_list(5, 6000, 900, 100, 0.01)
    _no_text(monkeypatch)
    calls = _count_calls(monkeypatch)
    for k in range(21, 25):
        if k == 24:  # the reads of the last step: pulled contigs of the walks at k = 22 and k = 21 are still virtual
            assert sum(len(b) >= 100 for b in _virtual_blocks(seqs)) >= 2
        res, seqs = _driver_step(seqs, k, 2)
        assert len(res[0][0]) > 0
    assert len(calls) == 3


@pytest.mark.parametrize("reads_args,k0,steps,thr", [
    ((5, 6000, 900, 100, 0.01), 21, 5, 2),
    ((31, 5000, 3000, 100, 0.01), 29, 5, 2),    # one key word to two inside the lineage
    ((43, 3000, 2500, 60, 0.02), 11, 5, 1),     # tie-heavy orders
    ((47, 5000, 2000, 100, 0.01), 40, 4, 2),    # two-word keys throughout
])
def test_exact_against_text_path_step_by_step(monkeypatch, reads_args, k0, steps, thr):
    seqs = synth.reads_list(*reads_args)
    for step, k in enumerate(range(k0, k0 + steps)):
        spelled = [seqs[i] for i in range(len(seqs))]
        want = _quiet(debruijn.construct_graph, spelled, k, threshold=thr)
        cw = _quiet(debruijn.output_contigs, want[0], want[2], want[3])
        if step >= 2:
            assert _virtual_blocks(seqs), "the tail holds no virtual block"
        with monkeypatch.context() as m:
            _no_text(m)
            calls = _count_calls(m)
            got, nxt = _driver_step(seqs, k, thr)
            assert len(calls) == (1 if step else 0)  # the device path, once per step
            sz = got[0][0]._graph.sizes()
            assert sz["n_reads"] == len(spelled) and sz["n_bytes"] == sum(map(len, spelled))
        assert _graph_view(got) == _graph_view(want)
        n = len(nxt._order)
        texts, wtexts = [nxt[i] for i in range(n)], [cw[i] for i in range(len(cw))]
        worder = sorted(range(len(wtexts)), key=lambda i: cw.scores[i], reverse=True)  # stable, like list.sort
        assert nxt.scores == [cw.scores[i] for i in worder] and texts == [wtexts[i] for i in worder]
        assert sorted(texts) == sorted(wtexts)
        seqs = nxt


# ---- arbitrary blocks through Graph.build_from_walks
def _repeat_rich_reads():
    """The read set of test_next_k_from_walk.test_exact_cycles_and_short_contigs, then reads that end in a branch after 15,
    16 and 17 characters (contigs of 3, 4, 5 nodes at k = 13 and of 1, 2, 3 nodes at k = 15) and a small genome's reads."""
    rng = np.random.default_rng(7)
    unit = "".join(rng.choice(list("ACGT"), 37))
    genome = unit * 40 + "".join(rng.choice(list("ACGT"), 400)) + unit * 10
    reads = [genome[i:i + 90] for i in range(0, len(genome) - 90, 7)]
    reads += [genome[i:i + 13] for i in range(5, 400, 41)] + [genome[i:i + 14] for i in range(9, 400, 53)]
    reads += ["ACGTACGTACGTA", "ACGTACGTACGTAC", "TTTTTTTTTTTTTTTT"]
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))
    x, y = rnd(13), rnd(13)
    reads += [x + "A" + rnd(40), x + "C" + rnd(40)]
    reads += ["G" + y + "A" + rnd(40), y + "C" + rnd(40)]
    for length in (15, 16, 17):
        w = rnd(length)
        reads += [w + "A" + rnd(40), w + "C" + rnd(40)]
    return reads + synth.reads_list(9, 3000, 400, 100, 0.01)


def _pack(reads):
    blob = np.frombuffer("".join(reads).encode("ascii"), dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return blob, off


def _walked(reads, k, thr):
    g = _dbg.Graph()
    g.set_reads(*_pack(reads))
    g.build(k)
    g.refine_edge_order()
    g.prune(thr)
    g.remove_tips()
    g.mark_pull_reads()
    g.walk(False, 1)
    return g


def _node_arrays(g):
    """Every node sorted by (keys_hi, keys): keys, hi, stamps, counts, F_INDEG and the ranks of the counted successors."""
    keys, stamps, counts, flags = g.export_nodes()
    hi = g.export_keys_hi()
    p = np.lexsort((keys, hi))
    counts = counts[p]

    def ranked(r):  # codes without a count dropped: their place is no part of the graph
        r = np.asarray(r)[p].astype(np.int64)
        r = np.where(np.take_along_axis(counts, r, axis=1) != 0, r, 4)
        return np.take_along_axis(r, np.argsort(r == 4, axis=1, kind="stable"), axis=1)

    mc, fs = g.export_orders()
    return p, [keys[p], hi[p], stamps[p], counts, flags[p] & _dbg.F_INDEG, ranked(mc), ranked(fs)]


def _traversed(g, p, thr):
    g.prune(thr)
    g.remove_tips()
    g.mark_pull_reads()
    return [g.export_keepmask()[p], g.export_nodes(False, False, False, True)[3][p], g.export_pull_reads()]


@pytest.fixture(scope="module")
def two_sources():
    import os
    old = os.environ.get("DBG_WALK_JUMP_MIN")
    os.environ["DBG_WALK_JUMP_MIN"] = "1"
    try:
        reads = _repeat_rich_reads()
        g13, g15 = _walked(reads, 13, 1), _walked(reads, 15, 1)
    finally:
        if old is None:
            del os.environ["DBG_WALK_JUMP_MIN"]
        else:
            os.environ["DBG_WALK_JUMP_MIN"] = old
    out = {"reads": reads}
    for name, g, k in (("g13", g13, 13), ("g15", g15, 15)):
        off = g.export_contig_index()[0]
        lens = np.diff(off).astype(np.int64)
        texts = [g.export_contig_text(c, int(lens[c])).decode("ascii") for c in range(lens.size)]
        out[name] = (g, lens - k + 1, texts)   # handle, nodes per contig, texts (the reference of every variant)
    return out


def _subset(nodes, d, rng):
    """Contig indices in a shuffled order: about two thirds of the index, and every contig of d, d + 1, d + 2 nodes."""
    for n in (d, d + 1, d + 2):
        assert (nodes == n).any(), f"no contig of {n} nodes"
    pick = np.nonzero((rng.random(nodes.size) < 0.66) | ((nodes >= d) & (nodes <= d + 2)))[0]
    return rng.permutation(pick)


VARIANTS = ["two_blocks", "swapped", "empty_block", "all_shorter_than_K", "extras_only"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_arbitrary_blocks_equal_a_build_on_the_spelled_reads(two_sources, variant):
    K = 16
    rng = np.random.default_rng(11)
    reads = two_sources["reads"]
    (g13, n13, t13), (g15, n15, t15) = two_sources["g13"], two_sources["g15"]
    s15, s13 = _subset(n15, 1, rng), _subset(n13, 3, rng)
    blocks = [(g15, s15, t15), (g13, s13, t13)]
    if variant == "swapped":
        blocks.reverse()
    elif variant == "empty_block":
        blocks[0] = (g15, s15[:0], t15)
    elif variant == "all_shorter_than_K":   # fewer than d + 1 nodes: fewer than K characters
        blocks[1] = (g13, np.nonzero(n13 < 4)[0], t13)
        assert len(blocks[1][1]) >= 2
    elif variant == "extras_only":
        blocks = []
    extras = reads[100:150]
    spelled = [t[int(c)] for _, idx, t in blocks for c in idx] + extras
    for thr in (1, 2):
        want = _dbg.Graph()
        want.set_reads(*_pack(spelled))
        want.build(K)
        want.refine_edge_order()
        got = _dbg.Graph()
        got.build_from_walks(K, [(g, idx) for g, idx, _ in blocks], *_pack(extras))
        got.refine_edge_order()
        sw, sg = want.sizes(), got.sizes()
        for name in ("n_reads", "n_bytes", "n_nodes", "n_edges", "n_kmer_instances", "n_edge_instances"):
            assert sg[name] == sw[name], name
        pw, aw = _node_arrays(want)
        pg, ag = _node_arrays(got)
        for a, b in zip(aw, ag):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(_traversed(want, pw, thr), _traversed(got, pg, thr)):
            np.testing.assert_array_equal(a, b)
        assert got.sizes()["n_pull_reads"] == want.sizes()["n_pull_reads"]


@pytest.mark.parametrize("k", [21, 31])
def test_one_block_equals_build_from_walk(k):
    reads = synth.reads_list(61 + k, 5000, 2000, 100, 0.01)
    src = _walked(reads, k, 2)
    n = src.sizes()["n_contigs"]
    order = np.random.default_rng(k).permutation(n)
    extras = _pack(reads[:40])
    a, b = _dbg.Graph(), _dbg.Graph()
    a.build_from_walk(src, k + 1, order, *extras)
    b.build_from_walks(k + 1, [(src, order)], *extras)
    assert a.sizes() == b.sizes()
    for g in (a, b):
        g.refine_edge_order()
        g.prune(2)
        g.remove_tips()
        g.mark_pull_reads()
        g.walk(False, 1)
    assert a.sizes() == b.sizes()
    def exports(g):  # node order aside: rows sorted by key, node ids replaced by the rank of their key
        keys, stamps, counts, flags = g.export_nodes()
        hi = g.export_keys_hi()
        p = np.lexsort((keys, hi))
        rank = np.empty(p.size + 1, dtype=np.int64)
        rank[p] = np.arange(p.size)
        rank[-1] = -1
        ids = lambda a: rank[np.where(a == _dbg.NO_NODE, p.size, a).astype(np.int64)]
        mc, fs = g.export_orders()
        rp, col, cnt = g.export_csr()
        row = rank[np.repeat(np.arange(p.size), np.diff(rp).astype(np.int64))]
        e = np.lexsort((ids(col), row))
        off, score, stamp, seq = g.export_contig_index()
        c = np.lexsort((seq, stamp))
        return [keys[p], hi[p], stamps[p], counts[p], flags[p], ids(g.export_succ()[p]), g.export_keepmask()[p], mc[p], fs[p],
                ids(g.export_dict_order()), g.export_pull_reads(), row[e], ids(col)[e], cnt[e],
                np.diff(off)[c], score[c], stamp[c], seq[c]]

    for x, y in zip(exports(a), exports(b)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["driver_dna_k5_8", "driver_dna_k12_15", "driver_dna_k30_34"])
def test_driver_traces_without_text(monkeypatch, name):
    import II_assembleFromReads as drv
    real_oc = debruijn.output_contigs
    lazy_steps = []

    def forced_lazy(g, branch, pulled):  # non-final walks keep the index only; the final walk spells its contigs
        debruijn.MAX_CONTIG_CHARS = 1 if len(branch) else 0
        out = real_oc(g, branch, pulled)
        lazy_steps.append(isinstance(out, debruijn.LazyContigs))
        return out

    monkeypatch.setattr(debruijn, "output_contigs", forced_lazy)
    calls = _count_calls(monkeypatch)
    case = load_golden(name)
    inp = case["inputs"]
    _no_text(monkeypatch)  # the final walk exports its materialised contigs as a whole; no step asks for one contig's text
    final = _quiet(drv.assemble, list(inp["reads"]), inp["k_lowerlimit"], inp["k_upperlimit"], inp["threshold"])
    assert list(final) == case["result"]["final_contigs"]
    steps = inp["k_upperlimit"] - inp["k_lowerlimit"]
    assert lazy_steps[:-1] == [True] * steps and len(calls) == steps


def test_refusals_leave_every_handle_usable():
    reads = synth.reads_list(51, 5000, 1500, 100, 0.01)
    res21 = _quiet(debruijn.construct_graph, reads, 21, threshold=2)
    lazy21 = _quiet(debruijn.output_contigs, res21[0], res21[2], res21[3])
    res25 = _quiet(debruijn.construct_graph, reads, 25, threshold=2)
    lazy25 = _quiet(debruijn.output_contigs, res25[0], res25[2], res25[3])
    a, b = lazy21._graph, lazy25._graph
    na, nb = len(lazy21._order), len(lazy25._order)
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    dst = _dbg.Graph()
    good = [(b, np.arange(nb)), (a, np.arange(na)[::2])]
    dst.build_from_walks(26, good, *empty)
    size0 = dst.sizes()

    def refused(k1, blocks, match, handle=dst):
        with pytest.raises(_dbg.DbgError, match=match) as e:
            handle.build_from_walks(k1, blocks, *empty)
        assert e.value.code == _dbg.DBG_E_ARG

    refused(26, [(a, [0]), (b, [0]), (a, [1])], "two blocks")
    refused(26, [(a, [0]), (dst, [0])], "different handles")
    refused(25, good, "larger than the k")                       # k(src) == k1
    refused(21, good, "larger than the k")
    refused(64, good, "63")
    refused(26, [(a, [na])], "out of range")
    refused(26, [(b, [0, 1, 0])], "twice")
    assert dst.sizes() == size0                                  # a refusal leaves dst's graph alone
    fresh = _dbg.Graph()
    fresh.set_reads(*_pack(reads))
    fresh.build(21)
    refused(26, [(fresh, [])], "walk")                           # no walk of its current graph
    parts = _dbg.Graph()
    parts.set_reads(*_pack(reads))
    parts.build_multipass(21, 2)
    refused(26, [(parts, [])], "parts")                          # a graph in parts (it cannot be walked as one graph)
    fin = _walked(reads, 21, 2)
    fin.walk(True, 0)
    refused(26, [(fin, [])], "final")
    pep = load_golden("driver_peptide_k10_14")["inputs"]
    rp = _quiet(debruijn.construct_graph, list(pep["reads"]), pep["k_lowerlimit"], threshold=pep["threshold"])
    lp = _quiet(debruijn.output_contigs, rp[0], rp[2], rp[3])
    refused(26, [(lp._graph, [])], "ACGT")
    import torch
    if torch.cuda.device_count() > 1:
        refused(26, good, "same device", handle=_dbg.Graph(device=1))
    with pytest.raises(_dbg.AlphabetError):
        dst.build_from_walks(26, good, *_pack(["ACGTNACGT" * 5]))
    assert lazy21[0] and lazy25[0] and lp[0]                     # the sources still answer
    dst.build_from_walks(26, good, *empty)                       # and a correct call on the same dst succeeds
    assert dst.sizes() == size0
