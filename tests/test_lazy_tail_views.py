"""Host logic of the driver's lineage (CPU only): LazyContigs with blocks of pulled contigs in its tail, _PulledReads that
keeps contigs as references, and the test that decides whether construct_graph may build from the chains.  The device
handle is a stand-in, as in test_host_views.py."""
import numpy as np

import debruijn as prod


class Handle:
    """Stand-in for _dbg.Graph: contig texts by index, the state construct_graph looks at, and a log of text exports."""

    def __init__(self, k, texts, bits=2):
        self.k, self.texts, self.bits = k, [t.encode() for t in texts], bits
        self.generation, self.walks = 1, 1
        self.fetched = []

    def export_contig_text(self, index, length):
        assert length == len(self.texts[index])
        self.fetched.append(index)
        return self.texts[index]

    def alphabet(self):
        return (b"ACTG", 2) if self.bits == 2 else (b"ACDEFGHIKLMNPQRSTVWY", 5)

    def sizes(self):
        return {"k": self.k}


def lazy_of(handle, order):
    lens = np.array([len(t) for t in handle.texts], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    lazy = prod.LazyContigs(handle, np.asarray(order), off, np.arange(len(lens), dtype=np.uint64))
    lazy._final, lazy._generation, lazy._walk = False, handle.generation, handle.walks
    return lazy


def lineage():
    """reads of a step at k = 8: main part on h7, blocks of h6 and h5 in the tail, then two strings."""
    h5 = Handle(5, ["AAAAAC", "CCCCCA", "GGGGGT", "TTTTTA"])
    h6 = Handle(6, ["ACACACA", "CGCGCGC", "GTGTGTG"])
    h7 = Handle(7, ["ACGTACGT", "TTGGCCAA", "GATTACAG", "CATCATCA"])
    l5 = lazy_of(h5, [3, 1, 0, 2])
    l5.extend(["AC", "GT"])
    p6 = prod._PulledReads(l5, [1, 2, 5])          # contigs 1, 0 of h5 and the read "GT"
    l6 = lazy_of(h6, [2, 0, 1])
    l6.extend(p6)
    p7 = prod._PulledReads(l6, [0, 2, 3, 5])       # contigs 2, 1 of h6, contig 1 of h5, "GT"
    l7 = lazy_of(h7, [1, 3, 0, 2])
    l7.extend(p7)
    return (h5, h6, h7), l7


def test_extend_with_pulled_reads_moves_no_text():
    (h5, h6, h7), l7 = lineage()
    assert not (h5.fetched or h6.fetched or h7.fetched)
    assert len(l7) == 4 + 2 + 1 + 1
    blocks = [t for t in l7._tail if type(t) is prod._ContigBlock]
    assert [(b._graph, b._idx.tolist(), b.lengths.tolist()) for b in blocks] == [(h6, [2, 1], [7, 7]), (h5, [1], [6])]
    assert l7._tail[-1] == "GT" and not (h5.fetched or h6.fetched or h7.fetched)


def test_order_len_indexing_slices_and_iteration():
    (h5, h6, h7), l7 = lineage()
    want = ["TTGGCCAA", "CATCATCA", "ACGTACGT", "GATTACAG", "GTGTGTG", "CGCGCGC", "CCCCCA", "GT"]
    assert list(l7) == want and [l7[i] for i in range(len(l7))] == want and len(l7) == len(want)
    assert l7[-1] == "GT" and l7[-2] == "CCCCCA" and l7[3:7] == want[3:7] and l7[::3] == want[::3]
    assert "CGCGCGC" in l7 and "AAAAAC" not in l7
    h6.fetched.clear()
    assert l7[5] == "CGCGCGC" and h6.fetched == [1]   # fetched on demand, from the graph that holds it
    l7.extend(["ACGT"])
    assert l7[len(want)] == "ACGT" and len(l7) == len(want) + 1
    # the pull-out reads of the next step: references grouped by source, strings last
    p8 = prod._PulledReads(l7, [1, 2, 4, 6, 7, 8])
    h5.fetched.clear(); h6.fetched.clear(); h7.fetched.clear()
    assert len(p8) == 6 and not (h5.fetched or h6.fetched or h7.fetched)
    assert [(type(p) is prod._ContigBlock, len(p)) for p in p8._parts] == [(True, 2), (True, 1), (True, 1), (False, 2)]
    assert [p._graph for p in p8._parts[:3]] == [h7, h6, h5]
    assert list(p8) == ["CATCATCA", "ACGTACGT", "GTGTGTG", "CCCCCA", "GT", "ACGT"] and p8 == list(p8)
    assert p8[-1] == "ACGT" and p8[1:3] == ["ACGTACGT", "GTGTGTG"]


def test_eligibility_of_a_tail():
    (h5, h6, h7), l7 = lineage()
    src = prod._walk_source(l7, 8)
    assert src is not None
    g, blocks, strings = src
    assert g is h7 and [(b, i.tolist()) for b, i in blocks] == [(h6, [2, 1]), (h5, [1])] and strings == ["GT"]
    assert prod._walk_source(l7, 9) is None               # the main part is not at k - 1
    # a string between blocks
    (h5, h6, h7), l7 = lineage()
    l7.extend(["ACGT"])
    l7.extend(prod._PulledReads(lazy_of(Handle(4, ["ACGTA"]), [0]), [0]))
    assert type(l7._tail[-1]) is prod._ContigBlock and prod._walk_source(l7, 8) is None
    assert list(l7)[-2:] == ["ACGT", "ACGTA"]               # still a sequence of strings for the text path
    # a stale graph, a graph named twice, a generic alphabet, a block at k - 1 or above
    (h5, h6, h7), l7 = lineage()
    h6.walks += 1
    assert prod._walk_source(l7, 8) is None
    (h5, h6, h7), l7 = lineage()
    h5.generation += 1
    assert prod._walk_source(l7, 8) is None
    (h5, h6, h7), l7 = lineage()
    l7._tail[1]._graph = h6
    assert prod._walk_source(l7, 8) is None
    (h5, h6, h7), l7 = lineage()
    h5.bits = 5
    assert prod._walk_source(l7, 8) is None
    (h5, h6, h7), l7 = lineage()
    h6.k = 8
    assert prod._walk_source(l7, 8) is None
    assert not (h5.fetched or h6.fetched or h7.fetched)
