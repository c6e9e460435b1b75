"""Host side of the batched contig output (CPU only): slices, iteration, ``packed()`` and ``write_fasta`` of a lineage of
three graphs fetch their texts with one batched call per block and batch and none per contig, return exactly what the
per-contig path returns, and stand-in handles without the batched calls behave as before.  The device handles are
stand-ins, as in test_lazy_tail_views.py."""
import numpy as np

import debruijn as prod


class Handle:
    """Stand-in for _dbg.Graph that offers only the per-contig call."""

    def __init__(self, k, texts, bits=2):
        self.k, self.texts, self.bits = k, [t.encode() for t in texts], bits
        self.generation, self.walks = 1, 1
        self.fetched, self.batches, self.writes = [], [], []

    def export_contig_text(self, index, length):
        assert length == len(self.texts[index])
        self.fetched.append(index)
        return self.texts[index]

    def alphabet(self):
        return (b"ACTG", 2) if self.bits == 2 else (b"ACDEFGHIKLMNPQRSTVWY", 5)

    def sizes(self):
        return {"k": self.k}


class BatchHandle(Handle):
    """... and one that also offers the batched calls, with a log of them."""

    def export_contig_texts(self, indices):
        idx = [int(i) for i in indices]
        self.batches.append(idx)
        chars = np.frombuffer(b"".join(self.texts[i] for i in idx), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(self.texts[i]) for i in idx])]).astype(np.uint64)
        return off, chars

    def write_contigs_fasta(self, path, indices=None, append=True, first_number=0, k_label=0, chunk_bytes=0):
        idx = [int(i) for i in indices]
        self.writes.append((idx, append, first_number, k_label))
        text = "".join(">SEQUENCE_{}_{}mer\n{}\n".format(first_number + j, k_label or self.k, self.texts[i].decode())
                       for j, i in enumerate(idx))
        with open(path, "ab" if append else "wb") as fh:
            fh.write(text.encode())
        return len(text)


def lazy_of(handle, order):
    lens = np.array([len(t) for t in handle.texts], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    lazy = prod.LazyContigs(handle, np.asarray(order), off, np.arange(len(lens), dtype=np.uint64))
    lazy._final, lazy._generation, lazy._walk = False, handle.generation, handle.walks
    return lazy


def lineage(cls):
    """The reads of a step at k = 8 (test_lazy_tail_views.lineage): main part on h7, blocks of h6 and h5, then a string."""
    h5 = cls(5, ["AAAAAC", "CCCCCA", "GGGGGT", "TTTTTA"])
    h6 = cls(6, ["ACACACA", "CGCGCGC", "GTGTGTG"])
    h7 = cls(7, ["ACGTACGT", "TTGGCCAA", "GATTACAG", "CATCATCA"])
    l5 = lazy_of(h5, [3, 1, 0, 2])
    l5.extend(["AC", "GT"])
    l6 = lazy_of(h6, [2, 0, 1])
    l6.extend(prod._PulledReads(l5, [1, 2, 5]))
    l7 = lazy_of(h7, [1, 3, 0, 2])
    l7.extend(prod._PulledReads(l6, [0, 2, 3, 5]))
    return (h5, h6, h7), l7


WANT = ["TTGGCCAA", "CATCATCA", "ACGTACGT", "GATTACAG", "GTGTGTG", "CGCGCGC", "CCCCCA", "GT"]


def _clear(hs):
    for h in hs:
        h.fetched.clear(), h.batches.clear(), h.writes.clear()


def _per_contig(fn):
    """What the same expression gives on handles that have only the per-contig call."""
    hs, l7 = lineage(Handle)
    out = fn(l7)
    assert not any(h.batches or h.writes for h in hs)
    return out


def test_iteration_and_slices_fetch_one_batch_per_block():
    hs, l7 = lineage(BatchHandle)
    h5, h6, h7 = hs
    assert not any(h.fetched or h.batches for h in hs)            # building the lineage moved no text
    assert list(l7) == WANT == _per_contig(list)
    assert (h7.batches, h6.batches, h5.batches) == ([[1, 3, 0, 2]], [[2, 1]], [[1]])
    assert not any(h.fetched for h in hs)
    for sl in (slice(3, 7), slice(None, None, 3), slice(None, None, -1), slice(5, 1, -2), slice(6, None), slice(2, 2)):
        _clear(hs)
        assert l7[sl] == WANT[sl] == _per_contig(lambda l: l[sl])
        assert not any(h.fetched for h in hs) and all(len(h.batches) <= 1 for h in hs)
    _clear(hs)
    assert l7[3:7] == WANT[3:7] and (h7.batches, h6.batches, h5.batches) == ([[2]], [[2, 1]], [[1]])
    # the blocks themselves, and the pull-out reads of the next step
    _clear(hs)
    block = l7._tail[0]
    assert list(block) == block[:] == ["GTGTGTG", "CGCGCGC"] and block[::-1] == ["CGCGCGC", "GTGTGTG"]
    assert h6.batches == [[2, 1], [2, 1], [1, 2]] and not h6.fetched
    p8 = prod._PulledReads(l7, [1, 2, 4, 6, 7])
    _clear(hs)
    assert list(p8) == ["CATCATCA", "ACGTACGT", "GTGTGTG", "CCCCCA", "GT"]
    assert (h7.batches, h6.batches, h5.batches) == ([[3, 0]], [[2]], [[1]]) and not any(h.fetched for h in hs)


def test_integer_indexing_stays_one_contig_per_call():
    hs, l7 = lineage(BatchHandle)
    h5, h6, h7 = hs
    assert l7[5] == "CGCGCGC" and h6.fetched == [1] and not h6.batches
    assert l7[0] == "TTGGCCAA" and l7[-2] == "CCCCCA" and h7.fetched == [1] and h5.fetched == [1]
    assert not any(h.batches for h in hs)


def test_batches_are_bounded(monkeypatch):
    hs, l7 = lineage(BatchHandle)
    h5, h6, h7 = hs
    monkeypatch.setattr(prod, "BATCH_CHARS", 16)                   # two contigs of 8 characters per batch
    assert list(l7) == WANT
    assert h7.batches == [[1, 3], [0, 2]] and h6.batches == [[2, 1]] and h5.batches == [[1]]
    _clear(hs)
    monkeypatch.setattr(prod, "BATCH_CHARS", 3)                    # smaller than a contig: one contig per batch, never none
    assert list(l7) == WANT and h7.batches == [[1], [3], [0], [2]]
    assert [(s.start, s.stop) for s in prod._batches([5, 5, 5, 1, 20, 1], 10)] == [(0, 2), (2, 4), (4, 5), (5, 6)]
    assert list(prod._batches([], 10)) == []


def test_packed_is_the_whole_sequence_without_strings():
    hs, l7 = lineage(BatchHandle)
    l7.extend(["ACGT", ""])
    want = WANT + ["ACGT", ""]
    chars, off = l7.packed()
    assert chars.dtype == np.uint8 and off.dtype == np.uint64 and len(off) == len(want) + 1
    assert chars.tobytes().decode() == "".join(want) and off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in want])]).tolist()
    assert [len(h.batches) for h in hs] == [1, 1, 1] and not any(h.fetched for h in hs)
    # _pack_reads takes that way for a LazyContigs, and gives what it gives for the spelled-out list
    _clear(hs)
    c2, o2 = prod._pack_reads(l7)
    c3, o3 = prod._pack_reads(want)
    assert np.array_equal(c2, c3) and np.array_equal(o2, o3) and not any(h.fetched for h in hs)
    # the per-contig stand-ins: the same arrays
    hs1, l1 = lineage(Handle)
    l1.extend(["ACGT", ""])
    c1, o1 = l1.packed()
    assert np.array_equal(c1, chars) and np.array_equal(o1, off) and sum(len(h.fetched) for h in hs1) == 7
    empty = lazy_of(BatchHandle(7, []), np.zeros(0, np.int64))
    c0, o0 = empty.packed()
    assert c0.size == 0 and o0.tolist() == [0]


def test_a_walk_that_is_gone_is_noticed():
    hs, l7 = lineage(BatchHandle)
    hs[2].texts[3] = b"CATCATCAT"  # the handle walked again: another contig at that index
    try:
        list(l7)
    except RuntimeError as e:
        assert "gone" in str(e)
    else:
        raise AssertionError("a changed contig length went unnoticed")


def test_write_fasta_numbers_across_blocks(tmp_path):
    def reference(seq, k):
        return "".join(">SEQUENCE_{}_{}mer\n{}\n".format(i, k, seq[i]) for i in range(len(seq)))

    hs, l7 = lineage(BatchHandle)
    h5, h6, h7 = hs
    l7.extend(["ACGT"])
    l7.extend(prod._PulledReads(lazy_of(BatchHandle(4, ["ACGTA", "TTTTT"]), [1, 0]), [0, 1]))
    h4 = l7._tail[-1]._graph
    want = WANT + ["ACGT", "TTTTT", "ACGTA"]
    path = tmp_path / "out.fasta"
    path.write_text("kept\n")
    l7.write_fasta(str(path), 12)
    assert path.read_text() == "kept\n" + reference(want, 12)       # appended; every record carries the driver's k
    assert h7.writes == [([1, 3, 0, 2], True, 0, 12)] and h6.writes == [([2, 1], True, 4, 12)]
    assert h5.writes == [([1], True, 6, 12)] and h4.writes == [([1, 0], True, 9, 12)]  # "GT" and "ACGT" came from the host
    assert not any(h.fetched or h.batches for h in (h4, h5, h6, h7))
    l7.write_fasta(str(path), 8, append=False)
    assert path.read_text() == reference(want, 8)
    # stand-ins without the writer: the host formats, the file is the same
    hs1, l1 = lineage(Handle)
    l1.extend(["ACGT"])
    p1 = tmp_path / "host.fasta"
    l1.write_fasta(str(p1), 8)
    assert p1.read_text() == reference(WANT + ["ACGT"], 8) and sum(len(h.fetched) for h in hs1) == 7
    # nothing to write: the file exists and is empty
    p0 = tmp_path / "empty.fasta"
    lazy_of(BatchHandle(7, []), np.zeros(0, np.int64)).write_fasta(str(p0), 8)
    assert p0.read_text() == ""


def test_write_fasta_refuses_a_walk_that_is_gone(tmp_path):
    import pytest
    for stale in ("walks", "generation"):
        hs, l7 = lineage(BatchHandle)
        setattr(hs[1], stale, getattr(hs[1], stale) + 1)  # h6 walked / built again after its block was made
        path = tmp_path / (stale + ".fasta")
        with pytest.raises(RuntimeError, match="gone"):
            l7.write_fasta(str(path), 8)
        assert not hs[1].writes and not hs[0].writes  # nothing of the stale block or behind it was written
