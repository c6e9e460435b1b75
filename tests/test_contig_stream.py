"""Contig text streamed off the device: batched texts (dbg_export_contig_texts) and the FASTA writer
(dbg_write_contigs_fasta) on materialised and index-only walks, against the same graph's chain walk (one thread per start
spells its contig: none of the code under test) and the host's formatting of those texts, through the binding,
debruijn.py and the driver.  The materialised list-ranking walk and export_sorted_fasta, which spell their text with the
same window kernel, and the one-contig call (one thread per character, the same descent) are held to the same reference.

Input H: synth.reads_list(82, 10000, 8000, 60, 0.03), k = 11, threshold 1 -- 2 111 contigs of 11 .. 2 632 characters, so the
record numbers cross 9 -> 10, 99 -> 100 and 999 -> 1000, records are shorter than a thread's run and contigs longer than
half a tile.  Input I: synth.reads_list(83, 30000, 4000, 100, 0.01), threshold 2, at k = 31 (a contig of 5 073 characters:
longer than a tile), 40 and 63 (two key words)."""
import contextlib
import io
import os

import numpy as np
import pytest

import _dbg
import debruijn
import synth
from conftest import case_reads, load_golden

pytestmark = pytest.mark.gpu

MIB = 1 << 20
DEFAULT_CHUNK = 4 * MIB  # the library's window size where a call names none
FIELDS = ("keyword", "number", "underscore", "k digits", "mer", "text", "newline")


@pytest.fixture(autouse=True)
def _jump_walks(monkeypatch):
    """Index-only walks need the list-ranking walk, which small graphs take only below this node count."""
    monkeypatch.setenv("DBG_WALK_JUMP_MIN", "1")


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _chain_walk(g):
    """The reference of this file: a materialised non-final walk in which one thread per start spells its chain character by
    character (k_walk_chain) -- no lifting table, no window kernel, no record layout
    -> (the text of every contig by index, scores, start stamps, emission indices inside the start)."""
    g.set_option("walk_jump_min_nodes", 1 << 40)
    try:
        g.walk(False, 0)
        assert g.sizes()["contigs_materialised"] == 1
        off, chars, score, stamp, seq = g.export_contigs()
    finally:
        g.set_option("walk_jump_min_nodes", 1)
    text, o = chars.tobytes(), off.tolist()
    return [text[o[i]:o[i + 1]] for i in range(len(score))], score, stamp, seq


def _driver_order(score, stamp, seq):
    """Contig indices in the driver's order: the emission order (start stamp, index inside the start), sorted by score,
    descending and stable."""
    emission = np.lexsort((seq, stamp))
    return emission[np.argsort(-score[emission].astype(np.int64), kind="stable")]


class Walked:
    """A graph, and what its chain walk (_chain_walk) gave: the text of every contig under (start stamp, emission index
    inside the start) -- contig indices belong to one walk --, the texts in the driver's order and their FASTA as the host
    formats it.  The materialised list-ranking walk and export_sorted_fasta are checked against those here, once."""

    def __init__(self, reads, k, thr):
        old = os.environ.get("DBG_WALK_JUMP_MIN")
        os.environ["DBG_WALK_JUMP_MIN"] = "1"  # the handle reads it when it is made
        try:
            self.res = _quiet(debruijn.construct_graph, list(reads), k, threshold=thr, final=False)
        finally:
            if old is None:
                del os.environ["DBG_WALK_JUMP_MIN"]
            else:
                os.environ["DBG_WALK_JUMP_MIN"] = old
        self.k, self.g = k, self.res[0][0]._graph
        texts, score, stamp, seq = _chain_walk(self.g)
        self.by_key = {(int(stamp[i]), int(seq[i])): texts[i] for i in range(len(score))}
        self.n = len(score)
        self.sorted_texts = [texts[i] for i in _driver_order(score, stamp, seq).tolist()]
        self.fasta = _fasta(self.sorted_texts, 0, k)
        self.lengths = np.array([len(t) for t in texts], dtype=np.int64)
        # the materialised list-ranking walk spells the same contigs, and its sorted FASTA is the host's
        self.g.walk(False, 0)
        assert self.g.sizes()["contigs_materialised"] == 1
        off, chars, score, stamp, seq = self.g.export_contigs()
        text, o = chars.tobytes(), off.tolist()
        assert len(score) == self.n
        for i in range(self.n):
            assert text[o[i]:o[i + 1]] == self.by_key[(int(stamp[i]), int(seq[i]))], i
        fasta, order = self.g.export_sorted_fasta()
        assert fasta == self.fasta
        assert order.tolist() == _driver_order(score, stamp, seq).tolist()

    def walk(self, materialised):
        """Walks again in the asked state -> (the texts by contig index of THIS walk, its emission order)."""
        self.g.walk(False, 0 if materialised else 16)
        assert self.g.sizes()["contigs_materialised"] == (1 if materialised else 0)
        off, score, stamp, seq = self.g.export_contig_index()
        texts = [self.by_key[(int(stamp[i]), int(seq[i]))] for i in range(self.n)]
        assert [len(t) for t in texts] == np.diff(off.astype(np.int64)).tolist()
        return texts, np.lexsort((seq, stamp))


@pytest.fixture(scope="module")
def H():
    w = Walked(synth.reads_list(82, 10000, 8000, 60, 0.03), 11, 1)
    # the input must keep its shape: a change of synth cannot hollow the cases out
    assert w.n >= 1001 and int(w.lengths.min()) == w.k and int(w.lengths.max()) > 2048
    yield w
    w.g.close()


@pytest.fixture(scope="module")
def I_reads():
    return synth.reads_list(83, 30000, 4000, 100, 0.01)


@pytest.fixture(scope="module")
def I31(I_reads):
    w = Walked(I_reads, 31, 2)
    assert int(w.lengths.max()) > 4096  # a contig longer than a tile
    yield w
    w.g.close()


def _fasta(texts, first=0, k=0):
    return b"".join(b">SEQUENCE_%d_%dmer\n%s\n" % (first + i, k, t) for i, t in enumerate(texts))


def _sizes_only(g, idx):
    """The first call of the two-call pattern, by hand."""
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    off = np.full(idx.size + 1, 77, dtype=np.uint64)
    total = _dbg.C.c_uint64(77)
    g._chk(g._lib.dbg_export_contig_texts(g._h, _dbg._ptr(idx) if idx.size else None, idx.size, _dbg._ptr(off), None, 0,
                                          _dbg.C.byref(total)))
    return off, total.value


def _check_batched(w, chunk):
    rng = np.random.default_rng(5)
    w.g.set_option("ctgout_chunk_bytes", chunk)  # the window size of calls that name none
    for materialised in (True, False):
        texts, _ = w.walk(materialised)
        shortest = int(np.argmin([len(t) for t in texts]))
        lists = {"ascending": np.arange(w.n), "permutation": rng.permutation(w.n),
                 "repeats": rng.integers(0, w.n, size=w.n // 2 + 3), "shortest": np.array([shortest]),
                 "one twice": np.array([shortest, shortest]), "empty": np.zeros(0, dtype=np.int64)}
        for name, idx in lists.items():
            off, chars = w.g.export_contig_texts(idx)
            want = [texts[i] for i in idx.tolist()]
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in want], dtype=np.int64)]).tolist(), name
            assert chars.tobytes() == b"".join(want), (name, materialised)
            off0, total0 = _sizes_only(w.g, idx)
            assert np.array_equal(off0, off) and total0 == chars.size, name
        st = w.g.contig_output_stats()  # of the last call that moved text: "one twice"
        assert st["bytes_written"] == 2 * len(texts[shortest]) and st["chunks"] == 1
        assert st["chunk_bytes"] == (chunk or DEFAULT_CHUNK)
        assert (st["lift_bytes"] > 0) == (not materialised)
    w.g.set_option("ctgout_chunk_bytes", 0)


def test_batched_texts_on_H(H):
    _check_batched(H, 0)


def test_batched_texts_on_H_with_borders_inside_contigs(H):
    """chunk 4096: the ascending list is 447 windows, nearly every border inside a contig."""
    assert int(H.lengths.sum()) // 4096 >= 400
    _check_batched(H, 4096)
    H.walk(False)
    H.g.set_option("ctgout_chunk_bytes", 4096)
    off, chars = H.g.export_contig_texts(np.arange(H.n))
    assert H.g.contig_output_stats()["chunks"] == -(-chars.size // 4096)
    H.g.set_option("ctgout_chunk_bytes", 0)


def test_batched_texts_on_I31(I31):
    _check_batched(I31, 0)


@pytest.mark.parametrize("k", [40, 63])
def test_batched_texts_with_two_key_words(I_reads, k):
    w = Walked(I_reads, k, 2)
    assert w.n > 100 and int(w.lengths.min()) == k  # characters j < k of such a contig come from both key words
    _check_batched(w, 0)
    w.g.close()


def _cut_kinds(texts, first, k_label, chunk):
    """How often a window border falls in each kind of field of the records -- strictly inside it where the field is longer
    than a byte, so that the field is written by two windows."""
    kinds = dict.fromkeys(FIELDS, 0)
    at, nxt = 0, chunk
    for i, t in enumerate(texts):
        for name, part in zip(FIELDS, (b">SEQUENCE_", b"%d" % (first + i), b"_", b"%d" % k_label, b"mer\n", t, b"\n")):
            lo, hi = at, at + len(part)
            while nxt < lo:
                nxt += chunk
            for b in range(nxt, hi, chunk):
                if lo < b or (len(part) == 1 and b == lo):
                    kinds[name] += 1
            at = hi
    return kinds


def test_writer_against_host_formatting(H, tmp_path):
    """From the index-only walk: all contigs in the driver's order (indices None, and LazyContigs' own sorted order), at
    three window sizes; a first number and k label of the caller's; lists in other orders.  Each of the two files written
    in a permuted order has, by itself, a 4096-byte window border in every kind of field of a record (a condition on the
    input, checked before comparing; the permutations were searched for with the CPU oracle -- the driver's order cuts
    every kind but the k digits)."""
    texts, emission = H.walk(False)
    path = str(tmp_path / "out.fasta")
    off, score, stamp, seq = H.g.export_contig_index()
    lazy = debruijn.LazyContigs(H.g, np.lexsort((seq, stamp)), off, score)
    lazy.sort(reverse=True)
    assert [texts[i] for i in lazy._order.tolist()] == H.sorted_texts and H.fasta == _fasta(H.sorted_texts, 0, H.k)
    perms = [np.random.default_rng(s).permutation(H.n) for s in (37, 63)]
    cases = [(None, 0, 0, H.sorted_texts), (lazy._order, 0, 0, H.sorted_texts), (lazy._order, 995, 12, H.sorted_texts)]
    cases += [(emission[p], 0, 0, [texts[i] for i in emission[p].tolist()]) for p in perms]
    for idx, first, k_label, want in cases:
        cut = _cut_kinds(want, first, k_label or H.k, 4096)
        print("fields cut by the 4096-byte windows:", cut)
        if idx is not None and idx is not lazy._order:
            assert all(cut[name] >= 1 for name in FIELDS), cut  # one file, every kind
    assert len(b"%d" % (995 + H.n - 1)) > len(b"%d" % 995)  # the number of digits changes inside the file
    for chunk in (4096, 8192, 0):
        for idx, first, k_label, want in cases:
            if chunk != 4096 and first == 0 and idx is not None and idx is not lazy._order:
                continue  # the other orders are there for the borders of the small windows
            n = H.g.write_contigs_fasta(path, idx, append=False, first_number=first, k_label=k_label, chunk_bytes=chunk)
            want_bytes = _fasta(want, first, k_label or H.k)
            with open(path, "rb") as fh:
                got = fh.read()
            assert n == len(got) == len(want_bytes) and got == want_bytes, (chunk, first, k_label)
            st = H.g.contig_output_stats()
            assert st["bytes_written"] == n and st["chunks"] == -(-n // (chunk or DEFAULT_CHUNK))
    # append keeps what is there and grows by bytes_written; append=False truncates
    with open(path, "wb") as fh:
        fh.write(b"kept\n")
    n = H.g.write_contigs_fasta(path, lazy._order[:7], first_number=3, chunk_bytes=4096)
    n2 = H.g.write_contigs_fasta(path, lazy._order[7:9], append=True, first_number=10)
    with open(path, "rb") as fh:
        got = fh.read()
    assert got == b"kept\n" + _fasta(H.sorted_texts[:9], 3, H.k) and len(got) == 5 + n + n2
    assert H.g.write_contigs_fasta(path, [], append=True) == 0 and os.path.getsize(path) == len(got)
    assert H.g.write_contigs_fasta(path, lazy._order[:1], append=False) == os.path.getsize(path) == len(_fasta(H.sorted_texts[:1], 0, H.k))
    assert H.g.write_contigs_fasta(path, [], append=False) == 0 and os.path.getsize(path) == 0
    # the materialised walk writes the same file
    H.walk(True)
    assert H.g.write_contigs_fasta(path, None, append=False, chunk_bytes=4096) == len(H.fasta)
    with open(path, "rb") as fh:
        assert fh.read() == H.fasta
    # export_sorted_fasta spells its text the same way and leaves the stats of the last streaming call alone
    st = H.g.contig_output_stats()
    assert H.g.export_sorted_fasta()[0] == H.fasta
    assert H.g.contig_output_stats() == st


def _off_of_index_only_walk(w):
    texts, _ = w.walk(False)
    return texts, w.g.export_contig_index()[0].astype(np.int64)


def test_one_contig_per_call_after_an_index_only_walk(H, I31):
    """dbg_export_contig_text for every contig of H -- its first character at every offset inside a 16-byte run of the
    walk's text, with and without a 4096-byte border inside it, so that the call may spell the contig as a piece of that
    text as well as by itself -- and for the contigs of I31 that are longer than 4096 characters."""
    texts, off = _off_of_index_only_walk(H)
    first, last = off[:-1], off[1:] - 1
    assert set((first % 16).tolist()) == set(range(16))
    assert np.any(first // 4096 != last // 4096) and np.any(first // 16 == last // 16)
    for i in range(H.n):
        assert H.g.export_contig_text(i, len(texts[i])) == texts[i], i
    texts, off = _off_of_index_only_walk(I31)
    longer = np.flatnonzero(np.diff(off) > 4096).tolist()
    assert longer
    for i in longer:
        assert I31.g.export_contig_text(i, len(texts[i])) == texts[i], i


def test_memory_bound_and_stats(I31, tmp_path):
    I31.walk(False)
    path = str(tmp_path / "i.fasta")
    n_bytes = I31.g.write_contigs_fasta(path, append=False)
    st = I31.g.contig_output_stats()
    print("stats of the default-chunk write:", st)
    chunk = st["chunk_bytes"]
    assert chunk == DEFAULT_CHUNK
    assert st["peak_device_bytes"] <= 2 * chunk + 24 * (I31.n + 1) + MIB
    assert st["bytes_written"] == n_bytes == os.path.getsize(path) and st["chunks"] == -(-n_bytes // chunk)
    assert st["lift_bytes"] > 0 and st["ms_total"] > 0 and st["ms_fill"] > 0 and st["ms_d2h"] > 0 and st["ms_io_wait"] >= 0
    with open(path, "rb") as fh:
        assert fh.read() == I31.fasta
    # small windows: the staging buffers are the two windows, the bound is tight
    n_bytes = I31.g.write_contigs_fasta(path, append=False, chunk_bytes=8192)
    st = I31.g.contig_output_stats()
    assert st["chunk_bytes"] == 8192 and st["chunks"] == -(-n_bytes // 8192)
    assert 2 * 8192 <= st["peak_device_bytes"] <= 2 * 8192 + 24 * (I31.n + 1) + MIB


def test_memory_bound_where_the_sort_scratch_dominates(tmp_path):
    """Every contig in the driver's order at 4096-byte windows, with so many contigs that 12 bytes per contig exceed the two
    windows and the MiB of the bound: a third copy of keys and ids in the sort's scratch would break it.  Reads: the first
    300 k of a 15 Mbp genome (the coverage of the measured 1 M-read input), about 1.8e5 contigs."""
    g = _dbg.Graph()
    g.synth_reads(1, 15_000_000, 300_000, 150, 0.01)
    g.build(31)
    g.refine_edge_order()
    g.prune(2)
    g.remove_tips()
    g.mark_pull_reads()
    texts, score, stamp, seq = _chain_walk(g)
    want = _fasta([texts[i] for i in _driver_order(score, stamp, seq).tolist()], 0, 31)
    g.walk(False, 16)
    sz = g.sizes()
    n, chunk = sz["n_contigs"], 4096
    assert sz["contigs_materialised"] == 0 and 12 * n > 2 * chunk + MIB
    path = str(tmp_path / "many.fasta")
    for c in (chunk, 0):
        n_bytes = g.write_contigs_fasta(path, None, append=False, chunk_bytes=c)
        st = g.contig_output_stats()
        print("contigs", n, "stats:", st)
        assert st["peak_device_bytes"] <= 2 * (c or DEFAULT_CHUNK) + 24 * (n + 1) + MIB
        assert st["bytes_written"] == n_bytes == len(want) and st["chunks"] == -(-n_bytes // (c or DEFAULT_CHUNK))
        with open(path, "rb") as fh:
            assert fh.read() == want
    g.close()


@pytest.mark.parametrize("k", [11, 12])
def test_generic_alphabet(k, tmp_path):
    """Peptides with packed 5-bit keys (k = 11) and with keys by reference into the reads (k = 12)."""
    pep = load_golden("driver_peptide_k10_14")["inputs"]
    w = Walked(list(pep["reads"]), k, pep["threshold"])
    assert w.n >= 1 and w.g.alphabet()[1] == 5
    assert bool(w.g.export_nodes(stamps=False, counts=False, flags=False)[0].any()) == (k <= 11)
    path = str(tmp_path / "pep.fasta")
    w.g.set_option("ctgout_chunk_bytes", 4096)
    for materialised in (True, False):
        texts, _ = w.walk(materialised)
        for idx in (np.arange(w.n), np.arange(w.n)[::-1], np.zeros(3, dtype=np.int64)):
            off, chars = w.g.export_contig_texts(idx)
            assert chars.tobytes() == b"".join(texts[i] for i in idx.tolist())
            assert np.diff(off.astype(np.int64)).tolist() == [len(texts[i]) for i in idx.tolist()]
        assert w.g.write_contigs_fasta(path, None, append=False, chunk_bytes=4096) == len(w.fasta)
        with open(path, "rb") as fh:
            assert fh.read() == w.fasta
    w.g.close()


def test_refusals_leave_the_handle_usable(H, tmp_path):
    texts, _ = H.walk(False)
    g, path = H.g, str(tmp_path / "r.fasta")

    def good():
        off, chars = g.export_contig_texts([1, 0])
        assert chars.tobytes() == texts[1] + texts[0]
        assert g.write_contigs_fasta(path, [2], append=False) == len(_fasta([texts[2]], 0, H.k))

    with pytest.raises(_dbg.DbgError, match="out of range"):
        g.export_contig_texts([0, H.n])
    good()
    with pytest.raises(_dbg.DbgError, match="out of range"):
        g.write_contigs_fasta(path, [H.n])
    good()
    # capacity one byte short: the capacity error, with n_chars set
    idx = np.array([3, 4], dtype=np.uint64)
    need = len(texts[3]) + len(texts[4])
    buf, total = np.zeros(need, dtype=np.uint8), _dbg.C.c_uint64()
    rc = g._lib.dbg_export_contig_texts(g._h, _dbg._ptr(idx), 2, None, _dbg._ptr(buf), need - 1, _dbg.C.byref(total))
    assert rc == _dbg.DBG_E_CAPACITY and total.value == need and not buf.any()
    rc = g._lib.dbg_export_contig_texts(g._h, _dbg._ptr(idx), 2, None, _dbg._ptr(buf), need, _dbg.C.byref(total))
    assert rc == _dbg.DBG_OK and buf.tobytes() == texts[3] + texts[4]
    missing = str(tmp_path / "no_such_dir" / "x.fasta")
    with pytest.raises(_dbg.DbgError, match="no_such_dir"):
        g.write_contigs_fasta(missing)
    good()
    with pytest.raises(_dbg.DbgError, match="1000"):
        g.write_contigs_fasta(path, chunk_bytes=1000)
    with pytest.raises(_dbg.DbgError):
        g.set_option("ctgout_chunk_bytes", 1000)
    good()
    # the calls that were there before behave as before on the same handle
    assert g.export_contig_text(5, len(texts[5])) == texts[5]
    with pytest.raises(_dbg.DbgError, match="not materialised"):
        g.export_sorted_fasta()
    H.walk(True)
    assert g.export_sorted_fasta()[0] == H.fasta


def test_refusals_without_a_walk_and_after_a_final_walk(tmp_path):
    path = str(tmp_path / "r.fasta")
    # no walk
    case = load_golden("dna_small_k40_e1_t3_final")
    reads, inp = case_reads(case), case["inputs"]
    res = _quiet(debruijn.construct_graph, list(reads), inp["k"], threshold=inp["threshold"], final=True)
    g = res[0][0]._graph
    with pytest.raises(_dbg.DbgError, match="dbg_walk must run first"):
        g.export_contig_texts([0])
    with pytest.raises(_dbg.DbgError, match="dbg_walk must run first"):
        g.write_contigs_fasta(path)
    # a final-mode walk over a graph with branch nodes (all simple paths) whose text exceeds max_chars keeps no index and
    # no start nodes
    assert g.sizes()["n_branch"] > 0
    with pytest.raises(_dbg.DbgError, match="max_chars"):
        g.walk(True, 16)
    with pytest.raises(_dbg.DbgError, match="no per-contig start nodes"):
        g.export_contig_texts([0])
    with pytest.raises(_dbg.DbgError, match="no per-contig start nodes"):
        g.write_contigs_fasta(path)
    with pytest.raises(_dbg.DbgError, match="dbg_walk must run first"):
        g.export_contig_text(0, 100)  # as before
    # the same walk with room for its text: both calls answer
    g.walk(True, 0)
    off, chars, score, stamp, seq = g.export_contigs()
    fasta, order = g.export_sorted_fasta()
    off2, chars2 = g.export_contig_texts(np.arange(len(score)))
    assert np.array_equal(off2, off) and np.array_equal(chars2, chars)
    assert g.write_contigs_fasta(path, append=False, chunk_bytes=4096) == len(fasta)
    with open(path, "rb") as fh:
        assert fh.read() == fasta
    g.close()


def _refuse_per_contig_calls(m):
    m.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("one contig per call")))


def test_driver_streams_its_last_step(monkeypatch, tmp_path):
    """Error-free reads: the final walk takes the chain path and keeps its index only; the driver writes the same file as
    with the text on the device, without one per-contig call."""
    import II_assembleFromReads as drv
    reads = synth.reads_list(73, 20000, 3000, 100, 0.0)
    want_path, got_path = str(tmp_path / "want.fasta"), str(tmp_path / "got.fasta")
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 0)
    out0 = io.StringIO()
    with contextlib.redirect_stdout(out0):
        want_seq = drv.assemble(list(reads), 21, 22, 2, want_path)
    with open(got_path, "w") as fh:
        fh.write("earlier run\n")  # the driver appends
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    out1 = io.StringIO()
    with monkeypatch.context() as m, contextlib.redirect_stdout(out1):
        _refuse_per_contig_calls(m)
        got_seq = drv.assemble(list(reads), 21, 22, 2, got_path)
        assert isinstance(got_seq, debruijn.LazyContigs) and got_seq._graph.sizes()["contigs_materialised"] == 0
    with open(want_path, "rb") as fh:
        want = fh.read()
    with open(got_path, "rb") as fh:
        got = fh.read()
    assert want.count(b">") == len(want_seq) >= 1 and max(map(len, want_seq)) > 4096  # a record longer than a tile
    assert got == b"earlier run\n" + want
    assert out1.getvalue() == out0.getvalue()
    assert list(got_seq) == list(want_seq)


def test_text_path_on_lazy_reads_makes_no_per_contig_call(monkeypatch):
    """Peptides cannot be built from chains: construct_graph at k + 1 on the lazy contigs and the pull-out reads of a
    forced-lazy step takes the text path -- one batched export per block."""
    pep = load_golden("driver_peptide_k10_14")["inputs"]
    k, thr = pep["k_lowerlimit"], pep["threshold"]
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    g, pull, branch, pulled, _ = _quiet(debruijn.construct_graph, list(pep["reads"]), k, threshold=thr)
    lazy = _quiet(debruijn.output_contigs, g, branch, pulled)
    assert isinstance(lazy, debruijn.LazyContigs) and len(lazy) >= 1
    lazy.sort(reverse=True)
    spelled = [lazy[i] for i in range(len(lazy))] + list(pull)  # one contig per call: the path that was there before
    lazy.extend(pull)
    want = _quiet(debruijn.construct_graph, spelled, k + 1, threshold=thr)
    calls = []
    real = _dbg.Graph.export_contig_texts
    with monkeypatch.context() as m:
        _refuse_per_contig_calls(m)
        m.setattr(_dbg.Graph, "export_contig_texts", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
        assert list(lazy) == spelled and lazy[:] == spelled
        n_before = len(calls)
        got = _quiet(debruijn.construct_graph, lazy, k + 1, threshold=thr)
        assert len(calls) - n_before >= 1

    def view(res):
        (V, E), pull_, branch_, pulled_, ect = res
        contigs = _quiet(debruijn.output_contigs, (V, E), branch_, pulled_)
        return ([(v, n.indegree, n.outdegree) for v, n in V.items()], {v: list(s) for v, s in E.items()}, list(ect.items()),
                list(branch_), list(pulled_), list(pull_), list(contigs), list(contigs.scores))

    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 0)
    assert view(got) == view(want)
