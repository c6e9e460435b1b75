"""Reads cut at the bytes that are not bases (dbg_split_reads, csrc/dbg_readsplit.h): the definition

    pieces(reads, fold) = [m for r in reads for m in re.findall(b"[ACGT]+", fold_acgt(r) if fold else r)]

against the device pass on hand cases, on inputs built for every granularity the kernels name (word, block, two blocks,
the round of the carry kernel) and on random sets; the calls that must leave the read set alone; the graph, the graph in
parts and the sharded graph of a split read set against those of the explicit pieces; the FASTA routes and the driver.

The kernels have no scan level beyond the round of the carry kernel (16 MiB: it loops over the rounds with the carry in
a register), so no border here needs more than a few rounds of input to cross."""
import contextlib
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

import _dbg
import debruijn as prod
import synth

W, B, R = _dbg.SPLIT_WORD_BYTES, _dbg.SPLIT_BLOCK_BYTES, _dbg.SPLIT_ROUND_BYTES
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
STATS = ("n_reads_in", "n_bytes_in", "n_reads_out", "n_bytes_out", "n_cut_bytes", "n_folded_bytes", "n_reads_changed",
         "n_reads_emptied", "changed")


# ---- the definition, twice: the regex of the issue and a numpy statement of the per-byte rule ---------------------------
def regex_pieces(reads, fold):
    tr = bytes.maketrans(b"acgt", b"ACGT")
    return [m for r in reads for m in re.findall(b"[ACGT]+", r.translate(tr) if fold else r)]


def pack(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def unpack(bases, off):
    raw = bases.tobytes()
    return [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def numpy_split(bases, off, fold):
    """-> dict(bases, offsets, read_index, pos, + every stats field) from the per-byte rule of the issue"""
    off = off.astype(np.int64)
    n, n_reads = bases.size, off.size - 1
    b = bases.copy()
    if fold:
        low = np.isin(b, np.frombuffer(b"acgt", dtype=np.uint8))
        b[low] -= 32
    keep = np.isin(b, ACGT)
    lens = np.diff(off)
    rs = np.zeros(n + 1, dtype=bool)
    rs[off[:-1][lens > 0]] = True
    prev = np.concatenate([[False], keep[:-1]]) if n else keep
    start = keep & (~prev | rs[:n])
    dst = np.cumsum(keep) - keep
    p = np.flatnonzero(start)
    rd = np.searchsorted(off, p, side="right") - 1
    ck = np.concatenate([[0], np.cumsum(keep)])
    kept_per_read = ck[off[1:]] - ck[off[:-1]]
    folded = int((keep & (b != bases)).sum())
    out = {"bases": b[keep], "offsets": np.concatenate([dst[p], [int(keep.sum())]]).astype(np.uint64),
           "read_index": rd.astype(np.uint64), "pos": (p - off[rd]).astype(np.uint64),
           "n_reads_in": n_reads, "n_bytes_in": n, "n_reads_out": p.size, "n_bytes_out": int(keep.sum()),
           "n_cut_bytes": n - int(keep.sum()), "n_folded_bytes": folded,
           "n_reads_changed": int((kept_per_read < lens).sum()), "n_reads_emptied": int((kept_per_read == 0).sum())}
    out["changed"] = int(out["n_cut_bytes"] > 0 or folded > 0 or p.size != n_reads)
    return out


HAND = [[b""], [b"N"], [b"NNNN"], [b"ACGT"], [b"NACGT"], [b"ACGTN"], [b"ACNNGT"], [b"acgt"], [b"AcGnT"], [b"AC>GT"],
        [b"AC\xc1GT"], [b"\xc1"], [b"ACGT", b"ACGT"], [b"ACGN", b"NCGT"], [b"", b"", b"A", b""], [],
        [b"NNN", b"N", b"", b"nn"], [b"acgt", b"ACGT"], [b"aNc", b"", b"gT"]]


# ---- inputs built for the borders --------------------------------------------------------------------------------------
def plain(n, seed):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)]


def even_offsets(n, step=150):
    return np.unique(np.concatenate([np.arange(0, n, step), [n]])).astype(np.uint64)


def border_inputs(G):
    """(name, bases, offsets, cut positions, offsets as claimed) for granularity G: what the issue lists"""
    tail = 3 * W + 17  # the total is no multiple of the word
    n = G + tail

    def make(name, cuts, off=None, length=n, seed=1):
        b = plain(length, seed)
        cuts = np.asarray(sorted(cuts), dtype=np.int64)
        b[cuts] = ord("N")
        off = even_offsets(length) if off is None else np.asarray(off, dtype=np.uint64)
        return f"{name}@{G}", b, off, cuts, off.copy()

    for d in (-2, -1, 0, 1):
        yield make(f"cut{d:+d}", [G + d], seed=10 + d)
    yield make("run", [G - 1, G, G + 1])
    interior = [x for x in even_offsets(n).tolist() if abs(x - G) > 3 and 0 < x < n]
    at_g = sorted(set([0] + interior + [G, n]))
    yield make("boundary", [], off=at_g)                       # bases on both sides: the two reads must not merge
    yield make("boundary,cut before", [G - 1], off=at_g)
    yield make("boundary,cut after", [G], off=at_g)
    yield make("boundary,cut both", [G - 1, G], off=at_g)
    yield make("empty reads", [], off=sorted([0] + interior + [G, G, G, n]))
    yield make("empty reads,cut", [G], off=sorted([0] + interior + [G, G, n, n]))
    yield make("last byte", [n - 1])
    yield make("ends on G", [G - 1], length=G)                 # a cut as the last byte of a buffer that ends on the border
    if G == B:
        yield block_of_cuts()


def block_of_cuts():
    n = 3 * B
    b = plain(n, 5)
    cuts = np.arange(B, 2 * B, dtype=np.int64)
    b[cuts] = ord("N")
    off = even_offsets(n)
    return "a block of cuts", b, off, cuts, off.copy()


SMALL_G = (W, B, 2 * B)


def random_set(seed, n, rate):
    rng = np.random.default_rng([seed, n, int(rate * 1e6)])
    b = plain(n, rng.integers(1 << 30))
    cut = rng.random(n) < rate
    other = np.frombuffer(b"NnacgtRY>-*\x00\xc1\xff", dtype=np.uint8)
    b[cut] = other[rng.integers(0, other.size, int(cut.sum()))]
    lens = rng.integers(0, 301, n // 100 + 2)
    off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n)
    off[-1] = n
    return b, off.astype(np.uint64)


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_the_struct():
    h = open(os.path.join(ROOT, "include", "dbg.h")).read()
    assert re.search(r"int dbg_split_reads\(dbg_t \*h, uint32_t flags, dbg_split_stats_t \*out", h)
    assert re.search(r"int dbg_read_origins\(dbg_t \*h, uint64_t \*read_index, uint64_t \*pos", h)
    assert re.search(r"#define DBG_SPLIT_FOLD_CASE 1u", h) and _dbg.SPLIT_FOLD_CASE == 1
    body = re.search(r"typedef struct dbg_split_stats \{(.*?)\} dbg_split_stats_t;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [x.strip() for decl in re.findall(r"uint64_t ([^;]*);", body) for x in decl.split(",")]
    assert names == [n for n, _ in _dbg.SplitStats._fields_] == list(STATS) + ["peak_extra_device_bytes"]
    assert re.search(r"#define DBG_ABI_VERSION 6\b", h)
    assert "dbg_split_reads" in _dbg.SYMBOLS and "dbg_read_origins" in _dbg.SYMBOLS


def test_binding_constants_equal_the_kernel_header():
    src = open(os.path.join(PKG, "csrc", "dbg_readsplit.h")).read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        expr = re.sub(r"\(uint64_t\)", "", expr)
        return int(eval(re.sub(r"RS_\w+", lambda m: str(const(m.group(0))), expr)))  # products of earlier constants

    assert const("RS_WORD_BYTES") == _dbg.SPLIT_WORD_BYTES == W
    assert const("RS_BLOCK_BYTES") == _dbg.SPLIT_BLOCK_BYTES == B
    assert const("RS_ROUND_BYTES") == _dbg.SPLIT_ROUND_BYTES == R
    assert W < B < R and B % W == 0 and R % B == 0


@pytest.mark.parametrize("fold", [False, True])
def test_acgt_pieces_is_the_regex_on_the_hand_cases(fold):
    for reads in HAND:
        want = regex_pieces(reads, fold)
        assert prod.acgt_pieces(reads, fold_case=fold) == want, reads
        assert prod.acgt_pieces([r.decode("latin-1") for r in reads], fold_case=fold) == [w.decode("latin-1") for w in want]
        s = numpy_split(*pack(reads), fold)  # the numpy statement of the per-byte rule says the same
        assert unpack(s["bases"], s["offsets"]) == want, reads
        assert s["n_reads_out"] == len(want) and s["n_reads_emptied"] == sum(not regex_pieces([r], fold) for r in reads)
    assert prod.acgt_pieces([b"AC\xc1GT"]) == [b"AC", b"GT"] and prod.acgt_pieces([b"AcGnT"], True) == [b"ACG", b"T"]
    assert prod.acgt_pieces([b"AcGnT"]) == [b"A", b"G", b"T"]


@pytest.mark.parametrize("G", SMALL_G + (R,))
def test_border_inputs_place_their_cuts_and_boundaries_where_they_claim(G):
    for name, b, off, cuts, claimed in border_inputs(G):
        assert np.array_equal(np.flatnonzero(~np.isin(b, ACGT)), cuts), name
        assert np.array_equal(off, claimed) and int(off[0]) == 0 and int(off[-1]) == b.size, name
        assert np.all(np.diff(off.astype(np.int64)) >= 0), name
        if name.startswith("cut"):
            assert cuts.size == 1 and int(cuts[0]) - G == int(name[3:5]), name
        if name.startswith("run"):
            assert cuts.tolist() == [G - 1, G, G + 1]
        if name.startswith("boundary"):
            assert G in off.tolist() and 0 < G < b.size and (name != "boundary@%d" % G or cuts.size == 0)
            assert set(cuts.tolist()) == {"boundary": set(), "boundary,cut before": {G - 1}, "boundary,cut after": {G},
                                          "boundary,cut both": {G - 1, G}}[name.split("@")[0]]
        if name.startswith("empty reads"):
            assert (off == G).sum() >= 2
        if name.startswith("last byte"):
            assert int(cuts[-1]) == b.size - 1 and b.size % W != 0
        if name.startswith("ends on G"):
            assert b.size == G and int(cuts[-1]) == G - 1
        if name.startswith("a block"):
            assert cuts.tolist() == list(range(B, 2 * B)) and b.size == 3 * B


# ---- GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    h = _dbg.Graph()
    yield h
    h.close()


def pointers(h):
    tb, to = h.reads_tensors()
    return tb.data_ptr(), to.data_ptr()


def check_split(h, bases, off, fold, name=""):
    """set_reads + split_reads on handle h against the numpy statement: pieces, offsets, origins, every stats field"""
    want = numpy_split(bases, off, fold)
    h.set_reads(bases, off)
    with pytest.raises(_dbg.DbgError):
        h.read_origins()  # set_reads forgot the origins of the split before
    before = pointers(h)
    st = h.split_reads(fold_case=fold)
    for f in STATS:
        assert st[f] == want[f], (name, fold, f, st, {x: want[x] for x in STATS})
    sz = h.sizes()
    assert sz["n_reads"] == want["n_reads_out"] and sz["n_bytes"] == want["n_bytes_out"], name
    got_b, got_o = h.copy_reads()
    assert np.array_equal(got_o, want["offsets"]), name
    assert np.array_equal(got_b, want["bases"]), name
    rd, pos = h.read_origins()
    assert np.array_equal(rd, want["read_index"]) and np.array_equal(pos, want["pos"]), name
    moved = st["n_reads_out"] != st["n_reads_in"] or st["n_cut_bytes"] > 0
    if moved:
        nblk = -(-bases.size // B)
        assert st["peak_extra_device_bytes"] == (st["n_bytes_out"] + 64) + 8 * (st["n_reads_out"] + 1) + \
            16 * max(st["n_reads_out"], 1) + 16 * nblk, (name, st)
    else:
        assert st["peak_extra_device_bytes"] == 0 and pointers(h) == before, (name, st)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [False, True])
def test_hand_cases(g, fold):
    for reads in HAND:
        bases, off = pack(reads)
        check_split(g, bases, off, fold, name=repr(reads))
        want = regex_pieces(reads, fold)
        assert unpack(*g.copy_reads()) == want, reads
        if want:
            chars, toff = g.take_reads(np.arange(len(want)))  # dbg_take_reads speaks of the pieces
            assert unpack(chars, toff) == want


@pytest.mark.gpu
def test_unknown_flags_and_a_handle_without_reads():
    h = _dbg.Graph()
    with pytest.raises(_dbg.DbgError) as e:
        h.split_reads()
    assert e.value.code == _dbg.DBG_E_ARG
    h.set_reads(*pack([b"ACGT"]))
    for flags in (2, 3, 1 << 31):
        assert h._lib.dbg_split_reads(h._h, flags, None) == _dbg.DBG_E_ARG
    assert h._lib.dbg_split_reads(h._h, 1, None) == _dbg.DBG_OK  # the stats are optional
    h.close()


def build_outcome(h, k):
    try:
        h.build(k)
    except _dbg.DbgError as e:
        return ("error", e.code)
    sz = h.sizes()
    return ("built", sz["n_nodes"], sz["n_edges"], sz["max_degree"])


@pytest.mark.gpu
def test_reads_of_cut_bytes_alone_leave_an_empty_read_set(g):
    bases, off = pack([b"NNNN", b"N", b"", b"nnn"])
    st = check_split(g, bases, off, False)
    assert st["n_reads_out"] == 0 and st["n_bytes_out"] == 0 and st["n_reads_emptied"] == 4 and st["n_reads_changed"] == 3
    empty = _dbg.Graph()
    empty.set_reads(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    for k in (5, 31, 40):
        assert build_outcome(g, k) == build_outcome(empty, k)
    empty.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G", SMALL_G)
def test_borders(g, G):
    for name, b, off, _, _ in border_inputs(G):
        for fold in (False, True):
            check_split(g, b, off, fold, name)


@pytest.mark.gpu
def test_borders_of_the_carry_round(g):
    for name, b, off, _, _ in border_inputs(R):
        check_split(g, b, off, False, name)


@pytest.mark.gpu
def test_two_rounds_of_mostly_cut_bytes(g):
    """more than two rounds of the carry kernel, nearly all of it cut: a piece on each side of both round borders"""
    n = 2 * R + B + 5
    b = np.full(n, ord("N"), dtype=np.uint8)
    for p in (0, R - 2, R - 1, R, 2 * R - 1, 2 * R + 1, n - 1):
        b[p] = ord("C")
    off = np.asarray([0, R, n], dtype=np.uint64)
    st = check_split(g, b, off, False)
    assert st["n_reads_out"] == 6 and st["n_bytes_out"] == 7


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sets(g, seed):
    for n in (1, W - 1, W, W + 1, B - 1, B, B + 1, 3 * B + 17):
        for rate in (0, 2 / B, 0.01, 0.5, 1):
            b, off = random_set(seed, n, rate)
            for fold in (False, True):
                check_split(g, b, off, fold, f"seed {seed} n {n} rate {rate}")


@pytest.mark.gpu
def test_nothing_to_do_leaves_the_read_set_where_it_is(g):
    reads = synth.reads_ascii(3, 5000, 700, 100, 0.01)
    g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, 100, dtype=np.uint64))
    before = pointers(g)
    for fold in (False, True):
        st = g.split_reads(fold_case=fold)
        assert pointers(g) == before
        assert st["changed"] == 0 and st["n_cut_bytes"] == 0 and st["n_folded_bytes"] == 0 and st["peak_extra_device_bytes"] == 0
        assert st["n_reads_out"] == st["n_reads_in"] == 700 and st["n_reads_changed"] == 0 and st["n_reads_emptied"] == 0
        rd, pos = g.read_origins()
        assert np.array_equal(rd, np.arange(700, dtype=np.uint64)) and not pos.any()
    got_b, _ = g.copy_reads()
    assert np.array_equal(got_b, reads.reshape(-1))
    g.synth_reads(3, 5000, 700, 100, 0.01)  # device-made reads: the same
    before = pointers(g)
    assert g.split_reads()["changed"] == 0 and pointers(g) == before
    g.build(21)
    assert g.sizes()["n_nodes"] > 0
    g.split_reads()  # like set_reads it drops the graph
    assert g.sizes()["n_nodes"] == 0 and g.sizes()["k"] == 0


@pytest.mark.gpu
def test_fold_alone_happens_in_place_on_owned_reads(g):
    b, off = pack([b"ACgtAC", b"acgt", b"TTTT"])
    g.set_reads(b, off)
    before = pointers(g)
    st = g.split_reads(fold_case=True)
    assert pointers(g) == before and st["changed"] == 1 and st["n_folded_bytes"] == 6 and st["n_cut_bytes"] == 0
    assert st["peak_extra_device_bytes"] == 0 and st["n_reads_changed"] == 0
    assert unpack(*g.copy_reads()) == [b"ACGTAC", b"ACGT", b"TTTT"]
    rd, pos = g.read_origins()
    assert rd.tolist() == [0, 1, 2] and pos.tolist() == [0, 0, 0]
    assert g.split_reads(fold_case=True)["changed"] == 0  # now there is nothing left to fold


@pytest.mark.gpu
@pytest.mark.parametrize("reads,fold", [([b"ACGTNACGT", b"ACGT"], False), ([b"ACgtAC", b"acgt"], True), ([b"ACGT", b""], False)])
def test_lent_tensors_are_never_written(reads, fold):
    import torch
    b, off = pack(reads)
    pad = np.concatenate([b, np.full(32, 0x5A, np.uint8)])  # bytes behind the reads that nobody may touch either
    tb = torch.from_numpy(pad).cuda()
    to = torch.from_numpy(off.astype(np.int64)).cuda()
    h = _dbg.Graph()
    h.set_reads_tensors(tb[:b.size], to)
    assert pointers(h) == (tb.data_ptr(), to.data_ptr())
    st = h.split_reads(fold_case=fold)
    assert st["changed"] == 1
    assert np.array_equal(tb.cpu().numpy(), pad) and np.array_equal(to.cpu().numpy(), off.astype(np.int64))
    now = pointers(h)
    assert now[0] != tb.data_ptr() and now[1] != to.data_ptr()
    assert unpack(*h.copy_reads()) == regex_pieces(reads, fold)
    rd, pos = h.read_origins()
    want = numpy_split(b, off, fold)
    assert np.array_equal(rd, want["read_index"]) and np.array_equal(pos, want["pos"])
    plain_b = torch.from_numpy(np.frombuffer(b"ACGTTGCA", dtype=np.uint8).copy()).cuda()
    h.set_reads_tensors(plain_b, torch.tensor([0, 4, 8], dtype=torch.int64).cuda())  # lent ACGT reads stay lent
    assert h.split_reads()["changed"] == 0 and pointers(h)[0] == plain_b.data_ptr()
    h.close()


# ---- the graph ----------------------------------------------------------------------------------------------------------
def planted_reads(k):
    """3 000 reads x 150 bp over 30 kbp with N in 1 % of the reads, three all-N reads, a lower-case stretch and one read
    cut into pieces of exactly k and k + 1 bases"""
    reads = [bytearray(r.encode()) for r in synth.reads_list(11, 30000, 3000, 150, 0.005)]
    rng = np.random.default_rng(7)
    for i in rng.choice(np.setdiff1d(np.arange(3000), [0, 100, 200, 1500, 2999]), 30, replace=False):
        for p in rng.integers(0, 150, rng.integers(1, 4)):
            reads[i][p] = ord("N")
    for i in (0, 1500, 2999):
        reads[i][:] = b"N" * 150
    reads[100][40:90] = bytes(reads[100][40:90]).lower()
    r = reads[200]
    r[k] = ord("N")                # [0, k): exactly k bases
    r[2 * k + 2] = ord("N")        # [k + 1, 2 k + 2): exactly k + 1 bases
    return [bytes(x) for x in reads]


def graph_arrays(h, k, threshold=2):
    """Every array of the build and of prune / tips / pull-out / walk.  The node ids of a build are slots of hash tables
    filled with atomics, not a function of the reads alone, so the arrays are put in stamp (first occurrence) order and
    every node id in them is replaced by the node's rank in that order; contigs in the driver's order (start stamp,
    emission index)."""
    out = {}
    h.build(k)
    sz = h.sizes()
    out["sizes"] = {f: sz[f] for f in ("n_reads", "n_bytes", "n_kmer_instances", "n_edge_instances", "n_nodes", "n_edges",
                                      "n_starts", "max_degree")}
    keys, stamps, counts, flags = h.export_nodes()
    o = np.argsort(stamps, kind="stable")
    assert np.all(np.diff(stamps[o].astype(np.int64)) > 0)  # a stamp names one node
    rank = np.empty(o.size, dtype=np.int64)
    rank[o] = np.arange(o.size)
    out["keys"], out["stamps"], out["counts"], out["flags"] = keys[o], stamps[o], counts[o], flags[o]
    out["keys_hi"] = h.export_keys_hi()[o]
    row_ptr, col, cnt = h.export_csr()
    deg = np.diff(row_ptr.astype(np.int64))
    e = np.argsort(rank[np.repeat(np.arange(o.size), deg)], kind="stable")  # the rows in stamp order, columns as they stand
    out["deg"], out["col"], out["cnt"] = deg[o], rank[col][e], cnt[e]
    h.refine_edge_order()
    h.prune(threshold)
    h.remove_tips()
    h.mark_pull_reads()
    h.walk(False)
    out["flags_after"] = h.export_nodes(keys=False, stamps=False, counts=False)[3][o]
    rows, out["branch_keys"], out["branch_hi"] = h.export_marked(_dbg.F_BRANCH)
    out["branch"] = rank[rows]
    rows, out["pulled_keys"], out["pulled_hi"] = h.export_marked(_dbg.F_PULLED)
    out["pulled"] = rank[rows]
    out["read_flags"] = h.export_pull_reads()
    off, chars, score, stamp, seq = h.export_contigs()
    c = np.lexsort((seq, stamp))
    text = chars.tobytes()
    out["contigs"] = np.asarray([text[int(off[i]):int(off[i + 1])] for i in c], dtype=object)
    out["ctg_score"], out["ctg_stamp"], out["ctg_seq"] = score[c], stamp[c], seq[c]
    sz = h.sizes()
    out["sizes_after"] = {f: sz[f] for f in ("n_branch", "n_pulled", "n_pull_reads", "n_contigs", "contig_chars")}
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        if isinstance(a[name], dict):
            assert a[name] == b[name], name
        else:
            assert a[name] is None and b[name] is None or np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 21, 31, 32, 63])
def test_graph_of_a_split_read_set_is_the_graph_of_the_pieces(k):
    reads = planted_reads(k)
    pieces = prod.acgt_pieces(reads, fold_case=True)
    assert [len(p) for p in prod.acgt_pieces([reads[200]], True)] == [k, k + 1, 150 - 2 * k - 3]
    a, b, raw = _dbg.Graph(), _dbg.Graph(), _dbg.Graph()
    a.set_reads(*pack(reads))
    st = a.split_reads(fold_case=True)
    assert st["n_reads_out"] == len(pieces) and st["n_reads_emptied"] == 3 and st["n_folded_bytes"] == 50
    b.set_reads(*pack(pieces))
    ga, gb = graph_arrays(a, k), graph_arrays(b, k)
    assert_same(ga, gb)
    assert ga["sizes"]["max_degree"] == 4 and ga["sizes"]["n_nodes"] > 0 and ga["sizes_after"]["n_contigs"] > 0
    raw.set_reads(*pack(reads))  # without the split: N and the lower-case bases are characters, the generic engine
    raw.build(k)
    assert raw.sizes()["max_degree"] == 32
    for h in (a, b, raw):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [5, 21])
def test_split_reads_through_construct_graph_equal_the_oracle_on_the_pieces(k, tmp_path):
    from oracle import dbg_oracle as orc
    reads = [r.decode() for r in planted_reads(k)]
    pieces = prod.acgt_pieces(reads, fold_case=True)
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, reads)
    dev = prod.DeviceReads(p, non_acgt="split", fold_case=True)
    assert list(dev) == pieces
    with contextlib.redirect_stdout(io.StringIO()):
        g, pull, branch, pulled, ect = prod.construct_graph(dev, k, threshold=2)
        contigs = prod.output_contigs(g, branch, pulled)
        og, opull, obranch, opulled, oect = orc.construct_graph(pieces, k, threshold=2)
        ocontigs = orc.output_contigs(og, obranch, opulled)
    assert [(v, n.indegree, n.outdegree) for v, n in g[0].items()] == [(v, n.indegree, n.outdegree) for v, n in og[0].items()]
    assert list(ect.items()) == list(oect.items())
    assert {v: list(s) for v, s in g[1].items()} == {v: list(s) for v, s in og[1].items()}
    assert list(branch) == list(obranch) and list(pulled) == list(opulled) and list(pull) == list(opull)
    assert list(contigs) == list(ocontigs)


# ---- parts and shards --------------------------------------------------------------------------------------------------
def canonical_part(parts, p):
    """a part's arrays in stamp order (local node ids are table slots, see graph_arrays); a column is named by the part
    and the k-mer of its target"""
    d = parts[p]
    o = np.argsort(d["stamps"], kind="stable")
    deg = np.diff(d["row_ptr"].astype(np.int64))
    rank = np.empty(o.size, dtype=np.int64)
    rank[o] = np.arange(o.size)
    e = np.argsort(rank[np.repeat(np.arange(o.size), deg)], kind="stable")
    tk, th = np.zeros(d["col"].size, np.uint64), np.zeros(d["col"].size, np.uint64)
    for q, dq in enumerate(parts):
        sel = d["col_part"] == q
        tk[sel], th[sel] = dq["keys"][d["col"][sel]], dq["keys_hi"][d["col"][sel]]
    return {"keys": d["keys"][o], "keys_hi": d["keys_hi"][o], "stamps": d["stamps"][o], "flags": d["flags"][o], "deg": deg[o],
            "col_part": d["col_part"][e], "col_key": tk[e], "col_key_hi": th[e], "cnt": d["cnt"][e]}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_multipass_build_of_a_split_read_set(k):
    reads = planted_reads(k)
    a, b = _dbg.Graph(), _dbg.Graph()
    a.set_reads(*pack(reads))
    with pytest.raises(_dbg.AlphabetError) as e:
        a.build_multipass(k, 4)
    assert e.value.code == _dbg.DBG_E_ALPHABET
    a.set_reads(*pack(reads))
    a.split_reads(fold_case=True)
    a.build_multipass(k, 4)
    b.set_reads(*pack(prod.acgt_pieces(reads, fold_case=True)))
    b.build_multipass(k, 4)
    assert a.part_count() == b.part_count() == 4
    pa, pb = [a.export_part(p) for p in range(4)], [b.export_part(p) for p in range(4)]
    for part in range(4):
        assert a.part_sizes(part) == b.part_sizes(part)
        ca, cb = canonical_part(pa, part), canonical_part(pb, part)
        for name in ca:
            assert np.array_equal(ca[name], cb[name]), (part, name)
    assert a.sizes()["n_nodes"] == b.sizes()["n_nodes"] > 0
    a.close()
    b.close()


def shard_nodes(h):
    keys, stamps, counts, _ = h.export_nodes(flags=False)
    hi = h.export_keys_hi()
    o = np.lexsort((hi, keys))
    return keys[o], hi[o], stamps[o], counts[o]


@pytest.mark.gpu
def test_two_ranks_split_their_own_lines_before_the_sharded_build(tmp_path):
    import inproc_dist
    import multi_gpu
    k = 31
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, [r.decode() for r in planted_reads(k)])

    def one(dist, rank):
        h = _dbg.Graph(device=0)
        multi_gpu.set_reads_fasta_shard(h, p, dist, chunk_bytes=1 << 16, non_acgt="split", fold_case=True)
        n_pieces = h.sizes()["n_reads"]
        multi_gpu.sharded_build(h, k, dist)
        keys, stamps, counts, _ = h.export_nodes(flags=False)
        out = (keys, h.export_keys_hi(), stamps, counts, n_pieces)
        h.close()
        return out

    shards = inproc_dist.run_ranks(2, one)
    keys, hi, stamps, counts = (np.concatenate([s[i] for s in shards]) for i in range(4))
    o = np.lexsort((hi, keys))
    whole = prod.DeviceReads(p, non_acgt="split", fold_case=True)
    assert sum(s[4] for s in shards) == len(whole)  # the ranks' pieces are the file's pieces
    whole._graph.build(k)
    want = shard_nodes(whole._graph)
    assert want[0].size == keys.size > 0
    for x, y in zip((keys[o], hi[o], stamps[o], counts[o]), want):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        multi_gpu.set_reads_fasta_shard(whole._graph, p, None, non_acgt="drop")


# ---- FASTA routes and driver -------------------------------------------------------------------------------------------
def small_fasta_reads():
    reads = synth.reads_list(41, 3000, 400, 80, 0.005)
    rng = np.random.default_rng(3)
    for i in rng.choice(400, 40, replace=False):
        r = bytearray(reads[i].encode())
        for p in rng.integers(0, 80, rng.integers(1, 4)):
            r[p] = ord("N")
        reads[i] = r.decode()
    reads[5] = "N" * 80
    reads[6] = reads[6][:20] + reads[6][20:50].lower() + reads[6][50:]
    reads[7] = ""
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [False, True])
def test_fasta_routes_list_the_pieces(tmp_path, fold):
    reads = small_fasta_reads()
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, reads)
    lines = prod.read_reads(p)
    assert lines == reads
    want = prod.acgt_pieces(lines, fold_case=fold)
    assert list(prod.DeviceReads(p)) == lines and prod.DeviceReads(p).split_stats is None  # the default: unchanged
    for kw in ({}, {"chunk_bytes": 64}):
        dev = prod.read_reads_device(p, non_acgt="split", fold_case=fold, **kw)
        assert list(dev) == want and len(dev) == len(want)
        assert dev.split_stats["n_reads_in"] == len(lines) and dev.split_stats["n_reads_out"] == len(want)
        rd, pos = dev.origins()
        tr = str.maketrans("acgt", "ACGT")
        for piece, r, q in zip(want, rd.tolist(), pos.tolist()):
            line = lines[r].translate(tr) if fold else lines[r]
            assert line[q:q + len(piece)] == piece
            assert (q == 0 or line[q - 1] not in "ACGT") and (q + len(piece) == len(line) or line[q + len(piece)] not in "ACGT")
    with pytest.raises(ValueError):
        prod.DeviceReads(p, non_acgt="drop")
    with pytest.raises(ValueError):
        prod.DeviceReads(p).origins()


@pytest.mark.gpu
def test_driver_with_split_in_the_settings_writes_what_the_pieces_give(tmp_path):
    reads = small_fasta_reads()
    synth.write_froot(str(tmp_path / "masked"), reads, 12, 15, threshold=2)
    with open(tmp_path / "masked" / "setting.json") as fh:
        setting = json.load(fh)
    setting.update(non_acgt="split", fold_case=True)
    with open(tmp_path / "masked" / "setting.json", "w") as fh:
        json.dump(setting, fh)
    synth.write_froot(str(tmp_path / "pieces"), prod.acgt_pieces(reads, fold_case=True), 12, 15, threshold=2)
    env = dict(os.environ, PYTHONPATH=PKG)
    out = {}
    for froot in ("masked", "pieces"):
        subprocess.check_call([sys.executable, os.path.join(PKG, "II_assembleFromReads.py"), "-froot", froot],
                              cwd=str(tmp_path), env=env, stdout=subprocess.DEVNULL)
        out[froot] = (tmp_path / froot / f"{froot}.fasta").read_bytes()
    assert out["masked"] == out["pieces"] and out["pieces"].startswith(b">SEQUENCE_0_15mer\n")
