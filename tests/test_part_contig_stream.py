"""Contig text and FASTA streamed off a graph in PARTS (dbg_part_set_skeleton, dbg_part_export_contig_texts,
dbg_part_write_contigs_fasta, dbg_part_contig_window; part_traversal.PartContigs on top): a multi-pass build on one handle,
and ranks x passes with the in-process exchange, against the single-GPU walk's contigs on all reads (debruijn.construct_graph
+ output_contigs, pinned by the reference's vectors) and host formatting of those texts.

Input: the 4000 x 120 reads and threshold 2 of test_part_traversal's text test -- 990 .. 2256 contigs of k .. 17 935
characters (they overlap: 0.5 .. 7.5 MB of text), so a file at 4096-byte windows has hundreds of borders."""
import os
import threading

import numpy as np
import pytest

import _dbg
import synth

pytestmark = pytest.mark.gpu

CASES = [(21, 4, 1), (63, 2, 1), (31, 1, 1), (31, 1, 4), (21, 2, 2)]
N_READS, L, THR = 4000, 120, 2
U64_MAX = np.iinfo(np.uint64).max
HEADER_FIELDS = ("keyword", "number", "k digits", "mer")   # the fields of a header longer than a byte (or cut strictly inside)


def _reads(rank, ranks):
    per = N_READS // ranks
    return synth.reads_ascii(31, N_READS * L // 20, per, L, 0.01, first_read=rank * per)


def _fasta(texts, first=0, k=0):
    return b"".join(b">SEQUENCE_%d_%dmer\n%s\n" % (first + i, k, t) for i, t in enumerate(texts))


_expected, _worlds = {}, {}


def expected(k):
    """The single-GPU walk on all reads, once per k: (texts as bytes in dict order of the starts, scores)."""
    if k not in _expected:
        import contextlib
        import io
        import debruijn as prod
        allr = np.concatenate([_reads(r, 4) for r in range(4)])
        assert np.array_equal(allr, _reads(0, 1))   # the ranks' reads are the one read set, cut
        with contextlib.redirect_stdout(io.StringIO()):
            gg, pull, branch, pulled, ect = prod.construct_graph([row.tobytes().decode() for row in allr], k, threshold=THR)
            wc = prod.output_contigs(gg, branch, pulled)
            texts, scores = [t.encode("ascii") for t in wc], [int(s) for s in prod.get_score_device(wc)]
        assert len(texts) > 50
        _expected[k] = (texts, scores)
    return _expected[k]


class World:
    """The ranks of one case, kept for all tests of it: handles, traversals, PartContigs, and the skeleton rank 0 handed to
    the library (host copies taken on the way in)."""

    def __init__(self, k, passes, ranks):
        import inproc_dist
        import multi_gpu
        import part_traversal
        self.k, self.passes, self.ranks, self.nv = k, passes, ranks, passes * ranks
        self.sk = {}

        def one(dist, rank):
            reads = _reads(rank, ranks)
            g = _dbg.Graph(device=0)
            g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, L, dtype=np.uint64))
            if dist is None:
                g.build_multipass(k, passes)
            else:
                multi_gpu.sharded_build_multipass(g, k, dist, passes)
            real = g.part_set_skeleton

            def keeping(*cols):
                if rank == 0:
                    self.sk = dict(zip(("gid", "next", "go_on", "hops", "rest"), [c.cpu().numpy().copy() for c in cols]))
                return real(*cols)
            g.part_set_skeleton = keeping
            t, _, _, _ = part_traversal.construct_graph(g, k, THR, dist)
            ctg = part_traversal.output_contigs(t)
            del g.part_set_skeleton
            return g, t, ctg

        got = [one(None, 0)] if ranks == 1 else inproc_dist.run_ranks(ranks, one)
        self.gs, self.ts, self.ctgs = (list(x) for x in zip(*got))
        self.want, self.scores = expected(k)
        self.n = len(self.want)

    def run(self, fn):
        """fn(rank, traversal, contigs) on every rank at once (the calls are collective) -> results by rank."""
        if self.ranks == 1:
            return [fn(0, self.ts[0], self.ctgs[0])]
        out, errors = [None] * self.ranks, []
        barrier = self.ts[0].net.dist._w.barrier   # the in-process world's: a rank that raised must not leave the others waiting

        def body(r):
            try:
                out[r] = fn(r, self.ts[r], self.ctgs[r])
            except BaseException as e:  # noqa: BLE001 -- reported below
                errors.append((r, e))
                barrier.abort()

        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.ranks)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            barrier.reset()
            errors.sort(key=lambda x: isinstance(x[1], threading.BrokenBarrierError))
            raise errors[0][1]
        return out

    def segments(self, c):
        """skeleton rows of contig c's chain, in order"""
        sk, i = self.sk, int(self.ts[0].skeleton["emit"][c])
        rows = [i]
        while sk["go_on"][i]:
            i = int(sk["next"][i])
            rows.append(i)
        return rows

    def close(self):
        for g in self.gs:
            g.close()


def world(case):
    if case not in _worlds:
        _worlds[case] = World(*case)
    return _worlds[case]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.close()
    _worlds.clear()
    _expected.clear()


def _cut_kinds(w, order, first, k_label, chunk):
    """How often a window border falls in each kind of place of the records of the contigs ``order`` -- strictly inside a
    header field (as test_contig_stream._cut_kinds counts them), inside a segment of a contig text, or exactly between two
    segments of it (the byte before the border is a segment's last character, the byte at it the next segment's first)."""
    kinds = {"header": 0, "inside a segment": 0, "between two segments": 0, "other": 0}
    k, sk = w.k, w.sk
    at, nxt = 0, chunk
    for i, c in enumerate(order):
        t = w.want[c]
        for name, part in zip(("keyword", "number", "underscore", "k digits", "mer", "text", "newline"),
                              (b">SEQUENCE_", b"%d" % (first + i), b"_", b"%d" % k_label, b"mer\n", t, b"\n")):
            lo, hi = at, at + len(part)
            while nxt < lo:
                nxt += chunk
            for b in range(nxt, hi, chunk):
                if name in HEADER_FIELDS and lo < b:
                    kinds["header"] += 1
                elif name == "text" and lo < b:
                    begins, a = set(), 0            # appended index at which a later segment begins
                    for row in w.segments(c)[:-1]:
                        a += int(sk["hops"][row]) + 1
                        begins.add(a)
                    j = b - lo                      # character of the contig at the border
                    kinds["between two segments" if j - k + 1 in begins else "inside a segment"] += 1
                else:
                    kinds["other"] += 1
            at = hi
    return kinds


@pytest.mark.parametrize("case", CASES)
def test_packed_and_batched_texts_equal_the_single_gpu_contigs(case):
    w = world(case)
    k = w.k
    rng = np.random.default_rng(7)
    shuffled = rng.integers(0, w.n, size=w.n // 3 + 5)      # any order, repeats
    assert np.unique(shuffled).size < shuffled.size

    def one(rank, t, ctg):
        assert len(ctg) == w.n and ctg.lengths.tolist() == [len(x) for x in w.want]
        chars, off = ctg.packed()
        texts = ctg.texts(range(len(ctg)))
        o2, c2 = t.contig_texts_packed(shuffled)
        return chars.tobytes(), off.tolist(), texts, c2.tobytes(), o2.tolist(), ctg.texts(shuffled.tolist()), ctg.texts([]), \
            t.contig_texts_packed([]), ctg[0], ctg[-1], ctg[5:9]

    # the input really exercises the feature: with more than one virtual shard some contig has at least 3 segments in at
    # least 2 shards; with one (n_passes = 1 on one rank) every chain is ONE segment, the long-segment path
    seg_counts = [len(w.segments(c)) for c in range(w.n)]
    if w.nv > 1:
        assert any(len(rows) >= 3 and len({int(w.sk["gid"][r]) >> 32 for r in rows}) >= 2 for rows in map(w.segments, range(w.n)))
    else:
        assert max(seg_counts) == 1 and int(w.sk["hops"].max()) > 4096
    for chars, off, texts, c2, o2, t2, empty, empty_packed, first, last, sl in w.run(one):
        assert off == np.concatenate([[0], np.cumsum([len(x) for x in w.want])]).tolist()
        assert chars == b"".join(w.want)
        assert [x.encode("ascii") for x in texts] == w.want
        assert c2 == b"".join(w.want[i] for i in shuffled) and o2 == np.concatenate([[0], np.cumsum([len(w.want[i]) for i in shuffled])]).tolist()
        assert [x.encode("ascii") for x in t2] == [w.want[i] for i in shuffled]
        assert empty == [] and empty_packed[0].tolist() == [0] and empty_packed[1].size == 0
        assert first.encode() == w.want[0] and last.encode() == w.want[-1] and [x.encode() for x in sl] == w.want[5:9]
    assert min(len(x) for x in w.want) >= k


@pytest.mark.parametrize("case", CASES)
def test_write_fasta_equals_host_formatting(case, tmp_path):
    """The driver's order and lists of the caller's; append on and off; record numbers over 9 -> 10 and 99 -> 100; windows of
    4096, 8192 and the default size.  The list written at 4096-byte windows has a border inside a header, inside a segment
    and exactly between two segments (a condition on the input: the first seed that gives all three is taken)."""
    w = world(case)
    k = w.k
    driver = sorted(range(w.n), key=lambda i: w.scores[i], reverse=True)   # sequences.sort(key=getScore, reverse=True)
    # the 4096-byte run takes a shorter list where a window is dear: several ranks gather every window, and with ONE virtual
    # shard a segment is a whole chain (up to 14 837 steps behind every descent, DESIGN 4g "long segments")
    n_short = w.n if w.ranks == 1 and w.nv > 1 else 60
    need = ("header", "inside a segment") + (("between two segments",) if w.nv > 1 else ())
    for seed in range(1, 100):
        perm = np.random.default_rng(seed).permutation(w.n)[:n_short].tolist()
        kinds = _cut_kinds(w, perm, 8, 7, 4096)
        if all(kinds[x] for x in need):
            break
    print(case, "seed", seed, kinds)
    assert all(kinds[x] for x in need), kinds

    def one(rank, t, ctg):
        p = lambda name: os.path.join(tmp_path, f"{name}.rank{rank}.fa")  # noqa: E731
        out = []
        out.append(ctg.write_fasta(p("driver"), k, append=False))                                  # truncates
        out.append(t.write_contigs_fasta(p("list"), perm, first_number=8, k_label=7, append=False, chunk_bytes=4096))
        out.append(t.write_contigs_fasta(p("list"), perm[:9], first_number=95, append=True, chunk_bytes=8192))
        out.append(t.write_contigs_fasta(p("list"), [], append=True))                              # nothing
        out.append(ctg.write_fasta(p("list"), 5, append=True))                                     # the default windows, appended
        out.append(t.write_contigs_fasta(p("none"), [], append=False))                             # touches nothing
        return out

    want_driver = _fasta([w.want[i] for i in driver], 0, k)
    want_list = [_fasta([w.want[i] for i in perm], 8, 7), _fasta([w.want[i] for i in perm[:9]], 95, k),
                 _fasta([w.want[i] for i in driver], 0, 5)]
    for out in w.run(one):   # every rank returns the same counts
        assert out == [len(want_driver), len(want_list[0]), len(want_list[1]), 0, len(want_list[2]), 0]
    assert open(os.path.join(tmp_path, "driver.rank0.fa"), "rb").read() == want_driver
    assert open(os.path.join(tmp_path, "list.rank0.fa"), "rb").read() == b"".join(want_list)
    assert sorted(os.listdir(tmp_path)) == ["driver.rank0.fa", "list.rank0.fa"]   # rank 0 alone writes; an empty list makes no file


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 1])
def test_peak_device_memory_of_the_writer(case, tmp_path):
    """skeleton copy (26 B a row) + lifting table + 2 windows + per-record arrays (36 B a record) + 1 MiB."""
    w = world(case)
    g, t = w.gs[0], w.ts[0]
    path = os.path.join(tmp_path, "peak.fa")
    which = None if w.nv > 1 else list(range(0, w.n, 20))   # one shard: long segments make 4096-byte windows dear
    n_rec = w.n if which is None else len(which)
    n_bytes = t.write_contigs_fasta(path, which, append=False, chunk_bytes=4096)
    st = g.contig_output_stats()
    n_rows = w.sk["gid"].size
    jumps = max(len(w.segments(c)) for c in range(w.n)) - 1
    levels = 0
    while (1 << levels) - 1 < jumps:
        levels += 1
    assert st["lift_bytes"] == levels * n_rows * 4      # the smallest table that covers the longest chain of a contig
    assert st["bytes_written"] == n_bytes == os.path.getsize(path) and st["chunk_bytes"] == 4096 and st["chunks"] == -(-n_bytes // 4096)
    bound = 26 * n_rows + st["lift_bytes"] + 2 * 4096 + 36 * (n_rec + 1) + (1 << 20)
    print(case, "peak device bytes", st["peak_device_bytes"], "bound", bound)
    assert 26 * n_rows + st["lift_bytes"] < st["peak_device_bytes"] <= bound


@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 1])
def test_host_facing_calls_refuse_one_rank_of_several(case, tmp_path):
    w = world(case)
    starts = w.ts[0].skeleton["emit"]
    for r in range(w.ranks):
        g = w.gs[r]
        with pytest.raises(_dbg.DbgError, match="dbg_part_contig_window"):
            g.part_export_contig_texts(starts)
        with pytest.raises(_dbg.DbgError, match="dbg_part_contig_window"):
            g.part_write_contigs_fasta(os.path.join(tmp_path, "x.fa"), starts, append=False)
    assert os.listdir(tmp_path) == []                    # a refused list leaves the path alone
    assert [x[0].encode() for x in w.run(lambda rank, t, ctg: ctg.texts([3]))] == [w.want[3]] * w.ranks   # the handles stay usable


@pytest.mark.parametrize("case", CASES)
def test_iteration_and_slices_are_batched(case, monkeypatch):
    """Neither a per-piece nor a per-contig library call: one batched export (one rank) or one window sequence (several)."""
    w = world(case)
    calls = []

    def boom(*a, **kw):
        raise AssertionError("part_segment_text was called")
    monkeypatch.setattr(_dbg.Graph, "part_segment_text", boom)
    for name in ("part_export_contig_texts", "part_contig_window", "part_gather", "export_contig_text"):
        real = getattr(_dbg.Graph, name)
        monkeypatch.setattr(_dbg.Graph, name, lambda self, *a, _real=real, _name=name, **kw: (calls.append(_name), _real(self, *a, **kw))[1])
    got = w.run(lambda rank, t, ctg: (list(ctg), ctg[10:40], ctg[::7]))
    for everything, sl, strided in got:
        assert [x.encode() for x in everything] == w.want and [x.encode() for x in sl] == w.want[10:40]
        assert [x.encode() for x in strided] == w.want[::7]
    windows = -(-sum(len(x) for x in w.want) // (4 << 20))
    per_rank = 3 if w.ranks == 1 else (1 + windows) + 2 + 2     # one export each; or the size call and the windows
    assert len(calls) <= per_rank * w.ranks < w.n, (len(calls), sorted(set(calls)))
    assert set(calls) == ({"part_export_contig_texts"} if w.ranks == 1 else {"part_contig_window"})


def test_refusals_leave_the_handle_usable(tmp_path):
    """Every DBG_E_ARG of the four calls, each followed by a call that works; broken skeletons are refused by
    part_set_skeleton before any kernel walks them (no test makes one walk)."""
    import torch
    import part_traversal
    k, passes = 21, 2
    reads = _reads(0, 1)
    want, _ = expected(k)
    g = _dbg.Graph(device=0)
    g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, L, dtype=np.uint64))
    g.build_multipass(k, passes)
    t, _, _, _ = part_traversal.construct_graph(g, k, THR)
    index = t.walk_index()                                # no skeleton kept
    with pytest.raises(_dbg.DbgError, match="skeleton"):
        g.part_export_contig_texts([0])
    with pytest.raises(_dbg.DbgError, match="skeleton"):
        g.part_write_contigs_fasta(os.path.join(tmp_path, "a.fa"), [0])
    with pytest.raises(_dbg.DbgError, match="skeleton"):
        g.part_contig_window(torch.zeros(1, dtype=torch.int64, device="cuda:0"), 0, 0)
    cols = {}
    real = g.part_set_skeleton
    g.part_set_skeleton = lambda *c: (cols.update(zip(("gid", "next", "go_on", "hops", "rest"), [x.clone() for x in c])), real(*c))[1]
    ctg = part_traversal.output_contigs(t)
    del g.part_set_skeleton
    emit, n_rows = t.skeleton["emit"], cols["gid"].numel()
    assert np.array_equal(ctg.lengths, index["length"])

    def works(c=3):
        off, chars = g.part_export_contig_texts([emit[c]])
        assert chars.tobytes() == want[c] and off.tolist() == [0, len(want[c])]

    def good():
        g.part_set_skeleton(*[cols[c] for c in ("gid", "next", "go_on", "hops", "rest")])

    works()
    path = os.path.join(tmp_path, "r.fa")
    with pytest.raises(_dbg.DbgError, match="not below"):
        g.part_export_contig_texts([emit[0], n_rows])     # a start >= n_entries
    works()
    with pytest.raises(_dbg.DbgError, match="multiple of 4096"):
        g.part_write_contigs_fasta(path, emit[:3], chunk_bytes=1000)
    with pytest.raises(_dbg.DbgError, match="multiple of 4096"):
        t.write_contigs_fasta(path, [0, 1], chunk_bytes=6000)
    with pytest.raises(_dbg.DbgError, match="multiple of 4096"):
        g.part_contig_window(torch.from_numpy(emit[:3].copy()).to("cuda:0"), 100, 4196, torch.zeros(8192, dtype=torch.uint8, device="cuda:0"))
    assert not os.path.exists(path)
    assert g.part_write_contigs_fasta(path, emit[:3], append=False) == len(_fasta(want[:3], 0, k))
    with pytest.raises(_dbg.DbgError, match="such"):
        g.part_write_contigs_fasta(os.path.join(tmp_path, "no", "such", "dir.fa"), emit[:3])
    assert g.part_write_contigs_fasta(path, emit[3:5], first_number=3) == len(_fasta(want[3:5], 3, k))
    assert open(path, "rb").read() == _fasta(want[:5], 0, k)
    assert g.part_write_contigs_fasta(path, [], append=False) == 0 and os.path.getsize(path) == len(_fasta(want[:5], 0, k))   # n = 0 touches nothing
    assert g.part_export_contig_texts([])[0].tolist() == [0]
    # the window call by hand: bytes [4096, 8192) of the bare texts
    d_starts = torch.from_numpy(emit.copy()).to("cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    total = g.part_contig_window(d_starts, 4096, 8192, buf)
    assert total == sum(len(x) for x in want) and buf.cpu().numpy().tobytes() == b"".join(want)[4096:8192]
    # a start whose rest is the sentinel (a start has no predecessor, so the rest of the skeleton stays consistent)
    rest = cols["rest"].clone()
    rest[int(emit[0])] = -1
    g.part_set_skeleton(cols["gid"], cols["next"], cols["go_on"], cols["hops"], rest)
    with pytest.raises(_dbg.DbgError, match="no contig"):
        g.part_export_contig_texts([emit[0]])
    works(1)
    # broken skeletons
    gid, nxt, hops = cols["gid"], cols["next"], cols["hops"]
    live_go = int(torch.nonzero((cols["rest"] >= 0) & cols["go_on"])[0])
    sizes = [g.part_sizes(p)["n_nodes"] for p in range(passes)]
    last0 = int(torch.nonzero((gid >> 32) == 0)[-1])      # the last row of part 0: its local id may grow and gid stays ascending
    broken = {}
    b = nxt.clone(); b[1] = n_rows
    broken["next"] = (gid, b, cols["go_on"], hops, cols["rest"])
    b = gid.clone(); b[[1, 2]] = gid[[2, 1]]
    broken["ascending"] = (b, nxt, cols["go_on"], hops, cols["rest"])
    b = cols["rest"].clone(); b[live_go] += 1
    broken["rest"] = (gid, nxt, cols["go_on"], hops, b)
    b = gid.clone(); b[last0] = sizes[0]
    broken["n_nodes"] = (b, nxt, cols["go_on"], hops, cols["rest"])
    for what, c in broken.items():
        with pytest.raises(_dbg.DbgError, match=what):
            g.part_set_skeleton(*c)
        with pytest.raises(_dbg.DbgError, match="skeleton"):   # nothing is kept
            g.part_export_contig_texts([emit[0]])
        good()
        works()
    # a graph rebuilt since the skeleton was set
    g.build_multipass(k, passes)
    with pytest.raises(_dbg.DbgError, match="skeleton"):
        g.part_export_contig_texts([emit[0]])
    t2, _, _, _ = part_traversal.construct_graph(g, k, THR)
    assert [x.encode() for x in part_traversal.output_contigs(t2).texts([0, 2])] == [want[0], want[2]]
    g.build(k)
    with pytest.raises(_dbg.DbgError, match="parts"):
        g.part_export_contig_texts([emit[0]])
    g.close()
