"""Every kernel that streams the reads takes its windows out of the tile image of load_tile (csrc/dbg_device.h): TILE = 8192
positions plus a halo of 64 (TileLds) or 128 (TileLdsW).  tests/test_extract_shared_hashes.py puts the two one-word
extraction kernels on inputs built for the borders of that image; this module does it for the other nine callers.
The tip removal and the walk do not read the reads: every input here has branch nodes and pull-out reads but no pulled node,
so compare()'s check of the pulled set holds trivially, and what these tests exercise of the traversal is the node table, the
successor ranks, keep masks, branch list, read flags and the contig index.

A. k_wsk_extract_w / k_wsk_extract (k = 32 .. 63): searched inputs of two or three tiles whose minimizers lie across the lane
   (32), wave (2 048) and tile (8 192) borders -- and, where the window allows it, a whole lane or two lanes beyond the
   k-mer's start --, against orc_c.build, the numpy record count and the builds that take other kernels.
B. k_edge_first_seen, k_pull_reads, k_count, k_wedge_first_seen, k_wpull_reads, k_wcount: planted inputs.  A branch k-mer X
   whose first X -> a instance starts d = k, k - 1, k / 2, 1, 0 positions before a tile border (the successor order of X
   then hangs on that one instance), a control Y whose straddling instance is the later one, reads of length exactly k
   on a border and at the end of the data, against Oracle.traverse.
B'. k_ws_extract (the instances a rank of a sharded build sends under wide_engine=0, reached through dbg_shard_extract): the
   planted sets and three of A's against a numpy enumeration that a CPU test ties to the C oracle.
C. the crowded fallback of k_sk_refine / k_sk_pull, proven to run by the counters "refine_crowded" / "pull_crowded".
D. one byte outside ACGT at the positions where load_tile's `bad` flag could miss it.  The sets are the existing module's,
   whose shortest read has 31 bases: "inside a read shorter than k" is that at k = 32 and 63 only, at k = 5, 21, 31 the
   position is one more interior byte.

Every input is checked in tests without the gpu mark, from numpy and the C oracle alone, for what it claims to exercise.

Part B, from the oracle (threshold 2), the same for k = 21, 31, 32, 47, 63:
  set       bytes    branch nodes  pulled nodes  pull-out reads
  exact3    24 576   1             0             6
  ragged    22 391   1             0             6
  pairs_a   21 387   2             0             8
  pairs_b   21 386   2             0             8
Part C's input: 4 086 nodes, 3 933 with two or more successors, 3 309 branch nodes, 0 pulled nodes, 133 pull-out reads of 139.

On an MI355X the 198 GPU tests of this module take 9.8 s; the slowest are the two of part C (2.4 s each), then 0.3 s.

What fails when the code is broken (each mutation built once on a scratch copy and run once, before part B' existed; from
the code, B' would fail under the first at "key words" and under the third at "stamps / has-successor bits"):
  load_tile leaves the halo words unwritten      part A from its first case on ("a successor k-mer was not found in its
                                                 bucket", n_nodes, successors); the broken graphs then fault a later kernel
  k_wsk_extract_w zeroes its third window        part A at k = 44, 45, 63, every set (n_nodes / successor not found), and
                                                 every part B row at k = 47, 63 that takes that extraction
  tile_inst takes at_end from bit k - 1          part A, all 30 cases, at the comparison with wide_engine=0; a broken graph of
                                                 part B then faulted a later kernel (the tip removal's copy reported it)
  k_wpull_reads breaks at p + k >= n_bytes       part B, exact3 and ragged at k = 32, 47, 63, every row: "pull_out_read differs"
                                                 (the read of length k that ends the data)
  k_wedge_first_seen without the next tile's     part B, ragged at k = 32, 47, 63, every row: "successor ranks differ" (X as a
  first start bit                                read that ends with the tile, followed by b)
"""
import numpy as np
import pytest

import _dbg
from oracle import orc_c
from test_extract_shared_hashes import (M, TILE, build, low_complexity_reads, minimizers, n_records_expected, random_reads,
                                         read_set)
from test_generic_engine import D as GENERIC_DEGREE
from test_generic_engine import table_reference
from test_traversal_vs_c_oracle import compare, device_traversal

gpu = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def long_reads(seed, total, starts_at=()):
    """random_reads with reads of 64 .. 300 bases: at k = 63 every read carries k-mers."""
    return random_reads(seed, total, starts_at, min_len=64)


def frozen(bases, offsets):
    bases.setflags(write=False)
    offsets.setflags(write=False)
    return bases, offsets


# =========================================================================================================================
# A. two-word extraction at the borders
# =========================================================================================================================
WIDE_KS = [32, 33, 44, 45, 63]  # W = k - 12 = 20, 21 (below a lane), 32 (W - 1 stays in the next lane), 33 (exactly a lane), 51
A_SETS = {
    # name: (maker, arguments); the seeds are the first for which every k passes assert_wide_borders
    "three_tiles": (long_reads, (0, 27_013, (TILE, 2 * TILE + 1))),
    "two_tiles_exactly": (long_reads, (0, 2 * TILE)),
    "two_tiles_and_a_byte": (long_reads, (0, 2 * TILE + 1)),
    "not_a_multiple_of_16": (long_reads, (0, 2 * TILE + 1000 + 7)),
    "low_complexity": (low_complexity_reads, (0, 26_000)),
    # a read's last byte is the first tile's last byte, so its last k-mer starts at TILE - k (one statement: a read that ends
    # at e has its last k-mer at e - k); reads lie across the second border
    "read_ends_on_border": (long_reads, (0, 2 * TILE + 3000 + 5, (TILE,))),
}
_a_sets = {}


def a_set(name):
    if name not in _a_sets:
        maker, args = A_SETS[name]
        _a_sets[name] = frozen(*maker(*args))
    return _a_sets[name]


def record_starts(valid, minpos):
    """n_records_expected's rule as a mask: the k-mer at p opens a super-k-mer record."""
    p = np.arange(valid.size)
    prev_valid = np.concatenate([[False], valid[:-1]])
    prev_min = np.concatenate([[-1], minpos[:-1]])
    return valid & ((p % TILE == 0) | ~prev_valid | (prev_min != minpos))


def assert_wide_borders(name, k, bases, offsets):
    """What assert_exercises_the_borders asks, for the three borders, and what only windows of a lane and more can show."""
    w = k - M + 1
    valid, minpos, tie = minimizers(bases, offsets, k)
    p = np.flatnonzero(valid)
    for border in (32, 2048, TILE):
        nxt = (p // border + 1) * border  # the next multiple after p
        assert ((nxt - p <= w - 1) & (minpos[p] >= nxt)).any(), (name, k, border)
    periodic = name == "low_complexity"  # (the leftmost of equal hashes lies within the first period of the window)
    if w - 1 >= 32 and not periodic:  # the minimizer a lane or more after the k-mer's start; the multiples of 32 in [p, minpos]
        assert (minpos[p] - p >= 32).any(), (name, k)
        assert (minpos[p] // 32 - (p + 31) // 32 + 1 >= 2).any(), (name, k)
    if w - 1 >= 33 and not periodic:  # two multiples of 32 in (p, minpos]: the hash comes from the lane after the next (impossible at W - 1 = 32)
        assert (minpos[p] // 32 - p // 32 >= 2).any(), (name, k)
    # a record's last k-mer in the final k - 1 positions of a tile whose read goes on: its has-successor bit (the start bit of
    # position p + k) lies in the halo
    starts = record_starts(valid, minpos)
    nxt_valid, nxt_start = np.concatenate([valid[1:], [False]]), np.concatenate([starts[1:], [False]])
    pos = np.arange(valid.size)
    assert (valid & nxt_valid & nxt_start & (pos % TILE >= TILE - (k - 1))).any(), (name, k)
    assert n_records_expected(valid, minpos) == int(np.count_nonzero(starts))
    if name == "three_tiles":
        at = set(int(x) for x in offsets[:-1])
        assert any(s and s % TILE == 0 for s in at) and any(s % TILE == 1 for s in at)
    if name == "low_complexity":  # equal hashes on both sides of a lane border, inside one window
        nxt = (p // 32 + 1) * 32
        assert (tie[p] & (nxt - p <= w - 1)).any(), (name, k)
    if name == "read_ends_on_border":  # the start bit that ends the read is bit 0 of the next tile's first word
        assert TILE in set(int(x) for x in offsets) and valid[TILE - k] and not valid[TILE - k + 1:TILE].any(), (name, k)
    return valid, minpos


@pytest.mark.parametrize("k", WIDE_KS)
@pytest.mark.parametrize("name", list(A_SETS))
def test_wide_inputs_exercise_the_borders(name, k):
    bases, offsets = a_set(name)
    assert bases.size <= 30_000
    if name != "low_complexity":
        assert 64 <= int(np.diff(offsets.astype(np.int64)).min()) and int(np.diff(offsets.astype(np.int64)).max()) <= 300
    assert {"two_tiles_exactly": bases.size == 2 * TILE, "two_tiles_and_a_byte": bases.size == 2 * TILE + 1,
            "not_a_multiple_of_16": bases.size % 16 != 0}.get(name, True)
    assert_wide_borders(name, k, bases, offsets)


SIZES = ("n_nodes", "n_edges", "n_kmer_instances", "n_edge_instances")  # (the table capacity depends on the engine)


def oracle_successors(want, k):
    """Rows (dict order) of the successors by code from the oracle's arrays: the node whose 2k-bit key is ((key << 2) | b) & mask
    wherever counts[:, b] != 0, -1 elsewhere.  Python integers."""
    full = [(int(h) << 64) | int(lo) for h, lo in zip(want["keys_hi"].tolist(), want["keys"].tolist())]
    row = {v: i for i, v in enumerate(full)}
    mask = (1 << (2 * k)) - 1
    out = np.full((len(full), 4), -1, dtype=np.int64)
    for i, b in zip(*(x.tolist() for x in np.nonzero(want["counts"]))):
        out[i, b] = row[((full[i] << 2) | b) & mask]
    return out


TABLE = ("keys", "keys_hi", "stamps", "counts", "succ")


@gpu
@pytest.mark.parametrize("k", WIDE_KS)
@pytest.mark.parametrize("name", list(A_SETS))
def test_wide_extraction_at_the_borders(name, k):
    bases, offsets = a_set(name)
    valid, minpos = assert_wide_borders(name, k, bases, offsets)
    got = build(bases, offsets, k)
    want = orc_c.build(bases, offsets, k)
    print(name, k, got["stats"], "expected records", n_records_expected(valid, minpos))
    for f in ("n_nodes", "n_kmer_instances", "n_edge_instances"):
        assert got["sizes"][f] == want[f], f
    for f in ("keys", "keys_hi", "stamps", "counts"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["succ"], oracle_successors(want, k)), "successors"
    for opts in (dict(extract_generic=1), dict(stamp64=1), dict(wcount_kernel=1), dict(wide_engine=0)):
        ref = build(bases, offsets, k, **opts)
        assert [got["sizes"][f] for f in SIZES] == [ref["sizes"][f] for f in SIZES], opts
        for f in TABLE:
            assert np.array_equal(got[f], ref[f]), (opts, f)
        if "wide_engine" not in opts:  # (the global-table engine has no records)
            assert got["stats"] == ref["stats"], opts
    # the two-word extraction has no pre-split, so no other record cut to fall back to: the count holds for every set
    assert got["stats"]["n_records"] == n_records_expected(valid, minpos)


# =========================================================================================================================
# B. the streaming traversal kernels and the global-table count kernels on planted inputs
# =========================================================================================================================
NARROW_KS, WIDE_B_KS = [21, 31], [32, 47, 63]
B_SETS = ["exact3", "ragged", "pairs_a", "pairs_b"]
B_TOTAL = {"exact3": 3 * TILE, "ragged": 2 * TILE + 6000 + 7, "pairs_a": 2 * TILE + 5000 + 3, "pairs_b": 2 * TILE + 5000 + 2}
FLANK = 40
B_ROWS = {
    "narrow": [(), (("refine_streaming", 1),), (("engine", 1),), (("stamp64", 1), ("refine_streaming", 1))],
    "wide": [(), (("wide_engine", 0),), (("stamp64", 1),), (("wcount_kernel", 1),)],
}


def kmer_int(b):
    v = 0
    for c in np.asarray(b).tolist():
        v = (v << 2) | ((c >> 1) & 3)
    return v


def plant(k, name):
    """-> bases, offsets and the plan: nodes (X / Y: k-mer, a, b, position of the first X -> a instance, whether the
    straddling instance is that first one), straddlers (read start, position of its one branch k-mer, d, border) and the
    reads of length k."""
    rng = np.random.default_rng(100 * k + B_SETS.index(name))
    total = B_TOTAL[name]
    rnd = lambda n: ACGT[rng.integers(0, 4, size=n)]  # noqa: E731
    fixed, nodes, straddlers, len_k = [], [], [], []
    cursor = [2 * TILE + 1000]  # "later, away from any border": the third tile, reads 70 bytes apart

    def pair(label):
        x = rnd(k)
        a, b = (ACGT[i] for i in rng.choice(4, size=2, replace=False))
        node = {"label": label, "x": x, "a": int(a), "b": int(b),
                "ra": np.concatenate([rnd(FLANK), x, [a], rnd(FLANK)]).astype(np.uint8),
                "rb": np.concatenate([rnd(FLANK), x, [b], rnd(FLANK)]).astype(np.uint8)}
        nodes.append(node)
        return node

    def at(start, read):
        fixed.append((int(start), np.asarray(read, dtype=np.uint8)))

    def later(read):
        at(cursor[0], read)
        cursor[0] += len(read) + 70

    def straddle(node, which, t0, d):  # the k-mer of read `which` starts at t0 - d
        at(t0 - d - FLANK, node[which])
        straddlers.append({"label": node["label"], "start": t0 - d - FLANK, "p": t0 - d, "d": d, "t0": t0, "first": which == "ra"})

    if name == "exact3":  # X ends on the first tile's last position; X as a read across the second border and as the last read
        x = pair("X")
        straddle(x, "ra", TILE, k)
        at(2 * TILE - k // 2, x["x"])
        len_k.append({"p": 2 * TILE - k // 2, "t0": 2 * TILE})
        for r in ("ra", "rb", "rb"):
            later(x[r])
        at(total - k, x["x"])
        len_k.append({"p": total - k, "t0": None})
    elif name == "ragged":  # X as a read that ENDS on the first tile's last position, the next read starts with b: a kernel
        x = pair("X")       # that misses the start bit at TILE sees X -> b there, before the first X -> a at 2 TILE - (k - 1)
        at(TILE - k, x["x"])
        len_k.append({"p": TILE - k, "t0": TILE})
        straddle(x, "ra", 2 * TILE, k - 1)
        for r in ("ra", "rb", "rb"):
            later(x[r])
        at(total - k, x["x"])
        len_k.append({"p": total - k, "t0": None})
    elif name == "pairs_a":
        x1, x2 = pair("X1"), pair("X2")
        straddle(x1, "ra", TILE, k // 2)
        straddle(x2, "ra", 2 * TILE, 1)
        for n in (x1, x2):
            for r in ("ra", "rb", "rb"):
                later(n[r])
    else:  # pairs_b: X starts on the second tile's first position; the control Y, seen early both ways, straddles later
        x, y = pair("X"), pair("Y")
        at(1000, y["ra"])
        at(1300, y["ra"])
        at(1600, y["rb"])
        straddle(x, "ra", TILE, 0)
        straddle(y, "rb", 2 * TILE, k)
        for r in ("ra", "rb", "rb"):
            later(x[r])
    bases, offsets = long_reads(int(rng.integers(1 << 30)), total, [(s, len(r)) for s, r in fixed])
    for s, r in fixed:
        bases[s:s + len(r)] = r
    if name == "ragged":
        bases[TILE] = nodes[0]["b"]
    for n in nodes:  # where its a-read and b-read first stand
        n["first_a"] = min(s for s, r in fixed if r is n["ra"]) + FLANK
        n["first_b"] = min(s for s, r in fixed if r is n["rb"]) + FLANK
    return frozen(bases, offsets) + ({"nodes": nodes, "straddlers": straddlers, "len_k": len_k},)


_b_cases = {}


def b_case(k, name):
    """The planted input, its C oracle and the oracle's traversal at threshold 2: made once, shared, left unchanged."""
    if (k, name) not in _b_cases:
        bases, offsets, plan = plant(k, name)
        o = orc_c.Oracle(bases, offsets, k)
        t = o.traverse(2)
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _b_cases[(k, name)] = {"bases": bases, "offsets": offsets, "plan": plan, "oracle": o, "t": t}
    return _b_cases[(k, name)]


@pytest.fixture(scope="module", autouse=True)
def _close_oracles():
    yield
    for c in list(_b_cases.values()) + ([_crowd] if _crowd else []):
        c["oracle"].close()
    _b_cases.clear()
    _crowd.clear()


def assert_plant(k, name):
    c = b_case(k, name)
    bases, offsets, plan, o, t = c["bases"], c["offsets"], c["plan"], c["oracle"], c["t"]
    n = bases.size
    assert n == B_TOTAL[name] <= 30_000
    assert {"exact3": n == 3 * TILE, "ragged": n % 16 != 0}.get(name, True)
    keys, hi, _, counts = o.nodes()
    full = [(int(h) << 64) | int(lo) for h, lo in zip(hi.tolist(), keys.tolist())]
    row = {v: i for i, v in enumerate(full)}
    branch = {full[i] for i in t["branch"].tolist()}
    # X and Y are the branch nodes and no chance repeat made another; the order byte ranks a before b on equal counts
    assert branch == {kmer_int(nd["x"]) for nd in plan["nodes"]}, (k, name)
    for nd in plan["nodes"]:
        i = row[kmer_int(nd["x"])]
        a, b = (nd["a"] >> 1) & 3, (nd["b"] >> 1) & 3
        assert counts[i, a] == counts[i, b] == 2 and int((counts[i] != 0).sum()) == 2
        assert int(t["order"][i]) & 3 == a and (int(t["order"][i]) >> 2) & 3 == b, (k, name, nd["label"])
        assert nd["first_a"] < nd["first_b"]
        assert bytes(bases[nd["first_a"]:nd["first_a"] + k + 1]) == bytes(nd["x"]) + bytes([nd["a"]])
    starts = offsets.astype(np.int64)

    def only_branch_kmer(read, p):  # the read's k-mers against the branch keys: one hit, at p
        s, e = int(starts[read]), int(starts[read + 1])
        hits = [q for q in range(s, e - k + 1) if kmer_int(bases[q:q + k]) in branch]
        assert hits == [p], (k, name, read, hits, p)
        assert t["read_flags"][read] == 1

    for st in plan["straddlers"]:
        read = int(np.searchsorted(starts, st["start"], side="right")) - 1
        assert starts[read] == st["start"] and starts[read] < st["t0"] <= starts[read + 1]
        only_branch_kmer(read, st["p"])
        nd = next(x for x in plan["nodes"] if x["label"] == st["label"])
        assert (st["p"] == nd["first_a"]) == st["first"]  # X: the straddling instance is the first X -> a; Y: it is not
        if not st["first"]:
            assert st["p"] > nd["first_a"] and st["p"] > nd["first_b"]
    for lk in plan["len_k"]:
        read = int(np.searchsorted(starts, lk["p"], side="right")) - 1
        assert starts[read] == lk["p"] and starts[read + 1] - starts[read] == k
        only_branch_kmer(read, lk["p"])
    if plan["len_k"]:
        assert plan["len_k"][-1]["p"] + k == n and int(starts[-2]) == n - k  # the last read of the data
    if name == "exact3":  # one read of length k across the border
        assert plan["len_k"][0]["p"] < 2 * TILE < plan["len_k"][0]["p"] + k
    if name == "ragged":  # one that ends with the tile, followed by b, before X -> a is first seen
        nd = plan["nodes"][0]
        assert plan["len_k"][0]["p"] + k == TILE and bases[TILE] == nd["b"] and TILE < nd["first_a"]
    return c


@pytest.mark.parametrize("k", NARROW_KS + WIDE_B_KS)
@pytest.mark.parametrize("name", B_SETS)
def test_planted_inputs_are_what_they_claim(name, k):
    assert_plant(k, name)


@pytest.mark.parametrize("k", NARROW_KS + WIDE_B_KS)
def test_planted_instances_sit_at_every_distance(k):
    seen = {(st["d"], st["t0"]) for name in B_SETS for st in plant(k, name)[2]["straddlers"] if st["first"]}
    assert {d for d, _ in seen} >= {k, k - 1, k // 2, 1, 0}
    assert {t0 for _, t0 in seen} == {TILE, 2 * TILE}


def b_params():
    for k in NARROW_KS + WIDE_B_KS:
        for name in B_SETS:
            for options in B_ROWS["narrow" if k <= 31 else "wide"]:
                yield pytest.param(k, name, options, id=f"k{k}-{name}-" + ("default" if not options else "-".join(f"{n}{v}" for n, v in options)))


@gpu
@pytest.mark.parametrize("k,name,options", list(b_params()))
def test_planted_traversal_equals_c_oracle(k, name, options):
    c = assert_plant(k, name)
    g, dev = device_traversal(c["bases"], c["offsets"], k, 2, options=options)
    try:
        compare(c["oracle"], c["t"], dev, k)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("k", NARROW_KS)
@pytest.mark.parametrize("name", B_SETS)
def test_first_seen_bytes_per_range_and_streaming(name, k):
    """export_orders()'s first-seen byte of X and Y: from the bucket's records and from the pass over the reads."""
    c = assert_plant(k, name)
    want = {kmer_int(nd["x"]): [(nd["a"] >> 1) & 3, (nd["b"] >> 1) & 3] for nd in c["plan"]["nodes"]}
    got = []
    for streaming in (0, 1):
        g = _dbg.Graph()
        try:
            g.set_option("refine_streaming", streaming)
            g.set_reads(c["bases"], c["offsets"])
            g.build(k)
            g.refine_edge_order()
            keys = g.export_nodes()[0]
            fs = g.export_orders()[1]
            rows = {int(key): fs[i, :2].tolist() for i, key in enumerate(keys.tolist()) if int(key) in want}
            assert g.stats()["refine_crowded"] == 0
        finally:
            g.close()
        assert rows == want, (streaming, rows, want)
        got.append(rows)
    assert got[0] == got[1]


# =========================================================================================================================
# B'. k_ws_extract: the k-mer instances a rank of a sharded build sends at k >= 32 on the global-table engine
# =========================================================================================================================
WS_CASES = [("plant", name, k) for name in B_SETS for k in WIDE_B_KS] + \
           [("searched", name, k) for name in ("two_tiles_exactly", "not_a_multiple_of_16", "read_ends_on_border") for k in (32, 63)]


def ws_input(kind, name, k):
    return plant(k, name)[:2] if kind == "plant" else a_set(name)


def instances_expected(bases, offsets, k):
    """Every k-mer instance of the reads longer than k, in position order, as k_ws_extract writes it: the low and high key word,
    the base after it (code; 0 where the read ends), the has-successor bit and the stamp (position << 1 | not at a read's
    start).  numpy; tied to the C oracle by test_instances_expected_equal_the_c_oracle."""
    code = ((bases >> 1) & 3).astype(np.uint64)
    pos, first, succ = [], [], []
    for s, e in zip(offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)):
        if e - s > k:
            q = np.arange(s, e - k + 1)
            pos.append(q)
            first.append(q == s)
            succ.append(q + k < e)
    pos, first, succ = np.concatenate(pos), np.concatenate(first), np.concatenate(succ)
    lo, hi = np.zeros(pos.size, dtype=np.uint64), np.zeros(pos.size, dtype=np.uint64)
    for i in range(k):  # base i of the k-mer stands 2 (k - 1 - i) bits above the least significant one
        sh = 2 * (k - 1 - i)
        if sh >= 64:
            hi |= code[pos + i] << np.uint64(sh - 64)
        else:
            lo |= code[pos + i] << np.uint64(sh)
    nxt = np.where(succ, code[np.minimum(pos + k, bases.size - 1)], np.uint64(0))
    stamp = (pos.astype(np.uint64) << np.uint64(1)) | (~first).astype(np.uint64)
    return {"lo": lo, "hi": hi, "next": nxt, "has_succ": succ.astype(np.uint64), "stamp": stamp}


@pytest.mark.parametrize("kind,name,k", WS_CASES)
def test_instances_expected_equal_the_c_oracle(kind, name, k):
    bases, offsets = ws_input(kind, name, k)
    exp = instances_expected(bases, offsets, k)
    want = orc_c.build(bases, offsets, k)
    assert exp["stamp"].size == want["n_kmer_instances"] and int(exp["has_succ"].sum()) == want["n_edge_instances"]
    keys = np.stack([exp["hi"], exp["lo"]], axis=1)
    _, firsts = np.unique(keys, axis=0, return_index=True)  # (the instances are in position order: the first index is the first seen)
    firsts.sort()
    assert np.array_equal(exp["lo"][firsts], want["keys"]) and np.array_equal(exp["hi"][firsts], want["keys_hi"])
    assert np.array_equal(exp["stamp"][firsts], want["stamps"])
    counts = np.zeros((firsts.size, 4), dtype=np.uint32)
    row = {kk: i for i, kk in enumerate(zip(want["keys_hi"].tolist(), want["keys"].tolist()))}
    has = exp["has_succ"] != 0
    rows = np.array([row[kk] for kk in zip(exp["hi"][has].tolist(), exp["lo"][has].tolist())], dtype=np.int64)
    np.add.at(counts, (rows, exp["next"][has].astype(np.int64)), 1)
    assert np.array_equal(counts, want["counts"])
    # an instance whose k-mer ends with a tile and one that starts a tile; in the planted sets the reads of length k send nothing
    p = (exp["stamp"] >> np.uint64(1)).astype(np.int64)
    assert ((p + k) % TILE == 0).any() and (p % TILE == 0).any() and ((p % TILE > TILE - k) & (exp["has_succ"] != 0)).any()
    if kind == "plant":
        lens = np.diff(offsets.astype(np.int64))
        starts_of_len_k = offsets[:-1][lens == k].astype(np.int64)
        assert (name in ("exact3", "ragged")) == bool(starts_of_len_k.size) and not np.isin(starts_of_len_k, p).any()


@gpu
@pytest.mark.parametrize("n_shards", [1, 4])
@pytest.mark.parametrize("kind,name,k", WS_CASES)
def test_shard_instances_at_the_borders(kind, name, k, n_shards):
    """dbg_shard_extract under wide_engine=0 (k_ws_extract, both passes): every instance once, with its key words, next base,
    has-successor bit and stamp; equal k-mers go to one owner."""
    bases, offsets = ws_input(kind, name, k)
    exp = instances_expected(bases, offsets, k)
    g = _dbg.Graph()
    try:
        g.set_option("wide_engine", 0)
        g.set_reads(bases, offsets)
        counts, arrays = g.shard_extract(k, n_shards)
        assert g.shard_record_layout() == (1, 8)
        t_lo, t_hi, t_st = (a.cpu().numpy().view(np.uint64) for a in arrays)
        sz = g.sizes()
    finally:
        g.close()
    assert len(counts) == n_shards and sum(counts) == exp["stamp"].size == t_lo.size == t_hi.size == t_st.size
    assert sz["n_kmer_instances"] == exp["stamp"].size and sz["n_edge_instances"] == int(exp["has_succ"].sum())
    owner = np.repeat(np.arange(n_shards), counts)
    o = np.argsort(t_st & np.uint64(0xFFFFFFFF), kind="stable")  # rank-local stamps are below 2^32 and distinct: position order
    t_lo, t_hi, t_st, owner = t_lo[o], t_hi[o], t_st[o], owner[o]
    assert np.array_equal(t_st, exp["stamp"] | (exp["has_succ"] << np.uint64(32))), "stamps / has-successor bits"
    assert np.array_equal(t_lo, exp["lo"]) and np.array_equal(t_hi & np.uint64((1 << 62) - 1), exp["hi"]), "key words"
    has = exp["has_succ"] != 0
    assert np.array_equal((t_hi >> np.uint64(62))[has], exp["next"][has]), "next bases"
    _, kid = np.unique(np.stack([exp["hi"], exp["lo"]], axis=1), axis=0, return_inverse=True)
    kid = kid.reshape(-1)
    first_owner = np.full(int(kid.max()) + 1, -1, dtype=np.int64)
    first_owner[kid[::-1]] = owner[::-1]
    assert np.array_equal(first_owner[kid], owner), "one owner per k-mer"
    if n_shards > 1:
        assert min(counts) > 0


# =========================================================================================================================
# C. the crowded fallback
# =========================================================================================================================
CROWD_K, CROWD_BYTES = 6, 25_000
_crowd = {}


def crowd_case():
    """Uniform reads at k = 6: nearly every 6-mer exists and nearly every one has several successors, far more than the RF_SLOTS / 2 =
    512 multi-successor (k_sk_refine) or branch (k_sk_pull) nodes a range may hold, however two buckets are cut into ranges."""
    if not _crowd:
        bases, offsets = frozen(*long_reads(6, CROWD_BYTES))
        o = orc_c.Oracle(bases, offsets, CROWD_K)
        _crowd.update(bases=bases, offsets=offsets, oracle=o, t=o.traverse(2))
    return _crowd


def test_crowd_input_crowds():
    c = crowd_case()
    counts = c["oracle"].nodes()[3]
    assert 4000 < c["oracle"].n_nodes <= 4 ** CROWD_K
    assert int(((counts != 0).sum(axis=1) >= 2).sum()) > 3500 and c["t"]["branch"].size > 3000  # (3 933 and 3 309)


@gpu
@pytest.mark.parametrize("streaming", [0, 1])
def test_crowded_ranges_fall_back_to_the_pass_over_the_reads(streaming):
    c = crowd_case()
    g, dev = device_traversal(c["bases"], c["offsets"], CROWD_K, 2, options=(("bucket_bits", 1), ("refine_streaming", streaming)))
    try:
        st = g.stats()
        print("records", st["n_records"], "buckets", st["n_buckets"], "refine_crowded", st["refine_crowded"], "pull_crowded", st["pull_crowded"])
        if streaming:
            assert st["refine_crowded"] == 0 and st["pull_crowded"] == 0
        else:
            assert st["n_records"] > 0 and st["refine_crowded"] == 1 and st["pull_crowded"] == 1
        compare(c["oracle"], c["t"], dev, CROWD_K)
    finally:
        g.close()


# =========================================================================================================================
# D. one byte outside ACGT
# =========================================================================================================================
BAD_KS = [5, 21, 31, 32, 63]
BAD_BYTES = {"N": ord("N"), "a": ord("a"), "0xC1": 0xC1}  # 'a' and 0xC1 pack like 'A': only the `bad` flag tells them apart
WORD256 = 256 * 16  # byte of 16-byte word 256 of a tile: the first word of the block's second round of loads


def bad_positions(name):
    """label -> position in the set, and the shortest k of BAD_KS (or None) for which the position lies in a read shorter than k."""
    bases, offsets = read_set(name)
    n = bases.size
    out = {"first": 0, "tile_last": TILE - 1, "tile_first": TILE, "word256_first": TILE + WORD256, "word256_last": TILE + WORD256 + 15}
    assert n % 16 != 0  # both sets end in a partial 16-byte word
    out["data_last"] = n - 1
    lens = np.diff(offsets.astype(np.int64))
    short = int(np.argmin(lens))
    out["short_read"] = int(offsets[short]) + int(lens[short]) // 2
    return out, int(lens[short])


BAD_SETS = ["three_tiles", "not_a_multiple_of_16"]
BAD_LABELS = ["first", "tile_last", "tile_first", "word256_first", "word256_last", "data_last", "short_read"]


def bad_input(name, label, byte):
    bases, offsets = read_set(name)
    pos, shortest = bad_positions(name)
    b = bases.copy()
    b[pos[label]] = byte
    return b, offsets, pos[label], shortest


@pytest.mark.parametrize("name", BAD_SETS)
def test_bad_byte_positions(name):
    bases, offsets = read_set(name)
    pos, shortest = bad_positions(name)
    assert sorted(pos) == sorted(BAD_LABELS) and len(set(pos.values())) == len(pos) and max(pos.values()) == bases.size - 1
    assert shortest < 63  # at k = 63 (and whenever k is larger than it) "short_read" lies in a read without a k-mer
    for byte in BAD_BYTES.values():
        assert byte not in b"ACGT"
    assert (ord("a") >> 1) & 3 == (ord("A") >> 1) & 3 == (0xC1 >> 1) & 3


@gpu
@pytest.mark.parametrize("byte", list(BAD_BYTES))
@pytest.mark.parametrize("label", BAD_LABELS)
@pytest.mark.parametrize("name", BAD_SETS)
def test_one_byte_outside_acgt_takes_the_generic_engine(name, label, byte):
    bases, offsets, p, shortest = bad_input(name, label, BAD_BYTES[byte])
    for k in BAD_KS:
        ref = table_reference(bases, offsets, k)
        if label == "short_read" and k > shortest:  # the byte is in no k-mer: the graph is that of the clean reads
            assert ref["n_kmer_instances"] == table_reference(read_set(name)[0], offsets, k)["n_kmer_instances"]
        for generic in (0, 1):
            g = _dbg.Graph()
            try:
                g.set_option("extract_generic", generic)
                g.set_reads(bases, offsets)
                g.build(k)
                sz = g.sizes()
            finally:
                g.close()
            assert sz["max_degree"] == GENERIC_DEGREE != 4, (k, generic)
            assert sz["n_nodes"] == ref["kmers"].shape[0] and sz["n_kmer_instances"] == ref["n_kmer_instances"], (k, generic)
