"""The HIP traversal (prune, branch list, tip removal, pull-out reads, walk, contig scores and the score sort) against the
C oracle's single-threaded restatement (oracle/dbg_oracle.c, orc_traverse; pinned to the Python oracle by
tests/test_oracle_c.py) at sizes the golden vectors cannot reach: dense branches at 3x coverage, long chains at 30x,
small k, two-word keys, several thresholds, the options that select other kernels, mixed read lengths, the final walk,
and a build in parts."""
import resource
import time

import numpy as np
import pytest

import _dbg
import synth
from oracle import orc_c

pytestmark = pytest.mark.gpu

READ_LEN = 150
CODE_SHIFT = np.array([0, 2, 4, 6], dtype=np.uint8)


def config1_reads(n):
    """The first n reads of BASELINE configs[1] (10 M x 150 bp, 1 % errors, 30x of a 50 Mbp genome, seed 1)."""
    g = _dbg.Graph()
    g.synth_reads(1, 50_000_000, n, READ_LEN, 0.01)
    bases, off = g.copy_reads()
    g.close()
    return bases, off


def synth_reads(seed, genome_len, n, read_len=READ_LEN, err=0.01):
    r = synth.reads_ascii(seed, genome_len, n, read_len, err)
    return r.reshape(-1), np.arange(0, r.size + 1, read_len, dtype=np.uint64)


def mixed_reads(k):
    """Host-built offsets over synthetic bases: lengths k - 1, k, k + 1 (pull-out reads and indegree edges at the
    borders of the rule len > k) mixed with 60, 150 and 400."""
    bases, _ = synth_reads(31, 2_000_000, 200_000, 100, 0.01)
    rng = np.random.default_rng(5)
    lens = rng.choice(np.array([k - 1, k, k + 1, 60, 150, 400], dtype=np.uint64), size=bases.size // 60)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    off = off[off <= bases.size]
    return np.ascontiguousarray(bases[:int(off[-1])]), off


READ_SETS = {
    "cfg1_1m": lambda: config1_reads(1_000_000),                   # 3x coverage: dense branches, tips, reservation conflicts
    "g5m_1m": lambda: synth_reads(2, 5_000_000, 1_000_000),        # 30x: the benchmarked regime, long chains
    "g2m_300k": lambda: synth_reads(3, 2_000_000, 300_000),        # 22x
    "g10m_300k": lambda: synth_reads(4, 10_000_000, 300_000),      # 4.5x
    "mixed": lambda: mixed_reads(31),
    "final_20k": lambda: synth_reads(7, 400_000, 20_000, 100, 0.001),
}

_cache = {}


def oracle_for(reads_name, k):
    """One C build per (read set, k) for the whole module; the previous one is freed first (host memory)."""
    key = (reads_name, k)
    if key not in _cache:
        for o in _cache.values():
            o["oracle"].close()
        _cache.clear()
        bases, off = READ_SETS[reads_name]()
        t0 = time.time()
        o = orc_c.Oracle(bases, off, k)
        _cache[key] = {"oracle": o, "bases": bases, "off": off, "build_s": time.time() - t0}
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _free_oracles():
    yield
    for o in _cache.values():
        o["oracle"].close()
    _cache.clear()


def device_traversal(bases, off, k, threshold, final=False, options=(), max_chars=0):
    """The single-handle path (as test_part_traversal.single_gpu_reference) with every intermediate export."""
    g = _dbg.Graph()
    for name, value in options:
        g.set_option(name, value)
    g.set_reads(bases, off)
    g.build(k)
    g.refine_edge_order()
    g.prune(threshold)
    g.remove_tips()
    g.mark_pull_reads()
    keys, stamps, counts, flags = g.export_nodes()
    out = {"keys": keys, "hi": g.export_keys_hi(), "stamps": stamps, "counts": counts, "flags": flags,
           "keep": g.export_keepmask(), "order": g.export_orders()[0], "ranks": g.export_pull_ranks(),
           "read_flags": g.export_pull_reads()}
    g.walk(final, max_chars)
    out["contig_off"], out["score"], out["stamp"], out["seq"] = g.export_contig_index()
    out["materialised"] = g.sizes()["contigs_materialised"]
    return g, out


NODE_SLICE = 1 << 23


def take(dev, name):
    """A device export, removed from dev (so that it is freed after use); a callable entry is exported only now."""
    v = dev.pop(name)
    return v() if callable(v) else v


def compare(o, t, dev, k):
    """Everything the device exported against orc_traverse's result t, exactly.  -> device contig indices in the
    oracle's emission order.  The node table is compared in slices of the oracle's dict order and the device's copy of
    each device array is dropped after use, so that the host holds one node table (the oracle's) and not three."""
    stamps = take(dev, "stamps")
    assert stamps.size == o.n_nodes, "node counts differ"
    d = np.argsort(stamps, kind="stable")                           # device table order -> dict order
    outdeg = np.empty(o.n_nodes, dtype=np.uint8)
    for field, col in (("stamps", 2), ("keys", 0), ("hi", 1), ("counts", 3)):   # one device array held at a time
        arr = stamps if field == "stamps" else take(dev, field)
        for lo in range(0, o.n_nodes, NODE_SLICE):
            want = o.nodes(lo, lo + NODE_SLICE)[col]
            assert np.array_equal(arr[d[lo:lo + want.shape[0]]], want), f"{field} differ"
            if field == "counts":
                outdeg[lo:lo + want.shape[0]] = (want != 0).sum(axis=1)
        del arr
    del stamps
    assert np.array_equal(take(dev, "keep")[d].astype(np.uint8), t["keep"]), "keep masks differ"
    want_rank = (t["order"][:, None] >> CODE_SHIFT[None, :]) & 3
    ranked = np.arange(4)[None, :] < outdeg[:, None]                # ranks beyond the out-degree carry nothing
    assert np.array_equal(np.where(ranked, take(dev, "order")[d], 0), np.where(ranked, want_rank, 0)), "successor ranks differ"
    del want_rank, ranked
    fl = take(dev, "flags")[d]
    assert np.array_equal(np.nonzero(fl & _dbg.F_BRANCH)[0], t["branch"]), "branch_kmer differs"
    pu = np.nonzero(fl & _dbg.F_PULLED)[0]
    pu = pu[np.argsort(take(dev, "ranks")[d][pu], kind="stable")]
    assert np.array_equal(pu, t["pulled"]), "already_pull_out differs (set or order)"
    assert np.array_equal(take(dev, "read_flags"), t["read_flags"]), "pull_out_read differs"
    c = np.lexsort((dev["seq"], dev["stamp"]))
    lens = (dev["contig_off"][1:] - dev["contig_off"][:-1])
    assert c.size == t["score"].size, "contig counts differ"
    assert np.array_equal(dev["stamp"][c], t["stamp"]) and np.array_equal(dev["seq"][c].astype(np.uint32), t["seq"])
    assert np.array_equal(lens[c], t["chars"]), "contig lengths differ"
    assert np.array_equal(dev["score"][c], t["score"]), "contig scores differ"
    return c


def compare_texts(o, g, t, c, n_pick=64):
    """The text of a spread of contigs (evenly spaced, the longest, the shortest)."""
    n = t["score"].size
    if not n:
        return
    pick = np.unique(np.concatenate([np.linspace(0, n - 1, n_pick).astype(np.int64),
                                     [int(np.argmax(t["chars"])), int(np.argmin(t["chars"]))]]))
    buf, off = o.spell(pick)
    for j, i in enumerate(pick.tolist()):
        assert g.export_contig_text(int(c[i]), int(t["chars"][i])) == buf[off[j]:off[j + 1]].tobytes(), f"contig {i} text"


def compare_sort(g, dev, t, c, min_ties=0):
    """LazyContigs.sort(reverse=True) and export_sorted_fasta's order against a stable descending sort of the oracle's
    scores (the driver's sequences.sort(key=getScore, reverse=True), II_assembleFromReads.py:64)."""
    import debruijn
    want = c[np.argsort(-t["score"].astype(np.int64), kind="stable")]
    ties = t["score"].size - np.unique(t["score"]).size
    assert ties >= min_ties, ties
    lazy = debruijn.LazyContigs(g, c, dev["contig_off"], dev["score"])
    lazy.sort(reverse=True)
    assert np.array_equal(np.asarray(lazy._order), want), "LazyContigs.sort order"
    if dev["materialised"]:
        _, order = g.export_sorted_fasta()
        assert np.array_equal(order.astype(np.int64), want), "export_sorted_fasta order"
    return ties


def report(name, o, t, oracle_s, device_s, extra=""):
    print(f"\n[{name}] nodes {o.n_nodes} branch {t['branch'].size} pulled {t['pulled'].size} pull_reads {t['n_pull_reads']} "
          f"contigs {t['score'].size} contig_chars {t['contig_chars']} oracle {oracle_s:.1f}s device {device_s:.1f}s "
          f"peak_rss {peak_rss_gb():.1f}GB {extra}")


def peak_rss_gb():
    """Most host memory this process has held so far (ru_maxrss is in KiB on Linux)."""
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20


def nonvacuous(t):
    assert t["branch"].size > 0 and t["pulled"].size > 0 and t["score"].size > 0 and t["n_pull_reads"] > 0


# (read set, k, threshold, device options, text+sort check)
CASES = [
    ("cfg1_1m", 31, 2, (), True),
    ("g5m_1m", 31, 2, (), True),
    ("g10m_300k", 15, 2, (), False),
    ("g10m_300k", 21, 2, (), False),
    ("g10m_300k", 32, 2, (), True),
    ("g10m_300k", 47, 2, (("wcount_kernel", 1),), False),   # non-default count kernel for two-word keys
    ("g10m_300k", 63, 2, (), True),
    ("mixed", 31, 2, (), True),
    ("g2m_300k", 31, 1, (), False),
    ("g2m_300k", 31, 1.5, (), False),
    ("g2m_300k", 31, 2, (("stamp64", 1),), False),
    ("g2m_300k", 31, 2, (("walk_jump_min_nodes", 0),), True),
    ("g2m_300k", 31, 2, (("walk_jump_min_nodes", 1 << 40),), False),
    ("g2m_300k", 31, 3, (("engine", 1),), False),             # the single global hash table build
    ("g2m_300k", 31, 5, (), False),
]


@pytest.mark.parametrize("reads_name,k,threshold,options,texts", CASES,
                         ids=[f"{c[0]}-k{c[1]}-t{c[2]}" + "".join(f"-{n}{v}" for n, v in c[3]) for c in CASES])
def test_traversal_equals_c_oracle(reads_name, k, threshold, options, texts):
    ent = oracle_for(reads_name, k)
    o = ent["oracle"]
    t0 = time.time()
    t = o.traverse(threshold)
    oracle_s = ent["build_s"] + time.time() - t0
    ent["build_s"] = 0.0
    # one thread per start (below walk_jump_min_nodes) always spells the text: room for this case's 4.3e9 characters
    max_chars = 1 << 33 if dict(options).get("walk_jump_min_nodes", 0) > o.n_nodes else 0
    t0 = time.time()
    g, dev = device_traversal(ent["bases"], ent["off"], k, threshold, options=options, max_chars=max_chars)
    device_s = time.time() - t0
    try:
        c = compare(o, t, dev, k)
        extra = f"max_contig {int(t['chars'].max())} mean_contig {float(t['chars'].mean()):.0f}"
        if texts:
            compare_texts(o, g, t, c)
            extra += f" score_ties {compare_sort(g, dev, t, c, min_ties=1000)}"
        report(f"{reads_name} k={k} thr={threshold} {dict(options)}", o, t, oracle_s, device_s, extra)
    finally:
        g.close()
    nonvacuous(t)
    if reads_name == "mixed":   # reads of length k take part in pull_out_read, shorter ones never do
        lens = np.diff(ent["off"])
        assert t["read_flags"][lens == k].any() and not t["read_flags"][lens < k].any()


def test_traversal_in_parts_equals_c_oracle():
    """A 4-pass build traversed through part_traversal (never one graph) against the oracle, not only against the
    single-handle path."""
    import part_traversal
    k, thr = 31, 2
    ent = oracle_for("g2m_300k", k)
    o = ent["oracle"]
    t = o.traverse(thr)
    keys, hi, stamps, _ = o.nodes()
    g = _dbg.Graph()
    g.set_reads(ent["bases"], ent["off"])
    t0 = time.time()
    g.build_multipass(k, 4)
    res = part_traversal.traverse(g, k, thr)
    device_s = time.time() - t0
    g.close()
    assert np.array_equal(res["branch"]["keys"].astype(np.uint64), keys[t["branch"]])
    assert np.array_equal(res["branch"]["keys_hi"].astype(np.uint64), hi[t["branch"]])
    assert np.array_equal(res["pulled"]["keys"], keys[t["pulled"]]) and np.array_equal(res["pulled"]["keys_hi"], hi[t["pulled"]])
    assert np.array_equal(res["read_flags"], t["read_flags"])
    assert np.array_equal(res["contigs"]["stamp"], t["stamp"])
    assert np.array_equal(res["contigs"]["length"], t["chars"].astype(np.int64))
    assert np.array_equal(res["contigs"]["score"], t["score"].astype(np.int64))
    nonvacuous(t)
    report("g2m_300k k=31 parts=4", o, t, 0.0, device_s)


def test_final_walk_equals_c_oracle():
    """Final mode (branch_kmer == []) beyond configs[0]: every simple path (debruijn.py:288-316) with branches present."""
    k, thr = 21, 2
    ent = oracle_for("final_20k", k)
    o = ent["oracle"]
    t0 = time.time()
    nf = o.traverse(thr)
    t = o.traverse(thr, final=True, max_paths=1_000_000)
    oracle_s = ent["build_s"] + time.time() - t0
    assert nf["branch"].size > 0 and t["score"].size > nf["score"].size   # branches multiply the paths
    t0 = time.time()
    g, dev = device_traversal(ent["bases"], ent["off"], k, thr, final=True)
    device_s = time.time() - t0
    try:
        c = compare(o, t, dev, k)
        compare_texts(o, g, t, c)
        compare_sort(g, dev, t, c)
        report("final_20k k=21 final", o, t, oracle_s, device_s)
    finally:
        g.close()
