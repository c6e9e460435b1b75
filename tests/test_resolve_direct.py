"""Option "resolve_direct": the resolver of a single-GPU build names a cross-bucket successor from the directory entry of its
home slot alone where dir_decide (csrc/dbg_dir.h) can, and reads no key for it.  The graph must not depend on the option:
every comparison here is independent of the order in which the table holds its nodes (nodes sorted by k-mer, successors
named by the successor's stamp).

The C oracle of the default build: orc_c.build_mt (totals and node digest) at k = 31; it takes k <= 31 only, so at k = 63
the same totals and the same digest come from orc_c.build's arrays (orc_c.digest), and the high key words are compared too.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _dbg
import inproc_dist
import synth
from oracle import orc_c

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")
READ_LEN = 100
SEED = 5
NO_NODE = np.uint32(0xFFFFFFFF)


# ---- the decision function on the host ----------------------------------------------------------------------------------
def test_decision_function_on_the_host(tmp_path):
    """tests/resolve_direct_host.cpp: includes only dbg_dir.h, built with the host compiler, run once."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "resolve_direct_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, os.path.join(HERE, "resolve_direct_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout


# ---- builds -------------------------------------------------------------------------------------------------------------
def graph_of(g):
    """(keys, high key words, stamps, counts, successor stamps) by ascending k-mer, and sizes()."""
    keys, stamps, counts, _ = g.export_nodes()
    keys_hi = g.export_keys_hi() if g.sizes()["k"] > 31 else np.zeros_like(keys)
    succ = g.export_succ()
    o = np.lexsort((keys, keys_hi))
    present = succ != NO_NODE
    succ_stamps = np.where(present, stamps[np.where(present, succ, 0)].astype(np.int64), np.int64(-1))
    return {"keys": keys[o], "keys_hi": keys_hi[o], "stamps": stamps[o], "counts": counts[o], "succ_stamps": succ_stamps[o],
            "sizes": g.sizes()}


def assert_same_nodes(a, b):
    for f in ("keys", "keys_hi", "stamps", "counts", "succ_stamps"):
        assert np.array_equal(a[f], b[f]), f


def assert_same_graph(a, b):
    """Two builds that differ in the resolver alone."""
    assert a["sizes"] == b["sizes"]
    assert a["n_queries"] == b["n_queries"] and a["n_buckets"] == b["n_buckets"]
    assert_same_nodes(a, b)


def build(bases, offsets, k, direct=None, count=False, **opts):
    """The graph of a fresh handle's one build; with count, the resolver's counting instantiation and its two counters."""
    g = _dbg.Graph()
    try:
        for name, v in opts.items():
            g.set_option(name, v)
        if direct is not None:
            g.set_option("resolve_direct", direct)
        if count:
            g.set_option("resolve_count", 1)
        g.set_reads(bases, offsets)
        g.build(k)
        gr = graph_of(g)
        st = g.stats()
        gr.update(n_queries=st["n_queries"], n_buckets=st["n_buckets"], hits=st["resolve_direct_hits"], keyed=st["resolve_keyed"])
        return gr
    finally:
        g.close()


@pytest.fixture(scope="module")
def synth_set():
    """20 000 reads x 100 bp of a 200 kbp genome, 1 % errors: 2 MB (the set of tests/test_extract_presplit.py)."""
    reads = synth.reads_ascii(SEED, 200_000, 20_000, READ_LEN, 0.01)
    bases = np.ascontiguousarray(reads.reshape(-1))
    bases.setflags(write=False)
    return bases, np.arange(0, bases.size + 1, READ_LEN, dtype=np.uint64)


_verified = {}


def verified(synth_set, k):
    """The resolve_direct = 0 graph (every query compares its key) of the default geometry, built once per k."""
    if k not in _verified:
        _verified[k] = build(*synth_set, k, direct=0, count=True)
    return _verified[k]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [13, 21, 31, 40, 63])  # one-word and two-word k-mers
def test_same_graph_with_and_without_the_shortcut(synth_set, k):
    ref = verified(synth_set, k)
    got = build(*synth_set, k, direct=1, count=True)
    assert_same_graph(got, ref)
    assert ref["hits"] == 0 and ref["keyed"] == ref["n_queries"]
    assert_same_graph(build(*synth_set, k, direct=1), ref)  # the instantiation that carries no counting


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_default_equals_the_c_oracle(synth_set, k):
    bases, offsets = synth_set
    gr = build(bases, offsets, k)
    sz = gr["sizes"]
    if k <= 31:
        mt = orc_c.build_mt(bases, offsets, k, 4)
    else:
        want = orc_c.build(bases, offsets, k)
        mt = {"n_nodes": want["n_nodes"], "n_edges": int(np.count_nonzero(want["counts"])),
              "n_kmer_instances": want["n_kmer_instances"], "n_edge_instances": want["n_edge_instances"],
              "digest": orc_c.digest(want["keys"], want["stamps"], want["counts"])}
        o = np.argsort(gr["stamps"], kind="stable")  # the oracle's dict order: ascending first occurrence
        assert np.array_equal(gr["keys_hi"][o], want["keys_hi"])
    for f in ("n_nodes", "n_edges", "n_kmer_instances", "n_edge_instances"):
        assert sz[f] == mt[f], f
    assert orc_c.digest(gr["keys"], gr["stamps"], gr["counts"]) == mt["digest"]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_both_paths_run(synth_set, k):
    """Default geometry, counting instantiation: every query is counted once, and each path takes at least a tenth (random
    linear probing decides 0.38 .. 0.52 of the keys from the mask at the fills the geometry aims at)."""
    got = build(*synth_set, k, count=True)
    n_q = got["n_queries"]
    print(f"k {k}: {n_q} queries, {got['hits']} direct, {got['keyed']} keyed, share {got['hits'] / max(n_q, 1):.3f}")
    assert n_q > 10_000
    assert got["hits"] + got["keyed"] == n_q
    assert got["hits"] >= n_q / 10 and got["keyed"] >= n_q / 10


GEOMETRIES = [
    # tables half to three-quarters full: runs across a block's end and around slot CAP - 1 -> 0, blocks of more than 31 nodes
    dict(bucket_bits=8),
    dict(bucket_bits=9, lds_slots=2048),
    dict(bucket_bits=3),    # every table overflows and is counted in hash sub-ranges: the verifying path
    dict(bucket_bits=22),   # three multisplit levels
]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", GEOMETRIES, ids=lambda o: "-".join(f"{n}{v}" for n, v in o.items()))
def test_geometries_that_stress_the_decision(synth_set, opts):
    k = 31
    ref = build(*synth_set, k, direct=0, **opts)
    got = build(*synth_set, k, direct=1, count=True, **opts)
    assert_same_graph(got, ref)
    assert_same_nodes(got, verified(synth_set, k))  # nor does the geometry change the graph
    assert got["hits"] + got["keyed"] == got["n_queries"]
    fill = got["sizes"]["n_nodes"] / (got["n_buckets"] * opts.get("lds_slots", 4096))
    print(opts, "buckets", got["n_buckets"], "mean fill", round(fill, 3), "direct", got["hits"], "keyed", got["keyed"])
    if opts["bucket_bits"] in (8, 9):
        assert 0.5 <= fill <= 0.75  # the input does what the case needs
        assert got["hits"] > 0 and got["keyed"] > 0
    if opts["bucket_bits"] == 3:
        assert got["hits"] == 0  # no bucket is one range: no directory is marked as a whole bucket's


@pytest.mark.gpu
@pytest.mark.parametrize("k,opts", [(31, dict(count_kernel=1)), (31, dict(count_kernel=2)), (31, dict(count_kernel=3)),
                                    (31, dict(stamp64=1)), (31, dict(stamp64=1, count_kernel_u64=1)),
                                    (31, dict(stamp64=1, count_kernel_u64=2)), (63, dict(wcount_kernel=1)),
                                    (63, dict(stamp64=1))],
                         ids=lambda v: "-".join(f"{n}{x}" for n, x in v.items()) if isinstance(v, dict) else str(v))
def test_every_count_kernel_feeds_the_shortcut(synth_set, k, opts):
    """Whichever kernel wrote the directory, the resolver that trusts it gives the graph of the one that compares keys."""
    ref = build(*synth_set, k, direct=0, **opts)
    got = build(*synth_set, k, direct=1, count=True, **opts)
    assert_same_graph(got, ref)
    assert_same_nodes(got, verified(synth_set, k))  # the stamp width and the count kernel change nothing a caller sees
    assert got["hits"] > 0 and got["hits"] + got["keyed"] == got["n_queries"]


@pytest.mark.gpu
def test_sharded_build_keeps_the_verifying_path(synth_set):
    """Two shards in one process (two handles on cuda:0, multi_gpu.sharded_build over an in-process exchange), k = 31: the
    union of the shards is the single-GPU graph under both option values, and neither the shards' own resolver nor the
    answer stage (queries of the other rank) takes the shortcut."""
    import multi_gpu
    k, per = 31, 4000
    bases, _ = synth_set
    part = bases[:2 * per * READ_LEN]
    offsets = np.arange(0, part.size + 1, READ_LEN, dtype=np.uint64)

    def sharded(direct):
        def one(dist, rank):
            g = _dbg.Graph(device=0)
            try:
                g.set_option("resolve_direct", direct)
                g.set_option("resolve_count", 1)
                mine = part[rank * per * READ_LEN:(rank + 1) * per * READ_LEN]
                g.set_reads(mine, np.arange(0, mine.size + 1, READ_LEN, dtype=np.uint64))
                multi_gpu.sharded_build(g, k, dist)
                keys, stamps, counts, _ = g.export_nodes()
                st = g.stats()
                return {"keys": keys, "stamps": stamps, "counts": counts, "succ": g.export_succ(),
                        "hits": st["resolve_direct_hits"], "keyed": st["resolve_keyed"]}
            finally:
                g.close()
        shards = inproc_dist.run_ranks(2, one)
        for s in shards:
            assert s["hits"] == 0 and s["keyed"] > 0
        succ_stamps = []
        for s in shards:  # successor ids of a shard: (owner << 29) | id on the owner
            present = s["succ"] != NO_NODE
            owner, idx = np.where(present, s["succ"] >> 29, 0), np.where(present, s["succ"] & ((1 << 29) - 1), 0)
            ss = np.full(s["succ"].shape, -1, dtype=np.int64)
            for d in range(2):
                sel = present & (owner == d)
                ss[sel] = shards[d]["stamps"][idx[sel]].astype(np.int64)
            succ_stamps.append(ss)
        keys = np.concatenate([s["keys"] for s in shards])
        o = np.argsort(keys, kind="stable")
        return {"keys": keys[o], "stamps": np.concatenate([s["stamps"] for s in shards])[o],
                "counts": np.concatenate([s["counts"] for s in shards])[o], "succ_stamps": np.concatenate(succ_stamps)[o]}

    single = build(part, offsets, k, direct=1)
    for direct in (0, 1):
        got = sharded(direct)
        for f in ("keys", "stamps", "counts", "succ_stamps"):
            assert np.array_equal(got[f], single[f]), (direct, f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["resolve_direct", "resolve_count"])
@pytest.mark.parametrize("value", [2, -1])
def test_option_range(name, value):
    g = _dbg.Graph()
    try:
        with pytest.raises(_dbg.DbgError) as e:
            g.set_option(name, value)
        assert e.value.code == _dbg.DBG_E_ARG
        g.set_option(name, 1)
        g.set_option(name, 0)
    finally:
        g.close()
