"""dbg_count_spectrum on the device (run with -m gpu on an MI355X): the edge spectrum, the out-weight spectrum and the degree
distributions of every kind of graph a handle can hold, against the host statement of the definitions
(debruijn.count_spectrum on plain dicts) run on the Python oracle's dicts, unless a case names another yardstick."""
import contextlib
import copy
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _dbg
import debruijn as prod
import inproc_dist
from conftest import GOLDEN, PKG, case_reads, golden_case_names, load_golden
from oracle import dbg_oracle as orc

pytestmark = pytest.mark.gpu

SCALARS = ("n_nodes", "n_edges", "sum_edge_counts", "max_edge_count", "max_out_weight")


def pack(reads):
    blob = "".join(reads).encode("latin-1")
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return np.frombuffer(blob, dtype=np.uint8), off


def build(reads, k, g=None, **opts):
    g = g or _dbg.Graph()
    for name, v in opts.items():
        g.set_option(name, v)
    g.set_reads(*pack(reads))
    g.build(k)
    return g


_ORACLE = {}


def oracle(tag, reads, k):
    """(vertices, edges, edge_count_table) of the oracle, computed once per tag and left alone"""
    if tag not in _ORACLE:
        V, E = orc.graph_from_reads(list(reads), k)
        _ORACLE[tag] = (V, E, orc.edge_count_table(E))
    return _ORACLE[tag]


def rule(tag, reads, k, B):
    V, E, ect = oracle(tag, reads, k)
    return prod.count_spectrum((V, E), ect, B)


def assert_same(got, want, what=""):
    for n in SCALARS:
        assert got[n] == want[n], f"{what}: {n}: {got[n]} != {want[n]}"
    assert got["n_bins"] == want["n_bins"]
    for n in ("edge_hist", "node_hist", "D"):
        assert np.array_equal(got[n], want[n]), f"{what}: {n}"
    assert int(got["edge_hist"][0]) == 0


def random_dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def dna_reads(seed=5, n=3000):
    import synth
    return synth.reads_list(seed, 20000, n, 100, 0.01)


# ---- the reference's vectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_case_names())
def test_golden_case(name):
    case = load_golden(name)
    reads, k = case_reads(case), case["inputs"]["k"]
    g = build(reads, k)
    for B in (64, 4):
        assert_same(g.count_spectrum(B), rule(name, reads, k, B), f"{name} B={B}")
    s = case["summary"]
    sp = g.count_spectrum(64, hists=False)
    assert "edge_hist" not in sp and (sp["n_nodes"], sp["n_edges"], sp["sum_edge_counts"]) == (
        s["n_vertices"], s["n_edge_names"], s["sum_edge_counts"])
    g.close()


@pytest.mark.parametrize("family", ["fuzz_small", "fuzz_peptide", "fuzz_wide", "fuzz_peptide_wide"])
def test_every_fourth_case_of_a_fuzz_family(family):
    """ACGT sub-alphabets, peptides (dense [n][32]), two-word k and reference-keyed generic graphs, all on one handle."""
    with open(os.path.join(GOLDEN, family + ".json")) as fh:
        cases = json.load(fh)[::4]
    g = _dbg.Graph()
    degrees = set()
    for i, case in enumerate(cases):
        reads, k = case["inputs"]["reads"], case["inputs"]["k"]
        build(reads, k, g)
        for B in (64, 4):
            want = rule(f"{family}{i}", reads, k, B)
            assert_same(g.count_spectrum(B), want, f"{family} {i} B={B}")
        degrees |= set(np.nonzero(want["D"])[0].tolist())
        assert want["n_edges"] == len(case["result"]["edge_count_table"])  # the reference's own table
    assert len(cases) >= 30 and len(degrees) >= 2
    g.close()


# ---- sizes and shapes at which the kernel takes another path ----------------------------------------------------------------
def test_counts_beyond_16_bits():
    reads = ["A" * 70000]
    g = build(reads, 5)
    for B in (1 << 17, 256):
        sp = g.count_spectrum(B)
        assert_same(sp, rule("a70000", reads, 5, B), f"B={B}")
        assert sp["max_edge_count"] == 70000 - 5 > 65535 and sp["n_edges"] == 1
        assert int(sp["edge_hist"][min(69995, B - 1)]) == 1 and int(sp["edge_hist"].sum()) == 1
    g.close()


def test_clamp_border():
    reads = dna_reads(7, 600)
    g = build(reads, 9)
    m = g.count_spectrum(2, hists=False)["max_edge_count"]
    assert m == max(oracle("clamp", reads, 9)[2].values()) and m > 3
    for B in (m + 2, m + 1, m):   # the maximum below the clamp bin, exactly in it (B - 1), and one above it (B)
        sp = g.count_spectrum(B)
        assert_same(sp, rule("clamp", reads, 9, B), f"B={B}")
        assert sp["max_edge_count"] == m
    g.close()


def test_one_hot_bin():
    """Every edge has count 3 000.  Bins 2 999 and 3 000 lie above the LDS range (_dbg.SP_LDS_BINS), so the first three runs
    send every edge to one global bin, as an exact bin, as the clamp bin B - 1 and one above it; the node bins and the degrees
    are one hot LDS bin each.  At B = 64 and B = 2 the one hot edge bin is the clamp bin in LDS."""
    assert _dbg.SP_LDS_BINS <= 2999
    rng = np.random.default_rng(11)
    reads = [random_dna(rng, 200)] * 3000
    g = build(reads, 31)
    for B in (4096, 3001, 3000):
        sp = g.count_spectrum(B)
        assert_same(sp, rule("hot", reads, 31, B), f"B={B}")
        assert sp["max_edge_count"] == 3000 and int(sp["edge_hist"][min(3000, B - 1)]) == sp["n_edges"] == 200 - 31
    for B in (64, 2):                  # ... and here the one hot bin is the clamp bin in LDS
        assert_same(g.count_spectrum(B), rule("hot", reads, 31, B), f"B={B}")
    g.close()


@pytest.mark.parametrize("k", [6, 9])
def test_rows_across_every_tile_border_all_degrees(k):
    rng = np.random.default_rng(12)
    reads = [random_dna(rng, 300000), random_dna(rng, 300000)]
    want = rule(f"tile{k}", reads, k, 256)
    if k == 6:
        assert want["n_nodes"] == 4096 and int(want["D"][4]) == 4096
    else:
        assert want["n_nodes"] > 2.3e5 and all(int(want["D"][d]) > 0 for d in range(1, 5))
    for variant in (0, 1, 2, 3):       # the ways of relieving the hot bins give the same bins
        g = build(reads, k, spectrum_variant=variant)
        assert_same(g.count_spectrum(256), want, f"k={k} variant={variant}")
        assert_same(g.count_spectrum(3), rule(f"tile{k}", reads, k, 3), f"k={k} variant={variant} B=3")
        g.close()


def peptide_reads():
    rng = np.random.default_rng(9)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    protein = rng.choice(aa, size=300)
    out = []
    for _ in range(2000):
        s0 = int(rng.integers(0, 300 - 40))
        r = protein[s0:s0 + 40].copy()
        m = rng.random(40) < 0.03
        r[m] = rng.choice(aa, size=int(m.sum()))
        out.append(r.tobytes().decode())
    return out


@pytest.mark.parametrize("k", [2, 12])
def test_wide_rows(k):
    reads = peptide_reads()
    want = rule(f"pep{k}", reads, k, 64)
    assert any(int(want["D"][d]) > 0 for d in range(5, 33)), "the oracle must see a node with more than 4 successors"
    for variant in (0, 2, 3):
        g = build(reads, k, spectrum_variant=variant)
        assert g.sizes()["max_degree"] == 32
        assert_same(g.count_spectrum(64), want, f"peptides k={k}")
        assert_same(g.count_spectrum(2), rule(f"pep{k}", reads, k, 2), f"peptides k={k} B=2")
        g.close()


def test_no_nodes():
    for reads, k in ((["ACGT", "AC", ""], 4), ([], 3), (["ELVIS"], 5)):
        g = build(reads, k)
        sp = g.count_spectrum(16)
        assert all(sp[n] == 0 for n in SCALARS) and sp["pruned"] == 0 and sp["n_bins"] == 16
        assert not sp["edge_hist"].any() and not sp["node_hist"].any() and not sp["D"].any() and not sp["K"].any()
        g.close()


# ---- every kind of graph ------------------------------------------------------------------------------------------------------
def test_dense_sources_equal_the_default_engine():
    reads = dna_reads()
    for k, opts in ((21, {"engine": 1}), (40, {"wide_engine": 0})):
        a, b = build(reads, k), build(reads, k, **opts)
        for B in (64, 4):
            want = a.count_spectrum(B)
            assert_same(b.count_spectrum(B), want, f"k={k} {opts}")
            assert_same(want, rule(f"dna{k}", reads, k, B), f"k={k} default engine")
        assert b.count_spectrum(64)["sum_edge_counts"] == b.sizes()["n_edge_instances"] == 3000 * (100 - k)
        a.close(), b.close()


def walked(reads, k):
    g = build(reads, k)
    g.refine_edge_order(), g.prune(2), g.remove_tips(), g.mark_pull_reads(), g.walk(False)
    assert g.sizes()["contigs_materialised"] == 1
    return g


@pytest.mark.parametrize("k", [21, 40])
def test_graph_built_from_a_walk(k):
    src = walked(dna_reads(), k)
    off, chars, _, _, _ = src.export_contigs()
    text = chars.tobytes().decode()
    contigs = [text[int(off[i]):int(off[i + 1])] for i in range(off.size - 1)]
    g = _dbg.Graph()
    g.build_from_walk(src, k + 1, np.arange(len(contigs), dtype=np.uint64), b"", np.zeros(1, dtype=np.uint64))
    plain = build(contigs, k + 1)
    for B in (64, 4):
        want = plain.count_spectrum(B)
        assert want["n_nodes"] > 0
        assert_same(g.count_spectrum(B), want, f"from walk k={k}")
    for h in (g, plain, src):
        h.close()


@pytest.mark.parametrize("k", [21, 40])
def test_imported_graph(k):
    import multi_gpu
    from test_multi_gpu import rank_reads

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        rows = rank_reads(2, rank, 3000, 100)
        g.set_reads(rows.reshape(-1), np.arange(0, rows.size + 1, 100, dtype=np.uint64))
        multi_gpu.sharded_build(g, k, dist)
        merged = multi_gpu.gather_graph(g, k, dist, dst=0)
        dist.barrier()
        return g, merged

    res = inproc_dist.run_ranks(2, one)
    merged = res[0][1]
    rows = np.concatenate([rank_reads(2, r, 3000, 100) for r in range(2)])
    plain = build([row.tobytes().decode() for row in rows], k)
    for B in (64, 4):
        assert_same(merged.count_spectrum(B), plain.count_spectrum(B), f"imported k={k}")
    merged.close(), plain.close()
    for g, _ in res:
        g.close()


@pytest.mark.parametrize("tag", ["dna", "tiny"])
def test_graphs_in_parts(tag):
    reads = dna_reads() if tag == "dna" else dna_reads(13, 6)
    single = build(reads, 21)
    for passes in (4, 64):
        g = _dbg.Graph()
        g.set_reads(*pack(reads))
        g.build_multipass(21, passes)
        assert g.part_count() == passes
        for B in (64, 4):
            want = single.count_spectrum(B)
            whole = g.count_spectrum(B)
            assert_same(whole, want, f"{passes} passes")
            parts = [g.count_spectrum(B, part=p) for p in range(passes)]
            for n in ("edge_hist", "node_hist", "D"):
                assert np.array_equal(sum(p[n] for p in parts), want[n])
            for n in ("n_nodes", "n_edges", "sum_edge_counts"):
                assert sum(p[n] for p in parts) == want[n]
            for n in ("max_edge_count", "max_out_weight"):
                assert max(p[n] for p in parts) == want[n]
            assert [p["n_nodes"] for p in parts] == [g.part_sizes(p)["n_nodes"] for p in range(passes)]
        if passes == 64 and tag == "tiny":
            assert any(g.part_sizes(p)["n_nodes"] == 0 for p in range(passes)), "six reads leave some of 64 parts empty"
        g.close()
    single.close()


@pytest.mark.parametrize("k", [21, 40])
def test_eight_ranks(k):
    import multi_gpu
    from test_multi_gpu import rank_reads

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        rows = rank_reads(8, rank, 4000, 100)
        g.set_reads(rows.reshape(-1), np.arange(0, rows.size + 1, 100, dtype=np.uint64))
        multi_gpu.sharded_build(g, k, dist)
        sp = [multi_gpu.count_spectrum(g, dist, B) for B in (64, 4)]
        mine = g.count_spectrum(64)
        g.close()
        return sp, mine

    res = inproc_dist.run_ranks(8, one)
    rows = np.concatenate([rank_reads(8, r, 4000, 100) for r in range(8)])
    plain = build([row.tobytes().decode() for row in rows], k)
    for i, B in enumerate((64, 4)):
        want = plain.count_spectrum(B)
        for sp, _ in res:                       # every rank holds the whole graph's numbers
            assert_same(sp[i], want, f"8 ranks k={k} B={B}")
    assert sum(mine["n_nodes"] for _, mine in res) == plain.sizes()["n_nodes"]
    assert sum(1 for _, mine in res if mine["n_nodes"]) > 1
    plain.close()


def test_ranks_times_passes_through_the_traversal():
    import multi_gpu
    import part_traversal
    from test_multi_gpu import rank_reads
    k, ranks, passes = 21, 2, 2

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        rows = rank_reads(ranks, rank, 3000, 100)
        g.set_reads(rows.reshape(-1), np.arange(0, rows.size + 1, 100, dtype=np.uint64))
        multi_gpu.sharded_build_multipass(g, k, dist, passes)
        t = part_traversal.PartTraversal(g, k, dist)
        before = t.count_spectrum(64)
        t.prune(2)
        after = t.count_spectrum(64)
        g.close()
        return before, after

    res = inproc_dist.run_ranks(ranks, one)
    rows = np.concatenate([rank_reads(ranks, r, 3000, 100) for r in range(ranks)])
    plain = build([row.tobytes().decode() for row in rows], k)
    want = plain.count_spectrum(64)
    plain.refine_edge_order(), plain.prune(2)
    pruned = plain.count_spectrum(64)
    for before, after in res:
        assert_same(before, want, "ranks x passes")
        assert before["pruned"] == 0 and not before["K"].any()
        assert_same(after, want, "ranks x passes, pruned")
        assert after["pruned"] == 1 and np.array_equal(after["K"], pruned["K"]) and int(after["K"].sum()) == want["n_nodes"]
    plain.close()


# ---- the call changes nothing ---------------------------------------------------------------------------------------------------
def everything(g):
    """every export, with the nodes in dict order (ascending stamp): the table order of two builds may differ"""
    keys, stamps, counts, flags = g.export_nodes()
    o = np.argsort(stamps, kind="stable")
    succ = g.export_succ()
    succ_stamp = np.where(succ == _dbg.NO_NODE, np.uint64(0xFFFFFFFFFFFFFFFF), stamps[np.minimum(succ, max(stamps.size - 1, 0))])
    rp, col, cnt = g.export_csr()
    rows = [(stamps[col[int(rp[i]):int(rp[i + 1])]].tolist(), cnt[int(rp[i]):int(rp[i + 1])].tolist()) for i in o]
    off, chars, score, stamp, seq = g.export_contigs()
    text = chars.tobytes()
    contigs = sorted((int(stamp[i]), int(seq[i]), int(score[i]), text[int(off[i]):int(off[i + 1])]) for i in range(stamp.size))
    out = {"nodes": (keys[o], stamps[o], counts[o], flags[o]), "succ": succ_stamp[o], "keep": g.export_keepmask()[o],
           "pull_reads": g.export_pull_reads(), "pull_ranks": g.export_pull_ranks()[o]}
    return out, (g.sizes(), rows, contigs)


@pytest.mark.parametrize("k,reads_tag", [(21, "dna"), (40, "dna"), (3, "pep")])
def test_read_only(k, reads_tag):
    reads = dna_reads() if reads_tag == "dna" else peptide_reads()[:300]
    tag = f"{reads_tag}{k}" if reads_tag == "dna" else f"pep300_{k}"
    V, E, ect = oracle(tag, reads, k)
    want = prod.count_spectrum((V, E), ect, 64)
    a, b = build(reads, k), build(reads, k)
    first = a.count_spectrum(64)
    assert_same(first, want, "before the prune")
    assert first["pruned"] == 0 and not first["K"].any()
    a.refine_edge_order(), b.refine_edge_order()
    assert_same(a.count_spectrum(64), want, "after refine")
    a.prune(2), b.prune(2)
    kept = np.bincount([len(s) for s in orc.prune_edges(copy.deepcopy(E), 2).values()], minlength=33).astype(np.uint64)
    mid = a.count_spectrum(64)
    assert mid["pruned"] == 1 and np.array_equal(mid["K"], kept)
    a.remove_tips(), b.remove_tips()
    a.count_spectrum(4)
    a.mark_pull_reads(), b.mark_pull_reads()
    a.count_spectrum(64)
    a.walk(False), b.walk(False)
    last = a.count_spectrum(64)
    assert_same(last, want, "after the walk")
    assert last["pruned"] == 1 and np.array_equal(last["K"], kept) and int(kept.sum()) == want["n_nodes"]
    ea, sa = everything(a)
    eb, sb = everything(b)
    assert sa == sb
    for name in ea:
        xa, xb = ea[name], eb[name]
        for u, v in zip(xa if isinstance(xa, tuple) else (xa,), xb if isinstance(xb, tuple) else (xb,)):
            assert np.array_equal(u, v), name
    a.close(), b.close()


def test_reuse_of_one_handle():
    big, small = dna_reads(), ["ACGTACGTTGCA", "CGTACGTTGCAT", "TTTTTTTTTTTT", "ACGTACGTTGAA"]
    g = build(big, 21)
    assert g.count_spectrum(64)["n_nodes"] > 10000
    build(small, 5, g)
    for B in (64, 1 << 12):
        assert_same(g.count_spectrum(B), rule("small4", small, 5, B), "the small graph alone")
    g.close()


def test_device_memory():
    reads = dna_reads()
    g = build(reads, 21)
    for B in (2, 256, 1 << 20):
        sp = g.count_spectrum(B, hists=False)
        assert 0 < sp["peak_extra_device_bytes"] <= 16 * B + (64 << 10)
        assert sp["ms_kernel"] > 0
    g.set_reads(*pack(reads))
    g.build_multipass(21, 4)
    for B in (2, 1 << 20):
        assert 0 < g.count_spectrum(B, hists=False)["peak_extra_device_bytes"] <= 16 * B + (64 << 10)
    g.close()


def test_refusals_leave_the_handle_usable():
    import torch
    reads = dna_reads()
    g = _dbg.Graph()
    g.set_reads(*pack(reads))

    def refused(match, *a, **kw):
        with pytest.raises(_dbg.DbgError, match=match) as e:
            g.count_spectrum(*a, **kw)
        assert e.value.code == _dbg.DBG_E_ARG

    refused("no graph", 64)
    g.build(21)
    want = g.count_spectrum(64)
    for bad in (0, 1, (1 << 20) + 1):
        refused("n_bins", bad)
    refused("part", 64, part=0)
    assert_same(g.count_spectrum(64), want, "after the refusals")
    g.build_multipass(21, 4)
    refused("no such part", 64, part=4)
    refused("n_bins", 1, part=2)
    assert_same(g.count_spectrum(64), want, "in parts, after the refusals")
    # a shard between dbg_shard_build and dbg_shard_apply
    counts, (w0, w1, st) = g.shard_extract(21, 1)
    buckets = g.shard_bucket_counts()
    g.shard_build(21, 1, 0, w0.clone(), w1.clone(), st.clone(), [sum(counts)], [0], [buckets])
    refused("dbg_shard_apply", 64)
    g.shard_apply(torch.empty(0, dtype=torch.int32, device=w0.device))
    assert_same(g.count_spectrum(64), want, "the shard, applied")
    g.build(21)
    assert_same(g.count_spectrum(64), want, "a build after all of it")
    g.close()


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def test_driver_writes_a_spectrum_per_k(tmp_path):
    import synth
    case = load_golden("driver_dna_k5_8")
    inp = case["inputs"]
    reads, kl, ku, thr = list(inp["reads"]), inp["k_lowerlimit"], inp["k_upperlimit"], inp["threshold"]
    env = dict(os.environ, PYTHONPATH=PKG)

    def run(froot, extra):
        setting = synth.write_froot(str(tmp_path / froot), reads, kl, ku, threshold=thr)
        setting.update(extra)
        with open(tmp_path / froot / "setting.json", "w") as fh:
            json.dump(setting, fh)
        return subprocess.run([sys.executable, os.path.join(PKG, "II_assembleFromReads.py"), "-froot", froot], cwd=str(tmp_path),
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    plain, spec = run("plain", {}), run("spec", {"spectrum_bins": 32})
    assert plain.returncode == 0 and spec.returncode == 0, spec.stderr
    assert plain.stdout == spec.stdout
    assert (tmp_path / "plain" / "plain.fasta").read_bytes() == (tmp_path / "spec" / "spec.fasta").read_bytes()
    assert not [p for p in os.listdir(tmp_path / "plain") if p.endswith(".hist")]
    with contextlib.redirect_stdout(io.StringIO()):
        _, trace = orc.assemble(reads, kl, ku, thr)
    seqs = list(reads)
    for k in range(kl, ku + 1):
        V, E = orc.graph_from_reads(seqs, k)
        want = prod.count_spectrum((V, E), orc.edge_count_table(E), 32)["edge_hist"]
        text = (tmp_path / "spec" / f"spec_k{k}.hist").read_text()
        assert text == "".join(f"{c}\t{int(want[c])}\n" for c in range(1, 32)), k
        if k < ku:
            seqs = trace[k]["contigs"] + trace[k]["pull_out_read"]
    bad = run("bad", {"spectrum_bins": "many"})
    assert bad.returncode != 0 and "spectrum_bins" in bad.stderr
    assert not os.path.exists(tmp_path / "bad" / "bad.fasta")
