"""The C restatement (oracle/dbg_oracle.c) against the pinned Python oracle, CPU only."""
import numpy as np
import pytest

from conftest import case_reads, golden_case_names, load_golden
from oracle import dbg_oracle as orc
from oracle import orc_c

CODE_CHAR = "ACTG"


def decode(key, k, hi=0):
    v = (int(hi) << 64) | int(key)
    return "".join(CODE_CHAR[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def pack(reads):
    blob = "".join(reads).encode("ascii")
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(blob, dtype=np.uint8), off


@pytest.mark.parametrize("name", [n for n in golden_case_names() if not n.startswith("peptide")])
def test_c_oracle_matches_python_oracle(name):
    case = load_golden(name)
    reads = case_reads(case)
    k = case["inputs"]["k"]
    V, E = orc.graph_from_reads(reads, k)
    ect = orc.edge_count_table(E)
    b, off = pack(reads)
    res = orc_c.build(b, off, k)
    assert res["n_nodes"] == len(V) == case["summary"]["n_vertices"]
    labels = [decode(x, k, hi) for x, hi in zip(res["keys"], res["keys_hi"])]
    assert labels == list(V.keys())  # dict order
    assert [int(s) & 1 for s in res["stamps"]] == [V[v].indegree for v in V]
    got = {}
    for lab, c in zip(labels, res["counts"]):
        for code in range(4):
            if c[code]:
                got[lab + CODE_CHAR[code]] = int(c[code])
    assert got == dict(ect)
    assert res["n_edge_instances"] == sum(ect.values())


def test_multithreaded_build_equals_the_single_threaded_one():
    """bench.py's cpu_baseline (orc_build_mt_partitioned, and orc_build_mt beside it: hash slices over threads) must build the same graph as orc_build."""
    import numpy as np
    import synth
    reads = synth.reads_ascii(5, 30000, 6000, 100, 0.01)
    off = np.arange(0, reads.size + 1, 100, dtype=np.uint64)
    for k in (5, 21, 31):
        a = orc_c.build(reads.reshape(-1), off, k)
        for threads in (1, 3, 8):
            for once in (False, True):  # every thread scans everything / k-mers partitioned once (bench.py uses the latter)
                b = orc_c.build_mt(reads.reshape(-1), off, k, threads, partition_once=once)
                assert b["n_nodes"] == a["n_nodes"] and b["n_kmer_instances"] == a["n_kmer_instances"]
                assert b["n_edge_instances"] == a["n_edge_instances"] and b["n_edges"] == int((a["counts"] != 0).sum())
                assert b["digest"] == orc_c.digest(a["keys"], a["stamps"], a["counts"])


# ---- the traversal (orc_traverse) against the Python oracle -----------------------------------------------------------
def check_traversal(reads, k, threshold, final, max_paths=10**7):
    """orc_traverse on an orc_build of `reads` must give construct_graph + output_contigs of oracle/dbg_oracle.py field by
    field and order by order: kept successors in rank order, branch_kmer, already_pull_out, pull_out_read, the contigs
    (text and emission order) and their getScore."""
    import contextlib
    import io
    b, off = pack(reads)
    o = orc_c.Oracle(b, off, k)
    try:
        t = o.traverse(threshold, final=final, max_paths=max_paths)   # OverflowError before the Python oracle runs
        with contextlib.redirect_stdout(io.StringIO()):
            (V, E), pull, branch, pulled, ect = orc.construct_graph(list(reads), k, threshold=threshold, final=final)
            contigs = orc.output_contigs((V, E), branch, pulled)
        keys, hi, _, _ = o.nodes()
        lab = orc_c.labels(keys, hi, k)
        assert lab == list(V.keys())
        pulled_set = set(pulled)
        kept = {}
        for i, v in enumerate(lab):
            if v in pulled_set:
                continue
            codes = [(int(t["order"][i]) >> (2 * j)) & 3 for j in range(V[v].outdegree)]
            kept[v] = [v[1:] + CODE_CHAR[c] for c in codes if (int(t["keep"][i]) >> c) & 1]
        assert kept == {v: list(s) for v, s in E.items()} and list(kept) == list(E)
        assert [lab[i] for i in t["pulled"]] == list(pulled)
        assert [lab[i] for i in t["branch"]] == ([v for v in E if len(E[v]) > 1] if final else list(branch))
        assert all(((int(f) & 1) != 0) == (len(E.get(v, ())) > 1) for v, f in zip(lab, t["flags"]))
        if not final:
            assert [r for r, f in zip(reads, t["read_flags"]) if f] == list(pull)
        n = len(t["score"])
        buf, coff = o.spell(np.arange(n))
        text = buf.tobytes().decode("ascii")
        got = [text[coff[i]:coff[i + 1]] for i in range(n)]
        assert got == list(contigs)
        assert t["chars"].tolist() == [len(c) for c in contigs]
        assert t["score"].tolist() == [orc.get_score(ect, c, k) for c in contigs]
        starts = [v for v in V if V[v].indegree == 0]
        seq_ok = []
        for i in range(n):   # contigs grouped by start in dict order, numbered within their start
            seq_ok.append(0 if i == 0 or t["stamp"][i] != t["stamp"][i - 1] else seq_ok[-1] + 1)
        assert t["seq"].tolist() == seq_ok and np.all(np.diff(t["stamp"].astype(np.int64)) >= 0)
        assert all(c[:k] in starts for c in contigs)
        return t
    finally:
        o.close()


@pytest.mark.parametrize("name", [n for n in golden_case_names() if not n.startswith("peptide")])
def test_c_traversal_matches_python_oracle_on_golden_cases(name):
    case = load_golden(name)
    inp = case["inputs"]
    check_traversal(case_reads(case), inp["k"], inp["threshold"], inp["final"])


@pytest.mark.parametrize("family", ["fuzz_small", "fuzz_wide"])
def test_c_traversal_matches_python_oracle_on_fuzz_cases(family):
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, family + ".json")) as fh:
        cases = json.load(fh)
    n = 0
    for case in cases:
        inp = case["inputs"]
        if any(set(r) - set("ACGT") for r in inp["reads"]):
            continue
        check_traversal(inp["reads"], inp["k"], inp["threshold"], inp["final"])
        n += 1
    assert n >= 100


def random_reads(rng, k, n_reads, genome_len, err):
    """Reads of a random genome with substitutions, lengths mixed around k (k - 1, k, k + 1) and long."""
    genome = rng.choice(list("ACGT"), size=genome_len)
    reads = []
    for _ in range(n_reads):
        ln = int(rng.choice([k - 1, k, k + 1, k + 2, 2 * k, 3 * k + 7]))
        ln = max(1, min(ln, genome_len))
        p = int(rng.integers(0, genome_len - ln + 1))
        r = genome[p:p + ln].copy()
        flip = rng.random(ln) < err
        r[flip] = rng.choice(list("ACGT"), size=int(flip.sum()))
        reads.append("".join(r))
    return reads


@pytest.mark.parametrize("k", [3, 5, 9, 31, 32, 33, 63])
def test_c_traversal_matches_python_oracle_on_random_cases(k):
    rng = np.random.default_rng(1000 + k)
    seen = {"branch": 0, "pulled": 0, "pull": 0, "contigs": 0, "final": 0}
    for it in range(12):
        reads = random_reads(rng, k, int(rng.integers(40, 200)), int(rng.integers(k + 5, 4 * k + 60)), float(rng.choice([0.0, 0.02, 0.06])))
        for thr in (1, 1.5, 2, 2.5, 3):
            t = check_traversal(reads, k, thr, False)
            seen["branch"] += len(t["branch"]) > 0
            seen["pulled"] += len(t["pulled"]) > 0
            seen["pull"] += t["n_pull_reads"] > 0
            seen["contigs"] += len(t["score"]) > 0
        for thr in (1.5, 2):
            try:
                check_traversal(reads, k, thr, True, max_paths=300)
                seen["final"] += 1
            except OverflowError:   # exponentially many simple paths: not a case for the Python oracle
                pass
    assert min(seen.values()) > 0, seen
