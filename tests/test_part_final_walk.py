"""The final-mode contig walk over a graph in PARTS (dbg_part_final_walk, part_traversal.walk_final, construct_graph /
output_contigs with final=True): against the vectors the REFERENCE produced with final = True (every DNA case at
threshold >= 1, built in 1 and in 4 parts), against the single-graph final walk on 3 k reads over 30 kbp (index, every text,
the FASTA file byte for byte; 4 parts, two-word keys, 2 ranks x 2 passes), on a read set of bubbles with 87 branch nodes
(more than two words of the walker's bitmap) against both that walk and the oracle, and the library's refusals."""
import json
import os

import numpy as np
import pytest

import _dbg
import synth
from conftest import GOLDEN, case_reads, golden_case_names, load_golden
from oracle import dbg_oracle as orc

pytestmark = pytest.mark.gpu

DNA = set("ACGT")


def _set_reads(g, reads):
    blob = np.frombuffer("".join(reads).encode("latin-1"), dtype=np.uint8)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    g.set_reads(blob, offs)


# ---- B: the reference's vectors ---------------------------------------------------------------------------------------------
def run_in_parts(reads, k, threshold, n_passes):
    import part_traversal
    g = _dbg.Graph()
    try:
        _set_reads(g, reads)
        g.build_multipass(k, n_passes)
        t, flags, branch, pulled = part_traversal.construct_graph(g, k, threshold, final=True)
        ctg = part_traversal.output_contigs(t)
        return {"branch_kmer": branch, "already_pull_out": pulled, "pull_out_read": [r for r, f in zip(reads, flags) if f],
                "contigs": ctg.texts(range(len(ctg))), "scores": ctg.scores.tolist()}
    finally:
        g.close()


def check(reads, inp, ref, tag):
    """-> (ran, one start branched: two consecutive contigs share their first k characters)"""
    if not inp["final"] or not all(set(r) <= DNA for r in reads) or inp["threshold"] < 1:
        return False, False
    ect = dict(map(tuple, ref["edge_count_table"]))
    want_scores = [orc.get_score(ect, c, inp["k"]) for c in ref["contigs"]]
    assert ref["branch_kmer"] == [] and ref["pull_out_read"] == []   # what final = True means in the reference
    for n_passes in (1, 4):
        got = run_in_parts(list(reads), inp["k"], inp["threshold"], n_passes)
        for key in ("contigs", "already_pull_out", "branch_kmer", "pull_out_read"):
            assert got[key] == ref[key], f"{tag} P={n_passes}: {key}"
        assert got["scores"] == want_scores, f"{tag} P={n_passes}: getScore"
    k, ct = inp["k"], ref["contigs"]
    return True, any(a[:k] == b[:k] for a, b in zip(ct, ct[1:]))


def test_golden_final_cases_in_parts():
    n = 0
    for name in golden_case_names():
        case = load_golden(name)
        if "result" not in case:
            continue
        n += check(case_reads(case), case["inputs"], case["result"], name)[0]
    assert n >= 26


_branched = {}


@pytest.mark.parametrize("family,n_min", [("fuzz_small", 160), ("fuzz_wide", 60)])
def test_fuzz_families_final_in_parts(family, n_min):
    with open(os.path.join(GOLDEN, family + ".json")) as fh:
        cases = json.load(fh)
    n = shared = 0
    for i, case in enumerate(cases):
        ran, branched = check(case["inputs"]["reads"], case["inputs"], case["result"], f"{family} {i} {case['inputs']['k']}")
        n += ran
        shared += branched
    assert n >= n_min
    _branched[family] = shared
    if len(_branched) == 2:   # over both families: the cases in which one start branches
        assert sum(_branched.values()) >= 40, _branched


# ---- C: against the single-graph final walk ---------------------------------------------------------------------------------
N_READS, L, GENOME, THR = 3000, 100, 30_000, 2
# (k, error rate, ranks, passes).  Error rate 0 is the input of the final case of test_hip_scale.py: it has no branch node at
# these k, so the final walk must be the non-final index.  With errors the same reads branch: 7 branch nodes, 1980 contigs
# and 20 MB of text at k = 31 / 0.001; 30 branch nodes, 8 pulled nodes, 5893 contigs and 30 MB at k = 40 / 0.002 (counted
# with the C oracle; a higher rate makes the enumeration explode -- at 0.01 and k = 31 it passes 6.5e7 DFS steps).
SCALE_CASES = [(31, 0.0, 1, 4), (40, 0.0, 1, 4), (31, 0.001, 1, 4), (40, 0.002, 1, 4), (40, 0.002, 2, 2), (31, 0.0, 2, 2)]


def _reads(err, rank=0, ranks=1):
    per = N_READS // ranks
    return synth.reads_ascii(1, GENOME, per, L, err, first_read=rank * per)


_single = {}


def walk_resident(set_reads, k, threshold, path):
    """dbg_walk(final) on the resident graph: index in dict order, texts, the FASTA file's bytes (written to ``path``)."""
    g = _dbg.Graph()
    try:
        set_reads(g)
        g.build(k)
        g.refine_edge_order()
        g.prune(threshold)
        g.remove_tips()
        sizes = g.sizes()
        g.walk(1, 1 << 30)
        off, score, stamp, seq = g.export_contig_index()
        order = np.lexsort((seq, stamp))     # starts in dict order, emission order within a start
        toff, chars = g.export_contig_texts(order)
        text = chars.tobytes()
        texts = [text[int(toff[i]):int(toff[i + 1])] for i in range(order.size)]
        g.write_contigs_fasta(path, indices=order[np.argsort(-score[order].astype(np.int64), kind="stable")], append=False, k_label=k)
        with open(path, "rb") as fh:
            fasta = fh.read()
    finally:
        g.close()
    return {"stamp": stamp[order], "seq": seq[order], "length": (off[1:] - off[:-1])[order].astype(np.int64),
            "score": score[order].astype(np.int64), "texts": texts, "fasta": fasta, "n_branch": sizes["n_branch"],
            "n_pulled": sizes["n_pulled"]}


def single(k, err, tmp):
    """walk_resident, once per (k, err)"""
    if (k, err) not in _single:
        reads = _reads(err)
        assert np.array_equal(np.concatenate([_reads(err, r, 2) for r in range(2)]), reads)   # the ranks' reads are the one read set, cut
        _single[(k, err)] = walk_resident(lambda g: g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, L, dtype=np.uint64)),
                                          k, THR, os.path.join(tmp, f"single_{k}_{err}.fa"))
    return _single[(k, err)]


def in_parts(k, err, ranks, passes, tmp):
    import inproc_dist
    import multi_gpu
    import part_traversal

    def one(dist, rank):
        reads = _reads(err, rank, ranks)
        g = _dbg.Graph(device=0)
        try:
            g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, L, dtype=np.uint64))
            if dist is None:
                g.build_multipass(k, passes)
            else:
                multi_gpu.sharded_build_multipass(g, k, dist, passes)
            t, flags, branch, pulled = part_traversal.construct_graph(g, k, THR, dist, final=True)
            assert branch == [] and not flags.any()
            ctg = part_traversal.output_contigs(t)
            index = {"stamp": ctg.start_stamps, "length": ctg.lengths, "score": ctg.scores}
            chars, off = ctg.packed()
            text = chars.tobytes()
            texts = [text[int(off[i]):int(off[i + 1])] for i in range(len(ctg))]
            path = os.path.join(tmp, f"parts_{k}_{err}_{ranks}x{passes}.fa")
            written = ctg.write_fasta(path, k, append=False)
            some = ctg[len(ctg) // 2:len(ctg) // 2 + 3] + [ctg[-1]]
            nonfinal = t.walk_index() if err == 0.0 else None
            return index, texts, path, written, some, nonfinal, t.final is not None
        finally:
            g.close()

    return [one(None, 0)] if ranks == 1 else inproc_dist.run_ranks(ranks, one)


@pytest.mark.parametrize("k,err,ranks,passes", SCALE_CASES)
def test_final_walk_in_parts_equals_the_single_graph(k, err, ranks, passes, tmp_path_factory):
    tmp = str(tmp_path_factory.getbasetemp())
    want = single(k, err, tmp)
    assert (want["n_branch"] > 0) == (err > 0) and len(want["texts"]) > 300
    if err > 0:
        assert int((want["seq"] > 0).sum()) > 300   # starts that branch
    got = in_parts(k, err, ranks, passes, tmp)
    for rank, (index, texts, path, written, some, nonfinal, stitched) in enumerate(got):
        tag = f"rank {rank}"
        assert stitched == (err > 0), tag          # without a branch node the final walk is the non-final index
        for col in ("stamp", "length", "score"):
            assert np.array_equal(index[col], want[col]), f"{tag}: {col}"
        assert texts == want["texts"], tag
        assert [s.encode("ascii") for s in some] == want["texts"][len(texts) // 2:len(texts) // 2 + 3] + [want["texts"][-1]], tag
        assert written == len(want["fasta"]), tag
        if nonfinal is not None:
            for col in ("stamp", "length", "score"):
                assert np.array_equal(nonfinal[col], want[col]), f"{tag}: walk_index {col}"
    with open(got[0][2], "rb") as fh:
        assert fh.read() == want["fasta"]   # several ranks name the same path: rank 0 alone wrote it


def test_walk_final_returns_seq_within_the_start():
    import part_traversal
    k, err = 40, 0.002
    reads = _reads(err)
    g = _dbg.Graph()
    try:
        g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, L, dtype=np.uint64))
        g.build_multipass(k, 4)
        res = part_traversal.traverse(g, k, THR, final=True)
    finally:
        g.close()
    want = _single.get((k, err))
    if want is None:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            want = single(k, err, tmp)
    for col in ("stamp", "seq", "length", "score"):
        assert np.array_equal(res["contigs"][col], want[col]), col


def test_stitch_in_small_blocks(monkeypatch):
    """BATCH_CHARS bounds the stitch: with a tiny bound every block holds a few contigs and the texts stay the same."""
    import part_traversal
    case = load_golden("dna_small_k40_e1_t3_final")
    reads, inp, ref = case_reads(case), case["inputs"], case["result"]
    g = _dbg.Graph()
    try:
        _set_reads(g, reads)
        g.build_multipass(inp["k"], 2)
        t, _, _, _ = part_traversal.construct_graph(g, inp["k"], inp["threshold"], final=True)
        ctg = part_traversal.output_contigs(t)
        monkeypatch.setattr(part_traversal, "BATCH_CHARS", 300)
        assert len(list(t._final_blocks(np.arange(len(ctg))))) > 3 or int(ctg.lengths.sum()) < 1200
        assert list(ctg) == ref["contigs"]
        assert ctg[::-1] == ref["contigs"][::-1]
    finally:
        g.close()


# ---- C2: more than 64 branch nodes: a read set of bubbles ---------------------------------------------------------------------
# 40 random genomes of 200 bp, each as two haplotypes that differ at 2 SNPs 70 bp apart, and one of 600 bp with 7 SNPs 65 bp
# apart; every haplotype is one whole read, given three times, and there is no error model.  Every SNP is a bubble whose arms
# are k nodes long (longer than TIP_DEPTH, so no tip is pulled) and whose first node is a branch node: 40 * 2 + 7 = 87 of
# them, 40 * 4 + 2^7 = 288 contigs, up to 7 branch nodes on a path (counted with the oracle at k = 21 and 40).  The on-path
# bitmap of a walker has three words here; in every other case of this file it has one.
BUBBLE_THR, BUBBLE_BRANCH, BUBBLE_CONTIGS = 2, 87, 288


def bubble_reads():
    import random
    rng = random.Random(2024)
    reads = []

    def genome(n, snps):
        a = [rng.choice("ACGT") for _ in range(n)]
        b = list(a)
        for x in snps:
            b[x] = "ACGT"[("ACGT".index(a[x]) + 1 + rng.randrange(3)) % 4]
        for hap in (a, b):
            reads.extend(["".join(hap)] * 3)
    for _ in range(40):
        genome(200, (60, 130))
    genome(600, tuple(70 + 65 * i for i in range(7)))
    return reads


_bubble = {}


def bubble_want(k, tmp):
    """once per k: walk_resident and the oracle's graph and contigs"""
    if k not in _bubble:
        reads = bubble_reads()
        want = walk_resident(lambda g: _set_reads(g, reads), k, BUBBLE_THR, os.path.join(tmp, f"bubble_single_{k}.fa"))
        og, _, obranch, opulled, oect = orc.construct_graph(reads, k, threshold=BUBBLE_THR, final=True, verbose=False)
        want.update(oracle=orc.output_contigs(og, obranch, opulled, verbose=False), oracle_pulled=opulled, ect=oect,
                    oracle_branch=sum(len(s) > 1 for s in og[1].values()))
        _bubble[k] = want
    return _bubble[k]


@pytest.mark.parametrize("ranks,passes", [(1, 1), (1, 2), (1, 4), (2, 2)])
@pytest.mark.parametrize("k", [21, 40])
def test_bubbles_with_more_than_64_branch_nodes(k, ranks, passes, tmp_path_factory):
    import inproc_dist
    import multi_gpu
    import part_traversal
    tmp = str(tmp_path_factory.getbasetemp())
    want = bubble_want(k, tmp)
    assert want["oracle_branch"] == BUBBLE_BRANCH > 64 and want["oracle_pulled"] == [] and len(want["oracle"]) == BUBBLE_CONTIGS
    assert want["n_branch"] == BUBBLE_BRANCH and want["n_pulled"] == 0
    assert [t.decode("ascii") for t in want["texts"]] == want["oracle"]
    assert want["score"].tolist() == [orc.get_score(want["ect"], c, k) for c in want["oracle"]]
    assert int(want["seq"].max()) == 127                       # 2^7 paths from one start
    all_reads = bubble_reads()
    per = len(all_reads) // ranks
    assert per * ranks == len(all_reads)

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        try:
            _set_reads(g, all_reads[rank * per:(rank + 1) * per])
            if dist is None:
                g.build_multipass(k, passes)
            else:
                multi_gpu.sharded_build_multipass(g, k, dist, passes)
            t, flags, branch, pulled = part_traversal.construct_graph(g, k, BUBBLE_THR, dist, final=True)
            assert branch == [] and not flags.any()
            assert t.branch["gid"].size == BUBBLE_BRANCH and pulled == []     # nothing pulled: the bubbles are whole
            index = t.walk_final()                                             # what output_contigs wraps; it drops seq
            ctg = part_traversal.PartContigs(t, index)
            assert t.final_mode and t.final is not None
            chars, off = ctg.packed()
            text = chars.tobytes()
            path = os.path.join(tmp, f"bubble_parts_{k}_{ranks}x{passes}.fa")
            written = ctg.write_fasta(path, k, append=False)
            return index, [text[int(off[i]):int(off[i + 1])] for i in range(len(ctg))], list(ctg), path, written
        finally:
            g.close()

    for rank, (index, texts, strs, path, written) in enumerate([one(None, 0)] if ranks == 1 else inproc_dist.run_ranks(ranks, one)):
        tag = f"rank {rank}"
        for col in ("stamp", "seq", "length", "score"):
            assert np.array_equal(index[col], want[col]), f"{tag}: {col}"
        assert texts == want["texts"], tag
        assert strs == want["oracle"], tag
        assert written == len(want["fasta"]), tag
    with open(path, "rb") as fh:
        assert fh.read() == want["fasta"]


# ---- D: refusals ------------------------------------------------------------------------------------------------------------
def _branching_traversal(g):
    import part_traversal
    case = load_golden("dna_small_k40_e1_t3_final")
    _set_reads(g, case_reads(case))
    g.build_multipass(case["inputs"]["k"], 2)
    t, _, _, _ = part_traversal.construct_graph(g, case["inputs"]["k"], case["inputs"]["threshold"], final=True)
    assert t.branch["gid"].size > 0
    return t, case["result"]["contigs"]


def test_step_budget_refuses_and_the_handle_stays_usable():
    g = _dbg.Graph()
    try:
        t, want = _branching_traversal(g)
        g.set_option("part_final_walk_steps", 3)
        with pytest.raises(_dbg.DbgError) as e:
            t.walk_final()
        assert e.value.code == _dbg.DBG_E_CAPACITY and "part_final_walk_steps" in str(e.value)
        g.set_option("part_final_walk_steps", 1 << 24)   # the default
        index = t.walk_final()
        assert index["length"].tolist() == [len(c) for c in want]
        assert t.contig_texts(range(len(want))) == want
        with pytest.raises(_dbg.DbgError):
            g.set_option("part_final_walk_steps", 0)
    finally:
        g.close()


def test_max_chars_refuses_with_valid_sizes():
    g = _dbg.Graph()
    try:
        t, want = _branching_traversal(g)
        total = sum(len(c) for c in want)
        with pytest.raises(_dbg.DbgError) as e:
            t.walk_final(max_chars=total - 1)
        assert e.value.code == _dbg.DBG_E_CAPACITY and "max_chars" in str(e.value)
        assert e.value.sizes["n_contigs"] == len(want) and e.value.sizes["n_chars"] == total and e.value.sizes["n_pieces"] >= len(want)
        assert len(t.walk_final(max_chars=total)["length"]) == len(want)
    finally:
        g.close()


def test_an_out_of_range_successor_row_is_refused_before_any_walk(monkeypatch):
    g = _dbg.Graph()
    try:
        t, want = _branching_traversal(g)
        real = g.part_final_walk

        def broken(kind, append, score, branch, succ_row, succ_count, starts, max_chars=0):
            succ_row = succ_row.clone()
            succ_row[int((succ_row >= 0).nonzero()[0])] = kind.numel()     # one row past the entries
            return real(kind, append, score, branch, succ_row, succ_count, starts, max_chars=max_chars)
        g.part_final_walk = broken
        with pytest.raises(_dbg.DbgError) as e:
            t.walk_final()
        assert e.value.code == _dbg.DBG_E_ARG and "successor row" in str(e.value) and "no walk ran" in str(e.value)
        assert e.value.sizes == {"n_contigs": 0, "n_pieces": 0, "n_chars": 0}
        del g.part_final_walk
        assert len(t.walk_final()["length"]) == len(want)
    finally:
        g.close()


def test_no_graph_in_parts_and_an_empty_contraction():
    import torch
    g = _dbg.Graph()
    try:
        dev = torch.device("cuda", g.sizes_device())
        z8, z64, z32 = (torch.empty(0, dtype=d, device=dev) for d in (torch.uint8, torch.int64, torch.int32))
        with pytest.raises(_dbg.DbgError) as e:
            g.part_final_walk(z8, z64, z64, z32, z32, z32, z32)
        assert e.value.code == _dbg.DBG_E_ARG
        _set_reads(g, ["ACGTTGCATG", "GTTGCATGCC"])
        g.build_multipass(5, 2)
        res = g.part_final_walk(z8, z64, z64, z32, z32, z32, z32)
        assert (res["n_contigs"], res["n_pieces"], res["n_chars"]) == (0, 0, 0) and res["piece_off"].tolist() == [0]
    finally:
        g.close()
