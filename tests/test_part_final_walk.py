"""The final-mode contig walk over a graph in PARTS (dbg_part_final_walk, part_traversal.walk_final, construct_graph /
output_contigs with final=True): against the vectors the REFERENCE produced with final = True (every DNA case at
threshold >= 1, built in 1 and in 4 parts), against the single-graph final walk on 3 k reads over 30 kbp (index, every text,
the FASTA file byte for byte; 4 parts, two-word keys, 2 ranks x 2 passes), and the library's refusals."""
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


def single(k, err, tmp):
    """dbg_walk(final) on the resident graph, once per (k, err): index in dict order, texts, the FASTA file's bytes."""
    if (k, err) not in _single:
        reads = _reads(err)
        assert np.array_equal(np.concatenate([_reads(err, r, 2) for r in range(2)]), reads)   # the ranks' reads are the one read set, cut
        g = _dbg.Graph()
        try:
            g.set_reads(reads.reshape(-1), np.arange(0, reads.size + 1, L, dtype=np.uint64))
            g.build(k)
            g.refine_edge_order()
            g.prune(THR)
            g.remove_tips()
            n_branch = g.sizes()["n_branch"]
            g.walk(1, 1 << 30)
            off, score, stamp, seq = g.export_contig_index()
            order = np.lexsort((seq, stamp))     # starts in dict order, emission order within a start
            toff, chars = g.export_contig_texts(order)
            text = chars.tobytes()
            texts = [text[int(toff[i]):int(toff[i + 1])] for i in range(order.size)]
            path = os.path.join(tmp, f"single_{k}_{err}.fa")
            g.write_contigs_fasta(path, indices=order[np.argsort(-score[order].astype(np.int64), kind="stable")], append=False, k_label=k)
            with open(path, "rb") as fh:
                fasta = fh.read()
        finally:
            g.close()
        _single[(k, err)] = {"stamp": stamp[order], "seq": seq[order], "length": (off[1:] - off[:-1])[order].astype(np.int64),
                             "score": score[order].astype(np.int64), "texts": texts, "fasta": fasta, "n_branch": n_branch}
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
