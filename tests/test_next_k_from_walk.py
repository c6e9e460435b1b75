"""The driver's k -> k+1 step built from the walk's chains on the device (dbg_build_from_walk): no contig text leaves the
device, and the (k+1)-graph, its pull-out reads and its contigs equal the text path's."""
import contextlib
import io

import numpy as np
import pytest

import _dbg
import debruijn
import synth
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _jump_walks(monkeypatch):
    """Forced-lazy contigs need the list-ranking walk, which small graphs take only below this node count."""
    monkeypatch.setenv("DBG_WALK_JUMP_MIN", "1")


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _lazy_step(reads, k, thr):
    g, pull, branch, pulled, _ = _quiet(debruijn.construct_graph, reads, k, threshold=thr)
    lazy = _quiet(debruijn.output_contigs, g, branch, pulled)
    assert isinstance(lazy, debruijn.LazyContigs)
    return lazy, list(pull), g


def _graph_view(res):
    (V, E), pull, branch, pulled, ect = res
    return ([(v, n.indegree, n.outdegree) for v, n in V.items()], {v: list(s) for v, s in E.items()}, list(ect.items()),
            list(branch), list(pulled), list(pull))


def _contigs(res):
    (V, E), pull, branch, pulled, ect = res
    c = _quiet(debruijn.output_contigs, (V, E), branch, pulled)
    texts = [c[i] for i in range(len(c))]
    scores = list(c.scores)
    order = sorted(range(len(texts)), key=lambda i: scores[i], reverse=True)
    return texts, scores, [texts[i] for i in order]


def _check_step(monkeypatch, reads, k, thr, sort=True, tail=True, min_calls=1):
    """One forced-lazy step at k, then k+1 by both paths; returns the new path's result."""
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    lazy, pull, _ = _lazy_step(reads, k, thr)
    if sort:
        lazy.sort(reverse=True)
    texts = [lazy[i] for i in range(len(lazy))]
    extra = pull if tail else []
    lazy.extend(extra)
    want = _quiet(debruijn.construct_graph, texts + extra, k + 1, threshold=thr)
    calls = []
    real = _dbg.Graph.build_from_walk
    monkeypatch.setattr(_dbg.Graph, "build_from_walk", lambda *a: (calls.append(1), real(*a))[1])
    with monkeypatch.context() as m:
        m.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("contig text left the device")))
        got = _quiet(debruijn.construct_graph, lazy, k + 1, threshold=thr)
        assert len(calls) >= min_calls
        sz = got[0][0]._graph.sizes()
        assert sz["n_reads"] == len(texts) + len(extra)
        assert sz["n_bytes"] == sum(map(len, texts)) + sum(map(len, extra))
    assert _graph_view(got) == _graph_view(want)
    assert _contigs(got) == _contigs(want)
    return got


def test_no_text_leaves_the_device(monkeypatch):
    reads = synth.reads_list(5, 6000, 900, 100, 0.01)
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    lazy, pull, _ = _lazy_step(reads, 21, 2)
    monkeypatch.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("text fetched")))
    lazy.sort(reverse=True)
    lazy.extend(pull)
    res = _quiet(debruijn.construct_graph, lazy, 22, threshold=2)
    assert len(res[0][0]) > 0


@pytest.mark.parametrize("k", [9, 15, 21, 30, 31, 40, 62])
@pytest.mark.parametrize("err", [0.0, 0.01])
def test_exact_against_text_path_k(monkeypatch, k, err):
    reads = synth.reads_list(11 + k, 5000, 3000, 100, err)
    _check_step(monkeypatch, reads, k, 2)


@pytest.mark.parametrize("thr", [1, 2, 3])
def test_exact_thresholds(monkeypatch, thr):
    reads = synth.reads_list(21, 8000, 3000, 100, 0.01)
    _check_step(monkeypatch, reads, 15, thr)


def test_exact_200k_reads(monkeypatch):
    reads = synth.reads_list(31, 200000, 200000, 100, 0.01)
    _check_step(monkeypatch, reads, 31, 2)


def test_exact_cycles_and_short_contigs(monkeypatch):
    """A repeat-rich genome (chains that close on themselves emit nothing) plus reads of exactly k and k+1 characters."""
    rng = np.random.default_rng(7)
    unit = "".join(rng.choice(list("ACGT"), 37))
    genome = unit * 40 + "".join(rng.choice(list("ACGT"), 400)) + unit * 10
    reads = [genome[i:i + 90] for i in range(0, len(genome) - 90, 7)]
    reads += [genome[i:i + 13] for i in range(5, 400, 41)] + [genome[i:i + 14] for i in range(9, 400, 53)]
    reads += ["ACGTACGTACGTA", "ACGTACGTACGTAC", "TTTTTTTTTTTTTTTT"]
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))
    x, y = rnd(13), rnd(13)
    reads += [x + "A" + rnd(40), x + "C" + rnd(40)]  # a start that is a branch node: a contig of k characters
    reads += ["G" + y + "A" + rnd(40), y + "C" + rnd(40)]  # a start whose successor branches: k + 1 characters
    for thr in (1, 2):
        monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
        lazy, _, _ = _lazy_step(reads, 13, thr)
        sz = lazy._graph.sizes()
        assert 13 in lazy.lengths and 14 in lazy.lengths  # contigs of exactly k and k+1 characters
        assert sz["n_starts"] > sz["n_contigs"] + sz["n_pulled"]  # a start that is not pulled emits nothing: its chain cycles
        _check_step(monkeypatch, reads, 13, thr)


def test_exact_empty_tail(monkeypatch):
    reads = synth.reads_list(41, 5000, 2000, 100, 0.01)
    _check_step(monkeypatch, reads, 21, 2, tail=False)


def test_exact_order_not_default(monkeypatch):
    """Many equal scores: the stable sort keeps a non-trivial order, and an unsorted index works as well."""
    reads = synth.reads_list(43, 3000, 2500, 60, 0.02)
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    lazy, _, _ = _lazy_step(reads, 11, 1)
    assert len(set(lazy.scores)) < len(lazy.scores)  # equal scores: their order is the stable sort's
    _check_step(monkeypatch, reads, 11, 1)
    _check_step(monkeypatch, reads, 11, 1, sort=False)


@pytest.mark.parametrize("name", ["driver_dna_k5_8", "driver_dna_k12_15", "driver_dna_k30_34",
                                  "driver_peptide_k3_5", "driver_peptide_k10_14"])
def test_driver_traces_forced_lazy(monkeypatch, name):
    import II_assembleFromReads as drv
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 0)
    real_oc = debruijn.output_contigs

    lazy_steps = []

    def forced_lazy(g, branch, pulled):  # non-final walks keep the index only; the final walk spells its contigs
        debruijn.MAX_CONTIG_CHARS = 1 if len(branch) else 0
        out = real_oc(g, branch, pulled)
        lazy_steps.append(isinstance(out, debruijn.LazyContigs))
        return out

    monkeypatch.setattr(debruijn, "output_contigs", forced_lazy)
    calls = []
    real = _dbg.Graph.build_from_walk
    monkeypatch.setattr(_dbg.Graph, "build_from_walk", lambda *a: (calls.append(1), real(*a))[1])
    case = load_golden(name)
    inp = case["inputs"]
    final = _quiet(drv.assemble, list(inp["reads"]), inp["k_lowerlimit"], inp["k_upperlimit"], inp["threshold"])
    assert [final[i] for i in range(len(final))] == case["result"]["final_contigs"]
    if "dna" in name:  # every k after the first is built from the walk, the later ones with pulled contigs in the tail
        assert lazy_steps[:-1] == [True] * (inp["k_upperlimit"] - inp["k_lowerlimit"])
        assert len(calls) == inp["k_upperlimit"] - inp["k_lowerlimit"]
    else:
        assert not calls


def test_refusals_leave_src_usable(monkeypatch):
    reads = synth.reads_list(51, 5000, 1500, 100, 0.01)
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    lazy, pull, g = _lazy_step(reads, 21, 2)
    src = lazy._graph
    n = len(lazy._order)
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))

    def refused(k1, order, match):
        dst = _dbg.Graph()
        with pytest.raises(_dbg.DbgError, match=match):
            dst.build_from_walk(src, k1, order, *empty)

    refused(22, np.arange(n - 1), "permutation")
    refused(22, np.zeros(n), "permutation")
    refused(23, np.arange(n), "k1")
    assert lazy[0]  # src still answers
    sz = src.sizes()
    # k1 > 63 and a final-mode walk
    lazy62, _, _ = _lazy_step(synth.reads_list(52, 5000, 1500, 100, 0.01), 63, 2)
    dst = _dbg.Graph()
    with pytest.raises(_dbg.DbgError, match="63"):
        dst.build_from_walk(lazy62._graph, 64, lazy62._order, *empty)
    src.walk(True, 0)
    with pytest.raises(_dbg.DbgError, match="final"):
        _dbg.Graph().build_from_walk(src, 22, np.arange(src.sizes()["n_contigs"]), *empty)
    # a walk older than the graph
    src.build(21)
    with pytest.raises(_dbg.DbgError, match="walk"):
        _dbg.Graph().build_from_walk(src, 22, np.arange(n), *empty)
    assert src.sizes()["n_nodes"] == sz["n_nodes"]
    # a generic alphabet
    pep = load_golden("driver_peptide_k10_14")["inputs"]
    lp, _, _ = _lazy_step(list(pep["reads"]), pep["k_lowerlimit"], pep["threshold"])
    with pytest.raises(_dbg.DbgError, match="ACGT"):
        _dbg.Graph().build_from_walk(lp._graph, pep["k_lowerlimit"] + 1, np.arange(len(lp._order)), *empty)
