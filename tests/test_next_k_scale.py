"""The k -> k+1 step from the walk (dbg_build_from_walk) at the benchmarked size: BASELINE configs[1] (10 M x 150 bp, 1 %
errors, k = 31, threshold 2), whose contig text (1.9e12 characters) cannot be spelled, and its first 1 M reads, where the
result is compared with the text path."""
import contextlib
import io
import json
import threading
import time

import numpy as np
import pytest

import _dbg
import debruijn

pytestmark = pytest.mark.gpu

GENOME = 50_000_000  # configs[1]: 30x coverage of a 50 Mbp genome, seed 1
READ_LEN = 150


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _device_reads(tmp_path, n):
    """The first n reads of configs[1] as a FASTA file, read back on the device (what the driver's CLI does)."""
    g = _dbg.Graph()
    g.synth_reads(1, GENOME, n, READ_LEN, 0.01)
    bases, _ = g.copy_reads()
    g.close()
    path = tmp_path / "reads.fasta"
    with open(path, "wb") as fh:
        step = 1 << 20
        for i in range(0, n, step):
            m = min(step, n - i)
            rec = np.empty((m, 3 + READ_LEN + 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            rec[:, 3:3 + READ_LEN] = bases[i * READ_LEN:(i + m) * READ_LEN].reshape(m, READ_LEN)
            rec[:, -1] = ord("\n")
            fh.write(rec.tobytes())
    del bases
    return debruijn.read_reads_device(str(path))


class _PeakMemory:
    """Most device memory in use while the block runs (sampled every millisecond: hipMemGetInfo through torch)."""

    def __enter__(self):
        import torch
        self._info = lambda: torch.cuda.mem_get_info(_dbg.default_device())
        free, total = self._info()
        self.before = total - free
        self.peak = self.before
        self._stop = False
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def _run(self):
        while not self._stop:
            free, total = self._info()
            self.peak = max(self.peak, total - free)
            time.sleep(0.001)

    def __exit__(self, *exc):
        self._stop = True
        self._t.join()


def _step_k(reads, k, thr, max_chars):
    debruijn.MAX_CONTIG_CHARS = max_chars
    g, pull, branch, pulled, _ = _quiet(debruijn.construct_graph, reads, k, threshold=thr)
    lazy = _quiet(debruijn.output_contigs, g, branch, pulled)
    assert isinstance(lazy, debruijn.LazyContigs)
    lazy.sort(reverse=True)
    lazy.extend(pull)
    return lazy


def _counting_calls(monkeypatch):
    calls = []
    real = _dbg.Graph.build_from_walk
    monkeypatch.setattr(_dbg.Graph, "build_from_walk", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def test_configs1_next_k(monkeypatch, tmp_path):
    """construct_graph(lazy, 32) completes at configs[1]; time, n_nodes and peak device memory go to the output."""
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 0)
    reads = _device_reads(tmp_path, 10_000_000)
    lazy = _step_k(reads, 31, 2, 0)
    n_ctg = len(lazy._order)
    src_sz = lazy._graph.sizes()
    assert src_sz["contig_chars"] > (1 << 40)  # the text path would have to spell all of it
    calls = _counting_calls(monkeypatch)
    monkeypatch.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("contig text fetched")))
    with _PeakMemory() as mem:
        t0 = time.perf_counter()
        res = _quiet(debruijn.construct_graph, lazy, 32, threshold=2)
        dt = time.perf_counter() - t0
    assert calls == [1]
    g32 = res[0][0]._graph
    sz = g32.sizes()
    assert sz["n_reads"] == len(lazy) and sz["n_bytes"] == src_sz["contig_chars"] + sum(map(len, lazy._tail))
    assert sz["n_nodes"] > 0 and sz["n_branch"] > 0
    pulled = res[1]
    pulled_ctg = [i for i in pulled._idx if i < n_ctg]
    out = {"what": "construct_graph(lazy, 32) at configs[1]", "seconds": round(dt, 3),
           "n_nodes_k32": sz["n_nodes"],
           "n_edges_k32": sz["n_edges"], "n_branch_k32": sz["n_branch"], "n_contigs_k31": n_ctg,
           "contig_chars_k31": src_sz["contig_chars"], "n_extra_reads": len(lazy._tail),
           "peak_device_bytes": mem.peak, "device_bytes_before": mem.before,
           "n_pull_reads_k32": len(pulled), "pulled_contigs_k32": len(pulled_ctg),
           "pulled_contig_chars_k32": int(sum(lazy.lengths[i] for i in pulled_ctg))}
    print("NEXTK_SCALE " + json.dumps(out))


def _graph_arrays(g):
    """Every node of a graph in dict (stamp) order: keys, stamps, counts, flags, keep mask and successor ranks."""
    keys, stamps, counts, flags = g.export_nodes()
    order, fsorder = g.export_orders()
    hi = g.export_keys_hi() if g.sizes()["k"] > 31 else np.zeros_like(keys)
    p = np.argsort(stamps, kind="stable")
    counts = counts[p]

    def ranked(r):  # successor codes by rank, the codes without a count dropped (their place is no part of the graph)
        r = np.asarray(r)[p].astype(np.int64)
        valid = r < 4
        r = np.where(valid & (np.take_along_axis(counts, np.where(valid, r, 0), axis=1) != 0), r, 4)
        return np.take_along_axis(r, np.argsort(r == 4, axis=1, kind="stable"), axis=1)

    return [a[p] for a in (keys, hi, stamps, flags, g.export_keepmask())] + [counts, ranked(order), ranked(fsorder)]


def test_1m_reads_equal_text_path(monkeypatch, tmp_path):
    """The first 1 M reads of configs[1]: the k+1 graph, its lists, pull-out reads and contig index equal the text path's;
    both times go to the output."""
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)
    reads = _device_reads(tmp_path, 1_000_000)
    lazy = _step_k(reads, 31, 2, 1)
    t0 = time.perf_counter()
    texts = [lazy[i] for i in range(len(lazy._order))] + list(lazy._tail)
    t_fetch = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = _quiet(debruijn.construct_graph, texts, 32, threshold=2)
    t_text = time.perf_counter() - t0
    calls = _counting_calls(monkeypatch)
    with monkeypatch.context() as m:
        m.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("contig text fetched")))
        t0 = time.perf_counter()
        got = _quiet(debruijn.construct_graph, lazy, 32, threshold=2)
        t_new = time.perf_counter() - t0
    assert calls == [1]
    gw, gg = want[0][0]._graph, got[0][0]._graph
    for a, b in zip(_graph_arrays(gw), _graph_arrays(gg)):
        np.testing.assert_array_equal(a, b)
    assert list(got[2]) == list(want[2]) and list(got[3]) == list(want[3])  # branch_kmer, already_pull_out
    np.testing.assert_array_equal(gg.export_pull_reads(), gw.export_pull_reads())
    assert list(got[1]) == list(want[1])
    cw = _quiet(debruijn.output_contigs, want[0], want[2], want[3])
    cg = _quiet(debruijn.output_contigs, got[0], got[2], got[3])
    assert cg.lengths == cw.lengths and cg.scores == cw.scores
    for i in range(0, len(cg), max(1, len(cg) // 200)):  # a spread of texts (each is one device fetch)
        assert cg[i] == cw[i]
    print("NEXTK_1M " + json.dumps({"n_nodes_k32": gg.sizes()["n_nodes"], "contig_chars_k31": len(texts) and
                                    int(sum(lazy.lengths)), "text_path_seconds": round(t_text, 3),
                                    "text_fetch_seconds": round(t_fetch, 3), "new_path_seconds": round(t_new, 3)}))


def _fasta_device_reads(tmp_path, bases, read_len):
    """Fixed-length reads (bases) as a FASTA file, read back on the device."""
    n = bases.size // read_len
    rec = np.empty((n, 3 + read_len + 1), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
    rec[:, 3:3 + read_len] = bases.reshape(n, read_len)
    rec[:, -1] = ord("\n")
    path = tmp_path / "reads.fasta"
    path.write_bytes(rec.tobytes())
    return debruijn.read_reads_device(str(path))


NEXTK_TEXT_BOUND = 4 << 30   # characters of contig text the oracle spells for the k + 1 build


@pytest.mark.parametrize("src,n,k", [("configs1", 1_000_000, 31), ("g10m", 300_000, 62)])
def test_next_k_equals_c_oracle(monkeypatch, tmp_path, src, n, k):
    """construct_graph(lazy, k + 1) (dbg_build_from_walk, no text) against the C oracle's own k -> k + 1 step: its
    contigs sorted stably by score, descending (II_assembleFromReads.py:64), its pull-out reads appended (:74), that
    text spelled and built at k + 1, then traversed.  Node table, ranks, branch and pulled lists, pull-out reads and the
    contig index must be equal."""
    import synth
    import test_traversal_vs_c_oracle as tv
    from oracle import orc_c
    thr = 2
    monkeypatch.setattr(debruijn, "MAX_CONTIG_CHARS", 1)   # the k walk keeps no text: the driver gets LazyContigs
    if src == "configs1":     # the first n reads of configs[1]
        g0 = _dbg.Graph()
        g0.synth_reads(1, GENOME, n, READ_LEN, 0.01)
        bases, off = g0.copy_reads()
        g0.close()
    else:                     # 4.5x of a 10 Mbp genome: branches and tips at k = 62 and 63
        bases = synth.reads_ascii(4, 10_000_000, n, READ_LEN, 0.01).reshape(-1)
        off = np.arange(0, bases.size + 1, READ_LEN, dtype=np.uint64)

    # the oracle's step: k-graph, sorted contigs + pull-out reads, (k+1)-graph
    t0 = time.perf_counter()
    o = orc_c.Oracle(bases, off, k)
    t = o.traverse(thr)
    assert t["branch"].size > 0 and t["n_pull_reads"] > 0
    order = np.argsort(-t["score"].astype(np.int64), kind="stable")
    assert t["contig_chars"] < NEXTK_TEXT_BOUND, t["contig_chars"]
    text, toff = o.spell(order)
    want_scores, want_lengths = t["score"][order], t["chars"][order]
    o.close()
    pr = np.nonzero(t["read_flags"])[0]
    starts, lens = off[pr], np.diff(off)[pr]
    pull_bytes = np.concatenate([bases[int(a):int(a + b)] for a, b in zip(starts, lens)])
    nbases = np.concatenate([text, pull_bytes])
    noff = np.concatenate([toff, toff[-1] + np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)
    del text, pull_bytes
    o1 = orc_c.Oracle(nbases, noff, k + 1)
    t1 = o1.traverse(thr)
    oracle_s = time.perf_counter() - t0

    # the device's step, through the driver's surface
    reads = _fasta_device_reads(tmp_path, bases, READ_LEN)
    del bases
    t0 = time.perf_counter()
    lazy = _step_k(reads, k, thr, 1)
    assert lazy.scores == want_scores.tolist() and lazy.lengths == want_lengths.tolist()   # the stable score sort
    assert len(lazy._tail) == pr.size
    calls = _counting_calls(monkeypatch)
    monkeypatch.setattr(_dbg.Graph, "export_contig_text", lambda *a: (_ for _ in ()).throw(AssertionError("contig text fetched")))
    got = _quiet(debruijn.construct_graph, lazy, k + 1, threshold=thr)
    assert calls == [1]                                            # the dbg_build_from_walk path was taken
    gg = got[0][0]._graph
    assert gg.sizes()["n_reads"] == noff.size - 1 and gg.sizes()["n_bytes"] == int(noff[-1])
    gg.walk(False, 0)
    # node arrays are exported when compare() reaches them (host memory: one device array at a time next to the oracle)
    dev = {"keys": lambda: gg.export_nodes(True, False, False, False)[0], "hi": gg.export_keys_hi,
           "stamps": lambda: gg.export_nodes(False, True, False, False)[1],
           "counts": lambda: gg.export_nodes(False, False, True, False)[2],
           "flags": lambda: gg.export_nodes(False, False, False, True)[3], "keep": gg.export_keepmask,
           "order": lambda: gg.export_orders()[0], "ranks": gg.export_pull_ranks, "read_flags": gg.export_pull_reads()}
    dev["contig_off"], dev["score"], dev["stamp"], dev["seq"] = gg.export_contig_index()
    device_s = time.perf_counter() - t0
    tv.compare(o1, t1, dev, k + 1)
    assert t1["branch"].size > 0 and t1["pulled"].size > 0 and t1["score"].size > 0
    tv.report(f"next_k {src} {n} reads k={k}->{k + 1}", o1, t1, oracle_s, device_s,
              f"k_contigs {order.size} k_contig_chars {int(toff[-1])} appended_reads {pr.size}")
    o1.close()
