"""Both strands on the device (dbg_add_revcomp, csrc/dbg_revcomp.h): the definition

    both_strands(reads) = [r0, revcomp(r0), r1, revcomp(r1), ...]

against the device pass on inputs built for the borders the tile kernel names (its tile of output bytes, the offsets slice
it keeps in LDS, the 16-byte chunk), through lent tensors, and through every surface: the graph against the Python oracle
run on the doubled list, origins after a split, the FASTA / FASTQ routes, sharded ingest, builds in parts, the driver."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

import _dbg
import debruijn as prod
import synth
from golden_util import canonical

pytestmark = pytest.mark.gpu

T = _dbg.RC_TILE_BYTES
MOVED = frozenset(b"ACGTacgt")
COUNTS = ("n_reads_in", "n_bytes_in", "n_reads_out", "n_bytes_out", "n_other_bytes", "n_palindromes")


def pack(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def unpack(bases, off):
    raw = bases.tobytes()
    return [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def host_counts(reads):
    n = sum(len(r) for r in reads)
    return {"n_reads_in": len(reads), "n_bytes_in": n, "n_reads_out": 2 * len(reads), "n_bytes_out": 2 * n,
            "n_other_bytes": n - sum(c in MOVED for c in b"".join(reads)),
            "n_palindromes": sum(len(r) > 0 and prod.revcomp(r) == r for r in reads)}


def check_doubling(h, reads, name="", origins=False):
    """the reads now on handle h -> add_revcomp -> bases, offsets and every count against the host statement
    (origins: the handle holds the origins of a split that cut something, which the call doubles too)"""
    want = prod.both_strands(reads)
    st = h.add_revcomp()
    wc = host_counts(reads)
    for f in COUNTS:
        assert st[f] == wc[f], (name, f, st, wc)
    assert st["peak_extra_device_bytes"] == 2 * wc["n_bytes_in"] + 64 + 8 * (2 * len(reads) + 1) + \
        (32 * max(len(reads), 1) if origins else 0), (name, st)
    assert st["ms_kernel"] >= 0
    sz = h.sizes()
    assert sz["n_reads"] == 2 * len(reads) and sz["n_bytes"] == wc["n_bytes_out"], name
    got_b, got_o = h.copy_reads()
    wb, wo = pack(want)
    assert np.array_equal(got_o, wo), name
    assert np.array_equal(got_b, wb), (name, np.flatnonzero(got_b != wb)[:8])
    return st


def rand_reads(rng, lens, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return [a[rng.integers(0, a.size, int(n))].tobytes() for n in lens]


def border_sets():
    rng = np.random.default_rng(18)
    mixed = b"ACGTacgtNnRY-*\x80\xc1\xe1\xff"
    yield "n = 0", []
    yield "one empty read", [b""]
    yield "one byte", [b"G"]
    for n in (T - 1, T, T + 1, T // 2, 3 * T + 5):  # a read over several output tiles, its strands starting in different ones
        yield f"single read of {n}", rand_reads(rng, [n])
    yield "empty runs", [b""] * 5000 + [b"GATTACA"] + [b""] * 5000  # more reads in a tile than the offsets slice holds
    short = rand_reads(rng, rng.integers(0, 41, 20000))
    for i in range(0, 20000, 97):
        short[i] = (b"ACGT", b"AATT", b"N", b"GAATTC", b"acgt", b"ANT")[(i // 97) % 6]  # planted palindromes
    assert host_counts(short)["n_palindromes"] >= 200
    yield "20 000 short reads", short
    yield "lengths 16 +- 1", rand_reads(rng, np.tile([15, 16, 17, 17, 15, 16, 16, 15], 64))  # borders at every alignment
    for k in (1, 3):
        for d in (-1, 0, 1):  # the doubled total is k T + 2 d: the last tile ends on, just before, just behind a border
            yield f"N = {k} T / 2 {d:+d}", rand_reads(rng, [150] * ((k * T // 2 + d) // 150) + [(k * T // 2 + d) % 150])
    for d in (-1, 1):  # and the input total itself next to a multiple of the tile
        yield f"N = 2 T {d:+d}", rand_reads(rng, [150] * ((2 * T + d) // 150) + [(2 * T + d) % 150])
    yield "other bytes", rand_reads(rng, rng.integers(0, 200, 300), mixed)
    yield "peptides", rand_reads(rng, rng.integers(5, 60, 300), b"ACDEFGHIKLMNPQRSTVWY")


@pytest.fixture(scope="module")
def g():
    h = _dbg.Graph()
    yield h
    h.close()


# ---- 1. bytes and offsets are exactly the rule ----------------------------------------------------------------------------
def test_bytes_offsets_and_counts_are_the_rule(g):
    seen = set()
    for name, reads in border_sets():
        g.set_reads(*pack(reads))
        check_doubling(g, reads, name)
        seen.add((sum(map(len, reads)) * 2) % 16)
    assert len(seen) > 2  # totals that are no whole chunk


def test_unknown_flags_and_a_handle_without_reads():
    h = _dbg.Graph()
    with pytest.raises(_dbg.DbgError) as e:
        h.add_revcomp()
    assert e.value.code == _dbg.DBG_E_ARG
    h.set_reads(*pack([b"ACGT"]))
    for flags in (1, 2, 1 << 31):
        assert h._lib.dbg_add_revcomp(h._h, flags, None) == _dbg.DBG_E_ARG
    assert unpack(*h.copy_reads()) == [b"ACGT"]  # a refused call leaves the reads
    assert h._lib.dbg_add_revcomp(h._h, 0, None) == _dbg.DBG_OK  # the stats are optional
    assert unpack(*h.copy_reads()) == [b"ACGT", b"ACGT"]
    h.close()


# ---- 2. lent buffers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tail", [0, 1, 15, 16, 33])
def test_lent_tensors_are_never_written_and_nothing_behind_them_is_needed(n_tail):
    import torch
    rng = np.random.default_rng(n_tail)
    reads = rand_reads(rng, [40, 0, 17, 150, 1, 16] * 30 + [n_tail], b"ACGTN")
    b, off = pack(reads)
    guard = np.full(64, 0x5A, np.uint8)
    whole = np.concatenate([guard, b, guard])
    tw = torch.from_numpy(whole).cuda()
    tb = tw[64:64 + b.size]  # no padding: the guard follows the last base
    to = torch.from_numpy(off.astype(np.int64)).cuda()
    h = _dbg.Graph()
    h.set_reads_tensors(tb, to)
    lent = h.reads_tensors()
    assert (lent[0].data_ptr(), lent[1].data_ptr()) == (tb.data_ptr(), to.data_ptr())
    check_doubling(h, reads, f"lent, tail {n_tail}")
    assert np.array_equal(tw.cpu().numpy(), whole) and np.array_equal(to.cpu().numpy(), off.astype(np.int64))
    now = h.reads_tensors()
    assert now[0].data_ptr() != tb.data_ptr() and now[1].data_ptr() != to.data_ptr()
    lo, hi = tw.data_ptr(), tw.data_ptr() + tw.numel()
    assert not lo <= now[0].data_ptr() < hi
    h.close()


# ---- 3. the graph ---------------------------------------------------------------------------------------------------------
def stranded_reads():
    """2 000 reads x 60 bp from a random 20 kbp genome, about half of them from the other strand, 1 % with substitutions"""
    rng = np.random.default_rng(2018)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20000)].tobytes().decode()
    reads, flipped = [], 0
    for _ in range(2000):
        s = int(rng.integers(0, 20000 - 60))
        r = genome[s:s + 60]
        if rng.random() < 0.01:
            p = int(rng.integers(0, 60))
            r = r[:p] + "ACGT"[("ACGT".index(r[p]) + 1 + int(rng.integers(0, 3))) % 4] + r[p + 1:]
        if rng.random() < 0.5:
            r = prod.revcomp(r)
            flipped += 1
        reads.append(r)
    assert 800 < flipped < 1200
    return reads


@pytest.fixture(scope="module")
def stranded():
    return stranded_reads()


@pytest.mark.parametrize("k", [21, 40])
def test_graph_of_both_strands_is_the_oracle_on_the_doubled_list(k, stranded, tmp_path):
    from oracle import dbg_oracle as orc
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, stranded)
    doubled = prod.both_strands(stranded)
    dev = prod.DeviceReads(p, strands="both")
    assert len(dev) == 2 * len(stranded) and dev.revcomp_stats["n_reads_out"] == len(doubled)
    with contextlib.redirect_stdout(io.StringIO()):
        g_, pull, branch, pulled, ect = prod.construct_graph(dev, k, threshold=2)
        contigs = prod.output_contigs(g_, branch, pulled)
        got = canonical(g_, pull, branch, pulled, ect, contigs)
        og, opull, obranch, opulled, oect = orc.construct_graph(list(doubled), k, threshold=2)
        ocontigs = orc.output_contigs(og, obranch, opulled)
        want = canonical(og, opull, obranch, opulled, oect, ocontigs)
    assert len(want["vertices"]) > 10000 and len(want["contigs"]) > 0
    for field in want:
        assert got[field] == want[field], field


@pytest.mark.parametrize("k", [21, 40])
def test_every_node_has_its_reverse_complement_only_with_both_strands(k, stranded):
    def missing(h):
        h.build(k)
        keys, _, _, _ = h.export_nodes(stamps=False, counts=False, flags=False)
        hi = h.export_keys_hi()
        rc = [_dbg.encode_kmer(prod.revcomp(s)) for s in _dbg.decode_keys(keys, k, keys_hi=hi)]
        lo_w = np.asarray([x & ((1 << 64) - 1) for x in rc], dtype=np.uint64)
        hi_w = np.asarray([x >> 64 for x in rc], dtype=np.uint64)
        ids = h.lookup_nodes(lo_w, hi_w)
        return int((ids == _dbg.NO_NODE).sum()), keys.size

    h = _dbg.Graph()
    h.set_reads(*pack([r.encode() for r in stranded]))
    absent, n = missing(h)
    assert absent > n // 100  # the input is not symmetric by itself
    h.set_reads(*pack([r.encode() for r in stranded]))
    h.add_revcomp()
    absent2, n2 = missing(h)
    assert absent2 == 0 and n2 > n
    h.close()


# ---- 4. origins -----------------------------------------------------------------------------------------------------------
def test_origins_are_doubled_after_a_split_and_refused_without_one(g):
    rng = np.random.default_rng(4)
    reads = rand_reads(rng, rng.integers(0, 120, 500), b"ACGTACGTACGTACGTNn")
    g.set_reads(*pack(reads))
    g.split_reads()
    rd, pos = g.read_origins()
    pieces = unpack(*g.copy_reads())
    assert pieces == prod.acgt_pieces(reads) and len(pieces) > len(reads)
    check_doubling(g, pieces, origins=True)
    rd2, pos2 = g.read_origins()
    assert np.array_equal(rd2, np.repeat(rd, 2)) and np.array_equal(pos2, np.repeat(pos, 2))
    for j, piece in enumerate(unpack(*g.copy_reads())):  # strand j & 1 of piece j >> 1, pos in forward orientation
        fwd = prod.revcomp(piece) if j & 1 else piece
        assert reads[int(rd2[j])][int(pos2[j]):int(pos2[j]) + len(fwd)] == fwd
    # identity origins (a split that had nothing to cut) become (j >> 1, 0), and again after a second doubling
    plain = rand_reads(rng, [30] * 10)
    g.set_reads(*pack(plain))
    assert g.split_reads()["changed"] == 0
    g.add_revcomp()
    rd, pos = g.read_origins()
    assert rd.tolist() == [j >> 1 for j in range(20)] and not pos.any()
    g.add_revcomp()
    rd, pos = g.read_origins()
    assert rd.tolist() == [j >> 2 for j in range(40)] and not pos.any()
    g.set_reads(*pack(plain))
    g.add_revcomp()
    with pytest.raises(_dbg.DbgError) as e:
        g.read_origins()  # no split on this read set: as before
    assert e.value.code == _dbg.DBG_E_ARG


def test_peak_counts_the_doubled_origins_of_a_split(g):
    reads = [b"ACGTNACGT", b"NN", b"AC"]
    g.set_reads(*pack(reads))
    g.split_reads()
    st = g.add_revcomp()
    assert st["n_reads_in"] == 3 and st["peak_extra_device_bytes"] == 2 * 10 + 64 + 8 * 7 + 32 * 3


# ---- 5. surfaces ----------------------------------------------------------------------------------------------------------
def masked_reads():
    reads = synth.reads_list(41, 3000, 400, 80, 0.005)
    rng = np.random.default_rng(3)
    for i in rng.choice(400, 40, replace=False):
        r = bytearray(reads[i].encode())
        for p in rng.integers(0, 80, rng.integers(1, 4)):
            r[p] = ord("N")
        reads[i] = r.decode()
    reads[5] = "N" * 80
    reads[7] = ""
    return reads


def test_fasta_and_fastq_routes_list_both_strands_of_the_pieces(tmp_path):
    reads = masked_reads()
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, reads)
    want = prod.both_strands(prod.acgt_pieces(reads))
    assert list(prod.DeviceReads(p)) == reads and prod.DeviceReads(p).revcomp_stats is None  # the default: unchanged
    assert list(prod.read_reads_device(p, strands="both")) == prod.both_strands(reads)
    for kw in ({}, {"chunk_bytes": 64}):
        dev = prod.read_reads_device(p, non_acgt="split", strands="both", **kw)
        assert list(dev) == want and len(dev) == len(want)
        assert dev.revcomp_stats["n_reads_in"] == len(want) // 2 == dev.split_stats["n_reads_out"]
        rd, pos = dev.origins()
        for j, piece in enumerate(want):
            fwd = prod.revcomp(piece) if j & 1 else piece
            assert reads[int(rd[j])][int(pos[j]):int(pos[j]) + len(fwd)] == fwd
    q = str(tmp_path / "reads.fastq")
    synth.write_fastq(q, [r for r in reads if r], seed=5)
    lines = prod.read_fastq(q, min_quality=20)
    assert any("N" in a and "N" not in b for a, b in zip(lines, [r for r in reads if r]))  # the mask did something
    dev = prod.read_reads_device(q, format="fastq", min_quality=20, non_acgt="split", strands="both")
    assert list(dev) == prod.both_strands(prod.acgt_pieces(lines))
    with pytest.raises(ValueError):
        prod.DeviceReads(p, strands="sideways")
    with pytest.raises(ValueError):
        prod.read_reads_device(p, strands=None)


def sorted_nodes(keys, hi, stamps, counts):
    o = np.lexsort((hi, keys))
    return keys[o], hi[o], stamps[o], counts[o]


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_double_their_own_reads_before_the_sharded_build(world, tmp_path):
    import inproc_dist
    import multi_gpu
    k = 31
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, masked_reads() + synth.reads_list(9, 3000, 800, 90, 0.01))

    def one(dist, rank):
        h = _dbg.Graph(device=0)
        multi_gpu.set_reads_fasta_shard(h, p, dist, chunk_bytes=1 << 14, non_acgt="split", strands="both")
        mine = unpack(*h.copy_reads())
        multi_gpu.sharded_build(h, k, dist)
        keys, stamps, counts, _ = h.export_nodes(flags=False)
        out = (keys, h.export_keys_hi(), stamps, counts, mine)
        h.close()
        return out

    shards = inproc_dist.run_ranks(world, one)
    whole = prod.DeviceReads(p, non_acgt="split", strands="both")
    assert [r.decode("latin-1") for s in shards for r in s[4]] == list(whole)  # rank order is file order
    whole._graph.build(k)
    keys, stamps, counts, _ = whole._graph.export_nodes(flags=False)
    want = sorted_nodes(keys, whole._graph.export_keys_hi(), stamps, counts)
    got = sorted_nodes(*(np.concatenate([s[i] for s in shards]) for i in range(4)))
    assert want[0].size == got[0].size > 0
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        multi_gpu.set_reads_fasta_shard(whole._graph, p, None, strands="sideways")


def test_build_in_four_parts_of_both_strands_equals_the_single_build(stranded):
    k = 31
    reads = [r.encode() for r in stranded]
    a, b = _dbg.Graph(), _dbg.Graph()
    a.set_reads(*pack(reads))
    a.add_revcomp()
    a.build_multipass(k, 4)
    assert a.part_count() == 4
    parts = [a.export_part(p) for p in range(4)]
    b.set_reads(*pack(reads))
    b.add_revcomp()
    b.build(k)
    keys, stamps, counts, _ = b.export_nodes(flags=False)
    o = np.argsort(keys, kind="stable")
    pk, ps = np.concatenate([d["keys"] for d in parts]), np.concatenate([d["stamps"] for d in parts])
    po = np.argsort(pk, kind="stable")
    assert pk.size == keys.size == a.sizes()["n_nodes"] > 0
    assert np.array_equal(pk[po], keys[o]) and np.array_equal(ps[po], stamps[o])
    deg = np.concatenate([np.diff(d["row_ptr"].astype(np.int64)) for d in parts])
    assert np.array_equal(deg[po], (counts != 0).sum(axis=1)[o])
    cnt = np.concatenate([np.add.reduceat(np.concatenate([d["cnt"], [0]]).astype(np.int64), d["row_ptr"][:-1].astype(np.int64))
                          * (np.diff(d["row_ptr"].astype(np.int64)) > 0) for d in parts])
    assert np.array_equal(cnt[po], counts.astype(np.int64).sum(axis=1)[o])
    a.close()
    b.close()


def test_driver_with_both_strands_in_the_settings_equals_the_oracle_on_the_doubled_reads(tmp_path):
    from oracle import dbg_oracle as orc
    reads = synth.reads_list(41, 3000, 400, 80, 0.005)
    rng = np.random.default_rng(6)
    reads = [prod.revcomp(r) if rng.random() < 0.5 else r for r in reads]
    froot = "stranded"
    synth.write_froot(str(tmp_path / froot), reads, 15, 17, threshold=2)
    with open(tmp_path / froot / "setting.json") as fh:
        setting = json.load(fh)
    setting.update(strands="both")
    with open(tmp_path / froot / "setting.json", "w") as fh:
        json.dump(setting, fh)
    subprocess.check_call([sys.executable, os.path.join(PKG, "II_assembleFromReads.py"), "-froot", froot],
                          cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=PKG), stdout=subprocess.DEVNULL)
    out = (tmp_path / froot / f"{froot}.fasta").read_text().splitlines()
    with contextlib.redirect_stdout(io.StringIO()):
        want, _ = orc.assemble(prod.both_strands(reads), 15, 17, 2)
        forward, _ = orc.assemble(reads, 15, 17, 2)
    assert out[1::2] == want and want != forward and len(want) > 0
    assert out[0] == ">SEQUENCE_0_17mer"


# ---- 6. state -------------------------------------------------------------------------------------------------------------
def test_a_prior_graph_is_gone_and_twice_doubles_twice(g):
    reads = [r.encode() for r in synth.reads_list(3, 5000, 300, 100, 0.01)]
    g.set_reads(*pack(reads))
    g.build(21)
    g.prune(2)
    g.remove_tips()
    g.walk(False)
    assert g.sizes()["n_nodes"] > 0
    g.add_revcomp()
    assert g.sizes()["n_nodes"] == 0 and g.sizes()["k"] == 0
    with pytest.raises(_dbg.DbgError) as e:
        g.walk(False)
    assert e.value.code == _dbg.DBG_E_ARG
    g.set_reads(*pack(reads))
    with pytest.raises(_dbg.DbgError) as e2:
        g.walk(False)
    assert e2.value.code == _dbg.DBG_E_ARG  # as after set_reads
    g.add_revcomp()
    g.add_revcomp()
    assert unpack(*g.copy_reads()) == prod.both_strands(prod.both_strands(reads))
    g.build(21)  # and the doubled reads build
    assert g.sizes()["n_nodes"] > 0
