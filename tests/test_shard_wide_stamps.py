"""Sharded builds of two-word k-mers (k = 32..63) on ranks that hold 2 GiB of reads or more.

The records keep 4-byte rank-local stamps on the wire; bits 61..32 of such a stamp travel in bits 63..34 of the record's
meta word (dbg_wsk.h WREC_ST_HI).  No test needs gigabytes of k-mers for that: a rank's real reads go behind 2^31 bytes of
31-base reads of A, which hold no k-mer at k >= 32, so the real reads' rank-local stamps need bit 32 while the graph stays
small.  Every result is compared with the C oracle, or with one handle on the same concatenation (the path that already
keeps 64-bit stamps).  At most two padded ranks are alive at a time, and every handle is closed explicitly."""
import numpy as np
import pytest

import _dbg
import synth
from oracle import orc_c
from test_hip_multipass import check_successors, dense_counts, gather_parts
from test_part_traversal import check as check_traversal

pytestmark = pytest.mark.gpu

PAD_LEN = 31                                # < 32: no k-mer at any k > 31, and no branch k-mer either
N_PAD = -(-(1 << 31) // PAD_LEN)            # reads of padding: 2^31 bytes and a few more


def real_reads(rank, n_reads, read_len, seed=41):
    return synth.reads_ascii(seed, max(4 * read_len, n_reads * read_len // 5), n_reads, read_len, 0.01,
                             first_read=rank * n_reads)


def with_padding(reads, read_len, pad):
    """(bases, offsets) of a rank's reads, behind 2^31 bytes of padding reads when ``pad``."""
    offs = np.arange(0, reads.size + 1, read_len, dtype=np.uint64)
    if not pad:
        return reads.reshape(-1), offs
    n = N_PAD * PAD_LEN
    bases = np.empty(n + reads.size, dtype=np.uint8)
    bases[:n] = ord("A")
    bases[n:] = reads.reshape(-1)
    return bases, np.concatenate([np.arange(0, n, PAD_LEN, dtype=np.uint64), offs + np.uint64(n)])


def concatenation(ranks):
    """[(bases, offsets)] of the ranks -> (bases, offsets) of the rank-major concatenation."""
    bases = np.concatenate([b for b, _ in ranks])
    offs, at = [np.zeros(1, dtype=np.uint64)], 0
    for b, o in ranks:
        offs.append(o[1:] + np.uint64(at))
        at += b.size
    return bases, np.concatenate(offs)


def oracle(ranks, k):
    bases, offs = concatenation(ranks)
    return orc_c.build(bases, offs, k)


def check_shards(shards, want, k):
    """Shards of multi_gpu.sharded_build (node ids (owner << 29) | local id) == the oracle; every successor is the shifted k-mer."""
    keys = np.concatenate([s["keys"] for s in shards])
    keys_hi = np.concatenate([s["keys_hi"] for s in shards])
    stamps = np.concatenate([s["stamps"] for s in shards])
    counts = np.concatenate([s["counts"] for s in shards])
    assert keys.size == want["n_nodes"]
    assert int(stamps.max()) >= 1 << 32                        # the padded rank's nodes really have stamps above 32 bits
    o = np.argsort(stamps, kind="stable")
    assert np.array_equal(keys[o], want["keys"]) and np.array_equal(keys_hi[o], want["keys_hi"])
    assert np.array_equal(stamps[o], want["stamps"])
    assert np.array_equal(counts[o], want["counts"])
    u64 = np.uint64
    lo_mask = u64((1 << (2 * k)) - 1) if 2 * k < 64 else u64(0xFFFFFFFFFFFFFFFF)
    hi_mask = u64((1 << (2 * k - 64)) - 1)
    for s in shards:
        for code in range(4):
            has = s["counts"][:, code] != 0
            ref = s["succ"][has, code]
            assert np.all(ref != 0xFFFFFFFF)
            owner, idx = ref >> 29, ref & ((1 << 29) - 1)
            got, got_hi = np.empty(ref.size, dtype=np.uint64), np.empty(ref.size, dtype=np.uint64)
            for d, sd in enumerate(shards):
                sel = owner == d
                got[sel] = sd["keys"][idx[sel]]
                got_hi[sel] = sd["keys_hi"][idx[sel]]
            lo, hi = s["keys"][has], s["keys_hi"][has]
            assert np.array_equal(got, ((lo << u64(2)) | u64(code)) & lo_mask)
            assert np.array_equal(got_hi, ((hi << u64(2)) | (lo >> u64(62))) & hi_mask)


def sharded_in_process(ranks_reads, k, padded, options=()):
    """multi_gpu.sharded_build over len(ranks_reads) handles on cuda:0 (in-process exchange) -> exported shards."""
    import inproc_dist
    import multi_gpu

    def one(dist, rank):
        bases, offs = ranks_reads[rank]
        g = _dbg.Graph(device=0)
        for name, value in options:
            g.set_option(name, value)
        g.set_reads(bases, offs)
        multi_gpu.sharded_build(g, k, dist)
        assert g.shard_record_layout() == (4, 4)                 # the wire keeps 4-byte stamps, wide ranks included
        keys, stamps, counts, _ = g.export_nodes()
        out = {"keys": keys, "keys_hi": g.export_keys_hi(), "stamps": stamps, "counts": counts, "succ": g.export_succ()}
        g.close()
        return out

    assert sum(padded) <= 2
    return inproc_dist.run_ranks(len(ranks_reads), one)


@pytest.mark.parametrize("k", [40, 63])
def test_two_ranks_one_of_them_above_2_gib(k):
    read_len, per = 150, 3000
    ranks = [with_padding(real_reads(r, per, read_len), read_len, r == 0) for r in range(2)]
    want = oracle(ranks, k)
    check_shards(sharded_in_process(ranks, k, [True, False]), want, k)


def test_eight_shards_with_two_wide_senders():
    """Ranks 1 and 6 send stamps with high bits, the other six narrow ones: every receiver takes both."""
    k, read_len, per = 63, 150, 1000
    padded = [r in (1, 6) for r in range(8)]
    ranks = [with_padding(real_reads(r, per, read_len), read_len, padded[r]) for r in range(8)]
    want = oracle(ranks, k)
    check_shards(sharded_in_process(ranks, k, padded), want, k)


def ranks_times_passes(ranks_reads, k, n_passes, chunks, traverse=False):
    import inproc_dist
    import multi_gpu
    import part_traversal

    def one(dist, rank):
        bases, offs = ranks_reads[rank]
        g = _dbg.Graph(device=0)
        g.set_reads(bases, offs)
        multi_gpu.sharded_build_multipass(g, k, dist, n_passes, chunks=chunks)
        assert g.shard_record_layout() == (4, 4)
        out = part_traversal.traverse(g, k, 2, dist) if traverse else (gather_parts(g), g.sizes())
        g.close()
        return out

    return inproc_dist.run_ranks(len(ranks_reads), one)


@pytest.mark.parametrize("chunks", [1, 3])
def test_ranks_times_passes_with_a_rank_above_2_gib(chunks):
    k, read_len, per, n_ranks, n_passes = 63, 150, 2000, 4, 2
    ranks = [with_padding(real_reads(r, per, read_len), read_len, r == 2) for r in range(n_ranks)]
    want = oracle(ranks, k)
    got = ranks_times_passes(ranks, k, n_passes, chunks)
    parts = [d for rank_parts, _ in got for d in rank_parts]
    keys = np.concatenate([d["keys"] for d in parts])
    stamps = np.concatenate([d["stamps"] for d in parts])
    assert keys.size == want["n_nodes"] == sum(sz["n_nodes"] for _, sz in got)
    assert sum(sz["n_kmer_instances"] for _, sz in got) == want["n_kmer_instances"]
    assert sum(sz["n_edge_instances"] for _, sz in got) == want["n_edge_instances"]
    assert int(stamps.max()) >= 1 << 32
    o = np.argsort(stamps, kind="stable")
    assert np.array_equal(keys[o], want["keys"]) and np.array_equal(stamps[o], want["stamps"])
    assert np.array_equal(np.concatenate([d["keys_hi"] for d in parts])[o], want["keys_hi"])
    assert np.array_equal(np.concatenate([dense_counts(d) for d in parts])[o], want["counts"])
    assert check_successors(parts, k, n_passes) > 0


def test_traversal_in_parts_with_a_rank_above_2_gib():
    """part_traversal on ranks x passes with a wide rank == the single-handle path on the concatenation (pull-out flags
    of every read, the padding's included)."""
    k, read_len, per, n_ranks, n_passes = 63, 150, 2000, 4, 2
    ranks = [with_padding(real_reads(r, per, read_len, seed=42), read_len, r == 1) for r in range(n_ranks)]
    bases, offs = concatenation(ranks)
    want = single_handle_traversal(bases, offs, k, 2)
    assert want["branch"][0].size > 0 and want["n_pulled"] > 0 and want["contigs"][0].size > 0
    got = ranks_times_passes(ranks, k, n_passes, 1, traverse=True)
    flags = np.concatenate([r["read_flags"] for r in got])
    for r in got:
        check_traversal(r, want, flags)


def single_handle_traversal(bases, offs, k, threshold):
    """test_part_traversal.single_gpu_reference for reads of different lengths: the same calls on one handle."""
    g = _dbg.Graph()
    g.set_reads(bases, offs)
    g.build(k)
    g.refine_edge_order()
    g.prune(threshold)
    g.remove_tips()
    g.mark_pull_reads()
    keys, stamps, _, flags = g.export_nodes(counts=False)
    hi = g.export_keys_hi()
    br = np.nonzero(flags & _dbg.F_BRANCH)[0]
    br = br[np.argsort(stamps[br], kind="stable")]
    ranks = g.export_pull_ranks()
    pu = np.nonzero(flags & _dbg.F_PULLED)[0]
    pu = pu[np.argsort(ranks[pu], kind="stable")]
    read_flags = g.export_pull_reads()
    g.set_option("walk_jump_min_nodes", 0)
    g.walk(False, 1)
    off, score, stamp, seq = g.export_contig_index()
    o = np.lexsort((seq, stamp))
    out = {"branch": (keys[br], hi[br]), "pulled": (keys[pu], hi[pu]), "read_flags": read_flags,
           "contigs": (stamp[o], (off[1:] - off[:-1])[o].astype(np.int64), score[o].astype(np.int64)),
           "n_pulled": int(pu.size)}
    g.close()
    return out


def _mix(x):
    """splitmix-style finaliser on int64 tensors (wrapping arithmetic, logical shifts)."""
    for c in (-0xAE502812AA7333, -0x3B314601E57A13AD):            # 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53 as int64
        x = x ^ ((x >> 33) & ((1 << 31) - 1))
        x = x * c
    return x ^ ((x >> 33) & ((1 << 31) - 1))


def device_digest(g):
    """Order-independent digest of (keys, keys_hi, stamps, counts) of a handle's nodes, on the device."""
    import torch
    t = g.node_tensors()
    c = t["counts"].view(-1, 4).to(torch.int64)
    w = c[:, 0] + 3 * c[:, 1] + 5 * c[:, 2] + 7 * c[:, 3] + 1
    h = _mix(t["keys"] ^ _mix(t["keys_hi"] ^ 0x5851F42D4C957F2D) ^ _mix(t["stamps"]) ^ _mix(w))
    return int(h.sum().item()), int(c.sum().item())


def test_a_real_rank_above_2_gib():
    """15 M x 150 bp of real reads on one rank (2.25 GB) plus a small rank, k = 63: node and edge totals and a device digest
    of the nodes equal one handle's build of both ranks' reads."""
    import inproc_dist
    import multi_gpu
    k, read_len, genome, err, seed = 63, 150, 2_000_000, 0.001, 7
    n_reads = [15_000_000, 200_000]

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        g.synth_reads(seed, genome, n_reads[rank], read_len, err, first_read=sum(n_reads[:rank]))
        assert (g.sizes()["n_bytes"] >= 1 << 31) == (rank == 0)
        multi_gpu.sharded_build(g, k, dist)
        sz = g.sizes()
        out = (sz["n_nodes"], sz["n_edges"], sz["n_kmer_instances"]) + device_digest(g)
        g.close()
        return out

    got = inproc_dist.run_ranks(2, one)
    g = _dbg.Graph(device=0)
    g.synth_reads(seed, genome, sum(n_reads), read_len, err)
    g.build(k)
    sz = g.sizes()
    digest, total_count = device_digest(g)
    g.close()
    assert sum(r[0] for r in got) == sz["n_nodes"] and sum(r[1] for r in got) == sz["n_edges"]
    assert sum(r[2] for r in got) == sz["n_kmer_instances"] == sum(n_reads) * (read_len - k + 1)
    assert sum(r[4] for r in got) == total_count
    assert sum(r[3] for r in got) % (1 << 64) == digest % (1 << 64)


def test_shard_stamp64_below_2_gib_sends_the_same_messages():
    """"shard_stamp64" takes the 64-bit sender path at a small size: the same (4, 4) layout, the same records to every owner
    bit for bit (the high bits are zero) and the same graph."""
    import torch
    k, read_len, per = 63, 150, 3000
    reads = real_reads(0, per, read_len)
    bases, offs = with_padding(reads, read_len, False)
    sent = []
    for wide in (0, 1):
        g = _dbg.Graph(device=0)
        g.set_option("shard_stamp64", wide)
        g.set_reads(bases, offs)
        counts, arrays = g.shard_extract(k, 4)
        assert g.shard_record_layout() == (4, 4) and arrays[2].dtype == torch.int32
        w0, w1, st = (a.cpu().numpy() for a in arrays)
        rows = np.concatenate([w0.reshape(-1, 4), w1.reshape(-1, 1), st.astype(np.int64).reshape(-1, 1)], axis=1)
        sent.append((counts, rows))
        g.close()
    assert sent[0][0] == sent[1][0]
    at = 0
    for c in sent[0][0]:  # the message to every owner, as a multiset of records (the multisplit keeps no order inside a bucket)
        a, b = (rows[at:at + c] for _, rows in sent)
        assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])
        at += c
    assert at == sent[0][1].shape[0]
    ranks = [with_padding(real_reads(r, per, read_len), read_len, False) for r in range(2)]
    want = oracle(ranks, k)
    shards = sharded_in_process(ranks, k, [False, False], options=[("shard_stamp64", 1)])
    stamps = np.concatenate([s["stamps"] for s in shards])
    o = np.argsort(stamps, kind="stable")
    assert np.array_equal(np.concatenate([s["keys"] for s in shards])[o], want["keys"])
    assert np.array_equal(stamps[o], want["stamps"])
    assert np.array_equal(np.concatenate([s["counts"] for s in shards])[o], want["counts"])
