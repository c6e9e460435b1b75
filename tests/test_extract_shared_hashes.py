"""The register extraction (k_sk_extract_w) hashes every m-mer once: a lane takes the hashes its windows reach beyond its own
32 positions from the next lane, a wave's last lane from LDS, and finds the record starts on packed index bytes
(csrc/dbg_minwin.h).  The records must be what they were: the default build is compared with the generic extraction
("extract_generic", which takes every window minimum through LDS and shares no code with it), with the un-split kernel, with
64-bit stamps and with the C oracle, on inputs of two or three tiles whose minimizers lie across the borders of lanes (32
positions), waves (2 048) and tiles (8 192).  The inputs are checked for that in numpy before anything is built."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _dbg
from oracle import orc_c

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")
TILE = 8192
M = 13
KS = [13, 14, 21, 30, 31]  # W = k - 12 = 1, 2, 9, 18, 19
NO_NODE = np.uint32(0xFFFFFFFF)


# ---- the per-lane arithmetic on the host --------------------------------------------------------------------------------
def test_lane_arithmetic_on_the_host(tmp_path):
    """tests/minwin_host.cpp: includes only dbg_minwin.h, built with the host compiler, run once."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "minwin_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, os.path.join(HERE, "minwin_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout


# ---- inputs -------------------------------------------------------------------------------------------------------------
def random_reads(seed, total, starts_at=(), min_len=31):
    """Uniform ACGT reads of min_len .. 300 bases, `total` bytes in all; a read starts at each position of starts_at.  An entry
    (start, length) of starts_at asks for a read of exactly that length there (any length; its bases are uniform too)."""
    rng = np.random.default_rng(seed)
    fixed = sorted((g, 0) if np.isscalar(g) else (int(g[0]), int(g[1])) for g in starts_at)
    offsets = [0]
    for goal, length in fixed + [(total, 0)]:
        while offsets[-1] < goal:
            gap = goal - offsets[-1]
            if gap <= 300:
                n = gap
            else:
                n = int(rng.integers(min_len, 301))
                if gap - n < min_len:
                    n = gap - min_len
            assert min_len <= n <= 300
            offsets.append(offsets[-1] + n)
        assert offsets[-1] == goal
        if length:
            offsets.append(goal + length)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=total)]
    return np.ascontiguousarray(bases), np.array(offsets, dtype=np.uint64)


def low_complexity_reads(seed, total):
    """Poly-A, period-2 and period-3 reads of 200 .. 400 bases: equal hashes everywhere, so the tie-break decides."""
    rng = np.random.default_rng(seed)
    units = [b"A", b"AC", b"GT", b"ACG", b"TTG", b"C", b"CA", b"GAT"]
    reads, n = [], 0
    while n < total:
        L = min(int(rng.integers(200, 401)), total - n)
        if total - n - L < 200:
            L = total - n
        u = np.frombuffer(units[len(reads) % len(units)], dtype=np.uint8)
        reads.append(np.resize(u, L))
        n += L
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([r.size for r in reads], out=offsets[1:])
    return np.ascontiguousarray(np.concatenate(reads)), offsets


SETS = {
    # name: (maker, arguments); the seeds are the first for which every k passes assert_exercises_the_borders
    "three_tiles": (random_reads, (13, 27_013, (TILE, 2 * TILE + 1))),  # a read starts on a tile border, one a position after one
    "two_tiles_exactly": (random_reads, (11, 2 * TILE)),
    "two_tiles_and_a_byte": (random_reads, (11, 2 * TILE + 1)),
    "not_a_multiple_of_16": (random_reads, (13, 2 * TILE + 1000 + 7)),
    "low_complexity": (low_complexity_reads, (15, 26_000)),
}
_sets = {}


def read_set(name):
    if name not in _sets:
        maker, args = SETS[name]
        bases, offsets = maker(*args)
        bases.setflags(write=False)
        _sets[name] = (bases, offsets)
    return _sets[name]


# ---- the minimizers in numpy ----------------------------------------------------------------------------------------------
def minimizers(bases, offsets, k):
    """valid[p]: a k-mer of a read longer than k starts at p; minpos[p]: start of its leftmost m-mer of minimal hash;
    tie[p]: that minimal hash occurs more than once in the window.  The m-mer hash is mmer_hash16 of csrc/dbg_minwin.h."""
    n, w = bases.size, k - M + 1
    code = ((bases >> 1) & 3).astype(np.uint64)  # A 0, C 1, T 2, G 3; the first base in the highest bits
    n_mm = n - M + 1
    mm = np.zeros(n_mm, dtype=np.uint64)
    for i in range(M):
        mm = (mm << np.uint64(2)) | code[i:i + n_mm]
    mm = mm.astype(np.uint32)
    with np.errstate(over="ignore"):
        h = ((mm ^ (mm >> np.uint32(9)) ^ np.uint32(0x3C6EF372)) * np.uint32(0x9E3779B1)) >> np.uint32(16)
    valid = np.zeros(n, dtype=bool)
    for s, e in zip(offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)):
        if e - s > k:
            valid[s:e - k + 1] = True
    n_k = n - k + 1
    win = np.lib.stride_tricks.sliding_window_view(h, w)[:n_k]
    arg = win.argmin(axis=1)  # the first of equal minima: ties go to the left
    minpos = np.full(n, -1, dtype=np.int64)
    minpos[:n_k] = np.arange(n_k) + arg
    tie = np.zeros(n, dtype=bool)
    tie[:n_k] = (win == win.min(axis=1, keepdims=True)).sum(axis=1) > 1
    return valid, minpos, tie


def n_records_expected(valid, minpos):
    """Super-k-mer records: runs of k-mers that share a minimizer occurrence, cut at tile borders."""
    p = np.arange(valid.size)
    prev_valid = np.concatenate([[False], valid[:-1]])
    prev_min = np.concatenate([[-1], minpos[:-1]])
    return int(np.count_nonzero(valid & ((p % TILE == 0) | ~prev_valid | (prev_min != minpos))))


def assert_exercises_the_borders(name, k):
    """The input takes the new paths: for each border there is a k-mer that starts within W - 1 positions before a multiple of
    it and has its minimizer at or after that multiple (the lane's neighbour, the wave's LDS row, the tile's halo)."""
    bases, offsets = read_set(name)
    w = k - M + 1
    valid, minpos, tie = minimizers(bases, offsets, k)
    p = np.flatnonzero(valid)
    if w > 1:
        for border in (32, 2048, TILE):
            nxt = (p // border + 1) * border  # the next multiple after p
            hit = (nxt - p <= w - 1) & (minpos[p] >= nxt)
            assert hit.any(), (name, k, border)
    if name == "three_tiles":
        starts = set(int(x) for x in offsets[:-1])
        assert any(s and s % TILE == 0 for s in starts) and any(s % TILE == 1 for s in starts)
    if name == "low_complexity" and w > 1:  # equal hashes on both sides of a lane border, inside one window
        nxt = (p // 32 + 1) * 32
        assert (tie[p] & (nxt - p <= w - 1)).any(), (name, k)
    return valid, minpos


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SETS))
def test_inputs_exercise_the_borders(name, k):
    bases, offsets = read_set(name)
    if name == "two_tiles_exactly":
        assert bases.size == 2 * TILE
    if name == "two_tiles_and_a_byte":
        assert bases.size == 2 * TILE + 1
    if name == "not_a_multiple_of_16":
        assert bases.size % 16 != 0
    assert 25_000 <= read_set("three_tiles")[0].size <= 30_000
    assert_exercises_the_borders(name, k)


# ---- builds -------------------------------------------------------------------------------------------------------------
def build(bases, offsets, k, **opts):
    """Nodes in stamp order (keys, keys_hi, stamps, counts, successors as stamps and as rows of that order), sizes() and three
    stats() of a fresh handle's build."""
    g = _dbg.Graph()
    try:
        for name, v in opts.items():
            g.set_option(name, v)
        g.set_reads(bases, offsets)
        g.build(k)
        keys, stamps, counts, _ = g.export_nodes()
        hi = g.export_keys_hi()
        succ = g.export_succ()
        present = succ != NO_NODE
        succ_stamps = np.where(present, stamps[np.where(present, succ, 0)].astype(np.int64), np.int64(-1))
        o = np.argsort(stamps, kind="stable")
        row = np.empty(o.size, dtype=np.int64)
        row[o] = np.arange(o.size)
        succ_rows = np.where(present, row[np.where(present, succ, 0)], np.int64(-1))
        st = g.stats()
        return {"keys": keys[o], "keys_hi": hi[o], "stamps": stamps[o].astype(np.uint64), "counts": counts[o],
                "succ_stamps": succ_stamps[o], "succ": succ_rows[o],
                "sizes": g.sizes(), "stats": {f: st[f] for f in ("n_records", "n_buckets", "n_queries")}}
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SETS))
def test_same_records_and_graph(name, k):
    bases, offsets = read_set(name)
    valid, minpos = assert_exercises_the_borders(name, k)
    got = build(bases, offsets, k)
    print(name, k, got["stats"], "expected records", n_records_expected(valid, minpos))
    for opts in (dict(extract_generic=1), dict(extract_presplit=0), dict(stamp64=1)):
        ref = build(bases, offsets, k, **opts)
        assert got["stats"] == ref["stats"], opts
        assert got["sizes"] == ref["sizes"], opts
        for f in ("keys", "stamps", "counts", "succ_stamps"):
            assert np.array_equal(got[f], ref[f]), (opts, f)
    want = orc_c.build(bases, offsets, k)
    for f in ("n_nodes", "n_kmer_instances", "n_edge_instances"):
        assert got["sizes"][f] == want[f], f
    for f in ("keys", "stamps", "counts"):
        assert np.array_equal(got[f], want[f]), f
    if name != "low_complexity":  # (there a pre-split sub-segment may fill up and the build fall back to another record cut)
        assert got["stats"]["n_records"] == n_records_expected(valid, minpos)
