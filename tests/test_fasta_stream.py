"""Streamed FASTA ingest by chunks and by byte range (dbg_set_reads_fasta_file, ABI 6).

CPU: the ABI surface, and a pure-Python statement of range ownership checked against the reference's read_reads.
GPU (-m gpu): the streamed reads equal dbg_set_reads_fasta on the same bytes at every chunk size (straddle cases at chunk
borders included), ranges split the file exactly, a 1 M-read file gives the same graph, and ranks that ingest their
byte slices give the same sharded graph as one handle ingesting the whole file.
"""
import hashlib
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import dbg_oracle as orc

# tests/test_hip_driver.py::FASTA_CASES
FASTA_CASES = {
    "plain": ">r0\nACGTACGTTG\n>r1\nTTGACCA\n",
    "no_final_newline": ">r0\nACGTACGTTG\n>r1\nTTGACCA",
    "crlf": ">r0\r\nACGTACGTTG\r\n>r1\r\nTTGACCA\r\n",
    "lone_cr": ">r0\rACGTACGTTG\r>r1\rTTGACCA\r",
    "blank_and_multiline": ">r0\nACGT\nACGTTG\n\n>r1\n\nTTGACCA\n\n",
    "trailing_space": ">r0 some text\nACGTACGTTG  \t\n>r1\nTTGACCA \n",
    "gt_inside": "ACG>TT\n>hdr\n >notheader\nAC\n",
    "empty": "",
    "only_headers": ">a\n>b\n",
    "double_cr": "ACGT\r\r\nTTGA\n",
}
# byte 15 / 16 is the border of 16-byte chunks (and of 1-, 2-, 4- and 8-byte ones)
STRADDLE_CASES = {
    "cr_lf_across_border": "ACGTACGTACGTACG\r\nTTTG\r\nAC\r\n",
    "gt_first_in_chunk": "ACGTACGTACGTACG\n>hdr r1\nACCA\n>h\nG\n",
    "long_read": ">r0\n" + "ACGT" * 250 + "\n>r1\nTTGA\n",
    "only_cr": "\r\r\r\r\r\r\r",
    "blank_lines_at_borders": "ACGTACGTACGTACG\n\n\n\n\nACGTACGTAC\n\n\n\n\n\n\nTT\n\n",
    "spaces_across_border": ">h\nACGTACGTACGT    \t   A  \n  \n",
}
ALL_CASES = {**FASTA_CASES, **STRADDLE_CASES}
CHUNKS = (1, 2, 3, 5, 16, 64, 4096, 0)
SPACE = frozenset([32] + list(range(9, 14)) + list(range(28, 32)))  # str.isspace() over ASCII


def line_starts(data):
    """Universal-newline line starts: p == 0, data[p-1] == '\\n', or data[p-1] == '\\r' and data[p] != '\\n'."""
    return [p for p in range(len(data))
            if p == 0 or data[p - 1] == 10 or (data[p - 1] == 13 and data[p] != 10)]


def expected_reads(data, begin=0, end=None):
    """read_reads on the lines that start in [begin, end): not starting with '>', rstrip'ed."""
    end = len(data) if end is None else end
    starts = line_starts(data)
    out = []
    for i, s in enumerate(starts):
        if not begin <= s < end:
            continue
        line = data[s:starts[i + 1] if i + 1 < len(starts) else len(data)]
        if line[:1] == b">":
            continue
        j = len(line)
        while j and line[j - 1] in SPACE:
            j -= 1
        out.append(bytes(line[:j]))
    return out


def write(tmp_path, name, text):
    p = tmp_path / (name + ".fasta")
    p.write_bytes(text.encode() if isinstance(text, str) else text)
    return str(p)


# ---------------------------------------------------------------------------------------------- CPU


def header_text():
    return open(os.path.join(ROOT, "include", "dbg.h")).read()


def test_header_declares_streamed_ingest():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"int\s+dbg_set_reads_fasta_file\s*\(\s*dbg_t\s*\*\s*h\s*,\s*const\s+char\s*\*\s*path\s*,\s*uint64_t\s+begin\s*,"
                     r"\s*uint64_t\s+end\s*,\s*uint64_t\s+chunk_bytes\s*\)", text)
    assert re.search(r"int\s+dbg_fasta_ingest_stats\s*\(\s*dbg_t\s*\*\s*h\s*,\s*dbg_ingest_stats_t\s*\*\s*out\s*\)", text)
    assert "peak_device_bytes" in text


def test_binding_matches_header_version_and_symbols():
    import _dbg
    ver = int(re.search(r"#define\s+DBG_ABI_VERSION\s+(\d+)", header_text()).group(1))
    assert ver == 6 and _dbg.ABI_VERSION == ver
    assert "dbg_set_reads_fasta_file" in _dbg.SYMBOLS and "dbg_fasta_ingest_stats" in _dbg.SYMBOLS
    assert hasattr(_dbg.Graph, "set_reads_fasta_file") and hasattr(_dbg.Graph, "ingest_stats")


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_range_ownership_agrees_with_read_reads(name, tmp_path):
    """Every split point b (inside a line, between '\\r' and '\\n', past the end): the reads of [0, b) then [b, n) are
    the reference's reads of the whole file."""
    p = write(tmp_path, name, ALL_CASES[name])
    data = open(p, "rb").read()
    want = orc.read_reads(p)
    assert [r.decode() for r in expected_reads(data)] == want
    for b in range(len(data) + 2):
        assert [r.decode() for r in expected_reads(data, 0, b) + expected_reads(data, b)] == want, b


# ---------------------------------------------------------------------------------------------- GPU


def one_shot(data):
    import _dbg
    g = _dbg.Graph()
    g.set_reads_fasta(np.frombuffer(data, dtype=np.uint8))
    out = g.copy_reads() + (g.reads_checksum(),)
    g.close()
    return out


def streamed(path, begin=0, end=None, chunk=0, stats=False):
    import _dbg
    g = _dbg.Graph()
    g.set_reads_fasta_file(path, begin, end, chunk)
    out = g.copy_reads() + (g.reads_checksum(),)
    st = g.ingest_stats()
    g.close()
    return out + (st,) if stats else out


def as_list(bases, offsets):
    b = bases.tobytes()
    return [b[int(x):int(y)] for x, y in zip(offsets[:-1], offsets[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_streamed_equals_one_shot_at_every_chunk_size(name, tmp_path):
    p = write(tmp_path, name, ALL_CASES[name])
    data = open(p, "rb").read()
    wb, wo, wsum = one_shot(data)
    want = orc.read_reads(p)
    for chunk in CHUNKS:
        b, o, s, st = streamed(p, chunk=chunk, stats=True)
        assert np.array_equal(o, wo) and np.array_equal(b, wb) and s == wsum, chunk
        assert [r.decode() for r in as_list(b, o)] == want, chunk
        assert st["n_reads"] == len(want) and st["bytes_read"] == len(data)
        if chunk:
            assert st["chunks"] == -(-len(data) // chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_two_ranges_make_the_whole(name, tmp_path):
    p = write(tmp_path, name, ALL_CASES[name])
    data = open(p, "rb").read()
    wb, wo, _ = one_shot(data)
    whole = as_list(wb, wo)
    step = 1 if len(data) < 200 else 7
    for i, b in enumerate(list(range(0, len(data) + 2, step)) + [len(data) - 1]):
        chunk = CHUNKS[i % len(CHUNKS)]
        left = as_list(*streamed(p, 0, b, chunk)[:2])
        right = as_list(*streamed(p, b, None, chunk)[:2])
        assert left == expected_reads(data, 0, b) and left + right == whole, (b, chunk)


@pytest.mark.gpu
def test_seeded_fuzz_of_files_chunks_and_splits(tmp_path):
    rng = random.Random(2024)
    alphabet = b"ACGTN> \t\r\n"
    for it in range(200):
        data = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 400)))
        p = write(tmp_path, f"f{it}", data)
        wb, wo, wsum = one_shot(data)
        whole = as_list(wb, wo)
        assert whole == expected_reads(data)
        b, o, s = streamed(p, chunk=rng.choice([1, 2, 3, 7, 13, 32, 100, 0]))
        assert np.array_equal(o, wo) and np.array_equal(b, wb) and s == wsum, it
        cuts = sorted(rng.randint(0, len(data) + 1) for _ in range(rng.randint(1, 3)))
        bounds = [0] + cuts + [None]
        got = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            part = as_list(*streamed(p, lo, hi, rng.choice([1, 3, 5, 16, 64, 0]))[:2])
            assert part == expected_reads(data, lo, hi), (it, lo, hi)
            got += part
        assert got == whole, (it, cuts)


@pytest.mark.gpu
def test_more_reads_in_the_first_chunk_than_the_first_offsets_hold(tmp_path):
    """The offsets start with 65 536 entries at the most and are sized from the reads seen only from the second chunk on:
    70 000 reads in the first chunk make the ingest grow them and parse the chunk a second time."""
    n = 70_000
    data = b"".join(b">\n" + s + b"\n" for s in (b"ACGT", b"CGTA", b"GTAC", b"TACG")) * (n // 4)
    p = write(tmp_path, "many", data)
    want = orc.read_reads(p)
    assert len(want) == n and want[:5] == ["ACGT", "CGTA", "GTAC", "TACG", "ACGT"]
    wb, wo, wsum = one_shot(data)
    b, o, s, st = streamed(p, stats=True)
    assert np.array_equal(o, wo) and np.array_equal(b, wb) and s == wsum
    assert [r.decode() for r in as_list(b, o)] == want
    assert st["chunks"] == 1 and st["n_reads"] == n and st["bytes_read"] == len(data)


@pytest.mark.gpu
def test_errors_and_empty_ranges(tmp_path):
    import _dbg
    p = write(tmp_path, "small", ">a\nACGT\n>b\nTTGA\n")
    g = _dbg.Graph()
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fasta_file(str(tmp_path / "missing.fasta"))
    assert e.value.code == _dbg.DBG_E_ARG and "missing.fasta" in str(e.value)
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fasta_file(p, 5, 4)
    assert e.value.code == _dbg.DBG_E_ARG and "begin" in str(e.value)
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fasta_file(str(tmp_path))  # a directory
    assert e.value.code == _dbg.DBG_E_ARG
    for begin in (16, 17, 1 << 40):
        g.set_reads_fasta_file(p, begin)
        assert g.sizes()["n_reads"] == 0 and g.sizes()["n_bytes"] == 0
    g.set_reads_fasta_file(p, 3, 3)  # empty range at a line start
    assert g.sizes()["n_reads"] == 0
    g.set_reads_fasta_file(p, 4, 4)  # empty range inside a line
    assert g.sizes()["n_reads"] == 0
    g.set_reads_fasta_file(p, 3, 4)  # one byte: owns the line that starts there
    assert as_list(*g.copy_reads()) == [b"ACGT"]
    g.close()


@pytest.mark.gpu
def test_device_reads_byte_range_and_stream_threshold(tmp_path, monkeypatch):
    import debruijn as prod
    import synth
    reads = synth.reads_list(9, 3000, 400, 80, 0.01)
    p = tmp_path / "reads.fasta"
    synth.write_fasta(str(p), reads)
    size = os.path.getsize(p)
    one = prod.read_reads_device(str(p))
    assert one._graph.ingest_stats()["chunks"] == 1 and list(one) == reads
    monkeypatch.setattr(prod, "STREAM_MIN_BYTES", size)  # at the threshold: streamed
    st = prod.read_reads_device(str(p))
    assert st._graph.ingest_stats()["chunk_bytes"] == 16 << 20 and list(st) == reads
    small = prod.read_reads_device(str(p), chunk_bytes=1000)
    assert small._graph.ingest_stats()["chunks"] == -(-size // 1000) and list(small) == reads
    halves = [prod.DeviceReads(str(p), byte_range=r, chunk_bytes=4096) for r in ((0, size // 2), (size // 2, None))]
    assert list(halves[0]) + list(halves[1]) == reads and 0 < len(halves[0]) < len(reads)


def synth_fasta(path, n, read_len, seed=7):
    import synth
    reads = synth.reads_ascii(seed, n * read_len // 30, n, read_len, 0.01)
    rec = np.empty((n, 3 + read_len + 1), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
    rec[:, 3:3 + read_len] = reads
    rec[:, -1] = 10
    rec.reshape(-1).tofile(path)
    return reads


def graph_digest(g):
    keys, stamps, counts, _ = g.export_nodes(flags=False)
    o = np.argsort(stamps, kind="stable")
    h = hashlib.sha256()
    for a in (keys[o], g.export_keys_hi()[o], stamps[o], counts[o]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_one_million_reads_streamed_in_8mib_chunks(tmp_path):
    import _dbg
    import synth
    n, L, chunk = 1_000_000, 150, 8 << 20
    p = str(tmp_path / "big.fasta")
    reads = synth_fasta(p, n, L)
    size = os.path.getsize(p)
    a = _dbg.Graph()
    a.set_reads_fasta(p)
    b = _dbg.Graph()
    b.set_reads_fasta_file(p, chunk_bytes=chunk)
    st = b.ingest_stats()
    assert b.sizes()["n_reads"] == n and b.reads_checksum() == a.reads_checksum() == synth.checksum(reads)
    assert st["chunks"] == -(-size // chunk) and st["bytes_read"] == size and st["n_bases"] == n * L
    bound = size + 64 + 12 * (n + 1) + 4 * chunk + (1 << 20)
    assert 0 < st["peak_device_bytes"] <= bound, (st, bound)
    for g in (a, b):
        g.build(31)
    assert a.sizes()["n_nodes"] == b.sizes()["n_nodes"] > 0
    assert graph_digest(a) == graph_digest(b)
    a.close()
    b.close()


def shard_nodes(g):
    keys, stamps, counts, _ = g.export_nodes(flags=False)
    return keys, g.export_keys_hi(), stamps, counts


def node_set(keys, hi, stamps, counts):
    o = np.lexsort((hi, keys))
    return keys[o], hi[o], stamps[o], counts[o]


@pytest.mark.gpu
@pytest.mark.parametrize("world,k", [(2, 31), (4, 31), (2, 63), (4, 63)])
def test_ranks_ingest_their_slices_for_the_sharded_build(world, k, tmp_path):
    import _dbg
    import debruijn as prod
    import inproc_dist
    import multi_gpu
    import synth
    p = str(tmp_path / "reads.fasta")
    synth.write_fasta(p, synth.reads_list(77, 60000, 8000, 150, 0.01))

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        multi_gpu.set_reads_fasta_shard(g, p, dist, chunk_bytes=1 << 16)
        multi_gpu.sharded_build(g, k, dist)
        out = shard_nodes(g)
        g.close()
        return out

    shards = inproc_dist.run_ranks(world, one)
    got = node_set(*(np.concatenate([s[i] for s in shards]) for i in range(4)))
    dev = prod.read_reads_device(p)
    g = dev._graph
    g.build(k)
    want = node_set(*shard_nodes(g))
    assert got[0].size == want[0].size == g.sizes()["n_nodes"]
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
