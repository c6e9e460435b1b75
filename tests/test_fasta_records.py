"""Record-mode FASTA ingest (dbg_set_reads_fasta_records[_file], csrc/dbg_fasta.h) and line-wrapped contig output
(dbg_write_contigs_fasta_wrapped, csrc/dbg_ctgout.h) on the device, against the plain-Python statement of both rules
(debruijn.parse_fasta_records, debruijn.wrap_fasta_record): the hand-written files of tests/test_fasta_records_host.py through
the one-image and the streamed call, line ends and headers moved over the chunk, word and block borders, byte ranges cut at
every byte of a stretch, composition with the split and both strands, the graph of a wrapped file against the oracle on the
host-parsed records, sharded ingest, wrapped output against the host rule byte for byte, the round trip, and the driver."""
import contextlib
import functools
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
from test_fasta_records_host import FILES, MALFORMED

pytestmark = pytest.mark.gpu


def unpack(bases, off):
    raw = bases.tobytes()
    return [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def pack(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


@pytest.fixture(scope="module")
def g():
    h = _dbg.Graph()
    yield h
    h.close()


@functools.lru_cache(maxsize=8)
def header_starts(data):
    """positions of the header line starts of the file, by the rule of include/dbg.h"""
    return [p for p in range(len(data)) if data[p:p + 1] == b">" and
            (p == 0 or data[p - 1:p] == b"\n" or data[p - 1:p] == b"\r")]  # after '\r' a '>' is no '\n'


def host_stats(data, begin=0, end=None):
    """what dbg_fasta_records_stats must say about the range, from the host parser and the rule"""
    end = len(data) if end is None else min(end, len(data))
    heads = header_starts(data)
    stop = min([p for p in heads if p >= end], default=len(data))
    first = min([p for p in heads if p >= begin], default=len(data))  # begin <= end: never past stop
    owned = data[first:stop]
    reads = prod.parse_fasta_records(owned)
    return {"n_records": len(reads), "n_sequence_lines": sum(not ln.startswith(b">") for ln in owned.splitlines()),
            "longest_record": max((len(r) for r in reads), default=0), "first_byte": first, "end_byte": stop}


def check_stats(h, data, begin=0, end=None):
    st, want = h.fasta_records_stats(), host_stats(data, begin, end)
    for f in want:
        assert st[f] == want[f], (f, st, want)
    ing = h.ingest_stats()
    assert ing["n_reads"] == want["n_records"] and ing["bytes_read"] == st["scan_bytes"] + want["end_byte"] - want["first_byte"]


def ingest(h, path, data, how):
    """how: None = the one-image call on the bytes, "path" = the one-image call on the path, int = streamed at that chunk size"""
    if how is None:
        h.set_reads_fasta_records(data)
    elif how == "path":
        h.set_reads_fasta_records(path)
    else:
        h.set_reads_fasta_records_file(path, chunk_bytes=how)
    return unpack(*h.copy_reads())


# ---- 1. hand-written files ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FILES))
def test_hand_written_files_equal_the_host_parser(name, g, tmp_path):
    data, want = FILES[name]
    assert prod.parse_fasta_records(data) == want
    p = str(tmp_path / "f.fasta")
    with open(p, "wb") as fh:
        fh.write(data)
    for how in (None, "path", 64, 4096, 1):
        assert ingest(g, p, data, how) == want, (name, how)
        check_stats(g, data)
        assert g.sizes()["n_reads"] == len(want)


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_sequence_before_the_first_header_fails_with_its_position_and_the_handle_stays_usable(name, g, tmp_path):
    data, _, pos = MALFORMED[name]
    p = str(tmp_path / "bad.fasta")
    with open(p, "wb") as fh:
        fh.write(data)
    good, want = FILES["lf"]
    for how in (None, 64, 4096):
        g.set_reads_fasta_records(good)
        with pytest.raises(_dbg.DbgError) as e:
            ingest(g, p, data, how)
        assert e.value.code == _dbg.DBG_E_ARG
        assert "sequence before the first header" in str(e.value) and str(e.value).endswith(f"at byte {pos}")
        assert g.sizes()["n_reads"] == 0  # left without reads
        assert ingest(g, p, good, None) == want
    # only the range with begin == 0 reports it; a later range takes what it owns
    heads = header_starts(data)
    if heads:
        g.set_reads_fasta_records_file(p, 1, None, 64)
        assert unpack(*g.copy_reads()) == prod.parse_fasta_records(data[heads[0]:])
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fasta_records_file(p, 0, 1, 64)  # even where the range owns no header
    assert e.value.code == _dbg.DBG_E_ARG
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fasta_records_file(str(tmp_path / "missing.fasta"))
    assert e.value.code == _dbg.DBG_E_ARG
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fasta_records_file(p, 5, 4)
    assert e.value.code == _dbg.DBG_E_ARG and "begin" in str(e.value)


def test_more_records_in_the_first_chunk_than_the_first_offsets_hold(g, tmp_path):
    """The offsets start with 65 536 entries at the most and are sized from the records seen only from the second chunk on:
    70 000 records in the first chunk make the ingest grow them and parse the chunk a second time."""
    n = 70_000
    data = b"".join(b">\n" + s + b"\n" for s in (b"ACGT", b"CGTA", b"GTAC", b"TACG")) * (n // 4)
    p = str(tmp_path / "many.fasta")
    with open(p, "wb") as fh:
        fh.write(data)
    want = prod.parse_fasta_records(data)
    assert len(want) == n and want[:5] == [b"ACGT", b"CGTA", b"GTAC", b"TACG", b"ACGT"]
    for how in (0, None):  # streamed from the file at the default chunk size, and the one-image call
        assert ingest(g, p, data, how) == want, how
        check_stats(g, data)
        st = g.ingest_stats()
        assert st["chunks"] == 1 and st["n_reads"] == n


# ---- 2. chunk, word and block borders -------------------------------------------------------------------------------------
def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def wrap(seq, width, nl=b"\n"):
    return b"".join(seq[i:i + width] + nl for i in range(0, len(seq), width))


def test_line_ends_and_headers_move_over_chunk_and_word_borders(g, tmp_path):
    rng = np.random.default_rng(19)
    long_rec = bases(rng, 10000)
    tail = b">s1\nACGT\n>s2\n\n>s3\r\nAC \r\nGT\r>s4\n" + wrap(bases(rng, 150), 60) + b">s5"
    p = str(tmp_path / "pad.fasta")
    for pad in range(71):
        data = b">" + b"h" * pad + b"\n" + b"TTGA\n>long some text\n" + wrap(long_rec, 60) + tail
        want = prod.parse_fasta_records(data)
        assert want[1] == long_rec and len(want) == 7
        with open(p, "wb") as fh:
            fh.write(data)
        for how in (64, 4096) + ((None,) if pad % 8 == 0 else ()):
            assert ingest(g, p, data, how) == want, (pad, how)
        check_stats(g, data)
        assert g.fasta_records_stats()["longest_record"] == 10000


@pytest.mark.parametrize("what", ["header", "line_end"])
def test_headers_and_line_ends_on_the_64k_block_border(what, g, tmp_path):
    rng = np.random.default_rng(23)
    block = _dbg_block_bytes()
    p = str(tmp_path / "block.fasta")
    for d in range(-2, 3):
        for nl in (b"\n", b"\r\n", b"\r"):
            # a first record whose last line end closes at block + d: the next byte starts a header, or a sequence line
            head = b">first\n"
            room = block + d - len(head)
            body = wrap(bases(rng, room), 60, nl)[:room - len(nl)]
            body = body[:-1] + b"A" if body[-1:] in (b"\n", b"\r") else body
            first = head + body + nl
            assert len(first) == block + d
            nxt = (b">on the border\n" if what == "header" else b"") + wrap(bases(rng, 75000), 70, nl) + b">last\nAC\n"
            data = first + nxt
            assert 135 * 1024 < len(data) < 150 * 1024
            want = prod.parse_fasta_records(data)
            assert len(want) == (3 if what == "header" else 2)
            with open(p, "wb") as fh:
                fh.write(data)
            for how in ((None, 1 << 17) if nl == b"\n" else (None,)):
                assert ingest(g, p, data, how) == want, (what, d, nl, how)
            check_stats(g, data)


def _dbg_block_bytes():
    import re
    src = open(os.path.join(PKG, "csrc", "dbg_fasta.h")).read()
    wpt = int(re.search(r"constexpr int FS_WPT = (\d+);", src).group(1))
    assert re.search(r"constexpr int FS_WPB = 256 \* FS_WPT;", src)
    assert 256 * wpt * 32 == 65536  # the block border the test aims at
    return 256 * wpt * 32


# ---- 3. ranges ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranged(tmp_path_factory):
    rng = np.random.default_rng(29)
    parts = []
    for i in range(200):
        nl = (b"\n", b"\r\n", b"\r")[i % 3]
        parts.append(b">rec%d x>y" % i + nl + wrap(bases(rng, int(rng.integers(0, 200))), 60, nl) + (nl if i % 7 == 0 else b""))
    data = b"".join(parts)
    p = str(tmp_path_factory.mktemp("ranges") / "ranged.fasta")
    with open(p, "wb") as fh:
        fh.write(data)
    return p, data, prod.parse_fasta_records(data)


def range_reads(h, p, begin, end):
    h.set_reads_fasta_records_file(p, begin, end, 4096)
    return unpack(*h.copy_reads())


def test_every_cut_of_a_stretch_gives_the_whole_file(ranged, g):
    p, data, whole = ranged
    assert len(whole) == 200 and range_reads(g, p, 0, None) == whole
    lo = data.index(b">rec30 ") - 5
    stretch = data[lo:lo + 300]
    assert stretch.count(b">rec") >= 2 and b"x>y" in stretch and b"\r\n" in stretch and b"\n>" in stretch and b"\r>" in stretch
    for b in range(lo, lo + 300):
        left = range_reads(g, p, 0, b)
        check_stats(g, data, 0, b)
        right = range_reads(g, p, b, None)
        check_stats(g, data, b, None)
        assert left + right == whole, b
        assert len(right) == sum(h >= b for h in header_starts(data))


def test_three_way_cuts_ranges_without_a_header_and_the_ends(ranged, g):
    p, data, whole = ranged
    size = len(data)
    heads = header_starts(data)
    rng = np.random.default_rng(31)
    cuts = [(size // 3, 2 * size // 3), (heads[50], heads[51]), (heads[50] + 1, heads[51] + 1), (heads[50] - 1, heads[50])]
    cuts += [tuple(sorted(int(x) for x in rng.integers(0, size + 1, 2))) for _ in range(8)]
    for a, b in cuts:
        got = range_reads(g, p, 0, a) + range_reads(g, p, a, b) + range_reads(g, p, b, 1 << 62)
        assert got == whole, (a, b)
    # a range inside one record owns nothing
    a = heads[100] + 1
    assert heads[101] - a > 2
    assert range_reads(g, p, a, heads[101]) == [] and g.sizes()["n_reads"] == 0
    st = g.fasta_records_stats()
    assert st["n_records"] == 0 and st["first_byte"] == st["end_byte"] == heads[101]
    assert range_reads(g, p, a, a) == [] and range_reads(g, p, size, None) == [] and range_reads(g, p, size + 9, None) == []
    assert range_reads(g, p, 0, 0) == []
    assert range_reads(g, p, heads[100], heads[100] + 1) == [whole[100]]
    assert range_reads(g, p, heads[199], None) == [whole[199]]


# ---- 4. composition -------------------------------------------------------------------------------------------------------
def test_record_mode_composes_with_the_split_and_both_strands(tmp_path):
    rng = np.random.default_rng(37)
    p = str(tmp_path / "mixed.fasta")
    with open(p, "wb") as fh:
        for i in range(120):
            seq = bytearray(bases(rng, int(rng.integers(0, 400))))
            for j in rng.integers(0, max(len(seq), 1), 3):
                if len(seq):
                    seq[j] = b"NnacgtR"[int(rng.integers(0, 7))]
            fh.write(b">r%d\n" % i + wrap(bytes(seq), 60))
    records = prod.read_fasta_records(p)
    want = prod.both_strands(prod.acgt_pieces(records, fold_case=True))
    assert any("N" in r for r in records) and any("a" in r for r in records)
    for kw in ({}, {"chunk_bytes": 64}, {"byte_range": (0, None)}):
        dev = prod.read_reads_device(p, non_acgt="split", fold_case=True, strands="both", records="record", **kw)
        assert list(dev) == want and len(dev) == len(want)
        assert dev.records_stats["n_records"] == len(records) == dev.split_stats["n_reads_in"]
        rd, pos = dev.origins()
        folded = [r.translate(str.maketrans("acgt", "ACGT")) for r in records]
        for j, piece in enumerate(want):  # the record, and the position in its JOINED read
            fwd = prod.revcomp(piece) if j & 1 else piece
            assert folded[int(rd[j])][int(pos[j]):int(pos[j]) + len(fwd)] == fwd
    assert list(prod.DeviceReads(p, records="record")) == records
    assert prod.DeviceReads(p).records_stats is None and list(prod.DeviceReads(p)) == prod.read_reads(p)  # the default: unchanged


# ---- 5. the graph ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapped_reads(tmp_path_factory):
    rng = np.random.default_rng(41)
    genome = bases(rng, 5000)
    reads = []
    for _ in range(300):
        s = int(rng.integers(0, 5000 - 150))
        reads.append(genome[s:s + 150].decode())
    d = tmp_path_factory.mktemp("graph")
    flat, wrapped = str(d / "flat.fasta"), str(d / "wrapped.fasta")
    with open(flat, "wb") as fh:
        fh.write(b"".join(b">r%d\n" % i + r.encode() + b"\n" for i, r in enumerate(reads)))
    with open(wrapped, "wb") as fh:
        fh.write(b"".join(b">r%d\n" % i + wrap(r.encode(), 60) for i, r in enumerate(reads)))
    return reads, flat, wrapped


def graph_of(reads, k, mod):
    with contextlib.redirect_stdout(io.StringIO()):
        g_, pull, branch, pulled, ect = mod.construct_graph(reads, k, threshold=2)
        contigs = mod.output_contigs(g_, branch, pulled)
        return canonical(g_, pull, branch, pulled, ect, contigs)


@pytest.mark.parametrize("k", [31, 63])
def test_graph_of_a_wrapped_file_is_the_oracle_on_its_records(k, wrapped_reads):
    from oracle import dbg_oracle as orc
    reads, flat, wrapped = wrapped_reads
    assert prod.read_fasta_records(wrapped) == reads == prod.read_reads(flat)
    want = graph_of(list(prod.read_fasta_records(wrapped)), k, orc)
    got = graph_of(prod.DeviceReads(wrapped, records="record"), k, prod)
    unwrapped = graph_of(prod.DeviceReads(flat), k, prod)
    assert len(want["vertices"]) > 1000 and len(want["contigs"]) > 0
    for field in want:
        assert got[field] == want[field], field
        assert unwrapped[field] == want[field], field
    if k == 31:  # line mode cuts every read into 60 + 60 + 30: 60 k-mers a read, not 120
        lines = prod.DeviceReads(wrapped)
        assert len(lines) == 3 * len(reads)
        lines._graph.build(k)
        rec = prod.DeviceReads(wrapped, records="record")
        rec._graph.build(k)
        assert lines._graph.sizes()["n_nodes"] < rec._graph.sizes()["n_nodes"]
    else:  # and at a k above the line width it finds nothing at all
        assert all(len(r) < k for r in prod.DeviceReads(wrapped))


def test_one_long_record_builds_the_node_table_of_its_sequence(g, tmp_path):
    rng = np.random.default_rng(43)
    seq = bases(rng, 150000)
    p = str(tmp_path / "genome.fasta")
    with open(p, "wb") as fh:
        fh.write(b">chr1 one record\n" + wrap(seq, 70))

    def nodes(h):
        h.build(31)
        keys, stamps, counts, _ = h.export_nodes(flags=False)
        o = np.argsort(keys, kind="stable")
        return keys[o], stamps[o], counts[o]

    g.set_reads(*pack([seq]))
    want = nodes(g)
    for how in ("path", 1 << 16):
        assert ingest(g, p, None, how) == [seq]
        st = g.fasta_records_stats()
        assert (st["n_records"], st["n_sequence_lines"], st["longest_record"]) == (1, -(-150000 // 70), 150000)
        got = nodes(g)
        assert got[0].size == want[0].size > 100000
        for x, y in zip(got, want):
            assert np.array_equal(x, y)


# ---- 6. sharded ingest ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_take_the_records_whose_header_starts_in_their_slice(world, ranged):
    import inproc_dist
    import multi_gpu
    p, data, whole = ranged

    def one(dist, rank):
        h = _dbg.Graph(device=0)
        multi_gpu.set_reads_fasta_shard(h, p, dist, chunk_bytes=1 << 12, records="record")
        mine, st = unpack(*h.copy_reads()), h.fasta_records_stats()
        h.close()
        return mine, st

    shards = inproc_dist.run_ranks(world, one)
    assert [r for mine, _ in shards for r in mine] == whole  # rank order is file order
    assert all(len(mine) > 0 for mine, _ in shards)
    for r in range(world - 1):
        assert shards[r][1]["end_byte"] == shards[r + 1][1]["first_byte"]
    assert shards[0][1]["first_byte"] == 0 and shards[-1][1]["end_byte"] == len(data)


# ---- 7. wrapped output, 8. round trip -------------------------------------------------------------------------------------
def host_fasta(texts, first, k, width):
    return "".join(f">SEQUENCE_{first + i}_{k}mer\n" + prod.wrap_fasta_record(t, width) for i, t in enumerate(texts)).encode("latin-1")


# a final-mode walk keeps no index without its text (dbg_walk: sizes only), so the index-only walk is the non-final one:
# both text sources of the kernel, CoCharsSrc and CoLiftSrc, and both walks are covered
@pytest.mark.parametrize("final,materialised", [(False, True), (False, False), (True, True)])
def test_wrapped_output_equals_the_host_rule_and_reads_back(final, materialised, wrapped_reads, tmp_path, monkeypatch):
    reads, flat, _ = wrapped_reads
    monkeypatch.setattr(prod, "MAX_CONTIG_CHARS", 0 if materialised else 16)
    k = 31
    dev = prod.DeviceReads(flat)
    dev._graph.set_option("walk_jump_min_nodes", 0)  # a graph this small keeps its index without the text only when asked
    with contextlib.redirect_stdout(io.StringIO()):
        g_, pull, branch, pulled, ect = prod.construct_graph(dev, k, threshold=2, final=final)
        contigs = prod.output_contigs(g_, branch, pulled)
    lazy = isinstance(contigs, prod.LazyContigs)
    assert lazy == (not materialised)
    graph = contigs._graph
    index = np.asarray(contigs._order if lazy else contigs._index, dtype=np.uint64)
    texts = list(contigs)
    assert len(texts) > 0 and sum(len(t) for t in texts) > 4096 and max(len(t) for t in texts) > 122
    rng = np.random.default_rng(47)
    lists = {"in order": np.arange(len(texts)), "repeats": rng.integers(0, len(texts), 2 * len(texts) + 3), "none": np.arange(0)}
    path = str(tmp_path / "out.fasta")
    for name, pos in lists.items():
        chosen = [texts[i] for i in pos.tolist()]
        n0 = graph.write_contigs_fasta(path, index[pos], append=False, first_number=8, k_label=k, chunk_bytes=4096)
        with open(path, "rb") as fh:
            plain = fh.read()
        assert plain == host_fasta(chosen, 8, k, 0) and n0 == len(plain)
        for width in (0, 1, 60, 61):
            n = graph.write_contigs_fasta(path, index[pos], append=False, first_number=8, k_label=k, chunk_bytes=4096,
                                          line_width=width)
            with open(path, "rb") as fh:
                got = fh.read()
            assert got == host_fasta(chosen, 8, k, width), (name, width)
            assert n == len(got) and (width or got == plain)
            if width and name != "none":  # 8. the round trip: the wrapped file read back in record mode
                back = prod.DeviceReads(path, records="record")
                assert list(back) == chosen, (name, width)
    # the whole list in the driver's order, through the list objects
    order = sorted(range(len(texts)), key=lambda i: contigs.scores[i], reverse=True)
    if lazy:
        contigs.sort(reverse=True)
        contigs.extend(["ACGT" * 40, ""])
        contigs.write_fasta(path, k, append=False, line_width=60)
        want = [texts[i] for i in order] + ["ACGT" * 40, ""]
    else:
        contigs.write_fasta(path, k, order, append=False, line_width=60)
        want = [texts[i] for i in order]
    with open(path, "rb") as fh:
        assert fh.read() == host_fasta(want, 0, k, 60)
    assert prod.read_fasta_records(path) == want


# ---- 9. the driver --------------------------------------------------------------------------------------------------------
def run_driver(tmp_path, froot, **keys):
    with open(tmp_path / froot / "setting.json") as fh:
        setting = json.load(fh)
    setting.update(keys)
    with open(tmp_path / froot / "setting.json", "w") as fh:
        json.dump(setting, fh)
    subprocess.check_call([sys.executable, os.path.join(PKG, "II_assembleFromReads.py"), "-froot", froot],
                          cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=PKG), stdout=subprocess.DEVNULL)
    return (tmp_path / froot / f"{froot}.fasta").read_bytes()


@pytest.fixture(scope="module")
def driver_case():
    from oracle import dbg_oracle as orc
    reads = synth.reads_list(41, 3000, 400, 80, 0.005)
    with contextlib.redirect_stdout(io.StringIO()):
        want, _ = orc.assemble(reads, 15, 17, 2)
    assert len(want) > 0 and max(len(c) for c in want) > 60
    return reads, want


def test_driver_reads_records_and_writes_wrapped_contigs(driver_case, tmp_path):
    reads, want = driver_case
    froot = "wrapped"
    synth.write_froot(str(tmp_path / froot), reads, 15, 17, threshold=2)
    with open(tmp_path / froot / "input_reads.fasta", "wb") as fh:
        fh.write(b"".join(b">input_read%d\n" % i + wrap(r.encode(), 60) for i, r in enumerate(reads)))
    out = run_driver(tmp_path, froot, fasta_records="record", fasta_line_width=60)
    assert out == host_fasta(want, 0, 17, 60)
    assert [r.decode() for r in prod.parse_fasta_records(out)] == want


def test_driver_without_the_keys_writes_the_bytes_it_always_wrote(driver_case, tmp_path):
    reads, want = driver_case
    froot = "plain"
    synth.write_froot(str(tmp_path / froot), reads, 15, 17, threshold=2)
    out = run_driver(tmp_path, froot)
    assert out == "".join(">SEQUENCE_{}_{}mer\n{}\n".format(i, 17, c) for i, c in enumerate(want)).encode()
