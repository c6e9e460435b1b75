"""Streamed FASTQ ingest with a quality mask (dbg_set_reads_fastq_file; the rules are in include/dbg.h and DESIGN.md 4i).

CPU: the ABI surface; ``read_fastq`` against hand-written lists; a Python restatement of record ownership by byte range
checked against it at every split point; every kind of malformed file.
GPU (-m gpu): the streamed reads equal ``read_fastq`` at every chunk size, across 64 KiB blocks and scan tiles, by ranges,
on seeded random files; malformed files fail with record and kind and leave the handle usable; the mask, alone and
feeding the split; the Python surface; the device-memory bound of DESIGN.md 4i.
"""
import hashlib
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import dbg_oracle as orc

LONG = "ACGT" * 250
PLAIN = "@r0\nACGTACGTTG\n+\nIIIIIIIIII\n@r1\nTTGACCA\n+\nIIIIIII\n"
# name -> (file text, the reads by hand)
CASES = {
    "plain": (PLAIN, ["ACGTACGTTG", "TTGACCA"]),
    "no_final_newline": (PLAIN[:-1], ["ACGTACGTTG", "TTGACCA"]),
    "crlf": (PLAIN.replace("\n", "\r\n"), ["ACGTACGTTG", "TTGACCA"]),
    "lone_cr": (PLAIN.replace("\n", "\r"), ["ACGTACGTTG", "TTGACCA"]),
    # '\r' is byte 15 and '\n' byte 16: the border of 16-byte chunks (and of 1-, 2-, 4- and 8-byte ones)
    "crlf_across_border": ("@r0\nACGTACGTACG\r\n+\r\nIIIIIIIIIII\r\n@r1\r\nTT\r\n+\r\nII\r\n", ["ACGTACGTACG", "TT"]),
    "trailing_blank_lines": (PLAIN + "\n\n  \n\r\n", ["ACGTACGTTG", "TTGACCA"]),
    "quality_starts_with_at_and_plus": ("@r0\nACGT\n+\n@III\n@r1\nTTGA\n+\n+@+@\n@r2\nAC\n+\n@+\n@r3\nG\n+\n@\n",
                                        ["ACGT", "TTGA", "AC", "G"]),
    "header_with_at_and_plus": ("@r0 @x +y\nACGT\n+\nIIII\n@+\nTT\n+\nII\n@@\nG\n+\n+\n", ["ACGT", "TT", "G"]),
    "plus_name_separators": ("@r0\nACGT\n+r0\nIIII\n@r1\nTT\n+r1 x +\nII\n", ["ACGT", "TT"]),
    "empty_read_in_the_middle": ("@a\nAC\n+\nII\n@b\n\n+\n\n@c\nGT\n+\n@I\n", ["AC", "", "GT"]),
    "empty_read_last_with_quality_line": ("@a\nAC\n+\nII\n@b\n\n+\n\n", ["AC", ""]),
    "empty_read_last_without_quality_line": ("@a\nAC\n+\nII\n@b\n\n+\n", ["AC", ""]),
    "empty_read_last_bare_separator": ("@a\nAC\n+\nII\n@b\r\n\r\n+", ["AC", ""]),
    "trailing_spaces": ("@r0 x \nACGT  \t\n+ \nIIII \t \n@r1\nTT \n+\nII  \n", ["ACGT", "TT"]),
    "inner_spaces_stay": ("@r0\nAC GT \n+\nII II\n", ["AC GT"]),
    # sequence and quality lie in different chunks at 16 and 64, and the pending white space crosses chunks
    "long_read": ("@r0\n" + LONG + "  \t \n+\n" + "I" * 1000 + "   \n@r1\nTTGA\n+\nIIII\n", [LONG, "TTGA"]),
    "lower_case_and_n": ("@r0\nacgtNNacgt\n+\nIIIIIIIIII\n@r1\nNNNN\n+\n!!!!\n", ["acgtNNacgt", "NNNN"]),
    "only_empty_reads": ("@a\n\n+\n\n@b\n\n+\n\n", ["", ""]),
    "only_white_space": (" \n\n\t\n", []),
    "empty": ("", []),
}
CHUNKS = (1, 2, 3, 5, 16, 64, 4096, 0)
SPACE = bytes([32] + list(range(9, 14)) + list(range(28, 32)))  # str.isspace() over ASCII

# name -> (file text, record, kind, min_quality)
MALFORMED = {
    "header_first_record": ("Xa\nAC\n+\nII\n@b\nGT\n+\nII\n", 0, "header", 0),
    "header": ("@a\nAC\n+\nII\nXb\nGT\n+\nII\n", 1, "header", 0),
    "header_is_fasta": (">a\nAC\n>b\nGT\n", 0, "header", 0),
    "separator_first_record": ("@a\nAC\n-\nII\n", 0, "separator", 0),
    "separator": ("@a\nAC\n+\nII\n@b\nGT\n-\nII\n@c\nA\n+\nI\n", 1, "separator", 0),
    "sequence_start_at": ("@a\nAC\n+\nII\n@b\n@T\n+\nII\n", 1, "sequence start", 0),
    "sequence_start_plus_first_record": ("@a\n+C\n+\nII\n", 0, "sequence start", 0),
    "multi_line_sequence": ("@a\nAC\nGT\n+\nIIII\n", 0, "separator", 0),
    "length_mismatch": ("@a\nAC\n+\nII\n@b\nGTT\n+\nII\n@c\nA\n+\nI\n", 1, "length mismatch", 0),
    "length_mismatch_first_record": ("@a\nAC\n+\nIII\n@b\nGTT\n+\nIII\n", 0, "length mismatch", 0),
    "length_mismatch_last_record": ("@a\nAC\n+\nII\n@b\nGTT\n+\nII\n", 1, "length mismatch", 0),
    "later_records_make_up_the_length": ("@a\nACG\n+\nII\n@b\nGT\n+\nIII\n", 0, "length mismatch", 0),
    "no_quality_line_for_a_read": ("@a\nAC\n+\nII\n@b\nGT\n+\n", 1, "length mismatch", 0),
    "truncated_after_sequence": ("@a\nAC\n+\nII\n@b\nGT\n", 1, "truncated record", 0),
    "truncated_after_header": ("@a\nAC\n+\nII\n@b\n", 1, "truncated record", 0),
    "truncated_first_record": ("@a\nAC", 0, "truncated record", 0),
    "first_of_two_violations": ("@a\nAC\n+\nII\nXb\nGT\n+\nII\n@c\nA\n-\nI\n", 1, "header", 0),
    "quality_byte_127": ("@a\nAC\n+\nII\n@b\nGT\n+\nI\x7f\n", 1, "quality byte", 1),
    "quality_byte_32": ("@a\nACG\n+\nI I\n@b\nGT\n+\nII\n", 0, "quality byte", 20),
    "length_before_quality_byte": ("@a\nACG\n+\nI I\n@b\nGT\n+\nI\n", 1, "length mismatch", 20),
}


def line_starts(data):
    """Universal-newline line starts: p == 0, data[p-1] == '\\n', or data[p-1] == '\\r' and data[p] != '\\n'."""
    return [p for p in range(len(data))
            if p == 0 or data[p - 1] == 10 or (data[p - 1] == 13 and data[p] != 10)]


def record_start(data, pos):
    """The ownership rule: the record start at or after pos is the first line start p >= pos with data[p] == '@' whose
    second-next line begins with '+' (0 for pos 0; the end of the file without its trailing white space if none)."""
    size = len(data.rstrip(SPACE))
    if pos == 0 or pos >= size:
        return min(pos, size)
    starts = line_starts(data[:size])
    for i, p in enumerate(starts):
        if p >= pos and data[p] == 64 and i + 2 < len(starts) and data[starts[i + 2]] == 43:
            return p
    return size


def expected_reads(data, begin=0, end=None, min_quality=0):
    """The reads of the records whose header starts in [begin, end), by the host parser."""
    import debruijn as prod
    end = len(data) if end is None else end
    return prod.parse_fastq(data[record_start(data, begin):record_start(data, end)], min_quality)


def write(tmp_path, name, text):
    p = tmp_path / (name + ".fastq")
    p.write_bytes(text.encode("latin-1") if isinstance(text, str) else text)
    return str(p)


# ---------------------------------------------------------------------------------------------- CPU


def header_text():
    return open(os.path.join(ROOT, "include", "dbg.h")).read()


def test_header_declares_fastq_ingest():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    assert re.search(r"int\s+dbg_set_reads_fastq_file\s*\(\s*dbg_t\s*\*\s*h\s*,\s*const\s+char\s*\*\s*path\s*,\s*uint64_t\s+begin\s*,"
                     r"\s*uint64_t\s+end\s*,\s*uint64_t\s+chunk_bytes\s*,\s*uint32_t\s+min_quality\s*\)", text)
    assert re.search(r"int\s+dbg_fastq_ingest_stats\s*\(\s*dbg_t\s*\*\s*h\s*,\s*dbg_fastq_stats_t\s*\*\s*out\s*\)", text)
    for field in ("n_records", "masked_bases", "quality_bytes_held", "peak_device_bytes"):
        assert re.search(r"uint64_t\s+%s\s*;" % field, text), field


def test_binding_lists_the_symbols_and_abi_stays_6():
    import _dbg
    ver = int(re.search(r"#define\s+DBG_ABI_VERSION\s+(\d+)", header_text()).group(1))
    assert ver == 6 and _dbg.ABI_VERSION == ver
    assert "dbg_set_reads_fastq_file" in _dbg.SYMBOLS and "dbg_fastq_ingest_stats" in _dbg.SYMBOLS
    assert hasattr(_dbg.Graph, "set_reads_fastq_file") and hasattr(_dbg.Graph, "fastq_stats")


@pytest.mark.parametrize("name", sorted(CASES))
def test_read_fastq_gives_the_hand_written_reads(name, tmp_path):
    import debruijn as prod
    text, want = CASES[name]
    assert prod.read_fastq(write(tmp_path, name, text)) == want


@pytest.mark.parametrize("name", sorted(CASES))
def test_range_ownership_splits_every_case_at_every_byte(name, tmp_path):
    """Every split point b (inside a line, between '\\r' and '\\n', past the end): the reads of [0, b) then [b, n) are
    the reads of the whole file."""
    text, want = CASES[name]
    data = text.encode()
    want = [r.encode() for r in want]
    assert expected_reads(data) == want
    for b in range(len(data) + 2):
        assert expected_reads(data, 0, b) + expected_reads(data, b) == want, b


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_read_fastq_names_record_and_kind_of_a_malformed_file(name, tmp_path):
    import debruijn as prod
    text, record, kind, q = MALFORMED[name]
    p = write(tmp_path, name, text)
    with pytest.raises(ValueError) as e:
        prod.read_fastq(p, min_quality=q)
    assert (e.value.record, e.value.kind) == (record, kind) and f"record {record}: {kind}" in str(e.value)
    if kind == "quality byte":
        assert prod.read_fastq(p)  # with the mask off no quality byte is looked at


def test_read_fastq_masks_by_phred_33(tmp_path):
    import debruijn as prod
    p = write(tmp_path, "mask", "@a\nACGTN\n+\n!\"5I~\n")  # Phred 0, 1, 20, 40, 93
    assert [prod.read_fastq(p, q)[0] for q in (0, 1, 2, 20, 21, 41, 93)] == \
        ["ACGTN", "NCGTN", "NNGTN", "NNGTN", "NNNTN", "NNNNN", "NNNNN"]
    with pytest.raises(ValueError):
        prod.read_fastq(p, 94)


def test_write_fastq_round_trips(tmp_path):
    import debruijn as prod
    import synth
    reads = ["ACGT", "", "TTGACCA"]
    p = str(tmp_path / "w.fastq")
    synth.write_fastq(p, reads, seed=5)
    first = open(p).read()
    assert prod.read_fastq(p) == reads and first.startswith("@input_read0\nACGT\n+\n")
    synth.write_fastq(p, reads, seed=5)
    assert open(p).read() == first
    synth.write_fastq(p, reads, quals=["IIII", "", "!!!!!!!"])
    assert prod.read_fastq(p, 1) == ["ACGT", "", "NNNNNNN"]
    with pytest.raises(ValueError):
        synth.write_fastq(p, reads, quals=["III", "", "!!!!!!!"])


# ---------------------------------------------------------------------------------------------- GPU


def as_list(bases, offsets):
    b = bases.tobytes()
    return [b[int(x):int(y)] for x, y in zip(offsets[:-1], offsets[1:])]


def packed(reads):
    """(bases, offsets, checksum) a handle holds for the list of bytes reads."""
    import _dbg
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    g = _dbg.Graph()
    g.set_reads(bases, offsets)
    s = g.reads_checksum()
    g.close()
    return bases, offsets, s


def streamed(path, begin=0, end=None, chunk=0, q=0):
    """(bases, offsets, checksum, ingest stats, fastq stats) of one ingest on a fresh handle"""
    import _dbg
    g = _dbg.Graph()
    g.set_reads_fastq_file(path, begin, end, chunk, q)
    out = g.copy_reads() + (g.reads_checksum(), g.ingest_stats(), g.fastq_stats())
    g.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_streamed_reads_at_every_chunk_size(name, tmp_path):
    import debruijn as prod
    text, hand = CASES[name]
    p = write(tmp_path, name, text)
    data = open(p, "rb").read()
    want = [r.encode() for r in hand]
    assert prod.read_fastq(p) == hand
    wb, wo, wsum = packed(want)
    for chunk in CHUNKS:
        b, o, s, st, fq = streamed(p, chunk=chunk)
        assert as_list(b, o) == want, chunk
        assert np.array_equal(o, wo) and np.array_equal(b, wb) and s == wsum, chunk
        assert fq["n_records"] == st["n_reads"] == len(want) and st["n_bases"] == wb.size, chunk
        assert st["bytes_read"] == len(data.rstrip(SPACE)), chunk
        assert (fq["first_byte"], fq["end_byte"]) == (0, len(data.rstrip(SPACE)))
        assert fq["masked_bases"] == 0 and fq["quality_bytes_held"] == 0
        if chunk:
            assert st["chunks"] == -(-st["bytes_read"] // chunk)


def border_file():
    """About 3 000 records of 40 to ~90 bases whose starts fall one before, on and one after the multiples of 65 536 (the
    parse kernels' blocks), and on every residue of 32 (their words)."""
    rng = random.Random(31)
    out, reads, pos, rec_starts, bangs = [], [], 0, [], 0
    target, shift = 65536, -1
    for i in range(3000):
        hdr = f"@r{i}"
        rem = target + shift - pos
        if rem >= 400:
            n = rng.randint(40, 90)
        elif rem >= 196:
            n = 40
        else:  # the next record starts exactly at target + shift
            n = (rem - 5 - len(hdr)) // 2
            hdr += "x" * (rem - 5 - len(hdr) - 2 * n)
            target, shift = target + 65536, (shift + 2) % 3 - 1
        seq = "".join(rng.choice("ACGT") for _ in range(n))
        qual = "".join(rng.choice("@+I5!~") for _ in range(n))
        rec = f"{hdr}\n{seq}\n+\n{qual}\n"
        rec_starts.append(pos)
        bangs += qual.count("!")
        out.append(rec)
        reads.append(seq.encode())
        pos += len(rec)
    return "".join(out).encode(), reads, rec_starts, bangs


@pytest.mark.gpu
def test_block_and_scan_borders(tmp_path):
    import debruijn as prod
    data, reads, rec_starts, bangs = border_file()
    assert len(data) > 5 * 65536 and len(data) // 32 > 4096  # several blocks, more words than one scan tile
    on = {d: sum(1 for s in rec_starts if s and (s - d) % 65536 == 0) for d in (-1, 0, 1)}
    assert min(on.values()) >= 1, on
    assert {s % 32 for s in rec_starts} >= {31, 0, 1}
    p = write(tmp_path, "borders", data)
    assert prod.parse_fastq(data) == reads
    wb, wo, wsum = packed(reads)
    for chunk, q in ((0, 0), (98305, 0), (0, 1), (98305, 1)):  # q = 1 masks nothing here ('!' is Phred 0: those it does)
        want = prod.parse_fastq(data, q)
        b, o, s, st, fq = streamed(p, chunk=chunk, q=q)
        assert np.array_equal(o, wo), (chunk, q)
        assert as_list(b, o) == want, (chunk, q)
        if q == 0:
            assert np.array_equal(b, wb) and s == wsum
        assert fq["n_records"] == len(reads) and st["bytes_read"] == len(data.rstrip(SPACE))
        assert fq["masked_bases"] == (bangs if q else 0)
    # a cut at a block border, one before and one after: the two parts make the whole
    for cut in (65535, 65536, 65537, 3 * 65536):
        left = as_list(*streamed(p, 0, cut, 98305)[:2])
        right = as_list(*streamed(p, cut, None, 0)[:2])
        assert left == expected_reads(data, 0, cut) and left + right == reads, cut


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_two_and_three_ranges_make_the_whole(name, tmp_path):
    text, hand = CASES[name]
    p = write(tmp_path, name, text)
    data = open(p, "rb").read()
    whole = [r.encode() for r in hand]
    step = 1 if len(data) < 200 else 97
    for i, b in enumerate(list(range(0, len(data) + 2, step)) + [max(len(data) - 1, 0)]):
        chunk = CHUNKS[i % len(CHUNKS)]
        left = as_list(*streamed(p, 0, b, chunk)[:2])
        right = as_list(*streamed(p, b, None, chunk)[:2])
        assert left == expected_reads(data, 0, b) and left + right == whole, (b, chunk)
        c = b + (i * 7) % 23  # a third range, often inside the same record, sometimes empty
        mid = as_list(*streamed(p, b, c, CHUNKS[(i + 3) % len(CHUNKS)])[:2])
        last = as_list(*streamed(p, c, None, chunk)[:2])
        assert mid == expected_reads(data, b, c) and left + mid + last == whole, (b, c, chunk)


def random_fastq(rng):
    term = rng.choice(["\n", "\r\n", "\r", None])
    recs = []
    while sum(map(len, recs)) < rng.randint(0, 330):
        n = rng.choice([0, 0, 1, 2, 3, 7, 15, 16, 17, 31, 32, 33, 40])
        seq = "".join(rng.choice("ACGTNacgt") for _ in range(n))
        qual = "".join(rng.choice("@+@+I5!~#") for _ in range(n))
        hdr = "@" + "".join(rng.choice("@+r1 ") for _ in range(rng.randint(0, 6)))
        sep = "+" + "".join(rng.choice("@+r1 ") for _ in range(rng.randint(0, 3)))
        pad = [" " * rng.choice([0, 0, 0, 1, 3]) for _ in range(4)]
        recs.append("".join(line + sp + (term or rng.choice(["\n", "\r\n", "\r"]))
                            for line, sp in zip((hdr, seq, sep, qual), pad)))
    text = "".join(recs)
    if rng.random() < 0.4:
        text = text.rstrip("\r\n")  # no final newline; a last empty read then loses its quality line
    return text[:399]


@pytest.mark.gpu
def test_seeded_fuzz_of_files_chunks_and_cuts(tmp_path):
    import debruijn as prod
    rng = random.Random(2025)
    done = 0
    while done < 200:
        text = random_fastq(rng)
        data = text.encode()
        try:
            whole = prod.parse_fastq(data)
        except ValueError:  # cut at 399 bytes inside a record
            continue
        p = write(tmp_path, f"f{done}", data)
        wb, wo, wsum = packed(whole)
        b, o, s, _, _ = streamed(p, chunk=rng.choice([1, 2, 3, 7, 13, 32, 100, 0]))
        assert as_list(b, o) == whole, done
        assert np.array_equal(o, wo) and np.array_equal(b, wb) and s == wsum, done
        cuts = sorted(rng.randint(0, len(data) + 1) for _ in range(rng.randint(1, 3)))
        bounds = [0] + cuts + [None]
        got = []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            part = as_list(*streamed(p, lo, hi, rng.choice([1, 3, 5, 16, 64, 0]))[:2])
            assert part == expected_reads(data, lo, hi), (done, lo, hi)
            got += part
        assert got == whole, (done, cuts)
        done += 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_files_fail_and_leave_the_handle_usable(name, tmp_path):
    import _dbg
    text, record, kind, q = MALFORMED[name]
    bad = write(tmp_path, name, text)
    good = write(tmp_path, "good", PLAIN)
    g = _dbg.Graph()
    for chunk in (1, 0):
        g.set_reads_fastq_file(good, chunk_bytes=chunk)
        assert g.sizes()["n_reads"] == 2
        with pytest.raises(_dbg.DbgError) as e:
            g.set_reads_fastq_file(bad, chunk_bytes=chunk, min_quality=q)
        assert e.value.code == _dbg.DBG_E_ARG and f"record {record}: {kind}" in str(e.value), (chunk, str(e.value))
        assert g.sizes()["n_reads"] == 0 and g.sizes()["n_bytes"] == 0
        g.set_reads_fastq_file(good, chunk_bytes=chunk)
        assert as_list(*g.copy_reads()) == [b"ACGTACGTTG", b"TTGACCA"]
    if kind == "quality byte":  # with the mask off no quality byte is looked at
        g.set_reads_fastq_file(bad)
        assert g.sizes()["n_reads"] == 2
    g.close()


@pytest.mark.gpu
def test_more_records_in_the_first_chunk_than_the_first_offsets_hold(tmp_path):
    """The offsets start with 65 536 entries at the most and are sized from the records seen only from the second chunk on:
    70 000 records in the first chunk make the ingest grow them and parse the chunk a second time."""
    import debruijn as prod
    n = 70_000
    data = b"".join(b"@\n" + s + b"\n+\nIIII\n" for s in (b"ACGT", b"CGTA", b"GTAC", b"TACG")) * (n // 4)
    p = write(tmp_path, "many", data)
    want = prod.parse_fastq(data)
    assert len(want) == n and want[:5] == [b"ACGT", b"CGTA", b"GTAC", b"TACG", b"ACGT"]
    for q in (0, 20):
        b, o, _, st, fq = streamed(p, q=q)
        assert as_list(b, o) == want, q
        assert st["chunks"] == 1 and st["n_reads"] == fq["n_records"] == n and st["n_bases"] == 4 * n, q


@pytest.mark.gpu
@pytest.mark.parametrize("q", [0, 20])
def test_a_read_of_more_than_half_its_record_grows_the_buffers_until_the_next_header_reports_it(q, tmp_path):
    """The bases (and, under a mask, the quality bytes) have room for half the range.  A 64-base read with a one-byte quality
    line outgrows it in a chunk that ends before the next header: the buffers grow and the chunk runs again, and the chunk
    with the next header reports the record.  At the default chunk size the report comes with the first parse."""
    import _dbg
    import debruijn as prod
    bad = write(tmp_path, "long_read_short_quality", "@a\n" + "ACGT" * 16 + "\n+\nI\n@b\nACGT\n+\nIIII\n")
    good = write(tmp_path, "good", PLAIN)
    with pytest.raises(ValueError) as e:
        prod.read_fastq(bad, min_quality=q)
    assert (e.value.record, e.value.kind) == (0, "length mismatch")
    g = _dbg.Graph()
    for chunk in (16, 64, 0):
        with pytest.raises(_dbg.DbgError) as e:
            g.set_reads_fastq_file(bad, chunk_bytes=chunk, min_quality=q)
        assert e.value.code == _dbg.DBG_E_ARG and "record 0: length mismatch" in str(e.value), (chunk, str(e.value))
        assert g.sizes()["n_reads"] == 0 and g.sizes()["n_bytes"] == 0
        g.set_reads_fastq_file(good, chunk_bytes=chunk, min_quality=q)
        assert as_list(*g.copy_reads()) == [b"ACGTACGTTG", b"TTGACCA"]
    g.close()


@pytest.mark.gpu
def test_errors_and_empty_ranges(tmp_path):
    import _dbg
    p = write(tmp_path, "small", PLAIN)
    g = _dbg.Graph()
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fastq_file(str(tmp_path / "missing.fastq"))
    assert e.value.code == _dbg.DBG_E_ARG and "missing.fastq" in str(e.value)
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fastq_file(p, 5, 4)
    assert e.value.code == _dbg.DBG_E_ARG and "begin" in str(e.value)
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fastq_file(str(tmp_path))  # a directory
    assert e.value.code == _dbg.DBG_E_ARG
    with pytest.raises(_dbg.DbgError) as e:
        g.set_reads_fastq_file(p, min_quality=94)
    assert e.value.code == _dbg.DBG_E_ARG and "min_quality" in str(e.value)
    for begin in (len(PLAIN), len(PLAIN) + 1, 1 << 40):
        g.set_reads_fastq_file(p, begin)
        assert g.sizes()["n_reads"] == 0 and g.sizes()["n_bytes"] == 0
    g.set_reads_fastq_file(p, 28, 28)  # empty range at a record start
    assert g.sizes()["n_reads"] == 0
    g.set_reads_fastq_file(p, 5, 5)  # empty range inside a record
    assert g.sizes()["n_reads"] == 0
    g.set_reads_fastq_file(p, 28, 29)  # one byte: owns the record that starts there
    assert as_list(*g.copy_reads()) == [b"TTGACCA"]
    g.set_reads_fastq_file(p, 1, 28)  # the first header is in front of the range
    assert g.sizes()["n_reads"] == 0
    g.close()


def mask_file(tmp_path):
    """Reads with lower case and N, qualities that run through Phred 0..41."""
    rng = random.Random(8)
    reads, quals = [], []
    for i in range(60):
        n = rng.choice([0, 1, 15, 16, 17, 33, 64, 100])
        reads.append("".join(rng.choice("ACGTACGTNa") for _ in range(n)))
        quals.append("".join(chr(33 + (7 * i + 5 * j) % 42) for j in range(n)))
    import synth
    p = str(tmp_path / "mask.fastq")
    synth.write_fastq(p, reads, quals)
    return p, reads, quals


@pytest.mark.gpu
@pytest.mark.parametrize("q", [0, 1, 20, 41, 93])
def test_quality_mask_alone_and_feeding_the_split(q, tmp_path):
    import debruijn as prod
    p, reads, quals = mask_file(tmp_path)
    want = prod.read_fastq(p, min_quality=q)
    count = sum(ord(c) - 33 < q for qual in quals for c in qual)
    assert [len(r) for r in want] == [len(r) for r in reads] and (q > 0 or want == reads)
    for chunk in (0, 7, 64):
        b, o, _, st, fq = streamed(p, chunk=chunk, q=q)
        assert [r.decode() for r in as_list(b, o)] == want, chunk
        assert fq["masked_bases"] == count and fq["min_quality"] == q
        assert (fq["quality_bytes_held"] > 0) == (q > 0)
    kept = prod.read_reads_device(p, format="fastq", min_quality=q)
    assert list(kept) == want and kept.split_stats is None
    cut = prod.read_reads_device(p, format="fastq", min_quality=q, non_acgt="split", chunk_bytes=100)
    assert list(cut) == prod.acgt_pieces(want)
    org = [(i, m.start()) for i, r in enumerate(want) for m in re.finditer("[ACGT]+", r)]
    ri, pos = cut.origins()
    assert list(zip(ri.tolist(), pos.tolist())) == org
    assert cut.split_stats["n_reads_in"] == len(reads) and cut.split_stats["n_reads_out"] == len(org)


@pytest.mark.gpu
def test_quality_bytes_out_of_range_fail_only_under_a_mask(tmp_path):
    import _dbg
    g = _dbg.Graph()
    for byte in (32, 127):
        p = write(tmp_path, f"q{byte}", b"@a\nACGT\n+\nIIII\n@b\nACG\n+\nI" + bytes([byte]) + b"I\n")
        for chunk in (1, 0):
            with pytest.raises(_dbg.DbgError) as e:
                g.set_reads_fastq_file(p, chunk_bytes=chunk, min_quality=1)
            assert e.value.code == _dbg.DBG_E_ARG and "record 1: quality byte" in str(e.value)
            assert g.sizes()["n_reads"] == 0
            g.set_reads_fastq_file(p, chunk_bytes=chunk, min_quality=0)
            assert as_list(*g.copy_reads()) == [b"ACGT", b"ACG"]
    g.close()


def graph_digest(g):
    keys, stamps, counts, _ = g.export_nodes(flags=False)
    o = np.argsort(stamps, kind="stable")
    h = hashlib.sha256()
    for a in (keys[o], g.export_keys_hi()[o], stamps[o], counts[o]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def synth_fastq(tmp_path_factory):
    import synth
    reads = synth.reads_list(9, 3000, 3000, 80, 0.01)
    p = str(tmp_path_factory.mktemp("fastq") / "reads.fastq")
    synth.write_fastq(p, reads, seed=3)
    return p, reads


@pytest.mark.gpu
def test_device_reads_surface(synth_fastq):
    import debruijn as prod
    p, reads = synth_fastq
    size = os.path.getsize(p)
    assert prod.read_fastq(p) == reads
    dev = prod.read_reads_device(p, format="fastq")
    assert list(dev) == reads and len(dev) == len(reads) and dev[-1] == reads[-1]
    assert dev._graph.ingest_stats()["chunks"] == 1  # the streamed call, whatever the size
    assert list(prod.read_reads_device(p, format="fastq", chunk_bytes=1000)) == reads
    as_fasta = prod.read_reads_device(p)  # nothing is detected: every line that does not begin with '>' is a read, as before
    assert list(as_fasta) == orc.read_reads(p) and 3 * len(reads) < len(as_fasta) <= 4 * len(reads)
    halves = [prod.DeviceReads(p, byte_range=r, chunk_bytes=4096, format="fastq") for r in ((0, size // 2), (size // 2, None))]
    assert list(halves[0]) + list(halves[1]) == reads and 0 < len(halves[0]) < len(reads)
    with pytest.raises(ValueError):
        prod.read_reads_device(p, format="fastx")
    with pytest.raises(ValueError):
        prod.read_reads_device(p, min_quality=20)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_ranks_ingest_their_slices_of_a_fastq_file(world, synth_fastq):
    import _dbg
    import inproc_dist
    import multi_gpu
    p, reads = synth_fastq

    def one(dist, rank):
        g = _dbg.Graph(device=0)
        multi_gpu.set_reads_fasta_shard(g, p, dist, chunk_bytes=1 << 16, format="fastq")
        out = as_list(*g.copy_reads())
        g.close()
        return out

    shards = inproc_dist.run_ranks(world, one)
    assert all(shards) and [r.decode() for s in shards for r in s] == reads


@pytest.mark.gpu
def test_graph_from_fastq_equals_graph_from_the_reads(synth_fastq):
    import _dbg
    p, reads = synth_fastq
    a = _dbg.Graph()
    a.set_reads(*packed([r.encode() for r in reads])[:2])
    b = _dbg.Graph()
    b.set_reads_fastq_file(p, chunk_bytes=1 << 16)
    assert a.reads_checksum() == b.reads_checksum()
    for g in (a, b):
        g.build(31)
    assert a.sizes()["n_nodes"] == b.sizes()["n_nodes"] > 0
    assert graph_digest(a) == graph_digest(b)
    a.close()
    b.close()


def memory_bound(range_bytes, n_reads, chunk, mask):
    """bases from half the range (twice while a mask holds the qualities), offsets (old and new array of a
    grow: 20 B a read), 1.75 chunks of parse state rounded up to 2, 1 MiB for everything small."""
    return (2 if mask else 1) * (range_bytes // 2 + 64) + 20 * (n_reads + 1) + 2 * min(chunk, range_bytes) + (1 << 20)


@pytest.mark.gpu
def test_peak_device_memory_stays_under_the_bound(tmp_path):
    n, L, chunk = 100_000, 100, 4 << 20
    rng = np.random.default_rng(4)
    hdr = np.frombuffer(b"@input_read\n", dtype=np.uint8)
    rec = np.empty((n, hdr.size + L + 3 + L + 1), dtype=np.uint8)
    rec[:, :hdr.size] = hdr
    rec[:, hdr.size:hdr.size + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
    rec[:, hdr.size + L:hdr.size + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, hdr.size + L + 3:-1] = rng.integers(33 + 2, 33 + 42, (n, L), dtype=np.uint8)
    rec[:, -1] = 10
    p = str(tmp_path / "big.fastq")
    rec.reshape(-1).tofile(p)
    size = os.path.getsize(p)
    quals = rec[:, hdr.size + L + 3:-1]
    for q in (0, 20):
        b, o, _, st, fq = streamed(p, chunk=chunk, q=q)
        assert fq["n_records"] == n and st["n_bases"] == n * L and st["chunks"] == -(-size // chunk)
        assert fq["masked_bases"] == int((quals < 33 + q).sum())
        want = np.where(quals < 33 + q, np.uint8(78), rec[:, hdr.size:hdr.size + L])
        assert np.array_equal(b.reshape(n, L), want)
        bound = memory_bound(size, n, chunk, q > 0)
        assert 0 < fq["peak_device_bytes"] == st["peak_device_bytes"] <= bound, (q, fq, bound)
        assert fq["quality_bytes_held"] == ((size - 1) // 2 + 64 if q else 0)  # the final newline is not a record's
