"""Record-mode FASTA and wrapped contig output on the CPU: the plain-Python statement of the rules
(debruijn.parse_fasta_records / read_fasta_records / wrap_fasta_record) on hand-written files, its agreement with read_reads
where a record is one line, and the plain-C++ parts -- the header search of csrc/dbg_fasta.h and the wrapped record geometry
of csrc/dbg_ctgout.h (tests/fasta_records_host.cpp) -- compiled with the host compiler under AddressSanitizer and UBSan where
it offers them and run as a stand-alone program; nothing is loaded into Python.  FILES is shared with the GPU tests
(tests/test_fasta_records.py), which run every file here through the device."""
import os
import re
import shutil
import subprocess

import pytest

import debruijn as prod

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")

# name -> (bytes of the file, the reads it holds, written down by hand)
FILES = {
    "lf": (b">a\nACGT\nAC\n>b\nGG\n", [b"ACGTAC", b"GG"]),
    "crlf": (b">a\r\nACGT\r\nAC\r\n>b\r\nGG\r\n", [b"ACGTAC", b"GG"]),
    "lone_cr": (b">a\rACGT\rAC\r>b\rGG\r", [b"ACGTAC", b"GG"]),
    "mixed_terminators": (b">a\rACGT\r\nAC\n>b\n\rGG\r\n", [b"ACGTAC", b"GG"]),
    "no_final_terminator": (b">a\nACGT\nAC\n>b\nGG", [b"ACGTAC", b"GG"]),
    "header_without_terminator": (b">a\nAC\n>b", [b"AC", b""]),
    "blank_lines": (b">a\n\nAC\n\n\nGT\n\n>b\n\n>c\nT\n\n", [b"ACGT", b"", b"T"]),
    "trailing_blanks_and_tabs": (b">a\nAC \t\nG T\t \n  \n>b \t\nC\x1f\x1c\n", [b"ACG T", b"C"]),
    "consecutive_headers": (b">a\n>b\n>c\nAC\n>d\n>e\n", [b"", b"", b"AC", b"", b""]),
    "header_at_the_end": (b">a\nAC\n>b\n", [b"AC", b""]),
    "headers_only": (b">a\n>b\r\n>c\r>d", [b"", b"", b"", b""]),
    "empty": (b"", []),
    "blank_only": (b"\n \n\t\r\n", []),
    "blank_before_first_header": (b"\n \t\n\r\n>a\nAC\nGT\n", [b"ACGT"]),
    "gt_inside_a_line": (b">a\nAC>GT\nA>\n>b>c\nT>\n", [b"AC>GTA>", b"T>"]),
    "space_then_gt": (b">a\nAC\n >b\nGT\n", [b"AC >bGT"]),
    "form_feed_inside_a_line": (b">a\nAC\x0cGT\nA\x0c\n\x0c\n>b\n\x0cT\n", [b"AC\x0cGTA", b"\x0cT"]),
    "space_inside_a_line": (b">a\nAC GT\n T\n", [b"AC GT T"]),
    "one_header_byte": (b">", [b""]),
    "wrapped_150_at_60": (b">r\n" + b"A" * 60 + b"\n" + b"C" * 60 + b"\n" + b"G" * 30 + b"\n", [b"A" * 60 + b"C" * 60 + b"G" * 30]),
}
# name -> (bytes, 0-based line and byte position of the first offending byte)
MALFORMED = {
    "sequence_first": (b"ACGT\n>a\nAC\n", 0, 0),
    "sequence_after_blanks": (b"\n \t\r\n  AC\n>a\nGT\n", 2, 7),
    "no_header_at_all": (b"\nACGT\nAC\n", 1, 1),
    "space_then_gt_first": (b" >a\nAC\n", 0, 1),
}


@pytest.mark.parametrize("name", sorted(FILES))
def test_host_parser_on_hand_written_files(name, tmp_path):
    data, want = FILES[name]
    assert prod.parse_fasta_records(data) == want
    assert prod.parse_fasta_records(bytearray(data)) == want
    p = tmp_path / "f.fasta"
    p.write_bytes(data)
    assert prod.read_fasta_records(str(p)) == [r.decode("latin-1") for r in want]


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_host_parser_names_sequence_before_the_first_header(name):
    data, line, pos = MALFORMED[name]
    with pytest.raises(prod.FastaError) as e:
        prod.parse_fasta_records(data)
    assert isinstance(e.value, ValueError)
    assert (e.value.kind, e.value.line, e.value.pos) == ("sequence before the first header", line, pos)
    assert "sequence before the first header" in str(e.value) and str(pos) in str(e.value)


def test_record_mode_is_line_mode_where_every_record_is_one_line(tmp_path):
    import synth
    reads = synth.reads_list(5, 2000, 40, 70, 0.02) + ["AC GT", "N", "acgt\x0cA"]
    for nl in ("\n", "\r\n", "\r"):
        p = tmp_path / "one_line.fasta"
        p.write_bytes("".join(f">r{i}{nl}{r}{nl}" for i, r in enumerate(reads)).encode("latin-1"))
        assert prod.read_fasta_records(str(p)) == prod.read_reads(str(p)) == reads


@pytest.mark.parametrize("width", [1, 2, 60])
def test_wrap_rule_and_its_inverse(width):
    for n in sorted({0, 1, width - 1, width, width + 1, 2 * width, 2 * width + 1}):
        text = "".join("ACGT"[(7 * i + n) & 3] for i in range(n))
        body = prod.wrap_fasta_record(text, width)
        lines = body.split("\n")
        assert lines[-1] == "" and "".join(lines) == text                       # every line ends with a newline
        assert len(body) == n + max(1, -(-n // width))                           # the record body's length
        assert all(len(x) == width for x in lines[:-2]) and len(lines[-2]) <= width
        assert n == 0 or 1 <= len(lines[-2])                                     # no extra empty line
        for q, ch in enumerate(body):                                            # the byte-by-byte statement
            nl = q % (width + 1) == width or q == len(body) - 1
            assert ch == ("\n" if nl else text[q - q // (width + 1)])
        assert prod.wrap_fasta_record(text.encode(), width) == body.encode()
        assert prod.wrap_fasta_record(text, 0) == text + "\n"
        assert prod.parse_fasta_records((">SEQUENCE_0_31mer\n" + body).encode()) == [text.encode()]
    texts = ["ACGTACGTA", "", "C" * (2 * width), "G"]
    image = "".join(f">SEQUENCE_{i}_9mer\n" + prod.wrap_fasta_record(t, width) for i, t in enumerate(texts))
    assert prod.parse_fasta_records(image.encode()) == [t.encode() for t in texts]


def _compile(cxx, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, "-o", exe,
           os.path.join(HERE, "fasta_records_host.cpp")]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_header_search_and_wrapped_geometry_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "fasta_records_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = _compile(cxx, exe, san)
    if r.returncode != 0 and ("sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout):
        r = _compile(cxx, exe, [])  # a compiler without the sanitizer runtimes: the plain build checks the same values
    assert r.returncode == 0, r.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout


def _struct_names(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [x.strip() for decl in re.findall(r"(?:uint64_t|double) ([^;]*);", body) for x in decl.split(",")]


def test_header_binding_and_struct_fields_agree():
    import inspect
    import _dbg
    import multi_gpu
    root = os.path.dirname(HERE)
    h = open(os.path.join(root, "include", "dbg.h")).read()
    assert re.search(r"int dbg_set_reads_fasta_records\(dbg_t \*h, const char \*text, uint64_t n_text\);", h)
    assert re.search(r"int dbg_set_reads_fasta_records_file\(dbg_t \*h, const char \*path, uint64_t begin, uint64_t end, "
                     r"uint64_t chunk_bytes\);", h)
    assert re.search(r"int dbg_fasta_records_stats\(dbg_t \*h, dbg_fasta_records_stats_t \*out\);", h)
    assert re.search(r"int dbg_write_contigs_fasta_wrapped\(dbg_t \*h, const char \*path, int append, const uint64_t \*indices, "
                     r"uint64_t n,\s*uint64_t first_number, int k_label, uint64_t chunk_bytes, uint32_t line_width,\s*"
                     r"uint64_t \*bytes_written\);", h)
    names = _struct_names(h, "dbg_fasta_records_stats")
    assert names == [n for n, _ in _dbg.FastaRecordsStats._fields_]
    assert names == ["n_records", "n_sequence_lines", "longest_record", "first_byte", "end_byte", "scan_bytes"]
    assert re.search(r"#define DBG_ABI_VERSION 6\b", h) and _dbg.ABI_VERSION == 6
    for sym in ("dbg_set_reads_fasta_records", "dbg_set_reads_fasta_records_file", "dbg_fasta_records_stats",
                "dbg_write_contigs_fasta_wrapped"):
        assert sym in _dbg.SYMBOLS
    for fn in (_dbg.Graph.set_reads_fasta_records, _dbg.Graph.set_reads_fasta_records_file, _dbg.Graph.fasta_records_stats):
        assert callable(fn)
    assert list(inspect.signature(_dbg.Graph.set_reads_fasta_records_file).parameters) == ["self", "path", "begin", "end", "chunk_bytes"]
    assert inspect.signature(_dbg.Graph.write_contigs_fasta).parameters["line_width"].default == 0
    assert inspect.signature(prod.LazyContigs.write_fasta).parameters["line_width"].default == 0
    for fn in (prod.DeviceReads.__init__, prod.read_reads_device, multi_gpu.set_reads_fasta_shard):  # the new LAST keyword
        assert list(inspect.signature(fn).parameters)[-1] == "records"
        assert inspect.signature(fn).parameters["records"].default == "line"


def test_bad_keywords_are_refused_before_anything_runs(tmp_path):
    p = tmp_path / "x.fasta"
    p.write_bytes(b">a\nAC\n")
    with pytest.raises(ValueError, match="records"):
        prod.DeviceReads(str(p), records="wrapped")
    with pytest.raises(ValueError, match="records"):
        prod.DeviceReads(str(p), format="fastq", records="record")
    import multi_gpu
    with pytest.raises(ValueError, match="records"):
        multi_gpu.set_reads_fasta_shard(None, str(p), None, records="both")
    with pytest.raises(ValueError, match="records"):
        multi_gpu.set_reads_fasta_shard(None, str(p), None, format="fastq", records="record")


@pytest.mark.parametrize("key,value", [("fasta_records", "both"), ("fasta_records", 1), ("fasta_line_width", -1),
                                       ("fasta_line_width", "60"), ("fasta_line_width", True)])
def test_driver_refuses_other_values_of_the_new_keys_before_it_reads_anything(key, value, tmp_path):
    import json
    import sys
    import synth
    froot = "badkeys"
    synth.write_froot(str(tmp_path / froot), ["ACGTACGTAC"], 3, 4, threshold=1)
    with open(tmp_path / froot / "setting.json") as fh:
        setting = json.load(fh)
    setting[key] = value
    with open(tmp_path / froot / "setting.json", "w") as fh:
        json.dump(setting, fh)
    pkg = os.path.join(os.path.dirname(HERE), "py-debruijn_amd")
    r = subprocess.run([sys.executable, os.path.join(pkg, "II_assembleFromReads.py"), "-froot", froot], cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=pkg), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "ValueError" in r.stderr and key in r.stderr, r.stderr
    assert not (tmp_path / froot / f"{froot}.fasta").exists()
