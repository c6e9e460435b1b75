"""The plain-C++ part of csrc/dbg_spectrum.h on the CPU (tests/spectrum_host.cpp): the bin of a count at the borders of
B = 2, 3, 4096 and 2^20, the split between LDS bins and global bins, the degree and the kept degree of every flag byte and of
masks with 0, 1, 20 and 32 bits, and the body of one row over CSRs with 32- and 64-bit row pointers (empty rows, a last row
that ends at n_edges, arrays of exactly n_nodes row pointers) and over dense rows of 4 and 32 counters -- all against the rule
stated count by count.  Compiled with the host compiler under AddressSanitizer and UBSan where it offers them, run as a
stand-alone program; nothing is loaded into Python.
The plain-Python statement of the rule (debruijn.count_spectrum on dicts) is checked here against the numbers the reference
itself recorded for every golden case."""
import contextlib
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import debruijn as prod
from conftest import case_reads, golden_case_names, load_golden
from oracle import dbg_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")


def _compile(cxx, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, "-o", exe,
           os.path.join(HERE, "spectrum_host.cpp")]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_plain_cpp_of_the_spectrum_kernel_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "spectrum_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = _compile(cxx, exe, san)
    if r.returncode != 0 and ("sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout):
        r = _compile(cxx, exe, [])  # a compiler without the sanitizer runtimes: the plain build checks the same values
    assert r.returncode == 0, r.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout


def test_header_binding_and_kernel_constants_agree():
    import _dbg
    root = os.path.dirname(HERE)
    h = open(os.path.join(root, "include", "dbg.h")).read()
    assert re.search(r"int dbg_count_spectrum\(dbg_t \*h, int part, uint64_t n_bins, uint64_t \*edge_hist, uint64_t \*node_hist, "
                     r"dbg_spectrum_t \*out\);", h)
    body = re.search(r"typedef struct dbg_spectrum \{(.*?)\} dbg_spectrum_t;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"(uint64_t|double) (\w+)(?:\[(\d+)\])?;", body)
    assert [n for _, n, _ in decls] == [n for n, _ in _dbg.Spectrum._fields_]
    assert [n for _, n, _ in decls] == ["n_nodes", "n_edges", "sum_edge_counts", "max_edge_count", "max_out_weight", "D", "K",
                                        "pruned", "n_bins", "peak_extra_device_bytes", "ms_kernel"]
    assert [(n, dim) for _, n, dim in decls if dim] == [("D", "33"), ("K", "33")]
    assert [t for t, n, _ in decls if n == "ms_kernel"] == ["double"]
    import ctypes
    assert ctypes.sizeof(_dbg.Spectrum) == 8 * (5 + 66 + 3 + 1)
    assert re.search(r"#define DBG_ABI_VERSION 6\b", h) and _dbg.ABI_VERSION == 6 and "dbg_count_spectrum" in _dbg.SYMBOLS
    src = open(os.path.join(CSRC, "dbg_spectrum.h")).read()
    assert int(re.search(r"constexpr uint32_t SP_LDS_BINS = (\d+);", src).group(1)) == _dbg.SP_LDS_BINS
    assert re.search(r"constexpr uint64_t SP_MAX_BINS = 1ull << 20;", src) and _dbg.SP_MAX_BINS == 1 << 20
    assert '#include "dbg_spectrum.h"' in open(os.path.join(CSRC, "dbg_hip.hip")).read()


def _oracle_dicts(case):
    inp = case["inputs"]
    with contextlib.redirect_stdout(io.StringIO()):
        g, _, _, _, ect = orc.construct_graph(list(case_reads(case)), inp["k"], threshold=inp["threshold"], final=inp["final"])
    return g, ect


@pytest.mark.parametrize("name", golden_case_names())
def test_host_rule_agrees_with_the_numbers_the_reference_recorded(name):
    case = load_golden(name)
    g, ect = _oracle_dicts(case)
    s = case["summary"]
    clamped = False
    for B in (64, 4):
        sp = prod.count_spectrum(g, ect, B)
        E, W, D = sp["edge_hist"], sp["node_hist"], sp["D"]
        assert E.dtype == W.dtype == D.dtype == np.uint64 and E.size == W.size == B and D.size == 33
        assert int(E[0]) == 0
        assert int(E.sum()) == s["n_edge_names"] == sp["n_edges"]
        assert int(W.sum()) == int(D.sum()) == s["n_vertices"] == sp["n_nodes"]
        assert sp["sum_edge_counts"] == s["sum_edge_counts"]
        # below the clamp bin every edge is worth its bin; the clamp bin holds the rest of the sum, by its definition
        below = sum(c * int(E[c]) for c in range(B - 1))
        rest = sum(c for c in ect.values() if c >= B - 1)
        assert below + rest == s["sum_edge_counts"]
        assert int(E[B - 1]) == sum(1 for c in ect.values() if c >= B - 1)
        if sp["max_edge_count"] < B - 1:
            assert sum(c * int(E[c]) for c in range(B)) == s["sum_edge_counts"]
        else:
            clamped = True
        assert sp["max_edge_count"] == max(ect.values(), default=0)
        want_d = np.bincount([n.outdegree for n in g[0].values()], minlength=33)
        assert np.array_equal(D, want_d.astype(np.uint64))
        assert int(W[0]) == sum(1 for n in g[0].values() if n.outdegree == 0)
    if name.startswith(("dna_med_", "dna_small_")):
        assert clamped, "B = 4 must really clamp on the sequencing-like cases"


def test_host_rule_refuses_bad_bin_counts():
    for bad in (0, 1, (1 << 20) + 1, -3):
        with pytest.raises(ValueError):
            prod.count_spectrum(({}, {}), {}, bad)
    sp = prod.count_spectrum(({}, {}), {}, 2)
    assert sp["n_nodes"] == sp["n_edges"] == sp["max_out_weight"] == 0 and not sp["edge_hist"].any() and not sp["node_hist"].any()
