"""The plain-C++ part of csrc/dbg_partfinal.h on the CPU: the final-mode walker over the contracted graph -- the very
function the kernel runs -- against a recursive node-by-node DFS written from debruijn.py:288-316, on hand-made cases (two
pulled successors of one branch node, a successor chain that re-enters the path inside a segment, a branching start, a
pulled start, a branch node with dead successors only, merging chains) and on 4000 random graphs of up to 40 nodes cut into
1 to 4 parts and contracted by a host restatement of the entry and segment rules -- each of them walked once with its own
stack and bitmap and once by three walkers that share one allocation, interleaved at stride 3 as the kernel lays them out,
with the neighbours' levels and words filled with a pattern that must survive --; a comb of 70 branch nodes (three bitmap
words, 70 levels) walked the same two ways; the validation predicate against each kind of broken row; the step budget
(tests/partfinal_host.cpp).  Compiled with the host compiler under AddressSanitizer and
UBSan where it offers them, run as a stand-alone program; nothing is loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")


def _compile(cxx, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, "-o", exe,
           os.path.join(HERE, "partfinal_host.cpp")]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_final_walker_over_the_contracted_graph_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "partfinal_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = _compile(cxx, exe, san)
    if r.returncode != 0 and ("sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout):
        r = _compile(cxx, exe, [])  # a compiler without the sanitizer runtimes: the plain build checks the same values
    assert r.returncode == 0, r.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout
