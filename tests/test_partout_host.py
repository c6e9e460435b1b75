"""The plain-C++ part of csrc/dbg_partout.h on the CPU: the validation predicate of a ranked skeleton against each kind of
broken row, the level count of the lifting table, and the text source over parts (CoPartsSrc) under the run emitter of
dbg_ctgout.h -- toy graphs in parts over 1, 2, 4 and 8 virtual shards, a run from every byte offset, one handle holding
all shards and one handle per shard whose outputs must add up to the text (tests/partout_host.cpp).  Compiled with the
host compiler under AddressSanitizer and UBSan where it offers them, run as a stand-alone program; nothing is loaded
into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")


def _compile(cxx, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, "-o", exe,
           os.path.join(HERE, "partout_host.cpp")]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_skeleton_validation_and_the_text_source_over_parts_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "partout_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = _compile(cxx, exe, san)
    if r.returncode != 0 and ("sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout):
        r = _compile(cxx, exe, [])  # a compiler without the sanitizer runtimes: the plain build checks the same values
    assert r.returncode == 0, r.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout
