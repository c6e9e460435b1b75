"""The plain-C++ part of csrc/dbg_fastq.h on the CPU: the line-start and non-space masks of a word, the sequence and quality
kind masks from a count of line starts, the quality mask on a dword, the record-start search and the trailing-white-space
trim, against byte-by-byte statements of the rules -- line starts at bit 0 and bit 31, tails of 1 to 31 bytes, every
position of files whose quality lines, headers and separators are full of '@' and '+' (tests/fastq_host.cpp).  Compiled with
the host compiler under AddressSanitizer and UBSan where it offers them, run as a stand-alone program; nothing is loaded
into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")


def _compile(cxx, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, "-o", exe,
           os.path.join(HERE, "fastq_host.cpp")]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_fastq_helpers_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "fastq_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = _compile(cxx, exe, san)
    if r.returncode != 0 and ("sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout):
        r = _compile(cxx, exe, [])  # a compiler without the sanitizer runtimes: the plain build checks the same values
    assert r.returncode == 0, r.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout
