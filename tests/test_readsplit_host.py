"""The plain-C++ part of csrc/dbg_readsplit.h on the CPU: the keep mask of a word, the start mask (previous byte's keep bit
set and clear; read starts on a kept byte, on a cut byte and after one) and the fold, against a byte-by-byte statement of
the definition -- a cut at bit 0, at the last bit and at every bit between, bytes of 0x80 and above, whole words of cut
bytes, tails that are no whole word (tests/readsplit_host.cpp).  Compiled with the host compiler under AddressSanitizer
and UBSan where it offers them, run as a stand-alone program; nothing is loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "py-debruijn_amd", "csrc")


def _compile(cxx, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra, "-o", exe,
           os.path.join(HERE, "readsplit_host.cpp")]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_mask_helpers_of_the_read_split_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(tmp_path, "readsplit_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = _compile(cxx, exe, san)
    if r.returncode != 0 and ("sanitize" in r.stdout or "asan" in r.stdout or "ubsan" in r.stdout):
        r = _compile(cxx, exe, [])  # a compiler without the sanitizer runtimes: the plain build checks the same values
    assert r.returncode == 0, r.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), run.stdout
