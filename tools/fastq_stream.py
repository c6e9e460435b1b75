#!/usr/bin/env python3
"""FASTQ file -> resident reads, beside the FASTA streamed ingest of the same reads (GPU box).

Times dbg_set_reads_fastq_file with the mask off and with min_quality 20, alternating in every round with
dbg_set_reads_fasta_file on a FASTA file of the same reads, page cache warm (both files are read once first), best of
--reps rounds, host clocks around calls that end in a synchronise.  Prints one JSON object: per path the wall ms, the
split (host file reads / H2D / parse / mask), the parse ms per GB of file, the peak device bytes against the bound of
DESIGN.md 4i, and whether the copies and the parse still hide under the host's file reads (ms_total - ms_io_wait small
against ms_h2d + ms_parse).  Checks that all three paths give the same bases where nothing is masked.

    python tools/fastq_stream.py [--reads 10e6] [--read-len 150] [--chunk 16] [--reps 3] [--min-quality 20]

The configs[1]-shaped files (N x 150 bp; FASTQ "@r\\n<read>\\n+\\n<qual>\\n", about 3.1 GB at 10 M reads; FASTA ">r\\n<read>\\n")
are written to a temporary directory first and removed afterwards.  Kernel times: run it under
``rocprofv3 --kernel-trace --stats -- python tools/fastq_stream.py --reps 1`` separately.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-debruijn_amd"))
import _dbg  # noqa: E402


def write_files(fastq, fasta, n, read_len, seed=1):
    g = _dbg.Graph()
    g.synth_reads(seed, n * 5, n, read_len, 0.01)
    bases, _ = g.copy_reads()
    g.close()
    rng = np.random.default_rng(seed)
    with open(fastq, "wb") as fq, open(fasta, "wb") as fa:
        step = 1 << 20
        for i in range(0, n, step):
            m = min(step, n - i)
            seq = bases[i * read_len:(i + m) * read_len].reshape(m, read_len)
            qual = rng.integers(33 + 2, 33 + 42, (m, read_len), dtype=np.uint8)  # Phred 2..41
            rec = np.empty((m, 3 + read_len + 3 + read_len + 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
            rec[:, 3:3 + read_len] = seq
            rec[:, 3 + read_len:6 + read_len] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 6 + read_len:-1] = qual
            rec[:, -1] = 10
            rec.tofile(fq)
            rec = np.empty((m, 3 + read_len + 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            rec[:, 3:3 + read_len] = seq
            rec[:, -1] = 10
            rec.tofile(fa)


def report(dt, st, size, extra=None):
    hidden = st["ms_total"] - st["ms_io_wait"]
    out = {"ms": round(dt * 1e3, 1), "ms_total": round(st["ms_total"], 1), "ms_io_wait": round(st["ms_io_wait"], 1),
           "ms_h2d": round(st["ms_h2d"], 1), "ms_parse": round(st["ms_parse"], 1),
           "parse_ms_per_GB_of_file": round(st["ms_parse"] / (size / 1e9), 2), "chunks": st["chunks"],
           "ms_not_in_file_reads": round(hidden, 1),
           "device_work_hidden_under_file_reads": bool(hidden < 0.5 * (st["ms_h2d"] + st["ms_parse"])),
           "peak_device_bytes": st["peak_device_bytes"], "peak_over_file": round(st["peak_device_bytes"] / size, 3)}
    out.update(extra or {})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=10e6)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--chunk", type=int, default=16, help="MiB")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-quality", type=int, default=20)
    args = ap.parse_args()
    n, chunk, mq = int(args.reads), args.chunk << 20, args.min_quality
    tmp = tempfile.mkdtemp(prefix="fastq_stream_")
    fastq, fasta = os.path.join(tmp, "reads.fastq"), os.path.join(tmp, "reads.fasta")
    try:
        write_files(fastq, fasta, n, args.read_len)
        sizes = {"fastq": os.path.getsize(fastq), "fasta": os.path.getsize(fasta)}
        for p in (fastq, fasta):  # warm the page cache
            with open(p, "rb") as fh:
                while fh.read(1 << 26):
                    pass
        g = _dbg.Graph()
        best = {}
        sums = {}
        for _ in range(args.reps):
            for name in ("fasta", "fastq", f"fastq_q{mq}"):
                t0 = time.perf_counter()
                if name == "fasta":
                    g.set_reads_fasta_file(fasta, chunk_bytes=chunk)
                else:
                    g.set_reads_fastq_file(fastq, chunk_bytes=chunk, min_quality=0 if name == "fastq" else mq)
                dt = time.perf_counter() - t0
                st = g.ingest_stats()
                fq = g.fastq_stats() if name != "fasta" else None
                sums[name] = (g.sizes()["n_reads"], g.reads_checksum())
                if name not in best or dt < best[name][0]:
                    best[name] = (dt, st, fq)
        g.close()
        out = {"reads": n, "read_len": args.read_len, "chunk_bytes": chunk, "file_bytes": sizes,
               "same_reads_fasta_fastq": bool(sums["fasta"] == sums["fastq"]),
               "fasta": report(best["fasta"][0], best["fasta"][1], sizes["fasta"])}
        for name in ("fastq", f"fastq_q{mq}"):
            dt, st, fq = best[name]
            mask = name != "fastq"
            bound = (2 if mask else 1) * (sizes["fastq"] // 2 + 64) + 20 * (n + 1) + 2 * min(chunk, sizes["fastq"]) + (1 << 20)
            out[name] = report(dt, st, sizes["fastq"], {
                "ms_mask": round(fq["ms_mask"], 2), "masked_bases": fq["masked_bases"], "n_records": fq["n_records"],
                "quality_bytes_held": fq["quality_bytes_held"], "bound_bytes": bound,
                "under_bound": bool(st["peak_device_bytes"] <= bound)})
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
