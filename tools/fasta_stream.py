#!/usr/bin/env python3
"""File -> resident reads, one-shot against streamed (GPU box).

One-shot: np.fromfile + dbg_set_reads_fasta (the whole image on the host, one pageable copy, the parse on the device).
Streamed: dbg_set_reads_fasta_file at several chunk sizes (pinned double-buffered staging, per-chunk parse).
Both are timed with the page cache warm (the file is read once first).  Prints one JSON object: wall ms per path, the
streamed path's split (host file reads / H2D / parse, H2D GB/s of the pinned copies) and the peak device bytes of each
path (dbg_fasta_ingest_stats), and checks that every path gives the same reads (checksum, count).

    python tools/fasta_stream.py [--reads 10e6] [--path FILE] [--chunks 4,16,64] [--reps 3]

Without --path the configs[1]-shaped file (N x 150 bp records ">r\\n<read>\\n", 1.54 GB at 10 M reads) is written to a
temporary directory first and removed afterwards.
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


def write_file(path, n, read_len, seed=1):
    g = _dbg.Graph()
    g.synth_reads(seed, n * 5, n, read_len, 0.01)
    bases, _ = g.copy_reads()
    g.close()
    with open(path, "wb") as fh:
        step = 1 << 20
        for i in range(0, n, step):
            m = min(step, n - i)
            rec = np.empty((m, 3 + read_len + 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            rec[:, 3:3 + read_len] = bases[i * read_len:(i + m) * read_len].reshape(m, read_len)
            rec[:, -1] = 10
            rec.tofile(fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=10e6)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--path", default=None)
    ap.add_argument("--chunks", default="4,16,64", help="MiB, comma separated")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    tmp = None
    path = args.path
    if path is None:
        tmp = tempfile.mkdtemp(prefix="fasta_stream_")
        path = os.path.join(tmp, "reads.fasta")
        write_file(path, int(args.reads), args.read_len)
    try:
        size = os.path.getsize(path)
        np.fromfile(path, dtype=np.uint8)  # warm the page cache
        out = {"file_bytes": size}
        g = _dbg.Graph()

        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            raw = np.fromfile(path, dtype=np.uint8)
            t1 = time.perf_counter()
            g.set_reads_fasta(raw)
            t2 = time.perf_counter()
            del raw
            if best is None or t2 - t0 < best[0]:
                best = (t2 - t0, t1 - t0, g.ingest_stats())
        want = (g.sizes()["n_reads"], g.reads_checksum())
        out["one_shot"] = {"ms": round(best[0] * 1e3, 1), "fromfile_ms": round(best[1] * 1e3, 1),
                           "h2d_ms": round(best[2]["ms_h2d"], 1),
                           "h2d_GB_per_s": round(size / best[2]["ms_h2d"] / 1e6, 1) if best[2]["ms_h2d"] else None,
                           "peak_device_bytes": best[2]["peak_device_bytes"],
                           "peak_over_file": round(best[2]["peak_device_bytes"] / size, 3)}

        out["streamed"] = {}
        for mib in [int(c) for c in args.chunks.split(",") if c]:
            best = None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                g.set_reads_fasta_file(path, chunk_bytes=mib << 20)
                dt = time.perf_counter() - t0
                if best is None or dt < best[0]:
                    best = (dt, g.ingest_stats())
            st = best[1]
            same = (g.sizes()["n_reads"], g.reads_checksum()) == want
            n = st["n_reads"]
            out["streamed"][f"{mib}MiB"] = {
                "ms": round(best[0] * 1e3, 1), "chunks": st["chunks"], "io_wait_ms": round(st["ms_io_wait"], 1),
                "h2d_ms": round(st["ms_h2d"], 1), "h2d_GB_per_s": round(st["bytes_read"] / st["ms_h2d"] / 1e6, 1) if st["ms_h2d"] else None,
                "parse_ms": round(st["ms_parse"], 1), "peak_device_bytes": st["peak_device_bytes"],
                "peak_over_file": round(st["peak_device_bytes"] / size, 3),
                "bound_bytes": size + 64 + 12 * (n + 1) + 4 * (mib << 20) + (1 << 20), "same_reads": bool(same)}
        g.close()
        print(json.dumps(out), flush=True)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
