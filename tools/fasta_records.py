#!/usr/bin/env python3
"""Record-mode FASTA ingest against line mode, and wrapped against unwrapped contig output (GPU box).

Input: the configs[1]-shaped image, N x 150 bp records (10 M: 1.54 GB), written twice to a temporary directory: one line
per read (">r\\n<read>\\n") and wrapped at 60 columns (three lines per read).  Every figure is the best of --reps runs with the
page cache warm, and every run is logged.  Steps:

  line     dbg_set_reads_fasta_file of the unwrapped file (16 MiB chunks): the yardstick of record mode
  record   dbg_set_reads_fasta_records_file of the same file: the same reads (checksum, count)
  wrapped  dbg_set_reads_fasta_records_file of the wrapped file: the same reads again; the host's search for the owned
           bytes shown apart (scan_bytes, and the time of a call on a one-byte range inside the file, which is the two
           searches and the call's fixed costs and nothing else), and the second half of the file as a range
  write    write_contigs_fasta of one contig list (the first 1 M reads, k = 31, threshold 2, non-final, index-only walk,
           the driver's order) to a tmpfs path, unwrapped and at line_width 60

With --pkg DIR the package and library of another checkout -- the parent commit, built -- run the one step they have
(line).  usage: fasta_records.py [--reads 10e6] [--reps 5] [--steps line,record,wrapped,write] [--pkg DIR]
Every result is one JSON line on stdout."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_LEN, WIDTH, K, THRESHOLD = 150, 60, 31, 2
MIB = 1 << 20


def out(**kw):
    print(json.dumps(kw), flush=True)


def write_files(np, _dbg, flat, wrapped, n):
    g = _dbg.Graph()
    g.synth_reads(1, n * 5, n, READ_LEN, 0.01)
    bases, _ = g.copy_reads()
    g.close()
    cuts = list(range(0, READ_LEN, WIDTH)) + [READ_LEN]
    with open(flat, "wb") as fa, open(wrapped, "wb") as fw:
        step = 1 << 20
        for i in range(0, n, step):
            m = min(step, n - i)
            rows = bases[i * READ_LEN:(i + m) * READ_LEN].reshape(m, READ_LEN)
            rec = np.empty((m, 3 + READ_LEN + 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            rec[:, 3:3 + READ_LEN] = rows
            rec[:, -1] = 10
            rec.tofile(fa)
            rec = np.empty((m, 3 + READ_LEN + len(cuts) - 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            at = 3
            for a, b in zip(cuts[:-1], cuts[1:]):
                rec[:, at:at + b - a] = rows[:, a:b]
                rec[:, at + b - a] = 10
                at += b - a + 1
            rec.tofile(fw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=10e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", default="line,record,wrapped,write")
    ap.add_argument("--pkg", default=None, help="root of another checkout whose package and library run instead")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.pkg or ROOT, "py-debruijn_amd"))
    import numpy as np
    import _dbg
    label = "parent" if args.pkg else "this"
    steps = [s for s in args.steps.split(",") if s]
    if args.pkg:
        steps = [s for s in steps if s == "line"]
    n = int(args.reads)
    tmp = tempfile.mkdtemp(prefix="fasta_records_")
    flat, wrapped = os.path.join(tmp, "reads.fasta"), os.path.join(tmp, "reads_wrapped.fasta")
    try:
        g = _dbg.Graph()
        want = None
        if set(steps) & {"line", "record", "wrapped"}:
            write_files(np, _dbg, flat, wrapped, n)
            for p in (flat, wrapped):
                np.fromfile(p, dtype=np.uint8)  # warm the page cache
            out(step="files", pkg=label, reads=n, flat_bytes=os.path.getsize(flat), wrapped_bytes=os.path.getsize(wrapped))

        def ingest(step, call, **extra):
            nonlocal want
            runs, best = [], None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                dt = time.perf_counter() - t0
                runs.append(round(dt * 1e3, 1))
                if best is None or dt < best[0]:
                    best = (dt, g.ingest_stats(), g.fasta_records_stats() if hasattr(g, "fasta_records_stats") and extra.get("rec") else None)
            got = (g.sizes()["n_reads"], g.reads_checksum())
            if want is None:
                want = got
            st, rs = best[1], best[2]
            row = dict(step=step, pkg=label, ms=round(best[0] * 1e3, 1), runs_ms=runs, spread_ms=round(max(runs) - min(runs), 1),
                       chunks=st["chunks"], io_wait_ms=round(st["ms_io_wait"], 1), h2d_ms=round(st["ms_h2d"], 1),
                       parse_ms=round(st["ms_parse"], 1), total_ms=round(st["ms_total"], 1), n_reads=st["n_reads"],
                       peak_device_bytes=st["peak_device_bytes"])
            if extra.get("same", True):
                row["same_reads"] = bool(got == want)
            if rs is not None:
                row.update(scan_bytes=rs["scan_bytes"], n_sequence_lines=rs["n_sequence_lines"], longest_record=rs["longest_record"])
            out(**row)

        if "line" in steps:
            ingest("line", lambda: g.set_reads_fasta_file(flat, chunk_bytes=16 * MIB))
        if "record" in steps:
            ingest("record", lambda: g.set_reads_fasta_records_file(flat, chunk_bytes=16 * MIB), rec=True)
        if "wrapped" in steps:
            ingest("wrapped", lambda: g.set_reads_fasta_records_file(wrapped, chunk_bytes=16 * MIB), rec=True)
            size = os.path.getsize(wrapped)
            t0 = time.perf_counter()
            g.set_reads_fasta_records_file(wrapped, size // 2 + 7, size // 2 + 8, 16 * MIB)  # one byte: the search alone
            dt = time.perf_counter() - t0
            out(step="wrapped_search_alone", pkg=label, ms=round(dt * 1e3, 2), stats=g.fasta_records_stats())
            ingest("wrapped_second_half", lambda: g.set_reads_fasta_records_file(wrapped, size // 2 + 7, None, 16 * MIB), rec=True,
                   same=False)
        if "write" in steps:
            g.set_option("walk_jump_min_nodes", 1)
            g.synth_reads(1, 50_000_000, min(n, 1_000_000), READ_LEN, 0.01)
            g.build(K)
            g.refine_edge_order()
            g.prune(THRESHOLD)
            g.remove_tips()
            g.mark_pull_reads()
            g.walk(False, 1)
            sz = g.sizes()
            shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tmp
            path = os.path.join(shm, f"fasta_records_{os.getpid()}.fasta")
            lengths = np.diff(g.export_contig_index()[0].astype(np.int64))
            g.export_contig_text(0, int(lengths[0]))  # the lifting tables are built once per walk: not part of any figure below
            try:
                for width in (0, WIDTH, 0, WIDTH):
                    runs, nbytes, best = [], 0, None
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        nbytes = g.write_contigs_fasta(path, None, append=False, line_width=width)
                        dt = time.perf_counter() - t0
                        runs.append(round(dt * 1e3, 1))
                        if best is None or dt < best[0]:
                            best = (dt, g.contig_output_stats())
                    out(step="write", pkg=label, line_width=width, contigs=sz["n_contigs"], longest=int(lengths.max()), bytes=nbytes, ms=round(best[0] * 1e3, 1),
                        runs_ms=runs, fill_ms=round(best[1]["ms_fill"], 1), d2h_ms=round(best[1]["ms_d2h"], 1),
                        io_wait_ms=round(best[1]["ms_io_wait"], 1), gb_per_s=round(nbytes / best[0] / 1e9, 3))
            finally:
                if os.path.exists(path):
                    os.unlink(path)
        g.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
