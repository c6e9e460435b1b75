#!/usr/bin/env python3
"""Time of the whole-graph statistics (dbg_count_spectrum) on the configs[1] reads (GPU box): N x 150 bp
synthetic reads made on the device at 30x coverage, 10 M reads by default.

For every case -- k = 31 with 1 % errors, k = 31 error-free, k = 63 with 1 % errors, k = 31 with 1 % errors built in 4 parts:
  spectrum  count_spectrum(256) with each way of relieving the hot bins (option "spectrum_variant" 0 plain LDS atomics,
            1 one sub-histogram per wave, 2 equal bins of a wave combined by ballots until every lane is served, 3 one such
            round for the first lane's bin, plain atomics for the rest): the call's own ms_kernel (events around
            the memset of the bins and the kernels) and the host clock around the call, best of --reps, all of them listed
  copy      a device-to-device copy, through torch, of exactly the bytes the kernel reads (4 B of row pointer per node +
            4 B per edge): the yardstick of this project's streaming kernels, by events
  export    the only route without the call: export_csr() (export_part() per part) + np.bincount over the counts, host
            clock, once; its bins must equal the call's.  On a single graph the export runs ensure_dense(); the spectrum is
            then timed once more (it reads the 64-bit row pointers from there on)
One JSON line per case on stdout.

    python tools/spectrum.py [--reads 10e6] [--reps 5] [--bins 256] [--cases k31,k31_clean,k63,k31_parts] [--no-export]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-debruijn_amd"))
import _dbg  # noqa: E402

L = 150
CASES = {"k31": (31, 0.01, 0), "k31_clean": (31, 0.0, 0), "k63": (63, 0.01, 0), "k31_parts": (31, 0.01, 4)}
VARIANTS = {0: "lds_atomics", 1: "per_wave", 2: "wave_combined", 3: "leader_combined"}


def timed(g, bins, reps):
    kernel, host, sp = [], [], None
    for _ in range(reps):
        t = time.perf_counter()
        sp = g.count_spectrum(bins)
        host.append(round((time.perf_counter() - t) * 1e3, 3))
        kernel.append(round(sp["ms_kernel"], 4))
    return kernel, host, sp


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=10e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-export", action="store_true")
    args = ap.parse_args()
    n, B = int(args.reads), args.bins
    for case in args.cases.split(","):
        k, err, passes = CASES[case]
        g = _dbg.Graph()
        g.synth_reads(1, n * L // 30, n, L, err)
        if passes:
            g.build_multipass(k, passes)
        else:
            g.build(k)
        res = {"tool": "spectrum", "case": case, "reads": n, "read_len": L, "k": k, "err": err, "passes": passes, "bins": B,
               "reps": args.reps}
        sp = None
        for v, name in VARIANTS.items():
            g.set_option("spectrum_variant", v)
            kernel, host, now = timed(g, B, args.reps)
            res[name + "_kernel_ms"], res[name + "_host_ms"] = kernel, host
            res[name + "_kernel_best_ms"] = min(kernel)
            if sp is not None:
                assert all(np.array_equal(sp[f], now[f]) for f in ("edge_hist", "node_hist", "D")), "the variants disagree"
            sp = now
        res.update({f: int(sp[f]) for f in ("n_nodes", "n_edges", "sum_edge_counts", "max_edge_count", "max_out_weight",
                                            "peak_extra_device_bytes")})
        res["D"] = [int(x) for x in sp["D"][:5]]
        res["edge_hist_head"] = [int(x) for x in sp["edge_hist"][:8]]
        res["edge_hist_peak_bin"] = int(np.argmax(sp["edge_hist"][2:]) + 2)
        # the yardstick: a copy of the bytes the kernel reads
        read_bytes = 4 * res["n_nodes"] + 4 * res["n_edges"]
        src = torch.empty(read_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copies = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src, non_blocking=True)
            b.record()
            torch.cuda.synchronize()
            copies.append(round(a.elapsed_time(b), 4))
        del src, dst
        torch.cuda.empty_cache()
        res["read_bytes"], res["copy_event_ms"], res["copy_event_best_ms"] = read_bytes, copies, min(copies)
        for name in VARIANTS.values():
            res[name + "_over_copy"] = round(res[name + "_kernel_best_ms"] / res["copy_event_best_ms"], 2)
        if not args.no_export:
            t = time.perf_counter()
            if passes:
                hist = np.zeros(B, dtype=np.int64)
                for p in range(passes):
                    hist += np.bincount(np.minimum(g.export_part(p)["cnt"], B - 1), minlength=B)
            else:
                _, _, cnt = g.export_csr()
                hist = np.bincount(np.minimum(cnt, B - 1), minlength=B)
                del cnt
            res["export_bincount_host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            assert np.array_equal(hist.astype(np.uint64), sp["edge_hist"]), "export + bincount disagrees with the device"
            if not passes:  # dense now: the same call reads the 64-bit row pointers
                g.set_option("spectrum_variant", 3)
                kernel, host, now = timed(g, B, args.reps)
                assert np.array_equal(now["edge_hist"], sp["edge_hist"]) and np.array_equal(now["node_hist"], sp["node_hist"])
                res["leader_combined_after_dense_kernel_ms"] = kernel
            res["export_over_kernel"] = round(res["export_bincount_host_ms"] / min(res[v + "_kernel_best_ms"] for v in VARIANTS.values()), 0)
        g.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
