"""ctypes loader for the oracle's C restatement (oracle/dbg_oracle.c) -- test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "_build", "liborc.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            subprocess.check_call(["make", "-s", "-C", _HERE])
        l = C.CDLL(_LIB)
        l.orc_build.restype = C.c_void_p
        l.orc_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        l.orc_free.argtypes = [C.c_void_p]
        for n in ("orc_n_nodes", "orc_n_kmer_instances", "orc_n_edge_instances"):
            getattr(l, n).restype = C.c_uint64
            getattr(l, n).argtypes = [C.c_void_p]
        l.orc_export2.restype = C.c_int
        l.orc_export2.argtypes = [C.c_void_p] * 5
        l.orc_build_mt.restype = C.c_int
        l.orc_build_mt.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]
        l.orc_build_mt_partitioned.restype = C.c_int
        l.orc_build_mt_partitioned.argtypes = l.orc_build_mt.argtypes
        l.orc_traverse.restype = C.c_int
        l.orc_traverse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_int, C.c_uint64, C.c_void_p]
        for n in ("orc_trav_nodes", "orc_trav_lists"):
            getattr(l, n).restype = C.c_int
            getattr(l, n).argtypes = [C.c_void_p] * 4
        l.orc_trav_contigs.restype = C.c_int
        l.orc_trav_contigs.argtypes = [C.c_void_p] * 5
        l.orc_index.restype = C.c_int
        l.orc_index.argtypes = [C.c_void_p]
        l.orc_export_range.restype = C.c_int
        l.orc_export_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
        l.orc_trav_spell.restype = C.c_int
        l.orc_trav_spell.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def build(bases, offsets, k, export=True):
    """Returns dict(keys, keys_hi, stamps, counts, n_nodes, n_kmer_instances, n_edge_instances); dict order.

    A k-mer is the 2k-bit number keys_hi * 2**64 + keys (keys_hi is zero for k <= 32)."""
    l = lib()
    b = np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases)
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    h = l.orc_build(b.ctypes.data, o.ctypes.data, o.size - 1, k)
    if not h:
        raise ValueError("orc_build failed (k outside 1..63, non-ACGT byte, or out of memory)")
    try:
        n = l.orc_n_nodes(h)
        out = {"n_nodes": n, "n_kmer_instances": l.orc_n_kmer_instances(h),
               "n_edge_instances": l.orc_n_edge_instances(h)}
        if export:
            keys = np.empty(n, dtype=np.uint64)
            keys_hi = np.empty(n, dtype=np.uint64)
            stamps = np.empty(n, dtype=np.uint64)
            counts = np.empty((n, 4), dtype=np.uint32)
            assert l.orc_export2(h, keys.ctypes.data, keys_hi.ctypes.data, stamps.ctypes.data, counts.ctypes.data) == 0
            out.update(keys=keys, keys_hi=keys_hi, stamps=stamps, counts=counts)
        return out
    finally:
        l.orc_free(h)


def _as_u8(bases):
    return np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases)


class Oracle:
    """One orc_build kept open, so that orc_traverse can run on it several times (thresholds, final and non-final).

    Node indices are positions in dict order (the rows of nodes()).  Holds the reads it was built from."""

    def __init__(self, bases, offsets, k):
        self._l = lib()
        self.bases = _as_u8(bases).reshape(-1)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.k = int(k)
        self._h = self._l.orc_build(self.bases.ctypes.data, self.offsets.ctypes.data, self.offsets.size - 1, self.k)
        if not self._h:
            raise ValueError("orc_build failed (k outside 1..63, non-ACGT byte, or out of memory)")
        self.n_nodes = int(self._l.orc_n_nodes(self._h))

    def close(self):
        if self._h:
            self._l.orc_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def nodes(self, lo=0, hi=None):
        """(keys, keys_hi, stamps, counts[n, 4]) of the nodes [lo, hi) in dict order, as build() exports them (a slice
        costs no more host memory than its own arrays)."""
        hi = self.n_nodes if hi is None else min(int(hi), self.n_nodes)
        n = max(0, hi - lo)
        keys, khi, st = (np.empty(n, dtype=np.uint64) for _ in range(3))
        cnt = np.empty((n, 4), dtype=np.uint32)
        if self._l.orc_index(self._h):
            raise MemoryError("orc_index")
        assert self._l.orc_export_range(self._h, lo, lo + n, keys.ctypes.data, khi.ctypes.data, st.ctypes.data,
                                        cnt.ctypes.data) == 0
        return keys, khi, st, cnt

    def traverse(self, threshold, final=False, max_paths=10**7):
        """pruningEdges, branch list, tip removal, pull-out reads and the walk (orc_traverse).  Returns a dict:
        order / keep / flags (uint8 per node: successor codes by rank 2 bits each, kept codes as bits, 1 branch |
        2 pulled), branch / pulled (node indices: dict order / pull order), read_flags (uint8 per read), and the contig
        index in emission order: stamp (of the start node), seq (index within the start), chars, score.
        The final walk raises OverflowError past max_paths emitted paths or 64 * max_paths + 2**20 DFS steps."""
        l, n = self._l, self.n_nodes
        sz = np.zeros(6, dtype=np.uint64)
        rc = l.orc_traverse(self._h, self.bases.ctypes.data, self.offsets.ctypes.data, self.offsets.size - 1,
                            float(threshold), 1 if final else 0, int(max_paths), sz.ctypes.data)
        if rc == -2:
            raise OverflowError(f"final walk passed its cap of {max_paths} paths")
        if rc == -5:
            raise OverflowError(f"final walk passed its cap of {64 * int(max_paths) + (1 << 20)} DFS steps "
                                f"(64 * max_paths + 2**20)")
        if rc:
            raise RuntimeError(f"orc_traverse failed ({rc})")
        nb, npu, _, nc = (int(x) for x in sz[:4])
        order, keep, flags = (np.empty(n, dtype=np.uint8) for _ in range(3))
        assert l.orc_trav_nodes(self._h, order.ctypes.data, keep.ctypes.data, flags.ctypes.data) == 0
        branch, pulled = np.empty(nb, dtype=np.uint32), np.empty(npu, dtype=np.uint32)
        rf = np.empty(self.offsets.size - 1, dtype=np.uint8)
        assert l.orc_trav_lists(self._h, branch.ctypes.data, pulled.ctypes.data, rf.ctypes.data) == 0
        stamp, chars, score = (np.empty(nc, dtype=np.uint64) for _ in range(3))
        seq = np.empty(nc, dtype=np.uint32)
        assert l.orc_trav_contigs(self._h, stamp.ctypes.data, seq.ctypes.data, chars.ctypes.data, score.ctypes.data) == 0
        return {"order": order, "keep": keep, "flags": flags, "branch": branch, "pulled": pulled, "read_flags": rf,
                "stamp": stamp, "seq": seq, "chars": chars, "score": score, "n_pull_reads": int(sz[2]),
                "contig_chars": int(sz[4])}

    def spell(self, idx):
        """Texts of the last traversal's contigs idx (emission-order indices) -> (uint8 chars, uint64 offsets[len + 1])."""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        off = np.empty(idx.size + 1, dtype=np.uint64)
        assert self._l.orc_trav_spell(self._h, idx.ctypes.data, idx.size, None, off.ctypes.data) == 0
        buf = np.empty(int(off[-1]), dtype=np.uint8)
        assert self._l.orc_trav_spell(self._h, idx.ctypes.data, idx.size, buf.ctypes.data, off.ctypes.data) == 0
        return buf, off


def labels(keys, keys_hi, k, alphabet="ACTG"):
    """k-mer strings of exported keys (first base in the top bit pair)."""
    out = []
    for lo, hi in zip(keys.tolist(), keys_hi.tolist()):
        v = (int(hi) << 64) | int(lo)
        out.append("".join(alphabet[(v >> (2 * (k - 1 - i))) & 3] for i in range(k)))
    return out


M64 = (1 << 64) - 1


def _mix64(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def digest(keys, stamps, counts):
    """The node digest orc_build_mt returns, from exported arrays (numpy; wraps modulo 2**64)."""
    with np.errstate(over="ignore"):
        c = counts.astype(np.uint64)
        w = c[:, 0] + np.uint64(3) * c[:, 1] + np.uint64(5) * c[:, 2] + np.uint64(7) * c[:, 3] + np.uint64(1)
        return int(_mix64(keys ^ _mix64(stamps) ^ _mix64(w)).sum(dtype=np.uint64))


def build_mt(bases, offsets, k, n_threads, partition_once=False):
    """Multi-threaded build (k <= 31): totals and the node digest only -- bench.py's cpu_baseline on all host cores.
    partition_once: orc_build_mt_partitioned (every window is rolled and hashed by ONE thread and handed to the owner of its
    hash slice; 16 bytes per k-mer instance between the phases) instead of orc_build_mt (every thread scans everything)."""
    l = lib()
    b = np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases)
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.zeros(5, dtype=np.uint64)
    fn = l.orc_build_mt_partitioned if partition_once else l.orc_build_mt
    rc = fn(b.ctypes.data, o.ctypes.data, o.size - 1, int(k), int(n_threads), out.ctypes.data)
    if rc:
        raise ValueError(f"orc_build_mt failed ({rc})")
    return {"n_nodes": int(out[0]), "n_edges": int(out[1]), "n_kmer_instances": int(out[2]),
            "n_edge_instances": int(out[3]), "digest": int(out[4])}
