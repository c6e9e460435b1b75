"""Traversal of a graph that lives in PARTS -- a multi-pass build on one GPU (BASELINE.json configs[3]), the ranks of a
sharded build (configs[2], [4]), or ranks x passes -- without any GPU ever holding the whole graph:

    pruningEdges + branch list          debruijn.py:150-166, :230-236     per part (dbg_part_prune)
    tip removal                         debruijn.py:169-186, :241-254     the <= 5-step neighbourhoods of the branch nodes are
                                                                          collected from all parts; every rank runs the library's
                                                                          reservation kernels on that small graph
    pull-out reads + Counter order      debruijn.py:274-278, :159-165     every rank streams ITS reads against the branch k-mers of
                                                                          the whole graph (dbg_scan_reads_for_keys)
    contig walk (non-final)             debruijn.py:288-347               chains leave a part at almost every change of minimizer:
                                                                          one short segment per entry node inside each part
                                                                          (dbg_part_segments), then the skeleton of segments --
                                                                          a few per cent of the nodes -- is ranked by pointer jumping

A node is (virtual shard v, local id); v = rank * n_passes + part, global id = v << 32 | local.  The heavy per-node work
is in the library (include/dbg.h "traversal of a graph in parts"); this module moves the small id lists and rows between
parts and ranks (``torch.distributed`` all-to-all, or nothing at all on one process) and sorts / joins them with torch
and numpy.  The result equals the reference's on the whole read set: ``branch_kmer`` (dict order), ``already_pull_out``
(append order), the pull-out reads of every rank, and the contig index (start stamp, length, score) in dict order.
threshold >= 1 (below 1 the kept successor itself depends on the Counter order).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import _dbg
import multi_gpu

F_INDEG, F_KEEP_MASK, F_KEEP_SHIFT, F_BRANCH, F_PULLED, PF_MARK = 0x01, 0x1E, 1, 0x20, 0x40, 0x80
NO_NODE = 0xFFFFFFFF
TIP_REACH = 5  # debruijn.py:246: the DFS enters nodes up to 4 steps from the branch node and looks at the flags of the fifth
K_EMIT, K_PULLED, K_REMOTE, K_CYCLE, K_NEXT_PULLED = 0, 1, 2, 3, 4


def _u32(t):
    """int32 tensor holding uint32 values -> int64"""
    return t.to(torch.int64) & 0xFFFFFFFF


def rank_skeleton(e, k, keep=False):
    """The skeleton of segments -> the contig index.  ``e``: dict of equally long int64 tensors, one row per entry node:
    gid (global id), kind (K_*), next (global id of the entry a REMOTE segment hands over to), hops, score, exit (count of the
    leaving edge), stamp, start (1: indegree 0).  Entering a pulled node ends the path at the previous one (debruijn.py:
    292-302); a chain that meets a cycle inside a part (K_CYCLE) or across parts (never resolves) emits nothing (:289-290), nor
    does a start that is itself pulled.  -> (dict(stamp, length, score) numpy in dict order of the starts, skeleton or None).
    The skeleton (``keep``) stays where ``e`` lives: the columns sorted by gid -- gid, next (row index), go_on, hops -- and
    rest, the characters the chain appends from the entry's segment to its end: hops + go_on * (1 + rest[next]), -1 (the
    library's UINT64_MAX) where the chain is dead or never resolved; emit (numpy): the row of contig i's start.  For the
    final-mode walk it also carries, per row: terminal (the row the chain ends in, valid where rest is), chain_score (the
    edge counts along the chain), and the sorted input columns kind, exit, stamp and start."""
    n = e["gid"].numel()
    if n == 0:
        z = np.empty(0, dtype=np.int64)
        zt = e["gid"].reshape(-1)
        sk = {"gid": zt, "next": zt, "go_on": zt.to(torch.bool), "hops": zt, "rest": zt, "emit": z, "terminal": zt, "chain_score": zt,
              "kind": zt, "exit": zt, "stamp": zt, "start": zt} if keep else None
        return {"stamp": z.astype(np.uint64), "length": z, "score": z}, sk
    o = torch.argsort(e["gid"])
    e = {c: t[o] for c, t in e.items()}
    remote = e["kind"] == K_REMOTE
    want = torch.where(remote, e["next"], e["gid"])
    j = torch.searchsorted(e["gid"], want).clamp_(max=n - 1)
    assert bool((e["gid"][j] == want).all()), "a chain continues at a node that is no entry"
    go_on = remote & (e["kind"][j] != K_PULLED)     # entering a pulled node ends the path at the previous one
    sk = {"gid": e["gid"].contiguous(), "next": j.contiguous(), "go_on": go_on.contiguous(), "hops": e["hops"].contiguous()} if keep else None
    hops = e["hops"] + go_on.to(torch.int64)
    score = e["score"] + torch.where(go_on, e["exit"], torch.zeros_like(e["exit"]))
    dead = e["kind"] == K_CYCLE
    done = ~go_on
    jump = torch.where(go_on, j, torch.arange(n, device=e["gid"].device))
    # pointer jumping over the entries that are not resolved yet (the list shrinks fast: most chains are a few segments);
    # a round reads the old values of its targets before anything is written
    act = torch.nonzero(~done).reshape(-1)
    for _ in range(max(1, math.ceil(math.log2(n + 1))) + 1):
        if act.numel() == 0:
            break
        tj = jump[act]
        h2, s2, d2, dn, j2 = hops[act] + hops[tj], score[act] + score[tj], dead[act] | dead[tj], done[tj], jump[tj]
        hops[act], score[act], dead[act], done[act], jump[act] = h2, s2, d2, dn, j2
        act = act[~dn]
    emit = (e["start"] == 1) & (e["kind"] != K_PULLED) & done & ~dead   # not done after log2(n) doublings: a cycle across parts
    em = torch.nonzero(emit).reshape(-1)
    em = em[torch.argsort(e["stamp"][em])]           # dict order of the starts (stamps are distinct), sorted on the device
    if keep:
        sk["rest"] = torch.where(done & ~dead, hops, torch.full_like(hops, -1))   # the jumping left the chain's sum in hops
        sk["emit"] = em.cpu().numpy()                # skeleton index of contig i's start
        sk.update(terminal=jump, chain_score=score, kind=e["kind"], exit=e["exit"], stamp=e["stamp"], start=e["start"])
    return {"stamp": e["stamp"][em].cpu().numpy().astype(np.uint64), "length": (hops[em] + k).cpu().numpy(),
            "score": score[em].cpu().numpy()}, sk


class _Net:
    """How rows reach the rank that owns them: torch.distributed, or a single process (dist None)."""

    def __init__(self, dist, device):
        self.dist, self.device = dist, device
        self.world = dist.get_world_size() if dist is not None else 1
        self.rank = dist.get_rank() if dist is not None else 0

    def route(self, dest_rank, *cols):
        """Rows (parallel 1-D tensors) to the rank dest_rank[i]; returns the received columns."""
        return self.route_there(dest_rank, *cols)[0]

    def route_there(self, dest_rank, *cols):
        """route() that also returns what the return leg needs: -> (received columns, plan)."""
        if self.world == 1:
            return cols, None
        order = torch.argsort(dest_rank, stable=True)
        send = torch.bincount(dest_rank, minlength=self.world).tolist()
        recv = multi_gpu.exchange_counts(self.dist, send, self.device)
        got = tuple(multi_gpu.alltoallv(self.dist, c[order].contiguous(), send, recv) for c in cols)
        return got, (order, send, recv)

    def route_back(self, plan, *cols):
        """The return leg of route_there: one answer row per received row (in the order received) back to the rank that sent
        it, in the order of ITS rows -- the same counts swapped, then the inverse of the stable sort."""
        if plan is None:
            return cols
        order, send, recv = plan
        out = []
        for c in cols:
            if c.numel() != sum(recv):
                raise RuntimeError(f"route_back: {c.numel()} answers for {sum(recv)} received rows")
            back = multi_gpu.alltoallv(self.dist, c.contiguous(), recv, send)
            if back.numel() != order.numel():
                raise RuntimeError(f"route_back: {back.numel()} answers came back for {order.numel()} rows sent")
            placed = torch.empty_like(back)
            placed[order] = back
            out.append(placed)
        return tuple(out)

    def gather_all(self, *cols, widths=None):
        """Every rank's rows on every rank (rank order).  widths[i]: elements per row of column i (1 unless given)."""
        if self.world == 1:
            return cols
        widths = widths or [1] * len(cols)
        n = cols[0].numel() // widths[0]
        sizes = [m[0] for m in multi_gpu._all_gather_ints(self.dist, [n], self.device)]
        return tuple(multi_gpu.alltoallv(self.dist, c.reshape(-1).repeat(self.world), [n * w] * self.world, [s * w for s in sizes])
                     for c, w in zip(cols, widths))

    def all_ints(self, vals):
        if self.world == 1:
            return [list(vals)]
        return multi_gpu._all_gather_ints(self.dist, list(vals), self.device)

    def min_u64(self, arr):
        """element-wise minimum over ranks of a numpy uint64 array (values below 2^63 or the all-ones sentinel)"""
        if self.world == 1:
            return arr
        t = torch.from_numpy(arr.view(np.int64).copy())
        t = torch.where(t < 0, torch.full_like(t, (1 << 63) - 1), t)  # the sentinel as the largest int64
        if self.dist.get_backend() == "nccl":
            t = t.to(self.device)
        parts = self.gather_all(t.reshape(-1))[0].reshape(self.world, -1)
        m = parts.min(dim=0).values.cpu().numpy().astype(np.uint64)
        m[m == np.uint64((1 << 63) - 1)] = np.iinfo(np.uint64).max
        return m.reshape(arr.shape)

    def sum_u64(self, arr):
        """element-wise sum over ranks of a numpy uint64 array (the sums stay below 2^63: they are edge-instance counts)"""
        if self.world == 1:
            return arr
        t = torch.from_numpy(arr.view(np.int64).copy())
        if self.dist.get_backend() == "nccl":
            t = t.to(self.device)
        parts = self.gather_all(t.reshape(-1))[0].reshape(self.world, -1)
        return parts.sum(dim=0).cpu().numpy().astype(np.uint64).reshape(arr.shape)


def merge_spectrum(net, sp):
    """Collective.  One rank's ``Graph.count_spectrum`` dict -> the whole graph's, on every rank: bins, degree
    distributions and the three totals are sums over ranks (every node and edge lives on exactly one), the maxima are
    maxima, ``pruned`` says that every rank that holds nodes has pruned them; ``ms_kernel`` and
    ``peak_extra_device_bytes`` are the largest any rank saw."""
    if net.world == 1:
        return sp
    totals = ("n_nodes", "n_edges", "sum_edge_counts")
    mine = [int(sp["n_bins"]), int(sp["n_nodes"]), int(sp["pruned"]), int(sp["max_edge_count"]), int(sp["max_out_weight"]),
            int(sp["peak_extra_device_bytes"]), int(sp["ms_kernel"] * 1e6), int("edge_hist" in sp)]
    seen = net.all_ints(mine)
    if any(s[0] != mine[0] or s[7] != mine[7] for s in seen):
        raise RuntimeError(f"count_spectrum: the ranks asked for different bins: {[list(s) for s in seen]}")
    cols = [sp["D"], sp["K"], np.array([sp[n] for n in totals], dtype=np.uint64)]
    if "edge_hist" in sp:
        cols += [sp["edge_hist"], sp["node_hist"]]
    flat = net.sum_u64(np.concatenate([np.asarray(c, dtype=np.uint64) for c in cols]))
    out = dict(sp)
    out["D"], out["K"] = flat[:33].copy(), flat[33:66].copy()
    for i, n in enumerate(totals):
        out[n] = int(flat[66 + i])
    if "edge_hist" in sp:
        B = mine[0]
        out["edge_hist"], out["node_hist"] = flat[69:69 + B].copy(), flat[69 + B:69 + 2 * B].copy()
    out["max_edge_count"], out["max_out_weight"] = max(s[3] for s in seen), max(s[4] for s in seen)
    out["pruned"] = int(out["n_nodes"] > 0 and all(s[2] for s in seen if s[1]))
    out["peak_extra_device_bytes"] = max(s[5] for s in seen)
    out["ms_kernel"] = max(s[6] for s in seen) / 1e6
    return out


class PartTraversal:
    """The traversal state of one process: its handle ``g`` with ``n_passes`` parts (part p = virtual shard rank * P + p)."""

    def __init__(self, g, k, dist=None):
        self.g, self.k = g, int(k)
        self.P = g.part_count()
        if self.P < 1:
            raise _dbg.DbgError(_dbg.DBG_E_ARG, "part_traversal: the handle holds no graph in parts (build_multipass / sharded_build_multipass first)")
        self.device = torch.device("cuda", g.sizes_device())
        self.net = _Net(dist, self.device)
        self.rank, self.world = self.net.rank, self.net.world
        self.nv = self.world * self.P
        self.n_nodes = [g.part_sizes(p)["n_nodes"] for p in range(self.P)]
        self.final_mode = False   # construct_graph(final=True): output_contigs walks every simple path
        self.final = None         # the pieces of the last walk_final (None: the last walk was a non-final one)

    # ---- helpers
    def _v(self, p):
        return self.rank * self.P + p

    def _to_parts(self, gids):
        """global ids (int64, any rank's) -> list over my parts of int32 local-id tensors, after routing to the owners"""
        v = gids >> 32
        (mine,) = self.net.route(torch.div(v, self.P, rounding_mode="floor"), gids)
        v = (mine >> 32) - self.rank * self.P
        loc = (mine & 0xFFFFFFFF).to(torch.int32)  # wraps to the int32 carrying the uint32
        return [loc[v == p].contiguous() for p in range(self.P)]

    def _rows(self, p, ids):
        r = self.g.part_gather(p, ids)
        n = ids.numel()
        gid = (self._v(p) << 32) | _u32(ids)
        so = r["succ_owner"].to(torch.int64).reshape(n, 4)
        sl = _u32(r["succ_local"]).reshape(n, 4)
        succ_gid = torch.where(so == 0xFF, torch.full_like(sl, -1), (so << 32) | sl)
        return {"gid": gid, "keys": r["keys"], "keys_hi": r["keys_hi"], "stamps": r["stamps"],
                "counts": _u32(r["counts"]).reshape(n, 4), "succ": succ_gid, "pflags": r["pflags"].to(torch.int64)}

    @staticmethod
    def _cat(rows):
        keys = rows[0].keys()
        return {c: torch.cat([r[c] for r in rows]) for c in keys}

    # ---- point queries on the graph in parts (include/dbg.h: dbg_part_lookup_nodes, dbg_part_score_sequences)
    def lookup(self, keys, keys_hi=None):
        """Collective.  Global ids (v << 32 | local, int64; -1 where the k-mer is no node of the whole graph) of THIS rank's
        queries: packed k-mers as numpy uint64 arrays (-> numpy int64) or int64 tensors on the handle's device (-> tensor);
        keys_hi None: zeros.  The kernel names the owner of every key; keys of other ranks travel to rank owner // P, are
        answered there and come back in query order.  One process makes no exchange."""
        as_numpy = isinstance(keys, np.ndarray) or not hasattr(keys, "data_ptr")
        if as_numpy:
            lo = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1).view(np.int64)).to(self.device)
            hi = None if keys_hi is None else \
                torch.from_numpy(np.ascontiguousarray(keys_hi, dtype=np.uint64).reshape(-1).view(np.int64)).to(self.device)
        else:
            lo, hi = keys.reshape(-1), None if keys_hi is None else keys_hi.reshape(-1)
        if hi is not None and hi.numel() != lo.numel():
            raise ValueError("keys and keys_hi differ in length")
        owner, local = self.g.part_lookup_nodes(lo, hi)
        owner, local = owner.to(torch.int64), _u32(local)
        named = owner != 0xFF                       # 0xFF: bits above 2k, no k-mer at all
        if bool((named & (owner >= self.nv)).any()):
            raise RuntimeError(f"lookup: an owner byte names a virtual shard beyond the {self.nv} of this build")
        dest = torch.div(owner, self.P, rounding_mode="floor")
        if self.world > 1:
            far = torch.nonzero(named & (dest != self.rank)).reshape(-1)
            if bool((local[far] != NO_NODE).any()):
                raise RuntimeError("lookup: a local id came back for a key that another rank owns")
            z = torch.zeros(far.numel(), dtype=torch.int64, device=self.device)
            (q_lo, q_hi), plan = self.net.route_there(dest[far], lo[far], z if hi is None else hi[far])
            a_owner, a_local = self.g.part_lookup_nodes(q_lo.contiguous(), q_hi.contiguous())
            a_owner = a_owner.to(torch.int64)
            if bool((torch.div(a_owner, self.P, rounding_mode="floor") != self.rank).any()):
                raise RuntimeError(f"lookup: rank {self.rank} was asked about a key it does not own (the ranks disagree on the owner rule)")
            b_owner, b_local = self.net.route_back(plan, a_owner, _u32(a_local))
            if bool((b_owner != owner[far]).any()):
                raise RuntimeError("lookup: the owner of a key differs between the asking and the answering rank")
            local[far] = b_local
        gid = torch.where(named & (local != NO_NODE), (owner << 32) | local, torch.full_like(local, -1))
        return gid.cpu().numpy() if as_numpy else gid

    def score_sequences(self, chars, offsets):
        """Collective; every rank passes the SAME sequences (chars + offsets[n + 1], as _dbg.Graph.score_sequences takes them).
        -> (scores uint64[n], first_missing uint64[n]) of the whole graph on every rank: the sum over ranks of the partial
        scores and the minimum over ranks of the first missing window."""
        c = np.frombuffer(chars, dtype=np.uint8) if not isinstance(chars, np.ndarray) else chars
        c = np.ascontiguousarray(c, dtype=np.uint8).reshape(-1)
        o = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        mine = [int(o.size) - 1, int(c.size), int(c.sum(dtype=np.uint64)) & ((1 << 63) - 1)]
        seen = self.net.all_ints(mine)
        if any(list(s) != mine for s in seen):
            raise RuntimeError(f"score_sequences: the ranks passed different sequences (n_seq, n_chars, text sum): {seen}")
        scores, miss = self.g.part_score_sequences(c, o)
        if scores.size == 0:
            return scores, miss
        return self.net.sum_u64(scores), self.net.min_u64(miss)

    def count_spectrum(self, n_bins=256, hists=True):
        """Collective.  Edge spectrum, out-weight spectrum and degree distributions of the WHOLE graph on every rank
        (include/dbg.h: dbg_count_spectrum): one device call over this handle's parts, then the sum over ranks."""
        return merge_spectrum(self.net, self.g.count_spectrum(n_bins, hists=hists))

    # ---- a5 + a6
    def prune(self, threshold):
        """pruningEdges + branch detection on every part; returns the branch nodes of the WHOLE graph in dict order:
        dict(gid, keys, keys_hi, stamps, counts [n, 4], succ [n, 4] global ids, pflags) as numpy arrays."""
        if not threshold >= 1:
            raise ValueError("traversal in parts takes threshold >= 1")
        self.threshold = float(threshold)
        rows = []
        for p in range(self.P):
            self.g.part_prune(p, threshold)
            ids = self.g.part_select(p, F_BRANCH, F_BRANCH) if self.n_nodes[p] else torch.empty(0, dtype=torch.int32, device=self.device)
            rows.append(self._rows(p, ids))
        mine = self._cat(rows)
        cols = list(mine.keys())
        got = dict(zip(cols, self.net.gather_all(*[mine[c].reshape(-1) for c in cols], widths=[4 if c in ("counts", "succ") else 1 for c in cols])))
        n = got["gid"].numel()
        got["counts"], got["succ"] = got["counts"].reshape(n, 4), got["succ"].reshape(n, 4)
        o = torch.argsort(got["stamps"])   # dict order = ascending first-occurrence stamp (distinct, below 2^63); sorted on the device
        self.branch = {c: t[o].cpu().numpy() for c, t in got.items()}
        return self.branch

    # ---- a9 + the Counter order of the branch nodes' successors
    def pull_out_reads(self):
        """-> uint8 flags over THIS rank's reads: 1 where the read holds a branch k-mer of the whole graph (debruijn.py:274-278).
        Also fills ``branch_order``: per branch node the successor codes by (count descending, first appearance) --
        Counter.most_common order, debruijn.py:159-165 -- needed by the tip removal."""
        b = self.branch
        keys = b["keys"].astype(np.uint64)
        hi = b["keys_hi"].astype(np.uint64)
        flags, seen = self.g.scan_reads_for_keys(self.k, keys, hi if self.k > 32 else None, first_seen=True)
        sizes = self.net.all_ints([self.g.sizes()["n_bytes"]])
        base = sum(s[0] for s in sizes[:self.rank])
        if seen.size:
            present = seen != np.iinfo(np.uint64).max
            seen = np.where(present, seen + np.uint64(base), seen)
            seen = self.net.min_u64(seen)
        self.first_seen = seen
        self.read_flags = flags
        return flags

    def _order_bytes(self, counts, first_seen):
        """rank bytes (dbg_export_orders layout: code at rank r in bits 2r+1:2r) by (count desc, first appearance asc, code)."""
        n = counts.shape[0]
        order = np.zeros(n, dtype=np.uint8)
        if not n:
            return order
        c = counts.astype(np.int64)
        fs = first_seen.astype(np.float64)  # only compared among present successors; 2^64 - 1 sorts last
        idx = np.lexsort((np.tile(np.arange(4), (n, 1)), fs, -c), axis=1)  # per row: codes sorted by (-count, first seen, code)
        for r in range(4):
            order |= (idx[:, r].astype(np.uint8) << np.uint8(2 * r))
        return order

    # ---- a7
    def remove_tips(self):
        """Tip removal on the neighbourhoods of the branch nodes; marks the pulled nodes in their parts and returns
        ``already_pull_out`` as dict(gid, keys, keys_hi) in append order (numpy)."""
        g, P = self.g, self.P
        for p in range(P):
            g.part_clear(p, PF_MARK)
        # breadth-first over kept edges from the branch nodes: TIP_REACH rounds, the last round's nodes are only looked at
        frontier = [g.part_select(p, F_BRANCH, F_BRANCH) if self.n_nodes[p] else torch.empty(0, dtype=torch.int32, device=self.device)
                    for p in range(P)]
        for p in range(P):
            g.part_mark(p, frontier[p], PF_MARK)
        rows, dist_of = [], []
        for depth in range(TIP_REACH + 1):
            out_gids = []
            for p in range(P):
                r = self._rows(p, frontier[p])
                rows.append(r)
                dist_of.append(torch.full((frontier[p].numel(),), depth, dtype=torch.int64, device=self.device))
                if depth < TIP_REACH:
                    keep = (r["pflags"][:, None] >> (F_KEEP_SHIFT + torch.arange(4, device=self.device)[None, :])) & 1
                    out_gids.append(r["succ"][(keep == 1) & (r["succ"] >= 0)])
            if depth == TIP_REACH:
                break
            nxt = self._to_parts(torch.cat(out_gids) if out_gids else torch.empty(0, dtype=torch.int64, device=self.device))
            frontier = []
            for p in range(P):
                ids = torch.unique(nxt[p])
                new = g.part_mark(p, ids, PF_MARK, newly=True)
                frontier.append(ids[new == 1].contiguous())
        mine = self._cat(rows)
        mine["dist"] = torch.cat(dist_of)
        cols = list(mine.keys())
        got = dict(zip(cols, self.net.gather_all(*[mine[c].reshape(-1) for c in cols], widths=[4 if c in ("counts", "succ") else 1 for c in cols])))
        n = got["gid"].numel()
        got["counts"], got["succ"] = got["counts"].reshape(n, 4), got["succ"].reshape(n, 4)
        o = torch.argsort(got["gid"])                      # sorted by global id on the device: the join below is a binary search
        got = {c: t[o] for c, t in got.items()}
        pos_t = torch.searchsorted(got["gid"], torch.where(got["succ"] >= 0, got["succ"], torch.zeros_like(got["succ"]))).clamp_(max=max(n - 1, 0))
        pulled_gid = np.empty(0, dtype=np.int64)
        if n:
            # the mini-graph stays on the device: masked counts, successors as positions in the sorted list, rank bytes
            dev = self.device
            ar4 = torch.arange(4, device=dev)
            keep = ((got["pflags"][:, None] >> (F_KEEP_SHIFT + ar4[None, :])) & 1) == 1
            full = (got["dist"] < TIP_REACH)[:, None]
            counts = torch.where(keep & full, got["counts"], torch.zeros_like(got["counts"]))  # pruned edges and the outermost ring: no successors
            found = (got["gid"][pos_t] == got["succ"]) & (counts != 0)
            dup = (got["gid"][1:] == got["gid"][:-1]).any() if n > 1 else torch.zeros((), dtype=torch.bool, device=dev)
            ok = torch.stack([~dup, (found == (counts != 0)).all()]).cpu().tolist()   # one host sync for both checks
            assert ok[0], "a node was collected twice"
            assert ok[1], "a kept successor inside the neighbourhood was not collected"
            succ = torch.where(found, pos_t, torch.full_like(pos_t, -1))
            # Counter order: exact for the branch nodes (the only nodes whose successor order the DFS can see);
            # any permutation serves a node with at most one kept successor
            order = torch.full((n,), 0xE4, dtype=torch.uint8, device=dev)
            b = self.branch
            if b["gid"].size:
                bpos = torch.searchsorted(got["gid"], torch.from_numpy(b["gid"].astype(np.int64)).to(dev))
                order[bpos] = torch.from_numpy(self._order_bytes(counts[bpos].cpu().numpy(), self.first_seen)).to(dev)
            helper = _dbg.Graph(device=g.sizes_device())
            try:
                helper.set_reads(np.frombuffer(b"A", dtype=np.uint8), np.array([0, 1], dtype=np.uint64))  # import wants a read set
                tc = counts.to(torch.int32).reshape(-1).contiguous()     # (the uint32 counts in int32 / int64 clothes)
                tsu = succ.to(torch.int32).reshape(-1).contiguous()      # -1 = NO_NODE
                helper.import_graph(self.k, [n], got["keys"].contiguous(), got["stamps"].contiguous(), tc, tsu,
                                    got["keys_hi"].contiguous() if self.k > 31 else None)
                helper.set_orders(order.cpu().numpy())
                helper.prune(self.threshold)
                helper.remove_tips()
                _, _, _, hflags = helper.export_nodes(keys=False, stamps=False, counts=False)
                hr = helper.export_pull_ranks()
                self.tip_rounds = helper.sizes()["tip_rounds"]
            finally:
                helper.close()
            sel = np.nonzero(hflags & F_PULLED)[0]
            sel = sel[np.argsort(hr[sel], kind="stable")]
            st = torch.from_numpy(sel.astype(np.int64)).to(dev)
            pulled_gid = got["gid"][st].cpu().numpy()
            self.pulled = {"gid": pulled_gid, "keys": got["keys"][st].cpu().numpy().astype(np.uint64),
                           "keys_hi": got["keys_hi"][st].cpu().numpy().astype(np.uint64)}
        else:
            self.pulled = {"gid": pulled_gid, "keys": np.empty(0, np.uint64), "keys_hi": np.empty(0, np.uint64)}
        # every rank computed the same list: it marks its own nodes
        gt = torch.from_numpy(pulled_gid.astype(np.int64)).to(self.device)
        v = gt >> 32
        for p in range(P):
            ids = (gt[v == self._v(p)] & 0xFFFFFFFF).to(torch.int32).contiguous()
            g.part_mark(p, ids, F_PULLED)
            g.part_clear(p, PF_MARK)
        return self.pulled

    # ---- a11 + a12 + a13, non-final mode
    def walk_index(self, keep_skeleton=False):
        """output_contigs (debruijn.py:326-347) with the branch list of construct_graph: the contig index in dict order of the
        starts -- dict(stamp uint64, length int64, score int64) numpy arrays.  A start whose chain runs into a cycle emits
        nothing (debruijn.py:289-290), nor does a start that was pulled.  keep_skeleton: hand the ranked skeleton to the
        library (dbg_part_set_skeleton: it stays on the device, with its lifting table) so that ``contig_texts`` and
        ``write_contigs_fasta`` can spell contigs afterwards; the host keeps 16 bytes per CONTIG (start row, length)."""
        self.final = None
        index, _ = self._ranked_skeleton(keep_skeleton)
        return index

    def _ranked_skeleton(self, keep_skeleton, extra_entries=None):
        """walk_index's work: entries, one segment each, ranking.  extra_entries: global ids (this rank's own among them are
        used) that are entries besides the starts and the cross-part targets.  -> (index, skeleton or None)"""
        g, P, dev = self.g, self.P, self.device
        # entries: the starts (indegree 0) and every node a chain of another part continues at
        sends = []
        for p in range(P):
            g.part_clear(p, PF_MARK)
            if self.n_nodes[p]:
                g.part_mark(p, g.part_select(p, F_INDEG, 0), PF_MARK)
                counts, targets = g.part_cross_targets(p)
                owner = torch.repeat_interleave(torch.arange(self.nv, device=dev), torch.tensor(counts, device=dev))
                sends.append((owner << 32) | _u32(targets))
        got = self._to_parts(torch.cat(sends) if sends else torch.empty(0, dtype=torch.int64, device=dev))
        if extra_entries is not None:
            v = extra_entries >> 32
            for p in range(P):
                got[p] = torch.cat([got[p], (extra_entries[v == self._v(p)] & 0xFFFFFFFF).to(torch.int32)])
        segs = []
        for p in range(P):
            if not self.n_nodes[p]:
                continue
            g.part_mark(p, torch.unique(got[p]), PF_MARK)
            ent = g.part_select(p, PF_MARK, PF_MARK)
            s = g.part_segments(p, ent)
            r = g.part_gather(p, ent, what=("stamps", "pflags"))
            gid = (self._v(p) << 32) | _u32(ent)
            nxt = (s["next_owner"].to(torch.int64) << 32) | _u32(s["next_local"])
            segs.append({"gid": gid, "kind": s["kind"].to(torch.int64), "next": nxt, "hops": _u32(s["hops"]), "score": s["score"],
                         "exit": _u32(s["last"]), "stamp": r["stamps"], "start": ((r["pflags"] & F_INDEG) == 0).to(torch.int64)})
            g.part_clear(p, PF_MARK)
        if segs:
            mine = self._cat(segs)
        else:
            mine = {c: torch.empty(0, dtype=torch.int64, device=dev) for c in ("gid", "kind", "next", "hops", "score", "exit", "stamp", "start")}
        cols = list(mine.keys())
        e = dict(zip(cols, self.net.gather_all(*[mine[c] for c in cols])))
        index, skeleton = rank_skeleton(e, self.k, keep_skeleton)
        if keep_skeleton:
            g.part_set_skeleton(skeleton["gid"], skeleton["next"], skeleton["go_on"], skeleton["hops"], skeleton["rest"])
            self.skeleton = {"emit": skeleton["emit"].astype(np.int64), "length": index["length"], "score": index["score"]}
        return index, skeleton

    # ---- a11 + a12 + a13, final mode (the driver's last k: branch_kmer == [], debruijn.py:281-283)
    def walk_final(self, max_chars=0):
        """output_contigs with an empty branch list: every simple path from every start (debruijn.py:288-316), stopped only by
        dead ends and pulled nodes -- dict(stamp uint64, seq uint32, length int64, score int64) in the reference's order (the
        starts in dict order, DFS order within a start).  The kept successors of all branch nodes become entries besides
        those of ``walk_index``; the ranked skeleton then names, for every entry, the end of its chain, and the library walks
        the contracted graph of entries and branch nodes (include/dbg.h: dbg_part_final_walk).  Every rank holds the same
        contracted graph and runs the same walk.  Without a branch node in the whole graph this is the non-final index.
        max_chars: refuse (DbgError, DBG_E_CAPACITY) contig text beyond it, 0 = 1 GiB."""
        b = getattr(self, "branch", None)
        if b is None:
            raise _dbg.DbgError(_dbg.DBG_E_ARG, "part_traversal: prune() must run before walk_final()")
        dev, nb = self.device, int(b["gid"].size)
        if nb == 0:
            index = self.walk_index(keep_skeleton=True)
            index["seq"] = np.zeros(index["stamp"].size, dtype=np.uint32)
            return index
        if getattr(self, "first_seen", None) is None:
            raise _dbg.DbgError(_dbg.DBG_E_ARG, "part_traversal: pull_out_reads() must run before walk_final() (it ranks the successors of the branch nodes)")
        # the branch table in Counter order, kept edges only: (successor gid, edge count) per rank
        keep = ((b["pflags"].astype(np.int64)[:, None] >> (F_KEEP_SHIFT + np.arange(4))[None, :]) & 1) == 1
        counts = np.where(keep, b["counts"].astype(np.int64), 0)
        order = self._order_bytes(counts, self.first_seen)
        code = (order[:, None].astype(np.int64) >> (2 * np.arange(4))[None, :]) & 3      # code at rank r
        kept_r = np.take_along_axis(keep, code, axis=1)
        succ_r = np.where(kept_r, np.take_along_axis(b["succ"].astype(np.int64), code, axis=1), -1)
        cnt_r = np.where(kept_r, np.take_along_axis(counts, code, axis=1), 0)
        if bool((kept_r & (succ_r < 0)).any()):
            raise RuntimeError("walk_final: a kept edge of a branch node has no successor node")
        slot = np.argsort(~kept_r, axis=1, kind="stable")                                # kept ranks first, in rank order
        succ_r, cnt_r = np.take_along_axis(succ_r, slot, axis=1), np.take_along_axis(cnt_r, slot, axis=1)
        d_succ = torch.from_numpy(succ_r.reshape(-1)).to(dev)
        self.final = None
        _, sk = self._ranked_skeleton(True, extra_entries=torch.unique(d_succ[d_succ >= 0]))
        n = sk["gid"].numel()
        gid, term, kind = sk["gid"], sk["terminal"], sk["kind"]
        live = sk["rest"] >= 0
        tk = kind[term]
        # the node a live chain ends at, joined with the branch list
        end_gid = (gid[term] & ~0xFFFFFFFF) | sk["exit"][term]
        bo = np.argsort(b["gid"], kind="stable")
        b_sorted = torch.from_numpy(b["gid"][bo].astype(np.int64)).to(dev)
        at = torch.searchsorted(b_sorted, end_gid).clamp_(max=nb - 1)
        at_branch = live & (tk == K_EMIT) & (b_sorted[at] == end_gid)
        out_kind = torch.full((n,), 3, dtype=torch.uint8, device=dev)                    # dead, unless:
        out_kind[live & (tk == K_EMIT)] = 0
        out_kind[live & ((tk == K_NEXT_PULLED) | (tk == K_REMOTE))] = 2
        out_kind[at_branch] = 4
        out_kind[kind == K_PULLED] = 1
        stray = live & (kind != K_PULLED) & ((tk == K_PULLED) | (tk == K_CYCLE))
        row = torch.searchsorted(gid, torch.where(d_succ >= 0, d_succ, torch.zeros_like(d_succ))).clamp_(max=max(n - 1, 0))
        lost = (d_succ >= 0) & (gid[row] != d_succ) if n else (d_succ >= 0)
        bad = torch.stack([stray.any(), lost.any()]).cpu().tolist()                      # one host sync for both checks
        if bad[0]:
            raise RuntimeError("walk_final: a resolved chain ends in a pulled entry or a cycle")
        if bad[1]:
            raise RuntimeError("walk_final: a kept successor of a branch node is no entry of the skeleton")
        out_branch = torch.zeros(n, dtype=torch.int32, device=dev)
        out_branch[at_branch] = torch.from_numpy(bo.astype(np.int32)).to(dev)[at[at_branch]]
        zero = torch.zeros_like(sk["rest"])
        st = torch.nonzero(sk["start"] == 1).reshape(-1)
        st = st[torch.argsort(sk["stamp"][st])]                                          # dict order of the starts
        res = self.g.part_final_walk(out_kind, torch.where(live, sk["rest"], zero).contiguous(),
                                     torch.where(live, sk["chain_score"], zero).contiguous(), out_branch,
                                     torch.where(d_succ >= 0, row, torch.full_like(row, -1)).to(torch.int32).contiguous(),
                                     torch.from_numpy(cnt_r.reshape(-1)).to(dev).to(torch.int32).contiguous(),
                                     st.to(torch.int32).contiguous(), max_chars=max_chars)
        stamps = sk["stamp"][st].cpu().numpy().astype(np.uint64)
        index = {"stamp": stamps[res["start_ordinal"]], "seq": res["seq"], "length": res["length"].astype(np.int64),
                 "score": res["score"].astype(np.int64)}
        # pieces: the skeleton rows a contig is stitched from (the library holds the skeleton: _ranked_skeleton set it)
        self.final = {"piece_off": res["piece_off"].astype(np.int64), "piece_row": res["piece_row"].astype(np.int64),
                      "length": index["length"], "score": index["score"], "rest": sk["rest"]}
        return index

    STITCH_CHARS = 32 << 20   # contig characters of one stitch: its gather index is 8 bytes a character

    def _rows_texts_packed(self, rows):
        """-> (offsets int64[n + 1], chars uint8): the texts of the chains that start at the skeleton rows ``rows`` (numpy
        int64; k + rest characters each), concatenated.  Collective like ``contig_texts_packed``."""
        if self.world == 1:
            off, chars = self.g.part_export_contig_texts(rows)
            return off.astype(np.int64), chars
        rest = self.final["rest"][torch.from_numpy(rows).to(self.device)].cpu().numpy()
        off = np.zeros(rows.size + 1, dtype=np.int64)
        off[1:] = np.cumsum(rest + self.k)
        chars = np.empty(int(off[-1]), dtype=np.uint8)
        if rows.size:
            at = [0]

            def sink(w):
                chars[at[0]:at[0] + w.size] = w
                at[0] += w.size
            total = self._windows(rows, False, 0, 0, self.WINDOW_BYTES, sink)
            if total != chars.size or at[0] != total:
                raise RuntimeError(f"contig_texts: the library lays out {total} characters, the skeleton {chars.size}")
        return off, chars

    def _final_which(self, which):
        f = self.final
        n = f["length"].size
        if which is None:
            which = np.argsort(-f["score"], kind="stable")
        which = np.asarray(list(which) if not isinstance(which, np.ndarray) else which, dtype=np.int64).reshape(-1)
        if which.size and (int(which.min()) < -n or int(which.max()) >= n):
            raise IndexError(f"contig index out of range (the walk has {n} contigs)")
        return np.where(which < 0, which + n, which)

    def _final_blocks(self, which):
        """slices of ``which`` of at most min(BATCH_CHARS, STITCH_CHARS) characters (a longer contig is a block of its own)"""
        ends = np.cumsum(self.final["length"][which], dtype=np.int64)
        limit, at = min(BATCH_CHARS, self.STITCH_CHARS), 0
        while at < which.size:
            base = int(ends[at - 1]) if at else 0
            stop = max(int(np.searchsorted(ends, base + limit, side="right")), at + 1)
            yield which[at:stop]
            at = stop

    def _final_stitch(self, which):
        """The texts of the final contigs ``which`` (one block): the first piece's text, then every later piece's without its
        first k - 1 characters (a branch node's successor overlaps it by k - 1).  The distinct pieces are spelled once by
        the window path; the stitch is one gather over their packed characters.  -> (offsets int64[n + 1], chars uint8)"""
        f, k = self.final, self.k
        p0, p1 = f["piece_off"][which], f["piece_off"][which + 1]
        n_p = p1 - p0
        first = np.zeros(which.size + 1, dtype=np.int64)
        first[1:] = np.cumsum(n_p)
        pieces = f["piece_row"][np.repeat(p0 - first[:-1], n_p) + np.arange(int(first[-1]))]
        rows, inv = np.unique(pieces, return_inverse=True)
        r_off, r_chars = self._rows_texts_packed(rows)
        skip = np.full(pieces.size, k - 1, dtype=np.int64)
        skip[first[:-1]] = 0
        src = r_off[inv] + skip
        length = r_off[inv + 1] - src
        dst = np.zeros(pieces.size + 1, dtype=np.int64)
        dst[1:] = np.cumsum(length)
        off = dst[first]
        if not np.array_equal(off[1:] - off[:-1], f["length"][which]):
            raise RuntimeError("walk_final: the pieces of a contig do not add up to its length")
        chars = r_chars[np.repeat(src - dst[:-1], length) + np.arange(int(dst[-1]))]
        return off, chars

    def _final_texts_packed(self, which):
        which = self._final_which(which)
        offs, chars, base = [np.zeros(1, dtype=np.int64)], [], 0
        for block in self._final_blocks(which):
            o, c = self._final_stitch(block)
            offs.append(o[1:] + base)
            chars.append(c)
            base += int(o[-1])
        return np.concatenate(offs).astype(np.uint64), (np.concatenate(chars) if chars else np.empty(0, dtype=np.uint8))

    def _final_write_fasta(self, path, which, first_number, k_label, append):
        which = self._final_which(which)
        if not which.size:
            return 0
        f = open(path, "ab" if append else "wb") if self.rank == 0 else None
        written, number = 0, int(first_number)
        try:
            for block in self._final_blocks(which):
                o, c = self._final_stitch(block)
                rec = []
                for i in range(block.size):
                    rec += [b">SEQUENCE_%d_%dmer\n" % (number + i, k_label or self.k), c[o[i]:o[i + 1]].tobytes(), b"\n"]
                number += block.size
                data = b"".join(rec)
                written += len(data)
                if f:
                    f.write(data)
        finally:
            if f:
                f.close()
        return written

    # ---- contig text (include/dbg.h: dbg_part_export_contig_texts, dbg_part_write_contigs_fasta, dbg_part_contig_window)
    WINDOW_BYTES = 4 << 20   # window of the several-rank path where the caller names none (the library's default)

    def _starts(self, which):
        """contig positions -> skeleton rows of their starts (numpy int64); None: the driver's order, score descending and
        stable over the index order (II_assembleFromReads.py:64)."""
        sk = getattr(self, "skeleton", None)
        if sk is None:
            raise _dbg.DbgError(_dbg.DBG_E_ARG, "part_traversal: walk_index(keep_skeleton=True) must run first")
        if which is None:
            which = np.argsort(-sk["score"], kind="stable")
        which = np.asarray(list(which) if not isinstance(which, np.ndarray) else which, dtype=np.int64).reshape(-1)
        n = sk["emit"].size
        if which.size and (int(which.min()) < -n or int(which.max()) >= n):
            raise IndexError(f"contig index out of range (the walk has {n} contigs)")
        return which, sk["emit"][which]

    def _windows(self, starts, fasta, first_number, k_label, chunk, sink):
        """Several ranks: every rank fills window after window with the bytes of ITS parts (the others' are 0), the windows
        are gathered and combined by an elementwise maximum, ``sink(bytes as a numpy view)`` takes each.  -> total bytes."""
        dev = self.device
        d_starts = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).to(dev)
        total = self.g.part_contig_window(d_starts, 0, 0, None, fasta, first_number, k_label)
        buf = torch.empty(min(chunk, -(-total // 4096) * 4096), dtype=torch.uint8, device=dev)
        for b0 in range(0, total, chunk):
            b1 = min(total, b0 + chunk)
            self.g.part_contig_window(d_starts, b0, b1, buf, fasta, first_number, k_label)
            (parts,) = self.net.gather_all(buf[:b1 - b0])
            sink(parts.reshape(self.world, -1).max(dim=0).values.cpu().numpy())
        return total

    def contig_texts_packed(self, which):
        """-> (offsets uint64[n + 1], chars uint8): the texts of the contigs ``which`` (positions in the index, any order,
        repeats allowed), concatenated.  Collective: every rank calls it with the same list and gets the same bytes."""
        if self.final is not None:
            return self._final_texts_packed(which)
        which, starts = self._starts(which)
        if self.world == 1:
            return self.g.part_export_contig_texts(starts)
        off = np.zeros(which.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum(self.skeleton["length"][which], dtype=np.uint64)
        chars = np.empty(int(off[-1]), dtype=np.uint8)
        if which.size:
            at = [0]

            def sink(w):
                chars[at[0]:at[0] + w.size] = w
                at[0] += w.size
            total = self._windows(starts, False, 0, 0, self.WINDOW_BYTES, sink)
            if total != chars.size or at[0] != total:
                raise RuntimeError(f"contig_texts: the library lays out {total} characters, the index {chars.size}")
        return off, chars

    def write_contigs_fasta(self, path, which=None, first_number=0, k_label=0, append=True, chunk_bytes=0):
        """``>SEQUENCE_{first_number + i}_{k_label}mer\\n{contig}\\n`` (II_assembleFromReads.py:64-69) for the contigs ``which``
        (None: all of them in the driver's order) to ``path``; k_label 0: this k.  Collective; rank 0 alone opens and
        writes the file, every rank returns the bytes written.  chunk_bytes: window size, a multiple of 4096 (0: default)."""
        if self.final is not None:   # stitched on the host: chunk_bytes sizes no window here
            return self._final_write_fasta(path, which, first_number, k_label, append)
        which, starts = self._starts(which)
        if chunk_bytes % 4096:
            raise _dbg.DbgError(_dbg.DBG_E_ARG, f"write_contigs_fasta: chunk_bytes {chunk_bytes} is no multiple of 4096")
        if self.world == 1:
            return self.g.part_write_contigs_fasta(path, starts, append=append, first_number=first_number, k_label=k_label,
                                                   chunk_bytes=chunk_bytes)
        if not which.size:
            return 0
        f = open(path, "ab" if append else "wb") if self.rank == 0 else None
        try:
            return self._windows(starts, True, first_number, k_label, chunk_bytes or self.WINDOW_BYTES,
                                 (lambda w: f.write(w.tobytes())) if f else (lambda w: None))
        finally:
            if f:
                f.close()

    def contig_texts(self, which):
        """The text of the contigs ``which`` (positions in the index ``walk_index(keep_skeleton=True)`` returned) -- every rank
        calls it with the same list and gets the same strings.  A contig is its start k-mer followed by the last base of every
        node its chain appends (debruijn.py:296-299); one batched export, one ``str`` per contig at the end."""
        off, chars = self.contig_texts_packed(which)
        text = chars.tobytes().decode("ascii")
        o = off.tolist()
        return [text[o[i]:o[i + 1]] for i in range(len(o) - 1)]


BATCH_CHARS = 256 << 20  # characters of one batched text export: bounds the host copy (as debruijn.BATCH_CHARS does)


class PartContigs:
    """The contigs of a graph in parts, in the reference's order (dict order of the starts): ``lengths``, ``scores`` (getScore,
    II_assembleFromReads.py:14-18), ``start_stamps``; ``texts(indices)``, slices, iteration and ``packed()`` spell them (all
    collective: every rank asks for the same ones), one batched export per block of contigs; ``write_fasta`` writes the
    driver's file.  At scale the contigs overlap massively -- 2e12 characters for 10 M reads -- so the text is on demand."""

    def __init__(self, traversal, index):
        self._t = traversal
        self.start_stamps, self.lengths, self.scores = index["stamp"], index["length"], index["score"]

    def __len__(self):
        return int(self.start_stamps.size)

    def _blocks(self, idx):
        """slices of ``idx`` whose texts add up to BATCH_CHARS at most (a longer contig is a block of its own)"""
        ends = np.cumsum(self.lengths[idx], dtype=np.int64)
        at = 0
        while at < idx.size:
            base = int(ends[at - 1]) if at else 0
            stop = max(int(np.searchsorted(ends, base + BATCH_CHARS, side="right")), at + 1)
            yield idx[at:stop]
            at = stop

    def texts(self, indices):
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        out = []
        for block in self._blocks(idx):
            out += self._t.contig_texts(block)
        return out

    def packed(self):
        """-> (uint8 characters, uint64 offsets[len + 1]) of all contigs in index order, as ``LazyContigs.packed`` gives
        them: one batched export per block, no ``str`` per contig."""
        chars = [self._t.contig_texts_packed(block)[1] for block in self._blocks(np.arange(len(self)))]
        off = np.zeros(len(self) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(self.lengths, dtype=np.uint64)
        return (np.concatenate(chars) if chars else np.empty(0, dtype=np.uint8)), off

    def __iter__(self):
        for block in self._blocks(np.arange(len(self))):
            yield from self._t.contig_texts(block)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.texts(range(*i.indices(len(self))))
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self.texts([i])[0]

    def write_fasta(self, path, k, append=True):
        """The driver's output (II_assembleFromReads.py:64-69): every contig as ``>SEQUENCE_{i}_{k}mer``, sorted by score
        descending and stable like ``sequences.sort(key=getScore, reverse=True)``, written to ``path`` (rank 0 writes; a
        list of the caller's goes through ``PartTraversal.write_contigs_fasta``).  -> bytes written."""
        return self._t.write_contigs_fasta(path, None, k_label=k, append=append)


def construct_graph(g, k, threshold=3, dist=None, final=False):
    """construct_graph (debruijn.py:206-285) after a build in parts (``g.build_multipass`` or, with ``dist``,
    ``multi_gpu.sharded_build_multipass``), every rank calling it: -> (traversal, pull_out_read_flags, branch_kmer,
    already_pull_out) with the reference's lists as str (dict order / append order; the same on every rank) and the
    pull-out reads as uint8 flags over THIS rank's reads (the reference's list is the flagged reads of rank 0, 1, ... in order).
    final (the driver's last k): no pull-out reads and an empty branch list (debruijn.py:281-283); ``output_contigs`` then
    walks every simple path."""
    t = PartTraversal(g, k, dist)
    t.final_mode = bool(final)
    b = t.prune(threshold)
    flags = t.pull_out_reads()
    p = t.remove_tips()
    if final:
        return t, np.zeros_like(flags), [], _dbg.decode_keys(p["keys"], t.k, keys_hi=p["keys_hi"])
    branch_kmer = _dbg.decode_keys(b["keys"].astype(np.uint64), t.k, keys_hi=b["keys_hi"].astype(np.uint64))
    already_pull_out = _dbg.decode_keys(p["keys"], t.k, keys_hi=p["keys_hi"])
    return t, flags, branch_kmer, already_pull_out


def output_contigs(traversal):
    """output_contigs (debruijn.py:326-347) for the branch list ``construct_graph`` above returned: the non-final walk, or,
    after ``construct_graph(final=True)``, every simple path (``walk_final``).  max_chars of the final walk: the default."""
    if traversal.final_mode:
        return PartContigs(traversal, traversal.walk_final())
    return PartContigs(traversal, traversal.walk_index(keep_skeleton=True))


def traverse(g, k, threshold, dist=None, final=False):
    """prune -> pull-out reads -> tips -> walk (final: every simple path, else the non-final one) over the graph in parts on
    ``g`` (every rank calls it).  -> dict(branch, pulled, read_flags, contigs)."""
    t = PartTraversal(g, k, dist)
    branch = t.prune(threshold)
    flags = t.pull_out_reads()
    pulled = t.remove_tips()
    contigs = t.walk_final() if final else t.walk_index()
    return {"branch": branch, "pulled": pulled, "read_flags": flags, "contigs": contigs, "tip_rounds": getattr(t, "tip_rounds", 0)}
