// Final-mode contig walk (debruijn.py:288-316 with branch_kmer == [], the driver's last k) over a graph in PARTS.
//
// The walk runs on a CONTRACTED graph that part_traversal.walk_final builds from the ranked skeleton of segments: one row
// per entry node (the starts, the targets of chain edges that leave a part, and every kept successor of a branch node),
// whose chain has been followed to its end by pointer jumping, and one row of a branch table per branch node of the
// whole graph with its kept successors in Counter.most_common order -- the order DFS tries E[current][i].
//
//   kind of a row                                                          entering it (k_walk_dfs of dbg_hip.hip is the model)
//   FW_EMIT           the chain ends at a node without kept successor     emit path + edge + row, that node included [:304-313]
//   FW_PULLED         the entry itself is pulled                          emit the path up to the parent branch node, once
//                                                                         per visit of that node [:292-303, `vec not in output`]
//   FW_BEFORE_PULLED  the chain ends in front of a pulled node            emit path + edge + row [:292-303]
//   FW_DEAD           the chain closes on itself, or never resolved       nothing [:289-290]
//   FW_BRANCH         the chain ends at branch-table row `branch`         on the path already: nothing [:289-290]; else push it
//                                                                         and try its successors in rank order [:314-315]
//
// Only branch nodes need an on-path mark.  A chain node has exactly one kept successor, so a chain that meets a node y of
// the current path follows y's successors to the branch node the path is branching at: the row's terminal IS an on-path
// branch node, and the reference, which returns silently at y, emits nothing either.  The visited state of a walker is
// therefore n_branch bits, and its stack n_branch + 1 levels (every level holds another branch node).
//
// A contig is a list of rows (its pieces): the start's row, then the row entered at every branching.  Its text is the
// text of the first piece followed by every later piece's text without its first k - 1 characters; its length is
// k + nodes - 1 and its score the sum of the edge counts along the path.
//
// Everything here is plain C++ that a host compiler can include (tests/test_partfinal_host.py does): the validation
// predicate and the walker itself, one __host__ __device__ function.  The kernels are in dbg_hip.hip.
#pragma once
#include <stdint.h>

#ifndef DBG_CO_HD
#if defined(__HIPCC__)
#define DBG_CO_HD __host__ __device__
#else
#define DBG_CO_HD
#endif
#endif

namespace dbgk {

enum FwKind : uint8_t { FW_EMIT = 0, FW_PULLED = 1, FW_BEFORE_PULLED = 2, FW_DEAD = 3, FW_BRANCH = 4, FW_N_KINDS = 5 };
constexpr uint32_t FW_NO_ROW = 0xFFFFFFFFu;           // DBG_NO_NODE: an empty successor slot of the branch table
constexpr int FW_FAN = 4;                             // successor slots of a branch node (DNA)
constexpr uint64_t FW_DEFAULT_STEPS = 1ull << 24;     // option "part_final_walk_steps": steps one walker may take in a pass (1.3 us each, measured)

// the contracted graph, as the caller hands it in (device arrays on the device, plain arrays in the host test)
struct FwGraph {
    const uint8_t *kind;       // [n_entries] FwKind
    const uint64_t *append;    // [n_entries] nodes the chain appends after the entry (the skeleton's rest); read for EMIT, BEFORE_PULLED, BRANCH
    const uint64_t *score;     // [n_entries] sum of the edge counts along those
    const uint32_t *branch;    // [n_entries] row of the branch table where kind is FW_BRANCH
    const uint32_t *succ_row;  // [n_branch * 4] entry row of the successor at rank r, FW_NO_ROW: none
    const uint32_t *succ_cnt;  // [n_branch * 4] count of the edge to it
    const uint32_t *starts;    // [n_starts] entry rows of the nodes with indegree 0, dict order
    uint64_t n_entries, n_branch, n_starts;
};

enum FwFault : int { FW_OK = 0, FW_BAD_KIND = 1, FW_BAD_BRANCH = 2, FW_BAD_SUCC = 4, FW_BAD_START = 8 };

// Index i runs over max(n_entries, n_branch * 4, n_starts): what makes row i, successor slot i or start i unfit to be walked
// (0: nothing).  Every index the walker follows is covered, so a graph that passes cannot lead it out of an array.
DBG_CO_HD inline int fw_fault_at(const FwGraph &g, uint64_t i) {
    int f = FW_OK;
    if (i < g.n_entries) {
        const uint8_t kd = g.kind[i];
        if (kd >= FW_N_KINDS) f |= FW_BAD_KIND;
        else if (kd == FW_BRANCH && g.branch[i] >= g.n_branch) f |= FW_BAD_BRANCH;
    }
    if (i < g.n_branch * FW_FAN) {
        const uint32_t r = g.succ_row[i];
        if (r != FW_NO_ROW && r >= g.n_entries) f |= FW_BAD_SUCC;
    }
    if (i < g.n_starts && g.starts[i] >= g.n_entries) f |= FW_BAD_START;
    return f;
}

// one level of a walker's stack: the row whose chain ended at the branch node this level stands on
struct FwLevel {
    uint32_t row;
    uint32_t state;   // bits 2:0 next rank to try, bit 7: the path up to this branch node was emitted for a pulled successor
    uint64_t nodes;   // nodes of the path up to and including this branch node
    uint64_t score;   // edge counts along them
};

// where pass 1 writes (pass 0 reads none of it); n_contigs / n_pieces bound every store
struct FwOut {
    uint32_t *start_ord, *seq;
    uint64_t *length, *score, *piece_off;
    uint32_t *piece_row;
    uint64_t n_contigs, n_pieces;
};

struct FwCount {
    uint64_t contigs, pieces, chars;
};

// All simple paths from start i.  Level d of the stack is lv[d * stride] and word q of the on-path bitmap bm[q * stride]
// (the walkers of a wave interleave theirs; the host test passes stride 1); the bitmap is all zero before and after.
// pass 0 counts into cnt, pass 1 also writes contig c_base + (ordinal within the start) and its pieces from p_base on.
// `steps` is what the walker may still take: false (bitmap left dirty) when they ran out.
DBG_CO_HD inline bool fw_walk_start(const FwGraph &g, int k, uint64_t i, FwLevel *lv, uint32_t *bm, uint64_t stride, int pass,
                                    uint64_t c_base, uint64_t p_base, const FwOut &o, FwCount &cnt, uint64_t &steps) {
    uint64_t depth = 0;
    // the path's rows are the levels 0 .. depth - 1, then `extra` (a row that ends the path) unless it is FW_NO_ROW
    auto emit = [&](uint32_t extra, uint64_t nodes, uint64_t score) {
        const uint64_t np = depth + (extra != FW_NO_ROW ? 1 : 0);
        const uint64_t len = (uint64_t)k + nodes - 1;
        if (pass == 1) {
            const uint64_t c = c_base + cnt.contigs, p = p_base + cnt.pieces;
            if (c < o.n_contigs && p + np <= o.n_pieces) {
                o.start_ord[c] = (uint32_t)i;
                o.seq[c] = (uint32_t)cnt.contigs;
                o.length[c] = len;
                o.score[c] = score;
                o.piece_off[c] = p;
                for (uint64_t d = 0; d < depth; ++d) o.piece_row[p + d] = lv[d * stride].row;
                if (extra != FW_NO_ROW) o.piece_row[p + depth] = extra;
            }
        }
        ++cnt.contigs;
        cnt.pieces += np;
        cnt.chars += len;
    };
    // DFS(current = the entry of row r), reached over an edge of count c from a path of `nodes` nodes and `score`
    auto enter = [&](uint32_t r, uint32_t c, uint64_t nodes, uint64_t score) {
        const uint8_t kd = g.kind[r];
        if (kd == FW_DEAD) return;
        if (kd == FW_PULLED) {
            if (depth > 0 && !(lv[(depth - 1) * stride].state & 0x80u)) {
                lv[(depth - 1) * stride].state |= 0x80u;
                emit(FW_NO_ROW, nodes, score);
            }
            return;
        }
        nodes += 1 + g.append[r];
        score += (uint64_t)c + g.score[r];
        if (kd != FW_BRANCH) { emit(r, nodes, score); return; }
        const uint32_t b = g.branch[r];
        if ((bm[(uint64_t)(b >> 5) * stride] >> (b & 31u)) & 1u) return;
        bm[(uint64_t)(b >> 5) * stride] |= 1u << (b & 31u);
        lv[depth * stride] = FwLevel{r, 0u, nodes, score};
        ++depth;
    };
    enter(g.starts[i], 0u, 0u, 0u);
    while (depth > 0) {
        if (steps == 0) return false;
        --steps;
        FwLevel &top = lv[(depth - 1) * stride];
        const uint32_t r = top.state & 7u, b = g.branch[top.row];
        if (r >= (uint32_t)FW_FAN) {
            bm[(uint64_t)(b >> 5) * stride] &= ~(1u << (b & 31u));
            --depth;
            continue;
        }
        top.state = (top.state & 0x80u) | (r + 1);
        const uint32_t nx = g.succ_row[(uint64_t)b * FW_FAN + r];
        if (nx == FW_NO_ROW) continue;
        enter(nx, g.succ_cnt[(uint64_t)b * FW_FAN + r], top.nodes, top.score);
    }
    return true;
}

}  // namespace dbgk
