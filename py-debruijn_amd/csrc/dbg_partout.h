// Output side of a walk over a graph in PARTS: a text source for the window kernel of dbg_ctgout.h that spells contigs
// from the ranked skeleton of segments (part_traversal.rank_skeleton) and the parts this handle holds
// (dbg_part_set_skeleton, dbg_part_contig_window, dbg_part_export_contig_texts, dbg_part_write_contigs_fasta).
//
// The skeleton has one row per entry node, sorted by global id (virtual shard << 32 | local id): the segment that starts
// there appends `hops` characters inside its part, then -- where go_on is set -- enters the entry `next`, which appends
// that node's last base and goes on.  rest[i] = hops[i] + go_on[i] * (1 + rest[next[i]]) is what the chain appends from
// entry i to its end, so the contig that starts at entry e has k + rest[e] characters and segment s of e's chain begins
// at appended index rest[e] - rest[s] (index 0 is the start node itself: its k-mer is the first k characters).  rest
// falls strictly along a chain: the last segment that begins at or before an index is found by a binary-lifting descent
// over up[l][i] (the 2^l-th segment after i; the chain's end loops to itself), and the characters inside the segment are
// kept-successor steps in that part -- at most hops[s] of them.  A segment in a part another handle holds contributes
// the byte 0 and is skipped by arithmetic.
//
// Like dbg_ctgout.h, the first part -- the validation predicate, the table geometry and the source itself over an
// abstract "part view" -- is plain C++ that a host compiler can include (tests/test_partout_host.py does); the device
// part view follows under __HIPCC__ (it needs pf_chain / pf_kept_col of dbg_hip.hip in front of it).
#pragma once
#include "dbg_ctgout.h"

namespace dbgk {

constexpr uint64_t PO_NO_REST = ~0ull;   // rest of an entry that is dead or whose chain never resolved: no contig starts there
constexpr uint8_t PO_ELSEWHERE = 0xFF;   // part byte of an entry whose virtual shard another handle holds
constexpr int PO_MAX_LEVELS = 32;        // entries are indexed with 32 bits

// ---- the skeleton as the caller hands it in (the columns of rank_skeleton, as the tensors hold them) ------------------------
struct PoRawSkel {
    const int64_t *gid;     // [n] strictly ascending
    const int64_t *next;    // [n] index of the entry the segment hands over to (any valid index where go_on is 0)
    const uint8_t *go_on;   // [n] 0 / 1
    const int64_t *hops;    // [n]
    const uint64_t *rest;   // [n] PO_NO_REST: no contig text from here
    uint64_t n;
};

// which virtual shards a handle holds: part p is virtual shard v_first + p
struct PoHold {
    int v_first, n_parts, n_virtual;
    const uint64_t *n_nodes;  // [n_parts]
};

DBG_CO_HD inline int po_part_of(const PoHold &hd, uint64_t gid) {
    const int64_t p = (int64_t)(gid >> 32) - hd.v_first;
    return p >= 0 && p < hd.n_parts ? (int)p : -1;
}

enum PoFault : int { PO_OK = 0, PO_BAD_GID = 1, PO_BAD_ORDER = 2, PO_BAD_LOCAL = 4, PO_BAD_NEXT = 8, PO_BAD_HOPS = 16, PO_BAD_REST = 32 };

// What makes row i unfit to be walked by a kernel (0: nothing).  Every pointer the text source follows is covered: next is an
// index, a local id of a held part is a node of it, and where rest is set it falls strictly along the chain (no cycle).
DBG_CO_HD inline int po_row_fault(const PoRawSkel &r, const PoHold &hd, uint64_t i) {
    const int64_t gid = r.gid[i];
    if (gid < 0 || (gid >> 32) >= (int64_t)hd.n_virtual) return PO_BAD_GID;
    if (i && r.gid[i - 1] >= gid) return PO_BAD_ORDER;
    const int p = po_part_of(hd, (uint64_t)gid);
    if (p >= 0 && ((uint64_t)gid & 0xFFFFFFFFull) >= hd.n_nodes[p]) return PO_BAD_LOCAL;
    const int64_t nx = r.next[i], hops = r.hops[i];
    if (nx < 0 || (uint64_t)nx >= r.n) return PO_BAD_NEXT;
    if (hops < 0 || hops > 0xFFFFFFFFll) return PO_BAD_HOPS;
    const uint64_t rest = r.rest[i];
    if (rest == PO_NO_REST) return PO_OK;
    uint64_t want = (uint64_t)hops;
    if (r.go_on[i]) {
        const uint64_t rn = r.rest[nx];
        if (rn == PO_NO_REST) return PO_BAD_REST;
        want += 1 + rn;
    }
    return rest == want ? PO_OK : PO_BAD_REST;
}

// smallest number of levels whose descent reaches `max_jumps` segments ahead: 2^levels - 1 >= max_jumps
DBG_CO_HD inline int po_levels_for(uint64_t max_jumps) {
    int l = 0;
    while (l < PO_MAX_LEVELS && ((1ull << l) - 1) < max_jumps) ++l;
    return l;
}

// ---- the library's copy ------------------------------------------------------------------------------------------------------
struct PoSkel {
    const uint64_t *gid;
    const uint32_t *next;
    const uint32_t *hops;
    const uint64_t *rest;
    const uint8_t *go_on;
    const uint8_t *part;   // part of this handle that holds the entry, PO_ELSEWHERE if none
    const uint32_t *up;    // [levels][n]; up[0][i] = go_on[i] ? next[i] : i
    uint64_t n;
    int levels;
};

// Contigs of a walk in parts.  V is the part view:
//   bool chain_step(int p, uint32_t &x)   x <- the kept successor of chain node x inside part p; false (x unchanged) where
//                                         x is no chain node or its successor lives in another part
//   char last_char(int p, uint32_t x)     last base of node x
//   char kmer_char(int p, uint32_t x, int q)
//   void fault()                          the skeleton does not fit the graph (the caller reports it; nothing is followed)
// starts[c] is the skeleton index of contig c's start entry (validated by the caller: below n, rest set).
template <class V>
struct CoPartsSrc {
    V v;
    PoSkel sk;
    const uint64_t *starts;
    int k;
    // cursor: the start entry, the segment, the node whose last base was spelled last, steps the segment has left, its part
    uint32_t e, s, x, left;
    int p;

    DBG_CO_HD inline void enter(uint32_t seg) {
        s = seg;
        p = sk.part[seg] == PO_ELSEWHERE ? -1 : (int)sk.part[seg];
        x = (uint32_t)sk.gid[seg];
        left = sk.hops[seg];
    }
    DBG_CO_HD inline char here() const { return p < 0 ? (char)0 : v.last_char(p, x); }
    DBG_CO_HD inline char kmer(uint64_t j) const {
        const uint8_t pe = sk.part[e];
        return pe == PO_ELSEWHERE ? (char)0 : v.kmer_char((int)pe, (uint32_t)sk.gid[e], (int)j);
    }
    DBG_CO_HD inline char first(uint32_t c, uint64_t j) {
        e = (uint32_t)starts[c];
        enter(e);
        if (j < (uint64_t)k) return kmer(j);
        const uint64_t a = j - (uint64_t)k + 1, re = sk.rest[e], target = re - a;  // a <= rest[e]: j is inside the contig
        uint32_t t = e;
        for (int l = sk.levels - 1; l >= 0; --l) {  // the last segment that begins at or before a: rest[t] >= rest[e] - a
            const uint32_t u = sk.up[(uint64_t)l * sk.n + t];
            if (sk.rest[u] >= target) t = u;
        }
        if (t != e) enter(t);
        const uint64_t w = a - (re - sk.rest[t]);  // steps inside the segment
        if (w > (uint64_t)left) { v.fault(); return (char)0; }
        left -= (uint32_t)w;
        if (p >= 0)
            for (uint32_t i = 0; i < (uint32_t)w; ++i)
                if (!v.chain_step(p, x)) { v.fault(); break; }
        return here();
    }
    DBG_CO_HD inline char next(uint64_t j) {
        if (j < (uint64_t)k) return kmer(j);
        if (left) {
            --left;
            if (p >= 0 && !v.chain_step(p, x)) v.fault();
        } else {
            enter(sk.next[s]);  // j is inside the contig: the segment hands over
        }
        return here();
    }
};

}  // namespace dbgk

#if defined(__HIPCC__)
namespace dbgk {

// what the source reads of one part (one table per handle, in device memory)
struct PoPart {
    const uint64_t *keys, *keys_hi;
    const uint8_t *flags, *pflags;
    const uint32_t *rowptr, *col;
    const uint8_t *col_owner;
    uint64_t n_nodes;
};

struct PoDevParts {
    const PoPart *tab;
    int v_first, k;
    unsigned long long *err;
    __device__ inline bool chain_step(int p, uint32_t &x) const {
        const PoPart &t = tab[p];
        const uint32_t pf = t.pflags[x];
        if (!pf_chain(pf)) return false;
        const uint32_t e = pf_kept_col(t.flags[x], pf, t.rowptr[x]);
        if ((int)t.col_owner[e] != v_first + p) return false;
        x = t.col[e];
        return true;
    }
    __device__ inline char last_char(int p, uint32_t x) const { return code_to_ascii((uint32_t)(tab[p].keys[x] & 3u)); }
    __device__ inline char kmer_char(int p, uint32_t x, int q) const {
        const int sh = 2 * (k - 1 - q);
        return code_to_ascii((uint32_t)(sh >= 64 ? tab[p].keys_hi[x] >> (sh - 64) : tab[p].keys[x] >> sh) & 3u);
    }
    __device__ inline void fault() const { atomicOr(err, 1ull); }
};

}  // namespace dbgk
#endif  // __HIPCC__
