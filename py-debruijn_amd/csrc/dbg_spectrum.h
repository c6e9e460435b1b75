// Whole-graph statistics on the device (dbg_count_spectrum): the abundance spectrum of the edges, the out-weight spectrum and
// the degree distributions of the nodes, in one read-only pass over the count arrays the graph already holds.
//   E[c]  (k+1)-mers with count c                       (edge_count_table)
//   W[c]  nodes whose successor counts sum to c         (len(edges[v]) before pruningEdges; W[0]: no successor)
//   D[d]  nodes with d distinct successors              (Node.outdegree; 0..4 on ACGT graphs, 0..32 on generic ones)
//   K[d]  nodes with d bits in the keep mask            (after a prune; pulled nodes included)
// With B bins a count c lands in bin min(c, B - 1); a count of 0 is no edge, so E[0] stays 0.
//
// Two count sources behind one kernel body (k_spectrum<Src, MODE>):
//   SpCsr<RP>    row pointers of 32 or 64 bits + the edge counts of the CSR: what the LDS engines leave behind (before and
//                after ensure_dense) and what every part of a graph in parts holds.  Row i ends at rowptr[i + 1], the last
//                row at n_edges: entry [n_nodes] of the row pointers is never read.
//   SpDense<D>   cnt[n][D], D = 4 or 32: every other graph.  A zero is no edge.
// One thread per node; a thread takes SP_UNROLL nodes in a trip of the grid-stride loop and issues all their loads before it
// counts anything.  The traffic is small (about 4 B of row pointer, 4 B per edge and one flag byte per node after a prune);
// the atomics are the work: real spectra put most edges into one or two bins.
//   * bins below SP_LDS_BINS are 32-bit counters in LDS, flushed to the global 64-bit bins with one atomic per non-zero
//     counter; counts at or above go straight to the global bins (rare on real data);
//   * a workgroup flushes at least every SP_FLUSH_TRIPS trips, so that no 32-bit counter can wrap (static_assert below);
//   * sum and maxima stay in registers, are reduced per wave and cost four atomics per workgroup;
//   * MODE picks how the hot bins are relieved (measured: DESIGN.md 4l): 0 plain LDS atomics, 1 one sub-histogram per wave,
//     2 equal bins of a wave are combined by ballots, round after round until every lane is served, and one lane adds their
//     number, 3 one such round for the first active lane's bin and plain atomics for the lanes that hold another.
//
// Everything up to the HIP part is plain C++: a host compiler can include this file alone (tests/spectrum_host.cpp does).
#pragma once
#include <stdint.h>

#ifndef DBG_SP_HD
#if defined(__HIPCC__)
#define DBG_SP_HD __host__ __device__
#else
#define DBG_SP_HD
#endif
#endif

namespace dbgk {

constexpr uint32_t SP_LDS_BINS = 1024;      // bins of each spectrum a workgroup keeps in LDS
constexpr uint32_t SP_DEG_BINS = 33;        // degrees 0..32
constexpr uint32_t SP_MAX_ROW = 32;         // most edges of one node
constexpr uint32_t SP_BLOCK = 256;
constexpr uint32_t SP_UNROLL = 4;           // rows a thread takes in one trip of the grid-stride loop, SP_BLOCK apart
constexpr uint32_t SP_CACHED = 4;           // counts of a row that are loaded ahead (every count of an ACGT row)
constexpr uint32_t SP_TILE = SP_BLOCK * SP_UNROLL;  // rows of a workgroup in one trip
constexpr uint32_t SP_FLUSH_TRIPS = 1u << 16;  // trips of the grid-stride loop between two flushes
constexpr uint32_t SP_MAX_GRID = 2048;
constexpr uint64_t SP_MAX_BINS = 1ull << 20;
// the most one LDS counter can receive between two flushes: every item of every thread of every trip
static_assert((uint64_t)SP_FLUSH_TRIPS * SP_TILE * (SP_MAX_ROW + 1) < (1ull << 32), "an LDS counter could wrap");

// slots of the LDS histogram of a workgroup (or of a wave, MODE 1)
constexpr uint32_t SP_SLOT_EDGE = 0;
constexpr uint32_t SP_SLOT_NODE = SP_LDS_BINS;
constexpr uint32_t SP_SLOT_DEG = 2 * SP_LDS_BINS;
constexpr uint32_t SP_SLOT_KEPT = SP_SLOT_DEG + SP_DEG_BINS;
constexpr uint32_t SP_SLOTS = SP_SLOT_KEPT + SP_DEG_BINS;

// layout of the global result: uint64 edge[n_bins], node[n_bins], deg[33], kept[33], then the scalars
enum SpScalar { SP_SUM_EDGE_COUNTS, SP_MAX_EDGE_COUNT, SP_MAX_OUT_WEIGHT, SP_N_EDGES, SP_SCALARS };
DBG_SP_HD inline uint64_t sp_result_words(uint64_t n_bins) { return 2 * n_bins + 2 * SP_DEG_BINS + SP_SCALARS; }

// ---- the rule, word by word -----------------------------------------------------------------------------------------------
// bin of a count: the last bin collects everything at or above n_bins - 1
DBG_SP_HD inline uint64_t sp_bin(uint64_t c, uint64_t n_bins) { return c < n_bins - 1 ? c : n_bins - 1; }
// a bin is counted in LDS iff it lies below SP_LDS_BINS; the others go to the global bins one by one
DBG_SP_HD inline bool sp_in_lds(uint64_t bin) { return bin < SP_LDS_BINS; }
// distinct successors from the flag byte the LDS engines write in the build (bit 1 + code: base `code` follows), and kept
// successors from the flag byte after a prune (the same four bits then hold the keep mask)
DBG_SP_HD inline uint32_t sp_degree_from_flags(uint32_t f) { return (uint32_t)__builtin_popcount((f >> 1) & 15u); }
DBG_SP_HD inline uint32_t sp_kept_from_flags(uint32_t f) { return (uint32_t)__builtin_popcount((f & 0x1Eu) >> 1); }
DBG_SP_HD inline uint32_t sp_kept_from_mask(uint32_t m) { return (uint32_t)__builtin_popcount(m); }

// ---- count sources: slots(i) places of row i, count(i, j) what stands at place j (0: no edge) ------------------------------
template <class RP>
struct SpCsr {
    const RP *rowptr;      // [n_nodes]; entry n_nodes is not read
    const uint32_t *ecnt;  // [max(n_edges, 1)]: at least one word that may be read
    uint64_t n_nodes, n_edges;
    DBG_SP_HD uint64_t row_begin(uint64_t i) const { return (uint64_t)rowptr[i]; }
    DBG_SP_HD uint64_t row_end(uint64_t i) const { return i + 1 < n_nodes ? (uint64_t)rowptr[i + 1] : n_edges; }
    DBG_SP_HD uint32_t slots(uint64_t i) const {
        const uint64_t b = row_begin(i), e = row_end(i);
        const uint64_t d = e > b ? e - b : 0;  // a damaged row pointer reads nothing
        return (uint32_t)(d < SP_MAX_ROW ? d : SP_MAX_ROW);
    }
    DBG_SP_HD uint32_t count(uint64_t i, uint32_t j) const { return ecnt[row_begin(i) + j]; }
    // count(i, j) where j < slots(i); beyond the row some count that may be read (the kernel loads ahead without a branch)
    DBG_SP_HD uint32_t count_ahead(uint64_t i, uint32_t j) const {
        const uint64_t e = row_begin(i) + j;
        return ecnt[e < n_edges ? e : 0];
    }
};
template <int D>
struct SpDense {
    const uint32_t *cnt;  // [n_nodes][D]
    uint64_t n_nodes, n_edges;
    DBG_SP_HD uint32_t slots(uint64_t) const { return (uint32_t)D; }
    DBG_SP_HD uint32_t count(uint64_t i, uint32_t j) const { return cnt[i * (uint64_t)D + j]; }
    DBG_SP_HD uint32_t count_ahead(uint64_t i, uint32_t j) const { return cnt[i * (uint64_t)D + (j < (uint32_t)D ? j : 0)]; }
};
// kept successors of a node: the flag byte (ACGT graphs and parts), the 32-bit mask (generic graphs), or nothing yet
struct SpKeep {
    const uint8_t *flags;
    const uint32_t *mask;
    DBG_SP_HD bool any() const { return flags || mask; }
    DBG_SP_HD uint32_t kept(uint64_t i) const { return flags ? sp_kept_from_flags(flags[i]) : sp_kept_from_mask(mask[i]); }
};

// a row whose first SP_CACHED counts are already in registers, as a count source of its own (the kernel loads ahead)
template <class Src>
struct SpCached {
    const Src *src;
    uint32_t n;             // slots of the row
    uint32_t c[SP_CACHED];  // count(i, j) for j < min(n, SP_CACHED)
    DBG_SP_HD uint32_t slots(uint64_t) const { return n; }
    DBG_SP_HD uint32_t count(uint64_t i, uint32_t j) const {
        return j == 0 ? c[0] : j == 1 ? c[1] : j == 2 ? c[2] : j == 3 ? c[3] : src->count(i, j);  // no indexed register array
    }
};
static_assert(SP_CACHED == 4, "SpCached::count names its four registers");

// what one thread carries in registers
struct SpAcc {
    uint64_t sum_edge_counts = 0, max_out_weight = 0, n_edges = 0;
    uint32_t max_edge_count = 0;
};

// The body of one row: every edge goes to sink.edge(bin), the node to sink.node(bin of its out-weight) and
// sink.degree(d).  Returns nothing; the running sum and maxima go to acc.
template <class Src, class Sink>
DBG_SP_HD inline void sp_row(const Src &src, uint64_t i, uint64_t n_bins, SpAcc &acc, Sink &sink) {
    const uint32_t n = src.slots(i);
    uint64_t weight = 0;
    uint32_t deg = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t c = src.count(i, j);
        if (!c) continue;
        ++deg;
        weight += c;
        if (c > acc.max_edge_count) acc.max_edge_count = c;
        sink.edge(sp_bin(c, n_bins));
    }
    acc.sum_edge_counts += weight;
    acc.n_edges += deg;
    if (weight > acc.max_out_weight) acc.max_out_weight = weight;
    sink.node(sp_bin(weight, n_bins));
    sink.degree(deg);
}

#if defined(__HIPCC__)
}  // namespace dbgk
#include "dbg_device.h"
namespace dbgk {

__device__ inline uint64_t sp_wave_max_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_down(v, d, 64);
        v = o > v ? o : v;
    }
    return v;  // valid in lane 0
}

// one add to the LDS histogram `s`, or to the global bin where the LDS does not hold it
__device__ inline void sp_add_plain(uint32_t *s, uint32_t lds_slot, bool in_lds, unsigned long long *g) {
    if (in_lds) atomicAdd(&s[lds_slot], 1u);
    else atomicAdd(g, 1ull);
}
// the same for a whole wave at once (every lane calls it; `active` says whether the lane has an item): the lanes that
// hold the same LDS slot are found by ballots and one of them adds their number
__device__ inline void sp_add_combined(uint32_t *s, uint32_t lds_slot, bool in_lds, unsigned long long *g, bool active) {
    if (active && !in_lds) atomicAdd(g, 1ull);
    uint64_t todo = __ballot(active && in_lds);
    const uint32_t lane = threadIdx.x & 63u;
    while (todo) {  // uniform in the wave
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t v = (uint32_t)__shfl((int)lds_slot, leader, 64);
        const uint64_t same = __ballot(active && in_lds && lds_slot == v) & todo;
        if ((int)lane == leader) atomicAdd(&s[v], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// one round of the same: the lanes that hold the first active lane's slot are counted by one ballot and that lane adds their
// number; the others add for themselves.  Works on whatever lanes are active (inside a divergent loop too): on a skewed
// spectrum the first lane's slot is nearly always the hot one, and a wave's add costs one LDS atomic of one lane in place
// of 64 serialised ones.
__device__ inline void sp_add_leader(uint32_t *s, uint32_t lds_slot, bool in_lds, unsigned long long *g) {
    const uint64_t todo = __ballot(in_lds);  // the active lanes that count in LDS
    if (!in_lds) atomicAdd(g, 1ull);
    if (!todo) return;                       // the same for every active lane
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t v = (uint32_t)__shfl((int)lds_slot, leader, 64);  // the leader is active: it is in todo
    const uint64_t same = __ballot(in_lds && lds_slot == v);
    if (!in_lds) return;
    if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&s[v], (uint32_t)__popcll(same));
    else if (lds_slot != v) atomicAdd(&s[lds_slot], 1u);
}

// LDS counters -> global bins; the counters are zero afterwards.  n_sub sub-histograms of SP_SLOTS counters each.
__device__ inline void sp_flush(uint32_t *s, int n_sub, uint64_t n_bins, unsigned long long *res) {
    __syncthreads();
    for (uint32_t slot = threadIdx.x; slot < SP_SLOTS; slot += SP_BLOCK) {
        uint32_t v = 0;
        for (int w = 0; w < n_sub; ++w) { v += s[w * SP_SLOTS + slot]; s[w * SP_SLOTS + slot] = 0; }
        if (!v) continue;
        uint64_t at;
        if (slot < SP_SLOT_NODE) at = slot;                                      // edge bin
        else if (slot < SP_SLOT_DEG) at = n_bins + (slot - SP_SLOT_NODE);        // node bin
        else at = 2 * n_bins + (slot - SP_SLOT_DEG);                             // degree, kept degree
        atomicAdd(&res[at], (unsigned long long)v);
    }
    __syncthreads();
}

template <class Src, int MODE>
__global__ __launch_bounds__(256) void k_spectrum(Src src, SpKeep keep, uint64_t n_bins, unsigned long long *res) {
    constexpr int N_SUB = MODE == 1 ? 4 : 1;
    __shared__ uint32_t s_hist[N_SUB * SP_SLOTS];
    __shared__ uint64_t s_red[4][4];
    for (uint32_t t = threadIdx.x; t < N_SUB * SP_SLOTS; t += SP_BLOCK) s_hist[t] = 0;
    __syncthreads();
    uint32_t *s = s_hist + (MODE == 1 ? (threadIdx.x >> 6) * SP_SLOTS : 0);
    unsigned long long *g_edge = res, *g_node = res + n_bins, *g_deg = res + 2 * n_bins;
    const bool has_keep = keep.any();
    SpAcc acc;
    uint32_t trips = 0;
    const uint64_t n = src.n_nodes, stride = (uint64_t)gridDim.x * SP_TILE;
    for (uint64_t base = (uint64_t)blockIdx.x * SP_TILE; base < n; base += stride) {  // uniform in the workgroup
        // all loads of the trip first, SP_UNROLL rows a thread: the row pointers, then the first SP_CACHED counts of every
        // row -- two rounds of independent loads in place of 2 * SP_UNROLL dependent ones
        SpCached<Src> row[SP_UNROLL];
#pragma unroll
        for (int u = 0; u < SP_UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * SP_BLOCK + threadIdx.x;
            const uint32_t slots = src.slots(i < n ? i : n - 1);  // a thread behind the last row reads the last row's
            row[u].src = &src;
            row[u].n = i < n ? slots : 0;
        }
#pragma unroll
        for (int u = 0; u < SP_UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * SP_BLOCK + threadIdx.x, i_read = i < n ? i : n - 1;
#pragma unroll
            for (uint32_t j = 0; j < SP_CACHED; ++j) {
                const uint32_t c = src.count_ahead(i_read, j);
                row[u].c[j] = j < row[u].n ? c : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < SP_UNROLL; ++u) {
            const uint64_t i = base + (uint64_t)u * SP_BLOCK + threadIdx.x;
            const bool valid = i < n;
            if constexpr (MODE == 2) {
                const uint32_t mine = row[u].n;
                uint32_t most = mine;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, d, 64));
                uint64_t weight = 0;
                uint32_t deg = 0;
                for (uint32_t j = 0; j < most; ++j) {
                    const uint32_t c = j < mine ? row[u].count(i, j) : 0;
                    const uint64_t b = sp_bin(c, n_bins);
                    if (c) { ++deg; weight += c; acc.max_edge_count = max(acc.max_edge_count, c); }
                    sp_add_combined(s, SP_SLOT_EDGE + (uint32_t)b, sp_in_lds(b), g_edge + b, c != 0);
                }
                acc.sum_edge_counts += weight;
                acc.n_edges += deg;
                acc.max_out_weight = weight > acc.max_out_weight ? weight : acc.max_out_weight;
                const uint64_t wb = sp_bin(weight, n_bins);
                sp_add_combined(s, SP_SLOT_NODE + (uint32_t)wb, sp_in_lds(wb), g_node + wb, valid);
                sp_add_combined(s, SP_SLOT_DEG + deg, true, nullptr, valid);
                if (has_keep) sp_add_combined(s, SP_SLOT_KEPT + (valid ? keep.kept(i) : 0), true, nullptr, valid);
            } else if (valid) {
                struct Sink {
                    uint32_t *s;
                    unsigned long long *g_edge, *g_node;
                    __device__ void add(uint32_t slot, bool in_lds, unsigned long long *g) {
                        if constexpr (MODE == 3) sp_add_leader(s, slot, in_lds, g);
                        else sp_add_plain(s, slot, in_lds, g);
                    }
                    __device__ void edge(uint64_t b) { add(SP_SLOT_EDGE + (uint32_t)b, sp_in_lds(b), g_edge + b); }
                    __device__ void node(uint64_t b) { add(SP_SLOT_NODE + (uint32_t)b, sp_in_lds(b), g_node + b); }
                    __device__ void degree(uint32_t d) { add(SP_SLOT_DEG + d, true, nullptr); }
                } sink{s, g_edge, g_node};
                sp_row(row[u], i, n_bins, acc, sink);
                if (has_keep) sink.add(SP_SLOT_KEPT + keep.kept(i), true, nullptr);
            }
        }
        if (++trips == SP_FLUSH_TRIPS) { sp_flush(s_hist, N_SUB, n_bins, res); trips = 0; }
    }
    sp_flush(s_hist, N_SUB, n_bins, res);
    // sum and maxima: per wave, then one atomic each per workgroup
    const uint64_t w_sum = wave_sum_u64(acc.sum_edge_counts), w_ne = wave_sum_u64(acc.n_edges);
    const uint64_t w_me = sp_wave_max_u64(acc.max_edge_count), w_mw = sp_wave_max_u64(acc.max_out_weight);
    if ((threadIdx.x & 63) == 0) {
        uint64_t *r = s_red[threadIdx.x >> 6];
        r[0] = w_sum; r[1] = w_me; r[2] = w_mw; r[3] = w_ne;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0, me = 0, mw = 0, ne = 0;
        for (int w = 0; w < 4; ++w) {
            sum += s_red[w][0]; ne += s_red[w][3];
            me = s_red[w][1] > me ? s_red[w][1] : me;
            mw = s_red[w][2] > mw ? s_red[w][2] : mw;
        }
        unsigned long long *sc = g_deg + 2 * SP_DEG_BINS;
        if (sum) atomicAdd(&sc[SP_SUM_EDGE_COUNTS], (unsigned long long)sum);
        if (ne) atomicAdd(&sc[SP_N_EDGES], (unsigned long long)ne);
        if (me) atomicMax(&sc[SP_MAX_EDGE_COUNT], (unsigned long long)me);
        if (mw) atomicMax(&sc[SP_MAX_OUT_WEIGHT], (unsigned long long)mw);
    }
}

#endif  // __HIPCC__

}  // namespace dbgk
