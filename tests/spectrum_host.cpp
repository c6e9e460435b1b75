// The plain-C++ part of csrc/dbg_spectrum.h on the CPU, against the rule stated without arithmetic tricks:
//   a count c lands in bin c if c < B - 1, else in bin B - 1; a bin is kept in LDS iff it is below SP_LDS_BINS;
//   degree = bits 1..4 of the build's flag byte, kept degree = bits 1..4 of the pruned flag byte or the bits of the mask;
//   a row of a CSR is ecnt[rowptr[i] .. rowptr[i + 1]) and the last row ends at n_edges; a dense row is its D counters,
//   a zero being no edge.
// The rows are also taken the way the kernel takes them: slots and the first SP_CACHED counts loaded ahead without a branch
// (SpCached, count_ahead), threads behind the last row included.
// The arrays have exactly the promised sizes -- n_nodes row pointers, not n_nodes + 1, and max(n_edges, 1) counts -- so a
// sanitizer sees every access beyond them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dbg_spectrum.h"

using namespace dbgk;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            ++g_fail;                                      \
        }                                                  \
    } while (0)

static uint64_t g_rng = 0x13198A2E03707344ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

static uint64_t bin_rule(uint64_t c, uint64_t B) {
    if (c < B - 1) return c;
    return B - 1;
}

static void test_bins() {
    const uint64_t Bs[] = {2, 3, 4096, 1ull << 20};
    for (uint64_t B : Bs) {
        const uint64_t cs[] = {0, 1, B - 2, B - 1, B, 0xFFFFFFFFull};
        for (uint64_t c : cs) {
            CHECK(sp_bin(c, B) == bin_rule(c, B), "bin c=%llu B=%llu", (unsigned long long)c, (unsigned long long)B);
            CHECK(sp_bin(c, B) < B, "bin in range c=%llu B=%llu", (unsigned long long)c, (unsigned long long)B);
        }
        CHECK(sp_bin(0xFFFFFFFFull * 32, B) == B - 1, "a 37-bit out-weight clamps");
    }
    CHECK(SP_MAX_BINS == (1ull << 20), "most bins");
    // the LDS / tail split: the border and one either side
    CHECK(sp_in_lds(SP_LDS_BINS - 2) && sp_in_lds(SP_LDS_BINS - 1), "below the border");
    CHECK(!sp_in_lds(SP_LDS_BINS) && !sp_in_lds(SP_LDS_BINS + 1), "at and above the border");
    CHECK(sp_in_lds(0) && !sp_in_lds(SP_MAX_BINS - 1), "ends");
    // every LDS slot the kernel can name lies inside the histogram
    CHECK(SP_SLOT_EDGE + SP_LDS_BINS - 1 < SP_SLOT_NODE && SP_SLOT_NODE + SP_LDS_BINS - 1 < SP_SLOT_DEG, "slots");
    CHECK(SP_SLOT_DEG + 32 < SP_SLOT_KEPT && SP_SLOT_KEPT + 32 < SP_SLOTS, "degree slots");
    CHECK(sp_result_words(2) == 4 + 66 + SP_SCALARS && sp_result_words(1ull << 20) * 8 <= 16 * (1ull << 20) + 65536, "result size");
}

static uint32_t bits_rule(uint32_t m) {
    uint32_t n = 0;
    for (int b = 0; b < 32; ++b) n += (m >> b) & 1u;
    return n;
}

static void test_degrees() {
    for (uint32_t f = 0; f < 256; ++f) {
        const uint32_t want = ((f >> 1) & 1u) + ((f >> 2) & 1u) + ((f >> 3) & 1u) + ((f >> 4) & 1u);
        CHECK(sp_degree_from_flags(f) == want, "degree of flag byte %u", f);
        CHECK(sp_kept_from_flags(f) == want, "kept degree of flag byte %u", f);  // indegree, branch, pulled and mark bits do not count
    }
    CHECK(sp_kept_from_mask(0) == 0 && sp_kept_from_mask(0xFFFFFFFFu) == 32, "empty and full mask");
    for (int b = 0; b < 32; ++b) CHECK(sp_kept_from_mask(1u << b) == 1, "one bit %d", b);
    for (int t = 0; t < 2000; ++t) {
        uint32_t m = 0;
        while (bits_rule(m) < 20) m |= 1u << (rnd() & 31u);
        CHECK(sp_kept_from_mask(m) == 20, "twenty bits %08x", m);
        const uint32_t any = rnd();
        CHECK(sp_kept_from_mask(any) == bits_rule(any), "mask %08x", any);
    }
    const uint8_t fl[3] = {0x1F, 0x41, 0x2B};
    const uint32_t mk[3] = {0, 0xF0F0F0F0u, 7};
    const SpKeep kf{fl, nullptr}, km{nullptr, mk}, none{nullptr, nullptr};
    CHECK(kf.any() && km.any() && !none.any(), "keep sources");
    CHECK(kf.kept(0) == 4 && kf.kept(1) == 0 && kf.kept(2) == 2, "kept from flags");  // 0x2B: bits 1 and 3
    CHECK(km.kept(0) == 0 && km.kept(1) == 16 && km.kept(2) == 3, "kept from masks");
}

struct Hists {
    uint64_t B;
    std::vector<uint64_t> E, W, D;
    explicit Hists(uint64_t b) : B(b), E(b, 0), W(b, 0), D(33, 0) {}
    void edge(uint64_t b) { CHECK(b < B, "edge bin"); if (b < B) ++E[b]; }
    void node(uint64_t b) { CHECK(b < B, "node bin"); if (b < B) ++W[b]; }
    void degree(uint32_t d) { CHECK(d <= 32, "degree"); if (d <= 32) ++D[d]; }
    bool operator==(const Hists &o) const { return E == o.E && W == o.W && D == o.D; }
};

// rows[i]: the non-zero counts of node i -> the histograms by the rule
static Hists rule(const std::vector<std::vector<uint32_t>> &rows, uint64_t B, SpAcc *acc) {
    Hists h(B);
    *acc = SpAcc();
    for (const auto &r : rows) {
        uint64_t w = 0;
        for (uint32_t c : r) {
            ++h.E[bin_rule(c, B)];
            w += c;
            acc->sum_edge_counts += c;
            if (c > acc->max_edge_count) acc->max_edge_count = c;
        }
        acc->n_edges += r.size();
        if (w > acc->max_out_weight) acc->max_out_weight = w;
        ++h.W[bin_rule(w, B)];
        ++h.D[r.size()];
    }
    return h;
}
static bool same(const SpAcc &a, const SpAcc &b) {
    return a.sum_edge_counts == b.sum_edge_counts && a.max_out_weight == b.max_out_weight && a.n_edges == b.n_edges &&
           a.max_edge_count == b.max_edge_count;
}

// the rows as the kernel takes them: slots and the first SP_CACHED counts loaded ahead without a branch (a thread behind the
// last row reads the last row's), the rest of a long row through the source
template <class Src>
static void cached_rows(const Src &src, const std::vector<std::vector<uint32_t>> &rows, uint64_t B, const Hists &want,
                        const SpAcc &want_acc, const char *what) {
    const uint64_t n = src.n_nodes;
    if (!n) return;
    Hists got(B);
    SpAcc acc;
    for (uint64_t i = 0; i < n + 3; ++i) {
        const uint64_t i_read = i < n ? i : n - 1;
        SpCached<Src> row;
        row.src = &src;
        const uint32_t slots = src.slots(i_read);
        row.n = i < n ? slots : 0;
        for (uint32_t j = 0; j < SP_CACHED; ++j) {
            const uint32_t c = src.count_ahead(i_read, j);
            if (j < slots) CHECK(c == src.count(i_read, j), "%s: count_ahead inside the row", what);
            row.c[j] = j < row.n ? c : 0;
        }
        if (i >= n) { CHECK(row.slots(i) == 0, "%s: a thread behind the last row has no row", what); continue; }
        (void)rows;
        sp_row(row, i, B, acc, got);
    }
    CHECK(got == want, "%s: histograms through the cached rows", what);
    CHECK(same(acc, want_acc), "%s: sum and maxima through the cached rows", what);
}

template <class RP>
static void csr_case(const std::vector<std::vector<uint32_t>> &rows, uint64_t B, const char *what) {
    // exact sizes on the heap: n row pointers and n_edges counts
    const uint64_t n = rows.size();
    uint64_t ne = 0;
    for (const auto &r : rows) ne += r.size();
    RP *rp = (RP *)malloc(n ? n * sizeof(RP) : 1);
    uint32_t *ec = (uint32_t *)malloc(ne ? ne * 4 : 4);  // at least one readable word: the kernel's look-ahead reads ecnt[0] beyond a row
    if (!ne) ec[0] = 0xDEADBEEFu;
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        rp[i] = (RP)at;
        for (uint32_t c : rows[i]) ec[at++] = c;
    }
    const SpCsr<RP> src{rp, ec, n, ne};
    Hists got(B);
    SpAcc acc, want_acc;
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(src.slots(i) == rows[i].size(), "%s: slots of row %llu", what, (unsigned long long)i);
        for (uint32_t j = 0; j < src.slots(i); ++j) CHECK(src.count(i, j) == rows[i][j], "%s: count", what);
        sp_row(src, i, B, acc, got);
    }
    const Hists want = rule(rows, B, &want_acc);
    CHECK(got == want, "%s: histograms (%d-bit row pointers, B=%llu)", what, (int)sizeof(RP) * 8, (unsigned long long)B);
    CHECK(same(acc, want_acc), "%s: sum and maxima", what);
    cached_rows(src, rows, B, want, want_acc, what);
    free(rp);
    free(ec);
}

template <int D>
static void dense_case(uint64_t n, uint64_t B, uint32_t fill_pct, uint32_t max_count) {
    uint32_t *cnt = (uint32_t *)malloc(n ? n * D * 4 : 1);
    std::vector<std::vector<uint32_t>> rows(n);
    for (uint64_t i = 0; i < n; ++i)
        for (int j = 0; j < D; ++j) {
            const uint32_t c = rnd() % 100 < fill_pct ? 1 + rnd() % max_count : 0;
            cnt[i * D + j] = c;
            if (c) rows[i].push_back(c);
        }
    const SpDense<D> src{cnt, n, 0};
    Hists got(B);
    SpAcc acc, want_acc;
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(src.slots(i) == (uint32_t)D, "dense slots");
        sp_row(src, i, B, acc, got);
    }
    const Hists want = rule(rows, B, &want_acc);
    CHECK(got == want, "dense D=%d B=%llu fill=%u", D, (unsigned long long)B, fill_pct);
    CHECK(same(acc, want_acc), "dense D=%d: sum and maxima", D);
    cached_rows(src, rows, B, want, want_acc, "dense");
    free(cnt);
}

static void test_rows() {
    using Rows = std::vector<std::vector<uint32_t>>;
    const Rows small = {{3}, {}, {1, 2, 0xFFFFFFFFu, 7}, {}, {}, {5, 5}, {9}};           // empty rows, a last row ending at n_edges
    const Rows ends_empty = {{1}, {2, 2}, {}};                                            // the last row empty: it begins at n_edges
    const Rows all_empty = {{}, {}, {}};
    const Rows none = {};
    const Rows one = {{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}};              // an out-weight beyond 32 bits
    Rows wide(5);
    for (uint32_t j = 0; j < 32; ++j) wide[1].push_back(1 + j);                           // a full generic row
    for (uint32_t j = 0; j < 20; ++j) wide[4].push_back(1000 + j);
    const uint64_t Bs[] = {2, 3, 4, 64, 4096, 1ull << 20};
    for (uint64_t B : Bs) {
        csr_case<uint32_t>(small, B, "small"); csr_case<uint64_t>(small, B, "small");
        csr_case<uint32_t>(ends_empty, B, "ends_empty"); csr_case<uint64_t>(ends_empty, B, "ends_empty");
        csr_case<uint32_t>(all_empty, B, "all_empty"); csr_case<uint64_t>(all_empty, B, "all_empty");
        csr_case<uint32_t>(none, B, "none"); csr_case<uint64_t>(none, B, "none");
        csr_case<uint32_t>(one, B, "one"); csr_case<uint64_t>(one, B, "one");
        csr_case<uint32_t>(wide, B, "wide"); csr_case<uint64_t>(wide, B, "wide");
    }
    for (int t = 0; t < 50; ++t) {
        Rows r(1 + rnd() % 40);
        for (auto &row : r) {
            const uint32_t d = rnd() % 5;
            for (uint32_t j = 0; j < d; ++j) row.push_back(1 + rnd() % (t % 2 ? 20 : 5000));
        }
        csr_case<uint32_t>(r, t % 3 ? 64 : 4, "random");
        csr_case<uint64_t>(r, t % 3 ? 64 : 4, "random");
    }
    for (uint64_t B : Bs) {
        dense_case<4>(0, B, 50, 10); dense_case<32>(0, B, 50, 10);
        dense_case<4>(37, B, 0, 10); dense_case<32>(11, B, 0, 10);       // no edge anywhere
        dense_case<4>(37, B, 100, 3); dense_case<32>(11, B, 100, 3);     // every slot an edge
        dense_case<4>(200, B, 40, 70000); dense_case<32>(60, B, 30, 70000);
        dense_case<4>(9, B, 60, 0xFFFFFFFFu); dense_case<32>(9, B, 60, 0xFFFFFFFFu);
    }
}

int main() {
    test_bins();
    test_degrees();
    test_rows();
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
