// Host check of the plain-C++ helpers that the queries on a graph in parts add to py-debruijn_amd/csrc/dbg_lookup.h: the
// owner rule (lk_owner_of) against the bit arithmetic written out, and the count of one out-edge in a part's CSR
// (lk_csr_count) against a dense table.  Built and run once by tests/test_part_lookup_host.py; includes only that header.
#include "dbg_lookup.h"

#include <cstdio>
#include <vector>

using namespace dbgk;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
#define EXPECT(cond, ...)                                                      \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                      \
    } while (0)

// The owner is the number that the top shard_bits of the 22 hash bits spell, most significant first.
static uint32_t owner_by_bits(uint32_t h, int shard_bits) {
    uint32_t v = 0;
    for (int b = 0; b < shard_bits; ++b) v = v * 2u + ((h >> (21 - b)) & 1u);
    return v;
}

static void test_owner() {
    for (int sb = 0; sb <= 6; ++sb) {
        const uint32_t n_virtual = 1u << sb;
        // the borders of every shard's hash interval, the ends of the hash space, and random hashes
        std::vector<uint32_t> hs = {0u, 1u, (1u << 22) - 1u, (1u << 21), (1u << 21) - 1u};
        for (uint32_t v = 0; v < n_virtual; ++v) {
            const uint32_t lo = v << (22 - sb);
            hs.push_back(lo);
            hs.push_back(lo + ((1u << (22 - sb)) - 1u));
        }
        for (int i = 0; i < 20000; ++i) hs.push_back((uint32_t)rnd() & ((1u << 22) - 1u));
        for (uint32_t h : hs) {
            const uint32_t got = lk_owner_of(h, sb), want = owner_by_bits(h, sb);
            EXPECT(got == want, "shard_bits %d, hash %x: owner %u, expected %u", sb, h, got, want);
            EXPECT(got < n_virtual, "shard_bits %d, hash %x: owner %u is no virtual shard", sb, h, got);
            EXPECT(got == h / ((1u << 22) / n_virtual), "shard_bits %d, hash %x: not the hash interval", sb, h);
        }
    }
}

// CSR rows from a dense table: per node the codes with dense[node][code] != 0 in ascending code order; the arrays are
// exactly as long as the graph needs, so a read past the last row or the last edge is one past an allocation.
static void check_csr(const std::vector<uint32_t> &masks, const char *what) {
    const size_t n = masks.size();
    std::vector<uint32_t> dense(n * 4, 0), row_ptr, ecnt;
    std::vector<uint8_t> flags;
    for (size_t i = 0; i < n; ++i) {
        row_ptr.push_back((uint32_t)ecnt.size());
        for (uint32_t c = 0; c < 4; ++c)
            if ((masks[i] >> c) & 1u) {
                dense[i * 4 + c] = 1u + (uint32_t)(rnd() % 100000);
                ecnt.push_back(dense[i * 4 + c]);
            }
        // bit 0 (indegree) and the bits above the successor mask are not the count's business: set them at random
        flags.push_back((uint8_t)(((rnd() & 1u) | (masks[i] << 1) | ((rnd() & 7u) << 5)) & 0xFFu));
    }
    row_ptr.push_back((uint32_t)ecnt.size());  // the last row ends at n_edges
    row_ptr.shrink_to_fit(); ecnt.shrink_to_fit(); flags.shrink_to_fit();
    for (size_t i = 0; i < n; ++i)
        for (uint32_t c = 0; c < 4; ++c) {
            const uint32_t got = lk_csr_count(flags.data(), row_ptr.data(), ecnt.data(), i, c);
            EXPECT(got == dense[i * 4 + c], "%s: node %zu code %u: %u, expected %u", what, i, c, got, dense[i * 4 + c]);
        }
}

static void test_csr_count() {
    for (uint32_t m = 0; m < 16; ++m) check_csr({m}, "one node");  // first and last node at once, every mask
    {
        std::vector<uint32_t> all;
        for (uint32_t m = 0; m < 16; ++m) all.push_back(m);
        check_csr(all, "masks ascending");
        std::vector<uint32_t> rev(all.rbegin(), all.rend());
        check_csr(rev, "masks descending");  // the last node has no edge: its row is empty and ends at n_edges
    }
    for (uint32_t last = 0; last < 16; ++last)
        for (uint32_t first = 0; first < 16; first += 5) {
            std::vector<uint32_t> masks = {first};
            for (int i = 0; i < 200; ++i) masks.push_back((uint32_t)rnd() & 15u);
            masks.push_back(last);
            check_csr(masks, "random rows");
        }
    check_csr(std::vector<uint32_t>(300, 15u), "every edge");
    check_csr(std::vector<uint32_t>(300, 0u), "no edge");
}

int main() {
    test_owner();
    test_csr_count();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
