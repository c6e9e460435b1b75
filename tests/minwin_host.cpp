// Host check of the per-lane arithmetic of the register extraction (py-debruijn_amd/csrc/dbg_minwin.h), built and run once
// by tests/test_extract_shared_hashes.py.  Includes only that header.
//   window_min32<W>   against the naive leftmost minimum of W packed values, W = 1, 2, 9, 18, 19
//   record_starts     against the rule taken position by position
#include "dbg_minwin.h"

#include <cstdio>
#include <cstdlib>

using namespace dbgk;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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

static long min_in_neighbour = 0;    // window minima found at index >= 32
static long start0_by_prev = 0;      // starts at position 0 that the predecessor byte decided

// ---- window minima ---------------------------------------------------------------------------------------------------
enum Fill { RANDOM, FEW_HASHES, MIN_IN_NEIGHBOUR };

template <int W>
static void check_minima(Fill fill, int rounds) {
    constexpr int NV = 32 + W - 1;
    for (int r = 0; r < rounds; ++r) {
        uint32_t pv[NV], mn[32];
        uint32_t few[3] = {(uint32_t)rnd() & 0xFFFFu, (uint32_t)rnd() & 0xFFFFu, (uint32_t)rnd() & 0xFFFFu};
        const int n_few = 2 + (int)(rnd() % 2);
        for (int i = 0; i < NV; ++i) {
            uint32_t h;
            if (fill == FEW_HASHES) h = few[rnd() % n_few];
            else if (fill == MIN_IN_NEIGHBOUR) h = (i >= 32) ? (uint32_t)(rnd() % 0x1000u) : 0x1000u + (uint32_t)(rnd() % 0xF000u);
            else h = (uint32_t)rnd() & 0xFFFFu;
            pv[i] = (h << 8) | (uint32_t)i;
        }
        if (r % 7 == 0) {  // the packed value of a real m-mer, so that mmer_packed is what the arrays are made of
            const uint32_t mm = (uint32_t)rnd() & ((1u << 26) - 1);
            pv[r % NV] = mmer_packed(mm, (uint32_t)(r % NV));
            EXPECT(pv[r % NV] == ((((mm ^ (mm >> 9) ^ 0x3C6EF372u) * 0x9E3779B1u) >> 16) << 16 | (uint32_t)(r % NV)), "mmer_packed");
        }
        window_min32<W>(pv, mn);
        for (int q = 0; q < 32; ++q) {
            int best = q;  // leftmost minimum of the hashes alone
            for (int i = q + 1; i < q + W; ++i)
                if ((pv[i] >> 8) < (pv[best] >> 8)) best = i;
            EXPECT(mn[q] == pv[best], "W %d fill %d round %d q %d: got index %u hash %u, want index %d hash %u", W, (int)fill, r, q,
                   mn[q] & 0xFFu, mn[q] >> 8, best, pv[best] >> 8);
            if (best >= 32) ++min_in_neighbour;
        }
    }
}

// ---- record starts ---------------------------------------------------------------------------------------------------
// off[q]: offset of the minimizer from position q (0 .. W - 1), valid where bit q of vmask is set.  prev_off: the offset at the
// previous lane's position 31, -1 = no k-mer there.  The rule: q starts a record iff it holds a k-mer and the position
// before it holds none or has another minimizer occurrence, that is prev != off[q] + 1.
template <int W>
static void check_starts_case(const int (&off)[32], uint32_t vmask, int prev_off) {
    uint32_t want = 0;
    for (int q = 0; q < 32; ++q) {
        const bool v = (vmask >> q) & 1u;
        const bool pv_valid = q ? ((vmask >> (q - 1)) & 1u) : (prev_off >= 0);
        const int p = q ? off[q - 1] : prev_off;
        if (v && (!pv_valid || p != off[q] + 1)) want |= 1u << q;
    }
    // the helper's inputs: window minima whose low byte is the index q + off[q] (the hash bits above it must not matter)
    uint32_t mn[32], D[8];
    for (int q = 0; q < 32; ++q) mn[q] = ((uint32_t)rnd() << 8) | (uint32_t)(q + off[q]);
    pack_index_bytes(mn, vmask, D);
    for (int q = 0; q < 32; ++q) {
        const uint32_t byte = (D[index_byte_at(q) >> 2] >> (8 * (index_byte_at(q) & 3))) & 0xFFu;
        EXPECT(((vmask >> q) & 1u) ? byte == (uint32_t)(q + off[q]) : (byte & MW_NO_KMER) != 0 && byte < 0x80u, "index byte of %d: %u", q, byte);
    }
    // the previous lane's edge byte, made the way the kernel makes it: from that lane's own packed bytes
    uint32_t Dp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Dp[7] = (prev_off >= 0 ? (uint32_t)(31 + prev_off) : MW_NO_KMER | (uint32_t)(31 + rnd() % W)) << 24;
    const uint32_t prev_byte = edge_index_byte(Dp);
    const uint32_t got = record_starts(D, prev_byte, vmask);
    EXPECT(got == want, "W %d vmask %08x prev %d: starts %08x, want %08x", W, vmask, prev_off, got, want);
    if ((vmask & 1u) && prev_off >= 0) ++start0_by_prev;
}

template <int W>
static void check_starts(int rounds) {
    int off[32];
    for (int r = 0; r < rounds; ++r) {  // random: runs of a shared occurrence (offset falls by one) broken at random
        const int mode = r % 4;
        for (int q = 0; q < 32; ++q) {
            if (mode == 0) off[q] = (int)(rnd() % W);
            else off[q] = (q && off[q - 1] > 0 && rnd() % 4) ? off[q - 1] - 1 : (int)(rnd() % W);
        }
        const uint32_t vmask = (mode == 3) ? (uint32_t)rnd() | (uint32_t)rnd() : (uint32_t)rnd();
        int prev_off = (int)(rnd() % (W + 1)) - 1;
        if (r % 3 == 0 && off[0] + 1 < W) prev_off = off[0] + 1;  // the predecessor byte says "same occurrence"
        check_starts_case<W>(off, vmask, prev_off);
    }
    const uint32_t masks[4] = {0u, 0xFFFFFFFFu, 0x55555555u, 0x80000001u};
    for (uint32_t vmask : masks)
        for (int fill = 0; fill < 3; ++fill)
            for (int prev_off = -1; prev_off < W; ++prev_off) {
                // all offsets 0, all W - 1, and the longest run W - 1, W - 2, .. 0 repeated
                for (int q = 0; q < 32; ++q) off[q] = fill == 0 ? 0 : fill == 1 ? W - 1 : W - 1 - q % W;
                check_starts_case<W>(off, vmask, prev_off);
            }
}

template <int W>
static void check_w() {
    check_minima<W>(RANDOM, 400);
    check_minima<W>(FEW_HASHES, 400);
    check_minima<W>(MIN_IN_NEIGHBOUR, 100);
    check_starts<W>(600);
}

int main() {
    check_w<1>();
    check_w<2>();
    check_w<9>();
    check_w<18>();
    check_w<19>();
    std::printf("window minima at index >= 32: %ld, starts at position 0 decided by the predecessor byte: %ld\n", min_in_neighbour,
                start0_by_prev);
    EXPECT(min_in_neighbour >= 1000, "too few minima in the neighbour's part");
    EXPECT(start0_by_prev >= 1000, "too few position-0 cases");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
