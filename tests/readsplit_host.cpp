// The plain-C++ part of csrc/dbg_readsplit.h on the CPU: the keep mask of a word, the start mask from the keep mask, the
// previous byte's keep bit and the read-start bits, and the fold -- against a byte-by-byte statement of the definition
//   keep(p)  = the byte at p, folded if asked, is one of ACGT
//   start(p) = keep(p) && (p == 0 || !keep(p - 1) || a read starts at p)
// over buffers of several words, so that every word sees both values of the carry.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dbg_readsplit.h"

using namespace dbgk;

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++failures;                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
        }                                                   \
    } while (0)

// the definition, one byte at a time
static bool ref_keep(unsigned char c, bool fold) {
    if (fold && (c == 'a' || c == 'c' || c == 'g' || c == 't')) c = (unsigned char)(c - 'a' + 'A');
    return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}

// checks every word of `buf` (read starts at the positions in `rs`) with the helpers, under both fold settings
static void check_buffer(const std::vector<unsigned char> &buf, const std::vector<bool> &rs, const char *what) {
    const size_t n = buf.size();
    for (int fold = 0; fold < 2; ++fold) {
        for (size_t p0 = 0; p0 < n; p0 += RS_WORD_BYTES) {
            const int nb = n - p0 >= (size_t)RS_WORD_BYTES ? RS_WORD_BYTES : (int)(n - p0);
            uint32_t v[RS_WORD_BYTES / 4] = {0};
            uint64_t rbits = 0, want_keep = 0, want_start = 0, want_folded = 0;
            for (int i = 0; i < nb; ++i) {
                const unsigned char c = buf[p0 + i];
                v[i >> 2] |= (uint32_t)c << (8 * (i & 3));
                if (rs[p0 + i]) rbits |= 1ull << i;
                const size_t p = p0 + i;
                const bool k = ref_keep(c, fold != 0);
                const bool st = k && (p == 0 || !ref_keep(buf[p - 1], fold != 0) || rs[p]);
                if (k) want_keep |= 1ull << i;
                if (st) want_start |= 1ull << i;
                if (k && !ref_keep(c, false)) want_folded |= 1ull << i;
            }
            uint64_t folded = ~0ull;
            const uint64_t keep = rs_keep_mask(v, nb, fold != 0, &folded);
            const uint32_t prev = p0 ? (uint32_t)rs_keep(buf[p0 - 1], fold != 0) : 0u;
            const uint64_t start = rs_start_mask(keep, prev, rbits);
            EXPECT(keep == want_keep, "%s fold %d word %zu: keep %016llx want %016llx", what, fold, p0 / RS_WORD_BYTES,
                   (unsigned long long)keep, (unsigned long long)want_keep);
            EXPECT(folded == want_folded, "%s fold %d word %zu: folded %016llx want %016llx", what, fold, p0 / RS_WORD_BYTES,
                   (unsigned long long)folded, (unsigned long long)want_folded);
            EXPECT(start == want_start, "%s fold %d word %zu: start %016llx want %016llx", what, fold, p0 / RS_WORD_BYTES,
                   (unsigned long long)start, (unsigned long long)want_start);
        }
    }
}

static std::vector<unsigned char> bases(size_t n) {
    std::vector<unsigned char> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = (unsigned char)"ACGT"[(i * 7 + i / 5) & 3];
    return b;
}

int main() {
    const size_t W = RS_WORD_BYTES;
    static_assert(RS_WORD_BYTES == 64, "the masks are 64 bits wide");
    static_assert(RS_BLOCK_BYTES == 256 * RS_WORDS_PER_THREAD * RS_WORD_BYTES, "block = 256 threads of words");
    static_assert(RS_ROUND_BYTES == (uint64_t)RS_ROUND_BLOCKS * RS_BLOCK_BYTES, "round = blocks of the carry kernel");

    // the fold and the byte classes, all 256 bytes
    for (unsigned c = 0; c < 256; ++c) {
        unsigned want = c;
        if (c == 'a' || c == 'c' || c == 'g' || c == 't') want = c - 'a' + 'A';
        EXPECT(rs_fold(c) == want, "fold of byte %u: %u want %u", c, rs_fold(c), want);
        EXPECT(rs_keep(c, false) == ref_keep((unsigned char)c, false), "keep of byte %u", c);
        EXPECT(rs_keep(c, true) == ref_keep((unsigned char)c, true), "keep under fold of byte %u", c);
        EXPECT(rs_is_acgt(c) == (c == 'A' || c == 'C' || c == 'G' || c == 'T'), "is_acgt of byte %u", c);
    }

    // one cut byte at every bit of the middle word of three: bit 0 (the carry into the word is set, the carry into the next
    // word too), the last bit (the carry into the next word is clear), and everything between; each cut byte in turn an
    // 'N', a lower-case base (a cut without the fold, kept with it), a byte >= 0x80 and a zero
    const unsigned char cuts[] = {'N', 'g', 0xC1, 0x00, 0xFF, 'n', '>'};
    for (unsigned char cut : cuts)
        for (size_t bit = 0; bit < W; ++bit) {
            std::vector<unsigned char> b = bases(3 * W);
            std::vector<bool> rs(3 * W, false);
            rs[0] = true;
            b[W + bit] = cut;
            check_buffer(b, rs, "one cut");
        }

    // a read start on a kept byte, on a cut byte and after a cut byte, at every bit (and so across the word border)
    for (size_t bit = 0; bit < W; ++bit) {
        for (int kind = 0; kind < 3; ++kind) {
            std::vector<unsigned char> b = bases(3 * W);
            std::vector<bool> rs(3 * W, false);
            rs[0] = true;
            const size_t p = W + bit;
            rs[p] = true;                     // kind 0: on a kept byte between kept bytes -- the pieces must not merge
            if (kind == 1) b[p] = 'N';        // on a cut byte
            if (kind == 2) b[p - 1] = 'N';    // after a cut byte
            check_buffer(b, rs, kind == 0 ? "start on kept" : kind == 1 ? "start on cut" : "start after cut");
        }
    }

    // runs of cuts over the word border, all-cut words, all-lower-case words, a tail that is no whole word
    for (size_t len : {W - 1, W, W + 1, 2 * W, 2 * W + 17, (size_t)1, (size_t)5}) {
        std::vector<unsigned char> b = bases(len);
        std::vector<bool> rs(len, false);
        rs[0] = true;
        check_buffer(b, rs, "plain");
        if (len > W) { b[W - 1] = 'N'; b[W] = 'N'; if (len > W + 1) b[W + 1] = 'N'; }
        check_buffer(b, rs, "run over the border");
        for (auto &c : b) c = 'N';
        check_buffer(b, rs, "all cut");
        for (size_t i = 0; i < len; ++i) b[i] = (unsigned char)"acgt"[i & 3];
        check_buffer(b, rs, "all lower case");
        b[len - 1] = 0x80;
        check_buffer(b, rs, "cut at the last byte");
    }

    // pseudo-random bytes over the whole byte range with dense read starts
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int round = 0; round < 200; ++round) {
        const size_t len = 1 + rnd() % (4 * W);
        std::vector<unsigned char> b(len);
        std::vector<bool> rs(len, false);
        const unsigned mode = (unsigned)(rnd() % 3);
        for (size_t i = 0; i < len; ++i) {
            const uint64_t r = rnd();
            b[i] = mode == 0 ? (unsigned char)r : (unsigned char)"ACGTacgtN\xC1"[r % (mode == 1 ? 10 : 5)];
            rs[i] = (r >> 32) % 9 == 0;
        }
        rs[0] = true;
        check_buffer(b, rs, "random");
    }

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("readsplit_host ok\n");
    return 0;
}
