// The plain-C++ part of csrc/dbg_revcomp.h on the CPU, against the rule stated byte by byte:
//   out[2 o[i] + j] = in[o[i] + j],  out[2 o[i] + len_i + j] = comp(in[o[i] + len_i - 1 - j])
// comp on 1, 4, 8 and 16 packed bytes over all 256 byte values, the byte reversal, the 16-byte window at every shift, the
// mapping output position -> (read, strand, source) over runs of empty reads, and the whole 16-byte chunk routine the
// tile kernel calls, tile by tile as the kernel walks them, with the offsets slice it keeps and with the global search
// it falls back to.  The input buffers have exactly the size the library promises (N for a lent buffer, N + 64 for an
// owned one) and the slice exactly RC_SLICE_READS + 1 entries, so a sanitizer sees every access beyond them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dbg_revcomp.h"

using namespace dbgk;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            ++g_fail;                                      \
        }                                                  \
    } while (0)

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// the rule, with no arithmetic
static uint8_t comp_rule(uint8_t c) {
    switch (c) {
        case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
        case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
        default: return c;
    }
}

static void test_comp() {
    for (uint32_t c = 0; c < 256; ++c) {
        CHECK(rc_comp1(c) == comp_rule((uint8_t)c), "comp1 %u", c);
        for (int lane = 0; lane < 4; ++lane) {
            const uint32_t noise = rnd(), sh = 8 * lane;
            const uint32_t v = (noise & ~(0xFFu << sh)) | (c << sh);
            uint32_t moved = 0;
            const uint32_t r = rc_comp4(v, &moved);
            for (int b = 0; b < 4; ++b) {
                const uint8_t in = (uint8_t)(v >> (8 * b)), want = comp_rule(in);
                CHECK((uint8_t)(r >> (8 * b)) == want, "comp4 byte %u lane %d", c, b);
                CHECK(((moved >> (8 * b)) & 0xFFu) == (want != in ? 0x80u : 0u), "comp4 moved %u lane %d", c, b);
            }
        }
        for (int lane = 0; lane < 8; ++lane) {
            const uint64_t noise = ((uint64_t)rnd() << 32) | rnd();
            const uint64_t v = (noise & ~(0xFFull << (8 * lane))) | ((uint64_t)c << (8 * lane));
            const uint64_t r = rc_comp8(v);
            for (int b = 0; b < 8; ++b)
                CHECK((uint8_t)(r >> (8 * b)) == comp_rule((uint8_t)(v >> (8 * b))), "comp8 byte %u lane %d", c, b);
        }
        for (int lane = 0; lane < 16; ++lane) {
            uint8_t bytes[16];
            for (int b = 0; b < 16; ++b) bytes[b] = (uint8_t)rnd();
            bytes[lane] = (uint8_t)c;
            uint32_t v[4];
            memcpy(v, bytes, 16);
            const int other16 = rc_other16(v);
            const int other = rc_comp16(v);
            uint8_t got[16];
            memcpy(got, v, 16);
            int want_other = 0;
            for (int b = 0; b < 16; ++b) {
                CHECK(got[b] == comp_rule(bytes[b]), "comp16 byte %u lane %d", c, b);
                want_other += comp_rule(bytes[b]) == bytes[b];
            }
            CHECK(other == want_other && other16 == want_other, "comp16 count %d %d != %d", other, other16, want_other);
        }
    }
}

static void test_reverse_and_extract() {
    uint8_t w8[32];
    for (int i = 0; i < 32; ++i) w8[i] = (uint8_t)(i * 7 + 3);
    uint32_t w[8];
    memcpy(w, w8, 32);
    for (uint32_t s = 0; s < 16; ++s) {
        uint32_t out[4];
        rc_extract16(w, s, out);
        uint8_t got[16];
        memcpy(got, out, 16);
        for (int b = 0; b < 16; ++b) CHECK(got[b] == w8[s + b], "extract16 shift %u byte %d", s, b);
        rc_reverse16(out);
        memcpy(got, out, 16);
        for (int b = 0; b < 16; ++b) CHECK(got[b] == w8[s + 15 - b], "reverse16 shift %u byte %d", s, b);
    }
}

struct ReadSet {
    std::vector<std::string> reads;
    std::vector<uint64_t> off;
    std::string in;        // concatenated
    std::string want;      // the rule applied
    std::vector<uint64_t> want_read, want_src;  // per output byte
    std::vector<uint32_t> want_strand;
    uint64_t want_other = 0;
    void finish() {
        off.assign(1, 0);
        for (auto &r : reads) { in += r; off.push_back(in.size()); }
        for (size_t i = 0; i < reads.size(); ++i) {
            const std::string &r = reads[i];
            for (size_t j = 0; j < r.size(); ++j) {
                want.push_back(r[j]);
                want_read.push_back(i); want_strand.push_back(0); want_src.push_back(off[i] + j);
                want_other += comp_rule((uint8_t)r[j]) == (uint8_t)r[j];
            }
            for (size_t j = 0; j < r.size(); ++j) {
                want.push_back((char)comp_rule((uint8_t)r[r.size() - 1 - j]));
                want_read.push_back(i); want_strand.push_back(1); want_src.push_back(off[i] + r.size() - 1 - j);
            }
        }
    }
};

static std::string random_read(size_t len, const char *alphabet, size_t na) {
    std::string r(len, 'A');
    for (auto &c : r) c = alphabet[rnd() % na];
    return r;
}

// the tile kernel's walk over the output, one thread at a time.  pad: bytes the input buffer has behind its last base.
static void run_pass(const ReadSet &rs, const char *name, uint64_t pad) {
    const uint64_t n = rs.in.size(), n2 = 2 * n, n_reads = rs.reads.size();
    if (!n2) return;
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, n + pad) != 0) { CHECK(false, "posix_memalign"); return; }
    char *in = (char *)mem;
    memcpy(in, rs.in.data(), n);
    memset(in + n, 0xEE, pad);
    std::vector<uint8_t> out(((n2 + 15) / 16) * 16, 0xCC);
    uint64_t other = 0;
    for (uint64_t t0 = 0; t0 < n2; t0 += RC_TILE_BYTES) {
        const uint64_t t1 = t0 + RC_TILE_BYTES < n2 ? t0 + RC_TILE_BYTES : n2;
        uint64_t i0 = 0, hi = n_reads;
        while (hi - i0 > 1) {
            const uint64_t mid = i0 + (hi - i0) / 2;
            if (2 * rs.off[mid] <= t0) i0 = mid; else hi = mid;
        }
        const uint64_t cnt = n_reads - i0 < (uint64_t)RC_SLICE_READS ? n_reads - i0 : (uint64_t)RC_SLICE_READS;
        std::vector<uint64_t> slice(rs.off.begin() + i0, rs.off.begin() + i0 + cnt + 1);  // exactly what the kernel keeps
        uint64_t n_in = 0;  // reads of the slice that begin in front of the tile's end
        while (n_in <= cnt && 2 * slice[n_in] < t1) ++n_in;
        const bool in_slice = n_in <= cnt;
        for (uint64_t q = t0; q < t1; q += RC_CHUNK_BYTES) {
            uint32_t v[4], v2[4];
            // the global search always has to work; the slice where it covers the tile
            const uint32_t o2 = rc_make_chunk(in, n + pad, rs.off.data(), i0, n_reads, q, n2, v2);
            uint32_t o1 = o2;
            memcpy(v, v2, 16);
            if (in_slice) o1 = rc_make_chunk(in, n + pad, slice.data(), 0, n_in, q, n2, v);
            CHECK(o1 == o2 && !memcmp(v, v2, 16), "%s: slice and global search differ at %llu", name, (unsigned long long)q);
            memcpy(&out[q], v, 16);
            other += o1;
            // the mapping itself, byte by byte
            RcPlace p = rc_locate(rs.off.data(), i0, n_reads, q);
            for (uint64_t b = 0; b < 16 && q + b < n2; ++b) {
                if (b && q + b == p.seg_end) p = rc_next_strand(rs.off.data(), n_reads, p);  // the next strand's first byte
                else if (b) p.src = p.strand ? p.src - 1 : p.src + 1;
                const RcPlace d = rc_locate(rs.off.data(), 0, n_reads, q + b);
                CHECK(p.read == rs.want_read[q + b] && p.strand == rs.want_strand[q + b] && p.src == rs.want_src[q + b],
                      "%s: walk to %llu", name, (unsigned long long)(q + b));
                CHECK(d.read == rs.want_read[q + b] && d.strand == rs.want_strand[q + b] && d.src == rs.want_src[q + b],
                      "%s: locate %llu", name, (unsigned long long)(q + b));
            }
        }
    }
    for (uint64_t q = 0; q < out.size(); ++q) {
        const uint8_t want = q < n2 ? (uint8_t)rs.want[q] : 0;  // the padding behind the last read is zero
        CHECK(out[q] == want, "%s: pad %llu: out[%llu] = %u, not %u", name, (unsigned long long)pad, (unsigned long long)q,
              out[q], want);
    }
    CHECK(other == rs.want_other, "%s: other %llu != %llu", name, (unsigned long long)other, (unsigned long long)rs.want_other);
    free(mem);
}

static void run_both(const ReadSet &rs, const char *name) {
    run_pass(rs, name, 0);   // a lent buffer: nothing behind the last base
    run_pass(rs, name, 64);  // an owned one
}

int main() {
    test_comp();
    test_reverse_and_extract();
    const char dna[] = "ACGT";
    const char mixed[] = "ACGTacgtNnRYKM-*\x80\xC1\xE1\xFF\x01";
    const char pep[] = "ACDEFGHIKLMNPQRSTVWY";
    // every length at every source alignment, with and without a tail behind it
    const size_t lens[] = {0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33};
    for (size_t len : lens)
        for (size_t align = 0; align < 16; ++align)
            for (int tail = 0; tail < 3; ++tail) {
                ReadSet rs;
                if (align) rs.reads.push_back(random_read(align, mixed, sizeof(mixed) - 1));
                rs.reads.push_back(random_read(len, tail == 1 ? mixed : dna, tail == 1 ? sizeof(mixed) - 1 : 4));
                if (tail) rs.reads.push_back(random_read(tail == 1 ? 7 : 40, mixed, sizeof(mixed) - 1));
                rs.finish();
                char name[64];
                snprintf(name, sizeof name, "len %zu align %zu tail %d", len, align, tail);
                run_both(rs, name);
            }
    {  // runs of empty reads, longer than the slice, around one short read; and at both ends of the set
        ReadSet rs;
        for (int i = 0; i < 3000; ++i) rs.reads.push_back("");
        rs.reads.push_back("ACGTNAC");
        for (int i = 0; i < 3000; ++i) rs.reads.push_back("");
        rs.reads.push_back(random_read(33, dna, 4));
        rs.reads.push_back("");
        rs.finish();
        run_both(rs, "empty runs");
    }
    {  // a tile with more short reads than the slice holds: the fall-back search over real reads
        ReadSet rs;
        for (int i = 0; i < 5000; ++i) rs.reads.push_back(random_read(rnd() % 4, mixed, sizeof(mixed) - 1));
        rs.finish();
        run_both(rs, "many short reads");
    }
    {  // reads across tile borders: the two strands of a read start in different tiles
        for (int d = -1; d <= 1; ++d) {
            ReadSet rs;
            rs.reads.push_back(random_read(RC_TILE_BYTES + d, dna, 4));
            rs.reads.push_back(random_read(RC_TILE_BYTES / 2 + d, mixed, sizeof(mixed) - 1));
            rs.finish();
            run_both(rs, "tile borders");
        }
    }
    for (int round = 0; round < 4; ++round) {  // random sets: lengths 0..40, every alphabet
        ReadSet rs;
        for (int i = 0; i < 3000; ++i)
            rs.reads.push_back(round == 3 ? random_read(rnd() % 41, pep, sizeof(pep) - 1)
                                          : random_read(rnd() % 41, round ? mixed : dna, round ? sizeof(mixed) - 1 : 4));
        rs.finish();
        run_both(rs, "random");
    }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
