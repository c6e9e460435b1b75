// The plain-C++ part of csrc/dbg_fastq.h on the CPU, against byte-by-byte statements of the rules:
//   line start  p == 0 (after the byte handed in as "before"), t[p-1] == '\n', or t[p-1] == '\r' and t[p] != '\n'
//   kind        byte p lies in line (lines in front of the buffer + line starts at or before p) - 1; kind = that mod 4
//   mask        base j becomes 'N' where qual[j] - 33 < q; a quality byte outside 33..126 is bad
//   start       the record start at or after pos: the first line start p >= pos with t[p] == '@' whose second-next line
//               begins with '+'
//   trim        the bytes in front of the trailing white space
// over words with line starts at bit 0 and bit 31 and tails of 1 to 31 bytes, and at every position of files whose quality
// lines, headers and separators are full of '@' and '+'.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dbg_fastq.h"

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

static bool ref_space(unsigned c) { return c == 32 || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

static std::vector<size_t> ref_line_starts(const std::string &t, unsigned before) {
    std::vector<size_t> out;
    for (size_t p = 0; p < t.size(); ++p) {
        const unsigned pv = p ? (unsigned char)t[p - 1] : before, c = (unsigned char)t[p];
        if (pv == '\n' || (pv == '\r' && c != '\n')) out.push_back(p);
    }
    return out;
}

// every word of every prefix of `t` (so every tail length occurs), with `lines0` lines in front of the buffer
static void check_words(const std::string &t, uint64_t lines0, const char *what) {
    for (size_t n = 1; n <= t.size(); ++n) {
        if (n > 70 && n + 40 < t.size() && n % 13) continue;  // all short prefixes, a sample of the long ones, all tails
        uint64_t lines = lines0;
        for (size_t p0 = 0; p0 < n; p0 += 32) {
            const int nb = n - p0 >= 32 ? 32 : (int)(n - p0);
            uint32_t v[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            for (int i = 0; i < 32; ++i) {  // beyond the tail: the next bytes of the buffer, or 0x0A -- the helpers must not look
                const unsigned c = p0 + i < t.size() ? (unsigned char)t[p0 + i] : '\n';
                v[i >> 2] = (v[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | (c << (8 * (i & 3)));
            }
            uint32_t want_ls = 0, want_ns = 0, want_s = 0, want_q = 0;
            uint64_t l = lines;
            for (int i = 0; i < nb; ++i) {
                const size_t p = p0 + i;
                const unsigned pv = p ? (unsigned char)t[p - 1] : '\n', c = (unsigned char)t[p];
                const bool st = pv == '\n' || (pv == '\r' && c != '\n');
                l += st;
                if (st) want_ls |= 1u << i;
                if (!ref_space(c)) want_ns |= 1u << i;
                if (((l - 1) & 3) == 1) want_s |= 1u << i;
                if (((l - 1) & 3) == 3) want_q |= 1u << i;
            }
            uint32_t ls = ~0u, ns = ~0u, s = ~0u, q = ~0u;
            fq_masks(v, nb, p0 ? (unsigned char)t[p0 - 1] : '\n', ls, ns);
            fq_kind_masks(ls, nb, lines, &s, &q);
            EXPECT(ls == want_ls && ns == want_ns, "%s n %zu word %zu: ls %08x want %08x, ns %08x want %08x", what, n, p0 / 32, ls,
                   want_ls, ns, want_ns);
            EXPECT(s == want_s && q == want_q, "%s n %zu word %zu lines %llu: seq %08x want %08x, qual %08x want %08x", what, n,
                   p0 / 32, (unsigned long long)lines, s, want_s, q, want_q);
            lines = l;
        }
    }
}

static void check_mask() {
    for (uint32_t q : {0u, 1u, 2u, 20u, 41u, 93u})
        for (int nb = 0; nb <= 4; ++nb)
            for (unsigned c = 0; c < 256; ++c) {
                // the byte under test at every place of the dword, the others fixed at Phred 20 ('5')
                for (int at = 0; at < 4; ++at) {
                    const unsigned char qs[4] = {(unsigned char)(at == 0 ? c : '5'), (unsigned char)(at == 1 ? c : '5'),
                                                 (unsigned char)(at == 2 ? c : '5'), (unsigned char)(at == 3 ? c : '5')};
                    const unsigned char bs[4] = {'A', 'c', 'N', 'T'};
                    uint32_t qual = 0, bases = 0, want = 0, want_masked = 0, want_bad = 0;
                    for (int i = 0; i < 4; ++i) {
                        qual |= (uint32_t)qs[i] << (8 * i);
                        bases |= (uint32_t)bs[i] << (8 * i);
                        unsigned char o = bs[i];
                        if (i < nb) {
                            if ((int)qs[i] - 33 < (int)q) { o = 'N'; ++want_masked; }
                            if (qs[i] < 33 || qs[i] > 126) want_bad = 1;
                        }
                        want |= (uint32_t)o << (8 * i);
                    }
                    uint32_t masked = 0, bad = 0;
                    const uint32_t got = fq_mask_dword(bases, qual, nb, q, &masked, &bad);
                    EXPECT(got == want && masked == want_masked && bad == want_bad,
                           "mask q %u nb %d byte %u at %d: %08x want %08x, masked %u want %u, bad %u want %u", q, nb, c, at, got, want,
                           masked, want_masked, bad, want_bad);
                }
            }
}

static uint64_t ref_record_start(const std::string &t, size_t pos) {
    const std::vector<size_t> ls = ref_line_starts(t, '\n');
    for (size_t i = 0; i + 2 < ls.size(); ++i)
        if (ls[i] >= pos && t[ls[i]] == '@' && t[ls[i + 2]] == '+') return ls[i];
    return ~0ull;
}

// the scan from every position, fed in windows of several sizes
static void check_starts(const std::string &t, const char *what) {
    for (size_t pos = 1; pos <= t.size(); ++pos) {
        const uint64_t want = ref_record_start(t, pos);
        for (size_t win : {(size_t)1, (size_t)3, (size_t)32, (size_t)1 << 16}) {
            FqStartScan scan((unsigned char)t[pos - 1]);
            bool found = false;
            for (size_t p = pos; p < t.size() && !found; p += win)
                found = scan.feed((const uint8_t *)t.data() + p, std::min(win, t.size() - p), p);
            EXPECT(scan.found == want && found == (want != ~0ull), "%s pos %zu window %zu: start %llu want %llu", what, pos, win,
                   (unsigned long long)scan.found, (unsigned long long)want);
        }
    }
}

static void check_trim() {
    const char *cases[] = {"", " ", "\n\r\t \x1c\x1f", "A", "A ", "A\n\n", " A", "@a\n\n+\n\n \t", "\x20\x7f\n", "a\x1b\n", "a\x20\x08"};
    for (const char *c : cases) {
        const std::string s(c);
        size_t want = s.size();
        while (want && ref_space((unsigned char)s[want - 1])) --want;
        EXPECT(fq_trim((const uint8_t *)s.data(), s.size()) == want, "trim of %zu bytes: want %zu", s.size(), want);
    }
    for (unsigned c = 0; c < 256; ++c) EXPECT(fq_space(c) == ref_space(c), "space %u", c);
}

int main() {
    std::vector<std::string> files = {
        "@r0\nACGTACGTTG\n+\nIIIIIIIIII\n@r1\nTTGACCA\n+\nIIIIIII\n",
        "@r0\r\nACGT\r\n+\r\n@III\r\n@r1\r\nTTGA\r\n+\r\n+@+@\r\n@r2\r\nAC\r\n+\r\n@+\r\n",
        "@r0 @x +y\rACGT\r+\r@+@+\r@+\rTT\r+r +\r+@\r@@\rG\r+\r+",
        "@a\nAC\n+\n@I\n@b\n\n+\n\n@c\nGT\n+\n@@\n@d\n\n+",
        "@a\n\n+\n\n@b\n\n+\n\n@c\n\n+\n\n",
        "\n\n\n\r\r\r\n\n@\n\n+\n\n",
    };
    // line starts at bit 0 and at bit 31 of a word: a 31-byte sequence line after a 32-byte header line, and so on
    files.push_back("@" + std::string(30, 'h') + "\n" + std::string(30, 'A') + "\n" + "+\n" + std::string(30, '@') + "\n@" +
                    std::string(29, 'h') + "\r\n" + std::string(31, 'C') + "\n+" + std::string(30, '+') + "\n" + std::string(31, '+') + "\n");
    // a long record, so that words lie wholly inside one line
    files.push_back("@long\n" + std::string(200, 'G') + "  \t\n+long\n" + std::string(200, '@') + "   \n@s\nA\n+\n+\n");
    for (size_t i = 0; i < files.size(); ++i) {
        const std::string name = "file " + std::to_string(i);
        for (uint64_t lines0 : {0ull, 1ull, 2ull, 3ull, 4ull, (1ull << 40) + 2}) check_words(files[i], lines0, name.c_str());
        check_starts(files[i], name.c_str());
    }
    check_mask();
    check_trim();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
