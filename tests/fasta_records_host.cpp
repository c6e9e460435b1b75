// Host check of the plain-C++ parts behind record-mode FASTA and wrapped contig output: the header search of
// py-debruijn_amd/csrc/dbg_fasta.h (FaHeaderScan) at every position of hand-written files and across window borders, and
// the wrapped record geometry of py-debruijn_amd/csrc/dbg_ctgout.h (body length, byte-to-field map, the run emitter with a
// host text source) against records built character by character.  Built and run once by tests/test_fasta_records_host.py;
// includes only those two headers (no HIP).
#include "dbg_ctgout.h"
#include "dbg_fasta.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace dbgk;

static int failures = 0;
#define EXPECT(cond, ...)                                                      \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                      \
    } while (0)

// ---- the header search -----------------------------------------------------------------------------------------------------
static bool is_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

// the rule, byte by byte: p starts a line iff p == 0, t[p-1] == '\n', or t[p-1] == '\r' and t[p] != '\n'
static bool line_start(const std::string &t, uint64_t p) {
    return p == 0 || t[p - 1] == '\n' || (t[p - 1] == '\r' && t[p] != '\n');
}

static void check_scan(const std::string &t, const char *what) {
    const uint64_t n = t.size();
    for (uint64_t from = 0; from <= n; ++from) {
        uint64_t want = n, want_seq = ~0ull;
        for (uint64_t p = from; p < n; ++p) {
            if (t[p] == '>' && line_start(t, p)) { want = p; break; }
            if (want_seq == ~0ull && !is_space((unsigned char)t[p])) want_seq = p;
        }
        for (uint64_t win : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)7, (uint64_t)64, n + 1}) {
            FaHeaderScan scan(from ? (unsigned char)t[from - 1] : '\n');
            uint64_t got = n;
            for (uint64_t pos = from; pos < n; pos += win) {
                const uint64_t len = n - pos < win ? n - pos : win;
                std::vector<uint8_t> buf(t.begin() + pos, t.begin() + pos + len);  // a window of its own: no byte past it
                if (scan.feed(buf.data(), len, pos)) { got = scan.found; break; }
            }
            EXPECT(got == want, "%s: header at or after %" PRIu64 " (windows of %" PRIu64 "): %" PRIu64 ", expected %" PRIu64, what,
                   from, win, got, want);
            EXPECT(scan.first_seq == want_seq, "%s: first sequence byte from %" PRIu64 " (windows of %" PRIu64 "): %" PRIu64
                   ", expected %" PRIu64, what, from, win, scan.first_seq, want_seq);
        }
    }
}

static void check_scans() {
    const char *files[] = {
        "",
        ">a\nACGT\nAC\n>b\nGG\n",
        ">a\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
        ">a\rACGT\rAC\r>b\rGG\r",
        ">a\nACGT\nAC\n>b\nGG",
        ">a\n\nAC \t\n\n\nGT\n\n>b\n\n",
        ">a\n>b\n>c\nAC\n>d",
        ">a\n>b\r>c\r\n>d",
        "\n \n\t\n>a\nAC\n",
        ">a\nAC>GT\n >b\nA\x0c" "C\n>c\n",
        "\n  AC\n>a\nGT\n",
        "ACGT\nAC\n",
        ">",
        "\r>\n\r\n>\r\r>",
        "A\n>\r\n>b\n\rG>\n>",
    };
    for (const char *f : files) check_scan(f, f);
    std::string big;  // headers on both sides of a 64-byte window border
    for (int i = 0; i < 40; ++i) big += ">r" + std::to_string(i) + "\n" + std::string(7 + i % 5, "ACGT"[i & 3]) + (i % 3 ? "\n" : "\r\n");
    check_scan(big, "forty records");
}

// ---- wrapped records -------------------------------------------------------------------------------------------------------
static std::string wrapped_body(const std::string &contig, uint32_t w) {
    if (!w || contig.empty()) return contig + "\n";
    std::string out;
    for (size_t i = 0; i < contig.size(); i += w) out += contig.substr(i, w) + "\n";
    return out;
}

static std::string record(uint64_t number, unsigned k, const std::string &contig, uint32_t w) {
    char head[96];
    std::snprintf(head, sizeof head, ">SEQUENCE_%" PRIu64 "_%umer\n", number, k);
    return std::string(head) + wrapped_body(contig, w);
}

static std::string text_of(uint64_t len, uint64_t salt) {
    std::string s(len, 'A');
    for (uint64_t i = 0; i < len; ++i) s[i] = "ACGT"[((i + salt) * 2654435761u >> 7) & 3];
    return s;
}

static void check_geometry() {
    for (uint32_t w : {0u, 1u, 2u, 60u}) {
        const uint64_t ww = w ? w : 60;
        for (uint64_t len : {(uint64_t)0, (uint64_t)1, ww - 1, ww, ww + 1, 2 * ww, 2 * ww + 1})
            for (uint64_t number : {(uint64_t)7, (uint64_t)42})  // one and two header digits
                for (unsigned k : {9u, 31u}) {
                    const std::string contig = text_of(len, number), want = record(number, k, contig, w);
                    const uint32_t nd = co_digits(number), kd = co_digits(k);
                    const uint64_t hdr = co_header_len(nd, kd);
                    EXPECT(co_body_len(len, w) == want.size() - hdr, "body of %" PRIu64 " at width %u: %" PRIu64, len, w, co_body_len(len, w));
                    EXPECT(co_body_len(len, w) == len + (w && len ? (len + w - 1) / w : 1), "the issue's formula, %" PRIu64 " at %u", len, w);
                    EXPECT(co_record_len_wrapped(number, kd, len, w) == want.size(), "record of %" PRIu64 " at width %u", len, w);
                    if (!w) EXPECT(co_record_len_wrapped(number, kd, len, 0) == co_record_len(true, number, kd, len), "width 0 is the unwrapped record");
                    uint64_t next_char = 0;
                    for (uint64_t rel = 0; rel < want.size(); ++rel) {
                        const CoWhere f = co_field_at_wrapped(rel, nd, kd, len, w);
                        if (f.field == CO_TEXT) {
                            EXPECT(f.at == next_char, "characters come in order: %" PRIu64 " after %" PRIu64, f.at, next_char);
                            ++next_char;
                        }
                        const char got = f.field == CO_TEXT ? contig[f.at] : co_fixed_char(f, number, nd, k, kd);
                        EXPECT(got == want[rel], "len %" PRIu64 " width %u number %" PRIu64 " byte %" PRIu64 ": '%c', expected '%c'", len, w,
                               number, rel, got, want[rel]);
                        if (!w) {
                            const CoWhere g = co_field_at(rel, nd, kd, len);
                            EXPECT(g.field == f.field && (f.field == CO_NEWLINE || g.at == f.at), "width 0 maps as co_field_at does, byte %" PRIu64, rel);
                        }
                    }
                    EXPECT(next_char == len, "every character once: %" PRIu64 " of %" PRIu64, next_char, len);
                }
    }
}

// contigs as strings, with a check that the cursor only ever steps by one
struct StringSrc {
    const std::vector<std::string> *texts;
    const std::string *cur = nullptr;
    uint64_t last = 0;
    char first(uint32_t c, uint64_t j) {
        cur = &(*texts)[c];
        EXPECT(j < cur->size(), "first(%u, %" PRIu64 ") past the contig", c, j);
        last = j;
        return (*cur)[j];
    }
    char next(uint64_t j) {
        EXPECT(j == last + 1 && j < cur->size(), "cursor jumped from %" PRIu64 " to %" PRIu64, last, j);
        last = j;
        return (*cur)[j];
    }
};

// runs that begin at EVERY byte of the text (the kernel starts them at multiples of CO_RUN; the emitter does not care)
static void check_runs(const std::vector<std::string> &texts, const std::vector<uint32_t> &list, uint64_t first_number, unsigned k,
                       uint32_t w, const char *what) {
    std::string want;
    std::vector<uint64_t> pos, off(1, 0);
    for (const std::string &t : texts) off.push_back(off.back() + t.size());
    for (size_t i = 0; i < list.size(); ++i) {
        pos.push_back(want.size());
        want += record(first_number + i, k, texts[list[i]], w);
    }
    CoText t;
    t.pos = pos.data(); t.list = list.data(); t.off = off.data();
    t.n = list.size(); t.total = want.size(); t.first_number = first_number;
    t.k_label = k; t.k_digits = co_digits(k); t.fasta = 1;
    t.line_width = w;
    for (uint64_t b = 0; b < want.size(); ++b) {
        const uint64_t rec = co_find_record(t.pos, 0, t.n, b);
        StringSrc src{&texts};
        uint32_t words[4];
        co_fill_run(t, rec, b, src, words);
        char run[CO_RUN];
        std::memcpy(run, words, CO_RUN);
        for (int q = 0; q < CO_RUN; ++q) {
            const char expect = b + q < want.size() ? want[b + q] : 0;
            EXPECT(run[q] == expect, "%s, width %u: run at byte %" PRIu64 ", byte %d: %d, expected %d", what, w, b, q, run[q], expect);
        }
    }
}

static void check_fills() {
    for (uint32_t w : {0u, 1u, 2u, 3u, 5u, 60u, 61u}) {
        const uint64_t ww = w ? w : 60;
        const std::vector<std::string> three = {text_of(2 * ww + 1, 1), text_of(0, 2), text_of(ww, 3)};
        check_runs(three, {0, 1, 2}, 9, 31, w, "three records, 9 -> 10");
        check_runs(three, {2, 2, 1, 0, 1}, 0, 7, w, "repeats and empty contigs");
        const std::vector<std::string> more = {text_of(ww - 1, 4), text_of(1, 5), text_of(2 * ww, 6), text_of(ww + 1, 7)};
        check_runs(more, {0, 1, 2, 3}, 98, 63, w, "four records, 99 -> 100");
    }
}

int main() {
    check_scans();
    check_geometry();
    check_fills();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
