// Host check of the plain-C++ part of py-debruijn_amd/csrc/dbg_ctgout.h: record lengths and digit counts, the map from a
// byte of a record to its field, the window planner and the run emitter, against records built with snprintf.  Built and
// run once by tests/test_ctgout_host.py; includes only that header (no HIP).
#include "dbg_ctgout.h"

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

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::string record(uint64_t number, unsigned k, const std::string &contig) {
    char head[96];
    std::snprintf(head, sizeof head, ">SEQUENCE_%" PRIu64 "_%umer\n", number, k);
    return std::string(head) + contig + "\n";
}

// contigs as strings: what CoCharsSrc / CoLiftSrc are on the device, with a check that the cursor only ever steps by one
struct StringSrc {
    const std::vector<std::string> *texts;
    const std::string *cur = nullptr;
    uint64_t last = 0;
    char first(uint32_t c, uint64_t j) { cur = &(*texts)[c]; last = j; return (*cur)[j]; }
    char next(uint64_t j) {
        EXPECT(j == last + 1, "cursor jumped from %" PRIu64 " to %" PRIu64, last, j);
        last = j;
        return (*cur)[j];
    }
};

static void check_numbers() {
    std::vector<uint64_t> numbers = {0, 1, 9};
    uint64_t p = 10;
    for (int e = 1; e <= 10; ++e, p *= 10)
        for (int64_t d = -2; d <= 2; ++d) numbers.push_back(p + (uint64_t)d);
    numbers.push_back(UINT64_MAX);
    const std::string contig = "ACGTTGCA";
    for (uint64_t number : numbers)
        for (unsigned k : {1u, 9u, 10u, 12u, 63u, 99u, 100u}) {
            const std::string want = record(number, k, contig);
            char digits[32];
            const uint32_t nd = (uint32_t)std::snprintf(digits, sizeof digits, "%" PRIu64, number), kd = co_digits(k);
            EXPECT(co_digits(number) == nd, "digits of %" PRIu64 ": %u", number, co_digits(number));
            EXPECT(kd == (k < 10 ? 1u : k < 100 ? 2u : 3u), "digits of k = %u", k);
            EXPECT(co_header_len(nd, kd) + contig.size() + 1 == want.size(), "header length of %" PRIu64, number);
            EXPECT(co_record_len(true, number, kd, contig.size()) == want.size(), "record length of %" PRIu64, number);
            EXPECT(co_record_len(false, number, kd, contig.size()) == contig.size(), "bare record length");
            int prev_field = -1;
            uint64_t prev_at = 0;
            for (uint64_t rel = 0; rel < want.size(); ++rel) {  // every offset of the record
                const CoWhere w = co_field_at(rel, nd, kd, contig.size());
                const char got = w.field == CO_TEXT ? contig[w.at] : co_fixed_char(w, number, nd, k, kd);
                EXPECT(got == want[rel], "number %" PRIu64 " k %u byte %" PRIu64 ": '%c', expected '%c'", number, k, rel, got, want[rel]);
                EXPECT(w.field >= prev_field && (w.field != prev_field ? w.at == 0 : w.at == prev_at + 1),
                       "fields out of order at byte %" PRIu64, rel);
                prev_field = w.field;
                prev_at = w.at;
            }
            EXPECT(prev_field == CO_NEWLINE, "a record ends in its newline");
        }
}

static void check_windows() {
    for (uint64_t chunk : {(uint64_t)CO_TILE, (uint64_t)2 * CO_TILE, (uint64_t)16 * CO_TILE})
        for (uint64_t total : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)16, (uint64_t)CO_TILE - 1, (uint64_t)CO_TILE, (uint64_t)CO_TILE + 1,
                               chunk - 1, chunk, chunk + 1, 3 * chunk, 3 * chunk + 17, 5 * chunk - 1}) {
            const uint64_t nw = co_n_windows(total, chunk), stage = co_stage_bytes(total, chunk);
            EXPECT(nw == (total + chunk - 1) / chunk, "windows of %" PRIu64, total);
            EXPECT(stage <= chunk && stage % CO_TILE == 0, "staging of %" PRIu64, total);
            uint64_t at = 0;
            for (uint64_t c = 0; c < nw; ++c) {
                const CoWindow w = co_window(total, chunk, c);
                EXPECT(w.b0 == at && w.b1 > w.b0 && w.b1 <= total && w.b0 % CO_TILE == 0, "window %" PRIu64 " of %" PRIu64, c, total);
                EXPECT(w.b1 - w.b0 <= chunk && (c + 1 == nw || w.b1 - w.b0 == chunk), "size of window %" PRIu64, c);
                EXPECT(w.tiles * CO_TILE >= w.b1 - w.b0 && (w.tiles - 1) * CO_TILE < w.b1 - w.b0, "tiles of window %" PRIu64, c);
                EXPECT(w.tiles * CO_TILE <= stage, "window %" PRIu64 " of %" PRIu64 " overruns its staging buffer", c, total);
                at = w.b1;
            }
            EXPECT(at == total, "windows cover %" PRIu64 " of %" PRIu64, at, total);
        }
    EXPECT(co_chunk_ok(0) && co_chunk_ok(4096) && co_chunk_ok(16u << 20) && !co_chunk_ok(1000) && !co_chunk_ok(4097), "chunk sizes");
}

// The kernel's work on the host: every window, every tile, every thread's run, compared with the text built record by record.
// identity: the list goes to the emitter as a null pointer ("record i is contig i"; `list` must then say the same).
// -> the text as the emitter spelled it
static std::string check_fill(const std::vector<std::string> &texts, const std::vector<uint32_t> &list, bool fasta, uint64_t first_number,
                              unsigned k, uint64_t chunk, const char *what, bool identity = false) {
    std::string want;
    std::vector<uint64_t> pos, off(1, 0);
    for (const std::string &t : texts) off.push_back(off.back() + t.size());
    for (size_t i = 0; i < list.size(); ++i) {
        pos.push_back(want.size());
        want += fasta ? record(first_number + i, k, texts[list[i]]) : texts[list[i]];
    }
    CoText t;
    t.pos = pos.data(); t.list = identity ? nullptr : list.data(); t.off = off.data();
    t.n = list.size(); t.total = want.size(); t.first_number = first_number;
    t.k_label = k; t.k_digits = co_digits(k); t.fasta = fasta ? 1 : 0;
    for (size_t i = 0; i < list.size(); ++i)
        EXPECT(co_record_len(fasta, first_number + i, t.k_digits, texts[list[i]].size()) ==
               (i + 1 < list.size() ? pos[i + 1] : want.size()) - pos[i], "%s: length of record %zu", what, i);
    std::string got(want.size(), '?');
    const uint64_t stage = co_stage_bytes(t.total, chunk);
    std::vector<char> staging(stage);
    for (uint64_t c = 0; c < co_n_windows(t.total, chunk); ++c) {
        const CoWindow w = co_window(t.total, chunk, c);
        std::fill(staging.begin(), staging.end(), '#');
        for (uint64_t tile = 0; tile < w.tiles; ++tile) {
            const uint64_t tile0 = w.b0 + tile * CO_TILE;
            uint64_t last = tile0 + CO_TILE - 1;
            if (last >= w.b1) last = w.b1 - 1;
            const uint64_t r0 = co_find_record(t.pos, 0, t.n, tile0), r1 = co_find_record(t.pos, 0, t.n, last);
            for (int th = 0; th < CO_NT; ++th) {
                const uint64_t b = tile0 + (uint64_t)th * CO_RUN;
                if (b >= w.b1) break;
                const uint64_t rec = co_find_record(t.pos, r0, r1 + 1, b);
                EXPECT(pos[rec] <= b && (rec + 1 == t.n || pos[rec + 1] > b), "%s: record of byte %" PRIu64, what, b);
                StringSrc src{&texts};
                uint32_t words[4];
                co_fill_run(t, rec, b, src, words);
                EXPECT(b - w.b0 + CO_RUN <= stage, "%s: store past the staging buffer at byte %" PRIu64, what, b);
                std::memcpy(staging.data() + (b - w.b0), words, CO_RUN);  // little-endian words: byte q of the run at q
                for (int q = 0; q < CO_RUN; ++q)
                    if (b + q >= t.total) EXPECT(staging[b - w.b0 + q] == 0, "%s: bytes behind the text stay zero", what);
            }
        }
        got.replace(w.b0, w.b1 - w.b0, staging.data(), w.b1 - w.b0);
    }
    EXPECT(got == want, "%s: text differs (%zu bytes)", what, want.size());
    return got;
}

// every contig once, in order: the null list spells what the explicit list 0, 1, 2, ... does, bare and as FASTA
static void check_identity(const std::vector<std::string> &texts, uint64_t first_number, unsigned k, uint64_t chunk, const char *what) {
    std::vector<uint32_t> iota;
    for (uint32_t i = 0; i < texts.size(); ++i) iota.push_back(i);
    for (bool fasta : {false, true}) {
        const std::string listed = check_fill(texts, iota, fasta, first_number, k, chunk, what);
        const std::string bare = check_fill(texts, iota, fasta, first_number, k, chunk, what, true);
        EXPECT(listed == bare && listed.size() > 0, "%s (%s): the null list differs from the list 0, 1, 2, ...", what, fasta ? "fasta" : "bare");
    }
}

static std::string random_text(uint64_t len) {
    std::string s(len, 'A');
    for (auto &ch : s) ch = "ACGT"[rnd() & 3];
    return s;
}

static void check_fills() {
    std::vector<std::string> texts;
    for (uint64_t len : {1, 2, 3, 5, 11, 11, 12, 15, 16, 17, 31, 100, 2047, 2048, 4095, 4096, 4097, 9001, 11, 11, 11, 40})
        texts.push_back(random_text(len));
    std::vector<uint32_t> all, mixed;
    for (uint32_t i = 0; i < texts.size(); ++i) all.push_back(i);
    for (int i = 0; i < 300; ++i) mixed.push_back((uint32_t)(rnd() % texts.size()));  // repeats, any order
    for (uint64_t chunk : {(uint64_t)CO_TILE, (uint64_t)2 * CO_TILE, (uint64_t)64 * CO_TILE}) {
        check_fill(texts, all, true, 0, 11, chunk, "fasta, ascending");
        check_fill(texts, all, false, 0, 11, chunk, "bare, ascending");
        check_fill(texts, mixed, true, 0, 9, chunk, "fasta, mixed");
        check_fill(texts, mixed, true, 995, 12, chunk, "fasta from 995");        // 999 -> 1000 inside
        check_fill(texts, mixed, true, 9999999990ull, 100, chunk, "fasta from 10^10 - 10");
        check_fill(texts, mixed, false, 0, 11, chunk, "bare, mixed");
        check_fill(texts, {0}, false, 0, 11, chunk, "one character");
        check_fill(texts, {0}, true, 7, 11, chunk, "one short record");
        check_fill(texts, {17, 17}, true, 0, 63, chunk, "two long records");
        check_identity(texts, 0, 11, chunk, "identity list");
        check_identity(texts, 995, 12, chunk, "identity list from 995");
    }
    // every alignment of a border inside a record: a growing pad contig in front moves the records over the tile border
    for (uint64_t pad = 4000; pad < 4000 + 140; ++pad) {
        std::vector<std::string> tx = {random_text(pad), random_text(13), random_text(11)};
        check_fill(tx, {0, 1, 2, 1}, true, 8, 11, CO_TILE, "border sweep");
        check_identity(tx, 8, 11, CO_TILE, "border sweep, identity list");
    }
    // many one-character contigs: hundreds of records inside one tile (bare) and tens (fasta)
    std::vector<std::string> tiny;
    for (int i = 0; i < 64; ++i) tiny.push_back(random_text(1));
    std::vector<uint32_t> many;
    for (int i = 0; i < 10000; ++i) many.push_back((uint32_t)(rnd() % tiny.size()));
    check_fill(tiny, many, false, 0, 1, CO_TILE, "bare, one character each");
    check_fill(tiny, many, true, 0, 1, CO_TILE, "fasta, one character each");
    for (int i = 0; i < 10000; ++i) tiny.push_back(random_text(1));  // more records than a tile has bytes
    check_identity(tiny, 0, 1, CO_TILE, "one character each, identity list");
}

int main() {
    check_numbers();
    check_windows();
    check_fills();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
