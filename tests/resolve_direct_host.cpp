// Host check of dir_decide (py-debruijn_amd/csrc/dbg_dir.h), built and run once by tests/test_resolve_direct.py.
// Includes only that header.  Tables are filled by linear probing as the count kernels fill theirs (no deletions), the
// directory is derived from the finished table the way the kernels derive it (per 64-slot block: occupancy mask, id of the
// block's first node, nodes in slot order), and for every key "decided" must imply the true node.
#include "dbg_dir.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using dbgk::SkDirEnt;
using dbgk::dir_decide;

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

struct Table {
    int cap;
    std::vector<int> owner;  // slot -> key index, -1 = empty
    std::vector<int> home;   // key index -> home slot
    explicit Table(int c) : cap(c), owner(c, -1) {}
    void insert(int h) {
        int s = h;
        while (owner[s] >= 0) s = (s + 1) & (cap - 1);
        owner[s] = (int)home.size();
        home.push_back(h);
    }
};

// checks every key of the table; returns the number of decided keys
static long check_table(const Table &t, uint32_t first_node, const char *what) {
    const int nblk = t.cap / 64;
    std::vector<SkDirEnt> dir(nblk);
    std::vector<uint64_t> node_of_key(t.home.size());
    uint32_t next = first_node;
    for (int b = 0; b < nblk; ++b) {
        dir[b].mask = 0;
        dir[b].base = next;
        dir[b].pad = dbgk::DIR_WHOLE_BUCKET;
        for (int i = 0; i < 64; ++i) {
            const int o = t.owner[b * 64 + i];
            if (o >= 0) { dir[b].mask |= 1ull << i; node_of_key[o] = next++; }
        }
    }
    long decided = 0;
    for (size_t key = 0; key < t.home.size(); ++key) {
        const int h = t.home[key], bit = h & 63;
        const SkDirEnt &de = dir[h >> 6];
        uint64_t node = ~0ull;
        const bool d = dir_decide(de, bit, &node);
        // what "decided" means, restated from the table itself: the run of occupied slots from the home slot is one slot
        // long and ends inside the block
        const bool want = bit < 63 && t.owner[h] >= 0 && t.owner[h + 1] < 0;
        EXPECT(d == want, "%s: key %zu home %d decided %d, expected %d", what, key, h, (int)d, (int)want);
        if (d) {
            ++decided;
            EXPECT(node == node_of_key[key], "%s: key %zu home %d decided node %llu, true node %llu", what, key, h,
                   (unsigned long long)node, (unsigned long long)node_of_key[key]);
        }
    }
    return decided;
}

int main() {
    // ---- random linear-probing tables at loads 0.2 .. 0.8, both table sizes of the engines
    for (int cap : {2048, 4096}) {
        for (int load10 = 2; load10 <= 8; ++load10) {
            long keys = 0, decided = 0;
            for (int rep = 0; rep < 50; ++rep) {
                Table t(cap);
                const int n = cap * load10 / 10;
                for (int i = 0; i < n; ++i) t.insert((int)(rnd() & (uint64_t)(cap - 1)));
                decided += check_table(t, (uint32_t)(rnd() & 0xFFFFFFu), "random");
                keys += n;
            }
            std::printf("cap %d load 0.%d: decided share %.3f\n", cap, load10, (double)decided / (double)keys);
        }
    }
    // ---- dense blocks: a block that is full is never decided; a full block next to an empty one neither
    {
        Table t(4096);
        for (int i = 0; i < 64; ++i) t.insert(128 + i);        // block 2 full, every key at home
        for (int i = 0; i < 64; ++i) t.insert(320);            // 64 keys of one home: block 5 full from its first slot
        for (int i = 0; i < 32; ++i) t.insert(64 * 9 + 2 * i); // more than 31 nodes in a block, every one a run of length 1
        t.insert(64 * 12 + 63);                                 // alone, but at bit 63
        EXPECT(check_table(t, 7, "dense") == 32, "dense: exactly the 32 isolated keys below bit 63 are decided");
    }
    // ---- runs over a block's end and around the table's end
    {
        Table t(4096);
        for (int i = 0; i < 8; ++i) t.insert(60);       // slots 60 .. 67
        for (int i = 0; i < 5; ++i) t.insert(4094);     // slots 4094, 4095, 0, 1, 2
        t.insert(4095);                                 // lands in slot 3: its home block is the last, its node in the first
        t.insert(127);                                  // alone at bit 63: the run reaches the block's end
        t.insert(200);                                  // alone in the middle of a block: decided
        EXPECT(check_table(t, 0, "ends") == 1, "ends: only the isolated key is decided");
    }
    // ---- every home bit against random masks: a run of two or more slots holds two candidates and is never decided; a
    //      run that reaches bit 63 is never decided; an empty home slot is never decided
    for (int rep = 0; rep < 200000; ++rep) {
        SkDirEnt de;
        de.mask = rnd() & rnd() & ((rep & 1) ? ~0ull : rnd());
        if (rep % 7 == 0) de.mask |= ~0ull << (int)(rnd() % 64);  // ones up to bit 63
        de.base = (uint32_t)rnd();
        de.pad = dbgk::DIR_WHOLE_BUCKET;
        for (int bit = 0; bit < 64; ++bit) {
            uint64_t node = 0;
            const bool d = dir_decide(de, bit, &node);
            int run = 0;
            while (bit + run < 64 && ((de.mask >> (bit + run)) & 1ull)) ++run;
            if (run >= 2) EXPECT(!d, "two candidates decided: mask %016llx bit %d", (unsigned long long)de.mask, bit);
            if (bit + run == 64) EXPECT(!d, "run to the block's end decided: mask %016llx bit %d", (unsigned long long)de.mask, bit);
            if (run == 0) EXPECT(!d, "empty home slot decided: mask %016llx bit %d", (unsigned long long)de.mask, bit);
            if (run == 1 && bit + run < 64) {
                int below = 0;
                for (int i = 0; i < bit; ++i) below += (int)((de.mask >> i) & 1ull);
                EXPECT(d && node == (uint64_t)de.base + (uint64_t)below, "single-slot run: mask %016llx bit %d", (unsigned long long)de.mask, bit);
            }
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
