// Host check of csrc/dbg_partfinal.h (tests/test_partfinal_host.py builds and runs it): the final-mode walker over the
// contracted graph against a recursive node-by-node DFS written from debruijn.py:288-316 (branch_kmer == []), on hand-made
// and random node-level graphs cut into parts, walked with stride 1 and by three interleaved walkers at stride 3; the
// validation predicate against each kind of broken row; the step budget.
#include "dbg_partfinal.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace dbgk;

static int failures = 0;
#define EXPECT(cond, ...)                                                      \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (++failures <= 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                      \
    } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- the node-level graph after pruning and tips: kept successors in Counter.most_common order, pulled marks, parts ----------
struct Node {
    std::vector<int> succ;        // E[node], rank order
    std::vector<uint32_t> cnt;    // counts of those edges
    bool pulled = false;
    int part = 0;
};
struct Toy {
    int k = 5;
    std::vector<Node> node;
    std::vector<int> starts;      // dict order
    uint32_t count_of(int a, int b) const {
        for (size_t q = 0; q < node[a].succ.size(); ++q)
            if (node[a].succ[q] == b) return node[a].cnt[q];
        return 0;
    }
};
struct Contig {
    int start_ord;
    std::vector<int> nodes;
    uint64_t score;
    bool operator==(const Contig &o) const { return start_ord == o.start_ord && nodes == o.nodes && score == o.score; }
};

// ---- the reference: debruijn.py:288-316, line by line (E of a pulled node is never read: the pulled test comes first) ---------
static void ref_dfs(const Toy &t, int current, std::vector<int> &vec, std::vector<std::vector<int>> &output) {
    if (std::find(vec.begin(), vec.end(), current) != vec.end()) return;             // :289
    vec.push_back(current);                                                           // :291
    if (t.node[current].pulled) {                                                     // :292
        if (vec.size() == 1) { vec.pop_back(); return; }                              // :293-295
        vec.pop_back();                                                               // :296
        if (std::find(output.begin(), output.end(), vec) == output.end()) output.push_back(vec);  // :297-302
        return;
    }
    if (t.node[current].succ.empty()) {                                               // :304 (branch_kmer is empty)
        if (std::find(output.begin(), output.end(), vec) == output.end()) output.push_back(vec);
        vec.pop_back();
        return;
    }
    for (int nx : t.node[current].succ) ref_dfs(t, nx, vec, output);                   // :314-315
    vec.pop_back();
}
static std::vector<Contig> reference(const Toy &t) {
    std::vector<Contig> all;
    for (size_t i = 0; i < t.starts.size(); ++i) {
        std::vector<int> vec;
        std::vector<std::vector<int>> output;
        ref_dfs(t, t.starts[i], vec, output);
        for (const auto &path : output) {
            uint64_t score = 0;
            for (size_t q = 1; q < path.size(); ++q) score += t.count_of(path[q - 1], path[q]);
            all.push_back(Contig{(int)i, path, score});
        }
    }
    return all;
}

// ---- the contraction: the entry and segment rules of the walk in parts, restated on the host ---------------------------------
enum { K_EMIT = 0, K_PULLED = 1, K_REMOTE = 2, K_CYCLE = 3, K_NEXT_PULLED = 4 };
struct Contracted {
    std::vector<int> entry;       // node of every row, ascending
    std::vector<uint8_t> kind;
    std::vector<uint64_t> append, score;
    std::vector<uint32_t> branch, succ_row, succ_cnt, starts;
    std::vector<int> branch_node;
    FwGraph view() const {
        return FwGraph{kind.data(), append.data(), score.data(), branch.data(), succ_row.data(), succ_cnt.data(), starts.data(),
                       kind.size(), branch_node.size(), starts.size()};
    }
};
static Contracted contract(const Toy &t) {
    const int n = (int)t.node.size();
    auto chain = [&](int x) { return t.node[x].succ.size() == 1; };
    std::set<int> ent(t.starts.begin(), t.starts.end());
    for (int x = 0; x < n; ++x) {
        if (chain(x) && t.node[t.node[x].succ[0]].part != t.node[x].part) ent.insert(t.node[x].succ[0]);  // chain edges that leave a part
        if (t.node[x].succ.size() > 1)
            for (int s : t.node[x].succ) ent.insert(s);                                                  // kept successors of branch nodes
    }
    Contracted c;
    c.entry.assign(ent.begin(), ent.end());
    const size_t ne = c.entry.size();
    std::map<int, uint32_t> row_of;
    for (size_t r = 0; r < ne; ++r) row_of[c.entry[r]] = (uint32_t)r;
    // one segment per entry, inside its part (k_part_segments)
    std::vector<int> skind(ne), last(ne), next(ne, -1);
    std::vector<uint64_t> hops(ne, 0), sscore(ne, 0), exit_cnt(ne, 0);
    for (size_t r = 0; r < ne; ++r) {
        int cur = c.entry[r];
        if (t.node[cur].pulled) { skind[r] = K_PULLED; last[r] = cur; continue; }
        std::set<int> seen{cur};
        for (;;) {
            if (!chain(cur)) { skind[r] = K_EMIT; break; }
            const int nx = t.node[cur].succ[0];
            if (t.node[nx].part != t.node[cur].part) { skind[r] = K_REMOTE; next[r] = nx; exit_cnt[r] = t.node[cur].cnt[0]; break; }
            if (t.node[nx].pulled) { skind[r] = K_NEXT_PULLED; break; }
            sscore[r] += t.node[cur].cnt[0];
            ++hops[r];
            cur = nx;
            if (!seen.insert(cur).second) { skind[r] = K_CYCLE; break; }
        }
        last[r] = cur;
    }
    // ranking (rank_skeleton): follow the hand-overs; more than n_entries of them is a cycle across parts
    for (int x = 0; x < n; ++x)
        if (t.node[x].succ.size() > 1) c.branch_node.push_back(x);
    c.kind.resize(ne); c.append.assign(ne, 0); c.score.assign(ne, 0); c.branch.assign(ne, 0);
    for (size_t r = 0; r < ne; ++r) {
        size_t s = r;
        uint64_t app = 0, sc = 0;
        uint8_t kd = FW_DEAD;
        for (size_t jumps = 0; jumps <= ne; ++jumps) {
            if (skind[s] == K_PULLED) { kd = FW_PULLED; break; }   // only the entry itself: a hand-over into a pulled entry stops before it
            if (skind[s] == K_CYCLE) break;
            app += hops[s];
            sc += sscore[s];
            if (skind[s] == K_NEXT_PULLED) { kd = FW_BEFORE_PULLED; break; }
            if (skind[s] == K_EMIT) {
                const auto b = std::find(c.branch_node.begin(), c.branch_node.end(), last[s]);
                if (b == c.branch_node.end()) kd = FW_EMIT;
                else { kd = FW_BRANCH; c.branch[r] = (uint32_t)(b - c.branch_node.begin()); }
                break;
            }
            const uint32_t nr = row_of.at(next[s]);  // K_REMOTE
            if (skind[nr] == K_PULLED) { kd = FW_BEFORE_PULLED; break; }
            app += 1;
            sc += exit_cnt[s];
            s = nr;
        }
        c.kind[r] = kd;
        c.append[r] = kd == FW_DEAD || kd == FW_PULLED ? 0 : app;
        c.score[r] = kd == FW_DEAD || kd == FW_PULLED ? 0 : sc;
    }
    c.succ_row.assign(c.branch_node.size() * FW_FAN, FW_NO_ROW);
    c.succ_cnt.assign(c.branch_node.size() * FW_FAN, 0);
    for (size_t b = 0; b < c.branch_node.size(); ++b) {
        const Node &bn = t.node[c.branch_node[b]];
        for (size_t q = 0; q < bn.succ.size(); ++q) {
            c.succ_row[b * FW_FAN + q] = row_of.at(bn.succ[q]);
            c.succ_cnt[b * FW_FAN + q] = bn.cnt[q];
        }
    }
    for (int s : t.starts) c.starts.push_back(row_of.at(s));
    return c;
}

// ---- the walker under test: two passes as the library runs them, pieces expanded back to nodes ------------------------------
struct Walked {
    bool ok = true;
    std::vector<Contig> contigs;
    uint64_t n_pieces = 0, n_chars = 0, steps = 0;
};
// With stride S, S walkers share one lv / bm allocation, interleaved as k_fw_walk lays them out (level d of walker v at
// lv[d * S + v], word q at bm[q * S + v]), and start i goes to walker i % S with that walker's own budget.  Before every
// start the other walkers' levels and words are filled with a pattern; the walker must leave them as they were.
static const uint32_t PAT = 0xA5A5A5A5u;
static const FwLevel PAT_LEVEL{PAT, PAT, 0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull};
struct Shared {
    uint64_t stride;
    std::vector<FwLevel> lv;
    std::vector<uint32_t> bm;
    Shared(const FwGraph &g, uint64_t s) : stride(s), lv((g.n_branch + 1) * s), bm(((g.n_branch + 31) / 32 + 1) * s, 0) {}
    void arm(uint64_t v) {
        std::fill(lv.begin(), lv.end(), PAT_LEVEL);
        for (size_t q = 0; q < bm.size(); ++q) bm[q] = q % stride == v ? 0u : PAT;
    }
    void verify(uint64_t v, uint64_t i) const {
        for (size_t q = 0; q < lv.size(); ++q)
            if (q % stride != v)
                EXPECT(lv[q].row == PAT && lv[q].state == PAT && lv[q].nodes == PAT_LEVEL.nodes && lv[q].score == PAT_LEVEL.score,
                       "start %" PRIu64 " (walker %" PRIu64 " of %" PRIu64 ") wrote level slot %zu of a neighbour", i, v, stride, q);
        for (size_t q = 0; q < bm.size(); ++q) {
            if (q % stride == v) EXPECT(bm[q] == 0, "the bitmap is dirty after start %" PRIu64, i);
            else EXPECT(bm[q] == PAT, "start %" PRIu64 " (walker %" PRIu64 " of %" PRIu64 ") wrote bitmap word %zu of a neighbour", i, v, stride, q);
        }
    }
};
static Walked walk(const Toy &t, const Contracted &c, uint64_t budget, uint64_t stride = 1) {
    Walked w;
    const FwGraph g = c.view();
    Shared sh(g, stride);
    std::vector<FwCount> per(g.n_starts);
    FwOut none{};
    std::vector<uint64_t> steps(stride, budget);
    for (uint64_t i = 0; i < g.n_starts; ++i) {
        const uint64_t v = i % stride;
        per[i] = FwCount{0, 0, 0};
        sh.arm(v);
        if (!fw_walk_start(g, t.k, i, sh.lv.data() + v, sh.bm.data() + v, stride, 0, 0, 0, none, per[i], steps[v])) { w.ok = false; return w; }
        sh.verify(v, i);
    }
    for (uint64_t v = 0; v < stride; ++v) w.steps += budget - steps[v];
    uint64_t nc = 0, np = 0;
    std::vector<uint64_t> cb(g.n_starts), pb(g.n_starts);
    for (uint64_t i = 0; i < g.n_starts; ++i) { cb[i] = nc; pb[i] = np; nc += per[i].contigs; np += per[i].pieces; w.n_chars += per[i].chars; }
    w.n_pieces = np;
    std::vector<uint32_t> so(nc + 1, 0xDEADu), seq(nc + 1, 0xDEADu), prow(np + 1, 0xDEADu);
    std::vector<uint64_t> len(nc + 1, 0), sc(nc + 1, 0), poff(nc + 1, 0);
    FwOut o{so.data(), seq.data(), len.data(), sc.data(), poff.data(), prow.data(), nc, np};
    steps.assign(stride, budget);
    for (uint64_t i = 0; i < g.n_starts; ++i) {
        const uint64_t v = i % stride;
        FwCount again{0, 0, 0};
        sh.arm(v);
        const bool ok = fw_walk_start(g, t.k, i, sh.lv.data() + v, sh.bm.data() + v, stride, 1, cb[i], pb[i], o, again, steps[v]);
        sh.verify(v, i);
        EXPECT(ok && again.contigs == per[i].contigs && again.pieces == per[i].pieces && again.chars == per[i].chars, "pass 1 differs from pass 0 at start %" PRIu64, i);
    }
    EXPECT(so[nc] == 0xDEADu && prow[np] == 0xDEADu, "pass 1 wrote behind its arrays");
    poff[nc] = np;
    uint64_t chars = 0;
    for (uint64_t q = 0; q < nc; ++q) {
        Contig ct{(int)so[q], {}, sc[q]};
        EXPECT(q == 0 || so[q] >= so[q - 1], "contigs are not grouped by start");
        EXPECT(seq[q] == (q && so[q] == so[q - 1] ? seq[q - 1] + 1 : 0u), "seq does not count within the start");
        EXPECT(poff[q] < poff[q + 1] && poff[q + 1] <= np, "piece offsets");
        for (uint64_t p = poff[q]; p < poff[q + 1] && p < np; ++p) {
            const uint32_t r = prow[p];
            EXPECT(r < g.n_entries && (g.kind[r] == FW_EMIT || g.kind[r] == FW_BEFORE_PULLED || g.kind[r] == FW_BRANCH), "a piece is no row with text");
            if (r >= g.n_entries) break;
            int x = c.entry[r];
            ct.nodes.push_back(x);
            for (uint64_t a = 0; a < g.append[r]; ++a) { x = t.node[x].succ[0]; ct.nodes.push_back(x); }
        }
        EXPECT(len[q] == (uint64_t)t.k + ct.nodes.size() - 1, "length %" PRIu64 " of a contig of %zu nodes", len[q], ct.nodes.size());
        chars += len[q];
        w.contigs.push_back(ct);
    }
    EXPECT(chars == w.n_chars, "the counted characters are not the sum of the lengths");
    return w;
}

static std::string show(const std::vector<Contig> &v) {
    std::string s;
    for (const auto &c : v) {
        s += "[" + std::to_string(c.start_ord) + ":";
        for (int x : c.nodes) s += " " + std::to_string(x);
        s += " |" + std::to_string(c.score) + "] ";
    }
    return s;
}

static Walked check(const Toy &t, const char *what, uint64_t stride = 1) {
    const Contracted c = contract(t);
    const FwGraph g = c.view();
    const uint64_t n_check = std::max<uint64_t>(std::max<uint64_t>(g.n_entries, g.n_branch * FW_FAN), g.n_starts);
    for (uint64_t i = 0; i < n_check; ++i) EXPECT(fw_fault_at(g, i) == FW_OK, "%s: the contraction fails validation at %" PRIu64, what, i);
    const Walked w = walk(t, c, 1ull << 40, stride);
    const std::vector<Contig> ref = reference(t);
    EXPECT(w.ok && w.contigs == ref, "%s: walker %s reference %s", what, show(w.contigs).c_str(), show(ref).c_str());
    return w;
}

// edges as {from, to, count}; successors of a node rank in the order given
struct E { int a, b; uint32_t c; };
static Toy make(int n, std::vector<E> edges, std::vector<int> starts, std::vector<int> pulled, std::vector<int> parts = {}) {
    Toy t;
    t.node.resize(n);
    for (const E &e : edges) { t.node[e.a].succ.push_back(e.b); t.node[e.a].cnt.push_back(e.c); }
    for (int p : pulled) t.node[p].pulled = true;
    for (size_t i = 0; i < parts.size(); ++i) t.node[i].part = parts[i];
    t.starts = starts;
    return t;
}

static void required_cases() {
    {   // two pulled successors of one branch node: one prefix, not two
        const Toy t = make(5, {{0, 1, 3}, {1, 2, 5}, {1, 3, 4}, {1, 4, 2}}, {0}, {2, 3});
        const Walked w = check(t, "two pulled successors");
        const std::vector<Contig> want{{0, {0, 1}, 3}, {0, {0, 1, 4}, 5}};
        EXPECT(w.contigs == want, "two pulled successors: %s", show(w.contigs).c_str());
    }
    {   // a successor chain that re-enters the path in the middle of a segment: 0 -> 1 -> 2 -> 3(branch) -> {4 -> 1, 5}
        for (int cut = 0; cut < 2; ++cut) {
            const Toy t = make(6, {{0, 1, 1}, {1, 2, 2}, {2, 3, 3}, {3, 4, 9}, {3, 5, 7}, {4, 1, 1}}, {0}, {},
                               cut ? std::vector<int>{0, 0, 1, 1, 2, 0} : std::vector<int>{});
            const Walked w = check(t, "re-entering chain");
            const std::vector<Contig> want{{0, {0, 1, 2, 3, 5}, 13}};
            EXPECT(w.contigs == want, "re-entering chain: %s", show(w.contigs).c_str());
        }
    }
    {   // a start that is a branch node
        const Toy t = make(4, {{0, 1, 2}, {0, 2, 1}, {1, 3, 4}}, {0}, {});
        const Walked w = check(t, "branching start");
        const std::vector<Contig> want{{0, {0, 1, 3}, 6}, {0, {0, 2}, 1}};
        EXPECT(w.contigs == want, "branching start: %s", show(w.contigs).c_str());
    }
    {   // a start that is pulled emits nothing; the next start still does
        const Toy t = make(3, {{0, 1, 1}, {2, 1, 1}}, {0, 2}, {0});
        const Walked w = check(t, "pulled start");
        const std::vector<Contig> want{{1, {2, 1}, 1}};
        EXPECT(w.contigs == want, "pulled start: %s", show(w.contigs).c_str());
    }
    {   // a branch node all of whose successors are dead (chains that close on themselves)
        const Toy t = make(6, {{0, 1, 1}, {1, 2, 2}, {1, 4, 2}, {2, 3, 1}, {3, 2, 1}, {4, 5, 1}, {5, 4, 1}}, {0}, {}, {0, 0, 0, 1, 0, 0});
        const Walked w = check(t, "dead successors");
        EXPECT(w.contigs.empty(), "dead successors: %s", show(w.contigs).c_str());
    }
    {   // merging chains and a branch successor inside another row's segment: 0 -> 1 -> 2 -> 3 -> 4, 5(branch) -> {2, 6}, 6 -> 3
        const Toy t = make(7, {{0, 1, 1}, {1, 2, 1}, {2, 3, 1}, {3, 4, 1}, {5, 2, 3}, {5, 6, 2}, {6, 3, 1}}, {0, 5}, {}, {0, 1, 1, 0, 0, 0, 1});
        const Walked w = check(t, "merging chains");
        const std::vector<Contig> want{{0, {0, 1, 2, 3, 4}, 4}, {1, {5, 2, 3, 4}, 5}, {1, {5, 6, 3, 4}, 4}};
        EXPECT(w.contigs == want, "merging chains: %s", show(w.contigs).c_str());
    }
}

static void random_cases() {
    uint64_t with_branch = 0, with_pulled_prefix = 0, n_contigs = 0, strided_starts = 0;
    for (int round = 0; round < 4000; ++round) {
        Toy t;
        t.k = 2 + (int)(rnd() % 40);
        const int n = 1 + (int)(rnd() % 40), parts = 1 + (int)(rnd() % 4);
        t.node.resize(n);
        int branches = 0;
        std::vector<int> indeg(n, 0);
        for (int x = 0; x < n; ++x) {
            const uint64_t roll = rnd() % 100;
            int deg = roll < 12 ? 0 : roll < 80 ? 1 : 2 + (int)(rnd() % 3);
            if (deg > 1 && ++branches > 6) deg = 1;   // the enumeration is exponential in the branch nodes
            deg = std::min(deg, n);
            while ((int)t.node[x].succ.size() < deg) {
                const int y = (int)(rnd() % n);
                if (std::find(t.node[x].succ.begin(), t.node[x].succ.end(), y) != t.node[x].succ.end()) continue;
                t.node[x].succ.push_back(y);
                t.node[x].cnt.push_back(1 + (uint32_t)(rnd() % 50));
                ++indeg[y];
            }
            t.node[x].pulled = deg < 2 && rnd() % 8 == 0;   // a branch node is never pulled (debruijn.py:251)
            t.node[x].part = (int)(rnd() % parts);
        }
        for (int x = 0; x < n; ++x)
            if (indeg[x] == 0 || rnd() % 10 == 0) t.starts.push_back(x);
        const Walked w = check(t, "random");
        const Walked w3 = check(t, "random, three interleaved walkers", 3);
        EXPECT(w3.contigs == w.contigs && w3.steps == w.steps && w3.n_pieces == w.n_pieces, "stride 3 differs from stride 1");
        strided_starts += t.starts.size() > 3;
        with_branch += branches > 0;
        n_contigs += w.contigs.size();
        for (size_t q = 1; q < w.contigs.size(); ++q) {
            const auto &a = w.contigs[q - 1].nodes, &b = w.contigs[q].nodes;
            with_pulled_prefix += a.size() < b.size() && std::equal(a.begin(), a.end(), b.begin());
        }
    }
    std::printf("random: %" PRIu64 " contigs, %" PRIu64 " graphs with branch nodes, %" PRIu64 " prefixes emitted before their extensions\n",
                n_contigs, with_branch, with_pulled_prefix);
    EXPECT(with_branch > 2000 && n_contigs > 4000, "the random graphs are too tame");
    std::printf("random: %" PRIu64 " graphs with more than three starts\n", strided_starts);
    EXPECT(strided_starts > 1400, "only %" PRIu64 " graphs gave a walker of three a second start", strided_starts);
}

// The random graphs have at most 6 branch nodes: one bitmap word.  A comb of 70 branch nodes, each with a leaf and the next
// branch node as successors and one arm back to the comb's first node, puts up to 70 levels on the stack and marks bits in
// three words, by three interleaved walkers whose starts enter the comb at different depths.
static void deep_comb() {
    const int B = 70;
    std::vector<E> edges;
    for (int j = 0; j < B; ++j) {
        edges.push_back({2 * j, j + 1 < B ? 2 * j + 2 : 2 * B, 3});
        edges.push_back({2 * j, 2 * j + 1, 2});
        if (j % 7 == 3) edges.push_back({2 * j, 0, 1});
    }
    const Toy t = make(2 * B + 1, edges, {0, 20, 80, 2, 66, 130, 1}, {5, 71});
    const Walked one = check(t, "comb");
    const Walked three = check(t, "comb, three interleaved walkers", 3);
    EXPECT(three.contigs == one.contigs && three.steps == one.steps, "comb: stride 3 differs from stride 1");
    size_t longest = 0;
    for (const auto &ct : one.contigs) longest = std::max(longest, ct.nodes.size());
    EXPECT(longest == (size_t)B + 1 && contract(t).branch_node.size() == (size_t)B, "comb: the longest path has %zu nodes", longest);
}

static int faults_of(const Contracted &c) {
    const FwGraph g = c.view();
    const uint64_t n_check = std::max<uint64_t>(std::max<uint64_t>(g.n_entries, g.n_branch * FW_FAN), g.n_starts);
    int f = 0;
    for (uint64_t i = 0; i < n_check; ++i) f |= fw_fault_at(g, i);
    return f;
}

static void check_validation() {
    const Toy t = make(5, {{0, 1, 3}, {1, 2, 5}, {1, 3, 4}, {1, 4, 2}}, {0}, {2});
    const Contracted good = contract(t);
    EXPECT(faults_of(good) == FW_OK, "the sound graph");
    EXPECT(good.branch_node.size() == 1 && good.kind[0] == FW_BRANCH, "the toy's shape");
    { Contracted c = good; c.kind[1] = FW_N_KINDS; EXPECT(faults_of(c) == FW_BAD_KIND, "kind out of range"); }
    { Contracted c = good; c.kind[1] = 0xFF; EXPECT(faults_of(c) == FW_BAD_KIND, "kind 255"); }
    { Contracted c = good; c.branch[0] = 1; EXPECT(faults_of(c) == FW_BAD_BRANCH, "branch row == n_branch"); }
    { Contracted c = good; c.branch[1] = 77; EXPECT(faults_of(c) == FW_OK, "branch of a row that ends elsewhere is not read"); }
    { Contracted c = good; c.succ_row[2] = (uint32_t)c.kind.size(); EXPECT(faults_of(c) == FW_BAD_SUCC, "successor row == n_entries"); }
    { Contracted c = good; c.succ_row[3] = 0xFFFFFFFEu; EXPECT(faults_of(c) == FW_BAD_SUCC, "successor row just below the sentinel"); }
    { Contracted c = good; c.succ_row[0] = FW_NO_ROW; EXPECT(faults_of(c) == FW_OK, "an empty slot"); }
    { Contracted c = good; c.starts[0] = (uint32_t)c.kind.size(); EXPECT(faults_of(c) == FW_BAD_START, "start == n_entries"); }
    { Contracted c = good; c.starts.push_back(0xFFFFFFFFu); c.kind[2] = 9;
      EXPECT(faults_of(c) == (FW_BAD_START | FW_BAD_KIND), "two faults at once"); }
}

static void check_budget() {
    // a ladder of branch nodes: 2^8 paths
    std::vector<E> edges;
    const int rungs = 8;
    for (int r = 0; r < rungs; ++r) {
        const int b = 3 * r;
        edges.push_back({b, b + 1, 2}); edges.push_back({b, b + 2, 1});
        edges.push_back({b + 1, b + 3, 1}); edges.push_back({b + 2, b + 3, 1});
    }
    const Toy t = make(3 * rungs + 1, edges, {0}, {});
    const Walked full = check(t, "ladder");
    EXPECT(full.contigs.size() == 256, "the ladder has %zu paths", full.contigs.size());
    const Contracted c = contract(t);
    EXPECT(!walk(t, c, 5).ok, "five steps must not be enough");
    EXPECT(!walk(t, c, full.steps - 1).ok, "one step short");
    EXPECT(walk(t, c, full.steps).ok, "the exact number of steps");
}

int main() {
    required_cases();
    random_cases();
    deep_comb();
    check_validation();
    check_budget();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
