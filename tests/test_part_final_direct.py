"""dbg_part_final_walk / dbg_part_final_export on hand-built contracted graphs (csrc/dbg_partfinal.h, kernels k_fw_check and
k_fw_walk): the library takes the contracted graph as plain device columns, so these tests hand it graphs that no build of
reads produces and compare all six exported columns and the three sizes, for equality, with a recursive Python walker written
from the table of kinds in include/dbg.h and the reference's DFS (oracle/dbg_oracle.py: _walk_from) -- a set of on-path branch
rows, a list of the path's rows, no explicit stack.  The handle only has to hold a graph in parts: two short reads.

The graphs are seeded "combs" of B branch nodes behind a random permutation of the branch table, so consecutive on-path
branch nodes land in different words of the walker's bitmap, with empty slots before, between and after the used ones, back
edges that close on the path, skips ahead that reach branch nodes by two routes, a few "diamond" slots that double the path
count (some name the same row twice), pulled / dead / emitting successors, starts that are pulled, dead, or rows the branch
table names too, and garbage in d_branch wherever the kind is not 4.  B in {1, 31, 32, 33, 64, 65, 97} and n_starts in
{1, 63, 64, 65, 300} sit on the word edges of the bitmap and the wave edges of the 64-thread launch; one case per B has scores
and counts around 2^31.

What the committed seeds exercise, counted by the reference (the floors below are about half of each count):
  contigs whose path holds >= 40 branch levels                                   90 415  (deepest path: 97 levels)
  contigs whose on-path branch rows span >= 3 words of the bitmap               153 215
  emissions caused by a pulled successor                                         87 000
  pulled successors that emitted nothing, another one of the same visit had      16 538
  back edges followed to a branch node on the path, emitting nothing             21 434
  starts per walker: 1 everywhere but in the walker-loop case (65 536 + 65 starts), where walkers 0..64 take two

Every graph stays below 50 000 contigs and 2 000 000 piece rows (the reference refuses to count further); a seed above that is
replaced in SEEDS, never skipped.  Not covered: the rule that caps the walkers at 4 GiB of stacks -- it needs more than 2 700
branch nodes with 2^16 starts, a 4 GiB allocation.  No case here provokes a fault: every bad graph is one the validation
kernel is documented to stop before any index is followed."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import _dbg

EMIT, PULLED, BEFORE_PULLED, DEAD, BRANCH = range(5)
NO_ROW = 0xFFFFFFFF
K = 5                                   # the k of the handle's graph in parts: length = K + nodes - 1
CAP_CONTIGS, CAP_PIECES = 50_000, 2_000_000
LOOP_CAP_CONTIGS, LOOP_CAP_PIECES = 300_000, 2_000_000
SIZES_B = (1, 31, 32, 33, 64, 65, 97)
SIZES_STARTS = (1, 63, 64, 65, 300)
SEEDS = (11, 12, 13)
BIG_SEED, BIG_STARTS = 7, 65            # per B: the case whose scores and counts are around 2^31
FLOORS = {"deep": 45_000, "words3": 76_000, "pulled_emit": 43_000, "pulled_silent": 8_000, "back": 10_000}
MAX_WALKERS = 1 << 16                   # include/dbg.h: 2^16 walkers at most; start i goes to walker i % n_walkers


# ---- the generator ----------------------------------------------------------------------------------------------------------
class Comb:
    """kind / append / score / branch per entry row, succ_row / succ_cnt per (branch row, slot), starts; plain lists"""


def comb(seed, B, n_starts, diamonds=2, skips=2, backs=None, back_reach=None, big=False, loop=False):
    rng = random.Random(f"{seed}/{B}/{n_starts}/{int(big)}/{int(loop)}")
    perm = list(range(B))
    rng.shuffle(perm)                                      # comb position p is branch-table row perm[p]
    backs = B // 8 + 1 if backs is None else backs
    back_reach = B if back_reach is None else back_reach
    val = (lambda: (1 << 31) + rng.randrange(-1000, 1000)) if big else (lambda: rng.randrange(0, 1001))
    kind, append, score, branch = [], [], [], []

    def row(kd, pos=None):
        kind.append(kd)
        append.append(rng.randrange(0, 51))
        score.append(val())
        branch.append(perm[pos] if kd == BRANCH else rng.randrange(0, 1 << 32))   # garbage where it must not be read
        return len(kind) - 1

    succ_row, succ_cnt = [NO_ROW] * (4 * B), [0] * (4 * B)
    for p in range(B):
        slots = rng.sample(range(4), rng.randint(2, 4))
        onward = None
        for q, slot in enumerate(slots):
            if q == 0:                                     # the comb itself; its last node gets a leaf
                onward = r = row(BRANCH, p + 1) if p + 1 < B else row(EMIT)
            else:
                what = rng.choice(("emit",) * 4 + ("pulled",) * 4 + ("before",) * 2 + ("dead", "back", "back", "skip", "diamond"))
                if what == "back" and backs > 0:
                    backs -= 1
                    r = row(BRANCH, rng.randrange(max(0, p - back_reach), p + 1))
                elif what == "skip" and skips > 0 and p + 2 < B:
                    skips -= 1
                    r = row(BRANCH, rng.randrange(p + 2, B))
                elif what == "diamond" and diamonds > 0 and p + 1 < B:
                    diamonds -= 1
                    r = onward if rng.random() < 0.5 else row(BRANCH, p + 1)   # two slots may name the same row
                else:
                    r = row({"pulled": PULLED, "before": BEFORE_PULLED, "dead": DEAD}.get(what, EMIT))
            succ_row[4 * perm[p] + slot] = r
            succ_cnt[4 * perm[p] + slot] = val()
    n_table = len(kind)
    starts = []
    for i in range(n_starts):
        roll = rng.random()
        if loop:   # short combs everywhere, but both starts of the walkers 0..64 enter in the comb's first half
            shared = i < 65 or i >= MAX_WALKERS
            if shared or roll < 0.5:
                starts.append(row(BRANCH, rng.randrange(B // 4, B // 2) if shared else rng.randrange(B - 4, B)))
            else:
                starts.append(row(rng.randrange(0, 4)))
        elif i == 0 or roll < 1.5 / n_starts:
            starts.append(row(BRANCH, 0))                  # the deepest stack
        elif roll < min(0.4, 10 / n_starts):               # about ten deep walks a graph keep the enumeration bounded
            starts.append(row(BRANCH, rng.randrange(0, B)))
        elif roll < min(0.65, 22 / n_starts):
            starts.append(rng.randrange(0, n_table))       # a row the branch table names too, of any kind
        else:
            starts.append(row(rng.randrange(0, 4)))        # bare: emits itself, or nothing
    relabel = list(range(len(kind)))
    rng.shuffle(relabel)                                   # rows in no order
    g = Comb()
    g.n_entries, g.n_branch, g.n_starts = len(kind), B, n_starts
    g.kind, g.append, g.score, g.branch = ([0] * len(kind) for _ in range(4))
    for old, new in enumerate(relabel):
        g.kind[new], g.append[new], g.score[new], g.branch[new] = kind[old], append[old], score[old], branch[old]
    g.succ_row = [NO_ROW if r == NO_ROW else relabel[r] for r in succ_row]
    g.succ_cnt = succ_cnt
    g.starts = [relabel[r] for r in starts]
    return g


# ---- the reference ----------------------------------------------------------------------------------------------------------
class TooLarge(Exception):
    pass


class Ref:
    pass


def reference(g, k=K, cap_contigs=CAP_CONTIGS, cap_pieces=CAP_PIECES):
    """Every simple path of every start over the contracted graph, recursively.  -> Ref with contigs (start ordinal, ordinal
    within the start, length, score, piece rows) in start order and DFS order, pushed[i] (branch levels start i pushed),
    touched[i] (the branch rows it entered) and the counts the floors are about."""
    ref = Ref()
    ref.contigs, ref.pushed, ref.touched = [], [], []
    ref.stats = dict.fromkeys(FLOORS, 0)
    ref.deepest = ref.n_pieces = 0
    on_path, path, words = set(), [], {}
    state = {}

    def emit(i, nodes, score, last):
        rows = path + [last] if last is not None else list(path)
        ref.contigs.append((i, state["seq"], k + nodes - 1, score, rows))
        state["seq"] += 1
        ref.n_pieces += len(rows)
        if len(ref.contigs) > cap_contigs or ref.n_pieces > cap_pieces:
            raise TooLarge()
        ref.stats["deep"] += len(path) >= 40
        ref.stats["words3"] += len(words) >= 3
        ref.deepest = max(ref.deepest, len(path))

    def enter(i, r, count, nodes, score, visit):
        """DFS(current = the entry of row r) over an edge of `count` from a path of `nodes` nodes; visit: the parent branch
        node's visit (None at the start), visit[0] once a pulled successor made it emit the path up to the parent"""
        kd = g.kind[r]
        if kd == DEAD:
            return
        if kd == PULLED:
            if visit is not None:
                if visit[0]:
                    ref.stats["pulled_silent"] += 1
                else:
                    visit[0] = True
                    ref.stats["pulled_emit"] += 1
                    emit(i, nodes, score, None)
            return
        nodes += 1 + g.append[r]
        score += count + g.score[r]
        if kd != BRANCH:
            emit(i, nodes, score, r)
            return
        b = g.branch[r]
        if b in on_path:
            ref.stats["back"] += 1
            return
        on_path.add(b)
        path.append(r)
        words[b >> 5] = words.get(b >> 5, 0) + 1
        state["pushed"] += 1
        state["touched"].add(b)
        mine = [False]
        for slot in range(4):
            nx = g.succ_row[4 * b + slot]
            if nx != NO_ROW:
                enter(i, nx, g.succ_cnt[4 * b + slot], nodes, score, mine)
        path.pop()
        on_path.remove(b)
        words[b >> 5] -= 1
        if not words[b >> 5]:
            del words[b >> 5]

    for i, s in enumerate(g.starts):
        state.update(seq=0, pushed=0, touched=set())
        enter(i, s, 0, 0, 0, None)
        assert not on_path and not path
        ref.pushed.append(state["pushed"])
        ref.touched.append(state["touched"])
    ref.n_contigs = len(ref.contigs)
    ref.n_chars = sum(c[2] for c in ref.contigs)
    return ref


def walker_needs(ref, n_starts):
    """steps per walker: one per successor slot tried and one per level popped (include/dbg.h), 5 per level pushed"""
    n_walkers = min(n_starts, MAX_WALKERS)
    need = [0] * n_walkers
    for i, p in enumerate(ref.pushed):
        need[i % n_walkers] += 5 * p
    return need


def columns_of(ref):
    off = np.zeros(ref.n_contigs + 1, dtype=np.uint64)
    np.cumsum([len(c[4]) for c in ref.contigs], out=off[1:])
    return {"start_ordinal": np.array([c[0] for c in ref.contigs], dtype=np.uint32),
            "seq": np.array([c[1] for c in ref.contigs], dtype=np.uint32),
            "length": np.array([c[2] for c in ref.contigs], dtype=np.uint64),
            "score": np.array([c[3] for c in ref.contigs], dtype=np.uint64),
            "piece_off": off,
            "piece_row": np.array([r for c in ref.contigs for r in c[4]], dtype=np.uint32)}


_cache = {}


def case(*key, **kw):
    """(graph, reference), computed once per case and left unchanged"""
    ck = (key, tuple(sorted(kw.items())))
    if ck not in _cache:
        g = comb(*key, **kw)
        caps = {"cap_contigs": LOOP_CAP_CONTIGS, "cap_pieces": LOOP_CAP_PIECES} if kw.get("loop") else {}
        _cache[ck] = (g, reference(g, **caps))
    return _cache[ck]


def cases_of(B):
    return [((seed, B, n), {}) for n in SIZES_STARTS for seed in SEEDS] + [((BIG_SEED, B, BIG_STARTS), {"big": True})]


def loop_case():
    return case(1, 40, MAX_WALKERS + 65, diamonds=0, skips=0, back_reach=2, loop=True)


# ---- without a GPU: the committed seeds against the caps and the floors -----------------------------------------------------
def test_the_committed_seeds_stay_under_the_caps_and_reach_the_floors():
    total = dict.fromkeys(FLOORS, 0)
    n = deepest = 0
    for B in SIZES_B:
        for key, kw in cases_of(B):
            _, ref = case(*key, **kw)        # TooLarge: replace the seed
            assert ref.n_contigs <= CAP_CONTIGS and ref.n_pieces <= CAP_PIECES
            for name in total:
                total[name] += ref.stats[name]
            deepest = max(deepest, ref.deepest)
            n += 1
    assert n == len(SIZES_B) * (len(SIZES_STARTS) * len(SEEDS) + 1)
    assert deepest == 97
    for name, floor in FLOORS.items():
        assert total[name] >= floor, (name, total)


def test_the_reference_on_graphs_small_enough_to_read():
    """the reference itself, on three graphs whose answer is written out by hand"""
    g = Comb()
    # row 0 -> branch 0 with slots (empty, pulled row 1, row 2 -> branch 0 again, pulled row 1, emit row 3)
    g.kind, g.append, g.score, g.branch = [BRANCH, PULLED, BRANCH, EMIT], [2, 9, 1, 4], [10, 99, 20, 30], [0, 7, 0, 7]
    g.succ_row, g.succ_cnt, g.starts = [NO_ROW, 1, 2, 3], [0, 5, 6, 7], [0, 1, 3]
    ref = reference(g, k=5)
    assert ref.contigs == [(0, 0, 5 + 3 - 1, 10, [0]), (0, 1, 5 + 3 + 5 - 1, 10 + 7 + 30, [0, 3]), (2, 0, 5 + 5 - 1, 30, [3])]
    assert ref.pushed == [1, 0, 0] and ref.stats["back"] == 1 and ref.stats["pulled_emit"] == 1
    g.succ_row = [1, 1, NO_ROW, 3]           # two pulled successors of one visit: one prefix
    ref = reference(g, k=5)
    assert [c[4] for c in ref.contigs] == [[0], [0, 3], [3]] and ref.stats["pulled_silent"] == 1
    g.succ_row = [3, NO_ROW, NO_ROW, 3]      # two slots name the same row: two edges, two contigs
    ref = reference(g, k=5)
    assert [c[3] for c in ref.contigs] == [10 + 0 + 30, 10 + 7 + 30, 30] and walker_needs(ref, 3) == [5, 0, 0]


# ---- on the GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    g = _dbg.Graph()
    blob = np.frombuffer(b"ACGTTGCATGGTTGCATGCC", dtype=np.uint8)
    g.set_reads(blob, np.array([0, 10, 20], dtype=np.uint64))
    g.build_multipass(K, 2)
    yield g
    g.close()


def device_columns(g, dev):
    import torch

    def col(values, np_type, torch_type):
        return torch.from_numpy(np.array(values, dtype=np_type).view(torch_type[0])).to(dev).to(torch_type[1]).contiguous()
    u32 = (np.uint32, (np.int32, torch.int32))
    return [col(g.kind, np.uint8, (np.uint8, torch.uint8)), col(g.append, np.uint64, (np.int64, torch.int64)),
            col(g.score, np.uint64, (np.int64, torch.int64)), col(g.branch, *u32), col(g.succ_row, *u32), col(g.succ_cnt, *u32),
            col(g.starts, *u32)]


def walk(handle, g, max_chars=1 << 62, cols=None):
    return handle.part_final_walk(*(cols or device_columns(g, handle._dev())), max_chars=max_chars)


def assert_equal(got, ref, tag=""):
    assert (got["n_contigs"], got["n_pieces"], got["n_chars"]) == (ref.n_contigs, ref.n_pieces, ref.n_chars), tag
    for name, want in columns_of(ref).items():
        assert got[name].dtype == want.dtype and np.array_equal(got[name], want), f"{tag}: {name}"


def export_refusal(handle):
    """dbg_part_final_export must refuse: -> its message"""
    rc = handle._lib.dbg_part_final_export(handle._h, None, None, None, None, None, None)
    assert rc == _dbg.DBG_E_ARG
    return handle._lib.dbg_last_error(handle._h).decode()


_ran = {}


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES_B)
def test_comb_graphs_equal_the_reference(handle, B):
    stats = dict.fromkeys(FLOORS, 0)
    n = 0
    for key, kw in cases_of(B):
        g, ref = case(*key, **kw)
        assert_equal(walk(handle, g), ref, f"{key} {kw}")
        for name in stats:
            stats[name] += ref.stats[name]
        n += 1
    assert n == len(SIZES_STARTS) * len(SEEDS) + 1          # no case was dropped
    _ran[B] = stats
    if len(_ran) == len(SIZES_B):                             # over all sizes: what the device was compared on
        for name, floor in FLOORS.items():
            assert sum(s[name] for s in _ran.values()) >= floor, (name, _ran)


@pytest.mark.gpu
def test_a_walker_takes_a_second_start(handle):
    g, ref = loop_case()
    assert g.n_starts == MAX_WALKERS + 65 and ref.n_contigs < 300_000
    for w in range(65):   # the second start enters branch nodes the first had on its path: a bit left set would silence it
        first, second = ref.touched[w], ref.touched[w + MAX_WALKERS]
        assert first & second and ref.pushed[w] >= 10 and ref.pushed[w + MAX_WALKERS] >= 10
    t0 = time.perf_counter()
    got = walk(handle, g)
    print(f"walker loop: {ref.n_contigs} contigs, walk {time.perf_counter() - t0:.2f} s")
    assert_equal(got, ref, "walker loop")
    per_start = np.bincount(got["start_ordinal"], minlength=g.n_starts)
    assert per_start[:65].min() > 0 and per_start[MAX_WALKERS:].min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one start a walker", "walker loop"])
def test_the_step_budget_is_the_sum_over_a_walkers_starts(handle, which):
    g, ref = case(12, 33, 64) if which == "one start a walker" else loop_case()
    need = walker_needs(ref, g.n_starts)
    most = max(need)
    assert most >= 5 * 20
    if which == "walker loop":   # a budget a start: every start alone fits into one step less
        assert most > 5 * max(ref.pushed) and need.index(most) < 65
    cols = device_columns(g, handle._dev())
    try:
        handle.set_option("part_final_walk_steps", most)
        assert_equal(walk(handle, g, cols=cols), ref, "the exact budget")
        handle.set_option("part_final_walk_steps", most - 1)
        with pytest.raises(_dbg.DbgError) as e:
            walk(handle, g, cols=cols)
        assert e.value.code == _dbg.DBG_E_CAPACITY and "part_final_walk_steps" in str(e.value)
        assert e.value.sizes == {"n_contigs": 0, "n_pieces": 0, "n_chars": 0}
        assert "must run first" in export_refusal(handle)
    finally:
        handle.set_option("part_final_walk_steps", 1 << 24)   # the default
    assert_equal(walk(handle, g, cols=cols), ref, "the default budget")


@pytest.mark.gpu
def test_max_chars_keeps_the_sizes_and_writes_nothing(handle):
    g, ref = case(11, 65, 63)
    cols = device_columns(g, handle._dev())
    assert_equal(walk(handle, g, max_chars=ref.n_chars, cols=cols), ref, "the exact bound")
    with pytest.raises(_dbg.DbgError) as e:
        walk(handle, g, max_chars=ref.n_chars - 1, cols=cols)
    assert e.value.code == _dbg.DBG_E_CAPACITY and "max_chars" in str(e.value)
    assert e.value.sizes == {"n_contigs": ref.n_contigs, "n_pieces": ref.n_pieces, "n_chars": ref.n_chars}
    assert "sizes only" in export_refusal(handle)
    assert_equal(walk(handle, g, max_chars=0, cols=cols), ref, "the bound lifted")


# ---- validation: k_fw_check stops every bad graph before an index is followed ----------------------------------------------
FAULTS = {"kind": "a kind is not one of the five", "branch": "names a branch row that is not below n_branch",
          "succ": "a successor row of the branch table is neither below n_entries nor DBG_NO_NODE", "start": "a start is not below n_entries"}


def valid_graph():
    g, ref = case(13, 65, 300)
    assert g.n_entries > 257 and 4 * g.n_branch > 257 and g.n_starts > 257   # index 256: the second block of k_fw_check
    return g, ref


def break_at(cols, g, fault, where):
    """one fault in (a clone of) its column, at the first, the last or the 257th element"""
    kind, _, _, branch, succ_row, _, starts = cols = [c.clone() for c in cols]
    at = {"first": 0, "last": -1, "256": 256}[where]
    if fault == "kind":
        kind[at] = 5
    elif fault == "branch":
        kind[at] = BRANCH
        branch[at] = g.n_branch
    elif fault == "succ":
        succ_row[at] = g.n_entries
    else:
        starts[at] = g.n_entries
    return cols


def refused(handle, g, cols, names):
    with pytest.raises(_dbg.DbgError) as e:
        walk(handle, g, cols=cols)
    assert e.value.code == _dbg.DBG_E_ARG and "no walk ran" in str(e.value)
    for name, text in FAULTS.items():
        assert (text in str(e.value)) == (name in names), (names, str(e.value))
    assert e.value.sizes == {"n_contigs": 0, "n_pieces": 0, "n_chars": 0}
    assert "must run first" in export_refusal(handle)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last", "256"])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_each_fault_is_named_and_no_walk_runs(handle, fault, where):
    g, _ = valid_graph()
    refused(handle, g, break_at(device_columns(g, handle._dev()), g, fault, where), [fault])


@pytest.mark.gpu
def test_two_faults_name_both_and_a_garbage_branch_is_none(handle):
    g, ref = valid_graph()
    good = device_columns(g, handle._dev())
    refused(handle, g, break_at(break_at(good, g, "kind", "last"), g, "start", "first"), ["kind", "start"])
    refused(handle, g, break_at(break_at(good, g, "succ", "256"), g, "branch", "256"), ["succ", "branch"])
    cols = [c.clone() for c in good]
    not_branch = cols[0] != BRANCH
    assert int(not_branch.sum()) > 100
    cols[3][not_branch] = -1                  # 0xFFFFFFFF: far above n_branch, on rows whose branch is not read
    assert_equal(walk(handle, g, cols=cols), ref, "garbage branch")


@pytest.mark.gpu
def test_null_successor_columns(handle):
    import torch
    g = Comb()    # no branch node at all: bare starts only, one of each kind and a row named twice
    g.kind, g.append, g.score, g.branch = [EMIT, PULLED, BEFORE_PULLED, DEAD], [3, 4, 0, 6], [1 << 33, 8, 9, 10], [5, 6, 7, 8]
    g.succ_row, g.succ_cnt, g.starts = [], [], [3, 2, 1, 0, 2]
    g.n_entries, g.n_branch, g.n_starts = 4, 0, 5
    ref = reference(g)
    assert [c[:4] for c in ref.contigs] == [(1, 0, K, 9), (3, 0, K + 3, 1 << 33), (4, 0, K, 9)]
    cols = device_columns(g, handle._dev())
    assert cols[4].numel() == 0               # the binding passes NULL for an empty column
    assert_equal(walk(handle, g, cols=cols), ref, "no branch node")
    # the same columns with n_branch = 1 and no branch table
    sk = _dbg.FinalSkeleton(4, 1, 5, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), None, None,
                            cols[6].data_ptr())
    sizes = [C.c_uint64(7) for _ in range(3)]
    torch.cuda.synchronize(handle._dev())
    rc = handle._lib.dbg_part_final_walk(handle._h, C.byref(sk), 0, *[C.byref(s) for s in sizes])
    assert rc == _dbg.DBG_E_ARG and "null column" in handle._lib.dbg_last_error(handle._h).decode()
    assert [s.value for s in sizes] == [0, 0, 0]
    assert "must run first" in export_refusal(handle)


# ---- lifetime ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_result_belongs_to_the_current_graph(handle):
    (g1, ref1), (g2, ref2) = case(11, 33, 65), case(12, 31, 63)
    assert ref1.n_contigs != ref2.n_contigs
    assert_equal(walk(handle, g1), ref1, "first")
    got = walk(handle, g2)                     # a second walk replaces the first one's result
    assert_equal(got, ref2, "second")
    again = {name: np.empty_like(got[name]) for name in ("start_ordinal", "seq", "length", "score", "piece_off", "piece_row")}
    handle._chk(handle._lib.dbg_part_final_export(handle._h, *[again[n].ctypes.data_as(C.c_void_p) for n in again]))
    for name in again:
        assert np.array_equal(again[name], got[name]), name
    handle.build_multipass(K, 2)               # the next build frees it
    assert "must run first" in export_refusal(handle)
    assert_equal(walk(handle, g1), ref1, "after the build")
