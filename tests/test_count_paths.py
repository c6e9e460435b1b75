"""The LDS count kernels' split, spill and retry paths, on inputs built for their compile-time limits.

The five count kernels (k_sk_count, k_sk_count2, k_sk_count3: k <= 31; k_wsk_count, k_wsk_count2: k > 31) hold paths that run
only when a bucket exceeds a capacity fixed at compile time.  Each such branch raises an event bit (CountEvent, csrc/dbg_device.h)
that the host reports as the counter "count_events"; the sub-range passes and the repeated launches are counted beside it.  Every
input below is checked on the CPU (numpy and the C oracle alone) for the condition that makes its path unavoidable, or, where the
order of the records inside a bucket decides, for the weaker bound that can be proven; the event bit carries the rest of the proof.

    kernel         limit                               event bit        set by
    -------------  ----------------------------------  ---------------  ----------------------------------------------
    all five       r_n > split_recs                    EV_PRESPLIT      P (the bucket of the shared minimizer)
    all five       table full, bucket counted whole    EV_SPLIT_ROOT    A, B, D
    all five       table full inside a sub-range       EV_SPLIT_PART    A, D, P
    k_sk_count2    > PSEG pending edges in a wave      EV_PEND_OVER     C at k = 13 and 31 (no split), A
    k_sk_count     > QBUF (768 / 640) queries a pass   EV_QUERY_SPILL   A, B, P, C at k = 13 (no split)
    k_sk_count2    > QS (512 / 256) queries a pass     EV_QUERY_SPILL   A, B, P, C at k = 13 (no split)
    k_sk_count3    > QBUF (256) queries a pass         EV_QUERY_SPILL   A, B, P, C at k = 13 (no split)
    k_sk_count3    > DSEG (64) deferred edges a wave   EV_DEFER_SPILL   A, B, P, C at k = 13 (no split)
    k_wsk_count    > QBUF (320 / 160) queries a pass   EV_QUERY_SPILL   A, B, P
    k_wsk_count2   > QBUF (128) queries a pass         EV_QUERY_SPILL   A, B, P
    k_wsk_count2   > DSEG (104) deferred edges a wave  EV_DEFER_SPILL   A, B, P
    host           STATUS_QUERY_CAP                    count_retries_query_cap   A (k >= 21), B, P
    host           STATUS_COUNTER16                    count_retries_counter16   D

A start in hash sub-ranges needs split_recs, and split_recs needs the distinct-k-mer estimate, which the partition stage samples only
when it chooses the geometry itself ("bucket_bits" 0) -- under a forced "bucket_bits" no bucket ever starts in parts.  Inputs A, B, C
and D force the geometry: the buckets of A, B and D are counted whole first, overflow (EV_SPLIT_ROOT) and, where a half still does
not fit, overflow again (EV_SPLIT_PART).  Input P is built for the start in parts: the default geometry and some thousand records
that share one minimizer, hence one bucket.

Not covered, and why:
  * STATUS_BUCKET_TOO_BIG needs eight consecutive overflows below a part, i.e. millions of distinct k-mers in one bucket: not a
    test of a few seconds.
  * EV_MULTI_STAGE (r_n > STAGE) was not defined: the staging loop's second round has no branch of its own to raise it in, and an
    ordinary bucket of the benchmark takes that loop.  Inputs A, C and D stage every bucket in dozens of rounds all the same.
  * A two-word bucket without a split cannot exceed k_wsk_count's 320 staged queries or k_wsk_count2's 104 deferred edges a wave: a
    pass without a split holds at most 4 096 distinct k-mers in records of about ten, so about 400 record ends, half of which stay
    in the bucket.  Those limits are reached through the splits of A and B only.
  * k_wsk_count2 raises EV_QUERY_SPILL from its deferred lookups (wave by wave), not from the lookups "where they are found": a
    second atomic there costs the kernel a register and three spills.  k_sk_count3 raises it from both.
  * NODE_EDGE_CAP retries are test_hip_engines.test_capacity_retry_when_the_estimate_is_low's; here count_retries_node_cap is
    asserted 0 next to the other retries.

Measured on an MI355X: the 93 GPU tests of this module take 17 s together, the slowest 0.8 s; the CPU tests 4 s.
"""
import functools
import os
import re

import numpy as np
import pytest

import _dbg
import synth
from oracle import orc_c
from test_extract_shared_hashes import minimizers, n_records_expected

gpu = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "py-debruijn_amd", "csrc")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# ---- copied from the headers (test_constants_equal_the_headers compares) -------------------------------------------------------
EV_PRESPLIT, EV_SPLIT_ROOT, EV_SPLIT_PART, EV_PEND_OVER, EV_QUERY_SPILL, EV_DEFER_SPILL = 1, 2, 4, 8, 16, 32
EV_SPLIT = EV_SPLIT_ROOT | EV_SPLIT_PART
EV_NAMES = {"PRESPLIT": 1, "SPLIT_ROOT": 2, "SPLIT_PART": 4, "PEND_OVER": 8, "QUERY_SPILL": 16, "DEFER_SPILL": 32}
SC_COUNT_EVENTS = 7
CAP = 4096              # slots of the LDS table, both engines (lds_slots 4096, WCAP)
START_PARTS_MAX = 16    # hash sub-ranges a bucket can start in
SPLIT_FILL = 0.80       # split_recs = SPLIT_FILL * CAP / (estimated distinct k-mers per record)
CNT_STACK = 24
SK_QBUF = {4: 768, 8: 640}                                      # k_sk_count: staged records = staged queries, by stamp bytes
SK2 = {4: dict(QBUF=768, QS=512, PEND=4096), 8: dict(QBUF=320, QS=256, PEND=2048)}
SK2_WAVES = 16                                                  # PSEG = PEND / 16 pending edges per wave
SK3 = dict(STAGE=768, QBUF=256, DSEG=64)
WSK = {4: dict(STAGE=288, QBUF=320), 8: dict(STAGE=128, QBUF=160)}
WSK2 = dict(STAGE=256, QBUF=128, DSEG=104)                      # DSEG = STAGE * WCNT_QMAX (13) / (WCNT_NT / 64 = 16 waves) / 2


def without_profiling_branches(text):
    """The header as the product build sees it: #ifdef DBG_CNT_PROF ... [#else ...] #endif keeps the #else side."""
    out, state, depth = [], 0, 0  # state: 0 outside, 1 in the profiling side, 2 in the #else side; depth: conditionals nested in it
    for line in text.splitlines():
        s = line.strip()
        if state == 0 and s.startswith("#ifdef DBG_CNT_PROF"):
            state = 1
            continue
        if state and s.startswith("#if"):
            depth += 1
        elif state and depth and s.startswith("#endif"):
            depth -= 1
            if state == 1:
                continue
        elif state == 1 and not depth and s.startswith("#else"):
            state = 2
            continue
        elif state and not depth and s.startswith("#endif"):
            state = 0
            continue
        if state != 1:
            out.append(line)
    return "\n".join(out)


def header(name):
    with open(os.path.join(CSRC, name)) as fh:
        return without_profiling_branches(fh.read())


def one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def test_constants_equal_the_headers():
    dev = header("dbg_device.h")
    assert {n: int(v) for n, v in re.findall(r"\bEV_(\w+) = (\d+),", dev)} == EV_NAMES
    assert int(one(r"constexpr int SC_COUNT_EVENTS = (\d+);", dev)) == SC_COUNT_EVENTS
    sk = header("dbg_sk.h")
    q8, q4, q2048 = one(r"QBUF = CAP == 4096 \? \(sizeof\(ST\) == 8 \? (\d+) : (\d+)\) : (\d+);", sk)
    assert {4: int(q4), 8: int(q8)} == SK_QBUF
    assert int(one(r"constexpr int CNT_STACK = (\d+);", sk)) == CNT_STACK
    sk2 = header("dbg_sk2.h")
    for name in ("QBUF", "QS", "PEND"):
        v8, v4 = one(r"static constexpr int %s = sizeof\(ST\) == 8 \? (\d+) : (\d+);" % name, sk2)
        assert (int(v4), int(v8)) == (SK2[4][name], SK2[8][name]), name
    assert int(one(r"static constexpr int CAP = (\d+);", sk2)) == CAP
    assert one(r"constexpr int PSEG = PEND / (\d+);", sk2) == str(SK2_WAVES)
    sk3 = header("dbg_sk3.h")
    assert one(r"static constexpr int CAP = (\d+), NT = (\d+);", sk3) == (str(CAP), "1024")
    for name in ("STAGE", "QBUF", "DSEG"):
        assert int(one(r"static constexpr int %s = (\d+);" % name, sk3)) == SK3[name], name
    wsk = header("dbg_wsk.h")
    assert int(one(r"constexpr int WCAP = (\d+);", wsk)) == CAP
    for name in ("STAGE", "QBUF"):
        v8, v4 = one(r"static constexpr int %s = sizeof\(ST\) == 8 \? (\d+) : (\d+);" % name, wsk)
        assert (int(v4), int(v8)) == (WSK[4][name], WSK[8][name]), name
    qmax, nt = int(one(r"constexpr int WCNT_QMAX = (\d+);", wsk)), int(one(r"#define DBG_WCNT_NT (\d+)", wsk))
    wsk2 = header("dbg_wsk2.h")
    for name in ("STAGE", "QBUF"):
        assert int(one(r"static constexpr int %s = (\d+);" % name, wsk2)) == WSK2[name], name
    assert "DSEG = STAGE * WCNT_QMAX / (WCNT_NT / 64) / 2;" in wsk2 and WSK2["STAGE"] * qmax // (nt // 64) // 2 == WSK2["DSEG"]
    for name in ("dbg_sk.h", "dbg_sk2.h", "dbg_sk3.h", "dbg_wsk.h", "dbg_wsk2.h"):  # the start in sub-ranges, alike in all five
        assert one(r"while \(parts < (\d+) && \(uint64_t\)parts \* split_recs < r_n\) parts <<= 1;", header(name)) == str(START_PARTS_MAX)
    host = header("dbg_hip.hip")
    assert re.findall(r"\((?:W?CAP) \* (0\.\d+)\) / \(est_distinct / \(double\)n_rec\)", host) == ["%.2f" % SPLIT_FILL] * 2
    assert float(one(r"const double want = \(double\)n_inst \* own \* (0\.\d+) / target;", host)) == AUTO_DISTINCT_SHARE
    assert float(one(r"constexpr double SK_TARGET_DISTINCT = CAP \* (0\.\d+);", host)) == TARGET_FILL
    assert int(one(r"if \(auto_T && l1 >= (\d+) && n_rec\) \{  // refine T from a sample", host)) == L1_ESTIMATE_FROM


# ---- the inputs -----------------------------------------------------------------------------------------------------------------
def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def flat(rows):
    """(bases, offsets) of a 2-D array of equally long reads."""
    return frozen(rows.reshape(-1)), np.arange(0, rows.size + 1, rows.shape[1], dtype=np.uint64)


A_KS, A_WIDE_KS = (13, 21, 31), (32, 40, 63)
B_KS = (31, 40)
B_SHAPE = {31: dict(read_len=100, genome=900_000, n_reads=4_700), 40: dict(read_len=120, genome=900_000, n_reads=4_000)}
P_KS = (31, 40)
P_READS, P_FILLER_LEN, P_INSTANCES = 5_000, 2_000, 1_000_000
AUTO_DISTINCT_SHARE, TARGET_FILL, L1_ESTIMATE_FROM = 0.4, 0.36, 9  # sk_provisional_bits, SK_TARGET_DISTINCT, sk_partition's sample
C_GENOME, C_READ = 3_600, 100
C_COPIES = {13: 40, 31: 150}
D_COPIES, D_K = 70_000, 31


@functools.lru_cache(maxsize=None)
def input_a(wide):
    """A. Oversubscribed buckets: 200 kbp error-free at 3x (3.6x for the two-word engine's reads of 120), bucket_bits = 1."""
    return flat(synth.reads_ascii(7, 200_000, 6_000, 120 if wide else 100, 0.0))


@functools.lru_cache(maxsize=None)
def input_b(k):
    """B. bucket_bits = 6 over a random error-free genome at coverage 0.5, so that a bucket holds more than CAP distinct k-mers."""
    s = B_SHAPE[k]
    rng = np.random.default_rng(3)
    genome = ACGT[rng.integers(0, 4, s["genome"])]
    starts = rng.integers(0, s["genome"] - s["read_len"], s["n_reads"])
    return flat(genome[starts[:, None] + np.arange(s["read_len"])[None, :]])


def mmer_hash16(mm):
    """mmer_hash16 of csrc/dbg_minwin.h on packed m-mers (uint32), as test_extract_shared_hashes.minimizers restates it."""
    with np.errstate(over="ignore"):
        return ((mm ^ (mm >> np.uint32(9)) ^ np.uint32(0x3C6EF372)) * np.uint32(0x9E3779B1)) >> np.uint32(16)


@functools.lru_cache(maxsize=None)
def p_core():
    """A 13-mer of minimal hash (0): wherever a window holds it, it is the window's minimizer."""
    mm = np.random.default_rng(23).integers(0, 1 << 26, 1 << 20, dtype=np.uint32)
    mm = int(mm[np.flatnonzero(mmer_hash16(mm) == 0)[0]])
    return np.frombuffer(b"ACTG", dtype=np.uint8)[[(mm >> (2 * (12 - i))) & 3 for i in range(13)]]  # codes: A 0, C 1, T 2, G 3


@functools.lru_cache(maxsize=None)
def input_p(k):
    """P. 5 000 random reads with the same 13-mer in the middle, at the default geometry: the k - 12 k-mers of a read that hold it
    are one record, all these records fall into the bucket of that minimizer, and no two of them share a k-mer.  Random reads of
    2 000 follow until the input holds a million k-mer instances: below 2^8 * 0.36 * 4 096 / 0.4 = 943 719 the geometry has fewer
    than 9 level-1 bits, the partition stage takes no sample, and without its estimate no bucket starts in parts."""
    L = 120 if k > 31 else 100
    rng = np.random.default_rng(29)
    rows = ACGT[rng.integers(0, 4, (P_READS, L))]
    rows[:, L // 2 - 6:L // 2 + 7] = p_core()[None, :]
    n_fill = -(-(P_INSTANCES - P_READS * (L - k + 1)) // (P_FILLER_LEN - k + 1))
    filler = ACGT[rng.integers(0, 4, n_fill * P_FILLER_LEN)]
    off = np.concatenate([np.arange(0, P_READS * L, L), P_READS * L + np.arange(0, (n_fill + 1) * P_FILLER_LEN, P_FILLER_LEN)])
    return frozen(np.concatenate([rows.reshape(-1), filler])), off.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def input_c(k):
    """C. A 3 600-base random genome tiled by reads of 100 that overlap by k - 1 (every k-mer of the genome, each with its
    successor but the last), every read copied C_COPIES[k] times, shuffled; bucket_bits = 1."""
    rng = np.random.default_rng(17)
    genome = ACGT[rng.integers(0, 4, C_GENOME)]
    starts = list(range(0, C_GENOME - C_READ, C_READ - (k - 1))) + [C_GENOME - C_READ]
    rows = np.stack([genome[s:s + C_READ] for s in starts])
    rows = np.tile(rows, (C_COPIES[k], 1))
    return flat(rows[rng.permutation(rows.shape[0])])


@functools.lru_cache(maxsize=None)
def input_d():
    """D. Input A next to 70 000 copies of one read of 60 (test_count_kernel_16_bit_counters_fall_back_to_32_bit's)."""
    a, _ = input_a(False)
    read = synth.reads_ascii(4, 200, 1, 60, 0.0)[0]
    rng = np.random.default_rng(1)
    lens = np.concatenate([np.full(a.size // 100, 100), np.full(D_COPIES, 60)])
    which = rng.permutation(lens.size)
    pieces = [a[i * 100:(i + 1) * 100] if i < a.size // 100 else read for i in which]
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens[which], out=off[1:])
    return frozen(np.concatenate(pieces)), off


INPUTS = {"A": lambda k: input_a(k > 31), "B": input_b, "C": input_c, "D": lambda k: input_d(), "P": input_p}


@functools.lru_cache(maxsize=None)
def oracle(name, k):
    """The C oracle's node table of an input, computed once for the module and left unchanged."""
    bases, off = INPUTS[name](k)
    want = orc_c.build(bases, off, k)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def records(name, k):
    """Super-k-mer records of an input (numpy restatement of the extraction's rule, both engines)."""
    bases, off = INPUTS[name](k)
    valid, minpos, _ = minimizers(bases, off, k)
    return n_records_expected(valid, minpos)


# ---- the CPU conditions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", A_KS + A_WIDE_KS)
def test_a_oversubscribes_two_buckets(k):
    """Two buckets of 4 096 slots: more distinct k-mers than 2 * 4 096 overflow a table that holds a whole bucket, and more than
    2 * 2 * 4 096 overflow one of the four halves as well, whatever the hashes do.  (The bound for buckets that start in 16 parts,
    2 * 16 * 4 096, holds too, but no bucket starts in parts under a forced geometry: see the module's docstring.)
    Whether the queries outgrow the first launch's list: a_query_retry."""
    want = oracle("A", k)
    assert want["n_nodes"] > 2 * START_PARTS_MAX * CAP > 2 * 2 * CAP
    assert INPUTS["A"](k)[0].size <= 1_000_000
    assert a_query_retry(k) is not None


def a_query_retry(k):
    """Whether input A outgrows the first launch's query list (one query per record + 1 024).  Never, if there are no more distinct
    edges than that.  Else: a bucket of ~90 000 distinct k-mers ends in sub-ranges of 4 096 slots, 22 and more of them (masks of 15
    and 31), and a successor falls into its k-mer's sub-range with probability 1 / 16 at most, so 15 / 16 of the edges are queries
    in expectation, with a binomial's spread over ~180 000 edges; 0.9 of the edges is asked to exceed the list.  None: neither."""
    edges, room = int((oracle("A", k)["counts"] != 0).sum()), records("A", k) + 1024
    return False if edges <= room else True if 0.9 * edges > room else None


def test_a_measured_node_counts():
    assert [oracle("A", k)["n_nodes"] for k in A_KS] == [184_987, 181_275, 174_888]


@pytest.mark.parametrize("k", B_KS)
def test_b_overflows_buckets_that_start_whole(k):
    """64 buckets with more than 4 096 distinct k-mers on average: some bucket's table overflows (pigeonhole), and it was counted
    whole (forced geometry).  Copies of one read, meant to lift split_recs above the ordinary buckets' records, have nothing to
    lift under "bucket_bits" 6 and are left out."""
    want = oracle("B", k)
    assert input_b(k)[0].size <= 1_000_000
    assert want["n_nodes"] / 64 > CAP


@pytest.mark.parametrize("k", P_KS)
def test_p_crowds_one_minimizer(k):
    """Every read of P gives one record of k - 12 k-mers around the shared 13-mer; these records fall into one bucket, hold more
    distinct k-mers than 16 tables have slots, and are more than four times split_recs (from the exact distinct-per-record ratio;
    the build samples one level-1 bucket for it): the bucket starts in 16 parts and one of them overflows."""
    bases, off = input_p(k)
    assert bases.size <= 1_250_000  # (a million instances are a megabyte and more)
    want = oracle("P", k)
    assert want["n_kmer_instances"] >= P_INSTANCES
    assert want["n_kmer_instances"] * AUTO_DISTINCT_SHARE / (TARGET_FILL * CAP) > 1.05 * (1 << (L1_ESTIMATE_FROM - 1))
    L = 120 if k > 31 else 100
    valid, minpos, _ = minimizers(bases, off, k)
    at_core = valid & (minpos % L == L // 2 - 6) & (np.arange(valid.size) < P_READS * L)
    assert int(np.count_nonzero(at_core)) >= P_READS * (k - 12) * 0.99  # (another m-mer of hash 0 in the window takes a few)
    # the crowd's k-mers are distinct: each holds its read's own random flanks
    code = ((bases >> 1) & 3).astype(np.uint64)
    p = np.flatnonzero(at_core)
    sig = np.zeros(p.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(k):
            sig = sig * np.uint64(0x9E3779B97F4A7C15) + code[p + i] + np.uint64(1)
    distinct = np.unique(sig).size
    assert distinct > START_PARTS_MAX * CAP
    prev_min = np.concatenate([[-1], minpos[:-1]])
    crowd_records = int(np.count_nonzero(at_core & (prev_min != minpos)))
    n_rec = records("P", k)
    split_recs = SPLIT_FILL * CAP * n_rec / want["n_nodes"]
    print(f"P k={k}: nodes {want['n_nodes']}, records {n_rec}, split_recs {split_recs:.0f}, crowd {crowd_records} records, {distinct} k-mers")
    assert crowd_records > 4 * split_recs and crowd_records >= P_READS * 0.99


@pytest.mark.parametrize("k", sorted(C_COPIES))
def test_c_crowds_the_lists_without_filling_a_table(k):
    """Fewer distinct k-mers than one table has slots, even if all fell into one bucket: no table overflows, and under the forced
    geometry no bucket starts in parts.
    What can be proven about the lists: identical records collapse only inside one staging round of at most QBUF = 768 records,
    and a record instance whose last k-mer has a successor is one pending edge unless it collapsed.  The number of such
    instances of the fuller bucket, divided by the copies one round could absorb if the order were the worst (all copies of a record
    in the same round: C_COPIES), is the proven bound -- the distinct record ends, which is below PEND.  For a shuffled order the
    expectation is the instances / (copies a round of 768 holds of one record); that figure is asserted to exceed PEND, and the
    event bit proves that the kernel met it.  At k = 13 a record is one k-mer (w = 1): every distinct edge is a record end, about
    half of them leave the bucket (queries beyond k_sk_count's 768, k_sk_count2's 512, k_sk_count3's 256), and no lane hands a
    successor over (all of a wave's 4 x 64 nodes defer: beyond k_sk_count3's 64)."""
    want = oracle("C", k)
    bases, off = input_c(k)
    assert bases.size <= 1_000_000
    assert want["n_nodes"] <= 2 * 2_500 and want["n_nodes"] < C_GENOME < CAP
    n_rec = records("C", k)
    # record instances that end inside a read: the next k-mer is valid and opens a record
    valid, minpos, _ = minimizers(bases, off, k)
    opens = valid & np.concatenate([[False], valid[:-1]]) & (np.concatenate([[-1], minpos[:-1]]) != minpos)
    ends_with_successor = int(np.count_nonzero(opens))
    distinct_records = n_rec // C_COPIES[k]
    per_round = max(1.0, SK2[4]["QBUF"] / distinct_records)  # copies of one record in a round of a shuffled bucket
    expected_pending = ends_with_successor / 2 / per_round
    print(f"C k={k}: nodes {want['n_nodes']}, records {n_rec} ({distinct_records} distinct), record ends with a successor "
          f"{ends_with_successor}, expected pending edges a bucket {expected_pending:.0f}")
    assert expected_pending > SK2[4]["PEND"]
    if k == 13:
        assert n_rec == int(np.count_nonzero(valid))  # w = 1: every k-mer instance is a record
        edges = int((want["counts"] != 0).sum())
        assert edges // 4 > SK_QBUF[4]  # half of the edges start in a bucket, half of those end in the other (890 +- 21)
        assert want["n_nodes"] // 2 // 16 > SK3["DSEG"]  # nodes a wave of the emptier bucket


def test_d_repeats_a_build_that_splits():
    want = oracle("D", D_K)
    assert int(want["counts"].max()) >= D_COPIES > 0xFFFF
    assert want["n_nodes"] > 2 * START_PARTS_MAX * CAP


# ---- the builds -------------------------------------------------------------------------------------------------------------------
NARROW_KERNELS = [dict(count_kernel=1), dict(count_kernel=2), dict(count_kernel=3),
                  dict(stamp64=1, count_kernel_u64=1), dict(stamp64=1, count_kernel_u64=2), dict(stamp64=1, count_kernel_u64=3)]
WIDE_KERNELS = [dict(wcount_kernel=1), dict(wcount_kernel=2), dict(stamp64=1)]


def kernel_of(k, opts):
    """Which of the five kernels a build with these options runs."""
    if k > 31:
        return "k_wsk_count2" if opts.get("wcount_kernel", 2) == 2 and not opts.get("stamp64") else "k_wsk_count"
    which = opts["count_kernel_u64"] if opts.get("stamp64") else opts["count_kernel"]
    return {1: "k_sk_count", 2: "k_sk_count2", 3: "k_sk_count3"}[which]


SPILLS = {"k_sk_count": EV_QUERY_SPILL, "k_sk_count2": EV_QUERY_SPILL, "k_sk_count3": EV_QUERY_SPILL | EV_DEFER_SPILL,
          "k_wsk_count": EV_QUERY_SPILL, "k_wsk_count2": EV_QUERY_SPILL | EV_DEFER_SPILL}


def ident(opts):
    return "-".join(f"{n}{v}" for n, v in opts.items()) or "default"


def names(bits):
    return "|".join(n for n, b in EV_NAMES.items() if bits & b) or "none"


def build(name, k, **opts):
    g = _dbg.Graph()
    for n, v in opts.items():
        g.set_option(n, v)
    g.set_reads(*INPUTS[name](k))
    g.build(k)
    return g


def shifted(keys, keys_hi, code, k):
    """(lo, hi) of the successor k-mers: the k-mer shifted by one base `code` (two words for k > 31)."""
    u64 = np.uint64
    lo_mask = u64((1 << (2 * k)) - 1) if 2 * k < 64 else u64(0xFFFFFFFFFFFFFFFF)
    hi_mask = u64((1 << (2 * k - 64)) - 1) if 2 * k > 64 else u64(0)
    return ((keys << u64(2)) | u64(code)) & lo_mask, ((keys_hi << u64(2)) | (keys >> u64(62))) & hi_mask


def assert_equals_oracle(g, want, k):
    """test_engine_matches_c_oracle's and test_two_word_engine_matches_c_oracle's comparison: the node table in dict order, every
    successor and the CSR."""
    sz = g.sizes()
    assert sz["n_kmer_instances"] == want["n_kmer_instances"] and sz["n_edge_instances"] == want["n_edge_instances"]
    assert sz["n_nodes"] == want["n_nodes"] and sz["n_edges"] == int((want["counts"] != 0).sum())
    keys, stamps, counts, flags = g.export_nodes()
    hi = g.export_keys_hi()
    o = np.argsort(stamps, kind="stable")
    assert np.array_equal(keys[o], want["keys"]) and np.array_equal(hi[o], want["keys_hi"])
    assert np.array_equal(stamps[o], want["stamps"]) and np.array_equal(counts[o], want["counts"])
    assert np.array_equal(flags & 1, (stamps & np.uint64(1)).astype(np.uint8))
    succ = g.export_succ()
    rp, col, cnt = g.export_csr()
    assert int(rp[-1]) == sz["n_edges"] == int((counts != 0).sum())
    assert np.array_equal(col, succ[counts != 0]) and np.array_equal(cnt, counts[counts != 0])
    for code in range(4):
        has = counts[:, code] != 0
        assert np.all(succ[~has, code] == _dbg.NO_NODE) and np.all(succ[has, code] != _dbg.NO_NODE)
        lo, up = shifted(keys[has], hi[has], code, k)
        assert np.array_equal(keys[succ[has, code]], lo) and np.array_equal(hi[succ[has, code]], up)


def report(tag, k, opts, st):
    print(f"[{tag} k={k} {ident(opts)} {kernel_of(k, opts)}] events {names(st['count_events'])} extra_ranges "
          f"{st['count_extra_ranges']} launches {st['count_launches']} retries q/n/c16 {st['count_retries_query_cap']}/"
          f"{st['count_retries_node_cap']}/{st['count_retries_counter16']} buckets {st['n_buckets']} queries {st['n_queries']} "
          f"count {st['ms_count']:.2f} ms")


def a_params():
    for k in A_KS:
        for opts in NARROW_KERNELS:
            yield pytest.param(k, opts, id=f"k{k}-{ident(opts)}")
    for k in A_WIDE_KS:
        for opts in WIDE_KERNELS:
            yield pytest.param(k, opts, id=f"k{k}-{ident(opts)}")


@gpu
@pytest.mark.parametrize("k,opts", list(a_params()))
def test_a_splits_inside_parts_and_spills(k, opts):
    g = build("A", k, bucket_bits=1, **opts)
    try:
        st = g.stats()
        report("A", k, opts, st)
        assert st["n_buckets"] == 2
        assert_equals_oracle(g, oracle("A", k), k)
        need = EV_SPLIT_ROOT | EV_SPLIT_PART | SPILLS[kernel_of(k, opts)]
        assert st["count_events"] & need == need, names(need & ~st["count_events"])
        assert st["count_events"] & EV_PRESPLIT == 0
        assert st["count_extra_ranges"] >= -(-oracle("A", k)["n_nodes"] // CAP)  # every sub-range that was written fits a table
        retry = int(a_query_retry(k))
        assert (st["count_retries_query_cap"], st["count_retries_node_cap"], st["count_retries_counter16"]) == (retry, 0, 0)
        assert st["count_launches"] == 1 + retry
    finally:
        g.close()


def b_params():
    for k in B_KS:
        for opts in (NARROW_KERNELS if k <= 31 else WIDE_KERNELS):
            yield pytest.param(k, opts, id=f"k{k}-{ident(opts)}")


@gpu
@pytest.mark.parametrize("k,opts", list(b_params()))
def test_b_splits_at_the_root(k, opts):
    g = build("B", k, bucket_bits=6, **opts)
    try:
        st = g.stats()
        report("B", k, opts, st)
        assert st["n_buckets"] == 64
        assert_equals_oracle(g, oracle("B", k), k)
        need = EV_SPLIT_ROOT | SPILLS[kernel_of(k, opts)]
        assert st["count_events"] & need == need, names(need & ~st["count_events"])
        assert st["count_events"] & EV_PRESPLIT == 0
        assert st["count_extra_ranges"] >= 2
        assert (st["count_retries_node_cap"], st["count_retries_counter16"]) == (0, 0)
        assert st["count_launches"] == 1 + st["count_retries_query_cap"]
    finally:
        g.close()


def p_params():
    for k in P_KS:
        for opts in (NARROW_KERNELS if k <= 31 else WIDE_KERNELS):
            yield pytest.param(k, opts, id=f"k{k}-{ident(opts)}")


@gpu
@pytest.mark.parametrize("k,opts", list(p_params()))
def test_p_starts_in_parts_and_splits_them(k, opts):
    g = build("P", k, **opts)
    try:
        st = g.stats()
        report("P", k, opts, st)
        assert_equals_oracle(g, oracle("P", k), k)
        need = EV_PRESPLIT | EV_SPLIT_PART | SPILLS[kernel_of(k, opts)]
        assert st["count_events"] & need == need, names(need & ~st["count_events"])
        assert st["count_extra_ranges"] > START_PARTS_MAX
        assert (st["count_retries_node_cap"], st["count_retries_counter16"]) == (0, 0)
        assert st["count_launches"] == 1 + st["count_retries_query_cap"]
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("k", sorted(C_COPIES))
@pytest.mark.parametrize("opts", NARROW_KERNELS, ids=ident)
def test_c_overflows_the_lists_without_a_split(k, opts):
    g = build("C", k, bucket_bits=1, **opts)
    try:
        st = g.stats()
        report("C", k, opts, st)
        assert st["n_buckets"] == 2
        assert_equals_oracle(g, oracle("C", k), k)
        kern = kernel_of(k, opts)
        need = (EV_PEND_OVER if kern == "k_sk_count2" else 0) | (SPILLS[kern] if k == 13 else 0)
        assert st["count_events"] & need == need, names(need & ~st["count_events"])
        assert st["count_events"] & (EV_PRESPLIT | EV_SPLIT) == 0, names(st["count_events"])
        assert st["count_extra_ranges"] == 0
        assert (st["count_retries_query_cap"], st["count_retries_node_cap"], st["count_retries_counter16"]) == (0, 0, 0)
        assert st["count_launches"] == 1
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("opts", [dict(count_kernel=2), dict(count_kernel=3), dict(stamp64=1, count_kernel_u64=3)], ids=ident)
def test_d_counter_fallback_repeats_a_build_that_splits(opts):
    """The kernels with 16-bit counters meet an edge seen 70 000 times in a build that also overflows its tables at the root and
    below: the launch is repeated once with k_sk_count's 32-bit counters -- same graph.  (The copies' 200 000 records leave room
    for every query: no retry for the list.)"""
    g = build("D", D_K, bucket_bits=1, **opts)
    try:
        st = g.stats()
        report("D", D_K, opts, st)
        assert st["n_buckets"] == 2
        assert_equals_oracle(g, oracle("D", D_K), D_K)
        need = EV_SPLIT_ROOT | EV_SPLIT_PART | EV_QUERY_SPILL
        assert st["count_events"] & need == need, names(need & ~st["count_events"])
        assert st["count_retries_counter16"] == 1 and st["count_retries_node_cap"] == 0
        assert st["count_launches"] == 1 + st["count_retries_counter16"] + st["count_retries_query_cap"]
        assert st["count_extra_ranges"] >= -(-oracle("D", D_K)["n_nodes"] // CAP)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("k,opts", [(31, dict()), (31, dict(stamp64=1)), (40, dict()), (40, dict(stamp64=1))], ids=lambda v: ident(v) if isinstance(v, dict) else f"k{v}")
def test_an_ordinary_build_splits_nothing(k, opts):
    """test_extract_presplit's synthetic set at the default geometry: whatever else it reports, no table overflows."""
    reads = synth.reads_ascii(5, 200_000, 20_000, 100, 0.01)
    g = _dbg.Graph()
    try:
        for n, v in opts.items():
            g.set_option(n, v)
        g.set_reads(*flat(reads))
        g.build(k)
        st = g.stats()
        print(f"[ordinary k={k} {ident(opts)}] events {names(st['count_events'])} extra_ranges {st['count_extra_ranges']} buckets {st['n_buckets']}")
        assert st["count_events"] & EV_SPLIT == 0
        assert st["count_launches"] == 1
    finally:
        g.close()


# ---- the consumers of the extra ranges ----------------------------------------------------------------------------------------------
CONSUMER_CASES = [("A", 31, 1), ("A", 40, 1), ("B", 31, 6), ("B", 40, 6), ("P", 31, 0), ("P", 40, 0)]  # (input, k, bucket_bits)
consumers = pytest.mark.parametrize("name,k,bits", CONSUMER_CASES, ids=[f"{n}-k{k}" for n, k, _ in CONSUMER_CASES])


@gpu
@consumers
@pytest.mark.parametrize("direct", [0, 1])
def test_resolver_reads_the_extra_ranges(name, k, bits, direct):
    """The resolver with and without the shortcut through the directory line: the same graph, the oracle's."""
    g = build(name, k, bucket_bits=bits, resolve_direct=direct, resolve_count=1)
    try:
        st = g.stats()
        assert st["count_extra_ranges"] > 0 and st["n_queries"] > 0
        assert st["resolve_direct_hits"] + st["resolve_keyed"] == st["n_queries"]
        if not direct:
            assert st["resolve_direct_hits"] == 0
        assert_equals_oracle(g, oracle(name, k), k)
    finally:
        g.close()


@gpu
@consumers
def test_lookups_through_the_extra_ranges(name, k, bits):
    """Every node's k-mer and as many absent ones, through the build's directory and through the sorted index."""
    want = oracle(name, k)
    g = build(name, k, bucket_bits=bits)
    try:
        assert g.stats()["count_extra_ranges"] > 0
        keys, stamps, _, _ = g.export_nodes()
        hi = g.export_keys_hi()
        rng = np.random.default_rng(k)
        lo_mask = np.uint64((1 << (2 * k)) - 1) if 2 * k < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        hi_mask = np.uint64((1 << (2 * k - 64)) - 1) if 2 * k > 64 else np.uint64(0)
        r_lo = rng.integers(0, 1 << 63, keys.size, dtype=np.uint64) * np.uint64(2) & lo_mask
        r_hi = rng.integers(0, 1 << 63, keys.size, dtype=np.uint64) & hi_mask
        have = set(zip(want["keys"].tolist(), want["keys_hi"].tolist()))
        absent = np.array([(a, b) not in have for a, b in zip(r_lo.tolist(), r_hi.tolist())])
        assert absent.sum() > keys.size * 0.9
        q_lo, q_hi = np.concatenate([keys, r_lo[absent]]), np.concatenate([hi, r_hi[absent]])
        expect = np.concatenate([np.arange(keys.size, dtype=np.uint32), np.full(int(absent.sum()), _dbg.NO_NODE, dtype=np.uint32)])
        mix = rng.permutation(q_lo.size)
        for index in (0, 1):
            g.set_option("lookup_index", index)
            before = g.stats()
            got = g.lookup_nodes(q_lo[mix], q_hi[mix] if k > 31 else None)
            after = g.stats()
            assert np.array_equal(got, expect[mix])
            which = "lookup_index_calls" if index else "lookup_dir_calls"
            assert after[which] == before[which] + 1
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("name,k,bits", [c for c in CONSUMER_CASES if c[1] <= 31], ids=[f"{n}-k{k}" for n, k, _ in CONSUMER_CASES if k <= 31])
def test_refine_per_range_and_streaming(name, k, bits):
    """k_sk_refine / k_sk_pull per range (the extra ranges among them) and the pass over the reads: the same rank bytes for
    every node with two or more successors, the same pull-out reads.  (Error-free reads: such nodes are the repeats' only; what
    this shows is that the per-range kernels walk the chains of extra ranges and agree with the pass over the reads.)"""
    got = []
    for streaming in (0, 1):
        g = build(name, k, bucket_bits=bits, refine_streaming=streaming)
        try:
            assert g.stats()["count_extra_ranges"] > 0
            g.refine_edge_order()
            _, stamps, counts, _ = g.export_nodes()
            o = np.argsort(stamps, kind="stable")
            mc, fs = g.export_orders()
            multi = (counts[o] != 0).sum(axis=1) >= 2
            g.prune(2)
            g.remove_tips()
            g.mark_pull_reads()
            st = g.stats()
            assert st["refine_crowded"] == 0 and st["pull_crowded"] == 0
            got.append((mc[o][multi], fs[o][multi], g.export_pull_reads(), g.sizes()["n_pull_reads"]))
        finally:
            g.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert got[0][3] == got[1][3] and np.array_equal(got[0][2], got[1][2])


@gpu
@consumers
def test_traversal_over_the_extra_ranges(name, k, bits):
    """test_traversal_vs_c_oracle's comparison at threshold 2: branch list, pulled set, pull-out reads and contig index."""
    from test_traversal_vs_c_oracle import compare, device_traversal
    bases, off = INPUTS[name](k)
    o = orc_c.Oracle(bases, off, k)
    try:
        t = o.traverse(2)
        g, dev = device_traversal(bases, off, k, 2, options=(("bucket_bits", bits),))
        try:
            assert g.stats()["count_extra_ranges"] > 0
            compare(o, t, dev, k)
        finally:
            g.close()
    finally:
        o.close()


@gpu
@pytest.mark.parametrize("k", P_KS)
def test_multipass_parts_hold_the_single_builds_nodes(k):
    """build_multipass(k, 2) over input P (a build in parts chooses its geometry itself: "bucket_bits" below 9 is refused): the part
    that owns the crowded bucket starts it in parts and splits them; the parent reports its parts' events and ranges, and the
    parts together hold the oracle's nodes, counts and successors."""
    from test_hip_multipass import check_successors, dense_counts, gather_parts
    want = oracle("P", k)
    g = _dbg.Graph()
    try:
        g.set_reads(*input_p(k))
        g.build_multipass(k, 2)
        st = g.stats()
        print(f"[multipass k={k}] events {names(st['count_events'])} extra_ranges {st['count_extra_ranges']} launches {st['count_launches']}")
        assert st["count_events"] & (EV_PRESPLIT | EV_SPLIT_PART) == EV_PRESPLIT | EV_SPLIT_PART
        assert st["count_extra_ranges"] > START_PARTS_MAX
        parts = gather_parts(g)
        keys = np.concatenate([d["keys"] for d in parts])
        hi = np.concatenate([d["keys_hi"] for d in parts])
        stamps = np.concatenate([d["stamps"] for d in parts])
        counts = np.concatenate([dense_counts(d) for d in parts])
        o = np.argsort(stamps, kind="stable")
        assert np.array_equal(keys[o], want["keys"]) and np.array_equal(hi[o], want["keys_hi"])
        assert np.array_equal(stamps[o], want["stamps"]) and np.array_equal(counts[o], want["counts"])
        check_successors(parts, k)
    finally:
        g.close()
