"""The multisplit scatter of a small fan-out (up to 64 children a group: 2 048-record rounds, three workgroups to a CU) and
option "extract_grid", which names the workgroups of the pre-split extraction and with them the length of the sub-segments
level 1 starts from.  Every case is compared with the default build and with the
C oracle, in the order-independent way of test_extract_presplit.py (nodes by k-mer, successors as stamps)."""
import numpy as np
import pytest

import _dbg
import synth
from test_extract_presplit import READ_LEN, SEED, assert_equals_oracle, assert_same_graph, awkward_reads, graph_of, records_per_child

pytestmark = pytest.mark.gpu


def build(bases, offsets, k, **options):
    """The graph of one build under the options, with the handle's counters."""
    g = _dbg.Graph()
    try:
        g.set_reads(bases, offsets)
        for name, value in options.items():
            g.set_option(name, value)
        g.build(k)
        gr = graph_of(g)
        gr["stats"] = g.stats()
        return gr
    finally:
        g.close()


def reads_of(n_reads):
    reads = synth.reads_ascii(SEED, 10 * n_reads, n_reads, READ_LEN, 0.01)
    bases = np.ascontiguousarray(reads.reshape(-1))
    bases.setflags(write=False)
    return bases, np.arange(0, bases.size + 1, READ_LEN, dtype=np.uint64)


@pytest.fixture(scope="module")
def synth_set():
    """20 000 reads x 100 bp of a 200 kbp genome, 1 % errors: 2 MB, 245 extraction tiles (test_extract_presplit.py's set)."""
    return reads_of(20_000)


@pytest.fixture(scope="module")
def large_set():
    """60 000 reads x 100 bp: 6 MB, 733 tiles, some 200 k records a group at f0 = 1."""
    return reads_of(60_000)


_checked = {}


def default_graph(data, k):
    """The default build of the set, checked against the C oracle once per (set, k)."""
    key = (data[0].size, k)
    if key not in _checked:
        gr = build(*data, k)
        assert_equals_oracle(gr, *data, k)
        _checked[key] = gr
    return _checked[key]


def check(data, k, **options):
    got = build(*data, k, **options)
    assert_same_graph(got, default_graph(data, k))
    assert_equals_oracle(got, *data, k)
    assert got["stats"]["extract_presplit_fallbacks"] == 0
    return got


@pytest.mark.parametrize("stamp64", [0, 1])
@pytest.mark.parametrize("f0,grid", [(1, 8), (4, 2), (4, 1)])
def test_sub_segments_of_several_rounds(synth_set, f0, grid, stamp64):
    """(1, 8): sub-segments of about 10 k records (level 1 splits 256 ways there: the wide scatter on long sub-segments);
    (4, 2): about 5 k, three rounds of the small scatter; (4, 1): about 10 k, five full rounds of 2 048 and a partial one."""
    st = check(synth_set, 31, extract_presplit=f0, extract_grid=grid, stamp64=stamp64)["stats"]
    if f0 == 4:  # (a second level, if the estimate asks for one, splits two or three ways: small as well)
        assert st["ms_scatter_small"] >= 1 and st["ms_scatter_wide"] == 0
    else:
        assert st["ms_scatter_wide"] >= 1


def test_one_tile_per_workgroup(synth_set):
    """245 workgroups of one tile: every sub-segment is far below one round."""
    check(synth_set, 31, extract_presplit=4, extract_grid=245)


def test_one_record_per_position(synth_set):
    """k = 13: W = 1, every k-mer is a record, so a sub-segment spans several rounds."""
    check(synth_set, 13, extract_presplit=4, extract_grid=8)


def test_grid_set_by_the_sub_segment_limit(synth_set):
    """k = 13 with f0 = 1: a tile may need 8 192 x 1.5 / 2 = 6 144 records of a sub-segment, so a workgroup takes at most 5
    of the 245 tiles -- 49 workgroups, which the extraction rounds up to whole multiples of the named grid of 8 (56)."""
    check(synth_set, 13, extract_presplit=1, extract_grid=8)


def test_fan_out_64_takes_the_small_scatter(synth_set):
    """20 bucket bits: level 1 takes 10 of them, 6 behind f0 = 4 -- the largest fan-out of the small scatter; level 2 is wide."""
    st = check(synth_set, 31, bucket_bits=20, extract_presplit=4)["stats"]
    assert (st["ms_scatter_small"], st["ms_scatter_wide"]) == (1, 1)


def test_fan_out_128_takes_the_wide_scatter(synth_set):
    st = check(synth_set, 31, bucket_bits=20, extract_presplit=3)["stats"]
    assert (st["ms_scatter_small"], st["ms_scatter_wide"]) == (0, 2)


@pytest.mark.parametrize("grid", [0, 1])
def test_groups_of_many_super_chunks(large_set, grid):
    """f0 = 1 on 6 MB: a group holds several super-chunks' worth of records; with extract_grid 1 the sub-segment limit
    sets the grid, and the sub-segments are as long as the extraction makes them."""
    got = check(large_set, 31, extract_presplit=1, extract_grid=grid)
    assert got["n_records"] > 2 * 2 * 32768


@pytest.mark.parametrize("k", [13, 31])
def test_awkward_reads(k):
    """Reads of k, k - 1 and k + 1 bases and one longer than a tile: empty sub-segments, groups below one round."""
    data = awkward_reads(k)
    for f0 in (1, 4, 6):
        for grid in (1, 3):
            check(data, k, extract_presplit=f0, extract_grid=grid)


def test_total_bytes_a_multiple_of_the_tile():
    rng = np.random.default_rng(12)
    bases = np.frombuffer(bytes(b"ACGT"[c] for c in rng.integers(0, 4, 16384)), dtype=np.uint8).copy()
    data = (bases, np.array([0, 8192, 16384], dtype=np.uint64))
    for f0 in (1, 4, 6):
        for grid in (1, 3):
            check(data, 31, extract_presplit=f0, extract_grid=grid)


def test_fallback_with_a_named_grid():
    """test_extract_presplit.py's low-complexity input: one child outgrows its sub-segment, once, under extract_grid 4 too."""
    k = 31
    rng = np.random.default_rng(13)
    one = bytes(b"ACGT"[c] for c in rng.integers(0, 4, READ_LEN))
    poly_a = b"A" * READ_LEN
    per_child = 20_000 * records_per_child(one, k, 4) + 2_000 * records_per_child(poly_a, k, 4)
    assert per_child.max() > 1.5 / 16 * per_child.sum(), per_child
    bases = np.frombuffer(one * 20_000 + poly_a * 2_000, dtype=np.uint8).copy()
    offsets = np.arange(0, bases.size + 1, READ_LEN, dtype=np.uint64)
    got = build(bases, offsets, k, extract_presplit=4, extract_grid=4)
    assert got["stats"]["extract_presplit_fallbacks"] == 1
    assert_same_graph(got, build(bases, offsets, k))
    assert_equals_oracle(got, bases, offsets, k)


@pytest.mark.parametrize("value", [-1, 65536])
def test_option_range(value):
    g = _dbg.Graph()
    try:
        with pytest.raises(_dbg.DbgError) as e:
            g.set_option("extract_grid", value)
        assert e.value.code == _dbg.DBG_E_ARG
        g.set_option("extract_grid", 65535)
        g.set_option("extract_grid", 0)
    finally:
        g.close()
