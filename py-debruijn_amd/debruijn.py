"""Drop-in for the reference's ``debruijn.py`` backed by the gfx950 HIP library.

Same module surface as the reference (``read_reads``, ``construct_graph``,
``output_contigs``, ``Node``; used by II_assembleFromReads.py:11-12,58,61,63), same
argument meaning, return shapes and stdout lines; the work happens on the MI355X
through the C ABI of ``include/dbg.h`` (binding: ``_dbg.py``).  There is no CPU
path: without the built library and a GPU every call raises.

Differences a caller can observe, all documented in DESIGN.md:
  * limits: 1 <= k <= 63 (reads of upper-case A/C/G/T only: two 64-bit words per k-mer above 31; any other
    alphabet -- peptides, lower case, N, ... --: at most 32 distinct single-byte characters, packed at
    5 bits up to k = 11 and keyed by reference into the reads above); ValueError otherwise, never a
    silent drop or split;
  * ``output_contigs`` needs the objects returned by this module's ``construct_graph``;
  * graphs of ``LAZY_MIN_NODES`` (2e6, env ``DBG_LAZY_MIN_NODES``) or more nodes come back as read-only
    ``Mapping`` views over the exported arrays (label lookup, ``len``, ordered iteration; equal to the
    reference's dicts when materialised) instead of Python dicts.  A lookup of one label (``in``, ``[]``) is
    answered on the device (dbg_lookup_nodes + dbg_gather_nodes) and exports nothing; iteration, ``len`` of
    ``edges`` / ``edge_count_table`` and ``items()`` export the arrays, after which lookups are served from them.
Everything else -- values AND orders (dict insertion order, ``Counter.most_common`` tie order,
the append order of ``already_pull_out``, contig order) -- equals the reference.
"""
from __future__ import annotations

import bisect
import os
import re
from collections.abc import ItemsView, Mapping, Sequence

import numpy as np

import _dbg

__all__ = ["Node", "read_reads", "read_fastq", "read_fasta_records", "wrap_fasta_record", "read_reads_device", "DeviceReads", "construct_graph", "output_contigs",
           "get_score_device", "score_sequences", "count_spectrum", "get_kmers", "get_graph_from_kmers"]



class Node:
    """debruijn.py:8-14."""

    __slots__ = ("label", "indegree", "outdegree")

    def __init__(self, lab, indegree=0, outdegree=0):
        self.label = lab
        self.indegree = indegree
        self.outdegree = outdegree


def read_reads(fname):
    """debruijn.py:22-32: every line that does not start with '>' is one read (rstrip'ed).

    Linear time (the reference's ``reads = reads + [...]`` is quadratic); same result.
    """
    with open(fname, "r") as fh:
        return [line.rstrip() for line in fh.readlines() if line[0] != ">"]


_FQ_SPACE = bytes([32, *range(9, 14), *range(28, 32)])  # str.isspace() over ASCII, as the FASTA path strips it
FASTQ_KINDS = ("header", "sequence start", "separator", "length mismatch", "truncated record", "quality byte")


class FastqError(ValueError):
    """A malformed FASTQ file: ``record`` (0-based) and ``kind`` (one of ``FASTQ_KINDS``)."""

    def __init__(self, record, kind):
        super().__init__(f"malformed FASTQ: record {record}: {kind}")
        self.record, self.kind = record, kind


def parse_fastq(data, min_quality=0):
    """The FASTQ rules of ``dbg_set_reads_fastq_file`` (include/dbg.h) over the bytes of a file, in plain Python ->
    list of bytes reads.  Strict four-line records over universal-newline lines; trailing white space of the file is
    ignored; only the last record may lack its quality line, and only if its read is empty.  A record is checked in the
    order header, sequence start, separator, length; quality bytes (``min_quality`` > 0) after all of that."""
    if not 0 <= int(min_quality) <= 93:
        raise ValueError(f"min_quality must be 0..93, not {min_quality!r}")
    lines = bytes(data).rstrip(_FQ_SPACE).splitlines()  # bytes.splitlines: \n, \r and \r\n only
    reads, quals = [], []
    for r in range(0, -(-len(lines) // 4)):
        grp = lines[4 * r:4 * r + 4]
        if grp[0][:1] != b"@":
            raise FastqError(r, "header")
        if len(grp) < 2:
            raise FastqError(r, "truncated record")
        if grp[1][:1] in (b"@", b"+"):
            raise FastqError(r, "sequence start")
        if len(grp) < 3:
            raise FastqError(r, "truncated record")
        if grp[2][:1] != b"+":
            raise FastqError(r, "separator")
        seq = grp[1].rstrip(_FQ_SPACE)
        qual = grp[3].rstrip(_FQ_SPACE) if len(grp) == 4 else b""
        if len(qual) != len(seq):
            raise FastqError(r, "length mismatch")
        reads.append(seq)
        quals.append(qual)
    if min_quality:
        for r, qual in enumerate(quals):
            if any(c < 33 or c > 126 for c in qual):
                raise FastqError(r, "quality byte")
        reads = [bytes(78 if q - 33 < min_quality else c for c, q in zip(seq, qual)) for seq, qual in zip(reads, quals)]
    return reads


def read_fastq(fname, min_quality=0):
    """The reads of a FASTQ file as ``read_reads`` gives those of a FASTA file: a list of str, one per record, on the
    host (no GPU needed).  ``min_quality`` q > 0 (Phred+33): base j becomes ``N`` where ``qual[j] - 33 < q``.
    ``FastqError`` (a ValueError) names record and kind of a malformed file; see ``parse_fastq`` for the rules."""
    with open(fname, "rb") as fh:
        return [r.decode("latin-1") for r in parse_fastq(fh.read(), min_quality)]


class FastaError(ValueError):
    """A malformed FASTA file in record mode: ``kind``, the 0-based ``line`` and the byte position ``pos`` of the first
    offending byte."""

    def __init__(self, kind, line, pos=None):
        super().__init__(f"malformed FASTA: {kind}: line {line}" + ("" if pos is None else f", byte {pos}"))
        self.kind, self.line, self.pos = kind, line, pos


def parse_fasta_records(data):
    """The record rules of ``dbg_set_reads_fasta_records`` (include/dbg.h) over the bytes of a file, in plain Python ->
    list of bytes reads, one per header.  Lines are universal-newline lines; a header is a line whose first byte is ``>``;
    read i is the sequence lines between header i and the next header (or the end of the file) joined, each rstrip'ed on
    its own, so a blank line adds nothing and a header followed at once by a header gives an empty read.  Lines in front
    of the first header must be blank after rstrip: anything else raises ``FastaError``."""
    reads, cur, pos = [], None, 0
    for ln, line in enumerate(bytes(data).splitlines(keepends=True)):  # bytes.splitlines: \n, \r and \r\n only
        if line[:1] == b">":
            cur = []
            reads.append(cur)
        else:
            body = line.rstrip(_FQ_SPACE)
            if cur is not None:
                cur.append(body)
            elif body:
                raise FastaError("sequence before the first header", ln, pos + len(line) - len(line.lstrip(_FQ_SPACE)))
        pos += len(line)
    return [b"".join(r) for r in reads]


def read_fasta_records(fname):
    """The reads of a FASTA file with one read per RECORD, as ``read_reads`` gives one per line: a list of str on the host
    (no GPU needed).  This is what a line-wrapped file means; see ``parse_fasta_records`` for the rules."""
    with open(fname, "rb") as fh:
        return [r.decode("latin-1") for r in parse_fasta_records(fh.read())]


def wrap_fasta_record(text, line_width):
    """The body of a FASTA record as ``write_contigs_fasta(line_width=)`` writes it: ``text`` in lines of ``line_width``
    characters, each ended by a newline, the last possibly shorter.  An empty text is one newline, a text of a whole
    number of lines gets no empty line, and ``line_width`` 0 puts the text on one line.  str in, str out; bytes likewise."""
    nl = "\n" if isinstance(text, str) else b"\n"
    if line_width <= 0 or not len(text):
        return text + nl
    return type(nl)().join(text[i:i + line_width] + nl for i in range(0, len(text), line_width))


# Files of at least this many bytes stream to the device in chunks (dbg_set_reads_fasta_file) instead of going over in one
# image (dbg_set_reads_fasta, which holds ~2.5x the file on the device at its peak).  The reads are the same either way.
STREAM_MIN_BYTES = int(os.environ.get("DBG_STREAM_MIN_BYTES", str(1 << 30)))


class DeviceReads:
    """``read_reads`` on the GPU: a read-only sequence of the reads of a FASTA file.

    The file is parsed on the device (``dbg_set_reads_fasta``: newline scan, header lines dropped,
    ``rstrip``) and stays there; ``construct_graph`` accepts the object in place of the list and
    builds from the resident reads, so no Python string is created per read.  Items are
    materialised lazily (one device-to-host copy of the packed buffer on first access).
    The object owns one device handle: a later ``construct_graph`` on the same object replaces the
    graph of an earlier one (``output_contigs`` on the earlier result then raises instead of walking the new graph).

    byte_range=(begin, end): only the lines whose first byte lies in [begin, end) (end None: to the end of the file);
    a line that starts in the range is read to its end.  The reads of [0, b) followed by those of [b, size) are the
    reads of the whole file for every b.  chunk_bytes: size of the staging chunks of the streamed ingest (0: library
    default).  Either argument, or a file of ``STREAM_MIN_BYTES`` or more, takes the streamed ingest
    (``dbg_set_reads_fasta_file``); smaller files go over in one image.

    non_acgt="keep" (default): every byte of a read is a character, as in the reference.  "split": after the ingest the
    reads are cut at every byte that is not A/C/G/T (``acgt_pieces``; ``fold_case``: a c g t are folded to upper case
    first) and the object lists the pieces; ``split_stats`` holds what the pass did, ``origins()`` where each piece came from.

    format="fastq": the file is strict four-line FASTQ (``read_fastq`` states the rules) and always takes the streamed
    call (``dbg_set_reads_fastq_file``); read i is the sequence of record i and a byte range owns the records whose header
    starts in it.  ``min_quality`` q > 0 turns every base below Phred q into ``N``: kept as a character by default, a cut
    point with non_acgt="split".  Nothing is detected: the default "fasta" reads a FASTQ file line by line, as it always did.

    strands="forward" (default): the reads as they are.  "both": after the ingest (and its quality mask) and after the split,
    every read is followed by its reverse complement (``both_strands``; ``Graph.add_revcomp``): the object lists
    r0, rc(r0), r1, rc(r1), ... and ``revcomp_stats`` holds what the pass did.  Cutting before complementing gives the same
    pieces as the other order.

    records="line" (default): every line that is no header is a read, as in the reference.  "record": read i is record i,
    the sequence lines between header i and the next header joined (``read_fasta_records`` states the rules) -- what a
    line-wrapped file means.  A byte range then owns the records whose header starts in it, ``records_stats`` holds what
    the ingest did, and ``origins()`` speaks of records and of positions in the joined read.  FASTA only.
    """

    def __init__(self, fname, byte_range=None, chunk_bytes=None, non_acgt="keep", fold_case=False, format="fasta",
                 min_quality=0, strands="forward", records="line"):
        if non_acgt not in ("keep", "split"):
            raise ValueError(f"non_acgt must be 'keep' or 'split', not {non_acgt!r}")
        if strands not in ("forward", "both"):
            raise ValueError(f"strands must be 'forward' or 'both', not {strands!r}")
        if format not in ("fasta", "fastq"):
            raise ValueError(f"format must be 'fasta' or 'fastq', not {format!r}")
        if min_quality and format != "fastq":
            raise ValueError("min_quality needs format='fastq'")
        if records not in ("line", "record"):
            raise ValueError(f"records must be 'line' or 'record', not {records!r}")
        if records == "record" and format == "fastq":
            raise ValueError("records='record' needs format='fasta': a FASTQ read is a record already")
        self._graph = _dbg.Graph()
        self.records_stats = None
        one_image = byte_range is None and chunk_bytes is None and os.path.getsize(fname) < STREAM_MIN_BYTES
        if records == "record":
            if one_image:
                self._graph.set_reads_fasta_records(fname)
            else:
                begin, end = (0, None) if byte_range is None else byte_range
                self._graph.set_reads_fasta_records_file(fname, begin, end, chunk_bytes or 0)
            self.records_stats = self._graph.fasta_records_stats()
        elif format == "fastq":
            begin, end = (0, None) if byte_range is None else byte_range
            self._graph.set_reads_fastq_file(fname, begin, end, chunk_bytes or 0, min_quality)
        elif one_image:
            self._graph.set_reads_fasta(fname)
        else:
            begin, end = (0, None) if byte_range is None else byte_range
            self._graph.set_reads_fasta_file(fname, begin, end, chunk_bytes or 0)
        self.split_stats = self._graph.split_reads(fold_case=fold_case) if non_acgt == "split" else None
        self.revcomp_stats = self._graph.add_revcomp() if strands == "both" else None
        self._n = self._graph.sizes()["n_reads"]
        self._host = None

    def origins(self):
        """non_acgt="split": (read_index, pos) uint64 arrays -- the read of the file (the line, headers not counted, or
        with records="record" the record and the position in its joined read; within the byte range) every piece came from and the position of its first byte in it.
        strands="both": entry j is strand ``j & 1`` of piece ``j >> 1``, pos in forward orientation."""
        if self.split_stats is None:
            raise ValueError("origins() needs non_acgt='split'")
        return self._graph.read_origins()

    def _pull(self):
        if self._host is None:
            bases, offsets = self._graph.copy_reads()
            self._host = (bases.tobytes().decode("latin-1"), offsets)  # one byte, one character, as everywhere else
        return self._host

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        text, off = self._pull()
        return text[int(off[i]):int(off[i + 1])]

    def __iter__(self):
        text, off = self._pull()
        for i in range(self._n):
            yield text[int(off[i]):int(off[i + 1])]

    def take(self, indices):
        """``[self[i] for i in indices]`` without bringing every read to the host: the selected reads are gathered on
        the device (pull_out_read of construct_graph is 3 % of the reads at the BASELINE size)."""
        idx = np.asarray(indices, dtype=np.int64)
        idx = np.where(idx < 0, idx + self._n, idx)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self._n):
            raise IndexError("read index out of range")
        if self._host is not None or idx.size == 0 or idx.size > self._n // 4:
            return [self[int(i)] for i in idx]
        chars, off = self._graph.take_reads(idx)  # dbg_take_reads: gathered on the device, one copy of the selection
        text = chars.tobytes().decode("latin-1")
        return [text[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def read_reads_device(fname, byte_range=None, chunk_bytes=None, non_acgt="keep", fold_case=False, format="fasta",
                      min_quality=0, strands="forward", records="line"):
    """``read_reads`` (debruijn.py:22-32) without leaving the GPU; see DeviceReads (byte ranges, streamed ingest, the
    split at bytes that are not bases, FASTQ files and their quality mask, both strands, one read per record)."""
    return DeviceReads(fname, byte_range, chunk_bytes, non_acgt, fold_case, format, min_quality, strands, records)


_ACGT_RUNS = re.compile(b"[ACGT]+")
_FOLD_ACGT = bytes.maketrans(b"acgt", b"ACGT")


def acgt_pieces(reads, fold_case=False):
    """What ``split_reads`` / ``non_acgt="split"`` computes, in plain Python: the maximal runs of A/C/G/T of every read,
    in order (``fold_case``: a c g t count as A C G T and come out folded).  Every other byte is a cut, a read without
    a base gives nothing, two reads never merge.  str reads (one byte per character, latin-1) give str pieces."""
    out = []
    for r in reads:
        text = isinstance(r, str)
        b = r.encode("latin-1") if text else bytes(r)
        if fold_case:
            b = b.translate(_FOLD_ACGT)
        out.extend(m.decode("latin-1") if text else m for m in _ACGT_RUNS.findall(b))
    return out


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(read):
    """The reverse complement of one read: the read backwards with A<->T, C<->G, a<->t, c<->g swapped and every other
    byte (``N``, bytes >= 0x80, ...) as it is.  str in (one byte per character, latin-1), str out; bytes in, bytes out."""
    if isinstance(read, str):
        return read.encode("latin-1").translate(_COMP)[::-1].decode("latin-1")
    return bytes(read).translate(_COMP)[::-1]


def both_strands(reads):
    """What ``add_revcomp`` / ``strands="both"`` computes, in plain Python: ``[r0, revcomp(r0), r1, revcomp(r1), ...]``.
    The graph of both strands is the reference run on this list; read j is strand ``j & 1`` of read ``j >> 1``."""
    out = []
    for r in reads:
        out.append(r if isinstance(r, str) else bytes(r))
        out.append(revcomp(r))
    return out


class _Vertices(dict):
    """``vertices`` dict that also carries the device handle for output_contigs."""
    _graph = None
    _state = None


# Above this many nodes construct_graph returns read-only Mapping views over the exported arrays instead of
# Python dicts (dicts are infeasible at 10^8 nodes); equal to the dicts when materialised.
LAZY_MIN_NODES = int(os.environ.get("DBG_LAZY_MIN_NODES", "2000000"))


_STALE_VIEWS = ("these views belong to a graph that a later build on the same reads replaced: read them "
                "(or dict() them) before the next construct_graph")
_HOST = object()  # _NodeStore.device_row: this lookup is the host arrays' to answer


class _NodeStore:
    """Host arrays of one graph (in the library's table order) + the dict-order permutation + label <-> index
    conversion.  Indices of this class's methods are positions in dict (first-occurrence) order; ``order[i]`` is the
    row of node i in the arrays, so nothing of size n_nodes is gathered or sorted on the host up front.

    While the arrays have not been loaded, one label is looked up on the device instead (``device_row``): the graph
    handle finds the node and hands back its row, and nothing of size n_nodes moves."""

    def __init__(self, k, alphabet, bits, n, loader, graph=None):
        self._graph = graph
        self._generation = None if graph is None else graph.generation
        self.k, self.alphabet, self.bits = k, alphabet, bits
        self.chars = alphabet.decode("latin-1")
        self.code_of = {ch: i for i, ch in enumerate(self.chars)}  # alphabet[code] = character
        self.n = int(n)
        # The arrays leave the device when something first asks for them: the reference's driver
        # (II_assembleFromReads.py:56-75) never reads vertices / edges / edge_count_table, and their export is most of
        # construct_graph's time at scale (37 bytes per node + the dict-order sort).
        self._loader = loader
        self._arrays = None
        self._sorted = None
        self._inverse = None

    def _get(self, name):
        if self._arrays is None:
            self._arrays = self._loader()
            self._loader = None
        return self._arrays[name]

    order = property(lambda self: self._get("order"))
    keys = property(lambda self: self._get("keys"))
    keys_hi = property(lambda self: self._get("keys_hi"))
    counts = property(lambda self: self._get("counts"))
    rank_mc = property(lambda self: self._get("rank_mc"))
    rank_fs = property(lambda self: self._get("rank_fs"))
    flags = property(lambda self: self._get("flags"))
    keep = property(lambda self: self._get("keep"))

    def device_row(self, lab, what):
        """The row of node ``lab`` (dict of the columns ``what``, one node each) from the device; None if ``lab`` is no
        node; _HOST if the host arrays answer: they are loaded already, or the library does not look up this kind of
        graph.  RuntimeError if a later build replaced the graph these views were made for."""
        g = self._graph
        if self._arrays is not None or g is None:
            return _HOST
        if g.generation != self._generation:
            raise RuntimeError(_STALE_VIEWS)
        e = self.encode(lab)
        if e is None:
            return None
        try:
            row = int(g.lookup_nodes(np.array([e[1]], dtype=np.uint64), np.array([e[0]], dtype=np.uint64))[0])
            if row == _dbg.NO_NODE:
                return None
            return g.gather_nodes([row], what) if what else {}
        except _dbg.DbgError as err:
            if err.code != _dbg.DBG_E_ARG:
                raise
            self._graph = None  # refused (a graph the query calls do not cover): the host path from now on
            return _HOST

    def rows(self, idx):
        return self.order[np.asarray(idx, dtype=np.int64)]

    def row_labels(self, rows):
        hi = None if self.keys_hi is None else self.keys_hi[rows]
        return _dbg.decode_keys(self.keys[rows], self.k, self.alphabet, self.bits, hi)

    def labels(self, idx):
        return self.row_labels(self.rows(idx))

    def indeg(self, i):
        return int(self.flags[self.order[i]] & _dbg.F_INDEG)

    def outdeg(self, i):
        return int(np.count_nonzero(self.counts[self.order[i]]))

    def pulled(self, i):
        return bool(self.flags[self.order[i]] & _dbg.F_PULLED)

    def alive(self):
        """Dict-order indices of the nodes that were not pulled out."""
        return np.nonzero((self.flags & _dbg.F_PULLED)[self.order] == 0)[0]

    def encode(self, lab):
        """(hi, lo) words of a k-character label, or None if it is not a k-mer over the alphabet."""
        if not isinstance(lab, str) or len(lab) != self.k:
            return None
        v = 0
        for ch in lab:
            c = self.code_of.get(ch)
            if c is None:
                return None
            v = (v << self.bits) | c
        return v >> 64, v & 0xFFFFFFFFFFFFFFFF

    def find(self, lab):
        """Index (dict order) of a label, or -1."""
        e = self.encode(lab)
        if e is None:
            return -1
        if self._sorted is None:  # one sort, on the first lookup
            if self.keys_hi is None:
                perm = np.argsort(self.keys, kind="stable")
            else:
                perm = np.lexsort((self.keys, self.keys_hi))
            self._sorted = (perm, self.keys[perm], None if self.keys_hi is None else self.keys_hi[perm])
            self._inverse = np.empty(self.n, dtype=np.int64)
            self._inverse[self.order] = np.arange(self.n, dtype=np.int64)
        perm, lo_s, hi_s = self._sorted
        hi, lo = e
        if hi_s is None:
            if hi:
                return -1
            a = int(np.searchsorted(lo_s, np.uint64(lo), side="left"))
            return int(self._inverse[perm[a]]) if a < self.n and int(lo_s[a]) == lo else -1
        a = int(np.searchsorted(hi_s, np.uint64(hi), side="left"))
        b = int(np.searchsorted(hi_s, np.uint64(hi), side="right"))
        c = a + int(np.searchsorted(lo_s[a:b], np.uint64(lo), side="left"))
        return int(self._inverse[perm[c]]) if c < b and int(lo_s[c]) == lo else -1

    def successors(self, i, pruned):
        """Successor labels of node i: Counter.most_common order; only the kept ones when `pruned`."""
        r = self.order[i]
        return self.ranked_successors(self.row_labels([r])[0], self.counts[r], self.rank_mc[r], int(self.keep[r]), pruned)

    def ranked_successors(self, lab, c, rank_mc, kp, pruned):
        """Successor labels of the node ``lab`` from its row: counts, most_common ranks and keep mask."""
        nd = int(np.count_nonzero(c))
        ranked = [int(code) for code in np.atleast_1d(rank_mc) if code != 0xFF and c[code]][:nd]
        return [lab[1:] + self.chars[code] for code in ranked if not pruned or (kp >> code) & 1]

    def edge_names(self, i):
        r = self.order[i]
        lab = self.row_labels([r])[0]
        c = self.counts[r]
        return [(lab + self.chars[code], int(c[code])) for code in np.atleast_1d(self.rank_fs[r]) if code != 0xFF and c[code]]

    def edge_count(self, i, code):
        return int(self.counts[self.order[i], code]) if code < self.counts.shape[1] else 0


class _LazyVertices(Mapping):
    """``vertices``: label -> Node, dict order; nothing is materialised until it is asked for."""

    def __init__(self, store):
        self._s = store
        self._graph = None
        self._state = None

    def __len__(self):
        return self._s.n

    def __iter__(self):
        for lo in range(0, self._s.n, 1 << 16):
            yield from self._s.labels(np.arange(lo, min(lo + (1 << 16), self._s.n)))

    def __contains__(self, lab):
        r = self._s.device_row(lab, ())
        if r is not _HOST:
            return r is not None
        return self._s.find(lab) >= 0

    def __getitem__(self, lab):
        r = self._s.device_row(lab, ("flags", "counts"))
        if r is not _HOST:
            if r is None:
                raise KeyError(lab)
            return Node(lab, int(r["flags"][0] & _dbg.F_INDEG), int(np.count_nonzero(r["counts"][0])))
        i = self._s.find(lab)
        if i < 0:
            raise KeyError(lab)
        return Node(lab, self._s.indeg(i), self._s.outdeg(i))


class _LazyEdges(Mapping):
    """``edges``: label -> surviving successor labels, for every node that was not pulled out."""

    def __init__(self, store):
        self._s = store
        self._alive_idx = None

    @property
    def _alive(self):
        if self._alive_idx is None:
            self._alive_idx = self._s.alive()
        return self._alive_idx

    def __len__(self):
        return int(self._alive.size)

    def __iter__(self):
        for lo in range(0, self._alive.size, 1 << 16):
            yield from self._s.labels(self._alive[lo:lo + (1 << 16)])

    def __contains__(self, lab):
        r = self._s.device_row(lab, ("flags",))
        if r is not _HOST:
            return r is not None and not (r["flags"][0] & _dbg.F_PULLED)
        i = self._s.find(lab)
        return i >= 0 and not self._s.pulled(i)

    def __getitem__(self, lab):
        r = self._s.device_row(lab, ("flags", "counts", "order", "keepmask"))
        if r is not _HOST:
            if r is None or r["flags"][0] & _dbg.F_PULLED:
                raise KeyError(lab)
            return self._s.ranked_successors(lab, r["counts"][0], r["order"][0], int(r["keepmask"][0]), True)
        i = self._s.find(lab)
        if i < 0 or self._s.pulled(i):
            raise KeyError(lab)
        return self._s.successors(i, True)


class _LazyEdgeCounts(Mapping):
    """``edge_count_table``: (k+1)-mer -> multiplicity, in the reference's insertion order."""

    def __init__(self, store):
        self._s = store
        self._n = None

    def __len__(self):
        if self._n is None:
            self._n = int(np.count_nonzero(self._s.counts))
        return self._n

    def __iter__(self):
        for i in range(self._s.n):
            for name, _ in self._s.edge_names(i):
                yield name

    def items(self):
        return _EdgeItems(self)

    def __contains__(self, name):
        try:
            self[name]
            return True
        except KeyError:
            return False

    def __getitem__(self, name):
        if not isinstance(name, str) or len(name) != self._s.k + 1:
            raise KeyError(name)
        code = self._s.code_of.get(name[-1])
        r = self._s.device_row(name[:-1], ("counts",)) if code is not None else None
        if r is not _HOST:
            n = int(r["counts"][0][code]) if r is not None and code < r["counts"].shape[1] else 0
            if not n:
                raise KeyError(name)
            return n
        i = self._s.find(name[:-1])
        n = self._s.edge_count(i, code) if i >= 0 and code is not None else 0
        if not n:
            raise KeyError(name)
        return n


class _EdgeItems(ItemsView):
    def __iter__(self):
        s = self._mapping._s
        for i in range(s.n):
            yield from s.edge_names(i)


class _Tracked(list):
    """list that remembers which construct_graph call produced it."""
    _token = None


class ContigList(list):
    """list[str] of contigs plus the device-computed getScore of each (``.scores``).

    ``sorted_fasta()`` returns the text the reference's driver writes for this list -- contigs sorted by score,
    descending and stable, as ``>SEQUENCE_{i}_{k}mer`` records (II_assembleFromReads.py:64-69) -- sorted and formatted
    on the device (dbg_export_sorted_fasta); valid until the graph handle builds or walks again."""
    scores = None
    _graph = None
    _generation = None
    _walk = None
    _index = None  # contig of the walk behind every position of the list

    def sorted_fasta(self):
        if self._graph is None or self._generation != self._graph.generation or self._walk != self._graph.walks:
            raise ValueError("the device contigs of this list are gone (the handle built another graph or walked again)")
        return self._graph.export_sorted_fasta()[0].decode("latin-1")

    def write_fasta(self, path, k, order=None, append=True, line_width=0):
        """``>SEQUENCE_{i}_{k}mer`` records of the positions ``order`` of this list (None: as it stands), formatted on the
        device and streamed to ``path`` (``Graph.write_contigs_fasta``); ``line_width`` W > 0 wraps every contig at W
        characters.  Valid until the graph handle builds or walks again, like ``sorted_fasta``."""
        if self._graph is None or self._generation != self._graph.generation or self._walk != self._graph.walks:
            raise ValueError("the device contigs of this list are gone (the handle built another graph or walked again)")
        pos = np.arange(len(self)) if order is None else np.asarray(order, dtype=np.int64)
        return self._graph.write_contigs_fasta(path, np.asarray(self._index, dtype=np.uint64)[pos], append=append, k_label=k,
                                               line_width=line_width)


MAX_CONTIG_CHARS = 0  # dbg_walk's max_chars; 0 = the library default (1 GiB of contig text kept on the device)


BATCH_CHARS = 256 << 20  # characters of one batched text export (dbg_export_contig_texts): bounds the host copy


def _batches(lengths, limit):
    """Slices of consecutive positions whose lengths add up to ``limit`` at most (a longer contig is a batch of its own)."""
    ends = np.cumsum(np.asarray(lengths, dtype=np.int64))
    at, n = 0, len(ends)
    while at < n:
        base = int(ends[at - 1]) if at else 0
        stop = max(int(np.searchsorted(ends, base + limit, side="right")), at + 1)
        yield slice(at, stop)
        at = stop


def _packed_texts(graph, idx, lengths):
    """(uint8 characters, lengths) of the contigs ``idx`` of ``graph``, batch by batch: one device call per batch where the
    handle offers export_contig_texts, one per contig where it does not."""
    idx, lengths = np.asarray(idx, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    many = getattr(graph, "export_contig_texts", None)
    for sl in _batches(lengths, BATCH_CHARS):
        if many is not None:
            off, chars = many(idx[sl])
            if not np.array_equal(np.diff(off.astype(np.int64)), lengths[sl]):
                raise RuntimeError("the device contigs of this list are gone (the handle walked again)")
        else:
            chars = np.frombuffer(b"".join(graph.export_contig_text(int(c), int(n)) for c, n in zip(idx[sl], lengths[sl])),
                                  dtype=np.uint8)
        yield chars, lengths[sl]


def _texts(graph, idx, lengths):
    """The same as strings."""
    for chars, lens in _packed_texts(graph, idx, lengths):
        text, at = chars.tobytes().decode("latin-1"), 0
        for n in lens.tolist():
            yield text[at:at + n]
            at += n


class _ContigBlock(Sequence):
    """Contigs of one walk by reference: the graph handle, contig indices into its index and their lengths.  A text is
    fetched from that graph when it is indexed (dbg_export_contig_text); slices and iteration fetch in batches
    (dbg_export_contig_texts); ``len`` and ``take`` move none."""

    def __init__(self, graph, idx, lengths, final, generation, walk):
        self._graph = graph
        self._idx = np.asarray(idx, dtype=np.int64)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self._final, self._generation, self._walk = final, generation, walk

    def __len__(self):
        return len(self._idx)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return list(_texts(self._graph, self._idx[i], self.lengths[i]))
        return self._graph.export_contig_text(int(self._idx[i]), int(self.lengths[i])).decode("latin-1")

    def __iter__(self):
        return _texts(self._graph, self._idx, self.lengths)

    def take(self, positions):
        p = np.asarray(positions, dtype=np.int64)
        return _ContigBlock(self._graph, self._idx[p], self.lengths[p], self._final, self._generation, self._walk)

    def current(self):
        """The graph still holds the non-final walk these indices point into."""
        g = self._graph
        return self._final is False and g.generation == self._generation and g.walks == self._walk


class LazyContigs(Sequence):
    """Contigs of a walk whose text was larger than MAX_CONTIG_CHARS: same order, ``.scores`` and ``.lengths`` as
    ContigList, every text fetched from the device when it is indexed (dbg_export_contig_text).

    ``sort`` and ``extend`` exist so that the reference's own driver (II_assembleFromReads.py:64,74:
    ``sequences.sort(key=lambda x: getScore(edge_count_table, x, k), reverse=True)`` and
    ``sequences.extend(pull_out_read)``) runs unchanged on this object.  Both only permute / append: no text moves.
    ``sort`` orders by the device-computed getScore of every contig -- the one key the pipeline sorts by; evaluating an
    arbitrary ``key`` would mean fetching every text (10^12 characters at the BASELINE size).  A ``key`` that is not
    that score is detected on a sample of the shortest contigs and refused.  ``extend`` with the pull_out_read of a graph
    built from walks (_PulledReads) appends its pulled contigs as blocks of references into the graphs that hold them."""

    _final = None       # set by output_contigs: the walk's mode and the handle state it read (construct_graph at k + 1
    _generation = None  # builds from the chains of a current non-final walk, dbg_build_from_walk)
    _walk = None

    def __init__(self, graph, order, off, score):
        self._graph = graph
        self._order = np.asarray(order)
        self._off = off
        self._score = np.asarray(score)
        self._tail = []   # appended by extend(): plain strings, and _ContigBlock's of contigs that stay on the device
        self._tail_first = []  # position (behind the main part) of the first element of every tail item
        self._tail_blocks = []  # which tail items are _ContigBlock's
        self._tail_len = 0
        self.scores = self._score[self._order].tolist()
        self.lengths = (off[1:] - off[:-1])[self._order].tolist()

    def __len__(self):
        return len(self._order) + self._tail_len

    def _texts_at(self, positions):
        """[self[p] for p in positions] with one batched export per block the positions fall into."""
        pos = np.asarray(positions, dtype=np.int64)
        out = np.empty(len(pos), dtype=object)
        for first, item in self._segments():
            here = np.nonzero((pos >= first) & (pos < first + len(item)))[0]
            if not len(here):
                continue
            rel = pos[here] - first
            out[here] = list(item.take(rel)) if type(item) is _ContigBlock else [item[j] for j in rel.tolist()]
        return out.tolist()

    def __iter__(self):
        for _, item in self._segments():
            yield from item

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self._texts_at(np.arange(len(self))[i])
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        if i >= len(self._order):
            i -= len(self._order)
            t = bisect.bisect_right(self._tail_first, i) - 1
            item = self._tail[t]
            return item[i - self._tail_first[t]] if type(item) is _ContigBlock else item
        c = int(self._order[i])
        return self._graph.export_contig_text(c, int(self._off[c + 1] - self._off[c])).decode("latin-1")

    def sort(self, key=None, reverse=False):
        """In-place, stable (``list.sort`` semantics) by the device getScore; see the class docstring."""
        if self._tail:
            raise NotImplementedError("sort after extend: the appended strings carry no device score")
        n = len(self._order)
        if key is not None and n:
            lens = (self._off[1:] - self._off[:-1])[self._order]
            for i in np.argsort(lens, kind="stable")[:4].tolist():  # the shortest ones are cheap to fetch
                if key(self[i]) != self.scores[i]:
                    raise NotImplementedError("LazyContigs.sort orders by the contig score (getScore); this key is a "
                                              "different function and would need every contig's text")
        sc = self._score[self._order].astype(np.int64)
        # stable in both directions: equal scores keep their current relative order, as list.sort(reverse=True) does
        perm = np.argsort(-sc if reverse else sc, kind="stable")
        self._order = self._order[perm]
        self.scores = [self.scores[i] for i in perm.tolist()]
        self.lengths = [self.lengths[i] for i in perm.tolist()]

    def extend(self, more):
        parts = more._parts if type(more) is _PulledReads else [more]
        for part in parts:
            if type(part) is _ContigBlock:
                if len(part):
                    self._tail_blocks.append(len(self._tail))
                    self._tail.append(part)
                    self._tail_first.append(self._tail_len)
                    self._tail_len += len(part)
            else:
                n = len(self._tail)
                self._tail.extend(part)
                n = len(self._tail) - n
                self._tail_first.extend(range(self._tail_len, self._tail_len + n))
                self._tail_len += n

    def packed(self):
        """-> (uint8 characters, uint64 offsets[len + 1]) of the whole sequence, tail blocks and strings included: one
        batched export per block, no Python ``str`` per contig."""
        chars, lens = [], []
        for _, item in self._segments():
            if type(item) is _ContigBlock:
                for c, n in _packed_texts(item._graph, item._idx, item.lengths):
                    chars.append(c)
                    lens.append(n)
            elif item:
                try:
                    chars.append(np.frombuffer("".join(item).encode("latin-1"), dtype=np.uint8))
                except UnicodeEncodeError as e:
                    raise ValueError("reads must be made of single-byte characters for the device path") from e
                lens.append(np.fromiter((len(r) for r in item), dtype=np.int64, count=len(item)))
        offsets = np.zeros(len(self) + 1, dtype=np.uint64)
        if lens:
            np.cumsum(np.concatenate(lens), out=offsets[1:])
        return (np.concatenate(chars) if chars else np.zeros(0, dtype=np.uint8)), offsets

    def write_fasta(self, path, k, append=True, line_width=0):
        """The driver's loop over this sequence (``>SEQUENCE_{i}_{k}mer`` records, II_assembleFromReads.py:65-69) written to
        ``path``: the main part and every tail block are formatted on the device of the graph that holds them and
        streamed to the file (dbg_write_contigs_fasta), runs of plain strings are written by the host in between.
        ``line_width`` W > 0 wraps every contig at W characters, on both routes (``wrap_fasta_record``)."""
        open(path, "a" if append else "w").close()
        for first, item in self._segments():
            if not len(item):
                continue
            write = getattr(item._graph, "write_contigs_fasta", None) if type(item) is _ContigBlock else None
            if write is not None:
                g = item._graph  # the writer takes bare indices: they must still be those of the walk the block came from
                if item._generation is not None and (g.generation != item._generation or g.walks != item._walk):
                    raise RuntimeError("the device contigs of this list are gone (the handle built another graph or walked again)")
                wrap = {"line_width": line_width} if line_width else {}
                write(path, item._idx, append=True, first_number=first, k_label=k, **wrap)
                continue
            with open(path, mode="a") as out_file:
                for j, text in enumerate(item):
                    out_file.write('>SEQUENCE_{}_{}mer\n{}'.format(first + j, k, wrap_fasta_record(text, line_width)))

    def _main_block(self):
        return _ContigBlock(self._graph, self._order, np.asarray(self.lengths, dtype=np.int64), self._final, self._generation,
                            self._walk)

    def _segments(self):
        """The whole sequence in order as (first position, _ContigBlock) and (first position, list of the strings of a run)."""
        yield 0, self._main_block()
        n, at = len(self._order), 0
        for b in self._tail_blocks + [len(self._tail)]:
            if b > at:
                yield n + self._tail_first[at], self._tail[at:b]
            if b < len(self._tail):
                yield n + self._tail_first[b], self._tail[b]
            at = b + 1


class _PulledReads(Sequence):
    """pull_out_read of a graph built from walks: the pulled contigs stay references (graph, contig indices, lengths),
    grouped by the graph that holds them -- the pulled contigs of the main part as one block, then the still pulled
    subset of every block of the tail -- and fetch their text when indexed; the pulled original reads are strings."""

    def __init__(self, reads, idx):
        self._idx = idx = np.asarray(idx, dtype=np.int64)
        self._parts = []  # _ContigBlock's and lists of strings, in read order
        self._first = []
        n = 0
        for first, item in reads._segments():
            lo, hi = np.searchsorted(idx, [first, first + len(item)])
            if type(item) is _ContigBlock:
                part = item.take(idx[lo:hi] - first)
            else:
                part = [item[i] for i in (idx[lo:hi] - first).tolist()]
                if part and self._parts and type(self._parts[-1]) is list:
                    self._parts[-1].extend(part)
                    n += len(part)
                    continue
            if len(part):
                self._parts.append(part)
                self._first.append(n)
                n += len(part)

    def __len__(self):
        return len(self._idx)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        t = bisect.bisect_right(self._first, i) - 1
        return self._parts[t][i - self._first[t]]

    def __iter__(self):
        for part in self._parts:
            yield from part

    def __eq__(self, other):
        return isinstance(other, (list, Sequence)) and list(self) == list(other)


def _walk_source(reads, k):
    """What builds the k-graph of ``reads`` from chains on the device (dbg_build_from_walk(s)), or None: a LazyContigs
    of a current non-final walk over ACGT at k - 1 whose appended tail holds zero or more blocks of contigs of current
    non-final ACGT walks on distinct graphs at smaller k, followed by plain strings.
    -> (graph of the main part, [(graph, contig indices) of the tail blocks], the strings)."""
    if type(reads) is not LazyContigs or reads._final is not False:
        return None
    g = reads._graph
    if g.generation != reads._generation or g.walks != reads._walk or g.alphabet()[1] != 2 or g.sizes()["k"] + 1 != k:
        return None
    nb = len(reads._tail_blocks)
    if reads._tail_blocks != list(range(nb)):  # a string in front of a block
        return None
    blocks, strings, seen = [], reads._tail[nb:], {id(g)}
    for item in reads._tail[:nb]:
        bg = item._graph
        if id(bg) in seen or not item.current() or bg.alphabet()[1] != 2 or bg.sizes()["k"] >= k:
            return None
        seen.add(id(bg))
        blocks.append((bg, item._idx))
    if not all(type(r) is str for r in strings):
        return None
    return g, blocks, strings


def _pack_reads(reads):
    if type(reads) is LazyContigs:
        return reads.packed()
    try:
        blob = "".join(reads).encode("latin-1")  # one byte per character
    except UnicodeEncodeError as e:
        raise ValueError("reads must be made of single-byte characters for the device path") from e
    arr = np.frombuffer(blob, dtype=np.uint8)
    lens = np.fromiter((len(r) for r in reads), dtype=np.uint64, count=len(reads))
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    return arr, offsets


def construct_graph(reads, k, threshold=3, final=False):
    """debruijn.py:206-285 on the GPU.

    Returns ((vertices, edges), pull_out_read, branch_kmer, already_pull_out, edge_count_table).
    """
    if not isinstance(k, (int, np.integer)) or not (1 <= int(k) <= 63):
        raise ValueError("the device path supports 1 <= k <= 63")
    k = int(k)
    src = _walk_source(reads, k)
    if src is not None:
        src, tail_blocks, strings = src
        bases, offsets = _pack_reads(strings)
        if not np.isin(bases, np.frombuffer(b"ACGT", dtype=np.uint8)).all():
            src = None
    if src is not None:
        # the contigs of the (k-1)-graph's walk + the pulled contigs of earlier walks + the appended reads, built from
        # the chains of the graphs that hold them: no contig text is spelled
        g = _dbg.Graph()
        g.build_from_walk(src, k, reads._order, bases, offsets, tail_blocks)
    else:
        if isinstance(reads, DeviceReads):
            g = reads._graph  # reads are resident (alphabet is checked by the kernels: AlphabetError is a ValueError)
        else:
            bases, offsets = _pack_reads(reads)
            g = _dbg.Graph()
            g.set_reads(bases, offsets)
        g.build(k)
    g.refine_edge_order()  # Counter order of the successors (first-seen ties), debruijn.py:159-165, :215-216
    sz = g.sizes()
    print('number of {}mer: '.format(k), sz["n_nodes"])  # debruijn.py:224

    if threshold == 0:
        # debruijn.py:163 divides by threshold as soon as a vertex has two distinct successors
        _, _, counts, _ = g.export_nodes(keys=False, stamps=False, flags=False)
        if ((counts != 0).sum(axis=1) > 1).any():
            raise ZeroDivisionError("division by zero")
        threshold = 1
    g.prune(threshold)
    n_branch = g.sizes()["n_branch"]
    print('branch number: ', n_branch)  # debruijn.py:236
    g.remove_tips()
    if not final:
        g.mark_pull_reads()

    alphabet, bits = g.alphabet()                 # code -> character
    chars = alphabet.decode("latin-1")
    n_nodes = sz["n_nodes"]
    two_words = bits == 2 and bits * k > 64

    def load_arrays():
        keys, stamps, counts, flags = g.export_nodes()
        rank_mc, rank_fs = g.export_orders()      # (n, D): successor codes by rank
        return {"keys": keys, "stamps": stamps, "counts": counts, "flags": flags, "rank_mc": rank_mc, "rank_fs": rank_fs,
                "order": g.export_dict_order().astype(np.int64),  # dict order == first-occurrence order (sorted on the device)
                "keys_hi": g.export_keys_hi() if two_words else None, "keep": g.export_keepmask()}

    byref = bits == 5 and bits * (k + 1) > 64  # generic alphabet, k >= 12: a node's k-mer is the text at its first occurrence
    lazy = n_nodes >= LAZY_MIN_NODES and not byref
    if lazy:  # the arrays stay on the device until a view is asked for something; then in table order, through `order`
        generation = g.generation

        def load_later():
            if g.generation != generation:
                raise RuntimeError(_STALE_VIEWS)
            return load_arrays()

        store = _NodeStore(k, alphabet, bits, n_nodes, load_later, graph=g)
        vertices, edges, ect = _LazyVertices(store), _LazyEdges(store), _LazyEdgeCounts(store)
    else:
        a = load_arrays()
        keys, stamps, counts, flags, rank_mc, rank_fs = a["keys"], a["stamps"], a["counts"], a["flags"], a["rank_mc"], a["rank_fs"]
        order, keys_hi, keep = a["order"], a["keys_hi"], a["keep"]
        n_ranks = rank_mc.shape[1]
        if byref:
            text = reads._pull()[0] if isinstance(reads, DeviceReads) else bases.tobytes().decode("latin-1")
            labels = [text[p:p + k] for p in (stamps[order] >> np.uint64(1)).tolist()]
        else:
            labels = _dbg.decode_keys(keys[order], k, alphabet, bits, None if keys_hi is None else keys_hi[order])
        vertices, edges, ect = _Vertices(), {}, {}
        inverse = np.empty(len(order), dtype=np.int64)
        inverse[order] = np.arange(len(order))
        row_labels = lambda rows: [labels[i] for i in inverse[rows]]
        counts_o = counts[order]
        rank_mc, rank_fs = rank_mc[order], rank_fs[order]
        flags_o = flags[order]
        outdeg = (counts_o != 0).sum(axis=1)
        indeg = flags_o & _dbg.F_INDEG
        pulled_o = (flags_o & _dbg.F_PULLED) != 0
        keep_o = keep[order]
    if not lazy:
        # plain Python lists: indexing numpy scalars per node costs more than everything else in this loop
        outdeg_l, indeg_l, pulled_l, keep_l = outdeg.tolist(), indeg.tolist(), pulled_o.tolist(), keep_o.tolist()
        code1_l, cnt1_l = counts_o.argmax(axis=1).tolist(), counts_o.max(axis=1).tolist()
        for i, lab in enumerate(labels):
            nd = outdeg_l[i]
            vertices[lab] = Node(lab, indeg_l[i], nd)
            if nd == 1:    # the common case: one successor, no ranking to consult
                code = code1_l[i]
                ch = chars[code]
                ect[lab + ch] = cnt1_l[i]
                if not pulled_l[i]:
                    edges[lab] = [lab[1:] + ch] if (keep_l[i] >> code) & 1 else []
                continue
            if nd == 0:
                if not pulled_l[i]:
                    edges[lab] = []
                continue
            c = counts_o[i]
            tail = lab[1:]
            # a rank holds a code only where the node has that many successors (DNA ranks all four codes)
            ranked = [int(code) for code in rank_mc[i, :n_ranks] if code != 0xFF and c[code]][:nd]  # Counter.most_common order
            for code in rank_fs[i, :n_ranks]:                                                        # Counter key order
                if code != 0xFF and c[code]:
                    ect[lab + chars[code]] = int(c[code])
            if not pulled_l[i]:
                kp = keep_l[i]
                edges[lab] = [tail + chars[code] for code in ranked if (kp >> code) & 1]

    # the two label lists: the (few) marked rows, selected, put into the reference's order and spelled on the device side
    def marked_labels(flag):
        rows, mk, mhi = g.export_marked(flag, keys=not byref)
        if byref:
            return row_labels(rows.astype(np.int64))
        return _dbg.decode_keys(mk, k, alphabet, bits, mhi if two_words else None)

    already_pull_out = _Tracked(marked_labels(_dbg.F_PULLED))

    if final:  # debruijn.py:281-283
        pull_out_read = []
        branch_kmer = _Tracked()
    else:
        rf = g.export_pull_reads()
        pulled_idx = np.nonzero(rf)[0]
        if src is not None:
            pull_out_read = _PulledReads(reads, pulled_idx)
        else:
            if isinstance(reads, DeviceReads):
                pull_out_read = reads.take(pulled_idx)
            elif type(reads) is LazyContigs:
                pull_out_read = reads._texts_at(pulled_idx)  # one batched export per block, not one call per read
            else:
                pull_out_read = [reads[i] for i in pulled_idx]
        branch_kmer = _Tracked(marked_labels(_dbg.F_BRANCH))

    token = object()
    vertices._graph = g
    vertices._state = {"token": token, "final": bool(final), "k": k, "n_branch": int(n_branch), "generation": g.generation}
    branch_kmer._token = token
    already_pull_out._token = token
    return (vertices, edges), pull_out_read, branch_kmer, already_pull_out, ect


def output_contigs(g, branch_kmer, already_pull_out):
    """debruijn.py:326-347 (DFS of :288-316) on the GPU.

    ``g``, ``branch_kmer`` and ``already_pull_out`` must come from one construct_graph call
    of this module (the graph lives on the device); ``branch_kmer == []`` selects the
    reference's final-mode walk.
    """
    V = g[0]
    graph = getattr(V, "_graph", None)
    state = getattr(V, "_state", None)
    if graph is None or state is None:
        raise TypeError("output_contigs needs the (vertices, edges) returned by this module's construct_graph")
    if state.get("generation") != graph.generation:
        raise ValueError("the device graph of this construct_graph result was replaced by a later build on the same handle "
                         "(construct_graph on the same DeviceReads): call output_contigs before building again")
    tok = state["token"]
    if getattr(already_pull_out, "_token", None) is not tok or (
            getattr(branch_kmer, "_token", None) is not tok and len(branch_kmer) != 0):
        raise ValueError("branch_kmer / already_pull_out must be the lists returned with this graph "
                         "(the device walk uses the graph state they describe)")
    final_mode = len(branch_kmer) == 0  # identical to the chain walk when the graph has no branch node
    sz = graph.sizes()
    print('Number of kmers have no income edges: ', sz["n_starts"])  # debruijn.py:336
    graph.walk(final_mode, MAX_CONTIG_CHARS)
    if not graph.sizes()["contigs_materialised"]:  # index only: the texts stay on the device until asked for
        off, score, stamp, seq = graph.export_contig_index()
        lazy = LazyContigs(graph, np.lexsort((seq, stamp)), off, score)
        lazy._final = bool(final_mode) and sz["n_branch"] > 0  # without a branch node the final walk is the chain walk
        lazy._generation, lazy._walk = graph.generation, graph.walks
        return lazy
    off, chars, score, stamp, seq = graph.export_contigs()
    order = np.lexsort((seq, stamp))  # starts in dict order, emission order inside a start
    text = chars.tobytes().decode("latin-1")
    out = ContigList(text[int(off[i]):int(off[i + 1])] for i in order)
    out.scores = [int(score[i]) for i in order]
    out._graph, out._generation, out._walk, out._index = graph, graph.generation, graph.walks, order
    return out


def get_score_device(contigs):
    """getScore (II_assembleFromReads.py:14-18) of each contig as computed by the walk kernel."""
    return list(contigs.scores)


def score_sequences(edge_count_table, sequences, k):
    """``[getScore(edge_count_table, s, k) for s in sequences]`` (II_assembleFromReads.py:14-18) as a list of ints.

    On the lazy table of a graph that still lives on the device this is one call (dbg_score_sequences): the text goes
    over once and every (k+1)-mer window is looked up and added there.  On a dict -- or a lazy table whose graph the
    library does not look up -- it is the reference's loop.  A sequence with a (k+1)-mer that is no edge raises KeyError
    with that (k+1)-mer, for the first such window of the first such sequence: what the reference's loop raises."""
    sequences = list(sequences)
    store = getattr(edge_count_table, "_s", None)
    g = getattr(store, "_graph", None) if type(edge_count_table) is _LazyEdgeCounts else None
    if g is not None and store.k == k and all(type(s) is str for s in sequences):
        if g.generation != store._generation:
            raise RuntimeError(_STALE_VIEWS)
        try:
            chars, offsets = _pack_reads(sequences)
            scores, miss = g.score_sequences(chars, offsets)
        except ValueError:       # a character of more than one byte: no edge holds it, the loop below says where
            scores = None
        except _dbg.DbgError as err:
            if err.code != _dbg.DBG_E_ARG:
                raise
            scores = None
        if scores is not None:
            bad = np.nonzero(miss != np.iinfo(np.uint64).max)[0]
            if bad.size:
                s, i = sequences[int(bad[0])], int(miss[bad[0]])
                raise KeyError(s[i:i + k + 1])
            return [int(x) for x in scores]
    return [sum(edge_count_table[s[i:i + k + 1]] for i in range(len(s) - k)) for s in sequences]


def count_spectrum(g, edge_count_table, n_bins=256):
    """Abundance spectrum and degree statistics of the graph ``construct_graph`` returned, as a dict:

      ``edge_hist[c]``  number of (k+1)-mers ``e`` with ``edge_count_table[e] == c`` -- a build at k counts (k+1)-mers, so
                        this is the exact (k+1)-mer abundance spectrum of the reads: for the 31-mer spectrum build at k = 30;
      ``node_hist[c]``  number of nodes whose successor counts sum to ``c`` (``len(edges[v])`` before pruningEdges;
                        ``node_hist[0]``: the nodes without a successor).  That sum is the number of windows that START
                        at the k-mer, not the k-mer's multiplicity: the last k-mer of a read is not counted;
      ``D[d]``          number of nodes with ``d`` distinct successors (``Node.outdegree``), uint64[33];
      ``n_nodes``, ``n_edges``, ``sum_edge_counts``, ``max_edge_count``, ``max_out_weight``, ``n_bins``.

    With ``n_bins = B`` a count ``c`` lands in bin ``min(c, B - 1)``; ``edge_hist[0]`` is always 0; 2 <= B <= 2**20.
    On the views (or the dicts) ``construct_graph`` of this module returned, while their graph still lives on the device,
    this is one call (dbg_count_spectrum): nothing of the size of the graph moves, and the dict also holds ``K`` (kept successors per node after pruningEdges, over all nodes),
    ``pruned``, ``peak_extra_device_bytes`` and ``ms_kernel``.  On plain dicts (the reference's own) it is the loop below -- the statement of the
    definitions that the device is tested against; ``K`` and ``pruned`` are None there (the dicts of a pruned graph no
    longer hold the pulled nodes' successors)."""
    B = int(n_bins)
    if not 2 <= B <= _dbg.SP_MAX_BINS:
        raise ValueError("n_bins must be in 2..2**20")
    store = getattr(edge_count_table, "_s", None)
    graph = getattr(store, "_graph", None) if type(edge_count_table) is _LazyEdgeCounts else None
    if graph is not None:
        if graph.generation != store._generation:
            raise RuntimeError(_STALE_VIEWS)
        return graph.count_spectrum(B)
    V = g[0]
    graph, state = getattr(V, "_graph", None), getattr(V, "_state", None)
    if graph is not None and state is not None and type(V) is _Vertices:  # the dicts of a small graph that is still on the device
        if state.get("generation") != graph.generation:
            raise RuntimeError(_STALE_VIEWS)
        return graph.count_spectrum(B)
    edge_hist, node_hist, deg = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64), np.zeros(33, dtype=np.uint64)
    weight = dict.fromkeys(V, 0)
    total = most = 0
    for e, c in edge_count_table.items():
        edge_hist[min(c, B - 1)] += 1
        weight[e[:-1]] += c
        total += c
        most = max(most, c)
    for v, w in weight.items():
        node_hist[min(w, B - 1)] += 1
        deg[V[v].outdegree] += 1
    return {"n_nodes": len(V), "n_edges": len(edge_count_table), "sum_edge_counts": total, "max_edge_count": most,
            "max_out_weight": max(weight.values(), default=0), "D": deg, "K": None, "pruned": None, "n_bins": B,
            "edge_hist": edge_hist, "node_hist": node_hist}


# ------------------------------------------------------------------------------------------------------------------
# The two helpers of the reference module that its pipeline never calls (debruijn.py:210 mentions get_kmers in a
# comment only).  Kept so that the module surface is complete; k-mer enumeration runs on the device, the glue
# step and the overlap adjacency are host bookkeeping over short lists.
# ------------------------------------------------------------------------------------------------------------------
def _glue_short_sequences(sequences, k):
    """debruijn.py:39-56: sequences shorter than k leave the list; each is then glued onto every remaining sequence
    that overlaps it by exactly three characters (at either end).  Mutates ``sequences`` like the reference, and walks
    the short list the way a Python ``for`` does while elements are removed from it (the element after a removed
    one is skipped)."""
    short = [s for s in sequences if len(s) < k]
    for s in short:
        sequences.remove(s)
    i = 0
    while i < len(short):
        piece = short[i]
        glued = False
        for j, seq in enumerate(sequences):
            if seq[len(seq) - 3:] == piece[:3]:
                sequences[j] = seq + piece[3:]
                glued = True
            if piece[len(piece) - 3:] == seq[:3]:      # tested against the sequence as it was before this step
                sequences[j] = piece + seq[3:]
                glued = True
        if glued:
            short.remove(piece)
        i += 1


def get_kmers(sequences, k):
    """debruijn.py:35-75: distinct k-mers of the sequences (after the glue step above, which mutates the argument), in
    first-occurrence order.  Sequences longer than k go through the device build (its node table IS that list);
    sequences of exactly k characters hold one k-mer each and are merged in by position on the host."""
    _glue_short_sequences(sequences, k)
    first = {}  # k-mer -> position of its first occurrence in the concatenation of the sequences
    if any(len(s) > k for s in sequences):
        bases, offsets = _pack_reads(sequences)
        g = _dbg.Graph()
        try:
            g.set_reads(bases, offsets)
            g.build(k)
            keys, stamps, _, _ = g.export_nodes(counts=False, flags=False)
            alphabet, bits = g.alphabet()
            pos = (stamps >> np.uint64(1)).tolist()
            if bits == 5 and bits * (k + 1) > 64:      # keyed by reference: the text at the stamp is the k-mer
                text = bases.tobytes().decode("latin-1")
                labels = [text[p:p + k] for p in pos]
            else:
                hi = g.export_keys_hi() if bits == 2 and bits * k > 64 else None
                labels = _dbg.decode_keys(keys, k, alphabet, bits, hi)
            first = dict(zip(labels, pos))
        finally:
            g.close()
    off = 0
    for s in sequences:
        if len(s) == k and first.get(s, off + 1) > off:
            first[s] = off
        off += len(s)
    return sorted(first, key=first.get)


def get_graph_from_kmers(kmers, k):
    """debruijn.py:78-95: (k-1)-overlap adjacency over a list of k-mers with true in/out degrees -- same dict and list
    orders as the reference's all-pairs scan (quadratic there; prefix / suffix indexes here)."""
    vertices, edges = {}, {}
    seq_no = {}                     # key -> its position in `edges` (insertion order)
    by_prefix, by_suffix = {}, {}   # (k-1)-character prefix / suffix -> keys in insertion order
    for kmer in kmers:
        if kmer not in seq_no:
            seq_no[kmer] = len(seq_no)
            by_prefix.setdefault(kmer[:k - 1], []).append(kmer)
            by_suffix.setdefault(kmer[1:], []).append(kmer)
        node = vertices[kmer] = Node(kmer)   # a repeated k-mer starts over, as in the reference
        edges[kmer] = []
        follows = by_prefix.get(kmer[1:], ())        # kmer -> other
        precedes = by_suffix.get(kmer[:k - 1], ())   # other -> kmer
        # the reference visits every key once, in insertion order, and tests "kmer -> key" before "key -> kmer"
        a = b = 0
        while a < len(follows) or b < len(precedes):
            if b >= len(precedes) or (a < len(follows) and seq_no[follows[a]] <= seq_no[precedes[b]]):
                other = follows[a]
                a += 1
                edges[kmer].append(other)
                node.outdegree += 1
                vertices[other].indegree += 1
            else:
                other = precedes[b]
                b += 1
                edges[other].append(kmer)
                vertices[other].outdegree += 1
                node.indegree += 1
    return vertices, edges
