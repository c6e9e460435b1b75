"""The generic (non-ACGT) engine's whole traversal against the Python oracle above the vector sizes: 10^5 short
peptide-like reads over a 20-letter and a 32-symbol alphabet, non-final, on both sides of the packed (k <= 11,
dbg_generic.h) / by-reference (k >= 12, dbg_genref.h) key switch.  construct_graph + output_contigs, orders included."""
import contextlib
import io
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AA20 = "ACDEFGHIKLMNPQRSTVWY"
SYM32 = AA20 + "BJOUXZ" + "acdefg"   # 32 distinct symbols: the most 5-bit codes hold


def peptide_reads(alphabet, seed, n_reads=100_000, n_proteins=4000, protein_len=300, err=0.005):
    """Reads of 20..40 symbols cut from random 'proteins' (2.5x coverage), with substitutions."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alphabet.encode(), dtype=np.uint8)
    prot = a[rng.integers(0, a.size, size=(n_proteins, protein_len))]
    lens = rng.integers(20, 41, size=n_reads)
    which = rng.integers(0, n_proteins, size=n_reads)
    start = (rng.random(n_reads) * (protein_len - lens + 1)).astype(np.int64)
    reads = []
    for p, s, ln in zip(which.tolist(), start.tolist(), lens.tolist()):
        r = prot[p, s:s + ln].copy()
        flip = rng.random(ln) < err
        r[flip] = a[rng.integers(0, a.size, size=int(flip.sum()))]
        reads.append(r.tobytes().decode("ascii"))
    return reads


@pytest.mark.parametrize("alphabet,k", [(AA20, 8), (AA20, 11), (AA20, 12), (AA20, 20),
                                        (SYM32, 8), (SYM32, 11), (SYM32, 12), (SYM32, 20)],
                         ids=lambda x: f"a{len(x)}" if isinstance(x, str) else f"k{x}")
def test_generic_traversal_equals_python_oracle(alphabet, k):
    import debruijn as prod
    from golden_util import canonical
    from oracle import dbg_oracle as orc
    reads = peptide_reads(alphabet, 100 + k + len(alphabet))
    res, secs = [], []
    for mod in (prod, orc):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            g, pull, branch, pulled, ect = mod.construct_graph(list(reads), k, threshold=2)
            contigs = mod.output_contigs(g, branch, pulled)
        r = canonical(g, pull, branch, pulled, ect, contigs)
        r["stdout"] = buf.getvalue()
        res.append(r)
        secs.append(time.perf_counter() - t0)
    for field in res[1]:
        assert res[0][field] == res[1][field], field
    o = res[1]
    assert o["branch_kmer"] and o["already_pull_out"] and o["pull_out_read"] and o["contigs"]
    print(f"\n[generic a{len(alphabet)} k={k}] nodes {len(o['vertices'])} branch {len(o['branch_kmer'])} "
          f"pulled {len(o['already_pull_out'])} pull_reads {len(o['pull_out_read'])} contigs {len(o['contigs'])} "
          f"contig_chars {sum(map(len, o['contigs']))} oracle {secs[1]:.1f}s device {secs[0]:.1f}s")
