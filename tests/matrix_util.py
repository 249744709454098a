"""What tests/test_matrix_host.py and tests/test_gpu_matrix.py share: the recorded files of tests/golden/matrix/ (made by
tests/golden/make_matrix.py from the reference's own write_matrix(), the CLI's partition-list lines and __str__), the
comparison of a written matrix with a recorded one, and flat orders with lengths for given copy counts."""
import glob
import os

import numpy as np

from pangenomenem_amd.matrix import FIELDS, LISTS, summary, write_partitions

MATRIX_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix", "*.json")))


def repeated_by_organism(rec):
    """which families were repeated when each organism came (the update declares its own on top of the base's)"""
    base, both = frozenset(rec["repeated"]), frozenset(rec["repeated"]) | frozenset(rec["update_repeated"])
    return dict([(org, base) for org in rec["organisms"]] + [(org, both) for org in rec["new_organisms"]])


def same_matrix_text(got, want, sep, what):
    """byte for byte, except the fields the reference joins from a set in hash order -- the products (column 3) and, in
    the .csv, a cell's genes -- which are compared as sets"""
    got_lines, want_lines = got.split("\n"), want.split("\n")
    assert len(got_lines) == len(want_lines), what
    assert got_lines[0] == want_lines[0] and got_lines[-1] == want_lines[-1] == "", what + ": header"
    for a, b in zip(got_lines[1:-1], want_lines[1:-1]):
        fa, fb = a.split(sep), b.split(sep)
        assert len(fa) == len(fb), what + ": " + a
        for col, (x, y) in enumerate(zip(fa, fb)):
            if col == 2 or (sep == "," and col >= 14):
                assert x[0] == x[-1] == '"' and len(x.split("|")) == len(y.split("|")) and set(x[1:-1].split("|")) == set(y[1:-1].split("|")), (what, col, a, b)
            else:
                assert x == y, (what, col, a, b)


def files_equal_fixture(table, rec, ann, tmp_path, budget=None):
    """write_matrix, write_partitions and summary of a table against a fixture's recorded text"""
    out = str(tmp_path)
    kw = {} if budget is None else dict(budget=budget)
    table.write_matrix(os.path.join(out, "matrix"), rec["labels"], ann, **kw)
    write_partitions(out, rec["labels"], table)
    want = rec["files"]
    got = {os.path.relpath(os.path.join(root, name), out): open(os.path.join(root, name), newline="").read()
           for root, _, names in os.walk(out) for name in names}
    assert sorted(got) == sorted(want)
    same_matrix_text(got["matrix.Rtab"], want["matrix.Rtab"], "\t", rec["name"] + " Rtab")
    same_matrix_text(got["matrix.csv"], want["matrix.csv"], ",", rec["name"] + " csv")
    for name in ["pangenome.txt"] + ["partitions/%s.txt" % k for k in LISTS]:
        assert got[name] == want[name], (rec["name"], name)
    assert summary(rec["labels"], table) == rec["summary"]


def same_table(got, want, what=""):
    for name in FIELDS:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s %s %s / %s %s" % (what, name, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b), "%s: %s differs at %s" % (what, name, np.flatnonzero(a != b)[:5].tolist())


def counts_orders(counts, rng, lengths="random", contigs=2):
    """flat orders in which organism o carries counts[i][o] genes of family i (ids 0 .. n - 1, no repeated family), the
    organisms walked in column order, each one's genes shuffled and cut into contigs; lengths: "random" (few values, so
    that lengths repeat inside a family), "equal", "distinct" or "negative".  Returns a dict with gene_len too."""
    counts = np.asarray(counts, np.int64)
    n, d = counts.shape
    genes, cptr, corg = [], [0], []
    for o in range(d):
        seq = rng.permutation(np.repeat(np.arange(n), counts[:, o]))
        cuts = np.sort(rng.integers(0, len(seq) + 1, contigs - 1))
        for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(seq)]])):
            genes.append(seq[lo:hi])
            cptr.append(cptr[-1] + hi - lo)
            corg.append(o)
    genes = np.concatenate(genes).astype(np.int32)
    g = len(genes)
    gene_len = dict(random=lambda: rng.integers(-3, 4, g) * 100, equal=lambda: np.full(g, 731), distinct=lambda: rng.permutation(g) - g // 2,
                    negative=lambda: -1 - rng.integers(0, 5, g))[lengths]().astype(np.int32)
    return dict(genes=genes, contig_ptr=np.asarray(cptr, np.int32), contig_org=np.asarray(corg, np.int32),
                contig_circular=np.zeros(len(corg), np.uint8), d=d, repeated=np.zeros(n, np.uint8), gene_len=gene_len)


def random_counts(rng, n, d, density=0.4, p_multi=0.1):
    """copy counts with every family somewhere and every organism carrying something"""
    counts = (rng.random((n, d)) < density).astype(np.int64)
    counts[np.arange(n), rng.integers(0, d, n)] = 1
    counts[rng.integers(0, n, d), np.arange(d)] = 1
    multi = (counts > 0) & (rng.random((n, d)) < p_multi)
    counts[multi] = rng.choice([2, 3, 9, 10, 11, 99, 100], int(multi.sum()))
    return counts
