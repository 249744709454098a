"""The loader on the device (loader.load_files: nemgpu_gff_*, csrc/nem_gff.hip) against its statement
loader.load_arrays_host -- which tests/test_loader_host.py holds against the reference's own loader -- array for array
and span for span: on the recorded sets of files, on sets sized around the byte kernels' tile (nemgpu_gff_info), with
the string hash cut to a few bits so that the tables' probes collide, and under different batch cuts; the first error
under different batch cuts; Master.from_files against Master.from_annotations of the recorded annotations, and a
partition run on either."""
import os
import random

import numpy as np
import pytest

from pangenomenem_amd import loader
from pangenomenem_amd.chunks import Master
from tests.loader_util import (CASES, RAISES, annotations_of, case_id, cds_line, equals_recording, error_of, paths, recorded, same_loaded,
                               write_set)
from tests.orders_util import same_master

pytestmark = pytest.mark.gpu

GOOD = [p for p in CASES if recorded(p)["raises"] is None]
BAD = [p for p in CASES if recorded(p)["raises"] is not None]


@pytest.mark.parametrize("path", GOOD, ids=case_id)
def test_recorded_sets(gpu_lib, path):
    rec = recorded(path)
    want = loader.load_arrays_host(*paths(path), **rec["args"])
    for options in (dict(), dict(batch_bytes=1), dict(_hash_bits=1)):
        got = loader.load_files(*paths(path), **rec["args"], **options)
        same_loaded(got, want, "%s %r" % (rec["name"], options))
        equals_recording(got, rec, "%s %r" % (rec["name"], options))


@pytest.mark.parametrize("path", BAD, ids=case_id)
def test_recorded_errors(gpu_lib, path):
    rec = recorded(path)
    want = error_of(lambda: loader.load_arrays_host(*paths(path), **rec["args"]))
    assert want is not None and want[0] is RAISES[rec["raises"]]
    for batch_bytes in (256 << 20, 1):
        assert error_of(lambda: loader.load_files(*paths(path), batch_bytes=batch_bytes, **rec["args"])) == want, rec["name"]


def test_info(gpu_lib):
    """The thresholds list is empty (one radix sort for every contig size), so its line asserts nothing: the sizes at
    which the sort and the scans do change their path are run by tests/test_gpu_loader_shapes.py."""
    info = loader.gff_info()
    assert info["tile"] >= 64 and info["tile"] % 16 == 0
    assert info["sort_thresholds"] == sorted(info["sort_thresholds"]) and all(t > 1 for t in info["sort_thresholds"])


def sized(lines, size):
    """the lines and a '#' comment of three fields that brings the file to `size` bytes"""
    body = b"".join(l + b"\n" for l in lines)
    pad = size - len(body) - len(b"#\tx\t\n")
    assert pad >= 0
    return body + b"#\tx\t" + b"y" * pad + b"\n"


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """One set around the kernels' tile and the sort's sizes, with its statement: files of tile - 1, 0, tile and
    tile + 1 bytes; a line longer than a tile after a line that ends exactly at a tile's edge; contigs of 1, 63, 64, 65
    genes (and of every sort threshold and its neighbours), their starts shuffled with ties; 1 000 contigs of one gene.
    The thresholds list is empty; rocPRIM's switches by total gene count are run by tests/test_gpu_loader_shapes.py."""
    info = loader.gff_info()
    tile = info["tile"]
    genes, gffs = [], []

    def gene():
        genes.append(b"g%d" % len(genes))
        return genes[-1]

    for size in (tile - 1, 0, tile, tile + 1):
        gffs.append(sized([cds_line(b"c%d" % (k % 2), 1000 - k, gene()) for k in range(5)], size) if size else b"")
    first = cds_line(b"edge", 5, gene())
    first = first + b"x" * (tile - 1 - len(first))                          # its '\n' is the tile's last byte
    gffs.append(b"\n".join([first, cds_line(b"edge", 3, gene(), pad=b"L" * (tile + 37)), cds_line(b"edge", 4, gene())]))
    rng = np.random.RandomState(11)
    sizes = sorted({1, 63, 64, 65} | {t + e for t in info["sort_thresholds"] for e in (-1, 0, 1)})
    lines = [(c, cds_line(b"k%d" % c, int(rng.randint(0, max(n // 2, 1))) - 3, gene())) for c, n in enumerate(sizes) for _ in range(n)]
    gffs.append(b"\r\n".join(lines[j][1] for j in rng.permutation(len(lines))) + b"\r\n")      # the contigs interleaved
    gffs.append(b"".join(cds_line(b"s%d" % k, 7, gene()) + b"\n" for k in range(1000)))
    fams = b"".join(b"F%d\t%s\n" % (k % 97, g) for k, g in enumerate(genes))
    orgs, fam = write_set(tmp_path_factory.mktemp("shapes"), gffs, fams)
    want = loader.load_arrays_host(orgs, fam, lim_occurence=10)
    assert [len(g) for g in gffs[:4]] == [tile - 1, 0, tile, tile + 1] and gffs[4][tile - 1:tile] == b"\n"
    per_contig = np.diff(want.orders["contig_ptr"]).tolist()
    assert per_contig[:7] == [3, 2, 3, 2, 3, 2, 3] and sorted(per_contig[7:-1000]) == sizes and per_contig[-1000:] == [1] * 1000
    assert want.families_repeted
    return orgs, fam, want, tile, sum(len(g) for g in gffs)


@pytest.mark.parametrize("options", [dict(), dict(batch_bytes=1), dict(batch_bytes=3), dict(_hash_bits=2), dict(_hash_bits=2, batch_bytes=1)],
                         ids=["whole", "file_per_batch", "three_tiles", "colliding", "colliding_file_per_batch"])
def test_shapes(gpu_lib, shapes, options):
    orgs, fam, want, tile, total = shapes
    if options.get("batch_bytes") == 3:
        options = dict(options, batch_bytes=3 * tile)
        assert tile < 3 * tile < total                                       # some batches of several files, not one of all
    same_loaded(loader.load_files(orgs, fam, lim_occurence=10, **options), want, repr(options))


def test_one_byte_file(gpu_lib, tmp_path):
    orgs, fam = write_set(tmp_path, [cds_line(b"c", 1, b"a") + b"\n", b"\n"], b"F a\n")
    want = error_of(lambda: loader.load_arrays_host(orgs, fam))
    assert want[0] is ValueError and "o1.gff: line 1" in want[1]
    assert error_of(lambda: loader.load_files(orgs, fam)) == want
    orgs, fam = write_set(tmp_path / "b", [b"#", cds_line(b"c", 1, b"a")], b"F a\n")
    assert error_of(lambda: loader.load_files(orgs, fam)) == error_of(lambda: loader.load_arrays_host(orgs, fam))


def test_inferred_singletons_at_size(gpu_lib, tmp_path):
    orgs, fam, _ = loader.synth_files(str(tmp_path), [[40, 3], [25], [60, 1, 1]], n_families=9, seed=5)
    with open(fam, "rb") as f:
        keep = b"".join(f.read().splitlines(True)[::2])                       # every other family's genes become singletons
    with open(fam, "wb") as f:
        f.write(keep + b"g0_3 late\n")                                       # and a family named like a gene
    want = loader.load_arrays_host(orgs, fam, lim_occurence=4, infer_singletons=True)
    assert len(want.families) > 9
    for options in (dict(), dict(batch_bytes=1, _hash_bits=3)):
        same_loaded(loader.load_files(orgs, fam, lim_occurence=4, infer_singletons=True, **options), want, repr(options))


def test_first_error_whatever_the_batches(gpu_lib, tmp_path):
    ok = lambda k, n: [cds_line(b"c", 10 * j, b"o%dg%d" % (k, j)) for j in range(n)]
    o1 = ok(1, 10)
    o1[6] = cds_line(b"c", 3, b"o1g1")                                       # line 7: the ID of line 2 again
    o1[8] = cds_line(b"c", 3, b"nobody")                                     # line 9: an unknown gene
    o2 = ok(2, 4)
    o2[0] = o2[0].replace(b"\t0\t", b"\tzero\t", 1)                          # line 1: a bad START
    gffs = [b"\n".join(x) + b"\n" for x in (ok(0, 6), o1, o2, [b"short"])]
    fams = b"F " + b" ".join(b"o%dg%d" % (k, j) for k in range(3) for j in range(10)) + b"\n"
    orgs, fam = write_set(tmp_path, gffs, fams)
    want = error_of(lambda: loader.load_arrays_host(orgs, fam))
    assert want[0] is ValueError and "o1.gff: line 7" in want[1] and "'o1g1'" in want[1]
    for batch_bytes in (1, len(gffs[0]) + len(gffs[1]) + 2, 256 << 20):
        assert error_of(lambda: loader.load_files(orgs, fam, batch_bytes=batch_bytes)) == want, batch_bytes
    o1[6] = cds_line(b"c", 3, b"o1g6")                                       # without it the unknown gene of line 9 is first
    orgs, fam = write_set(tmp_path / "b", [gffs[0], b"\n".join(o1) + b"\n", gffs[2], gffs[3]], fams)
    want = error_of(lambda: loader.load_arrays_host(orgs, fam))
    assert want[0] is KeyError and "o1.gff: line 9" in want[1]
    for batch_bytes in (1, 256 << 20):
        assert error_of(lambda: loader.load_files(orgs, fam, batch_bytes=batch_bytes)) == want, batch_bytes


@pytest.mark.parametrize("path", GOOD, ids=case_id)
def test_master_from_files(gpu_lib, path):
    rec = recorded(path)
    for directed in (False, True):
        a = Master.from_annotations(annotations_of(rec), rec["organisms"], rec["circular_contig_size"], rec["families_repeted"], directed=directed)
        b = Master.from_files(*paths(path), directed=directed, **rec["args"])
        try:
            assert a.names == b.names and a.organism_names == b.organism_names and a.id_names == b.id_names
            assert np.array_equal(a.order, b.order) and a.directed == b.directed and a.f == b.f
            assert a.repeated_by_organism == b.repeated_by_organism
            same_master(b.arrays(), a.arrays(), "%s directed %d" % (rec["name"], directed))
        finally:
            a.close()
            b.close()


def test_partition_of_a_master_from_files(gpu_lib, tmp_path):
    orgs, fam, _ = loader.synth_files(str(tmp_path), [[150, 60]] * 30, n_families=300, seed=2, shuffle_starts=False)
    want = loader.load_arrays_host(orgs, fam, lim_occurence=2)
    assert want.families_repeted
    a = Master.from_annotations(want.annotations(), want.organisms, want.circular_contig_size, want.families_repeted)
    b = Master.from_files(orgs, fam, lim_occurence=2)
    try:
        same_master(b.arrays(), a.arrays(), "synthetic")
        ra = a.partition(chunk_size=10, rng=random.Random(5), batch=8, tie="libc", seed=3)
        rb = b.partition(chunk_size=10, rng=random.Random(5), batch=8, tie="libc", seed=3)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2] and ra[2] > 0
    finally:
        a.close()
        b.close()


def test_two_loads_give_identical_bytes(gpu_lib, shapes):
    orgs, fam, want, _, _ = shapes
    a, b = loader.load_files(orgs, fam, lim_occurence=10), loader.load_files(orgs, fam, lim_occurence=10)
    for k, v in a.arrays().items():
        assert v.tobytes() == b.arrays()[k].tobytes(), k
    assert os.path.isfile(orgs)
