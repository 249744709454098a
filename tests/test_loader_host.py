"""loader.load_arrays_host, the statement of the device loader, against what the reference's own
__initialize_from_files made of the recorded sets of files (tests/golden/loader/): the annotations with their dict
orders, the circular sizes, the repeated families, the organisms, and orders == orders_from_annotations of the
reference's output; every error case by type and message; that nothing depends on where the batches are cut."""
import os

import numpy as np
import pytest

from pangenomenem_amd import loader
from tests.loader_util import CASES, RAISES, case_id, equals_recording, error_of, paths, recorded, same_loaded, write_set, cds_line

GOOD = [p for p in CASES if recorded(p)["raises"] is None]
BAD = [p for p in CASES if recorded(p)["raises"] is not None]
# the message of every recorded error case: the file and the line (1-based) it names, and a word of the reason
MESSAGES = {"err_unknown": ("o2.gff: line 2", "'zz'"), "err_short_line": ("o2.gff: line 2", "fewer than 3"),
            "err_blank_line": ("o2.gff: line 2", "fewer than 3"), "err_cds_8_fields": ("o2.gff: line 1", "fewer than 9"),
            "err_attribute": ("o2.gff: line 1", "key=value"), "err_attribute_two_eq": ("o2.gff: line 1", "key=value"),
            "err_attribute_blank": ("o2.gff: line 1", "key=value"), "err_no_id": ("o2.gff: line 1", "ID"),
            "err_start": ("o2.gff: line 1", "START"), "err_end": ("o2.gff: line 1", "END"),
            "err_dup_organism": ("o1", "Redondant"), "err_circular_unsized": ("c1", "sequence-region"),
            "err_first": ("o1.gff: line 2", "START")}


def test_the_recorded_cases_are_there():
    assert len(GOOD) >= 9 and len(BAD) >= 13 and set(MESSAGES) == {case_id(p) for p in BAD}


@pytest.mark.parametrize("path", GOOD, ids=case_id)
def test_statement_equals_reference(path):
    rec = recorded(path)
    ld = loader.load_arrays_host(*paths(path), **rec["args"])
    equals_recording(ld, rec, rec["name"])
    one = loader.load_arrays_host(*paths(path), batch_bytes=1, **rec["args"])      # a file per batch
    same_loaded(one, ld, rec["name"] + ": a file per batch")


@pytest.mark.parametrize("path", BAD, ids=case_id)
def test_statement_refuses_what_the_reference_refuses(path):
    rec = recorded(path)
    for batch_bytes in (256 << 20, 1):
        got = error_of(lambda: loader.load_arrays_host(*paths(path), batch_bytes=batch_bytes, **rec["args"]))
        assert got is not None and got[0] is RAISES[rec["raises"]], (rec["name"], got)
        for part in MESSAGES[rec["name"]]:
            assert part in got[1], (rec["name"], got[1])


def test_open_files_and_gzip_streams(tmp_path):
    path = [p for p in GOOD if case_id(p) == "gz"][0]
    rec = recorded(path)
    with open(paths(path)[0]) as orgs, open(paths(path)[1], "rb") as fams:
        equals_recording(loader.load_arrays_host(orgs, fams, **rec["args"]), rec, "open files")


def test_duplicate_id_within_an_organism_is_refused(tmp_path):
    gffs = [b"\n".join([cds_line(b"c1", 1, b"a"), cds_line(b"c2", 5, b"b"), cds_line(b"c2", 9, b"a"), cds_line(b"c1", 3, b"a")]) + b"\n",
            cds_line(b"c1", 1, b"a") + b"\n"]
    orgs, fams = write_set(tmp_path, gffs, b"F a b\n")
    got = error_of(lambda: loader.load_arrays_host(orgs, fams))
    assert got[0] is ValueError and "o0.gff: line 3" in got[1] and "'a'" in got[1], got
    orgs, fams = write_set(tmp_path / "ok", [gffs[1], gffs[1]], b"F a b\n")          # the same ID in two organisms is fine
    assert loader.load_arrays_host(orgs, fams).orders["genes"].tolist() == [0, 0]


def test_numbers_python_would_take_are_refused(tmp_path):
    for k, tok in enumerate((b"1_000", "١".encode(), b"2147483648", b"-2147483649", b"+", b"1 2")):
        line = cds_line(b"c", 1, b"a").replace(b"\t1\t", b"\t" + tok + b"\t")
        orgs, fams = write_set(tmp_path / str(k), [line], b"F a\n")
        got = error_of(lambda: loader.load_arrays_host(orgs, fams))
        assert got is not None and got[0] is ValueError and "line 1" in got[1] and "START" in got[1], (tok, got)
    orgs, fams = write_set(tmp_path / "edge", [cds_line(b"c", 1, b"a").replace(b"\t1\t51\t", b"\t-2147483648\t+2147483647\t")], b"F a\n")
    ld = loader.load_arrays_host(orgs, fams)
    assert ld.orders["starts"].tolist() == [-2147483648] and ld.orders["ends"].tolist() == [2147483647]
    assert ld.orders["lengths"].dtype == np.int32


def test_high_bytes_are_token_bytes(tmp_path):
    gene = "g \u0085x".encode()                                               # NBSP and NEL: whitespace to str, bytes here
    orgs, fams = write_set(tmp_path, [cds_line(b"c", 1, gene)], b"F " + gene + b"\n")
    ld = loader.load_arrays_host(orgs, fams)
    assert list(ld.gene_ids) == [gene.decode()] and ld.families == ["F"]


def test_generator_round_trip(tmp_path):
    orgs, fams, size = loader.synth_files(str(tmp_path), [[1, 5, 0, 3], [], [70]], n_families=7, seed=3)
    ld = loader.load_arrays_host(orgs, fams, lim_occurence=2)
    assert size == sum(os.path.getsize(os.path.join(str(tmp_path), "o%d.gff" % o)) for o in range(3))
    assert np.diff(ld.orders["contig_ptr"]).tolist() == [1, 5, 3, 70] and ld.orders["contig_org"].tolist() == [0, 0, 0, 2]
    for c in range(4):
        s = ld.orders["starts"][ld.orders["contig_ptr"][c]:ld.orders["contig_ptr"][c + 1]]
        assert np.all(np.diff(s) >= 0)
    assert ld.families_repeted


def test_a_missing_file_waits_for_the_errors_before_it(tmp_path):
    orgs, fams = write_set(tmp_path, [cds_line(b"c", 1, b"a") + b"\n", b"c\tshort\n", b""], b"F a\n")
    os.remove(os.path.join(str(tmp_path), "o2.gff"))
    for batch_bytes in (1, 256 << 20):
        got = error_of(lambda: loader.load_arrays_host(orgs, fams, batch_bytes=batch_bytes))
        assert got[0] is ValueError and "o1.gff: line 1" in got[1], got
    orgs, fams = write_set(tmp_path / "b", [cds_line(b"c", 1, b"a") + b"\n", b""], b"F a\n")
    os.remove(os.path.join(str(tmp_path / "b"), "o1.gff"))
    assert error_of(lambda: loader.load_arrays_host(orgs, fams))[0] is FileNotFoundError
