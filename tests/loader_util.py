"""What tests/test_loader_host.py and tests/test_gpu_loader.py share: the recorded loader fixtures
(tests/golden/loader/, written by tests/golden/make_loader.py), the comparison of a Loaded with a recording and of two
Loaded with each other, and the sets of files the device tests are sized around."""
import glob
import json
import os
from collections import OrderedDict

import numpy as np

from pangenomenem_amd.chunks import orders_from_annotations

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(os.path.dirname(p) for p in glob.glob(os.path.join(HERE, "golden", "loader", "*", "expected.json")))
ORDER_KEYS = ("genes", "contig_ptr", "contig_org", "contig_circular", "repeated")
# the reference's exception -> ours (an IndexError or an exit() of the reference is a ValueError that names the place)
RAISES = {"KeyError": KeyError, "IndexError": ValueError, "ValueError": ValueError, "SystemExit": ValueError}


def case_id(path):
    return os.path.basename(path)


def recorded(path):
    with open(os.path.join(path, "expected.json")) as f:
        return json.load(f)


def paths(path):
    return os.path.join(path, "organisms.tsv"), os.path.join(path, "families.tsv")


def annotations_of(rec):
    return OrderedDict((org, OrderedDict((contig, OrderedDict((gene, info) for gene, info in genes)) for contig, genes in contigs))
                       for org, contigs in rec["annotations"])


def nested_lists(ann):
    """annotations with their dict orders made explicit"""
    return [[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in contigs.items()]] for org, contigs in ann.items()]


def equals_recording(ld, rec, what):
    """the contract: annotations (dict orders included), circular sizes, repeated families and organisms are the
    reference's, and orders is orders_from_annotations of the reference's output, array for array"""
    assert list(ld.organisms) == rec["organisms"], what
    assert nested_lists(ld.annotations()) == rec["annotations"], what + ": annotations"
    assert ld.circular_contig_size == rec["circular_contig_size"], what + ": circular_contig_size"
    assert list(ld.circular_contig_size) == list(rec["circular_contig_size"]), what + ": circular_contig_size order"
    assert sorted(ld.families_repeted) == rec["families_repeted"], what + ": families_repeted"
    want = orders_from_annotations(annotations_of(rec), rec["organisms"], rec["circular_contig_size"], rec["families_repeted"])
    for k in ORDER_KEYS:
        assert ld.orders[k].dtype == want[k].dtype and np.array_equal(ld.orders[k], want[k]), what + ": orders[%s]" % k
    assert ld.orders["d"] == want["d"] and ld.orders["families"] == want["families"] and ld.orders["organisms"] == want["organisms"], what
    assert ld.families == want["families"], what
    infos = [info for _, contigs in rec["annotations"] for _, genes in contigs for _, info in genes]
    assert ld.orders["starts"].tolist() == [i[2] for i in infos] and ld.orders["ends"].tolist() == [i[3] for i in infos], what
    assert ld.orders["lengths"].tolist() == [i[3] - i[2] for i in infos], what
    assert ld.orders["strand"].tolist() == [ord(i[4][0]) if i[4] else 0 for i in infos] and ld.orders["strand"].dtype == np.uint8, what
    cnames = [contig for _, contigs in rec["annotations"] for contig, _ in contigs]
    assert list(ld.contig_names) == cnames, what
    assert ld.orders["contig_sizes"].tolist() == [rec["circular_contig_size"].get(c, -1) for c in cnames], what
    for k in ("starts", "ends", "lengths", "contig_sizes"):
        assert ld.orders[k].dtype == np.int32, what
    assert list(ld.gene_ids) == [gene for _, contigs in rec["annotations"] for _, genes in contigs for gene, _ in genes], what
    assert list(ld.gene_names) == [i[5] for i in infos] and list(ld.products) == [i[6] for i in infos], what


def same_loaded(got, want, what):
    """two loads, array for array and span for span"""
    a, b = got.arrays(), want.arrays()
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), what + ": " + k
    assert got.organisms == want.organisms and got.families == want.families, what
    assert got.families_repeted == want.families_repeted and got.circular_contig_size == want.circular_contig_size, what
    assert list(got.circular_contig_size) == list(want.circular_contig_size), what


def error_of(call):
    """(type, message) of what the call raises, None if it returns"""
    try:
        call()
    except Exception as e:                                # noqa: BLE001
        return type(e), str(e)
    return None


def write_set(directory, gffs, families, circular=None):
    """files of given bytes: gffs = [bytes per organism]; returns (organisms file, families file)"""
    os.makedirs(str(directory), exist_ok=True)
    lines = []
    for o, data in enumerate(gffs):
        with open(os.path.join(str(directory), "o%d.gff" % o), "wb") as f:
            f.write(data)
        lines.append("\t".join(["o%d" % o, "o%d.gff" % o] + list((circular or {}).get(o, ()))))
    orgs, fams = os.path.join(str(directory), "organisms.tsv"), os.path.join(str(directory), "families.tsv")
    with open(orgs, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(fams, "wb") as f:
        f.write(families)
    return orgs, fams


def cds_line(contig, start, gene, pad=b""):
    return b"\t".join([contig, b"t", b"CDS", b"%d" % start, b"%d" % (start + 50), b".", b"+", b"0", b"ID=" + gene + b";Name=n" + pad])
