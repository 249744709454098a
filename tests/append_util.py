"""What tests/test_master_append_host.py and tests/test_gpu_master_append.py share: the recorded graphs of
tests/golden/orders_update/ (made by tests/golden/make_orders_update.py from the reference's own add_organism), the
orders of a base and of its updates in one id space, and slices of flat orders by organism."""
import glob
import os
from collections import OrderedDict

import numpy as np

from pangenomenem_amd.chunks import master_arrays_append_orders, master_arrays_from_orders, orders_from_annotations
from tests.orders_util import load

UPDATE_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orders_update", "*.json")))


def lists_to_annotations(lists):
    return OrderedDict((org, OrderedDict((contig, OrderedDict((gene, ["CDS", fam]) for gene, fam in genes)) for contig, genes in contigs))
                       for org, contigs in lists)


def fixture_parts(rec):
    """(base orders, update orders): the update's in the base's id space grown, its columns behind the base's, circular
    contigs and repeated families the unions add_organism leaves"""
    base = orders_from_annotations(lists_to_annotations(rec["annotations"]), rec["organisms"], rec["circular"], rec["repeated"])
    upd = orders_from_annotations(lists_to_annotations(rec["update_annotations"]), rec["organisms"] + rec["new_organisms"],
                                  set(rec["circular"]) | set(rec["update_circular"]), set(rec["repeated"]) | set(rec["update_repeated"]),
                                  families=base["families"])
    return base, upd


def build_host(o):
    return master_arrays_from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"])


def append_host(master, f_old, upd, d_new):
    """master: what build_host / append_host returned"""
    return master_arrays_append_orders(master, master[4], f_old, upd["genes"], upd["contig_ptr"], upd["contig_org"], upd["contig_circular"],
                                       d_new, repeated=upd["repeated"])


def split_annotations(ann, orgs, cuts):
    """the walk of ann cut into len(cuts) + 1 parts (cuts: organisms walked before each cut); the columns: every part's
    organisms in orgs' order, part after part (inside a part walk order is not column order).  Returns parts, columns."""
    walk = list(ann.items())
    bounds = [0] + list(cuts) + [len(walk)]
    parts = [OrderedDict(walk[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    cols = [o for part in parts for o in orgs if o in part]
    return parts, cols


def part_orders(parts, cols, circular, repeated):
    """every part's orders in one id space (a part numbers on from the parts before it), its columns absolute; and the
    orders of all parts at once"""
    out, fams, d = [], [], 0
    for part in parts:
        d += len(part)
        o = orders_from_annotations(part, cols[:d] if not out else cols, circular, repeated, families=fams)
        fams = o["families"]
        out.append(o)
    whole = orders_from_annotations(OrderedDict((k, v) for part in parts for k, v in part.items()), cols, circular, repeated)
    return out, whole


def slice_orders(o, lo, hi):
    """the contigs of organisms lo .. hi - 1 of flat orders whose organisms are walked in column order (synthetic_orders)"""
    sel = np.flatnonzero((o["contig_org"] >= lo) & (o["contig_org"] < hi))
    a, b = sel[0], sel[-1] + 1
    g0, g1 = o["contig_ptr"][a], o["contig_ptr"][b]
    return dict(genes=o["genes"][g0:g1], contig_ptr=(o["contig_ptr"][a:b + 1] - g0).astype(np.int32), contig_org=o["contig_org"][a:b],
                contig_circular=o["contig_circular"][a:b], repeated=o["repeated"])
