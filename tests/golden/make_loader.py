#!/usr/bin/env python3
"""Generate tests/golden/loader/: what the REAL `__initialize_from_files` (ppanggolin/ppanggolin.py:180-315, with its own
`__load_gff`) makes of a few small sets of files.

Runs only where the reference tree exists; nothing of the reference travels: what is stored is data -- per case a
directory with the input files (organisms.tsv, families.tsv, the GFFs) and expected.json: the arguments and either the
recorded annotations ({organism: {contig: [[gene, info], ...]}} in dict order), circular_contig_size, families_repeted
(sorted) and organisms, or the type of the exception the reference raised.  tests/test_loader_host.py and
tests/test_gpu_loader.py read it.

The reference is run as make_orders.py runs it (stand-in modules for the third-party imports the loader never uses, an
OrderedSet with `add`, a tqdm that only iterates); a PPanGGOLiN object is made without its __init__ and given the
attributes the method reads.  The working directory is the case's, as the organisms file names the GFFs relatively.

    python tests/golden/make_loader.py
"""
import gzip
import json
import os
import shutil
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loader")


class OrderedSet(list):
    """stands in for ordered_set.OrderedSet"""

    def add(self, item):
        if item not in self:
            self.append(item)


def reference_class():
    for name, attr in (("bidict", "bidict"), ("fa2", "ForceAtlas2"), ("highcharts", "Highchart")):
        stub = types.ModuleType(name)
        setattr(stub, attr, type(attr, (), {}))
        sys.modules[name] = stub
    osm = types.ModuleType("ordered_set")
    osm.OrderedSet = OrderedSet
    sys.modules["ordered_set"] = osm
    nem = types.ModuleType("nem")
    nem.__all__ = []
    sys.modules["nem"] = nem

    class Bar:
        def __init__(self, it, **kw):
            self.it = it

        def __iter__(self):
            return iter(self.it)

        def set_description(self, *a):
            pass

        def refresh(self):
            pass

    tq = types.ModuleType("tqdm")
    tq.tqdm = Bar
    sys.modules["tqdm"] = tq
    sys.dont_write_bytecode = True
    sys.path.insert(0, "/root/reference")
    import ppanggolin.ppanggolin as mod
    mod.get_num_lines = lambda f: 0
    return mod.PPanGGOLiN


def cds(contig, start, end, attrs, strand="+", feature="CDS"):
    return "\t".join([contig, "src", feature, str(start), str(end), ".", strand, "0", attrs])


def cases():
    out = []
    simple = lambda c, ids, s0=1: [cds(c, s0 + 100 * k, s0 + 100 * k + 90, "ID=%s;Name=n_%s;product=p %s" % (g, g, g)) for k, g in enumerate(ids)]
    out.append(dict(name="newlines", args=dict(lim_occurence=0, infer_singletons=False), files={
        "organisms.tsv": "o1\to1.gff\r\no2\to2.gff\no3\to3.gff",
        "families.tsv": "FA a1 a2 a3\nFB\tb1\tb2\r\nFC c1 c3\rFD d3",
        "o1.gff": "##gff-version 3\r\n" + "\r\n".join(simple("c1", ["a1", "b1", "c1"])) + "\r\n",
        "o2.gff": "##gff-version 3\r" + "\r".join(simple("c1", ["b2", "a2"])) + "\r",
        "o3.gff": "\n".join(simple("c1", ["a3", "c3"]) + simple("c2", ["d3"]))}))
    out.append(dict(name="fasta_pragma", args=dict(lim_occurence=0, infer_singletons=False), files={
        "organisms.tsv": "o1\to1.gff\tcircA\tcircB\no2\to2.gff\tcircC\n",
        "families.tsv": "FA a1 a2\nFB b1 b2\nFC c1\n",
        "o1.gff": "\n".join(["##gff-version 3", "##sequence-region circA 1 1000", "##sequence-region other 1 77", "#c\tx\ty",
                             "# a comment\twith\tCDS in the wrong field\t1\t2", "circA\tsrc\tgene\t1\t90\t.\t+\t0\tID=gene1"] +
                            simple("circA", ["a1", "b1"]) + simple("lin", ["c1"]) +
                            ["##sequence-region circA 1 5000", "##sequence-region circC 1 42", "##FASTA", ">circA", "ACGT\tACGT",
                             cds("circA", 7, 8, "ID=never"), "##sequence-region circA 1 9"]) + "\n",
        "o2.gff": "\n".join(simple("circB", ["a2"]) + simple("circC", ["b2"]) +
                            ["##sequence-region circB 1 2000", "##sequence-regionX circC 5 3000 extra"]) + "\n"}))
    out.append(dict(name="attributes", args=dict(lim_occurence=0, infer_singletons=False), files={
        "organisms.tsv": " o1 \t o1.gff \n",
        "families.tsv": "FA a1 a2 a3 a4 a5 a6\n",
        "o1.gff": "\n".join([
            cds("c1", 1, 90, "id=a1;NaMe=nm;gene=gn;Product=the product"),
            cds("c1", 100, 190, "ID=a2;gene=only gene;;"),
            cds("c1", 200, 290, "ID=wrong;ID=a3;name=first;Name=second;note=x;;"),
            " c1 \tsrc\t CDS \t 300\t390 \t.\t + \t0\t ID=a4; product= padded value ;Name=n4 ",
            cds("c1", 400, 490, "Parent=p;ID=a5"),
            cds("c1", "+500", "-5", "ID=a6;name=;product=", strand=""),
            "c2\tsrc\tcds\t1\t2\t.\t+\t0\tnot parsed",
        ]) + "\n"}))
    out.append(dict(name="families", args=dict(lim_occurence=0, infer_singletons=True), files={
        "organisms.tsv": "o1\to1.gff\no2\to2.gff\n",
        "families.tsv": "FA a1 a2 moved\nFB b1 moved\n\nFC\nFB b2\nFD\x0bd1\x1cd2\n",
        "o1.gff": "\n".join(simple("c1", ["s1", "a1", "moved", "FA", "b1", "d1"])) + "\n",
        "o2.gff": "\n".join(simple("c1", ["FA", "s1", "b2", "FC", "s2", "d2", "a2"])) + "\n"}))
    out.append(dict(name="order", args=dict(lim_occurence=0, infer_singletons=False), files={
        "organisms.tsv": "o1\to1.gff\nempty\tempty.gff\nnocds\tnocds.gff\no4\to4.gff\n",
        "families.tsv": "FA a1 a2 a3 a4 a5\nFB b1 b2 b3 b4\nFC c1 c2 c3\n",
        "o1.gff": "\n".join([cds("c1", 500, 600, "ID=a1"), cds("c2", 50, 60, "ID=b1"), cds("c1", 400, 450, "ID=c1"), cds("c1", 400, 420, "ID=b2"),
                             cds("c3", 9, 10, "ID=a2"), cds("c1", 300, 310, "ID=a3"), cds("c2", 50, 55, "ID=c2"), cds("c1", 400, 401, "ID=b3"),
                             cds("c2", -5, 5, "ID=a4")]) + "\n",
        "empty.gff": "",
        "nocds.gff": "##gff-version 3\nc1\tsrc\tgene\t1\t2\t.\t+\t0\tID=x\n",
        "o4.gff": "\n".join([cds("c1", 3, 4, "ID=c3"), cds("c1", 2, 4, "ID=b4"), cds("c1", 1, 4, "ID=a5")]) + "\n"}))
    lim_files = {
        "organisms.tsv": "o1\to1.gff\no2\to2.gff\n",
        "families.tsv": "FA a1 a2 a3 a4\nFB b1 b2 b3\nFC c1 c2 c3 c4\nFD d1 d2\n",
        "o1.gff": "\n".join(simple("c1", ["a1", "b1", "a2", "d1", "b2", "c1", "b3", "c2"])) + "\n",
        "o2.gff": "\n".join(simple("c1", ["a3", "c3", "d2", "a4", "c4"])) + "\n"}
    out.append(dict(name="lim2", args=dict(lim_occurence=2, infer_singletons=False), files=lim_files))
    out.append(dict(name="lim1", args=dict(lim_occurence=1, infer_singletons=False), files=lim_files))
    out.append(dict(name="lim3", args=dict(lim_occurence=3, infer_singletons=False), files=lim_files))
    out.append(dict(name="gz", args=dict(lim_occurence=0, infer_singletons=False), gz=["o1.gff", "families.tsv"], files={
        "organisms.tsv": "o1\to1.gff\no2\to2.gff\n",
        "families.tsv": "FA a1 a2\nFB b1 b2\n",
        "o1.gff": "\n".join(simple("c1", ["a1", "b1"])) + "\n",
        "o2.gff": "\n".join(simple("c1", ["b2", "a2"])) + "\n"}))
    # ---- the reference raises
    one = lambda gff, fam="FA a1 a2\n", org="o1\to1.gff\no2\to2.gff\n", **args: dict(
        args=dict(dict(lim_occurence=0, infer_singletons=False), **args),
        files={"organisms.tsv": org, "families.tsv": fam, "o1.gff": "\n".join(simple("c1", ["a1"])) + "\n", "o2.gff": gff})
    out.append(dict(name="err_unknown", **one("\n".join(simple("c1", ["a2", "zz"])) + "\n")))
    out.append(dict(name="err_short_line", **one(cds("c1", 1, 2, "ID=a2") + "\nc1\tonly two\n")))
    out.append(dict(name="err_blank_line", **one(cds("c1", 1, 2, "ID=a2") + "\n\n")))
    out.append(dict(name="err_cds_8_fields", **one("c1\tsrc\tCDS\t1\t2\t.\t+\t0\n")))
    out.append(dict(name="err_attribute", **one(cds("c1", 1, 2, "ID=a2;flag") + "\n")))
    out.append(dict(name="err_attribute_two_eq", **one(cds("c1", 1, 2, "ID=a2;note=a=b") + "\n")))
    out.append(dict(name="err_attribute_blank", **one(cds("c1", 1, 2, "ID=a2; ;") + "\n")))
    out.append(dict(name="err_no_id", **one(cds("c1", 1, 2, "Name=a2") + "\n")))
    out.append(dict(name="err_start", **one(cds("c1", "1.5", 2, "ID=a2") + "\n")))
    out.append(dict(name="err_end", **one(cds("c1", 1, "", "ID=a2") + "\n")))
    out.append(dict(name="err_dup_organism", **one(cds("c1", 1, 2, "ID=a2") + "\n", org="o1\to1.gff\no1\to2.gff\n")))
    out.append(dict(name="err_circular_unsized", **one(cds("c1", 1, 2, "ID=a2") + "\n", org="o1\to1.gff\tc1\no2\to2.gff\n")))
    # the first error in (organism, line) order: a bad START in o1 line 2 precedes an unknown gene in o1 line 3 and o2's
    c = one("c1\tshort\n")
    c["files"]["o1.gff"] = "\n".join([cds("c1", 1, 2, "ID=a1"), cds("c1", "x", 2, "ID=a2"), cds("c1", 1, 2, "ID=zz")]) + "\n"
    out.append(dict(name="err_first", **c))
    return out


def run(PPanGGOLiN, directory, args):
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    obj.annotations, obj.organisms, obj.circular_contig_size, obj.families_repeted = dict(), OrderedSet(), dict(), set()
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        with open("organisms.tsv") as orgs, open("families.tsv") as fams:
            try:
                obj._PPanGGOLiN__initialize_from_files(orgs, fams, args["lim_occurence"], args["infer_singletons"])
            except BaseException as e:                    # (exit() where a circular contig has no size)
                return dict(raises=type(e).__name__)
    finally:
        os.chdir(cwd)
    return dict(raises=None, organisms=list(obj.organisms), circular_contig_size=obj.circular_contig_size,
                families_repeted=sorted(obj.families_repeted),
                annotations=[[org, [[contig, [[gene, info] for gene, info in annot.items()]] for contig, annot in contigs.items()]]
                             for org, contigs in obj.annotations.items()])


def main():
    PPanGGOLiN = reference_class()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    for cs in cases():
        d = os.path.join(OUT, cs["name"])
        os.makedirs(d)
        for name, text in cs["files"].items():
            data = text.encode()
            if name in cs.get("gz", ()):
                data = gzip.compress(data, mtime=0)
            with open(os.path.join(d, name), "wb") as f:
                f.write(data)
        rec = dict(name=cs["name"], args=cs["args"], **run(PPanGGOLiN, d, cs["args"]))
        with open(os.path.join(d, "expected.json"), "w") as f:
            json.dump(rec, f, indent=0)
            f.write("\n")
        print(cs["name"], rec["raises"] or "ok")


if __name__ == "__main__":
    main()
