#!/usr/bin/env python3
"""Generate tests/golden/layout/: what the REAL `export_to_GEXF()` (ppanggolin/ppanggolin.py:1294-1362) and networkx's
write_gexf write, full and light, for three of make_gexf.py's cases after the real body of `compute_layout`
(:1285-1292) has put `viz:position` on every node.

`compute_layout` delegates to the external package fa2, which is not part of the reference tree: what it would compute
is not the reference's.  What IS the reference's -- `z` from the partition and the dict that networkx writes as
`<viz:position>` -- is executed as it stands: lines 1285-1292 are read from the reference's file and run with a stand-in
`forceatlas2` whose `forceatlas2_networkx_layout` returns the positions listed in the case (negative values, 3.0, 1e-05,
a 17-digit value among them), as fa2 returns them: {node: (x, y)}.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- the
case's name (its annotations are tests/golden/gexf/<name>.json's), the families in node order with their positions, the
labelling and the text of the two files.  tests/test_layout_host.py and tests/test_gpu_layout.py read it.

    python tests/golden/make_layout.py
"""
import json
import os
import shutil
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_gexf  # noqa: E402
from make_orders import reference_class  # noqa: E402

OUT = os.path.join(HERE, "layout")
CASES = ("links", "duplicates", "repeated_late")
SPECIAL = (-1234.5, 3.0, 1e-05, 0.10000000000000002, -0.0, 1e+22, -7.062513305931046e-15, 123456789.12345679, 0.0, 2.5e-310)


def positions_for(k):
    """node k's (x, y): the special values walked at two strides, so every one appears as an x and as a y"""
    return SPECIAL[k % len(SPECIAL)], SPECIAL[(3 * k + 1) % len(SPECIAL)]


class StandIn:
    """fa2.ForceAtlas2 as compute_layout uses it (:1285): the listed positions, a tuple per node"""

    def __init__(self):
        self.nodes = None

    def forceatlas2_networkx_layout(self, G, pos=None, iterations=100):
        assert pos is None and iterations == 500
        self.nodes = list(G.nodes())
        return {node: positions_for(k) for k, node in enumerate(self.nodes)}


def laid_out(PPanGGOLiN, stand_in):
    """the class with an export_to_GEXF that first runs compute_layout's own loop (:1285-1292), once"""
    import ppanggolin.ppanggolin as module
    with open(module.__file__) as f:
        lines = f.read().splitlines()[1284:1292]
    assert "forceatlas2_networkx_layout" in lines[0] and "['position']" in lines[-1]
    body = textwrap.dedent("\n".join(lines))
    real = PPanGGOLiN.export_to_GEXF

    class Laid(PPanGGOLiN):
        def export_to_GEXF(self, path, **kw):
            if stand_in.nodes is None:
                exec(body, dict(self=self, G=self.neighbors_graph, forceatlas2=stand_in, iterations=500))
            return real(self, path, **kw)

    return Laid


def main():
    PPanGGOLiN = reference_class()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for cs in make_gexf.cases():
        if cs["name"] not in CASES:
            continue
        stand_in = StandIn()
        rec = make_gexf.run(laid_out(PPanGGOLiN, stand_in), cs)
        assert "<viz:position" in rec["gexf"] and "<viz:position" in rec["gexf_light"]
        out = dict(name=rec["name"], families=stand_in.nodes, positions=[list(positions_for(k)) for k in range(len(stand_in.nodes))],
                   labels=rec["labels"], gexf=rec["gexf"], gexf_light=rec["gexf_light"])
        with open(os.path.join(OUT, cs["name"] + ".json"), "w") as f:
            json.dump(out, f, indent=0, sort_keys=False)
            f.write("\n")
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
