"""partition_shell in numpy and Python (pangenomenem_amd/shell.py, gexf.write_gexf(subpartition=)) against what the
reference's own writer, its own partition_shell() and export_to_GEXF() and the compiled reference's random starts did on
the pangenomes of tests/golden/partition_shell/ (made by tests/golden/make_partition_shell.py)."""
from collections import Counter

import numpy as np
import pytest

from pangenomenem_amd.gexf import write_gexf
from pangenomenem_amd.projection import shell_q_auto
from pangenomenem_amd.shell import (LONG, form_subproblem_host, mf_parameters, mf_value, outside_entry_host, resolve_q, shell_init_params,
                                    shell_labels, uf_classes)
from tests.gexf_util import GEXF_FIXTURES, host_tables, same_gexf_text
from tests.orders_util import load as load_json
from tests.partition_shell_util import (REF_QS, REF_SEED, SHELL_FIXTURES, SHELL_IDS, TOL, host_problem, init_of, load, nei_sets, parse_files,
                                        parse_m, synthetic_master)
from tests.util import maxdiff


def same_as_files(rec, problem, files, what, node_order=True):
    """node_order False: the families by name.  The filtered writer keeps the graph's node order (:843-844); a networkx
    subgraph view iterates whichever is smaller, the graph's nodes or the SET it was given, that one in hash order, so
    the unfiltered writer on subgraph(shell) numbers a small shell differently -- the same problem, renumbered"""
    x, (ptr, idx, w), fam = problem
    index, dat, nei, shape = parse_files(files)
    mine = [rec["names"][i] for i in fam]
    assert shape == (len(fam), len(rec["everyone"])), what
    assert (mine == index) if node_order else (sorted(mine) == sorted(index) and len(set(index)) == len(index)), what
    got = nei_sets(ptr, idx, w)
    for j, name in enumerate(mine):
        r = index.index(name)
        assert np.array_equal(x[j], dat[r]), (what, name)
        assert Counter({(mine[b - 1], wt): c for (b, wt), c in got[j + 1].items()}) == Counter({(index[b - 1], wt): c for (b, wt), c in nei[r + 1].items()}), (what, name)


def test_fixtures_cover_the_cases():
    recs = {name: load(p) for name, p in zip(SHELL_IDS, SHELL_FIXTURES)}
    assert set(recs) == {"closed", "open", "outside_only", "selfloop", "twice", "circular", "grown", "noshell"}
    for name, rec in recs.items():
        assert 6 <= len(rec["everyone"]) <= 12 and 12 <= len(rec["names"]) <= 48, name
        assert ("error" in rec["writer"]) == (name in ("open", "outside_only")), name
    assert recs["grown"]["new_organisms"] and not recs["noshell"]["select"].any()
    # a shell family all of whose neighbours are outside: degree 0 in the induced graph, neighbours in the master
    rec = recs["outside_only"]
    m = rec["master"]
    i = rec["names"].index("SX")
    assert m[1][0][i + 1] > m[1][0][i] and not rec["select"][m[1][1][m[1][0][i]:m[1][0][i + 1]]].any()
    _, (ptr, _, _), fam = host_problem(rec)
    j = fam.tolist().index(i)
    assert ptr[j + 1] == ptr[j]
    for name, twice in (("selfloop", False), ("twice", True)):
        _, (ptr, idx, w), _ = host_problem(recs[name])
        rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        assert (rows == idx).any() or twice, name            # a self-loop is a neighbour like any other
        assert (w >= 2).any(), name
    assert recs["circular"]["circular"]


@pytest.mark.parametrize("path", SHELL_FIXTURES, ids=SHELL_IDS)
def test_the_two_edge_rules_equal_the_writers_files(path):
    rec = load(path)
    same_as_files(rec, host_problem(rec, "induced"), rec["induced"]["files"], rec["name"] + " induced", node_order=False)
    if "error" in rec["writer"]:
        kind, args = rec["writer"]["error"]
        assert kind == "KeyError"
        with pytest.raises(KeyError) as err:
            host_problem(rec, "reference")
        # the reference walks a set of neighbours: which outside neighbour it trips on first is its hash order's; ours
        # is the first in the master's row.  Both are neighbours of a shell family and not shell
        m = rec["master"]
        mine = rec["names"][err.value.args[0]]
        for culprit in (mine, args[0]):
            assert rec["labels"][culprit] != "S"
            i = rec["names"].index(culprit)
            assert rec["select"][m[1][1][m[1][0][i]:m[1][0][i + 1]]].any()
        assert err.value.args[0] == m[1][1][outside_entry_host(m[0], m[1][0], m[1][1], m[2], np.arange(m[0].shape[1]), rec["select"], m[3])]
    else:
        problem = host_problem(rec, "reference")
        same_as_files(rec, problem, rec["writer"]["files"], rec["name"] + " reference")
        assert len(problem[1][1]) == 0
        m = rec["master"]
        assert outside_entry_host(m[0], m[1][0], m[1][1], m[2], np.arange(m[0].shape[1]), rec["select"], m[3]) == -1


def test_an_organism_subset_drops_families_and_edges():
    x, ptr, idx, eb, counts = synthetic_master(90, 12, 5, loops=True, extras=(1, 3))
    select = np.arange(90) % 3 != 0
    orgs = [7, 2, 9]
    xs, (p, i, w), fam = form_subproblem_host(x, ptr, idx, eb, orgs, select, counts)
    keep = select & x[:, orgs].any(axis=1)
    assert np.array_equal(fam, np.flatnonzero(keep)) and 0 < len(fam) < select.sum()
    assert np.array_equal(xs, x[fam][:, orgs])
    # every kept edge: between kept families, its weight the counts over the subset (a plain walk)
    renum = {int(f): j for j, f in enumerate(fam)}
    for j, f in enumerate(fam):
        want = []
        for e in range(ptr[f], ptr[f + 1]):
            bits = np.unpackbits(eb[e].view(np.uint8), bitorder="little")
            c = sum(int(bits[o]) for o in orgs)
            for t in range(counts[0][e], counts[0][e + 1]):
                if counts[1][t] in orgs:
                    c += int(counts[2][t]) - 1
            if c > 0 and int(idx[e]) in renum:
                want.append((renum[int(idx[e])], float(c)))
        assert list(zip(i[p[j]:p[j + 1]].tolist(), w[p[j]:p[j + 1]].tolist())) == want
    with pytest.raises(ValueError):
        form_subproblem_host(x, ptr, idx, eb, orgs, select[:-1], counts)
    with pytest.raises(ValueError):
        form_subproblem_host(x, ptr, idx, eb, orgs, select, counts, edges="both")


@pytest.mark.parametrize("name", ["closed", "circular"])
def test_init_params_equal_the_recorded_m(name):
    rec = load(SHELL_FIXTURES[SHELL_IDS.index(name)])
    d = len(rec["everyone"])
    for key, Q in (("dict", 4), ("list", 3)):
        init = init_of({key: rec["m_inits"][key]})
        head, center, disp = parse_m(rec["m_" + key], Q, d)
        prop, c, e = shell_init_params(init, rec["everyone"])
        assert prop.dtype == c.dtype == e.dtype == np.float32 and len(prop) == Q
        assert np.array_equal(prop[:-1], np.asarray(head, np.float32)), key
        rem = np.float32(1.0)
        for v in head:
            rem = np.float32(rem - np.float32(v))
        assert prop[-1] == rem and rem > 0
        assert np.array_equal(c, center) and np.array_equal(e, disp), key
        assert (c == 0.5).any() and (e == 0.5).any()         # (an organism in no group)


def test_init_params_refuse_what_nem_refuses():
    orgs = ["o%d" % i for i in range(8)]
    for groups in (2, 4, 6, 7, 8):                            # 1 - len x round(1 / len, 4) in float32, term by term: nothing is left
        init = {"g%d" % g: {orgs[g]} for g in range(groups)}
        with pytest.raises(ValueError, match="proportion"):
            shell_init_params(init, orgs)
    assert shell_init_params({"a": {"o0"}, "b": {"o1"}, "c": {"o2"}}, orgs)[0][-1] == np.float32(1.0) - np.float32(0.3333) - np.float32(0.3333) - np.float32(0.3333)
    # five groups: 1 - 0.2 - 0.2 - 0.2 - 0.2 - 0.2 is one rounding above zero in float32, and ReadParamFile accepts it
    assert shell_init_params({"g%d" % g: {orgs[g]} for g in range(5)}, orgs)[0][-1] == np.float32(2.9802322e-08)
    with pytest.raises(ValueError):
        shell_init_params("default", orgs)


def test_mf_rounding():
    # "%5.3g" of the proportion, "%10g" of a dispersion, "%10.3g" of a centre and then its truth (nem_io.cpp:523-526)
    assert mf_value(np.float32(0.33333334), "%5.3g") == 0.333 and mf_value(np.float32(1.0) / 7, "%5.3g") == 0.143
    assert mf_value(np.float32(0.123456789), "%10g") == 0.123457 and mf_value(np.float32(1e-7), "%10g") == 1e-07
    assert mf_value(np.float32(0.0004), "%10.3g") == 0.0004
    res = dict(status=0, center=np.asarray([[1, 0, 0.5], [0, 0, 1e-30]], np.float32), disp=np.asarray([[0.1, 0.1, 0.1], [1 / 3, 0.25, 0.0999999]], np.float32),
               prop=np.asarray([0.66666, 0.33334], np.float32))
    p = mf_parameters(res, 2)
    assert p[0] == ([True, False, True], [0.1, 0.1, 0.1], 0.667)
    assert p[1] == ([False, False, True], [0.333333, 0.25, 0.0999999], 0.333)
    assert mf_parameters(dict(res, status=2), 2) == {}
    # the `.uf`: the LAST maximum after three decimals
    c = np.asarray([[0.2, 0.5, 0.3], [0.3334, 0.3333, 0.3333], [0.0, 1.0, 0.0], [0.25, 0.2504, 0.2496]], np.float32)
    assert uf_classes(c).tolist() == [1, 2, 1, 2]


@pytest.mark.parametrize("path", SHELL_FIXTURES, ids=SHELL_IDS)
def test_labels_equal_the_real_partition_shell(path):
    rec = load(path)
    n_shell = int(rec["select"].sum())
    shell = [f for f in rec["names"] if rec["labels"][f] == "S"]
    seen = set()
    for run in rec["runs"]:
        init = init_of(run["init"])
        if "error" in run:                                    # no shell family: Q = "auto" divides by the mean 0.0
            assert run["error"][0] == "ZeroDivisionError" and n_shell == 0
            with pytest.raises(ZeroDivisionError):
                resolve_q(run["Q"], init, n_shell, rec["means"][1])
            continue
        if run["returned"] == []:                             # Q <= 1: the reference logs an error and returns ()
            with pytest.raises(ValueError):
                resolve_q(run["Q"], init, n_shell, rec["means"][1])
            seen.add("low")
            continue
        Q = resolve_q(run["Q"], init, n_shell, rec["means"][1])
        assert Q == run["returned"] == run["calls"][0]["Q"]
        assert run["calls"][0]["init"] == ("random" if init is None else "param_file")
        call = run["calls"][0]
        parameters = {k: (mu, eps, prop) for k, mu, eps, prop in call["parameters"]}
        fams, classes = [f for f, _ in call["classes"]], [k for _, k in call["classes"]]
        assert fams == shell
        params, by_org, families, labels = shell_labels(parameters, classes, fams, rec["everyone"], run["exclusity_th"], init)
        assert [[label, v[0], v[1], v[2]] for label, v in params.items()] == run["parameters"]
        assert {org: sorted(v) for org, v in by_org.items()} == run["organisms"]
        assert families == run["families"]
        attr = {f: LONG[rec["labels"][f]] for f in rec["names"]}
        attr.update({f: labels[k] for f, k in call["classes"]})
        assert attr == run["node_attribute"]
        seen.update(label.split(":")[0].split("_")[1] for label in params)
        seen.add("groups" if any(label.count("_") == 2 for label in params) else type(init).__name__)
    assert {"low", "exclusive", "shared"} <= seen
    if n_shell:
        assert Q == 3 and shell_q_auto(n_shell, rec["means"][1]) == rec["runs"][0]["returned"]


def test_a_run_that_emptied_a_class_is_the_references_keyerror():
    with pytest.raises(KeyError):
        shell_labels({}, ["U", "U"], ["a", "b"], ["o1"])


def test_q_rules():
    assert resolve_q("auto", None, 20, 7.375) == 4 and resolve_q("auto", {"a": 1, "b": 2}, 20, None) == 3 and resolve_q("auto", [set(), set()], 20, None) == 3
    assert resolve_q(32, None, 5, None) == 32
    for bad in (1, 0, -3, 33, "many"):
        with pytest.raises(ValueError):
            resolve_q(bad, None, 20, 7.0)
    with pytest.raises(ValueError):
        resolve_q("auto", None, 20, None)


def test_gexf_carries_the_subpartition(tmp_path):
    rec = load(SHELL_FIXTURES[SHELL_IDS.index("closed")])
    ft, et, ann = host_tables(rec)
    sub = ("subpartition_shell", rec["gexf_node_attribute"])
    write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, subpartition=sub)
    write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, subpartition=sub)
    same_gexf_text(open(str(tmp_path / "full.gexf"), newline="", encoding="utf-8").read(), rec["gexf"], rec["everyone"], "full")
    same_gexf_text(open(str(tmp_path / "light.gexf"), newline="", encoding="utf-8").read(), rec["gexf_light"], rec["everyone"], "light")
    assert 'title="subpartition_shell" type="string"' in rec["gexf"] and "_exclusive:" in rec["gexf"]


def test_gexf_without_a_subpartition_is_the_file_as_before(tmp_path):
    rec = load_json([p for p in GEXF_FIXTURES if p.endswith("links.json")][0])
    ft, et, ann = host_tables(rec)
    write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, subpartition=None)
    same_gexf_text(open(str(tmp_path / "full.gexf"), newline="", encoding="utf-8").read(), rec["gexf"], rec["organisms"] + rec["new_organisms"], "links")
    assert "subpartition_shell" not in rec["gexf"]


@pytest.mark.parametrize("path", [p for p, i in zip(SHELL_FIXTURES, SHELL_IDS) if i != "noshell"], ids=[i for i in SHELL_IDS if i != "noshell"])
def test_oracle_on_the_host_formed_problem_equals_the_compiled_reference(path, oracle):
    rec = load(path)
    x, nei, _ = host_problem(rec)
    for Q in REF_QS:
        ref = {key: rec["ref"]["%s_%d" % (key, Q)] for key in ("status", "best_start", "c", "center", "disp", "prop")}
        got = oracle.run_random(x, nei, Q, n_starts=50, rng_seed=REF_SEED, algo="ncem", disper="sk_", beta=0.5, it_max=100, tie="libc")
        assert got["status"] == int(ref["status"]) and got["best_start"] == int(ref["best_start"]), Q
        assert np.array_equal(got["c"], ref["c"]), Q
        assert np.array_equal(got["center"], ref["center"]), Q
        for key in ("disp", "prop"):
            assert maxdiff(got[key], ref[key]) <= TOL, (Q, key)
