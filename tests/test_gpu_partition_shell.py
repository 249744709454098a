"""partition_shell on the device (nemgpu_master_subproblem, Master.partition_shell): the device-formed problem against
shell.form_subproblem_host bit for bit at the shapes where the kernels can go wrong, and the runs against
run_partitioning_arrays on the host-formed arrays and against the compiled reference's recorded random starts
(tests/golden/partition_shell/)."""
import numpy as np
import pytest

from pangenomenem_amd.chunks import Master, pack_rows
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.partitioning import class_sums, run_partitioning_arrays
from pangenomenem_amd.shell import LONG, Subproblem, form_subproblem_host, mf_parameters, outside_entry_host, shell_init_params
from tests.partition_shell_util import REF_QS, REF_SEED, SHELL_FIXTURES, SHELL_IDS, TOL, grouped_matrix, host_problem, init_of, load, synthetic_master
from tests.projection_util import annotations_of
from tests.util import maxdiff

pytestmark = pytest.mark.gpu


def same_problem(m, arrays, select, organisms=None, edges="induced", k=3):
    """the device-formed problem == the numpy statement, bit for bit: families, rows, ptr, idx, w"""
    x, ptr, idx, eb, counts = arrays
    orgs = np.arange(x.shape[1]) if organisms is None else np.asarray(organisms)
    xs, (ph, ih, wh), fam = form_subproblem_host(x, ptr, idx, eb, orgs, select, counts, edges)
    sub = Subproblem(m, select, k, organisms, edges)
    try:
        assert sub.engine is not None and sub.outside_entry == -1
        assert (sub.n, sub.nnz) == (len(fam), len(ih))
        assert np.array_equal(sub.families, fam)
        rows, (p, i, w) = sub.fetch()
        assert np.array_equal(rows, pack_rows(xs))
        assert np.array_equal(p, ph) and np.array_equal(i, ih)
        assert np.array_equal(w.view(np.uint32), wh.view(np.uint32))
    finally:
        sub.close()
    return fam, (ph, ih, wh)


def selections(n):
    one = np.zeros(n, bool)
    one[n // 2] = True
    return [("one", one), ("all", np.ones(n, bool)), ("seventh", np.arange(n) % 7 == 0)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1030])
def test_families_around_words_and_tiles(gpu_lib, n):
    arrays = synthetic_master(n, 40, 1000 + n, loops=n > 1, extras=(1, 2))
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        for what, select in selections(n):
            fam, (ptr, idx, _) = same_problem(m, arrays, select)
            if what == "all" and n > 4:
                j = fam.tolist().index(3)
                assert ptr[j + 1] == ptr[j]                   # a kept family with degree 0
                assert (idx == np.repeat(np.arange(len(fam)), np.diff(ptr))).any()      # self-loops
        with pytest.raises(NemGpuError, match="keeps no family"):
            Subproblem(m, np.zeros(n, bool), 3)
    finally:
        m.close()


@pytest.mark.parametrize("d", [1, 31, 32, 33, 64, 65])
def test_organisms_around_words(gpu_lib, d):
    arrays = synthetic_master(300, d, 2000 + d, loops=True, extras=(1,) if d > 1 else ())
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        same_problem(m, arrays, np.arange(300) % 3 != 1)
        if d > 2:
            same_problem(m, arrays, np.arange(300) % 3 != 1, organisms=np.arange(d)[::-1][:d - 1])
    finally:
        m.close()


def test_a_sparse_selection_spans_more_words_than_a_tile_stages(gpu_lib):
    n = 3000
    arrays = synthetic_master(n, 70, 7)
    select = np.arange(n) % 60 == 0                           # 50 families: one tile, 47 words of every organism row
    assert (np.flatnonzero(select)[-1] >> 6) - (np.flatnonzero(select)[0] >> 6) > 12
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        same_problem(m, arrays, select)
        dense = (np.arange(n) % 60 == 0) | (np.arange(n) < 700)      # a staged tile, then unstaged ones
        same_problem(m, arrays, dense)
    finally:
        m.close()


def test_an_organism_subset_leaves_selected_families_out(gpu_lib):
    arrays = synthetic_master(500, 24, 11, loops=True, extras=(2, 5), density=0.15)
    select = np.arange(500) % 2 == 0
    orgs = [5, 20, 3]
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        fam, _ = same_problem(m, arrays, select, organisms=orgs)
        assert 0 < len(fam) < select.sum()
        gone = select & ~arrays[0][:, orgs].any(axis=1)
        lone = np.zeros(500, bool)
        lone[np.flatnonzero(gone)[0]] = True
        with pytest.raises(NemGpuError, match="keeps no family"):          # selected, but in none of these organisms
            Subproblem(m, lone, 3, organisms=orgs)
    finally:
        m.close()


def test_extras_lists_of_every_walk(gpu_lib):
    arrays = synthetic_master(260, 256, 13, loops=True, extras=(1, 32, 33, 200), density=0.95)
    assert {1, 32, 33, 200} <= set(np.diff(arrays[4][0]).tolist())
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        same_problem(m, arrays, np.ones(260, bool))
        same_problem(m, arrays, np.arange(260) % 7 != 0, organisms=np.arange(0, 256, 2))
    finally:
        m.close()


def test_a_bits_only_master(gpu_lib):
    x, ptr, idx, eb, _ = synthetic_master(257, 33, 17, loops=True)
    m = Master(x, ptr, idx, eb)
    try:
        same_problem(m, (x, ptr, idx, eb, None), np.arange(257) % 3 == 0)
    finally:
        m.close()


def test_the_reference_rule(gpu_lib):
    arrays = synthetic_master(400, 20, 19, loops=True, extras=(3,))
    x, ptr, idx, eb, counts = arrays
    m = Master(x, ptr, idx, eb, edge_counts=counts)
    try:
        # closed under adjacency (everything selected): an empty graph
        _, (p, i, _) = same_problem(m, arrays, np.ones(400, bool), edges="reference")
        assert len(i) == 0 and not p.any()
        # an open selection: the smallest CSR entry from a kept family to an unselected one, coverage > 0
        for select, orgs in ((np.arange(400) >= 200, None), (np.arange(400) % 5 == 2, [4, 9, 1]), (np.arange(400) % 2 == 1, [0])):
            want = outside_entry_host(x, ptr, idx, eb, np.arange(20) if orgs is None else orgs, select, counts)
            assert want >= 0
            sub = Subproblem(m, select, 3, orgs, "reference")
            assert sub.engine is None and sub.outside_entry == want
            with pytest.raises(KeyError) as err:
                form_subproblem_host(x, ptr, idx, eb, np.arange(20) if orgs is None else orgs, select, counts, "reference")
            assert err.value.args[0] == idx[want]
    finally:
        m.close()


def test_refusals(gpu_lib):
    arrays = synthetic_master(70, 9, 23)
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        select = np.ones(70, bool)
        for orgs in ([0, 9], [-1], [3, 3], []):
            with pytest.raises(NemGpuError):
                Subproblem(m, select, 3, organisms=orgs)
        for k in (0, 33):
            with pytest.raises(NemGpuError):
                Subproblem(m, select, k)
        with pytest.raises(ValueError):
            Subproblem(m, select[:-1], 3)
        with pytest.raises(ValueError):
            Subproblem(m, select, 3, edges="none")
        for Q in (1, 0, 33):
            with pytest.raises(ValueError):
                m.partition_shell(select=select, Q=Q)
        with pytest.raises(ValueError):
            m.partition_shell(select=select)                 # Q = "auto" without a mean
        with pytest.raises(ValueError):
            m.partition_shell(select=select, Q=3, init_using_qual={"a": {0, 1}, "b": {2}})       # no proportion is left
        with pytest.raises(ValueError):
            m.partition_shell()
    finally:
        m.close()
    # a master built directed
    genes, cptr, corg, circ = np.asarray([0, 1, 2, 1, 0], np.int32), np.asarray([0, 3, 5], np.int32), np.asarray([0, 1], np.int32), np.zeros(2, np.uint8)
    dm = Master.from_orders(genes, cptr, corg, circ, 2, directed=True)
    try:
        with pytest.raises(NemGpuError, match="directed"):
            Subproblem(dm, np.ones(dm.n, bool), 2)
        with pytest.raises(NemGpuError, match="directed"):
            dm.partition_shell(select=np.ones(dm.n, bool), Q=2)
    finally:
        dm.close()


def fixture_master(rec):
    m = Master.from_annotations(annotations_of(rec, rec["organisms"]), rec["organisms"], rec["circular"], rec["repeated"])
    if rec["new_organisms"]:
        grown = m.add_annotations(annotations_of(rec, rec["new_organisms"]), rec["new_organisms"], set(rec["circular"]) | set(rec["update_circular"]),
                                  set(rec["repeated"]) | set(rec["update_repeated"]))
        m.close()
        m = grown
    return m


def same_as_host_run(sub, x, nei, names, Q, seed, free_dispersion=False, init="random", params=None, beta=0.5):
    """Master.partition_shell == run_partitioning_arrays on the host-formed arrays: labels exact, parameters bit-equal"""
    parts, allp = run_partitioning_arrays(x, nei, beta, free_dispersion, Q, init=init, names=names, params=params, rng_seed=seed, tie="libc")
    assert sub.run["status"] == 0 and len(allp) == Q
    assert [parts[f] for f in names] == sub.classes.tolist()
    mus, epss = class_sums(sub.run["center"], sub.run["disp"], Q)
    for k in range(Q):
        assert allp[k] == (mus[k], epss[k], float(sub.run["prop"][k])), k


@pytest.mark.parametrize("path", SHELL_FIXTURES, ids=SHELL_IDS)
def test_fixture_runs(gpu_lib, path):
    rec = load(path)
    m = fixture_master(rec)
    try:
        assert m.names == rec["names"] and m.organism_names == rec["everyone"]
        if not rec["select"].any():
            sub = m.partition_shell(rec["labels"], Q=3, seed=1)
            assert (sub.Q, sub.parameters, sub.organisms, sub.families) == (3, {}, {}, {})
            assert sub.node_attribute == {f: LONG[c] for f, c in rec["labels"].items()}
            with pytest.raises(ZeroDivisionError):
                m.partition_shell(rec["labels"], mean_shell=rec["means"][1])
            return
        x, nei, fam = host_problem(rec)
        names = [rec["names"][i] for i in fam]
        for Q in REF_QS:
            sub = m.partition_shell(rec["labels"], Q=Q, seed=REF_SEED)
            assert sub.Q == Q and np.array_equal(sub.family_index, fam)
            same_as_host_run(sub, x, nei, names, Q, REF_SEED)
            # the compiled reference's run of the same problem and seed: labels exact, parameters within 1e-6
            ref = {key: rec["ref"]["%s_%d" % (key, Q)] for key in ("status", "best_start", "c", "center", "disp", "prop")}
            assert sub.run["status"] == int(ref["status"]) and sub.run["best_start"] == int(ref["best_start"])
            assert np.array_equal(sub.run["c"], ref["c"]) and np.array_equal(sub.run["center"], ref["center"])
            for key in ("disp", "prop"):
                assert maxdiff(sub.run[key], ref[key]) <= TOL, (Q, key)
            # what the labels are made of
            assert sub.parameters and sorted(f for v in sub.families.values() for f in v) == sorted(names)
            want = mf_parameters(sub.run, Q)
            for label, (orgs, eps, prop) in sub.parameters.items():
                k = int(label.split("_")[0])
                assert orgs == [o for o, b in zip(rec["everyone"], want[k][0]) if b] and prop == want[k][2]
                assert label.split(":")[0] == "%d_%s" % (k, "exclusive" if eps < 0.1 else "shared") and label.split(":")[1] == str(round(eps, 2))
            for f, c in rec["labels"].items():
                assert (sub.node_attribute[f] in sub.families) if c == "S" else (sub.node_attribute[f] == LONG[c])
        auto = m.partition_shell(rec["labels"], mean_shell=rec["means"][1], seed=3)
        assert auto.Q == rec["runs"][0]["returned"]
        byann = m.partition_shell(rec["labels"], annotations=annotations_of(rec), seed=3)
        assert byann.Q == auto.Q and byann.families == auto.families and byann.parameters == auto.parameters
    finally:
        m.close()


@pytest.mark.parametrize("n,d,Q,free", [(300, 40, 4, False), (700, 70, 9, True)])
def test_synthetic_runs(gpu_lib, n, d, Q, free):
    arrays = synthetic_master(n, d, 31 + n, loops=True, extras=(1, 4), density=0.4)
    select = np.random.default_rng(n).random(n) < 0.34
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        x, nei, fam = form_subproblem_host(*arrays[:4], np.arange(d), select, arrays[4])
        sub = m.partition_shell(select=select, Q=Q, free_dispersion=free, seed=77)
        assert np.array_equal(sub.family_index, fam)
        same_as_host_run(sub, x, nei, ["fam%d" % (i + 1) for i in fam], Q, 77, free_dispersion=free)
    finally:
        m.close()


def test_dict_and_list_inits(gpu_lib):
    x, groups = grouped_matrix()
    n, d = x.shape
    arrays = synthetic_master(n, d, 43, loops=True, extras=(2,), x=x)
    select = np.arange(n) % 10 != 9
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        xs, nei, fam = form_subproblem_host(*arrays[:4], np.arange(d), select, arrays[4])
        names = ["fam%d" % (i + 1) for i in fam]
        as_dict = {"g%d" % (g + 1): set(orgs) for g, orgs in enumerate(groups)}
        for init, Q in ((as_dict, 4), ([set(groups[0]), set(groups[1])], 3)):
            sub = m.partition_shell(select=select, init_using_qual=init, seed=5)
            assert sub.Q == Q
            same_as_host_run(sub, xs, nei, names, Q, 5, init="param_file", params=shell_init_params(init, list(range(d))))
            if isinstance(init, dict):                        # every group's class names it
                assert all(any(label.startswith("%d_" % g) and ("g%d" % (g + 1)) in label.split("_", 2)[2].split("|") for label in sub.parameters)
                           for g in range(3))
            else:
                assert all(label.count("_") == 1 for label in sub.parameters)
    finally:
        m.close()


def test_an_emptied_class_and_the_reference_edges(gpu_lib):
    rec = load(SHELL_FIXTURES[SHELL_IDS.index("closed")])
    m = fixture_master(rec)
    try:
        x, nei, fam = host_problem(rec)
        names = [rec["names"][i] for i in fam]
        # twenty families do not fill the fourth class of this parameter file: nem() writes no files, run_partitioning
        # returns 'U' for every family and no parameters, and partition_shell dies on labels['U']
        with pytest.raises(KeyError, match="U"):
            m.partition_shell(rec["labels"], init_using_qual=init_of({"dict": rec["m_inits"]["dict"]}), seed=5)
        # the writer as written on a closed shell: the same families on an empty graph
        sub = m.partition_shell(rec["labels"], Q=4, edges="reference", seed=REF_SEED)
        same_as_host_run(sub, x, None, names, 4, REF_SEED)
    finally:
        m.close()
    rec = load(SHELL_FIXTURES[SHELL_IDS.index("open")])
    m = fixture_master(rec)
    try:
        with pytest.raises(KeyError) as err:
            m.partition_shell(rec["labels"], Q=4, edges="reference", seed=1)
        with pytest.raises(KeyError) as host:
            host_problem(rec, "reference")
        assert err.value.args[0] == rec["names"][host.value.args[0]] and rec["labels"][err.value.args[0]] != "S"
    finally:
        m.close()


def test_the_master_is_only_read(gpu_lib):
    arrays = synthetic_master(600, 30, 41, loops=True, extras=(2,))
    m = Master(*arrays[:4], edge_counts=arrays[4])
    try:
        before = m.partition(seed=9)
        kept = m.arrays()
        shell = np.asarray([before[0].get("fam%d" % (i + 1)) == "S" for i in range(600)])
        sub = m.partition_shell(select=shell if shell.sum() > 3 else np.arange(600) % 3 == 0, Q=3, seed=4)
        assert len(sub.family_index) > 3
        after = m.partition(seed=9)
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2] == after[2]
        for a, b in zip(kept, m.arrays()):
            for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert np.array_equal(u, v)
    finally:
        m.close()
