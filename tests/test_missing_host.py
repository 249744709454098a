"""Missing cells (nan in the .dat), host side: the file reader, and the numpy statement of the masked NCEM
(tests/missing_util.py) pinned to the oracle where nothing is missing and to the recorded reference where cells are."""
import numpy as np
import pytest

from tests import missing_util as mu
from tests.util import bits_equal, maxdiff, random_hard_partition

TOL = 1e-6


@pytest.fixture(scope="module")
def io_lib():
    from pangenomenem_amd import build, engine
    build.build()
    return engine


def _write_case(tmp_path, n, d, seed, frac=0.1):
    from pangenomenem_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.random((n, d)) < 0.5).astype(np.uint8)
    obs = rng.random((n, d)) >= frac
    prop, center, disp = synth.default_init(d)
    return x, obs, prop, center, disp


def test_reader_marks_nan_cells_unobserved(io_lib, tmp_path):
    """nan / NaN / nan(0) tokens in rows of the regular form (one character and a tab per value elsewhere in the row:
    the row fast path up to the token, the tokeniser from there), in rows separated by spaces, and the last cell."""
    n, d = 37, 44
    x, obs, prop, center, disp = _write_case(tmp_path, n, d, 5)
    obs[3, :] = False                                        # a family without an observed cell
    obs[n - 1, d - 1] = False                                # the last cell of the file
    obs[7, :] = True                                         # a complete regular row between masked ones
    base = mu.write_masked_inputs(str(tmp_path), x, obs, None, prop, center, disp, tokens=mu.NAN_TOKENS)
    lines = open(base + ".dat").read().split("\n")
    lines[5] = lines[5].replace("\t", "  ")                  # a spaced row
    lines[9] = " " + lines[9].replace("\t", " \t ")
    lines[11] = lines[11].replace("1", "1.0", 1)             # (what already left the fast path: a decimal value)
    open(base + ".dat", "w").write("\n".join(lines))
    got = io_lib.read_inputs(base, 3)
    assert got["n_missing"] == int((~obs).sum())
    assert np.array_equal(got["observed"], obs)
    assert np.array_equal(got["x"][obs], x[obs])
    assert not got["x"][~obs].any()                          # the matrix bit of an unobserved cell is cleared


def test_reader_nan_in_a_file_the_parallel_reader_would_share(io_lib, tmp_path):
    """A regular file of more than 2 MB is read by several threads, each its share of rows at known offsets.  A nan
    token is longer than the value it stands for, so the file no longer has the regular size and the general reader
    takes over -- as for `1.0`: nan cells in what would have been the second thread's rows, and the rows around them
    through the row fast path."""
    n, d = 2200, 512                                         # 2 * n * d bytes: 2.25 MB
    rng = np.random.Generator(np.random.PCG64(9))
    x = (rng.random((n, d)) < 0.5).astype(np.uint8)
    obs = np.ones((n, d), bool)
    obs[1500, 3] = obs[1500, 400] = obs[2100, 511] = obs[n - 1, 0] = False
    from pangenomenem_amd import synth
    prop, center, disp = synth.default_init(d)
    base = mu.write_masked_inputs(str(tmp_path), x, obs, None, prop, center, disp, tokens=mu.NAN_TOKENS)
    got = io_lib.read_inputs(base, 3)
    assert got["n_missing"] == 4
    assert np.array_equal(got["observed"], obs)
    assert np.array_equal(got["x"], np.where(obs, x, 0))


def test_reader_complete_file_has_no_mask(io_lib, tmp_path):
    n, d = 40, 12                                            # d % 4 == 0: the parallel reader's regular form
    x, obs, prop, center, disp = _write_case(tmp_path, n, d, 6)
    base = mu.write_masked_inputs(str(tmp_path), x, np.ones_like(obs), None, prop, center, disp)
    got = io_lib.read_inputs(base, 3)
    assert got["observed"] is None and got["n_missing"] == 0
    assert np.array_equal(got["x"], x)


def test_reader_still_refuses_other_values(io_lib, tmp_path):
    from pangenomenem_amd.engine import NemGpuError
    n, d = 10, 6
    x, obs, prop, center, disp = _write_case(tmp_path, n, d, 7)
    base = mu.write_masked_inputs(str(tmp_path), x, obs, None, prop, center, disp)
    text = open(base + ".dat").read().replace("0", "2", 1)
    open(base + ".dat", "w").write(text)
    with pytest.raises(NemGpuError, match="0/1"):
        io_lib.read_inputs(base, 3)


# ---- the statement against the oracle: nothing missing ----------------------------------------------------------------
def _problem(n, d, k, seed):
    from pangenomenem_amd import synth
    x, _ = synth.bernoulli_pa_matrix(n, d, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    prop = rng.random(k).astype(np.float32)
    prop /= prop.sum()
    center = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(k, d))
    disp = (0.02 + 0.6 * rng.random((k, d))).astype(np.float32)
    return x, prop, center, disp


def test_density_all_ones_mask_equals_oracle(oracle):
    x, prop, center, disp = _problem(203, 37, 3, 11)
    disp[1, 4] = 0.0                                         # a null dispersion: zero densities where the cell mismatches
    disp[2, :] = 0.7                                         # eps > 1/2: a negative log ratio
    want_pk, want_lp, want_sts = oracle.density(x, prop, center, disp)
    pk, lp, sts = mu.density_masked_host(x, np.ones(x.shape, bool), prop, center, disp)
    assert sts == want_sts
    assert bits_equal(lp, want_lp)
    assert bits_equal(pk, want_pk)


@pytest.mark.parametrize("disper", mu.DISPERSIONS)
@pytest.mark.parametrize("propor", ["pk", "p_"])
def test_mstep_all_ones_mask_equals_oracle(oracle, disper, propor):
    n, d, k = 240, 21, 3
    x, prop, center, disp = _problem(n, d, k, 13)
    c = random_hard_partition(n, k, 17)
    # exact median ties: organism 0 of class 0 and organism 5 of class 2 have as many zeros as ones among the members
    for h, j in ((0, 0), (2, 5)):
        members = np.flatnonzero(c[:, h] == 1)
        if len(members) % 2:
            c[members[-1]] = 0
            c[members[-1], 1] = 1                            # (class 1 has no forced tie)
            members = members[:-1]
        x[members, j] = np.arange(len(members)) % 2
    want = oracle.mstep(x, c, disper, propor, prop, center, disp)
    got = mu.mstep_masked_host(x, np.ones(x.shape, bool), c, disper, propor, prop, center, disp)
    assert (want["center"] == 0.5).sum() >= 2
    assert got["status"] == want["status"] and got["emptyk"] == want["emptyk"]
    for key in ("prop", "center", "disp", "nbobs_k", "nbobs_kd", "iner"):
        assert bits_equal(got[key], want[key]), key


def test_mstep_empty_class_equals_oracle(oracle):
    n, d, k = 90, 9, 3
    x, prop, center, disp = _problem(n, d, k, 19)
    c = random_hard_partition(n, k, 23)
    c[c[:, 1] == 1] = np.array([1, 0, 0], np.float32)        # class 1 loses its members
    want = oracle.mstep(x, c, "skd", "pk", prop, center, disp)
    got = mu.mstep_masked_host(x, np.ones(x.shape, bool), c, "skd", "pk", prop, center, disp)
    assert got["emptyk"] == want["emptyk"] == 2 and got["status"] == want["status"] == 2
    for key in ("prop", "center", "disp", "nbobs_k", "nbobs_kd", "iner"):
        assert bits_equal(got[key], want[key]), key


def test_mstep_centre_rule_in_integers():
    """The literal walk gives 0 / 0.5 / 1 for 2 zeros >, =, < obs -- the rule of k_finish_masked -- at every count."""
    for obs_n in range(1, 9):
        for zeros in range(obs_n + 1):
            n = obs_n + 3                                    # three unobserved members besides
            xj = np.array([False] * zeros + [True] * (obs_n - zeros) + [True, False, True])
            oj = np.array([True] * obs_n + [False] * 3)
            ch = np.ones(n, np.float32)
            got = mu._median_walk(xj, oj, ch, np.float32(obs_n))
            want = 0.0 if 2 * zeros > obs_n else 0.5 if 2 * zeros == obs_n else 1.0
            assert got == want, (obs_n, zeros, got)


# ---- ... and against the recorded reference: cells missing --------------------------------------------------------------
@pytest.mark.parametrize("name", mu.fixture_names())
def test_run_masked_host_reproduces_reference(oracle, name):
    """Labels equal to the reference's .uf, centres equal to its .mf, dispersions within TOL (the .mf prints them
    with six significant digits: 5e-7 at most below 1).  The .mf prints a proportion with THREE digits; the reference's
    value is N_k / N of the partition its last M-step saw, and in a converged run that is the final partition, which
    the .uf gives exactly: the proportions are held to TOL against those counts, and to the print against the .mf."""
    case = mu.load_fixture(name)
    cfg, k = case["cfg"], case["k"]
    n, d = case["x"].shape
    got = mu.run_masked_host(oracle, case["x"], case["obs"], case["nei"], k, case["prop"], case["center"], case["disp"],
                             beta=cfg["beta"], disper=cfg["disper"], propor=cfg["propor"], cvtest=cfg["cvtest"],
                             cvthres=cfg["cvthres"], it_max=cfg["it_max"])
    assert got["status"] == 0 and got["iters"] == case["meta"]["iters"] and got["converged"] == case["meta"]["converged"]
    labels = mu.parse_uf(case["ref_uf"], k)
    assert np.array_equal(got["c"].argmax(axis=1), labels)
    prop, center, disp = mu.parse_mf(case["ref_mf"], k, d)
    assert np.array_equal(got["center"], center.astype(np.float32))
    assert maxdiff(got["disp"], disp) <= TOL
    assert case["meta"]["converged"]
    counts = np.bincount(labels, minlength=k).astype(np.float32)
    assert maxdiff(got["prop"], counts / np.float32(n)) <= TOL
    assert maxdiff(got["prop"], prop) <= 5.1e-4              # " %5.3g ": three significant digits of a value below 1
