"""profile_density_many (the benchmark's E1 probe of a lock-step batch): the members' density kernels zipped into one
launch with each member's own grid width.  Three members of 300, 2100 and 700 families: K = 3 and density_blocks
(nem_kernels.hip) give 8 K, 16 K and 8 K blocks (512, 2304 and 768 padded families), so the launch is as wide as the
second member and the blocks beyond the others' widths return.  The probe rewrites the densities from the parameters
the run left and must leave the engines as they were: a second run() gives the first one's answer bit for bit."""
import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.lockstep_members import SOLO_KEYS

pytestmark = pytest.mark.gpu

FAMILIES = (300, 2100, 700)


def density_blocks(n, k):
    npad = (n + 255) // 256 * 256
    return (npad // 256 + 7) // 8 * 8 * k


@pytest.mark.parametrize("d", [24, 300])                       # 300 organisms: the fast-forwarded chain
def test_the_probe_counts_every_member_and_leaves_the_engines_as_they_were(gpu_lib, d):
    from pangenomenem_amd.engine import NemEngine, profile_density_many
    assert [density_blocks(n, 3) for n in FAMILIES] == [24, 48, 24]
    engines = []
    try:
        for j, n in enumerate(FAMILIES):
            x, _ = synth.grouped_pa_matrix(n, d, 70 + j, groups=6)
            prop, center, disp = synth.kclass_init(x, 3)
            e = NemEngine(n, d, 3)
            engines.append(e)
            e.set_matrix(x); e.set_graph(synth.contiguity_graph(n, 70 + j)); e.set_params(prop, center, disp)
            e.configure(algo="ncem", beta=0.5, disper="sk_", propor="pk", it_max=4, tie="hash", seed=3)
        first = [e.run() for e in engines]
        ms, nbytes = profile_density_many(engines, 2)
        alone = [profile_density_many([e], 2) for e in engines]
        again = [e.run() for e in engines]
    finally:
        for e in engines:
            e.close()
    assert ms > 0 and all(t > 0 for t, _ in alone)
    assert nbytes == sum(b for _, b in alone)
    for a, b, n in zip(first, again, FAMILIES):
        assert a["iters"] == b["iters"] and a["status"] == b["status"], n
        for key in SOLO_KEYS:
            assert np.array_equal(a[key], b[key], equal_nan=True), (key, n)
