"""The masters of tests/master_shapes.py reach the kernel branches tests/test_gpu_master_shapes.py is there to run, so
that those tests cannot quietly stop covering them: asserted on the CPU from the fixtures and the kernels' launch
arithmetic.  And the master builders' default spectrum still gives every older fixture bit for bit."""
import hashlib

import numpy as np
import pytest

from pangenomenem_amd import synth
from tests import master_shapes as ms


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def flat(out):
    return [a for v in out for a in (v if isinstance(v, tuple) else (v,))]


# recorded from the builders before they took a / b
@pytest.mark.parametrize("counts,args,kw,want", [
    (False, (3000, 300, 5), {}, "1e7537fff1a0b894"),
    (False, (2000, 40, 3), {}, "2c3095a467e19cae"),
    (True, (1500, 40, 8), dict(multi_frac=0.1, loops=0.02), "7be050c21c3a46ff"),
    (True, (2500, 320, 2), dict(multi_frac=0.05, dense_loops=2, directed=True), "a1bc8506edd1b1eb")])
def test_default_spectrum_keeps_the_old_fixtures(counts, args, kw, want):
    build = synth.master_pangenome_counts if counts else synth.master_pangenome
    assert digest(flat(build(*args, **kw))) == want
    assert digest(flat(build(*args, a=0.3, b=0.3, **kw))) == want
    assert digest(flat(build(*args, a=0.05, b=1.0, **kw))) != want


def test_spectrum_reaches_the_matrix():
    x0, _, _ = synth.master_pangenome(4000, 60, 1)
    x1, _, _ = synth.master_pangenome(4000, 60, 1, a=0.05, b=1.0)
    assert x1.mean() < 0.2 < x0.mean()


def test_launch_arithmetic():
    assert ms.index_passes(65536) == 1 and ms.index_passes(65537) == 2 and ms.index_passes(140000) == 3
    assert ms.core_y_blocks(4096) == 1 and ms.core_y_blocks(4097) == 2
    assert ms.tile_shape(1) == (0, 1, 256) and ms.tile_shape(255) == (0, 255, 256)
    assert ms.tile_shape(256) == (1, 256, 256) and ms.tile_shape(257) == (1, 1, 512)
    assert ms.organism_passes(256) == 1 and ms.organism_passes(257) == 2
    fam = np.arange(256) * 3
    assert ms.tile_staged(fam) == [True] and ms.tile_staged(fam * 4) == [False]
    assert ms.tile_staged(np.r_[0, np.arange(255) + 11 * 64 - 254]) == [True]      # first and last 11 words apart
    assert ms.tile_staged(np.r_[0, np.arange(255) + 12 * 64 - 254]) == [False]     # 12


def test_wide_masters_pass_2048_words():
    for x, _, _, *rest in (ms.wide_master(), ms.wide_counts_master()):
        n = x.shape[0]
        assert ms.nw64(n) > 2048 and ms.index_passes(n) >= 3
        assert ms.core_y_blocks(n) >= 2 and ms.vote_blocks(n) > 256


def test_cloud_master_mixes_staged_and_unstaged_samples():
    x, _, _ = ms.cloud_master()
    assert ms.core_y_blocks(x.shape[0]) >= 2
    staged = [ms.tile_staged(ms.kept(x, s)) for s in ms.cloud_samples()]
    assert any(not all(t) for t in staged) and any(all(t) for t in staged)
    assert any(all(not v for v in t) for t in staged)       # a sample of unstaged tiles only
    dcs = [len(s) for s in ms.cloud_samples()]
    assert 1 in dcs and 257 in dcs and 300 in dcs
    assert ms.organism_passes(257) == 2


@pytest.mark.parametrize("which", ["bits", "counts"])
def test_wide_groups_straddle_65536(which):
    x = (ms.wide_master() if which == "bits" else ms.wide_counts_master())[0]
    nc = [len(ms.kept(x, s)) for s in ms.wide_samples()]
    groups = [nc[g:g + ms.WIDE_GROUP] for g in range(0, len(nc), ms.WIDE_GROUP)]
    assert all(min(g) < ms.FUSED_LIMIT <= max(g) for g in groups), nc
    assert 1 in map(len, ms.wide_samples()) and 257 in map(len, ms.wide_samples())


def test_boundary_masters():
    for n, d in ms.BOUNDARY_SHAPES:
        x, (ptr, idx), eb = ms.boundary_master(n, d)
        assert x.shape == (n, d) and eb.shape == (len(idx), (d + 31) // 32)
    ns = {n for n, _ in ms.BOUNDARY_SHAPES}
    ds = {d for _, d in ms.BOUNDARY_SHAPES}
    assert {1, 63, 64, 65, 4097} <= ns and {1, 32, 33, 65} <= ds
    assert 64 * ms.nw64(63) - 63 == 1 and 64 * ms.nw64(64) == 64 and ms.nw64(65) == 2


def test_tile_master_keeps():
    x, (ptr, idx), eb = ms.tile_master()
    assert x.shape == (600, 6) and x.any(axis=1).all()
    for o, c in enumerate(ms.TILE_KEEPS):
        assert len(ms.kept(x, [o])) == c
    tails = {ms.tile_shape(len(ms.kept(x, s)))[1:] for s in ms.tile_samples()}
    assert {(1, 256), (255, 256), (256, 256), (1, 512)} <= tails
    # its edges are the organisms that hold both ends
    src = np.repeat(np.arange(600), np.diff(ptr))
    bits = np.unpackbits(eb.view(np.uint8), axis=1, bitorder="little")[:, :6]
    assert np.array_equal(bits, x[src] & x[idx]) and bits.any()
