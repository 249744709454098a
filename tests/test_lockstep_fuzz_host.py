"""What the member lists of tests/test_gpu_lockstep_fuzz.py cover, asserted on the CPU so that a later edit cannot
quietly shrink them.  (a) from the problems and the oracle's results; (b) to (d) from the members' sizes and
configurations with the arithmetic the library uses, restated in tests/lockstep_members.py:

  * nem_sweep.hip, sweep_variant: template K = K when 1 <= K <= 10, else the generic instance; the mode is fuzzy,
    NCEM, or NCEM under the reference's tie stream;
  * nem_sweep.hip, sweep_block_sites: big = n >= 65 536 and K <= 10 selects the __launch_bounds__(1024)
    instances (the generic one has none), launched with ceil(n / 256 blocks) sites per block rounded up to whole waves, 256 to 1024;
  * nem_engine.hip, nemgpu_engine::fused_update(): d <= kFusedMaxD = 1024 and dispersion sk_ or skd;
    nemgpu_engine::use_ff(): d >= 256;
  * nem_kernels.hip, launch_finish: one block per class for sk_ / skd (variant 1), one block for s__ / s_d (variant 0);
    launch_mstep_counts: four organism rows per block when d + 1 >= 1024.

One thing the arithmetic says about (d) that its issue did not expect: enqueue_iteration (nem_engine.hip) takes the
fused density launch only when nothing records (current_recorder() == nullptr), so a lock-step step never holds one
(launch_density_fused refuses a recorder): every member of a step updates in k_finish_b and takes k_density_b, and the
three classes of fused_update() x use_ff() differ in what the members' SOLO runs take, which the lock-step results must
equal bit for bit.  Within the step the classes still differ by fast-forward, by k_finish_b's variant and by the counts
kernel."""
import numpy as np

from tests import lockstep_members as M


def test_the_random_groups_cover_what_they_are_meant_to(oracle):
    groups = [M.fuzz_group(g) for g in range(M.FUZZ_GROUPS)]
    probs = [p for grp in groups for p in grp]
    assert len(probs) == 80
    want = [oracle.run(*p[:6], **p[6]) for p in probs]
    cfgs = [p[6] for p in probs]
    assert {p[2] for p in probs} == {1, 2, 3, 4, 5, 8, 12}                      # every K of the generator
    assert {c["algo"] for c in cfgs} == {"ncem", "nem"}
    assert {c["disper"] for c in cfgs} == {"sk_", "skd", "s__", "s_d"}
    assert {c["propor"] for c in cfgs} == {"pk", "p_"}
    assert {c["tie"] for c in cfgs} == {"hash", "first", "libc"}
    assert any(p[0].shape[0] == 1 for p in probs)                              # one family
    assert any(p[1] is None for p in probs)                                    # no graph
    assert any(c["it_max"] == 0 for c in cfgs)
    assert any(c["param_fix"] for c in cfgs)
    assert any(p[0].shape[1] >= M.FF_MIN_D for p in probs)                     # the fast-forwarded chain
    assert sum(w["status"] == 2 for w in want) == 19                           # stopped by an empty class
    assert any(w["n_zero_density"] > 0 for w in want)
    for grp in groups:
        assert len({p[2] for p in grp}) >= 4                                   # so: four sequence groups at least
    # members of one call leave it at different iterations, and in most calls for different reasons
    for g in range(M.FUZZ_GROUPS):
        assert len({w["iters"] for w in want[8 * g:8 * g + 8]}) >= 2, g
    assert sum(len({w["status"] for w in want[8 * g:8 * g + 8]}) == 2 for g in range(M.FUZZ_GROUPS)) >= 6


def test_every_sweep_instance_is_reached():
    reached = set()
    for algo, tie in M.SWEEP_CASES:
        specs = M.every_k_specs(algo, tie)
        assert [s["k"] for s in specs] == list(range(1, 13)) + [17, 32]
        assert specs[0]["n"] == 300 and 1400 <= specs[-1]["n"] <= 1600 and len({s["n"] for s in specs}) == len(specs)
        assert len({(s["n"] + 255) // 256 for s in specs}) >= 4                # grid widths differ
        assert all(s["d"] == 24 and s["cfg"]["it_max"] == (4 if algo == "nem" else 6) for s in specs)
        reached |= {M.sweep_instance(s["n"], s["k"], s["cfg"]) for s in specs}
    small = {i for i in M.all_sweep_instances() if i[2] == 256}
    assert len(small) == 33 and small <= reached                               # (b) alone: every 256-site instance
    for algo, tie in M.BIG_CASES:
        specs = M.big_specs(algo, tie)
        big = specs[:M.BIG_SMALL_MEMBER]
        assert [s["k"] for s in big] == list(range(1, 11))
        assert sorted(s["n"] for s in big) == [65536] * 5 + [100003] * 5
        assert all(M.sweep_block_sites(s["n"], s["k"])[0] for s in big)
        assert {M.sweep_block_sites(s["n"], s["k"])[1] for s in big} == {256, 448}
        assert not M.sweep_block_sites(65535, 3)[0] and not M.sweep_block_sites(65536, 11)[0]      # the threshold; the generic K
        lone = specs[M.BIG_SMALL_MEMBER]
        assert lone["n"] == 200 and (lone["n"] + 255) // 256 == 1 and M.sweep_instance(lone["n"], lone["k"], lone["cfg"])[2] == 256
        # 1 block beside 256 (65 536 / 256) and 224 (100 003 / 448, the last one short)
        assert {(s["n"] + M.sweep_block_sites(s["n"], s["k"])[1] - 1) // M.sweep_block_sites(s["n"], s["k"])[1] for s in big} == {256, 224}
        assert all(s["d"] == 12 and s["cfg"]["it_max"] == 2 for s in specs)
        reached |= {M.sweep_instance(s["n"], s["k"], s["cfg"]) for s in specs}
    # K 0..10 x three modes x two block classes would be 66; the generic instance has no large-block form (big needs
    # K <= 10, nem_sweep.hip, sweep_block_sites, and sweep_dispatch's default branch launches 256-site blocks only), which leaves 63
    assert len(M.all_sweep_instances()) == 63
    assert M.all_sweep_instances() == reached


def test_every_density_and_update_path_is_reached():
    for algo in M.DENSITY_CASES:
        specs = M.density_specs(algo)
        assert len(specs) == 16 and {(s["d"], s["cfg"]["disper"]) for s in specs} == {(d, m) for d in M.DENSITY_D for m in M.DENSITY_DISPER}
        assert all(s["cfg"]["algo"] == algo and s["cfg"]["it_max"] == 4 and 600 <= s["n"] <= 720 for s in specs)
        assert len({s["n"] for s in specs}) == 16
        classes = {(M.density_class(s["d"], s["cfg"]["disper"]), s["k"]) for s in specs}
        assert classes == {(c, k) for c in ("fused plain", "fused fast-forward", "non-fused") for k in (3, 4)}
        # what differs inside the recorded step: fast-forward, k_finish_b's variant, the counts kernel -- each at K 3 and 4
        step = {(M.use_ff(s["d"]), M.finish_separable(s["cfg"]["disper"]), M.wide_counts(s["d"]), s["k"]) for s in specs}
        assert step == {(ff, sep, wide, k) for ff, wide in ((False, False), (True, False), (True, True)) for sep in (False, True)
                        for k in (3, 4)}
        # both sides of every threshold
        assert M.density_class(1024, "skd") != M.density_class(1025, "skd") and M.use_ff(255) != M.use_ff(256)


def test_the_solve_many_calls_hold_every_problem_and_every_class_count():
    calls = M.solve_many_calls()
    assert len(calls) == 5
    assert sum(len(probs) for _, probs in calls[:4]) == 80 and all(len(probs) >= 16 for _, probs in calls)
    assert len({tuple(cfg[f] for f in M.CONFIG_KEY) for cfg, _ in calls}) == 5
    assert {cfg["algo"] for cfg, _ in calls} == {"ncem", "nem"}
    assert (calls[4][0]["algo"], calls[4][0]["tie"]) == ("ncem", "libc")
    assert all(cfg["it_max"] >= 3 and not cfg["param_fix"] for cfg, _ in calls)
    for cfg, probs in calls:
        assert len({p[2] for p in probs}) >= 5
        assert any(p[1] is None for p in probs)
        # a group of three holds problems of different shapes and class counts
        assert any(len({(q[0].shape, q[2]) for q in probs[i:i + 3]}) == 3 for i in range(0, len(probs) - 2, 3))
    assert {p[2] for _, probs in calls for p in probs} == {1, 2, 3, 4, 5, 8, 12}
    assert sum(p[0].shape[0] == 1 for _, probs in calls[:4] for p in probs) == 9
    x = calls[0][1][0][0]
    assert np.array_equal(np.unpackbits(M.as_bit_rows(x).view(np.uint8), axis=1, bitorder="little")[:, :x.shape[1]], x)


def test_the_random_starts_cases():
    assert {(k, d) for k, d, algo in M.STARTS_CASES if algo == "ncem"} == {(k, d) for k in (2, 6, 11) for d in (20, 300)}
    assert {M.sweep_template_k(k) for k, _, _ in M.STARTS_CASES} == {2, 6, 0}
    assert {M.use_ff(d) for _, d, _ in M.STARTS_CASES} == {False, True}
    assert M.STARTS == 6 and all(850 <= M.starts_spec(k, d)["n"] <= 950 for k, d, _ in M.STARTS_CASES)
