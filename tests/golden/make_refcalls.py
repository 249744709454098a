#!/usr/bin/env python3
"""Record the compiled reference's answers to the calls the tests make: tests/golden/refcalls/.

Needs the compiled reference (oracle/_ref/libnem_ref.so: `make -C oracle ref` where the reference's sources are).
The CPU tests that call it (tests/test_oracle_vs_reference.py) run once with NEM_REFERENCE_RECORD=1, which records
every call; the GPU tests' reference calls are made here on the same inputs, built by the tests' own helpers.  Data
only: what the reference returned and the files its nem() wrote.  No reference source text is stored.

    python tests/golden/make_refcalls.py
"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402
from tests import refcalls  # noqa: E402


def gpu_test_calls(ref):
    from tests import test_gpu_dropin_fullsize as fullsize
    from tests import test_gpu_edges as edges
    from tests import test_gpu_golden as golden
    with tempfile.TemporaryDirectory() as tmp:
        for i, case in enumerate(golden.LOG_CASES):
            base, args = golden.log_case(os.path.join(tmp, "log%d" % i), *case)
            assert ref.nem(base, *args) == 0
        for i, case in enumerate(golden.CRIT_CASES):
            base, args = golden.crit_case(os.path.join(tmp, "crit%d" % i), *case)
            assert ref.nem(base, *args) == 0
        _, base = fullsize.configs1_files(os.path.join(tmp, "configs1"))
        assert fullsize._call(ref.nem, base, 3)[0] == 0
    for n, d, k, starts, seed in edges.TIE_STREAM_CASES:
        x, nei = edges.tie_stream_inputs(n, d, seed)
        ref.classify_random(x, nei, k, n_starts=starts, rng_seed=seed, algo="ncem", disper="sk_", beta=0.5, it_max=20)
    n, d, k, seed = fullsize.RANDOM_STARTS_CASE
    x, nei = fullsize.random_starts_inputs(n, d)
    ref.classify_random(x, nei, k, n_starts=50, rng_seed=seed, algo="ncem", disper="sk_", beta=0.5, it_max=100)


def main():
    pyoracle.build(ref=True)
    if not pyoracle.have_reference():
        raise SystemExit("the compiled reference (oracle/_ref) is needed")
    shutil.rmtree(refcalls.REFCALLS, ignore_errors=True)
    env = dict(os.environ, NEM_REFERENCE_RECORD="1")
    subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_oracle_vs_reference.py"],
                   cwd=ROOT, env=env, check=True)
    gpu_test_calls(refcalls.RecordedReference(live=pyoracle.Reference()))
    print("recorded %d calls under %s" % (len([f for f in os.listdir(refcalls.REFCALLS) if f.endswith(".json")]),
                                          os.path.relpath(refcalls.REFCALLS, ROOT)))


if __name__ == "__main__":
    main()
