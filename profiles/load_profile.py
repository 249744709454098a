#!/usr/bin/env python3
"""Times for profiles/load.md: loading a synthetic set of GFF files and its families table (loader.synth_files ->
loader.load_files / Master.from_files; needs the GPU).  The set is generated from a seed under a temporary directory,
its bytes are stated.  One warm-up load, then --repeat loads; of each load the host clocks that loader._load keeps (the
file reads, the device calls -- each ends in a synchronise -- and the host steps after them) and the device's own stage
times (hip events around the stages of every batch, summed over the batches).  Rates are the GFF text's bytes over a
stage's time; the HBM bound is the bytes a stage must at least read over 6.3 TB/s (MI355X_MICROARCH's measured copy
rate), the text once.  Then Master.from_files as a whole, and the plain-Python statement load_arrays_host on the first
--host-organisms organisms of the same set.  Writes profiles/load.md (or --out) and prints one JSON line.

    python profiles/load_profile.py --organisms 2000 --genes 4000
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from pangenomenem_amd import loader  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def contigs_of(genes):
    """a chromosome and two plasmids"""
    small = max(genes // 40, 1)
    return [genes - 2 * small, small, small]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--organisms", type=int, default=2000)
    ap.add_argument("--genes", type=int, default=4000)
    ap.add_argument("--families", type=int, default=12000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-organisms", type=int, default=20)
    ap.add_argument("--batch-bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=os.path.join(HERE, "load.md"))
    a = ap.parse_args()
    from pangenomenem_amd import engine
    from pangenomenem_amd.chunks import Master
    if engine.device_count() <= 0:
        raise SystemExit("load_profile: no HIP device visible")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        orgs, fams, text_bytes = loader.synth_files(d, [contigs_of(a.genes)] * a.organisms, n_families=a.families, seed=a.seed,
                                                    shuffle_starts=False)
        made = time.perf_counter() - t0
        fam_bytes = os.path.getsize(fams)
        genes = a.organisms * a.genes
        loader.load_files(orgs, fams, lim_occurence=3, batch_bytes=a.batch_bytes)                # (warm-up: code objects, the page cache)
        runs = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            ld = loader.load_files(orgs, fams, lim_occurence=3, batch_bytes=a.batch_bytes)
            wall = time.perf_counter() - t0
            runs.append(dict(wall_s=wall, **{k: v for k, v in ld.timing.items()}))
        assert len(ld.orders["genes"]) == genes
        med = lambda f: statistics.median(f(r) for r in runs)
        spread = lambda f: (min(f(r) for r in runs), max(f(r) for r in runs))
        stage = {s: med(lambda r: r["device_stage_ms"][s]) * 1e-3 for s in loader.STAGES}
        t0 = time.perf_counter()
        m = Master.from_files(orgs, fams, lim_occurence=3, batch_bytes=a.batch_bytes)
        n, dd, nnz, _ = m.shape()
        master_s = time.perf_counter() - t0
        m.close()
        # the statement on a smaller set: the first organisms of the same one
        with open(orgs) as f:
            few = f.read().splitlines()[:a.host_organisms]
        small = os.path.join(d, "few.tsv")
        with open(small, "w") as f:
            f.write("\n".join(few) + "\n")
        small_bytes = sum(os.path.getsize(os.path.join(d, line.split("\t")[1])) for line in few)
        t0 = time.perf_counter()
        hs = loader.load_arrays_host(small, fams)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ds = loader.load_files(small, fams)
        dev_small_s = time.perf_counter() - t0
        assert all((hs.arrays()[k] == v).all() for k, v in ds.arrays().items())
    wall = med(lambda r: r["wall_s"])
    out = dict(organisms=a.organisms, genes_per_organism=a.genes, genes=genes, families=a.families, gff_bytes=text_bytes, families_bytes=fam_bytes,
               batch_bytes=a.batch_bytes, generate_s=made, repeat=a.repeat, load_wall_s=wall, load_wall_spread_s=spread(lambda r: r["wall_s"]),
               host_read_s=med(lambda r: r["host_read_s"]), device_calls_s=med(lambda r: r["batch_s"]), host_after_s=med(lambda r: r["host_finish_s"]),
               number_s=med(lambda r: r.get("number_s", 0.0)), device_stage_s=stage, master_from_files_s=master_s, master_shape=[n, dd, nnz],
               host_statement=dict(organisms=len(few), gff_bytes=small_bytes, load_arrays_host_s=host_s, load_files_s=dev_small_s))
    print(json.dumps(out))
    gb = text_bytes / 1e9
    lines = ["# Loading the GFF files and the families table: measured", "",
             "Written by `profiles/load_profile.py` on an MI355X (one GPU). No figure here had been measured before this run.", "",
             "The set: %d organisms x %d genes = %d CDS lines, %d families; %.3f GB of GFF text (%d bytes) and %.1f MB of families table,"
             % (a.organisms, a.genes, genes, a.families, gb, text_bytes, fam_bytes / 1e6),
             "synthetic (`loader.synth_files`, seed %d), in a temporary directory, read through the page cache (the files were written" % a.seed,
             "moments before: this is not a cold read from disk). Batches of %d MiB. Median of %d loads after one warm-up;" % (a.batch_bytes >> 20, a.repeat),
             "the whole load took between %.2f and %.2f s." % spread(lambda r: r["wall_s"]), "",
             "| part of `load_files` | seconds | GB/s of GFF text | share of the load |", "|---|---|---|---|"]
    for name, sec in (("whole load (host clock)", wall), ("host: reading the files and joining a batch", out["host_read_s"]),
                      ("device calls (upload, kernels, download; each ends in a synchronise)", out["device_calls_s"]),
                      ("host: after the batches (pragmas, concatenation, names, the numbering call)", out["host_after_s"])):
        lines.append("| %s | %.3f | %.2f | %.0f %% |" % (name, sec, gb / sec if sec > 0 else float("nan"), 100 * sec / wall))
    lines += ["", "The device calls by stage (hip events, summed over the batches; the bound: the text read once at %.1f TB/s = %.2f ms):"
              % (HBM_BYTES_PER_S / 1e12, 1e3 * text_bytes / HBM_BYTES_PER_S), "",
              "| stage | seconds | GB/s of GFF text | x the HBM bound |", "|---|---|---|---|"]
    for s in loader.STAGES:
        sec = stage[s]
        lines.append("| %s | %.4f | %.1f | %.0f |" % (s, sec, gb / sec if sec > 0 else float("nan"), sec / (text_bytes / HBM_BYTES_PER_S)))
    kernels = sum(stage[s] for s in loader.STAGES if s not in ("upload", "gather_download"))
    lines += ["", "A stage's time includes the device allocations it makes and, where a count sizes the next array, a wait for that count.",
              "`upload` is the host-to-device copy of the text from pageable memory and `gather_download` ends with nothing but the error word;",
              "the arrays come back in `nemgpu_gff_fetch`, inside the device calls' host clock. The kernels proper (lines, parse, contigs and IDs,",
              "sort) took %.4f s = %.1f %% of the load; %.2e genes per second for the whole load, %.2e over the kernels alone."
              % (kernels, 100 * kernels / wall, genes / wall, genes / kernels if kernels > 0 else float("nan")), "",
              "Host file reading and batch joining is %.0f %% of the load, everything on the host together %.0f %%. %s"
              % (100 * out["host_read_s"] / wall, 100 * (wall - kernels) / wall,
                 "The device stages do not matter next to the file read and the host's copies: a faster kernel would not show in the total."
                 if kernels < 0.25 * wall else "The device stages are a visible part of the total."), "",
             "`Master.from_files` on the same set (the load, then `Master.from_orders`): %.2f s; the master has %d families, %d organisms, %d CSR entries."
             % (master_s, n, dd, nnz), "",
             "The plain-Python statement `load_arrays_host` on the first %d organisms of the same set (%.1f MB of GFF text), same machine: %.2f s;"
             % (len(few), small_bytes / 1e6, host_s),
             "`load_files` on those: %.2f s (families table of the whole set in both). The reference's own loader was not timed: it does not exist on this machine."
             % dev_small_s, ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
