#!/usr/bin/env python3
"""Two schedules of the E1 fast-forward (nem_kernels.hip), emulated lane for lane on the CPU (no GPU needed): the
word-synchronous chain_ff, where a wave takes ff_word's crossing branch whenever ANY of its 64 lanes leaves its binade in
the wave's current word, and chain_ff_batched, where every lane walks its own row and the wave runs one crossing pass for
all waiting lanes once T of them wait or nobody can advance.

The emulation uses the bench's matrix at configs[1] (synth.ushaped_pa_matrix(20000, 500, 2), the default .m), the
parameters the oracle reaches after 0, 1, 2, 4 and 7 iterations, the engine's lane order (a stable sort of every
256-family tile by popcount), ff_entry's increment tables (nemgpu_ff_table) and the kernels' sequence of operations: 32
stepped organisms, then per word cand / five-probe search / exact step / table reload.  Every schedule's densities are
compared bit for bit with the oracle's.  Per wave it counts words or trips and crossing passes, and prices them with the
instruction counts of NOTES_negative_results.md (192 issue slots for the stepped word, 10 per plain word, 14 per lane
step, 80 per crossing pass; what the device charges is in NOTES_negative_results.md section 15).

    python3 profiles/ff_schedule_model.py [--out profiles/r09_ff_schedule_model.json] [--iterations 0,1,2,4,7]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS_STEPPED, SLOTS_WORD, SLOTS_TRIP, SLOTS_PASS = 192, 10, 14, 80
INVALID = 1 << 23


def popc(v):
    v = v.astype(np.uint64)
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    v = (v + (v >> 4)) & 0x0F0F0F0F
    return ((v * 0x01010101) & 0xFFFFFFFF) >> 24


class Chain:
    """one class's uniform chain over all lanes at once; integers are held in uint64 (true values stay below 2^32)"""

    def __init__(self, lib, eps):
        e = np.float32(eps)
        self.l1 = float(np.log(np.float64((np.float32(1.0) - e) / e)))
        self.l0 = float(np.log(np.float64(np.float32(1.0) - e)))
        q0 = (C.c_uint32 * 256)(); q1 = (C.c_uint32 * 256)()
        assert lib.nemgpu_ff_table(C.c_double(self.l1), C.c_double(self.l0), q0, q1) == 0
        q0 = np.array(list(q0), np.uint64); q1 = np.array(list(q1), np.uint64)
        q1[q0 == INVALID] = INVALID                      # ff_build
        self.Q0, self.DQ = q0, q1 - q0
        self.usable = self.l1 >= 0.0 and self.l0 <= 0.0

    def load(self, bits):
        E = (bits >> np.uint64(23)) & np.uint64(255)
        return self.Q0[E], self.DQ[E], (E + np.uint64(1)) << np.uint64(23)

    def exact(self, bits, bit):
        dk = bits.astype(np.uint32).view(np.float32).astype(np.float64)
        r = ((dk + np.where(bit != 0, self.l1, 0.0)) - self.l0).astype(np.float32)      # nem_mod.c:661
        return r.view(np.uint32).astype(np.uint64)

    def stepped_word(self, m):
        bits = np.zeros(len(m), np.uint64)
        for b in range(32):
            bits = self.exact(bits, (m >> np.uint64(b)) & np.uint64(1))
        return bits

    def cross(self, bits, q0, dq, end, mm, rem):
        """ff_word's crossing step for every lane given: (bits, q0, dq, end, mm, rem) behind it"""
        j = np.zeros(len(bits), np.uint64); at = bits.copy()
        for sh in (4, 3, 2, 1, 0):
            t = j + np.uint64(1 << sh)
            at_t = at + (q0 << np.uint64(sh))
            low = mm & ((np.uint64(1) << t) - np.uint64(1))
            ok = at_t + popc(low) * dq < end
            j = np.where(ok, t, j); at = np.where(ok, at_t, at)
        assert np.all(j < rem)
        low = mm & ((np.uint64(1) << j) - np.uint64(1))
        bits = self.exact(at + popc(low) * dq, (mm >> j) & np.uint64(1))
        q0, dq, end = self.load(bits)
        return bits, q0, dq, end, mm >> (j + np.uint64(1)), rem - (j + np.uint64(1))


def word_synchronous(ch, M, nbs, wave):
    """chain_ff.  M: [lanes][words] mismatch words in lane order; returns (bits, words per wave, passes per wave)"""
    nw = int(wave.max()) + 1
    passes = np.zeros(nw, np.int64)
    bits = ch.stepped_word(M[:, 0])
    q0, dq, end = ch.load(bits)
    for w in range(1, M.shape[1]):
        m = M[:, w].copy(); nb = np.uint64(nbs[w])
        cand = bits + nb * q0 + popc(m) * dq
        crossing = cand >= end
        bits = np.where(crossing, bits, cand)
        idx = np.flatnonzero(crossing)
        mm = m[idx]; rem = np.full(len(idx), nb, np.uint64)
        while len(idx):
            passes[np.unique(wave[idx])] += 1
            b, a, d, e, mm, rem = ch.cross(bits[idx], q0[idx], dq[idx], end[idx], mm, rem)
            c2 = b + rem * a + popc(mm) * d
            done = (rem == 0) | (c2 < e)
            b = np.where((rem > 0) & (c2 < e), c2, b)
            bits[idx], q0[idx], dq[idx], end[idx] = b, a, d, e
            idx, mm, rem = idx[~done], mm[~done], rem[~done]
    return bits, np.full(nw, M.shape[1] - 1, np.int64), passes


def batched(ch, M, nbs, wave, T, S=1):
    """chain_ff_batched with threshold T and S lane steps per wave decision (the first of them decides, the others only
    advance the lanes that fit); returns (bits, lane steps per wave, passes per wave)"""
    n, W = M.shape
    nw = int(wave.max()) + 1
    trips = np.zeros(nw, np.int64); passes = np.zeros(nw, np.int64)
    bits = ch.stepped_word(M[:, 0])
    q0, dq, end = ch.load(bits)
    w = np.ones(n, np.int64)
    mm = M[:, 1].copy(); rem = np.full(n, nbs[1], np.uint64)
    nbs = np.asarray(list(nbs) + [0], np.uint64)
    Mx = np.concatenate([M, np.zeros((n, 1), np.uint64)], axis=1)
    rows = np.arange(n)
    step = 0
    while True:
        active = w < W
        decide = step % S == 0
        if decide and not active.any():
            break
        step += 1
        cand = bits + rem * q0 + popc(mm) * dq
        fits = active & (cand < end)
        waits = active & ~fits
        nwait = np.bincount(wave[waits], minlength=nw); nadv = np.bincount(wave[fits], minlength=nw)
        bits = np.where(fits, cand, bits)
        if decide:
            trips += S * ((nwait + nadv) > 0)                # (a wave leaves its loop at a decision step only)
            run = (nwait >= T) | ((nadv == 0) & (nwait > 0))
        else:
            run = np.zeros(nw, bool)
        passes += run
        idx = np.flatnonzero(waits & run[wave])
        take = fits.copy()
        if len(idx):
            b, a, d, e, m2, r2 = ch.cross(bits[idx], q0[idx], dq[idx], end[idx], mm[idx], rem[idx])
            bits[idx], q0[idx], dq[idx], end[idx], mm[idx], rem[idx] = b, a, d, e, m2, r2
            take[idx] = r2 == 0
        w = w + take
        wc = np.minimum(w, W)
        mm = np.where(take, Mx[rows, wc], mm); rem = np.where(take, nbs[wc], rem)
    return bits, trips, passes


def summary(units, passes, slots_unit):
    slots = SLOTS_STEPPED + slots_unit * units + SLOTS_PASS * passes
    nb = len(slots) // 4
    blk = slots[:nb * 4].reshape(nb, 4).max(axis=1)
    return {"units_per_wave_mean_max": [round(float(units.mean()), 2), int(units.max())],
            "passes_per_wave_mean_max": [round(float(passes.mean()), 2), int(passes.max())],
            "slots_mean_wave": round(float(slots.mean())), "slots_slowest_wave_per_block_median": round(float(np.median(blk))),
            "slots_worst_wave": int(slots.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iterations", default="0,1,2,4,7")
    ap.add_argument("--thresholds", default="16,32,48,64")
    ap.add_argument("--steps", default="1,3", help="lane steps per wave decision")
    ap.add_argument("--families", type=int, default=20000)
    ap.add_argument("--organisms", type=int, default=500)
    args = ap.parse_args()
    from oracle.pyoracle import Oracle
    from pangenomenem_amd import build, synth
    from pangenomenem_amd.engine import load_library
    build.build()
    lib = load_library()
    lib.nemgpu_ff_table.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    n, d, k = args.families, args.organisms, 3
    x, _ = synth.ushaped_pa_matrix(n, d, 2)
    nei = synth.contiguity_graph(n, 2, d=d)
    start = synth.default_init(d)
    orc = Oracle()
    W = (d + 31) // 32
    nbs = [32] * (W - 1) + [d - 32 * (W - 1)]
    xp = np.zeros((n, W * 32), np.uint8); xp[:, :d] = x
    xw = (xp.reshape(n, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    # the engine's lane order: every 256-family tile sorted by popcount, stable
    pc = x.sum(axis=1)
    perm = np.concatenate([t0 + np.argsort(pc[t0:t0 + 256], kind="stable") for t0 in range(0, n, 256)])
    wave = np.arange(n) // 64
    out = {"shape": [n, d, k], "slots": {"stepped_word": SLOTS_STEPPED, "word": SLOTS_WORD, "trip": SLOTS_TRIP, "pass": SLOTS_PASS},
           "units": "word-synchronous: words; batched: lane steps (S per wave decision, each priced as a trip)", "iterations": {}}
    for it in [int(v) for v in args.iterations.split(",")]:
        if it == 0:
            prop, center, disp = start
        else:
            r = orc.run(x, nei, k, *start, algo="ncem", beta=0.5, disper="sk_", cvtest="none", it_max=it, tie="hash")
            prop, center, disp = r["prop"], r["center"], r["disp"]
        _, lp, _ = orc.density(x, prop, center, disp)
        res = {}
        for c in range(k):
            eps = float(disp[c, 0])
            assert np.all(disp[c] == disp[c, 0]) and set(np.unique(center[c])) <= {0.0, 0.5, 1.0}
            ch = Chain(lib, eps)
            # mismatch word: organisms where |x - mu| truncates to 1 (table_entry's am0 / am1)
            a0 = np.abs((0.0 - center[c]).astype(np.int32)) != 0; a1 = np.abs((1.0 - center[c]).astype(np.int32)) != 0
            mis = np.where(xp[:, :d] != 0, a1[None, :], a0[None, :]).astype(np.uint8)
            mp = np.zeros((n, W * 32), np.uint8); mp[:, :d] = mis
            M = (mp.reshape(n, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2)[perm]
            logpk = np.float32(np.log(np.float64(prop[c])))
            want = lp[perm, c]

            def held(bits):
                got = logpk + (-bits.astype(np.uint32).view(np.float32))
                return bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
            rc = {"epsilon": eps}
            bits, units, passes = word_synchronous(ch, M, nbs, wave)
            rc["word_synchronous"] = dict(summary(units, passes, SLOTS_WORD), oracle_bits=held(bits))
            for S in [int(v) for v in args.steps.split(",")]:
                for T in [int(v) for v in args.thresholds.split(",")]:
                    bits, units, passes = batched(ch, M, nbs, wave, T, S)
                    rc["batched_T%d_S%d" % (T, S)] = dict(summary(units, passes, SLOTS_TRIP), oracle_bits=held(bits))
            res["class_%d" % c] = rc
            print("iteration", it, "class", c, json.dumps(rc), file=sys.stderr, flush=True)
        out["iterations"][str(it)] = res
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0 if all(v["oracle_bits"] for r in out["iterations"].values() for c in r.values()
                    for v in c.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
