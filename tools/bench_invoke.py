"""Time the gated publish on the GPU: owgs_invoke_activations against the calls it replaces -- owgs_admit_batch, the
caller's filter of the admitted actions (numpy) and owgs_publish_activations over them -- in warm steady state on the
headline draw over 10,000 healthy invokers, for drained batches of 512 and 4,096 jobs of which 10 % are rejected by the
rate throttle.  Both legs are the two-stage form (no messages): what differs between them is the seam, not the
serialiser.

    python tools/bench_invoke.py --out profiles/invoke_fused.jsonl

One process, two contexts with the same seed: context F takes the fused call, context S the separate calls, on the same
inputs and sequence numbers, alternating call by call so that drift of the shared host shows up as spread inside both
legs instead of as a difference between them.  After every call the tracked activations are completed (forced,
untimed), so the pool, the table and the books are back in the same state; the outputs of the two legs are compared after
every call (untimed) and the run fails if they ever differ.  Host clock from entry to return (every call ends in a
stream synchronisation), microseconds.  One JSON line per batch size: p50 / p99 / p10 / p90 of both legs, the separate
leg's three parts, and the ratio of the medians.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (512, 4_096)
N_INVOKERS = 10_000
REJECTED = 0.10
RO, CO = 2, 4


def pct(v):
    import numpy as np

    return {k: round(float(np.percentile(v, q)), 1) for k, q in (("p50", 50), ("p99", 99), ("p10", 10), ("p90", 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
    from openwhisk_amd import workload as W

    w = W.config("headline", n_activations=max(SIZES), n_invokers=N_INVOKERS)
    healthy = np.zeros(len(w.inv_ids), np.uint8)   # the headline's action draw, every invoker healthy
    names = sorted({x.namespace for x in w.actions})
    index = {s: k for k, s in enumerate(names)}
    ctxs = []
    for _ in range(2):
        b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                             rng_seed=w.rng_seed)
        b.update_invokers_arrays(w.inv_ids, w.inv_mem, healthy)
        b.update_cluster(w.cluster_size)
        b.register_actions(w.actions)
        handles = b.register_namespaces([0xA11 << 64 | k for k in range(len(names))])
        ctxs.append(b)
    (bF, bS), L = ctxs, ctxs[0]._L
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(9)
    lines = []
    seq = 0
    for n in SIZES:
        act = np.ascontiguousarray(w.stream.act[:n], dtype=np.int32)
        ns = np.ascontiguousarray(handles[[index[w.actions[x].namespace] for x in act]], dtype=np.int32)
        aids = W.activation_ids(rng, n)
        a32 = np.frombuffer("".join(aids).encode("ascii"), np.uint8).reshape(n, 32).copy()
        words = np.array([(int(x[:16], 16), int(x[16:], 16)) for x in aids], dtype=np.uint64)
        tks = np.arange(n, dtype=np.int32)
        lims = np.full(n, 60_000, np.int64)
        kind = np.full(n, RO | CO, np.uint8)       # every item carries its limits: the rejected ones a rate limit of 0
        ro = np.where(rng.random(n) < REJECTED, 0, 1 << 30).astype(np.int32)
        co = np.full(n, 1 << 30, np.int32)
        t_ms = np.zeros(n, np.int64)
        o = {k: [np.zeros(n, np.uint8) for _ in range(3)] + [np.zeros(n, np.int32) for _ in range(6)] for k in "FS"}
        summF, summS = np.zeros(16, np.int64), np.zeros(8, np.int64)
        vF, flF, exF, rcF, rlF, ccF, clF, invF, tkF = o["F"]
        vS, flS, exS, rcS, rlS, ccS, clS, invS, tkS = o["S"]
        io = _lib.owgs_invoke_io(n, P(ns), P(kind), P(t_ms), P(ro), P(co), P(act), None, 0, P(words), P(tks), P(lims),
                                 0, P(vF), P(rcF), P(rlF), P(ccF), P(clF), P(invF), P(flF), P(tkF), P(exF))
        ck, ct, cf = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        forced = np.ones(n, np.uint8)

        def complete(b, ids, inv):
            k = len(ids)
            rc = L.owgs_complete_activations(b._h, k, P(np.ascontiguousarray(a32[ids])),
                                             P(np.ascontiguousarray(inv[ids])), P(forced), P(ck), P(ct), P(cf))
            assert rc == 0 and np.all(ck[:k] == 3), rc

        def fused(now):
            io.seq_base, io.now_ms = seq, now
            t0 = time.perf_counter_ns()
            rc = L.owgs_invoke_activations(bF._h, C.byref(io), None, None, P(summF))
            t1 = time.perf_counter_ns()
            assert rc == 0 and summF[6] == 2, (rc, summF)
            return (t1 - t0) / 1e3

        def separate(now):
            t0 = time.perf_counter_ns()
            rc = L.owgs_admit_batch(bS._h, n, P(ns), P(kind), P(t_ms), P(ro), P(co), P(vS), P(rcS), P(rlS), P(ccS),
                                    P(clS))
            t1 = time.perf_counter_ns()
            assert rc == 0, rc
            adm = np.nonzero(((kind & 1) == 0) & (vS == 0))[0]   # the caller filters the batch on the CPU
            k = len(adm)
            s = [np.ascontiguousarray(x[adm]) for x in (act, words, ns, tks, lims)]
            oi, of_, ot, oe = np.empty(k, np.int32), np.empty(k, np.uint8), np.empty(k, np.int32), np.empty(k, np.uint8)
            pio = _lib.owgs_publish_io(k, P(s[0]), None, seq, P(s[1]), P(s[2]), P(s[3]), P(s[4]), now, P(oi), P(of_),
                                       P(ot), P(oe))
            t2 = time.perf_counter_ns()
            rc = L.owgs_publish_activations(bS._h, C.byref(pio), None, None, P(summS))
            t3 = time.perf_counter_ns()
            assert rc == 0, rc
            invS[:], flS[:], tkS[:], exS[:] = _lib.NOT_PUBLISHED, 0, -1, 0   # (untimed: only for the comparison below)
            invS[adm], flS[adm], tkS[adm], exS[adm] = oi, of_, ot, oe
            return [(t3 - t0) / 1e3, (t1 - t0) / 1e3, (t2 - t1) / 1e3, (t3 - t2) / 1e3]

        rowsF, rowsS = [], []
        for r in range(a.warm + a.reps):
            t_ms[:] = 60_000 * (r + 1) + np.arange(n) % 1000      # a new minute for every call
            order = (fused, separate) if r % 2 == 0 else (separate, fused)
            got = {fn: fn(1_000 + r) for fn in order}
            for x, y in zip(o["F"], o["S"]):
                assert np.array_equal(x, y), "the fused call and the separate calls disagree"
            assert summF[:6].tolist() == summS[:6].tolist()
            seq += n
            placed = np.nonzero(invF >= 0)[0]
            complete(bF, placed, invF)
            complete(bS, placed, invS)
            if r >= a.warm:
                rowsF.append(got[fused])
                rowsS.append(got[separate])
        cols = list(zip(*rowsS))
        row = {"what": "invoke_fused", "n": n, "invokers": N_INVOKERS, "rejected_share": round(float((vF != 0).mean()), 3),
               "admitted": int(summF[8]), "placed": int(summF[0]), "waits_fused": int(summF[12]), "calls_per_leg": a.reps,
               "unit": "us per call sequence, host clock, entry to return", "outputs_equal": True,
               "fused": pct(rowsF), "separate": pct(cols[0]), "separate_admit": pct(cols[1]),
               "separate_filter": pct(cols[2]), "separate_publish": pct(cols[3])}
        row["fused_over_separate_p50"] = round(row["fused"]["p50"] / row["separate"]["p50"], 3)
        row["fused_p50_below_separate_p10"] = bool(row["fused"]["p50"] < row["separate"]["p10"])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
