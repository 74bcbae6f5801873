"""Time publish end to end on the GPU: owgs_publish_activations against the three calls it replaces, in warm steady
state on the headline draw over 10,000 healthy invokers, for n = 128, 512 and 4,095 activations per drained batch.

Legs (host clock from entry to return, microseconds):
    A   owgs_publish_batch + owgs_track_activations_timed (on the placed subset, which the caller filters) +
        owgs_serialize_activations; its three halves are timed inside the same calls
    A2  the first two of those alone
    B   owgs_publish_activations with msgs
    B2  owgs_publish_activations without
After every call the tracked activations are completed (forced, untimed), so the pool and the table stay in steady state.

Each variant is a libowgs.so (optionally with the checkout its Python package is imported from, for a library of
another commit that lacks the new symbol and is then timed on A and A2 only):

    python tools/time_publish.py --out profiles/publish_pipeline.jsonl \
        parent=/path/to/parent/openwhisk_amd/libowgs.so,/path/to/parent  kept=openwhisk_amd/libowgs.so

Every variant runs in a fresh child process, the variants alternating over `--rounds` rounds so that drift of the
shared host shows up as spread inside every variant instead of as a difference between them.  One JSON line per variant
and batch size: p50, p10, p90 over all rounds' samples and the p50 of each round; then one line per batch size
comparing the first variant's A / A2 with the last variant's B / B2.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (128, 512, 4_095)
N_INVOKERS = 10_000


def child(reps, warm):
    sys.path.insert(0, os.environ.get("OWGS_TREE") or ROOT)
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
    from openwhisk_amd import workload as W

    w = W.config("headline", n_activations=max(SIZES), n_invokers=N_INVOKERS)
    healthy = np.zeros(len(w.inv_ids), np.uint8)   # the headline's action draw, every invoker healthy
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, healthy)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    b.register_templates(['"action":{"path":"%s","name":"a"},"revision":null,"user":{"subject":"u%d"}' % (a.path, k)
                          for k, a in enumerate(w.actions)], ["[]"] * len(w.actions))
    L, h = b._L, b._h
    fused = hasattr(L, "owgs_publish_activations") and hasattr(_lib, "owgs_publish_io")
    if fused:
        L.owgs_publish_activations.restype = C.c_int
        L.owgs_publish_activations.argtypes = [C.c_void_p] * 5
    names = sorted({a.namespace for a in w.actions})
    handles = b.register_namespaces([0xA11 << 64 | k for k in range(len(names))])
    index = {s: k for k, s in enumerate(names)}
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(9)
    out = {"fused": bool(fused), "sizes": {}}
    seq = 0
    for n in SIZES:
        act = np.ascontiguousarray(w.stream.act[:n], dtype=np.int32)
        ns = np.ascontiguousarray(handles[[index[w.actions[a].namespace] for a in act]], dtype=np.int32)
        aids = W.activation_ids(rng, n)
        a32 = np.frombuffer("".join(aids).encode("ascii"), np.uint8).reshape(n, 32).copy()
        words = np.array([(int(a[:16], 16), int(a[16:], 16)) for a in aids], dtype=np.uint64).reshape(-1)
        tks = np.arange(n, dtype=np.int32)
        lims = np.full(n, 60_000, np.int64)
        inv, fl = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        otk, oex = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        tid = np.frombuffer(b"".join(b"sid_%07d" % k for k in range(n)) + b"\0", np.uint8).copy()
        tid_off = (np.arange(n + 1, dtype=np.int64) * 11)
        tstart = np.arange(n, dtype=np.int64) + 1_700_000_000_000
        mfl = np.zeros(n, np.uint8)
        cap = 1024 * n
        obuf = C.create_string_buffer(cap)
        ooff, oord, otop = np.zeros(n + 1, np.int64), np.zeros(n, np.int32), np.zeros(N_INVOKERS + 1, np.int32)
        total, mm = C.c_int64(0), C.c_int32(0)
        summ = np.zeros(8, np.int64)
        ck, ct, cf = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        forced = np.ones(n, np.uint8)
        B_ser = _lib.owgs_msg_batch(n, P(inv), P(act), P(words), P(tid), P(tid_off), P(tstart), P(mfl))
        if fused:
            B_fused = _lib.owgs_msg_batch(n, None, P(act), None, P(tid), P(tid_off), P(tstart), P(mfl))
            io = _lib.owgs_publish_io(n, P(act), None, 0, P(words), P(ns), P(tks), P(lims), 0, P(inv), P(fl), P(otk),
                                      P(oex))
            mo = _lib.owgs_msg_out(N_INVOKERS, C.cast(obuf, C.c_void_p), cap, P(ooff), P(oord), P(otop), 0, 0)

        def complete():
            p = np.nonzero(inv >= 0)[0]
            k = len(p)
            rc = L.owgs_complete_activations(h, k, P(np.ascontiguousarray(a32[p])), P(np.ascontiguousarray(inv[p])),
                                             P(forced), P(ck), P(ct), P(cf))
            assert rc == 0 and np.all(ck[:k] == 3), rc

        def three(now, with_msgs):
            t0 = time.perf_counter_ns()
            rc = L.owgs_publish_batch(h, n, P(act), None, seq, P(inv), P(fl))
            t1 = time.perf_counter_ns()
            assert rc == 0, rc
            p = np.nonzero(inv >= 0)[0]   # publish skips setupActivation without an invoker: the caller filters
            k = len(p)
            if k == n:
                rc = L.owgs_track_activations_timed(h, n, P(a32), P(act), P(ns), P(tks), P(inv), P(lims), now, P(otk),
                                                    P(oex))
            else:
                s = [np.ascontiguousarray(x[p]) for x in (a32, act, ns, tks, inv, lims)]
                rc = L.owgs_track_activations_timed(h, k, *[P(x) for x in s], now, P(otk), P(oex))
            t2 = time.perf_counter_ns()
            assert rc == 0, rc
            if with_msgs:
                rc = L.owgs_serialize_activations(h, C.byref(B_ser), N_INVOKERS, obuf, cap, P(ooff), P(oord), P(otop),
                                                  C.byref(total), C.byref(mm))
                assert rc == 0, rc
            t3 = time.perf_counter_ns()
            return [(t3 - t0) / 1e3, (t1 - t0) / 1e3, (t2 - t1) / 1e3, (t3 - t2) / 1e3]

        def one(now, with_msgs):
            io.seq_base, io.now_ms = seq, now
            t0 = time.perf_counter_ns()
            rc = L.owgs_publish_activations(h, C.byref(io), C.byref(B_fused) if with_msgs else None,
                                            C.byref(mo) if with_msgs else None, P(summ))
            t1 = time.perf_counter_ns()
            assert rc == 0 and summ[6] == (3 if with_msgs else 2), (rc, summ)
            return [(t1 - t0) / 1e3]

        res = {"placed_share": 0.0}
        legs = [("A", three, True), ("A2", three, False)] + ([("B", one, True), ("B2", one, False)] if fused else [])
        bytes_of = {}
        for key, fn, with_msgs in legs:
            rows = []
            for r in range(warm + reps):
                v = fn(1_000 + r, with_msgs)
                if with_msgs and r == 0:
                    bytes_of[key] = (obuf.raw[:(mo.total if fn is one else total.value)], ooff.copy())
                seq += n
                complete()
                if r >= warm:
                    rows.append(v)
            cols = list(zip(*rows))
            res[key + "_us"] = list(cols[0])
            if key == "A":
                res["A_publish_us"], res["A_track_us"], res["A_serialize_us"] = (list(c) for c in cols[1:4])
            res["placed_share"] = float((inv >= 0).mean())
        res["bytes_A"] = len(bytes_of["A"][0])
        out["sizes"][str(n)] = res
    print(json.dumps(out), flush=True)


def summary(samples_by_round):
    import numpy as np

    allv = np.concatenate([np.asarray(s, dtype=np.float64) for s in samples_by_round])
    return {"p50": round(float(np.percentile(allv, 50)), 1), "p10": round(float(np.percentile(allv, 10)), 1),
            "p90": round(float(np.percentile(allv, 90)), 1),
            "round_p50": [round(float(np.percentile(s, 50)), 1) for s in samples_by_round], "samples": int(len(allv))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*", help="label=libowgs.so[,checkout to import openwhisk_amd from]")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.warm)
    variants = []
    for v in a.variants or ["kept=" + os.path.join(ROOT, "openwhisk_amd", "libowgs.so")]:
        label, rest = v.split("=", 1)
        lib, _, tree = rest.partition(",")
        variants.append((label, os.path.abspath(lib), os.path.abspath(tree) if tree else ROOT))
    got = {label: [] for label, _, _ in variants}
    for _ in range(a.rounds):
        for label, lib, tree in variants:
            env = dict(os.environ, OWGS_LIB=lib, OWGS_TREE=tree)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                                  "--warm", str(a.warm)], env=env, capture_output=True, text=True, timeout=400)
            if out.returncode != 0:  # nothing more is started after a failure
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(f"variant {label} failed with exit status {out.returncode}")
            got[label].append(json.loads(out.stdout.strip().splitlines()[-1]))
    lines, stat = [], {}
    for n in SIZES:
        for label, _, _ in variants:
            rs = got[label]
            row = {"what": "publish_pipeline", "variant": label, "n": n, "invokers": N_INVOKERS,
                   "placed_share": rs[0]["sizes"][str(n)]["placed_share"],
                   "message_bytes": rs[0]["sizes"][str(n)]["bytes_A"],
                   "unit": "us per call sequence, host clock, entry to return"}
            for key in ("A", "A_publish", "A_track", "A_serialize", "A2", "B", "B2"):
                if key + "_us" in rs[0]["sizes"][str(n)]:
                    row[key] = stat[(label, n, key)] = summary([r["sizes"][str(n)][key + "_us"] for r in rs])
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    first, last = variants[0][0], variants[-1][0]
    for n in SIZES:
        if (last, n, "B") in stat:
            A, A2, B, B2 = (stat[(first, n, "A")], stat[(first, n, "A2")], stat[(last, n, "B")], stat[(last, n, "B2")])
            lines.append(json.dumps({"what": "publish_pipeline_compare", "n": n, "A": f"{first} three calls",
                                     "B": f"{last} owgs_publish_activations", "B_over_A_p50": round(B["p50"] / A["p50"], 3),
                                     "B2_over_A2_p50": round(B2["p50"] / A2["p50"], 3),
                                     "B_p50_below_A_p10": bool(B["p50"] < A["p10"]),
                                     "B2_p50_below_A2_p10": bool(B2["p50"] < A2["p10"])}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
