"""Time the in-flight accounting on the GPU: one batch of 50,000 tracked activation ids with the headline workload's
namespace draw (the invoking namespace of each activation's action), then the completion of that batch, in warm
steady state; and owgs_throttle_batch over 4,095 jobs of the same draw.

Each variant is a libowgs.so (optionally with the checkout its Python package is imported from, for a library of
another commit that lacks the new symbols):

    python tools/time_inflight.py --out profiles/inflight_counts.jsonl \
        parent=/path/to/parent/openwhisk_amd/libowgs.so,/path/to/parent  kept=openwhisk_amd/libowgs.so

Every variant runs in a fresh child process, the variants alternating over `--rounds` rounds so that drift of the
shared host shows up as spread inside every variant instead of as a difference between them.  A call is timed on the
host clock from entry to return; both calls end in a stream synchronisation.  One JSON line per variant: p50, p10, p90
over all rounds' samples and the p50 of each round (microseconds).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 50_000
N_THROTTLE = 4_095


def child(reps, warm):
    sys.path.insert(0, os.environ.get("OWGS_TREE") or ROOT)
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer
    from openwhisk_amd import workload as W

    w = W.config("headline", n_activations=N)
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.register_actions(w.actions)
    L, h = b._L, b._h
    with_ns = hasattr(L, "owgs_track_activations_ns") and hasattr(b, "register_namespaces")
    act = np.ascontiguousarray(w.stream.act[:N], dtype=np.int32)
    names = sorted({a.namespace for a in w.actions})
    index = {s: k for k, s in enumerate(names)}
    draw = np.array([index[w.actions[a].namespace] for a in act], dtype=np.int32)
    rng = np.random.default_rng(9)
    aid = np.frombuffer("".join(W.activation_ids(rng, N)).encode("ascii"), dtype=np.uint8)
    tk = np.arange(N, dtype=np.int32)
    inv = np.zeros(N, dtype=np.int32)
    fl = np.zeros(N, dtype=np.uint8)
    o_t, o_e = np.zeros(N, np.int32), np.zeros(N, np.uint8)
    o_k, o_f = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ns = None
    if with_ns:
        ns = np.ascontiguousarray(b.register_namespaces([0xA11 << 64 | k for k in range(len(names))])[draw])

    def track():
        if with_ns:
            return L.owgs_track_activations_ns(h, N, P(aid), P(act), P(ns), P(tk), P(o_t), P(o_e))
        return L.owgs_track_activations(h, N, P(aid), P(act), P(tk), P(o_t), P(o_e))

    def complete():
        return L.owgs_complete_activations(h, N, P(aid), P(inv), P(fl), P(o_k), P(o_t), P(o_f))

    t_track, t_done, t_thr = [], [], []
    for r in range(warm + reps):
        t0 = time.perf_counter_ns()
        rc1 = track()
        t1 = time.perf_counter_ns()
        rc2 = complete()
        t2 = time.perf_counter_ns()
        assert rc1 == 0 and rc2 == 0 and not o_e.any() and np.all(o_k == 3), (rc1, rc2)
        if r >= warm:
            t_track.append((t1 - t0) / 1e3)
            t_done.append((t2 - t1) / 1e3)
    if with_ns:
        assert not b.active_activations_for(np.arange(len(names))).any() and b.activation_totals() == (0, 0, 0)
        track()  # the throttle check reads the counters of a tracked batch
        q_ns = np.ascontiguousarray(ns[:N_THROTTLE])
        q_lim = np.full(N_THROTTLE, 100, dtype=np.int32)
        q_c, q_ok = np.zeros(N_THROTTLE, np.int32), np.zeros(N_THROTTLE, np.uint8)
        for r in range(warm + reps):
            t0 = time.perf_counter_ns()
            rc = L.owgs_throttle_batch(h, N_THROTTLE, P(q_ns), P(q_lim), P(q_c), P(q_ok))
            t1 = time.perf_counter_ns()
            assert rc == 0, rc
            if r >= warm:
                t_thr.append((t1 - t0) / 1e3)
    print(json.dumps({"track_us": t_track, "complete_us": t_done, "throttle_us": t_thr,
                      "namespaces": len(names), "hottest_share": float(np.bincount(draw).max()) / N,
                      "counted": bool(with_ns)}), flush=True)


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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
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
    lines = []
    for label, lib, _ in variants:
        rs = got[label]
        row = {"what": "inflight_counts", "variant": label, "n": N, "namespaces": rs[0]["namespaces"],
               "hottest_namespace_share": round(rs[0]["hottest_share"], 4), "counted": rs[0]["counted"],
               "unit": "us per call, host clock, entry to return (ends in a stream synchronisation)",
               "track": summary([r["track_us"] for r in rs]), "complete": summary([r["complete_us"] for r in rs])}
        if rs[0]["throttle_us"]:
            row["throttle_n"] = N_THROTTLE
            row["throttle"] = summary([r["throttle_us"] for r in rs])
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
