"""Time the entitlement throttle gate on the GPU: owgs_admit_batch over 512 and 4,095 jobs with the headline
workload's namespace draw (the invoking namespace of each activation's action), against owgs_throttle_batch -- the
concurrent check alone -- over the same jobs, in warm steady state.  The counters the checks read are those of one
tracked batch of 50,000 activations of the same draw.

Each variant is a libowgs.so (optionally with the checkout its Python package is imported from, for a library of
another commit that lacks the new symbols):

    python tools/time_admit.py --out profiles/admit_gate.jsonl \
        parent=/path/to/parent/openwhisk_amd/libowgs.so,/path/to/parent  kept=openwhisk_amd/libowgs.so

A library without owgs_admit_batch is timed on owgs_throttle_batch only.  Every variant runs in a fresh child process,
the variants alternating over `--rounds` rounds so that drift of the shared host shows up as spread inside every
variant instead of as a difference between them.  A call is timed on the host clock from entry to return; every call
ends in a stream synchronisation.  One JSON line per variant and batch size: p50, p10, p90 over all rounds' samples and
the p50 of each round (microseconds); then one line per batch size with the ratio of the last variant's gate to the
first variant's owgs_throttle_batch.

owgs_admit_batch is timed twice: `admit` without override arrays (three uploads: handles, kinds, times) and
`admit_overrides` with both (five uploads, every fourth job carrying its own limits).  Every call of a sample series is
one minute after the previous one, so each starts with fresh counts, as a controller's batches mostly do.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRACK = 50_000
SIZES = (512, 4_095)


def child(reps, warm):
    sys.path.insert(0, os.environ.get("OWGS_TREE") or ROOT)
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer
    from openwhisk_amd import workload as W

    w = W.config("headline", n_activations=N_TRACK)
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.register_actions(w.actions)
    L, h = b._L, b._h
    with_gate = hasattr(L, "owgs_admit_batch") and hasattr(b, "admit_batch")
    act = np.ascontiguousarray(w.stream.act[:N_TRACK], dtype=np.int32)
    names = sorted({a.namespace for a in w.actions})
    index = {s: k for k, s in enumerate(names)}
    draw = np.array([index[w.actions[a].namespace] for a in act], dtype=np.int32)
    ns = np.ascontiguousarray(b.register_namespaces([0xA11 << 64 | k for k in range(len(names))])[draw])
    rng = np.random.default_rng(9)
    b.track_activations(W.activation_ids(rng, N_TRACK), act, np.arange(N_TRACK), ns=ns)
    if with_gate:
        b.set_throttle_limits(60, 60, 100)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = {"namespaces": len(names), "hottest_share": float(np.bincount(draw).max()) / N_TRACK, "gate": bool(with_gate),
           "sizes": {}}
    minute = 28_500_000
    for n in SIZES:
        q_ns = np.ascontiguousarray(ns[:n])
        q_lim = np.full(n, 100, dtype=np.int32)
        q_c, q_ok = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        kind = np.zeros(n, np.uint8)
        kind_ov = np.where(np.arange(n) % 4 == 0, 6, 0).astype(np.uint8)
        ro, co = np.full(n, 120, np.int32), np.full(n, 100, np.int32)
        t_ms = np.zeros(n, np.int64)
        o_v, o_i = np.zeros(n, np.uint8), np.zeros((4, n), np.int32)
        res = {"throttle_us": [], "admit_us": [], "admit_overrides_us": [], "rate_rejected": 0.0}
        for r in range(warm + reps):
            t0 = time.perf_counter_ns()
            rc = L.owgs_throttle_batch(h, n, P(q_ns), P(q_lim), P(q_c), P(q_ok))
            t1 = time.perf_counter_ns()
            assert rc == 0, rc
            if r >= warm:
                res["throttle_us"].append((t1 - t0) / 1e3)
        for key, kd, a_ro, a_co in (("admit_us", kind, None, None), ("admit_overrides_us", kind_ov, P(ro), P(co))):
            if not with_gate:
                break
            for r in range(warm + reps):
                minute += 1
                t_ms[:] = minute * 60_000 + np.arange(n) % 60_000
                t0 = time.perf_counter_ns()
                rc = L.owgs_admit_batch(h, n, P(q_ns), P(kd), P(t_ms), a_ro, a_co, P(o_v), P(o_i[0]), P(o_i[1]),
                                        P(o_i[2]), P(o_i[3]))
                t1 = time.perf_counter_ns()
                assert rc == 0, rc
                if r >= warm:
                    res[key].append((t1 - t0) / 1e3)
            if key == "admit_us":
                res["rate_rejected"] = float((o_v == 1).mean())
                # with equal limits and nothing rate-rejected before it, a job's concurrent verdict is the old check's
                keep = o_v != 1
                assert np.array_equal(o_i[2][keep] < 100, o_v[keep] == 0)
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
    lines, p50 = [], {}
    for n in SIZES:
        for label, _, _ in variants:
            rs = got[label]
            row = {"what": "admit_gate", "variant": label, "n": n, "namespaces": rs[0]["namespaces"],
                   "hottest_namespace_share": round(rs[0]["hottest_share"], 4),
                   "unit": "us per call, host clock, entry to return (ends in a stream synchronisation)",
                   "throttle": summary([r["sizes"][str(n)]["throttle_us"] for r in rs])}
            p50[(label, n, "throttle")] = row["throttle"]["p50"]
            if rs[0]["gate"]:
                row["rate_rejected_share"] = round(rs[0]["sizes"][str(n)]["rate_rejected"], 4)
                for key in ("admit", "admit_overrides"):
                    row[key] = summary([r["sizes"][str(n)][key + "_us"] for r in rs])
                    p50[(label, n, key)] = row[key]["p50"]
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    first, last = variants[0][0], variants[-1][0]
    for n in SIZES:
        if (last, n, "admit") in p50:
            base = p50[(first, n, "throttle")]
            lines.append(json.dumps({"what": "admit_gate_ratio", "n": n, "of": f"{last} owgs_admit_batch p50",
                                     "to": f"{first} owgs_throttle_batch p50",
                                     "admit": round(p50[(last, n, "admit")] / base, 3),
                                     "admit_overrides": round(p50[(last, n, "admit_overrides")] / base, 3)}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
