"""Time the throttle gate's user events on the GPU: owgs_invoke_activations_events against owgs_invoke_activations for
the same drained batch, and owgs_throttle_events alone, in warm steady state on the headline draw over 10,000 healthy
invokers, for a mixed batch of 4,096 items: 15 % triggers, 10 % rejected by the rate throttle, 10 % by the concurrent
throttle, the rest admitted actions.  All legs are the two-stage form (no messages).

Legs (host clock from entry to return, every call ends in a stream synchronisation, microseconds):
    old         owgs_invoke_activations
    events      owgs_invoke_activations_events with the events of the batch (one identity per namespace, printed as
                spray-json would: about 80 bytes of pieces, a 13-byte source)
    standalone  owgs_throttle_events over the outputs of the call before
After every call the tracked activations are completed (forced, untimed), so the pool, the table and the books stay in
steady state, and every call takes a new minute, so the rate records restart.

Each variant is a libowgs.so (optionally with the checkout its Python package is imported from, for a library of
another commit that lacks the new symbols and is then timed on `old` only):

    python tools/time_events.py --out profiles/throttle_events.jsonl \
        parent=/path/to/parent/openwhisk_amd/libowgs.so,/path/to/parent  kept=openwhisk_amd/libowgs.so

Every variant runs in a fresh child process, the variants alternating over `--rounds` rounds so that drift of the
shared host shows up as spread inside every variant instead of as a difference between them: naming the same library
twice (parent=..., parent2=...) measures that spread.  One JSON line per variant: p50, p10, p90 over all rounds'
samples and the p50 of each round; then one line per pair of variants with the ratio of their `old` medians.
`--child` alone runs one process (for a kernel trace around it).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4_096
N_INVOKERS = 10_000
TRIG, RO, CO = 1, 2, 4


def child(reps, warm):
    sys.path.insert(0, os.environ.get("OWGS_TREE") or ROOT)
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
    from openwhisk_amd import workload as W

    n = N
    w = W.config("headline", n_activations=n, n_invokers=N_INVOKERS)
    healthy = np.zeros(len(w.inv_ids), np.uint8)   # the headline's action draw, every invoker healthy
    names = sorted({x.namespace for x in w.actions})
    index = {s: k for k, s in enumerate(names)}
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, healthy)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    handles = b.register_namespaces([0xA11 << 64 | k for k in range(len(names))])
    L, h = b._L, b._h
    has_events = hasattr(L, "owgs_invoke_activations_events") and hasattr(_lib, "owgs_event_io")
    if has_events:
        b.set_event_source('"controller0"')
        b.register_event_identities(
            ['"subject":"user-%04d"' % k for k in range(len(names))],
            ['"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8%04d","namespace":"%s"' % (k, s) for k, s in enumerate(names)])
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(9)
    act = np.ascontiguousarray(w.stream.act[:n], dtype=np.int32)
    ident = np.array([index[w.actions[x].namespace] for x in act], np.int32)
    ns = np.ascontiguousarray(handles[ident], dtype=np.int32)
    aids = W.activation_ids(rng, n)
    a32 = np.frombuffer("".join(aids).encode("ascii"), np.uint8).reshape(n, 32).copy()
    words = np.array([(int(x[:16], 16), int(x[16:], 16)) for x in aids], dtype=np.uint64)
    tks = np.arange(n, dtype=np.int32)
    lims = np.full(n, 60_000, np.int64)
    u = rng.random(n)
    kind = (np.where(u < 0.15, TRIG, 0) | RO | CO).astype(np.uint8)   # every item carries its limits
    ro = np.where((u >= 0.15) & (u < 0.25), 0, 1 << 30).astype(np.int32)      # rate limit 0: rejected
    co = np.where((u >= 0.25) & (u < 0.35), 0, 1 << 30).astype(np.int32)      # concurrent limit 0: rejected
    t_ms = np.zeros(n, np.int64)
    ver, fl, ex = (np.zeros(n, np.uint8) for _ in range(3))
    rc_, rl, cc, cl, inv, tk = (np.zeros(n, np.int32) for _ in range(6))
    summ = np.zeros(16, np.int64)
    io = _lib.owgs_invoke_io(n, P(ns), P(kind), P(t_ms), P(ro), P(co), P(act), None, 0, P(words), P(tks), P(lims), 0,
                             P(ver), P(rc_), P(rl), P(cc), P(cl), P(inv), P(fl), P(tk), P(ex))
    ck, ct, cf = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    forced = np.ones(n, np.uint8)
    if has_events:
        ev_cap, rej_cap = n * (_lib.EVENT_MAX_FIXED + 13 + 160), n * _lib.REJECT_TEXT_MAX
        ev_out, rej_out = C.create_string_buffer(ev_cap), C.create_string_buffer(rej_cap)
        ev_off, rej_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        E = _lib.owgs_event_io(P(ident), C.cast(ev_out, C.c_void_p), ev_cap, P(ev_off), C.cast(rej_out, C.c_void_p),
                               rej_cap, P(rej_off), 0, 0, 0, 0)

    def complete():
        p = np.nonzero(inv >= 0)[0]
        k = len(p)
        rc = L.owgs_complete_activations(h, k, P(np.ascontiguousarray(a32[p])), P(np.ascontiguousarray(inv[p])),
                                         P(forced), P(ck), P(ct), P(cf))
        assert rc == 0 and np.all(ck[:k] == 3), rc

    def old():
        t0 = time.perf_counter_ns()
        rc = L.owgs_invoke_activations(h, C.byref(io), None, None, P(summ))
        t1 = time.perf_counter_ns()
        assert rc == 0 and summ[6] == 2 and summ[15] == 0, (rc, summ)
        return (t1 - t0) / 1e3

    def events():
        t0 = time.perf_counter_ns()
        rc = L.owgs_invoke_activations_events(h, C.byref(io), None, None, C.byref(E), P(summ))
        t1 = time.perf_counter_ns()
        assert rc == 0 and summ[6] == 2 and summ[15] == 1, (rc, summ)
        return (t1 - t0) / 1e3

    def standalone():
        t0 = time.perf_counter_ns()
        rc = L.owgs_throttle_events(h, n, P(kind), P(ver), P(rc_), P(rl), P(cc), P(cl), P(t_ms), C.byref(E))
        t1 = time.perf_counter_ns()
        assert rc == 0, rc
        return (t1 - t0) / 1e3

    out = {"events": bool(has_events)}
    seq, minute = 0, 0
    for key, fn in [("old", old)] + ([("events", events), ("standalone", standalone)] if has_events else []):
        rows = []
        for r in range(warm + reps):
            if fn is not standalone:
                minute += 1
                t_ms[:] = 60_000 * minute + np.arange(n) % 1000       # a new minute for every call
                io.seq_base, io.now_ms = seq, 1_000 + minute
            v = fn()
            if fn is not standalone:
                seq += n
                out["waits"] = int(summ[12])
                out["verdicts"] = [int(summ[8]), int(summ[9]), int(summ[10]), int(summ[11])]
                complete()
            if r >= warm:
                rows.append(v)
        out[key + "_us"] = rows
        if has_events and fn is not old:
            out["event_bytes"], out["text_bytes"] = int(E.ev_total), int(E.rej_total)
            out["n_events"], out["n_texts"] = int(E.n_events), int(E.n_rejects)
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
    for label, _, _ in variants:
        rs = got[label]
        row = {"what": "throttle_events", "variant": label, "n": N, "invokers": N_INVOKERS,
               "admitted_rate_conc_triggers": rs[0]["verdicts"], "waits": rs[0]["waits"],
               "unit": "us per call, host clock, entry to return"}
        for key in ("event_bytes", "text_bytes", "n_events", "n_texts"):
            if key in rs[0]:
                row[key] = rs[0][key]
        for key in ("old", "events", "standalone"):
            if key + "_us" in rs[0]:
                row[key] = stat[(label, key)] = summary([r[key + "_us"] for r in rs])
        if "events" in row:
            row["events_minus_old_p50"] = round(row["events"]["p50"] - row["old"]["p50"], 1)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    for i, (x, _, _) in enumerate(variants):
        for y, _, _ in variants[i + 1:]:
            lines.append(json.dumps({"what": "throttle_events_compare", "leg": "old (owgs_invoke_activations)",
                                     "a": x, "b": y, "b_over_a_p50": round(stat[(y, "old")]["p50"] / stat[(x, "old")]["p50"], 4),
                                     "b_over_a_round_p50": [round(q / p, 4) for p, q in zip(stat[(x, "old")]["round_p50"],
                                                                                              stat[(y, "old")]["round_p50"])]}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
