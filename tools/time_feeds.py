"""Time the supervision feeds on the GPU: what one ack batch and one ping batch cost from entry
to return, with the events built on the device against the older two-call path.

  acks   A  owgs_process_acks, the host filter that builds the four event arrays from its outcomes, then
            owgs_health_events(apply = 0) -- the only path a library without the feeds has
         B  owgs_process_acks_supervised(apply = 2)
         at n = 128 (the feed's batch, LB:94-108) and n = 4,095, on the headline draw with a Healthy pool: every call
         completes n freshly published and tracked activations, all Success, so nothing changes and B hands nothing over
  pings  A  owgs_health_events over host-parsed (instance, time, bytes) arrays (the parse itself is not timed)
         B  owgs_process_pings(apply = 0) over the raw messages
         at n = 128 and n = 10,000

Each variant is a libowgs.so (optionally with the checkout its Python package is imported from, for a library of
another commit that lacks the new symbols):

    python tools/time_feeds.py --out profiles/supervision_feeds.jsonl \
        parent=/path/to/parent/openwhisk_amd/libowgs.so,/path/to/parent  kept=openwhisk_amd/libowgs.so

A library without the feeds is timed on path A only; one with them on both (A on the new library shows what the
refactor of owgs_health_events cost).  Every variant runs in a fresh child process, the variants alternating over
`--rounds` rounds so that drift of the shared host shows up as spread inside every variant instead of as a difference
between them.  A call is timed on the host clock from entry to return; every call ends in a stream synchronisation.
For path A two figures are kept: `two_call` with the numpy filter between the calls (what a shim pays in some form) and
`two_call_native`, the two native calls alone -- the comparison that favours A; `process_acks` and `health_events` are
its two halves on their own.  One JSON line per variant, feed and batch size: p50, p10, p90 over all rounds' samples
and the p50 of each round (microseconds); then one line per feed and size with the ratio of the last variant's B to the
first variant's A.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACK_SIZES = (128, 4_095)
PING_SIZES = (128, 10_000)
H = 1700000000123
MAX_ID = 1 << 24


def child(reps, warm):
    sys.path.insert(0, os.environ.get("OWGS_TREE") or ROOT)
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer
    from openwhisk_amd import workload as W

    w = W.config("headline", n_activations=60_000)
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    b.set_health_tid(H)
    L, h = b._L, b._h
    feeds = hasattr(L, "owgs_process_acks_supervised") and hasattr(b, "process_acks_supervised")
    n_inv = len(w.inv_ids)
    ids = np.arange(n_inv, dtype=np.int32)
    # a Healthy pool through the FSM: a ping and a Success per invoker, handed to the scheduler
    b.health_events(ids, np.zeros(n_inv, np.uint8), np.zeros(n_inv, np.int64), w.inv_mem, 0)
    b.health_events(ids, np.ones(n_inv, np.uint8), np.ones(n_inv, np.int64), w.inv_mem, 1, apply=True)
    assert (b.health_read()[0] == 0).all()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(9)
    out = {"feeds": bool(feeds), "invokers": n_inv, "acks": {}, "pings": {}}
    now, seq, cur = 10, 0, 0

    def batch(n):
        """n fresh activations published and tracked; their ack messages (all Success) as one byte buffer."""
        nonlocal seq, cur
        if cur + n > len(w.stream.act):
            cur = 0
        acts = np.ascontiguousarray(w.stream.act[cur:cur + n], dtype=np.int32)
        cur += n
        inv, _ = b.publish(acts, seq_base=seq)
        seq += n
        ok = np.flatnonzero(inv >= 0)
        aids = W.activation_ids(rng, len(ok))
        b.track_activations(aids, acts[ok], ok)
        msgs = [W.completion_message(a, int(i)) for a, i in zip(aids, inv[ok])]
        off = np.zeros(len(msgs) + 1, np.int64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return len(msgs), np.frombuffer(b"".join(msgs) + b"\0", np.uint8), off

    for n in ACK_SIZES:
        kind, inv, tk, fl = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        summ = np.zeros(3, np.int32)
        res = {"two_call_us": [], "two_call_native_us": [], "process_acks_us": [], "health_events_us": [],
               "supervised_us": [], "events": 0}
        for mode in ("two_call", "supervised"):
            if mode == "supervised" and not feeds:
                break
            for r in range(warm + reps):
                m, buf, off = batch(n)
                now += 1
                if mode == "two_call":
                    t0 = time.perf_counter_ns()
                    rc = L.owgs_process_acks(h, m, P(buf), P(off), P(kind), P(inv), P(tk), P(fl))
                    t1 = time.perf_counter_ns()
                    k, i = kind[:m], inv[:m]
                    sel = ((k == 3) | (k == 4)) & (i >= 0) & (i < MAX_ID)
                    e_inv = np.ascontiguousarray(i[sel])
                    e_kind = np.where(fl[:m][sel] & 1, 2, 1).astype(np.uint8)
                    e_t = np.full(len(e_inv), now, np.int64)
                    e_mem = np.zeros(len(e_inv), np.int64)
                    t2 = time.perf_counter_ns()
                    rc2 = L.owgs_health_events(h, len(e_inv), P(e_inv), P(e_kind), P(e_t), P(e_mem), now, 0)
                    t3 = time.perf_counter_ns()
                    assert rc == 0 and rc2 == 0, (rc, rc2)
                    fed = len(e_inv)
                    if r >= warm:
                        res["two_call_us"].append((t3 - t0) / 1e3)
                        res["two_call_native_us"].append((t1 - t0 + t3 - t2) / 1e3)
                        res["process_acks_us"].append((t1 - t0) / 1e3)
                        res["health_events_us"].append((t3 - t2) / 1e3)
                else:
                    t0 = time.perf_counter_ns()
                    rc = L.owgs_process_acks_supervised(h, m, P(buf), P(off), P(kind), P(inv), P(tk), P(fl), now, 2,
                                                        P(summ))
                    t1 = time.perf_counter_ns()
                    assert rc == 0 and summ[1] == 0, (rc, summ)
                    fed = int(summ[0])
                    if r >= warm:
                        res["supervised_us"].append((t1 - t0) / 1e3)
                assert fed == m and (kind[:m] == 3).all()
                res["events"] = fed
        out["acks"][str(n)] = res
    assert (b.health_read()[0] == 0).all() and b.activations_live() == 0

    for n in PING_SIZES:
        inst = (np.arange(n) % n_inv).astype(np.int32)
        msgs = [('{"name":{"instance":%d,"userMemory":"%d MB"}}' % (i, w.inv_mem[i] >> 20)).encode("ascii")
                for i in inst]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        buf = np.frombuffer(b"".join(msgs) + b"\0", np.uint8)
        e_kind, e_mem = np.zeros(n, np.uint8), np.ascontiguousarray(w.inv_mem[inst], dtype=np.int64)
        kind, o_inst, o_mem, summ = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(3, np.int32)
        res = {"health_events_us": [], "process_pings_us": []}
        for mode in ("health_events", "process_pings"):
            if mode == "process_pings" and not feeds:
                break
            for r in range(warm + reps):
                now += 1
                t = np.full(n, now, np.int64)
                t0 = time.perf_counter_ns()
                if mode == "health_events":
                    rc = L.owgs_health_events(h, n, P(inst), P(e_kind), P(t), P(e_mem), now, 0)
                else:
                    rc = L.owgs_process_pings(h, n, P(buf), P(off), P(t), now, 0, P(kind), P(o_inst), P(o_mem), P(summ))
                t1 = time.perf_counter_ns()
                assert rc == 0, rc
                if mode == "process_pings":
                    assert summ[0] == n and np.array_equal(o_inst, inst) and np.array_equal(o_mem, e_mem)
                if r >= warm:
                    res[mode + "_us"].append((t1 - t0) / 1e3)
        out["pings"][str(n)] = res
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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warm", type=int, default=10)
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
    unit = "us per call, host clock, entry to return (ends in a stream synchronisation)"
    lines, p50 = [], {}
    for feed, sizes, keys in (("acks", ACK_SIZES, ("two_call", "two_call_native", "process_acks", "health_events", "supervised")),
                              ("pings", PING_SIZES, ("health_events", "process_pings"))):
        for n in sizes:
            for label, _, _ in variants:
                rs = got[label]
                row = {"what": "supervision_feeds", "feed": feed, "variant": label, "n": n,
                       "invokers": rs[0]["invokers"], "unit": unit}
                for key in keys:
                    if rs[0][feed][str(n)][key + "_us"]:
                        row[key] = summary([r[feed][str(n)][key + "_us"] for r in rs])
                        p50[(label, feed, n, key)] = row[key]
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    first, last = variants[0][0], variants[-1][0]
    for feed, sizes, a_key, b_key in (("acks", ACK_SIZES, "two_call_native", "supervised"),
                                      ("pings", PING_SIZES, "health_events", "process_pings")):
        for n in sizes:
            if (last, feed, n, b_key) in p50:
                A, B = p50[(first, feed, n, a_key)], p50[(last, feed, n, b_key)]
                lines.append(json.dumps({"what": "supervision_feeds_ratio", "feed": feed, "n": n,
                                         "of": f"{last} {b_key} p50", "to": f"{first} {a_key} p50",
                                         "ratio": round(B["p50"] / A["p50"], 3),
                                         "b_p90_below_a_p10": bool(B["p90"] < A["p10"]),
                                         "b_p50_below_a_p50": bool(B["p50"] <= A["p50"])}))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
