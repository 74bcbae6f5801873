"""Time the result-carrying acks on the GPU: what one ack batch costs from entry to return when part of
it are CombinedCompletionAndResultMessages, through the new call against the two calls a library without it needs.

  A  owgs_process_acks_supervised, then the Python stand-in for the JVM's parse of the messages it left (kind 1: the
     id, the invoker and isSystemError out of json.loads), then owgs_complete_activations_supervised for them
  B  owgs_process_result_acks (with a summary, apply = 2)
  at n = 128 (the feed's batch, LB:94-108) and n = 4,095 acks of the headline draw with a Healthy pool, the Combined
  share 0 %, 50 % and 100 %, canonical messages (tests/result_ack_cases.py) with results of ~300 bytes.  Every call
  completes n freshly published and tracked activations, all Success.

Each variant is a libowgs.so (optionally with the checkout its Python package is imported from, for a library of
another commit that lacks the new symbol):

    python tools/time_result_acks.py --out profiles/result_acks.jsonl \
        parent=/path/to/parent/openwhisk_amd/libowgs.so,/path/to/parent  kept=openwhisk_amd/libowgs.so

A library without the call is timed on leg A only.  Every variant runs in a fresh child process, the variants
alternating over `--rounds` rounds; a call is timed on the host clock from entry to return (every call ends in a stream
synchronisation).  For leg A `two_call` includes the stand-in parse, `two_call_native` is the two native calls alone
and `supervised` the first of them; what the JVM itself saves (its own parse, the promise map) is not measured.  One
JSON line per variant, size and share: p50, p10, p90 over all rounds' samples and each round's p50 (microseconds).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (128, 4_095)
SHARES = (0, 50, 100)
H = 1700000000123
PLACEHOLDER = "f" * 32


def child(reps, warm):
    sys.path.insert(0, os.environ.get("OWGS_TREE") or ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    from openwhisk_amd import GpuShardingContainerPoolBalancer
    from openwhisk_amd import workload as W
    from result_ack_cases import activation_members, combined_message, print_object

    w = W.config("headline", n_activations=60_000)
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    b.set_health_tid(H)
    L, h = b._L, b._h
    new = hasattr(L, "owgs_process_result_acks") and hasattr(b, "process_result_acks")
    n_inv = len(w.inv_ids)
    ids = np.arange(n_inv, dtype=np.int32)
    b.health_events(ids, np.zeros(n_inv, np.uint8), np.zeros(n_inv, np.int64), w.inv_mem, 0)
    b.health_events(ids, np.ones(n_inv, np.uint8), np.ones(n_inv, np.int64), w.inv_mem, 1, apply=True)
    assert (b.health_read()[0] == 0).all()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rng = np.random.default_rng(9)
    # canonical bodies printed once; a batch only puts its ids in
    bodies = [print_object(activation_members(rng, PLACEHOLDER, 300)) for _ in range(64)]
    out = {"new": bool(new), "invokers": n_inv, "res": {}}
    now, seq, cur = 10, 0, 0

    def batch(n, share):
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
        msgs = []
        for q, (a, i) in enumerate(zip(aids, inv[ok])):
            if (q * share) // 100 != ((q + 1) * share) // 100:
                msgs.append(combined_message(bodies[q % 64].replace(PLACEHOLDER, a), int(i)))
            else:
                msgs.append(W.completion_message(a, int(i)))
        off = np.zeros(len(msgs) + 1, np.int64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return len(msgs), np.frombuffer(b"".join(msgs) + b"\0", np.uint8), off, msgs

    for n in SIZES:
        kind, fl = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        inv, tk, rlen = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        aid, roff, summ = np.zeros(2 * n, np.uint64), np.zeros(n, np.int64), np.zeros(3, np.int32)
        k2, t2, f2 = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        for share in SHARES:
            res = {"two_call_us": [], "two_call_native_us": [], "supervised_us": [], "result_acks_us": [],
                   "bytes_per_batch": 0}
            for leg in ("A", "B"):
                if leg == "B" and not new:
                    break
                for r in range(warm + reps):
                    m, buf, off, msgs = batch(n, share)
                    now += 1
                    if leg == "A":
                        t0 = time.perf_counter_ns()
                        rc = L.owgs_process_acks_supervised(h, m, P(buf), P(off), P(kind), P(inv), P(tk), P(fl), now, 2,
                                                            P(summ))
                        t1 = time.perf_counter_ns()
                        jvm = np.flatnonzero(kind[:m] == 1)
                        a32, ci, cf = [], np.zeros(max(len(jvm), 1), np.int32), np.zeros(max(len(jvm), 1), np.uint8)
                        for z, q in enumerate(jvm):
                            d = json.loads(msgs[q])
                            a32.append(d["response"]["activationId"])
                            ci[z] = d["invoker"]["instance"]
                            cf[z] = 2 if d.get("isSystemError") else 0
                        ab = np.frombuffer("".join(a32).encode("ascii") or b"\0", np.uint8)
                        t2_ = time.perf_counter_ns()
                        rc2 = 0
                        if len(jvm):
                            rc2 = L.owgs_complete_activations_supervised(h, len(jvm), P(ab), P(ci), P(cf), P(k2), P(t2),
                                                                         P(f2), now, 2, P(summ))
                        t3 = time.perf_counter_ns()
                        assert rc == 0 and rc2 == 0 and (kind[:m][kind[:m] != 1] == 3).all(), (rc, rc2)
                        assert len(jvm) == 0 or (k2[:len(jvm)] == 3).all()
                        if r >= warm:
                            res["two_call_us"].append((t3 - t0) / 1e3)
                            res["two_call_native_us"].append((t1 - t0 + t3 - t2_) / 1e3)
                            res["supervised_us"].append((t1 - t0) / 1e3)
                    else:
                        from openwhisk_amd._lib import owgs_ack_out
                        o = owgs_ack_out(P(kind), P(inv), P(tk), P(fl), P(aid), P(roff), P(rlen))
                        t0 = time.perf_counter_ns()
                        rc = L.owgs_process_result_acks(h, m, P(buf), P(off), C.byref(o), now, 2, P(summ))
                        t1 = time.perf_counter_ns()
                        assert rc == 0 and (kind[:m] == 3).all() and summ[0] == m, (rc, summ)
                        if r >= warm:
                            res["result_acks_us"].append((t1 - t0) / 1e3)
                    res["bytes_per_batch"] = int(off[m])
            out["res"]["%d/%d" % (n, share)] = res
    assert (b.health_read()[0] == 0).all() and b.activations_live() == 0
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
    lines = []
    for n in SIZES:
        for share in SHARES:
            for label, _, _ in variants:
                rs = got[label]
                key = "%d/%d" % (n, share)
                row = {"what": "result_acks", "variant": label, "n": n, "combined_percent": share,
                       "bytes_per_batch": rs[0]["res"][key]["bytes_per_batch"], "invokers": rs[0]["invokers"],
                       "unit": unit}
                for k in ("two_call", "two_call_native", "supervised", "result_acks"):
                    if rs[0]["res"][key][k + "_us"]:
                        row[k] = summary([r["res"][key][k + "_us"] for r in rs])
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
