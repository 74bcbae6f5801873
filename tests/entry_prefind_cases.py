"""Workloads of the engine's entry pre-find (the I/O wave finds or inserts the concurrency-map entries
that were absent when a chunk's lanes speculated), shared by test_entry_prefind_inputs.py (CPU: each case's
precondition, from the oracle's decisions alone) and test_gpu_entry_prefind.py (GPU: parity and the two counters).

An "absent-entry lane" is a concurrent decision whose (invoker, fqn@version) entry did not exist when its chunk
started.  The engine's map holds an entry exactly while its operationCount is positive, so the count follows from the
oracle's assignment vector and the stream: acquisitions minus releases per pair, looked at every CHUNK decisions of a
batch (192 lanes, the narrowest chunk the engine picks for these pools)."""
import functools

import numpy as np

import oracle as O
from openwhisk_amd import workload as W

CHUNK = 192
ODD_MEM = (129, 255, 257, 1000, 1023)  # (the ODD set of test_gpu_engine_division.py)
ODD = dict(n_invokers=120, user_memory_mb=4099, mem_choices=ODD_MEM, delay_mean=1.5, n_actions=300, n_namespaces=30,
           unhealthy_frac=0.0)
_A = dict(n_invokers=200, n_activations=6000, batch=1500, user_memory_mb=4096, mem_choices=(128, 256), conc_frac=1.0,
          conc_range=(2, 4), n_actions=4000, n_namespaces=50, zipf_s=0.0, unhealthy_frac=0.0, delay_mean=1.5)

CASES = {
    # many keys: far more absent-entry lanes per chunk than one round of the I/O wave takes
    "A": ("headline", _A),
    # one key, many lanes: six actions with hundreds of container slots, so the lanes of a chunk meet on one entry.
    # Popularity is the generator's Zipf (s = 1): the most popular action then holds up to 72 lanes of a 192-lane
    # chunk, more than one round of the I/O wave; spread evenly (A's s = 0) no action gets past 37
    "B": ("headline", dict(_A, conc_range=(100, 500), n_actions=6, n_namespaces=2, shared_frac=0.0, zipf_s=1.0)),
    # a map beyond the on-chip table's fill: the fill gate, the overflow table and a rebuild
    "C": ("headline", dict(n_invokers=400, n_activations=20000, user_memory_mb=8192, mem_choices=(128,), conc_frac=1.0,
                           conc_range=(2, 3), n_actions=8000, n_namespaces=50, zipf_s=0.0, unhealthy_frac=0.0,
                           delay_mean=6.0, load=0.9)),
    # stops and forced acquires: lanes behind a stop speculate again elsewhere
    "D": ("headline", dict(ODD, conc_frac=0.5, load=1.2, blackbox_frac=0.1, n_activations=6000)),
}


@functools.lru_cache(maxsize=None)
def workload(name):
    base, kw = CASES[name]
    return W.config(base, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle over the whole stream, once per case: (final permits, decisions, overload flags, release flags)."""
    w = workload(name)
    st = O.state_for(w)
    inv, fl, rf = st.replay(w.stream)
    return st.permits().copy(), inv, fl, rf


@functools.lru_cache(maxsize=None)
def facts(name):
    """Per chunk: the absent-entry lanes and the most lanes on one absent pair; the most live entries at a batch end;
    forced acquires.  From the oracle's decisions and the stream alone."""
    w = workload(name)
    _, inv, fl, _ = oracle_run(name)
    s = w.stream
    keys = {}
    slot = np.array([keys.setdefault(a.key, len(keys)) for a in w.actions])
    maxc = np.array([a.max_concurrent for a in w.actions])
    ops = {}  # (invoker, fqn@version key) -> operationCount
    absent, same, live_max = [], [], 0
    for b in range(s.n_batches):
        for aid in s.rel_aid[s.rel_off[b]:s.rel_off[b + 1]]:
            a = s.act[aid]
            if maxc[a] > 1 and inv[aid] >= 0:
                p = (int(inv[aid]), int(slot[a]))
                ops[p] -= 1
                if ops[p] == 0:
                    del ops[p]
        for c0 in range(int(s.acq_off[b]), int(s.acq_off[b + 1]), CHUNK):
            c1 = min(c0 + CHUNK, int(s.acq_off[b + 1]))
            pairs = [(int(inv[i]), int(slot[s.act[i]])) for i in range(c0, c1) if maxc[s.act[i]] > 1 and inv[i] >= 0]
            miss = {}
            for p in pairs:
                if p not in ops:
                    miss[p] = miss.get(p, 0) + 1
            absent.append(sum(miss.values()))
            same.append(max(miss.values(), default=0))
            for p in pairs:
                ops[p] = ops.get(p, 0) + 1
        live_max = max(live_max, len(ops))
    forced = (fl & 1) != 0
    return dict(batches=s.n_batches, chunks=len(absent), absent_mean=float(np.mean(absent)),
                chunks_over_64=int((np.array(absent) > 64).sum()), same_key_max=int(max(same)), live_max=live_max,
                forced=int(forced.sum()), forced_conc=int((forced & (maxc[s.act] > 1)).sum()))
