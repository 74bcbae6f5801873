"""Workloads of the concurrency map's HBM overflow across calls (the unbounded map; ensure_ovf, restore_impl
and reset_ctab of openwhisk_amd/csrc/owgs_host.cpp), shared by test_ovf_growth_inputs.py (CPU: what each stream
reaches, from the oracle alone) and test_gpu_ovf_growth.py (GPU: parity call by call on one context).

Three streams over one cluster and one action list (the spill case of test_gpu_parity.py), told apart by length and
batching only:

  S1  60,000 activations: leaves more live (invoker, fqn@version) entries than the on-chip table has room for, so a
      context that replayed it keeps entries in the overflow for good (what S1 leaves unreleased is never released);
  S2  cap // 2 activations in one call, cap the overflow's capacity after S1: no capacity for `used` entries and n_new
      activations, ovf_need(used, n_new) = 2 * (used + n_new + OWGS_CTC) rounded up to a power of two, is within cap for
      that n_new, whatever `used` is -- the call has to move the live entries to a larger table;
  S3  300,000 activations in batches of 2,000, issued one batch per call: each call adds its activations to the
      host's upper bound of the entry count, which runs out long before the count itself needs a larger table.

An oracle run is a tuple of steps on one BalancerState: "S1", "S2:<cap>", "S3" (batch by batch) and "cluster2"
(updateCluster(2))."""
import functools

import numpy as np

import oracle as O
from openwhisk_amd import workload as W

OWGS_CTC = 4096  # entries of the on-chip primary table (include/owgs.h)
BASE = dict(n_invokers=3000, n_actions=6000, n_namespaces=600, conc_frac=1.0, conc_range=(2, 3), delay_mean=6.0,
            unhealthy_frac=0.0, blackbox_frac=0.0)
N1 = 60_000
N3, BATCH3 = 300_000, 2_000
SAMPLE = (200, 40)  # invokers x keys whose concurrentState is compared at the end of a case


def ovf_need(used, n_new):
    """The overflow capacity for `used` entries plus n_new activations (owgs_host.cpp): at least twice the entries it
    may have to hold (every one it has, one per activation of the call, a primary table's worth), a power of two from
    2^19 up to 2^30."""
    want, cap = 2 * (used + n_new + OWGS_CTC), 1 << 19
    while cap < want and cap < (1 << 30):
        cap <<= 1
    return cap


CAP0 = ovf_need(0, N1)  # what a fresh context allocates for S1


@functools.lru_cache(maxsize=None)
def s1():
    return W.config("headline", n_activations=N1, **BASE)


@functools.lru_cache(maxsize=None)
def s2(cap):
    return W.config("headline", n_activations=cap // 2, load=0.5, **BASE)


@functools.lru_cache(maxsize=None)
def s3():
    return W.config("headline", n_activations=N3, batch=BATCH3, **BASE)


def live_entries(st):
    """(invoker, fqn@version) entries of the oracle's NestedSemaphores (a zombies=False state keeps no empty ones)."""
    sl = st.invoker_slots
    return sum(sl[i].concurrent_size() for i in range(len(sl)))


def replay_by_batch(st, s):
    """The oracle over stream s one batch per call, as a caller that issues one batch at a time sees it."""
    n = len(s.act)
    out = np.full(max(n, 1), -9, dtype=np.int32)
    fl = np.zeros(max(n, 1), dtype=np.uint8)
    rf = np.zeros(max(len(s.rel_aid), 1), dtype=np.uint8)
    acq = np.ascontiguousarray(s.acq_off, dtype=np.int64)
    rel = np.ascontiguousarray(s.rel_off, dtype=np.int64)
    act = np.ascontiguousarray(s.act, dtype=np.int32)
    aid = np.ascontiguousarray(s.rel_aid if len(s.rel_aid) else np.zeros(1), dtype=np.int64)
    for b in range(len(acq) - 1):  # (offset views: absolute indices, earlier decisions in `out`)
        O.lib().owo_replay(st.h, 1, O._ptr(acq[b:]), O._ptr(act), O._ptr(rel[b:]), O._ptr(aid), int(s.seq_base),
                           O._ptr(out), O._ptr(fl), O._ptr(rf))
    return out[:n], fl[:n], rf[: len(s.rel_aid)]


def _step(st, step):
    name, _, arg = step.partition(":")
    if name == "cluster2":
        st.update_cluster(2)
        return None
    if name == "S1":
        return st.replay(s1().stream)
    if name == "S2":
        return st.replay(s2(int(arg)).stream)
    if name == "S3":
        return replay_by_batch(st, s3().stream)
    raise ValueError(step)


@functools.lru_cache(maxsize=None)
def oracle_run(steps):
    """The steps on one fresh oracle state: per step (decisions, flags, release flags, permits after it, live entries
    after it), and the state itself for concurrentState."""
    st = O.state_for(s1(), zombies=False)
    res = []
    for step in steps:
        r = _step(st, step)
        inv, fl, rf = r if r is not None else (None, None, None)
        res.append((inv, fl, rf, st.permits().copy(), live_entries(st)))
    return res, st


@functools.lru_cache(maxsize=None)
def s1_live_pairs():
    """The (invoker, key) entries S1 leaves for good: those of the activations it never releases (every action here
    is concurrent, and no other stream releases S1's activations).  They are the entries a later growth or restore has
    to carry over one by one; a call that never walks to one of them does not notice its loss."""
    w = s1()
    s = w.stream
    inv = oracle_run(("S1",))[0][0][0]
    keys = {}
    kid = np.array([keys.setdefault(a.key, len(keys)) for a in w.actions])
    left = np.setdiff1d(np.arange(len(s.act)), s.rel_aid)
    return sorted({(int(inv[i]), int(kid[s.act[i]])) for i in left if inv[i] >= 0})


def sample_pairs(n_slots, n_keys):
    """The seeded (invoker, key) sample of test_concurrency_map_beyond_the_primary_table."""
    rng = np.random.default_rng(0)
    return [(int(i), int(k)) for i in rng.choice(n_slots, size=SAMPLE[0], replace=False)
            for k in rng.choice(n_keys, size=SAMPLE[1], replace=False)]


def n_keys(w):
    return len({a.key for a in w.actions})
