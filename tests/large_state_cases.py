"""Workloads of the large-state engine's hot small-pool sweep (openwhisk_amd/csrc/owgs_seq.hip), shared by
test_large_state_inputs.py (CPU: each case's precondition, from the literal oracle) and test_gpu_large_state.py (GPU:
parity and the engine's path counters).

Every case is W.config("headline", **kw) plus one action that is never invoked, maxConcurrent 5000: beyond the on-chip
map's 12-bit field, so the context runs on the large-state engine however small its pool is.  On pools of 16 to 600
invokers the decisions of a 64-decision group meet on the same invokers all the time, which is where the engine's
group speculation can be wrong: its validation, its rejected speculations, its forced acquires and its map growth."""
import functools

import numpy as np

import oracle as O
from openwhisk_amd import workload as W
from openwhisk_amd.balancer import Action

WIDE = Action("zz", "zz/wide", "0.0.1", 128, 5000)
_SMALL = dict(n_activations=20_000, n_actions=200, n_namespaces=20)

CASES = {
    # two pools (36 managed, 4 blackbox), overloaded, shared fqn@version keys: forced plain and concurrent acquires,
    # rejected speculations
    "p40": dict(n_invokers=40, load=1.3, conc_frac=0.3, conc_range=(2, 6), shared_frac=0.4, **_SMALL),
    # a managed pool of SEQ_SPEC_C = 16 positions (concurrent speculation off: n > 16 fails) and a one-invoker blackbox pool
    "p17": dict(n_invokers=17, load=1.2, conc_frac=0.5, conc_range=(2, 4), user_memory_mb=2048, **_SMALL),
    # a managed pool of exactly SEQ_SPEC = 64 positions, plain actions only: the 64-step budget ends where the walk does
    "p64": dict(n_invokers=71, load=1.0, conc_frac=0.0, blackbox_frac=0.0, unhealthy_frac=0.0, **_SMALL),
    # ... and just past it, with unhealthy invokers and a blackbox pool that starts at id 66
    "p65": dict(n_invokers=73, load=1.1, conc_frac=0.2, unhealthy_frac=0.1, **_SMALL),
    # concurrent actions only, small slots: the walks' empty entries take the map past half of its first 65,536
    "p300": dict(n_invokers=300, load=1.3, conc_frac=1.0, conc_range=(2, 3), n_activations=60_000, n_actions=400,
                 n_namespaces=40, shared_frac=0.3, user_memory_mb=2048),
    # nearly full, mixed: fast runs of both kinds and concurrent decisions kept in order
    "p600": dict(n_invokers=600, load=0.95, conc_frac=0.3, conc_range=(2, 6), shared_frac=0.4, n_activations=40_000,
                 n_actions=500, n_namespaces=50, user_memory_mb=1024),
}


@functools.lru_cache(maxsize=None)
def workload(name):
    w = W.config("headline", **CASES[name])
    w.actions.append(WIDE)  # (no activation names it: the stream's handles end before it)
    assert int(w.stream.act.max()) < len(w.actions) - 1
    return w


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The literal oracle over the whole stream, once per case: (state, decisions, overload flags, release flags).
    The state is the stream's end state: read it, do not drive it further.  st.keys: fqn@version -> its map key."""
    w = workload(name)
    keys = {}
    st = O.state_for(w, zombies=True, slot_keys=keys)
    st.keys = keys
    inv, fl, rf = st.replay(w.stream)
    return st, inv, fl, rf


def facts(name):
    """What the oracle says about a case: pool sizes, batches, releases, forced acquires by kind, map entries."""
    w = workload(name)
    st, inv, fl, rf = oracle_run(name)
    s = w.stream
    maxc = np.array([a.max_concurrent for a in w.actions])[s.act]
    bb = np.array([a.blackbox for a in w.actions])[s.act]
    forced = (fl & 1) != 0
    slots = st.invoker_slots
    return dict(nm=st.managed_size, nb=st.blackbox_size, batches=s.n_batches, batch=int(w.info["batch"]),
                releases=len(s.rel_aid), forced=int(forced.sum()), forced_plain=int((forced & (maxc <= 1)).sum()),
                forced_conc=int((forced & (maxc > 1)).sum()), forced_blackbox=int((forced & bb).sum()),
                none=int((inv < 0).sum()), entries=sum(slots[i].concurrent_size() for i in range(len(slots))))
