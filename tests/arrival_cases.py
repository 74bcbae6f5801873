"""Drained batches in arrival order, shared by test_arrival_inputs.py (CPU: what the literal oracle says about each
case's calls) and test_gpu_arrival_order.py (GPU: parity of owgs_process_batch over its four routes).

The shim cuts a drained queue into runs, each a maximal block of completions followed by a block of publishes
(runBatch, integration/GpuShardingContainerPoolBalancer.scala).  The other tests queue every stream batch as all of its
completions, then all of its publishes, and their stream batches are thousands of jobs long: a call then holds one to
three runs.  A controller's queue holds completions and publishes as they arrive.  jobs() merges the two kinds of every
stream batch by a seeded random interleave that keeps the order inside each kind; a completion still names an
activation of an earlier stream batch, so the order stays causal.  The pools here are small, so the capacity-calibrated
stream batch is 60 to 150 jobs: a drain of a few hundred jobs spans several stream batches, holds dozens of runs, and
many of its completions name an activation published earlier in the same drain."""
import functools

import numpy as np

import oracle as O
from large_state_cases import WIDE
from openwhisk_amd import workload as W

_SMALL = dict(n_activations=20_000)
CASES = {
    # two pools (36 managed, 4 blackbox), overloaded, concurrent actions under shared fqn@version keys
    "a40": dict(n_invokers=40, user_memory_mb=4096, load=1.1, conc_frac=0.3, conc_range=(2, 6), shared_frac=0.4,
                n_actions=200, n_namespaces=20, **_SMALL),
    # half of the actions concurrent with small maxConcurrent, nearly full
    "b100": dict(n_invokers=100, user_memory_mb=2048, load=0.95, conc_frac=0.5, conc_range=(2, 4), n_actions=300,
                 n_namespaces=30, **_SMALL),
    # plain actions only, overloaded
    "c200": dict(n_invokers=200, user_memory_mb=2048, load=1.2, conc_frac=0.0, n_actions=300, n_namespaces=30,
                 **_SMALL),
}
INTERLEAVE_SEED = 7
SMALL_DRAINS = (1, 600, 1)      # (lo, hi, seed): calls the resident engine takes (at most OWGS_RES_MAX = 1,024 jobs)
LARGE_DRAINS = (1025, 4095, 2)  # calls beyond it, up to the shim's drainTo(jobs, 4095)


@functools.lru_cache(maxsize=None)
def workload(name, wide=False):
    """wide: the never-invoked maxConcurrent 5000 action of large_state_cases.py registered last, which moves the
    context to the large-state engine."""
    w = W.config("headline", **CASES[name])
    if wide:
        w.actions.append(WIDE)
        assert int(w.stream.act.max()) < len(w.actions) - 1
    return w


def jobs(w, seed=INTERLEAVE_SEED):
    """The queue in arrival order: (0, activation) = its completion, (1, activation) = its publish."""
    rng = np.random.default_rng(seed)
    s = w.stream
    out = []
    for b in range(s.n_batches):
        rel = s.rel_aid[s.rel_off[b]:s.rel_off[b + 1]]
        pub = np.arange(int(s.acq_off[b]), int(s.acq_off[b + 1]))
        assert len(rel) == 0 or int(rel.max()) < int(s.acq_off[b])  # causal: completions of earlier batches only
        kind = np.zeros(len(rel) + len(pub), np.int64)
        kind[len(rel):] = 1
        rng.shuffle(kind)
        idx = np.empty(len(kind), np.int64)
        idx[kind == 0] = rel
        idx[kind == 1] = pub
        out += list(zip(kind.tolist(), idx.tolist()))
    return out


def n_runs(batch):
    """Runs of one drained batch as runBatch cuts it: a run ends where a completion follows a publish."""
    return 1 + sum(1 for x, y in zip(batch, batch[1:]) if x[0] == 1 and y[0] == 0) if batch else 0


def drains(n_jobs, lo, hi, seed, limit=None):
    """[begin, end) of every drain of lo..hi jobs over the first `limit` jobs of the queue."""
    rng = np.random.default_rng(seed)
    end = n_jobs if limit is None else min(limit, n_jobs)
    cuts, pos = [], 0
    while pos < end:
        n = min(int(rng.integers(lo, hi + 1)), end - pos)
        cuts.append((pos, pos + n))
        pos += n
    return cuts


@functools.lru_cache(maxsize=None)
def facts(case, drain_lo, drain_hi, drain_seed):
    """The literal oracle alone through the drains: what the calls look like, and what they reach."""
    w = workload(case)
    st = O.state_for(w, zombies=True)
    act = w.stream.act
    maxc = np.array([a.max_concurrent for a in w.actions])
    q = jobs(w)
    dec = np.full(len(act), -9, np.int64)
    call_of = np.full(len(act), -1, np.int64)
    runs = []
    same = same_conc = forced = forced_conc = rejected = releases = 0
    for c, (b, e) in enumerate(drains(len(q), drain_lo, drain_hi, drain_seed)):
        runs.append(n_runs(q[b:e]))
        for kind, a in q[b:e]:
            if kind == 0:
                if dec[a] < 0:  # a failed publish holds no ActivationEntry (CLB:278-279)
                    continue
                releases += 1
                rejected += O._rel_bits(st.release(int(dec[a]), int(act[a]))) != 0
                if call_of[a] == c:
                    same += 1
                    same_conc += int(maxc[act[a]] > 1)
            else:
                x, f = st.publish(int(act[a]), int(a))
                dec[a], call_of[a] = x, c
                if f & 1:
                    forced += 1
                    forced_conc += int(maxc[act[a]] > 1)
    r = np.array(runs)
    return dict(batch=int(w.info["batch"]), jobs=len(q), calls=len(r), runs_median=int(np.median(r)),
                runs_max=int(r.max()), runs_min=int(r.min()), share_over_8=float((r > 8).mean()), releases=releases,
                same_call=same, same_call_conc=same_conc, forced=forced, forced_conc=forced_conc,
                rejected=int(rejected))
