"""The entitlement throttle gate (owgs_admit_batch): the per-minute rate throttle and, for actions that passed it, the
concurrent throttle, over a drained batch in array order.

`admit_model` is a literal per-item replay of the definition in include/owgs.h (RateThrottler.scala:47-86,
ActivationThrottler.scala:41-68, Entitlement.scala:97-133, 197-202, 354-381).  The CPU tests pin it to vectors written
by hand from the reference source (tests/golden/make_admit_golden.py) and its limit function to exact integer
arithmetic; the GPU tests compare the device with those vectors, with literal arrays and with the model -- never with
the device's own outputs.
"""
import itertools
import json
import math
import os

import numpy as np
import pytest

from openwhisk_amd import GpuShardingContainerPoolBalancer
from openwhisk_amd._lib import EINVAL, ENOENT, NONE, NS_INITIAL_CAP, OwgsError
from openwhisk_amd.balancer import Action

OK, RATE, CONC = 0, 1, 2       # OWGS_ADMIT_OK, OWGS_ADMIT_RATE, OWGS_ADMIT_CONCURRENT
ACT, TRIG, RO, CO = 0, 1, 2, 4
ABSENT = -2**63                # INT64_MIN: no record
MIN = 60_000
MB = 1 << 20
MANAGED = Action("ns", "ns/managed", "0.0.1", 256)
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "admit_vectors.json")) as _f:
    VECTORS = json.load(_f)


# ------------------------------------------------------------------------------------------------------- the model
def individual_limit(abs_limit, cs):
    """calculateIndividualLimit (Entitlement.scala:123-133) of dilateLimit (:99)."""
    d = math.ceil(float(abs_limit) * (1.2 if cs > 1 else 1.0))   # IEEE double product, Math.ceil
    dil = min(max(d, -2**31), 2**31 - 1)                         # Double.toInt saturates
    if dil == 0:
        return 0
    q = abs(dil) // cs * (1 if dil > 0 else -1)                  # JVM division truncates
    return max(q, 1)


def _wrap32(x):
    return (x + 2**31) % 2**32 - 2**31


def admit_model(state, limits, cs, active, ns, kind, t_ms, rate_override=None, conc_override=None):
    """One batch in array order.  state: {(handle, which): [lastMin, count]}, updated in place (which = 0 the invoke
    throttler, 1 the fire throttler); limits = the three system defaults; active: handle -> activations in flight.
    Returns (verdict, rate_count, rate_limit, conc_count, conc_limit)."""
    admitted = {}
    out = [[], [], [], [], []]
    for i in range(len(ns)):
        h, k, trig = int(ns[i]), int(kind[i]), int(kind[i]) & 1
        rl = individual_limit(int(rate_override[i]) if k & RO else limits[1 if trig else 0], cs)
        cl = 0 if trig else individual_limit(int(conc_override[i]) if k & CO else limits[2], cs)
        m = int(t_ms[i]) // MIN
        r = state.get((h, trig))
        if r is None or r[0] != m:               # new RateInfo / roll(): curMin != lastMin
            r = state[(h, trig)] = [m, 0]
        r[1] = _wrap32(r[1] + 1)                  # incrementAndGet, charged whatever the outcome
        cc = -1
        if not r[1] <= rl:                        # TimedRateLimit.ok
            v = RATE
        elif trig:
            v = OK
        else:
            cc = _wrap32(int(active.get(h, 0)) + admitted.get(h, 0))
            v = OK if cc < cl else CONC           # ConcurrentRateLimit.ok
            if v == OK:
                admitted[h] = admitted.get(h, 0) + 1
        for o, x in zip(out, (v, r[1], rl, cc, cl)):
            o.append(x)
    return (np.array(out[0], np.uint8),) + tuple(np.array(o, np.int32) for o in out[1:])


def _items(batch):
    it = np.array(batch["items"], dtype=np.int64).reshape(-1, 5)
    return it[:, 0], it[:, 1], it[:, 2], it[:, 3], it[:, 4]


def _want(batch):
    return tuple(batch[k] for k in ("verdict", "rate_count", "rate_limit", "conc_count", "conc_limit"))


def _final(case):
    """the case's final records as {(namespace index, which): [lastMin, count]}"""
    return {(h, w): list(r) for w, key in enumerate(("invoke", "fire")) for h, r in enumerate(case["final"][key])
            if r is not None}


# ------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("case", VECTORS, ids=[c["name"] for c in VECTORS])
def test_model_reproduces_the_golden_vectors(case):
    state = {}
    active = dict(enumerate(case["active"]))
    for batch in case["batches"]:
        ns, kind, t, ro, co = _items(batch)
        got = admit_model(state, case["limits"], case["cluster"], active, ns, kind, t, ro, co)
        for g, w in zip(got, _want(batch)):
            assert g.tolist() == w
    assert state == _final(case)


def test_golden_vectors_cover_the_issue_cases():
    names = " | ".join(c["name"] for c in VECTORS)
    for part in ("limit 0", "limit 1:", "override 5", "cluster size 1", "cluster size 2", "cluster size 3",
                 "cluster size 8", "stepping back", "interleaved", "no concurrent room"):
        assert part in names, part


def test_constants_match_the_header():
    from openwhisk_amd import _lib
    src = open(_lib.HEADER).read()
    for name, val in (("OK", OK), ("RATE", RATE), ("CONCURRENT", CONC), ("TRIGGER", TRIG), ("RATE_OVERRIDE", RO),
                      ("CONC_OVERRIDE", CO)):
        assert getattr(_lib, "ADMIT_" + name) == val
        assert f"#define OWGS_ADMIT_{name} {val}" in src
    assert _lib.RATE_ABSENT == ABSENT


@pytest.mark.parametrize("cs", [2, 8])
def test_limit_function_equals_exact_integer_arithmetic(cs):
    # ceil(1.2 l) = ceil(6 l / 5) in integers: the double product never lands on the wrong side of an integer here
    for l in range(1, 100_001):
        assert individual_limit(l, cs) == max(-(-6 * l // 5) // cs, 1), l
    assert individual_limit(0, cs) == 0 and individual_limit(-5, cs) == 1
    assert individual_limit(2**31 - 1, cs) == (2**31 - 1) // cs


# ------------------------------------------------------------------------------------------------------ GPU tests
gpu = pytest.mark.gpu
_next_id = itertools.count(1)
_next_minute = itertools.count(28_400_000, 10)


def fresh_ids(n):
    return ["%032x" % (0xA6 << 100 | next(_next_id)) for _ in range(n)]


def fresh_t0():
    """The start of a minute no test has used: every rate record resets at its first check in it, so a test on a
    shared balancer needs no knowledge of what ran before."""
    return next(_next_minute) * MIN


def new_balancer(n_ns, active=(), cluster=1):
    """A balancer with n_ns namespaces (handles 0..n_ns-1) and active[h] tracked activations of namespace h."""
    b = GpuShardingContainerPoolBalancer()
    b.update_invokers_arrays(np.arange(4), np.full(4, 4096 * MB), np.zeros(4, np.uint8))
    if cluster != 1:
        b.update_cluster(cluster)
    (m,), _ = b.register_actions([MANAGED])
    ns = b.register_namespaces([0xAD317 << 64 | k for k in range(n_ns)])
    assert ns.tolist() == list(range(n_ns))
    h = np.repeat(np.arange(len(active)), active)
    if len(h):
        t, e = b.track_activations(fresh_ids(len(h)), np.full(len(h), m), np.arange(len(h)), ns=h)
        assert not e.any()
    return b


def check_state(b, state, handles):
    """rate_state of the touched records against the model's"""
    for which in (0, 1):
        last, cnt = b.rate_state(handles, which)
        for h, lm, c in zip(handles, last.tolist(), cnt.tolist()):
            if (int(h), which) in state:
                assert [lm, c] == state[(int(h), which)], (h, which)


def same(got, want, tag=None):
    for name, g, w in zip(("verdict", "rate_count", "rate_limit", "conc_count", "conc_limit"), got, want):
        assert np.array_equal(g, np.asarray(w)), (name, tag, np.nonzero(np.asarray(g) != np.asarray(w))[0][:8])


@pytest.fixture(scope="module")
def gate():
    """300 namespaces; five of them with 3, 10, 45, 64 and 130 activations in flight (tests/test_gpu_inflight.py's
    pattern).  admit_batch only reads the books, so they stay; tests take fresh minutes and set the limits they need."""
    b = GpuShardingContainerPoolBalancer()
    (m,), _ = b.register_actions([MANAGED])
    ns = b.register_namespaces([0xC0DE << 64 | k for k in range(300)])
    five = ns[[0, 17, 63, 64, 299]]
    base = [3, 10, 45, 64, 130]
    h = np.repeat(five, base)
    b.track_activations(fresh_ids(len(h)), np.full(len(h), m), np.arange(len(h)), ns=h)
    return b, five, dict(zip(five.tolist(), base))


# 1 ---------------------------------------------------------------------------------------------- golden vectors
@gpu
@pytest.mark.parametrize("case", VECTORS, ids=[c["name"] for c in VECTORS])
def test_gpu_golden_vectors(case):
    b = new_balancer(len(case["active"]), case["active"], case["cluster"])
    b.set_throttle_limits(*case["limits"])
    handles = np.arange(len(case["active"]))
    for which in (0, 1):
        last, cnt = b.rate_state(handles, which)
        assert np.all(last == ABSENT) and not cnt.any()
    for batch in case["batches"]:
        ns, kind, t, ro, co = _items(batch)
        same(b.admit_batch(ns, kind, t, ro, co), _want(batch), case["name"])
    final = _final(case)
    for which in (0, 1):
        last, cnt = b.rate_state(handles, which)
        want = [final.get((int(h), which), [ABSENT, 0]) for h in handles]
        assert [list(x) for x in zip(last.tolist(), cnt.tolist())] == want
    assert b.active_activations_for(handles).tolist() == case["active"]  # read-only for the books


# 2 ------------------------------------------------------------------------------------------ hand case with books
@gpu
def test_gpu_hand_case_leaves_the_books_alone():
    b = new_balancer(1, [2])
    t0 = fresh_t0()
    got = b.admit_batch([0] * 6, [CO, CO | RO, CO, CO, CO, TRIG], [t0 + k for k in range(6)],
                        rate_override=[0, 1, 0, 0, 0, 0], conc_override=[3, 9, 3, 1, 4, 0])
    # 2 in flight.  #0 admitted (2 < 3); #1 is the 2nd invoke against its own limit 1: rejected, no concurrent check;
    # #2 and #3 see 3 (only #0 was admitted); #4 is admitted (3 < 4); the trigger has its own count and no concurrent
    # throttle
    same(got, ([OK, RATE, CONC, CONC, OK, OK], [1, 2, 3, 4, 5, 1], [60, 1, 60, 60, 60, 60], [2, -1, 3, 3, 3, -1],
               [3, 9, 3, 1, 4, 0]))
    assert b.active_activations_for([0]).tolist() == [2] and b.activation_totals() == (2, 512, 0)
    assert [x.tolist() for x in b.rate_state([0], 0)] == [[t0 // MIN], [5]]
    assert [x.tolist() for x in b.rate_state([0], 1)] == [[t0 // MIN], [1]]


# 3 --------------------------------------------------------------------------------- against the model at the edges
def _random_batch(rng, n, five, base, t0, blocky):
    which = rng.integers(0, 5, n)
    ns = five[which]
    bs = np.array(base)[which]
    kind = (rng.random(n) < .3).astype(np.int64)                                        # 30 % triggers
    co = np.stack([np.zeros(n, np.int64), bs - 1, bs, bs + 1, bs + 40])[rng.integers(0, 5, n), np.arange(n)]
    kind |= np.where(rng.random(n) < .8, CO, 0)
    t = t0 + rng.integers(0, 3 * MIN, n)                                                # three minutes, unsorted
    if blocky:  # long runs of one minute with a few items out of place
        t = np.sort(t)
        sw = rng.integers(0, n, (max(n // 20, 1), 2))
        for x, y in sw:
            t[[x, y]] = t[[y, x]]
        ro = rng.choice([1, 2, 4, 12], n)
    else:
        ro = rng.choice([0, 1, 1, 3], n)
    kind |= np.where(rng.random(n) < .8, RO, 0)
    return ns, kind, t, ro, co


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_gpu_matches_the_model_at_the_edges(gate, n):
    b, five, active = gate
    limits = (20, 15, 30)
    b.set_throttle_limits(*limits)
    base = [active[int(h)] for h in five]
    t0 = fresh_t0()
    state, rejected = {}, 0
    for seed in range(3):  # the same three minutes each time: the records carry from batch to batch
        rng = np.random.default_rng(1000 * n + seed)
        ns, kind, t, ro, co = _random_batch(rng, n, five, base, t0, blocky=seed == 1)
        want = admit_model(state, limits, 1, active, ns, kind, t, ro, co)
        same(b.admit_batch(ns, kind, t, ro, co), want, (n, seed))
        check_state(b, state, five)
        rejected += int((want[0] == RATE).sum())
    if n == 1000:  # (a property of the inputs: about a third is rate-rejected)
        assert 0.2 < rejected / 3000 < 0.5, rejected
    assert b.active_activations_for(five).tolist() == base


# 4 ------------------------------------------------------------------------------------ one namespace, 257 actions
@gpu
def test_gpu_257_actions_one_limit_pair(gate):
    b, five, active = gate
    h, n, i = five[2], 257, np.arange(257)
    got = b.admit_batch(np.full(n, h), np.full(n, RO | CO), fresh_t0() + i, np.full(n, 100), np.full(n, 45 + 300))
    same(got, (np.where(i < 100, OK, RATE), i + 1, np.full(n, 100), np.where(i < 100, 45 + i, -1), np.full(n, 345)))


@gpu
def test_gpu_257_actions_rank_among_the_eligible(gate):
    b, five, active = gate
    h, n, i = five[2], 257, np.arange(257)
    ro = np.where(i % 3 == 0, 0, 1000)        # every third action is rate-rejected
    t = fresh_t0() + i
    got = b.admit_batch(np.full(n, h), np.full(n, RO | CO), t, ro, np.full(n, 45 + 100))
    elig = i % 3 != 0
    rank = np.cumsum(elig) - elig              # eligible actions before i: the 100th one is item 150
    verdict = np.where(~elig, RATE, np.where(rank < 100, OK, CONC))
    same(got, (verdict, i + 1, ro, np.where(elig, 45 + np.minimum(rank, 100), -1), np.full(n, 145)))
    same(got, admit_model({}, (60, 60, 30), 1, active, np.full(n, h), np.full(n, RO | CO), t, ro, np.full(n, 145)))


@gpu
def test_gpu_257_actions_mixed_concurrent_limits(gate):
    b, five, active = gate
    h, n, i = five[2], 257, np.arange(257)
    limits = (1000, 1000, 30)
    b.set_throttle_limits(*limits)
    co = np.where(i % 3 == 0, 45 + 20, 45 + 100)  # a stricter limit on every third: a true in-order dependency
    t = fresh_t0() + i
    for kind, ro in ((CO, None), (CO | RO, np.where(i % 5 == 1, 0, 1000))):  # ... and with rate-rejected ones between
        state = {}
        want = admit_model(state, limits, 1, active, np.full(n, h), np.full(n, kind), t, ro, co)
        same(b.admit_batch(np.full(n, h), np.full(n, kind), t, ro, co), want)
        check_state(b, state, [h])
        t = fresh_t0() + i


@gpu
@pytest.mark.parametrize("pos", [0, 63, 64, 128])
def test_gpu_257_actions_minute_change(gate, pos):
    b, five, active = gate
    h, n, i = five[2], 257, np.arange(257)
    b.set_throttle_limits(1000, 1000, 1000)
    t0 = fresh_t0()
    got = b.admit_batch(np.full(5, h), np.zeros(5), np.full(5, t0))
    assert got[1].tolist() == [1, 2, 3, 4, 5]
    t = np.where(i < pos, t0 + 59_999, t0 + MIN)  # the minute changes at sorted position pos
    got = b.admit_batch(np.full(n, h), np.zeros(n), t)
    same(got, (np.zeros(n), np.where(i < pos, 5 + i + 1, i - pos + 1), np.full(n, 1000), 45 + i, np.full(n, 1000)))
    assert [x.tolist() for x in b.rate_state([h], 0)] == [[t0 // MIN + 1], [n - pos]]


@gpu
def test_gpu_257_actions_and_triggers_alternating(gate):
    b, five, active = gate
    h, n, i = five[2], 257, np.arange(257)
    limits = (100, 40, 45 + 60)
    b.set_throttle_limits(*limits)
    t = fresh_t0() + i
    kind = i & 1
    got = b.admit_batch(np.full(n, h), kind, t)
    state = {}
    same(got, admit_model(state, limits, 1, active, np.full(n, h), kind, t))
    assert got[1].tolist() == (i // 2 + 1).tolist()  # two independent counts
    # actions: 100 pass the rate check, the first 60 of them find room; triggers: 40 pass, no concurrent check
    a = i // 2
    verdict = np.where(kind == 1, np.where(a < 40, OK, RATE), np.where(a < 60, OK, np.where(a < 100, CONC, RATE)))
    assert got[0].tolist() == verdict.tolist()
    check_state(b, state, [h])


# 5 ------------------------------------------------------------------------- split invariance of the rate part
@gpu
def test_gpu_rate_part_is_split_invariant(gate):
    b, five, active = gate
    b.set_throttle_limits(20, 15, 30)
    base = [active[int(h)] for h in five]
    rng = np.random.default_rng(55)
    ns, kind, dt, ro, co = _random_batch(rng, 1000, five, base, 0, blocky=True)

    def run(cuts):
        t0 = fresh_t0()
        edges = [0] + cuts + [1000]
        parts = [b.admit_batch(ns[x:y], kind[x:y], t0 + dt[x:y], ro[x:y], co[x:y]) for x, y in zip(edges, edges[1:])]
        st = [b.rate_state(five, w) for w in (0, 1)]
        return (np.concatenate([p[1] for p in parts]).tolist(), np.concatenate([p[2] for p in parts]).tolist(),
                [((lm - t0 // MIN).tolist(), c.tolist()) for lm, c in st])

    whole = run([])
    for cut in (1, 64, 500):
        assert run([cut]) == whole, cut


# 6 ------------------------------------------------------------------------------------------------- cluster size
@gpu
def test_gpu_limits_follow_cluster_size_and_defaults():
    b = new_balancer(9)
    lims = [0, 1, 2, 3, 5, 30, 60, 2**31 - 1, -5]
    ns = np.concatenate([np.arange(9), np.arange(9), [0, 0]])
    kind = np.concatenate([np.full(9, RO | CO), np.full(9, TRIG | RO), [ACT, TRIG]])
    ov = np.concatenate([lims, lims, [0, 0]])
    state = {}
    for cs, limits in ((1, (60, 60, 30)), (2, (60, 60, 30)), (8, (60, 60, 30)), (8, (7, 100, 1000)), (2, (7, 100, 1000))):
        b.update_cluster(cs)
        b.set_throttle_limits(*limits)  # takes effect on the next call
        t = np.full(len(ns), fresh_t0())
        want = admit_model(state, limits, cs, {}, ns, kind, t, ov, ov)
        got = b.admit_batch(ns, kind, t, ov, ov)
        same(got, want, (cs, limits))
        # the two items without overrides carry the dilated defaults
        assert got[2][-2:].tolist() == [individual_limit(limits[0], cs), individual_limit(limits[1], cs)]
        assert got[4][-2:].tolist() == [individual_limit(limits[2], cs), 0]
    assert got[2][:9].tolist() == [0, 1, 1, 2, 3, 18, 36, 1073741823, 1]  # cs = 2, by hand (the golden table)


# 7 ------------------------------------------------------------------------------------------ errors change nothing
@gpu
def test_gpu_errors_change_nothing():
    b = new_balancer(2, [1])
    t0 = fresh_t0()
    b.admit_batch([0, 0, 1], [ACT, TRIG, ACT], [t0] * 3)
    before = [[x.tolist() for x in b.rate_state([0, 1], w)] for w in (0, 1)]
    assert before == [[[t0 // MIN] * 2, [1, 1]], [[t0 // MIN, ABSENT], [1, 0]]]
    t1 = t0 + MIN
    for code, ns, kind, t, ro in ((EINVAL, [0, 1, NONE], [0, 0, 0], [t1] * 3, None),
                                  (ENOENT, [0, 1, 2], [0, 0, 0], [t1] * 3, None),
                                  (ENOENT, [0, 1, -7], [0, 0, 0], [t1] * 3, None),
                                  (EINVAL, [0, 1, 1], [0, 0, 8], [t1] * 3, None),
                                  (EINVAL, [0, 1, 1], [0, 0, 128 | TRIG], [t1] * 3, None),
                                  (EINVAL, [0, 1, 1], [0, 0, 0], [t1, t1, -1], None),
                                  (EINVAL, [0, 1, 1], [0, 0, 0], [t1, t1, 2**60], None),
                                  (EINVAL, [0, 1, 1], [0, 0, CO], [t1] * 3, [5, 5, 5])):  # bit 2 without its array
        with pytest.raises(OwgsError) as err:
            b.admit_batch(ns, kind, t, rate_override=ro)
        assert err.value.code == code, (ns, kind, t)
        assert [[x.tolist() for x in b.rate_state([0, 1], w)] for w in (0, 1)] == before
    with pytest.raises(OwgsError) as err:
        b.rate_state([2], 0)
    assert err.value.code == ENOENT
    assert all(len(x) == 0 for x in b.admit_batch([], [], []))  # n = 0 is fine
    assert len(b.rate_state([], 1)[0]) == 0
    assert b.admit_batch([0], [ACT], [2**60 - 1])[1].tolist() == [1]  # the largest valid time
    assert b.active_activations_for([0, 1]).tolist() == [1, 0]


# 8 ------------------------------------------------------------------------------------------------------- growth
@gpu
def test_gpu_rate_records_survive_growth():
    b = GpuShardingContainerPoolBalancer()
    uu = [0xBEEF << 64 | (k * 2654435761) for k in range(2400)]
    assert b.register_namespaces(uu[:1000]).tolist() == list(range(1000)) and 1000 < NS_INITIAL_CAP
    t0 = fresh_t0()
    h = np.arange(1000)
    ns = np.concatenate([np.repeat(h, h % 3 + 1), h[::2]])           # 1..3 invokes each, a fire on the even ones
    kind = np.concatenate([np.zeros(len(ns) - 500, np.int64), np.ones(500, np.int64)])
    t = t0 + (ns % 2) * MIN                                           # odd handles one minute later
    b.admit_batch(ns, kind, t)
    want = [(t0 // MIN + h % 2, h % 3 + 1), (np.where(h % 2 == 0, t0 // MIN, ABSENT), (h % 2 == 0).astype(int))]

    def check(upto):
        for w in (0, 1):
            last, cnt = b.rate_state(np.arange(upto), w)
            assert np.array_equal(last[:1000], want[w][0]) and np.array_equal(cnt[:1000], want[w][1])
            assert np.all(last[1000:] == ABSENT) and not cnt[1000:].any()

    check(1000)
    assert b.register_namespaces(uu[1000:1200]).tolist() == list(range(1000, 1200)) and 1200 > NS_INITIAL_CAP
    check(1200)
    assert b.register_namespaces(uu[1100:2400]).tolist() == list(range(1100, 2400)) and 2400 > 2 * NS_INITIAL_CAP
    check(2400)
    # old records go on counting in their minute; a new handle starts at 1
    got = b.admit_batch([6, 2399, 6, 7], [ACT, ACT, TRIG, ACT], [t0, t0, t0, t0 + MIN])
    assert got[1].tolist() == [2, 1, 2, 3] and got[0].tolist() == [OK] * 4
