"""GPU tests of the in-flight books (totalActivations, the two memory totals, activationsPerNamespace) and of the
batched throttle check.

The model (`Books`) restates CommonLoadBalancer.scala:121-127 (setupActivation counts every message before
activationSlots.getOrElseUpdate) and :280-284 (processCompletion subtracts the removed entry's values).  Which
completions remove an entry, and which entry, is taken from the oracle (oracle.AckFlow: outcome RELEASED, the removed
ticket naming the first tracker) or from numbers written out by hand -- never from the GPU's own outputs.
"""
import itertools
import types
from collections import defaultdict

import numpy as np
import pytest

import oracle as O
from openwhisk_amd import GpuShardingContainerPoolBalancer
from openwhisk_amd import workload as W
from openwhisk_amd._lib import (ACK_FORCED_NOENTRY, ACK_NOENTRY, ACK_RELEASED, EINVAL, ENOENT, NONE, NS_INITIAL_CAP,
                                OwgsError)
from openwhisk_amd.balancer import Action

pytestmark = pytest.mark.gpu
H = 1700000000123
MANAGED = Action("ns", "ns/managed", "0.0.1", 256)
BLACKBOX = Action("ns", "ns/blackbox", "0.0.1", 512, 1, True)
_next_id = itertools.count(1)


def fresh_ids(n):
    """n activation ids no other test of this module has used."""
    return ["%032x" % (0xA5 << 100 | next(_next_id)) for _ in range(n)]


class Books:
    """CLB:62-65 with the updates of CLB:121-127 and CLB:280-284."""

    def __init__(self, actions):
        self.actions = actions
        self.active = defaultdict(int)   # activationsPerNamespace
        self.total = 0                   # totalActivations
        self.mem = [0, 0]                # totalManagedActivationMemory, totalBlackBoxActivationMemory
        self.first = {}                  # ticket of an entry -> (namespace, action) of its first tracker

    def track(self, ns, action, ticket, existed):
        a = self.actions[action]
        self.total += 1                                  # CLB:121
        self.mem[1 if a.blackbox else 0] += a.mem_mb     # CLB:122-125
        if ns != NONE:
            self.active[ns] += 1                         # CLB:127
        if not existed:                                  # getOrElseUpdate created the entry (CLB:148-166)
            self.first[ticket] = (ns, action)

    def release(self, ticket):
        ns, action = self.first.pop(ticket)              # Some(entry), CLB:279
        a = self.actions[action]
        self.total -= 1                                  # CLB:280
        self.mem[1 if a.blackbox else 0] -= a.mem_mb     # CLB:281-283
        if ns != NONE:
            self.active[ns] -= 1                         # CLB:284

    def check(self, b, handles):
        want = np.array([self.active[int(h)] for h in handles], dtype=np.int32)
        assert np.array_equal(b.active_activations_for(handles), want)
        assert b.activation_totals() == (self.total, self.mem[0], self.mem[1])


def books(b, handles):
    return b.active_activations_for(handles).tolist(), b.activation_totals()


@pytest.fixture(scope="module")
def bal():
    """A balancer with one managed 256 MB and one blackbox 512 MB action and 300 namespaces; every test that uses it
    leaves all counters at zero."""
    b = GpuShardingContainerPoolBalancer()
    acts, _ = b.register_actions([MANAGED, BLACKBOX])
    ns = b.register_namespaces([0xC0DE << 64 | k for k in range(300)])
    assert ns.tolist() == list(range(300))
    return b, acts, ns


# ---------------------------------------------------------------------------------------------- 1. literal semantics
def test_literal_counts_leak_and_first_tracker():
    b = GpuShardingContainerPoolBalancer()
    (m, x), _ = b.register_actions([MANAGED, BLACKBOX])
    A, B, C = ns = b.register_namespaces([11, 22, 33]).tolist()
    R, P, Q, S, T = fresh_ids(5)
    assert books(b, ns) == ([0, 0, 0], (0, 0, 0))
    # batch 1: R three times (A with the managed action, B with the blackbox one, A again)
    t, e = b.track_activations([R, P, R, Q, R, S], [m, x, x, m, m, x], [10, 11, 12, 13, 14, 15], ns=[A, B, B, C, A, C])
    assert t.tolist() == [10, 11, 10, 13, 10, 15] and e.tolist() == [0, 0, 1, 0, 1, 0]
    # every item counted, the two duplicates of R too: 3 managed x 256, 3 blackbox x 512
    assert books(b, ns) == ([2, 2, 2], (6, 768, 1536))
    assert b.activations_live() == 4
    # batch 2: P again, under C with the managed action: counted, the entry stays B / blackbox
    t, e = b.track_activations([P], [m], [20], ns=[C])
    assert (t[0], e[0]) == (11, 1)
    assert books(b, ns) == ([2, 2, 3], (7, 1024, 1536))
    # R completes: the first tracker's namespace (A) and action (managed) are subtracted; its two leaked counts stay
    k, t, _ = b.complete_activations([R], [0])
    assert (k[0], t[0]) == (ACK_RELEASED, 10)
    assert books(b, ns) == ([1, 2, 3], (6, 768, 1536))
    k, t, _ = b.complete_activations([R], [0])
    assert (k[0], t[0]) == (ACK_NOENTRY, -1)
    assert books(b, ns) == ([1, 2, 3], (6, 768, 1536))
    # P completes: B / blackbox of its first tracker, not C / managed of the later one
    k, t, _ = b.complete_activations([P, P], [0, 0], forced=[0, 1])
    assert k.tolist() == [ACK_RELEASED, ACK_FORCED_NOENTRY] and t.tolist() == [11, -1]
    assert books(b, ns) == ([1, 1, 3], (5, 768, 1024))
    # track_activations without ns: the totals move, no namespace does
    t, e = b.track_activations([T], [x], [30])
    assert (t[0], e[0]) == (30, 0)
    assert books(b, ns) == ([1, 1, 3], (6, 768, 1536))
    # an unknown handle and a malformed id change nothing
    before = books(b, ns), b.activations_live()
    for bad in (3, -2):
        with pytest.raises(OwgsError) as err:
            b.track_activations(fresh_ids(2), [m, m], [40, 41], ns=[A, bad])
        assert err.value.code == ENOENT
    with pytest.raises(OwgsError) as err:
        b.track_activations(fresh_ids(1) + ["XYZ" * 10 + "ab"], [m, m], [42, 43], ns=[A, B])
    assert err.value.code == EINVAL
    with pytest.raises(OwgsError) as err:
        b.active_activations_for([3])
    assert err.value.code == ENOENT
    assert (books(b, ns), b.activations_live()) == before


# ---------------------------------------------------------------------------------- 2. wave / block edges of counting
@pytest.mark.parametrize("pattern", ["same", "distinct", "alternating", "none_at_0_63"])
def test_counts_at_wave_and_block_edges(bal, pattern):
    b, (m, x), ns = bal
    for n in (1, 63, 64, 65, 129, 256, 257):
        i = np.arange(n)
        if pattern == "same":
            h = np.full(n, ns[7])
        elif pattern == "distinct":
            h = ns[i]
        elif pattern == "alternating":
            h = ns[3 + (i & 1)]
        else:
            h = ns[(i * 7) % 5]
            h[(i % 64 == 0) | (i % 64 == 63)] = NONE
        act = np.where(i % 3 == 0, x, m)
        ids = fresh_ids(n)
        t, e = b.track_activations(ids, act, i, ns=h)
        assert np.array_equal(t, i) and not e.any()
        want = np.bincount(h[h != NONE], minlength=len(ns)).astype(np.int32)
        assert np.array_equal(b.active_activations_for(ns), want), (pattern, n)
        nb = int((act == x).sum())
        assert b.activation_totals() == (n, 256 * (n - nb), 512 * nb), (pattern, n)
        k, t, _ = b.complete_activations(ids[::-1], np.zeros(n, np.int32))
        assert np.all(k == ACK_RELEASED) and np.array_equal(t, i[::-1])
        assert not b.active_activations_for(ns).any() and b.activation_totals() == (0, 0, 0), (pattern, n)


# ------------------------------------------------------------------------------------------ 3. flow against the oracle
def _publish_first_batch(w):
    """GPU and oracle states after the first batch of w's stream (no releases), as tests/test_gpu_acks.py does."""
    n = int(w.stream.acq_off[1])
    s1 = types.SimpleNamespace(acq_off=np.array([0, n]), act=w.stream.act[:n], rel_off=np.array([0, 0]),
                               rel_aid=np.zeros(0, np.int64), seq_base=w.stream.seq_base)
    st = O.state_for(w)
    o_inv, _, _ = st.replay(s1)
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, w.inv_status)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    g_inv, _, _ = b.replay(s1)
    assert np.array_equal(o_inv, g_inv)
    return b, st, g_inv, w.stream.act[:n]


def test_flow_matches_oracle_and_model():
    w = W.config("c4", n_activations=6000)
    b, st, inv, act = _publish_first_batch(w)
    b.set_health_tid(H)
    rng = np.random.default_rng(7)
    sched = np.nonzero(inv >= 0)[0]
    aids = W.activation_ids(rng, len(sched))
    handles = b.register_namespaces([0xFEED << 64 | k for k in range(200)])
    nsd = handles[W._zipf_sample(rng, 200, 1.0, len(sched))]
    flow = O.AckFlow(st, H)
    model = Books(w.actions)
    gt, gx = b.track_activations(aids, act[sched], sched, ns=nsd)
    for j, i in enumerate(sched):
        t, x = flow.track(aids[j], int(act[i]), int(i))
        assert (gt[j], gx[j]) == (t, x)
        model.track(int(nsd[j]), int(act[i]), int(i), x)
    model.check(b, handles)
    assert b.activations_live() == flow.live() == len(sched)
    # raw acks for 80 %: duplicates, unknown ids, health acks, garbage and combined messages mixed in
    part = rng.permutation(len(sched))[: int(0.8 * len(sched))]
    msgs = W.ack_batch(rng, [aids[j] for j in part], inv[sched[part]], H)
    ok, _, ot, of = flow.process_acks(msgs)
    gk, _, gtk, gf = b.process_acks(msgs)
    assert np.array_equal(ok, gk) and np.array_equal(ot, gtk) and np.array_equal(of, gf)
    released = ot[ok == ACK_RELEASED]
    assert len(released) > 0.7 * len(part)
    for t in released:
        model.release(int(t))
    model.check(b, handles)
    assert b.activations_live() == flow.live()
    assert np.array_equal(b.permits(), st.permits())
    # forced timeouts for everything the oracle still tracks, plus 50 already completed
    pos = {int(i): j for j, i in enumerate(sched)}
    done = np.array([pos[int(t)] for t in released])
    rest = np.setdiff1d(np.arange(len(sched)), done)
    ids = np.concatenate([rest, done[:50]])
    kk, tt, ff = b.complete_activations([aids[j] for j in ids], inv[sched[ids]], forced=np.ones(len(ids), np.uint8))
    for q, j in enumerate(ids):
        hi, lo = O.aid_words(aids[j])
        o, t, _, rf = flow.complete(hi, lo, int(inv[sched[j]]), True, False)
        assert (kk[q], tt[q], ff[q] >> 1) == (o, t, O._rel_bits(rf))
        if o == ACK_RELEASED:
            model.release(t)
    assert np.all(kk[:len(rest)] == ACK_RELEASED) and np.all(kk[len(rest):] == ACK_FORCED_NOENTRY)
    model.check(b, handles)
    assert b.activations_live() == flow.live() == 0
    assert not b.active_activations_for(handles).any() and b.activation_totals() == (0, 0, 0)
    assert np.array_equal(b.permits(), st.permits())


# -------------------------------------------------------------------------------------------------- 4. table rehash
def test_rehash_carries_the_namespace(bal):
    b, (m, x), ns = bal
    rng = np.random.default_rng(4)
    n = 20_000
    ids1, ids2 = fresh_ids(n), fresh_ids(n)
    h1, h2 = ns[rng.integers(0, 50, n)], ns[rng.integers(0, 50, n)]
    a1, a2 = np.where(rng.random(n) < .5, m, x), np.where(rng.random(n) < .5, m, x)
    b.track_activations(ids1, a1, np.arange(n), ns=h1)
    # 40,000 entries are more than half of the table's first 65,536 slots: this batch rehashes it
    b.track_activations(ids2, a2, np.arange(n, 2 * n), ns=h2)
    k, t, _ = b.complete_activations(ids1, np.zeros(n, np.int32))
    assert np.all(k == ACK_RELEASED) and np.array_equal(t, np.arange(n))
    assert np.array_equal(b.active_activations_for(ns), np.bincount(h2, minlength=len(ns)))
    nb = int((a2 == x).sum())
    assert b.activation_totals() == (n, 256 * (n - nb), 512 * nb)
    k, _, _ = b.complete_activations(ids2, np.zeros(n, np.int32))
    assert np.all(k == ACK_RELEASED)
    assert not b.active_activations_for(ns).any() and b.activation_totals() == (0, 0, 0)


# ----------------------------------------------------------------------------------------- 5. namespace array growth
def test_namespace_array_growth_keeps_counts():
    b = GpuShardingContainerPoolBalancer()
    (m,), _ = b.register_actions([MANAGED])
    uu = [0xABCD << 64 | (k * 2654435761) for k in range(2400)]
    h1 = b.register_namespaces(uu[:600])
    assert h1.tolist() == list(range(600)) and 600 < NS_INITIAL_CAP
    i1 = np.arange(0, 600, 7)
    b.track_activations(fresh_ids(len(i1) * 2), np.full(len(i1) * 2, m), np.arange(len(i1) * 2), ns=np.repeat(h1[i1], 2))
    h2 = b.register_namespaces(uu[600:1200])       # 1,200 > the first capacity: the array grows
    assert h2.tolist() == list(range(600, 1200)) and 1200 > NS_INITIAL_CAP
    want = np.zeros(2400, np.int32)
    want[i1] = 2
    assert np.array_equal(b.active_activations_for(np.arange(1200)), want[:1200])
    i2 = np.arange(590, 1200, 5)
    b.track_activations(fresh_ids(len(i2)), np.full(len(i2), m), np.arange(len(i2)), ns=i2)
    want[i2] += 1
    h3 = b.register_namespaces(uu[1100:2400])      # 100 known, 1,200 new: 2,400 > 2 x the first capacity
    assert h3.tolist() == list(range(1100, 2400)) and 2400 > 2 * NS_INITIAL_CAP
    assert np.array_equal(b.active_activations_for(np.arange(2400)), want)
    b.track_activations(fresh_ids(3), [m] * 3, [0, 1, 2], ns=[2399, 0, 2399])
    want[2399] += 2
    want[0] += 1
    assert np.array_equal(b.active_activations_for(np.arange(2400)), want)
    assert b.register_namespaces(uu).tolist() == list(range(2400))
    assert b.register_namespaces([uu[5], 0x77, uu[5], 0x77]).tolist() == [5, 2400, 5, 2400]
    assert b.activation_totals()[0] == int(want.sum())


# ---------------------------------------------------------------------------------------------------- 6. throttle
def throttle_model(active, ns, limits):
    """The definition: ActivationThrottler.check per job in array order, an admitted job counted (CLB:127)."""
    cur = dict(active)
    cnt, ok = [], []
    for h, lim in zip(ns, limits):
        c = cur[int(h)]
        o = c < int(lim)          # ConcurrentRateLimit.ok
        cnt.append(c)
        ok.append(int(o))
        cur[int(h)] = c + int(o)
    return np.array(cnt, np.int32), np.array(ok, np.uint8)


def test_throttle_hand_case():
    b = GpuShardingContainerPoolBalancer()
    (m,), _ = b.register_actions([MANAGED])
    (h,) = b.register_namespaces([5])
    b.track_activations(fresh_ids(2), [m, m], [0, 1], ns=[h, h])
    cnt, ok = b.throttle_batch([h] * 6, [3, 3, 3, 1, 4, 4])
    assert ok.tolist() == [1, 0, 0, 0, 1, 0] and cnt.tolist() == [2, 3, 3, 3, 3, 4]
    assert books(b, [h]) == ([2], (2, 512, 0))  # read-only
    with pytest.raises(OwgsError) as err:
        b.throttle_batch([h, NONE], [3, 3])
    assert err.value.code == EINVAL
    with pytest.raises(OwgsError) as err:
        b.throttle_batch([h, 1], [3, 3])
    assert err.value.code == ENOENT


def test_throttle_matches_the_definition(bal):
    b, (m, x), ns = bal
    five = ns[[0, 17, 63, 64, 299]]
    base = [3, 10, 45, 64, 130]
    h = np.repeat(five, base)
    ids = fresh_ids(len(h))
    b.track_activations(ids, np.full(len(h), m), np.arange(len(h)), ns=h)
    active = dict(zip(five.tolist(), base))
    before = books(b, ns)
    rng = np.random.default_rng(6)
    for n in (1, 64, 65, 1000):
        for rep in range(3):
            which = rng.integers(0, 5, n)
            bs = np.array(base)[which]
            lim = np.stack([np.zeros(n, np.int64), bs - 1, bs, bs + 1, bs + 40])[rng.integers(0, 5, n), np.arange(n)]
            cnt, ok = b.throttle_batch(five[which], lim)
            wc, wo = throttle_model(active, five[which], lim)
            assert np.array_equal(ok, wo) and np.array_equal(cnt, wc), (n, rep)
    # 257 jobs of one namespace with one limit that is reached mid-batch (three full waves and one job)
    cnt, ok = b.throttle_batch(np.full(257, five[2]), np.full(257, 45 + 100))
    assert ok.tolist() == [1] * 100 + [0] * 157
    assert cnt.tolist() == list(range(45, 145)) + [145] * 157
    # the same with a stricter limit on every third job: a true in-order dependency
    lim = np.where(np.arange(257) % 3 == 0, 45 + 20, 45 + 100)
    cnt, ok = b.throttle_batch(np.full(257, five[2]), lim)
    wc, wo = throttle_model(active, np.full(257, five[2]), lim)
    assert np.array_equal(ok, wo) and np.array_equal(cnt, wc)
    assert books(b, ns) == before  # read-only
    k, _, _ = b.complete_activations(ids, np.zeros(len(ids), np.int32))
    assert np.all(k == ACK_RELEASED)
    assert not b.active_activations_for(ns).any() and b.activation_totals() == (0, 0, 0)
