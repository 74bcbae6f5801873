"""The supervision feeds on the GPU (owgs_process_pings, owgs_process_acks_supervised,
owgs_complete_activations_supervised; owgs_feeds.hip, the ping parser in owgs_acks.hip) against the host model
(tests/feeds_model.py) and the oracles: oracle.HealthPool for the FSM, oracle.AckFlow for the completion path,
oracle.BalancerState for the scheduler the status vector is handed to."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from feeds_model import FAIL, FED, RANGE, ack_events, ping_model
from openwhisk_amd import GpuShardingContainerPoolBalancer, OwgsError, _lib
from openwhisk_amd import workload as W
from openwhisk_amd._lib import ACK_FORCED_NOENTRY, ACK_HEALTH, ACK_NOENTRY, ACK_RELEASED
from test_feeds_cpu import FUZZ_SEEDS, fuzz_messages, vectors

pytestmark = pytest.mark.gpu
H = 1700000000123
MB = 1 << 20
# 1, a wave and its neighbours, a few waves; then the compaction's tile of 1,024 items and its neighbours, two tiles + 1
EDGES = [1, 63, 64, 65, 256, 257, 1023, 1024, 1025, 2049]
NAMES = ("status", "mem", "tests", "ring", "tick")


def same_health(g, o):
    for name, a, b in zip(NAMES, g, o):
        assert np.array_equal(a, b), f"{name} differs at {np.flatnonzero(np.asarray(a) != np.asarray(b))[:8]}"


def expected_summary(before, after, n_ev):
    """(events, status entries changed or new, test actions) from the oracle's vectors around a batch."""
    k = len(before[0])
    changed = int(((before[0] != after[0][:k]) | (before[1] != after[1][:k])).sum()) + len(after[0]) - k
    return (n_ev, changed, int(after[2].sum()))


class Loop:
    """One controller: the GPU balancer with the device feeds beside the oracles, driven in lock step.  two_call=True
    drives the GPU through the older calls instead (process_acks / complete_activations, then a host-built
    health_events), which the supervised calls must equal."""

    def __init__(self, w, zombies=False, two_call=False):
        self.w, self.two_call = w, two_call
        self.b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction,
                                                  blackbox_fraction=w.blackbox_fraction, rng_seed=w.rng_seed)
        self.b.update_cluster(w.cluster_size)
        self.b.register_actions(w.actions)
        self.b.set_health_tid(H)
        self.st = O.BalancerState(w.managed_fraction, w.blackbox_fraction, rng_seed=w.rng_seed, zombies=zombies)
        self.st.update_cluster(w.cluster_size)
        keys = {}
        for a in w.actions:
            self.st.register_action(a.namespace, a.path, keys.setdefault(a.key, len(keys)), a.mem_mb,
                                    a.max_concurrent, a.blackbox)
        self.flow = O.AckFlow(self.st, H)
        self.hp = O.HealthPool()
        self.seq = 0
        # the in-flight books as CLB:121-127 / 280-284 keep them: total, managed MB, blackbox MB; entries by ticket
        self.books, self.entry, self.next_ticket = [0, 0, 0], {}, 0

    def _count(self, action, sign):
        a = self.w.actions[int(action)]
        self.books[0] += sign
        self.books[2 if a.blackbox else 1] += sign * a.mem_mb

    def _hand(self, apply, changed):
        """The oracle's updateInvokers when the device hands its vector over."""
        if apply == 1 or (apply == 2 and changed > 0):
            s, m = self.hp.read()[:2]
            self.st.update_invokers(np.arange(len(s), dtype=np.int32), m, s)
            return True
        return False

    def _check(self, summ, before, n_ev, apply):
        after = self.hp.read()
        exp = expected_summary(before, after, n_ev)
        if summ is not None:
            assert summ == exp
        same_health(self.b.health_read(), after)
        self._hand(apply, exp[1])
        return exp

    def pings(self, msgs, t_ms, now, apply=0):
        kind, inst, mem = ping_model(msgs)
        t = np.asarray(t_ms, dtype=np.int64)
        fed = kind == FED
        before = self.hp.read()
        self.hp.events(inst[fed], np.zeros(fed.sum(), np.uint8), t[fed], mem[fed], now)
        summ = None
        if self.two_call:
            exp = expected_summary(before, self.hp.read(), int(fed.sum()))
            self.b.health_events(inst[fed], np.zeros(fed.sum(), np.uint8), t[fed], mem[fed], now,
                                 apply=apply == 1 or (apply == 2 and exp[1] > 0))
        else:
            gk, gi, gm, summ = self.b.process_pings(msgs, t, now, apply=apply)
            bad = np.flatnonzero(gk != kind)
            assert len(bad) == 0, [(msgs[i], int(gk[i]), int(kind[i])) for i in bad[:3]]
            assert np.array_equal(gi, inst) and np.array_equal(gm, mem)
        return self._check(summ, before, int(fed.sum()), apply)

    def _feed(self, ev_inv, ev_kind, now, apply, summ, before):
        if len(ev_inv) == 0:  # nothing for the pool: its clock stays
            assert summ is None or summ == (0, 0, 0)
            same_health(self.b.health_read(), self.hp.read())
            if apply == 1:
                self._hand(1, 0)
            return (0, 0, 0)
        z = np.zeros(len(ev_inv), np.int64)
        self.hp.events(ev_inv, ev_kind, z + now, z, now)
        if self.two_call:
            exp = expected_summary(before, self.hp.read(), len(ev_inv))
            self.b.health_events(ev_inv, ev_kind, z + now, z, now, apply=apply == 1 or (apply == 2 and exp[1] > 0))
        return self._check(summ, before, len(ev_inv), apply)

    def acks(self, msgs, now, apply=0):
        ok, oi, ot, of = self.flow.process_acks(msgs)
        before = self.hp.read()
        summ = None
        if self.two_call:
            gk, gi, gt, gf = self.b.process_acks(msgs)
        else:
            gk, gi, gt, gf, summ = self.b.process_acks_supervised(msgs, now, apply=apply)
        bad = np.flatnonzero(ok != gk)
        assert len(bad) == 0, [(msgs[i], int(gk[i]), int(ok[i])) for i in bad[:3]]
        comp = ok >= ACK_RELEASED
        assert np.array_equal(oi[comp], gi[comp]) and np.array_equal(ot, gt) and np.array_equal(of, gf)
        for t in ot[ok == ACK_RELEASED]:
            self._count(self.entry.pop(int(t)), -1)
        ev_inv, ev_kind = ack_events(ok, oi, of)
        return gk, self._feed(ev_inv, ev_kind, now, apply, summ, before)

    def complete(self, aids, invokers, now, apply=0, forced=None, system_error=None, health=None):
        n = len(aids)
        fo, se, he = (np.zeros(n, np.uint8) if x is None else np.asarray(x, np.uint8)
                      for x in (forced, system_error, health))
        before = self.hp.read()
        summ = None
        if self.two_call:
            gk, gt, gf = self.b.complete_activations(aids, invokers, forced=fo, system_error=se, health=he)
        else:
            gk, gt, gf, summ = self.b.complete_activations_supervised(aids, invokers, now, apply=apply, forced=fo,
                                                                      system_error=se, health=he)
        ok = np.zeros(n, np.uint8)
        for q in range(n):
            hi, lo = O.aid_words(aids[q])
            o, t, a, rf = self.flow.complete(hi, lo, int(invokers[q]), bool(fo[q]), bool(he[q]))
            assert (gk[q], gt[q], gf[q] >> 1, gf[q] & 1) == (o, t, O._rel_bits(rf), se[q]), q
            if o == ACK_RELEASED:
                assert self.entry.pop(t) == a
                self._count(a, -1)
            ok[q] = o
        ev_inv, ev_kind = ack_events(ok, np.asarray(invokers), se, forced=fo)
        return gk, self._feed(ev_inv, ev_kind, now, apply, summ, before)

    def publish(self, acts):
        gi, _ = self.b.publish(acts, seq_base=self.seq)
        oi = [self.st.publish(int(a), self.seq + k)[0] for k, a in enumerate(acts)]
        self.seq += len(acts)
        assert gi.tolist() == oi
        return gi

    def track(self, aids, acts):
        """setupActivation's entry and counts for each id; tickets are this controller's own, never reused."""
        tickets = np.arange(self.next_ticket, self.next_ticket + len(aids))
        self.next_ticket += len(aids)
        gt, gx = self.b.track_activations(aids, acts, tickets)
        for j, aid in enumerate(aids):
            t, x = self.flow.track(aid, int(acts[j]), int(tickets[j]))
            assert (gt[j], gx[j]) == (t, x)
            self._count(acts[j], 1)
            if not x:
                self.entry[int(tickets[j])] = int(acts[j])

    def same_books(self):
        """Permits, activationSlots and the in-flight books (totalActivations and the two memory totals) equal the
        oracle flow's."""
        assert np.array_equal(self.b.permits(), self.st.permits())
        assert self.b.activations_live() == self.flow.live() == len(self.entry)
        assert tuple(self.b.activation_totals()) == tuple(self.books)


def register_all(lp, n, mem_mb, t=0, apply=2):
    """Pings of ids 0..n-1 at time t, then a health test action's ack of each: every invoker Healthy, handed over."""
    exp = lp.pings([W.ping_message(i, "%d MB" % mem_mb[i]) for i in range(n)], np.full(n, t), t, apply=apply)
    assert exp == (n, n, n)  # registration sends each new actor its first test action (ISUP:351-361)
    assert np.all(lp.hp.read()[0] == O_UNHEALTHY)
    rng = np.random.default_rng(99)
    msgs = [W.completion_message(a, i, tid=("sid_invokerHealth", H))
            for i, a in enumerate(W.activation_ids(rng, n))]
    gk, exp = lp.acks(msgs, t + 1, apply=apply)
    assert np.all(gk == ACK_HEALTH) and exp[:2] == (n, n)
    st, mem = lp.hp.read()[:2]
    assert np.all(st == O_HEALTHY) and np.array_equal(mem, np.asarray(mem_mb, np.int64) * MB)


O_HEALTHY, O_UNHEALTHY, O_UNRESPONSIVE, O_OFFLINE = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------------- the ping parser
def test_ping_vectors_give_the_models_outcome():
    vs = vectors()
    b = GpuShardingContainerPoolBalancer()
    msgs = [v["msg"].encode("utf-8") for v in vs]
    gk, gi, gm, summ = b.process_pings(msgs, np.zeros(len(msgs), np.int64), 0)
    for i, v in enumerate(vs):
        assert (int(gk[i]), int(gi[i]), int(gm[i])) == (v["kind"], v["instance"], v["bytes"]), v["name"]
    assert summ[0] == sum(v["kind"] == FED for v in vs)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_ping_fuzz_matches_the_model(seed):
    msgs = fuzz_messages(seed)
    kind, inst, mem = ping_model(msgs)
    assert all((kind == k).any() for k in (FAIL, FED, RANGE))
    b = GpuShardingContainerPoolBalancer()
    gk, gi, gm, _ = b.process_pings(msgs, np.zeros(len(msgs), np.int64), 0)
    bad = np.flatnonzero((gk != kind) | (gi != inst) | (gm != mem))
    assert len(bad) == 0, [(msgs[i], int(gk[i]), int(kind[i]), int(gi[i]), int(inst[i])) for i in bad[:3]]


# ------------------------------------------------------------------------------------------------ compaction edges
def _small():
    return W.config("c4", n_activations=6_000, n_invokers=40)


@pytest.fixture(scope="module")
def small():
    return _small()


@pytest.mark.parametrize("n", EDGES)
def test_ping_compaction_edges(n):
    """Every third message is garbage, ids repeat and leave gaps: the FSM sees the FED subset in order, and the padded
    entries take the userMemory of the ping that grew the vector past them (ISUP:196-199)."""
    lp = Loop.__new__(Loop)
    lp.two_call, lp.b, lp.hp, lp.st = False, GpuShardingContainerPoolBalancer(), O.HealthPool(), None
    lp._hand = lambda apply, changed: False
    msgs, t = [], []
    for i in range(n):
        if i % 3 == 1:
            msgs.append(b'{"name":{"instance":%d,"userMemory":"1 MB"' % i)
        else:
            msgs.append(W.ping_message(((i * 5) % 97) * 2, "%d MB" % (128 + i % 61)))  # even ids: odd ones are padded
        t.append(i // 4)
    exp = lp.pings(msgs, t, t[-1] + 5)
    assert exp[0] == n - (n + 1) // 3
    st, mem = lp.hp.read()[:2]
    if n >= 3:
        assert (st[1::2] == O_OFFLINE).all() and (mem[1::2] > 0).all()
    # a second batch of the same pings 12 s later: the actors exist, nothing registers, Offline ones come back
    lp.pings(msgs, [12_000 + x for x in t], 12_000 + t[-1])


def _ack_mix(lp, n, rng, acts, now):
    """n ack messages: RELEASED, NOENTRY duplicates, HEALTH and garbage interleaved, over freshly tracked ids."""
    k = max(1, n // 2)
    inv = lp.publish(acts[:k])
    ok = np.flatnonzero(inv >= 0)
    aids = W.activation_ids(rng, len(ok))
    lp.track(aids, acts[:k][ok])
    msgs, j = [], 0
    while len(msgs) < n:
        r = len(msgs) % 4
        if r == 0 and j < len(aids):
            msgs.append(W.completion_message(aids[j], int(inv[ok[j]]), system_error=j % 5 == 0))
            j += 1
        elif r == 1 and j > 0:
            msgs.append(W.completion_message(aids[j - 1], int(inv[ok[j - 1]])))  # its entry is gone: NOENTRY
        elif r == 2:
            msgs.append(W.completion_message(W.activation_ids(rng, 1)[0], int(rng.integers(0, 45)),
                                             tid=("sid_invokerHealth", H)))  # ids 40..44 have no actor
        else:
            msgs.append(W.completion_message(aids[0], 3)[:-2])
    gk, exp = lp.acks(msgs, now, apply=2)
    return gk, exp


def test_ack_compaction_edges(small):
    lp = Loop(small)
    register_all(lp, 40, small.inv_mem // MB)
    rng = np.random.default_rng(5)
    acts = small.stream.act
    now = 10
    seen = set()
    for n in EDGES:
        gk, exp = _ack_mix(lp, n, rng, acts[rng.integers(0, len(acts), size=n)], now)
        seen |= set(gk.tolist())
        lp.same_books()
        now += 7
    assert {ACK_RELEASED, ACK_NOENTRY, ACK_HEALTH, 0} <= seen


# ------------------------------------------------------------------------------------------------- the closed loop
def closed_loop(lp):
    w = lp.w
    n = len(w.inv_ids)
    register_all(lp, n, w.inv_mem // MB)
    assert lp.b.managed_size == lp.st.managed_size and lp.b.blackbox_size == lp.st.blackbox_size
    a0, a1, a2 = (int(x) for x in w.stream.acq_off[:3])
    inv = lp.publish(w.stream.act[a0:a1])
    ok = np.flatnonzero(inv >= 0)
    assert len(ok) > 200
    rng = np.random.default_rng(3)
    aids = W.activation_ids(rng, len(ok))
    lp.track(aids, w.stream.act[a0:a1][ok])
    # the five busiest invokers of the batch return only system errors
    cnt = np.bincount(inv[ok], minlength=n)
    bad5 = np.argsort(-cnt, kind="stable")[:5]
    assert cnt[bad5].min() >= 4  # more than the tolerance of 3 (ISUP:438)
    order = rng.permutation(len(ok))
    msgs = []
    for j in order:
        i = int(inv[ok[j]])
        msgs.append(W.completion_message(aids[j], i, system_error=i in bad5))
        if j % 17 == 0:
            msgs.append(msgs[-1])  # duplicate: NOENTRY, feeds nothing
        if j % 23 == 0:
            msgs.append(b"{" + msgs[-1])
    gk, exp = lp.acks(msgs, 5_000, apply=2)
    assert (gk == ACK_RELEASED).sum() == len(ok) and exp[1] >= 5
    st = lp.hp.read()[0]
    assert (st[bad5] == O_UNHEALTHY).all() and (np.delete(st, bad5) == O_HEALTHY).all()
    lp.same_books()
    assert lp.b.activation_totals()[0] == lp.flow.live() == 0
    nxt = lp.publish(w.stream.act[a1:a2])
    assert not np.isin(nxt, bad5).any() and (nxt >= 0).any()
    lp.same_books()
    return lp.b.health_read(), lp.b.permits(), nxt


def test_closed_loop_on_a_small_pool(small):
    """pings -> Unhealthy -> health acks -> Healthy -> publish -> system errors -> Unhealthy -> the next publish skips
    them; and the same through process_acks + a host-built health_events: supervised equals the two-call path."""
    h1, p1, n1 = closed_loop(Loop(small))
    h2, p2, n2 = closed_loop(Loop(small, two_call=True))
    same_health(h1, h2)
    assert np.array_equal(p1, p2) and np.array_equal(n1, n2)


def test_apply_2_leaves_the_scheduler_alone_when_nothing_changes(small):
    lp = Loop(small)
    n = len(small.inv_ids)
    register_all(lp, n, small.inv_mem // MB)
    acts = small.stream.act[:290]
    inv = lp.publish(acts)
    ok = np.flatnonzero(inv >= 0)
    aids = W.activation_ids(np.random.default_rng(8), len(ok))
    lp.track(aids, acts[ok])
    half = len(ok) // 2
    # the oracle's scheduler gets no updateInvokers here (Loop._hand only calls it on a change): equal permits and
    # decisions afterwards show the device handed nothing over, or handed over what changes nothing
    _, exp = lp.acks([W.completion_message(aids[j], int(inv[ok[j]])) for j in range(half)], 100, apply=2)
    assert exp == (half, 0, 0)
    lp.same_books()
    lp.publish(small.stream.act[290:580])
    mirror = lp._hand
    lp._hand = lambda apply, changed: False  # apply = 1 hands an unchanged vector over: the oracle still gets nothing
    _, exp = lp.acks([W.completion_message(aids[j], int(inv[ok[j]])) for j in range(half, len(ok))], 200, apply=1)
    lp._hand = mirror
    assert exp[1] == 0
    lp.same_books()
    lp.publish(small.stream.act[580:870])
    lp.same_books()


def test_complete_activations_supervised(small):
    lp = Loop(small)
    n = len(small.inv_ids)
    register_all(lp, n, small.inv_mem // MB)
    acts = small.stream.act[:64]
    inv = lp.publish(acts)
    ok = np.flatnonzero(inv >= 0)[:8]
    aids = W.activation_ids(np.random.default_rng(9), 10)
    lp.track(aids[:8], acts[ok])
    # four forced completions name invoker 3 (the call's invoker, not the entry's): four Timeouts -> Unresponsive;
    # a forced item without an entry feeds nothing; bit 2 without an entry is a health ack: Success for invoker 7
    ids = aids[:4] + [aids[8], aids[9]]
    gk, exp = lp.complete(ids, [3, 3, 3, 3, 5, 7], 50, apply=2, forced=[1, 1, 1, 1, 1, 0], health=[0, 0, 0, 0, 0, 1])
    assert gk.tolist() == [ACK_RELEASED] * 4 + [ACK_FORCED_NOENTRY, ACK_HEALTH]
    assert exp[0] == 5 and exp[1] == 1
    st, _, _, ring, _ = lp.hp.read()
    assert st[3] == O_UNRESPONSIVE and st[5] == O_HEALTHY and (ring[5] >> 20) == 1 and (ring[7] >> 20) == 2
    lp.same_books()
    # the rest regular, with a system error, at a later time; then an empty call
    gk, exp = lp.complete(aids[4:8], inv[ok[4:8]], 60, apply=2, system_error=[0, 1, 0, 0])
    assert gk.tolist() == [ACK_RELEASED] * 4 and exp[0] == 4
    lp.complete([], [], 70, apply=1)
    lp.same_books()
    nxt = lp.publish(small.stream.act[64:200])
    assert 3 not in nxt.tolist()


def test_health_events_hands_over_for_any_non_zero_apply():
    """owgs_health_events' contract is `apply != 0`: 2 (the feeds' change-only mode elsewhere) hands the vector over here
    even when the batch changes no entry."""
    b = GpuShardingContainerPoolBalancer()
    ids, mem = np.arange(6, dtype=np.int32), np.full(6, 2048 * MB, np.int64)
    b.health_events(ids, np.zeros(6, np.uint8), np.zeros(6, np.int64), mem, 0)            # registered, not handed over
    b.health_events(ids, np.ones(6, np.uint8), np.ones(6, np.int64), mem, 1)              # Healthy, not handed over
    assert len(b.permits()) == 0
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k, t = np.ones(6, np.uint8), np.full(6, 2, np.int64)
    before = b.health_read()
    assert b._L.owgs_health_events(b._h, 6, P(ids), P(k), P(t), P(mem), 2, 2) == 0        # Success on Healthy: no change
    same_health(b.health_read()[:2], before[:2])
    assert len(b.permits()) == 6
    b2 = GpuShardingContainerPoolBalancer()
    b2.health_events(ids, np.zeros(6, np.uint8), np.zeros(6, np.int64), mem, 0)
    b2.health_events([], [], [], [], 1, apply=2)                                           # through the Python method
    assert len(b2.permits()) == 6


# ------------------------------------------------------------------------------------------------------- errors
def test_errors_change_nothing(small):
    lp = Loop(small)
    n = len(small.inv_ids)
    register_all(lp, n, small.inv_mem // MB, t=1_000)
    acts = small.stream.act[:100]
    inv = lp.publish(acts)
    ok = np.flatnonzero(inv >= 0)
    aids = W.activation_ids(np.random.default_rng(4), len(ok))
    lp.track(aids, acts[ok])
    b = lp.b
    health, permits, live = b.health_read(), b.permits(), b.activations_live()

    def unchanged():
        same_health(b.health_read(), health)
        assert np.array_equal(b.permits(), permits) and b.activations_live() == live

    msgs = [W.completion_message(aids[j], int(inv[ok[j]]), system_error=True) for j in range(len(ok))]
    for now in (1_000, -1, 1 << 60):  # the FSM's clock stands at 1,001
        with pytest.raises(OwgsError) as e:
            b.process_acks_supervised(msgs, now, apply=1)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(OwgsError):
            b.complete_activations_supervised(aids[:3], inv[ok[:3]], now, forced=[1, 1, 1])
        unchanged()
    with pytest.raises(OwgsError):
        b.process_acks_supervised(msgs, 2_000, apply=3)
    # a NULL out_summary with a live context and otherwise valid arguments
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    one = W.ping_message(1, "1 MB")
    buf, off, t1 = np.frombuffer(one + b"\0", np.uint8), np.array([0, len(one)], np.int64), np.array([2_000], np.int64)
    k8, i32, t32, f8, m64 = (np.zeros(1, d) for d in (np.uint8, np.int32, np.int32, np.uint8, np.int64))
    aid1 = np.frombuffer(aids[0].encode("ascii"), np.uint8)
    inv1, cf1 = np.array([int(inv[ok[0]])], np.int32), np.zeros(1, np.uint8)
    L, h = b._L, b._h
    assert L.owgs_process_pings(h, 1, P(buf), P(off), P(t1), 2_000, 0, P(k8), P(i32), P(m64), None) == _lib.EINVAL
    assert L.owgs_process_acks_supervised(h, 1, P(buf), P(off), P(k8), P(i32), P(t32), P(f8), 2_000, 0, None) \
        == _lib.EINVAL
    assert L.owgs_complete_activations_supervised(h, 1, P(aid1), P(inv1), P(cf1), P(k8), P(t32), P(f8), 2_000, 0,
                                                  None) == _lib.EINVAL
    unchanged()
    pings = [W.ping_message(1, "1 MB"), b"garbage", W.ping_message(50, "2 MB")]
    for t, now in (([2_000, 1_999, 2_000], 2_000),   # a decreasing time at the garbage message
                   ([1_000, 2_000, 2_000], 2_000),   # before the previous batch's now
                   ([2_000, 2_000, 2_000], 1_999),   # now before the last message
                   ([2_000, 2_000, 1 << 60], 1 << 60)):
        with pytest.raises(OwgsError) as e:
            b.process_pings(pings, t, now, apply=1)
        assert e.value.code == _lib.EINVAL
        unchanged()
    gk, _ = lp.acks(msgs, 1_001, apply=2)  # and the batch still goes through at the clock's own time
    assert (gk == ACK_RELEASED).all()


# ------------------------------------------------------------------------------------------------- large state
def test_large_state_context_registers_and_runs_through_the_feeds():
    mx, ms = C.c_int32(), C.c_int32()
    _lib.lib().owgs_limits(C.byref(mx), C.byref(ms))
    n = mx.value + 2_100
    w = W.config("headline", n_activations=2_000, n_invokers=n)
    assert len(w.inv_ids) == n > mx.value
    lp = Loop(w, zombies=True)
    mem_mb = w.inv_mem // MB
    # the status vector grows to n - 2,049, then by 1,024, then by 1,025 entries: one ping batch each
    lo = 0
    for t, hi in enumerate((n - 2_049, n - 1_025, n)):
        ids = np.arange(lo, hi)
        exp = lp.pings([W.ping_message(int(i), "%d MB" % mem_mb[i]) for i in ids], np.full(len(ids), t), t, apply=2)
        assert exp == (hi - lo, hi - lo, hi - lo)
        lo = hi
    assert len(lp.b.health_read()[0]) == n
    rng = np.random.default_rng(2)
    gk, exp = lp.acks([W.completion_message(a, i, tid=("sid_invokerHealth", H))
                       for i, a in enumerate(W.activation_ids(rng, n))], 3, apply=2)
    assert exp[:2] == (n, n) and (lp.hp.read()[0] == O_HEALTHY).all()
    assert lp.b.large_stats() is not None
    acts = w.stream.act[:300]
    inv = lp.publish(acts)
    ok = np.flatnonzero(inv >= 0)
    aids = W.activation_ids(rng, len(ok))
    lp.track(aids, acts[ok])
    bad = int(inv[ok[0]])
    msgs = [W.completion_message(aids[j], int(inv[ok[j]]), system_error=int(inv[ok[j]]) == bad)
            for j in range(len(ok))]
    msgs += [W.completion_message(aids[0], bad, system_error=True)] * 2 + [b"[]"]
    msgs += [W.completion_message(W.activation_ids(rng, 1)[0], bad, system_error=True,
                                  tid=("sid_invokerHealth", H))] * 4
    gk, exp = lp.acks(msgs, 4, apply=2)
    assert lp.hp.read()[0][bad] == O_UNHEALTHY and exp[1] == 1
    lp.same_books()
    nxt = lp.publish(w.stream.act[300:600])
    assert bad not in nxt.tolist()
    lp.same_books()
