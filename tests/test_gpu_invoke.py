"""owgs_invoke_activations on the device: the throttle gate feeding publish in one call.

Every case is compared bit for bit with tests/invoke_model.py (admit_model + PublishModel over the admitted sub-batch,
messages from the oracle's serialiser) and with a twin context driven through admit_batch, a host filter and
publish_activations.  The pool is small on purpose: 8 invokers of 512 MB, actions of 128 and 256 MB and a concurrent one,
so that it fills and the overload fallback's sequence numbers matter; 5 namespaces with 3 invokes / 3 fires per minute
and 2 concurrent invocations, so that all three verdicts appear.  Items that must pass carry overrides.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle as O
from invoke_model import InvokeModel
from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd import workload as W
from openwhisk_amd._lib import (ADMIT_CONCURRENT, ADMIT_OK, ADMIT_RATE, EINVAL, ENOENT, NONE, NOT_PUBLISHED, OFFLINE,
                                OwgsError)
from openwhisk_amd.balancer import Action, _msg_io, _p
from publish_model import PublishModel

pytestmark = pytest.mark.gpu
H = 1700000000123
MB = 2**20
ACT, TRIG, RO, CO = 0, 1, 2, 4
BIGLIM = 1_000_000
SMALL = Action("ns", "ns/small", "0.0.1", 128)
BIG = Action("ns", "ns/big", "0.0.1", 256)
CONC = Action("ns", "ns/conc", "0.0.1", 128, 3)
WIDE = Action("ns", "ns/wide", "0.0.1", 128, 4096)          # beyond the on-chip engine: a large-state context
TA = ['"action":{"path":"ns","name":"a%d"},"revision":null,"user":{"subject":"s%d"}' % (k, k) for k in range(3)]
TB = ["[]", '["x1"]', "[]"]
RCI = '{"asString":"7"}'
N_TOPICS = 8
_next_id = itertools.count(1)


def fresh_ids(n):
    return ["%032x" % (0xE7 << 100 | next(_next_id)) for _ in range(n)]


class Ctx:
    """A balancer with its oracle state and model; gpu=False: the model alone."""

    def __init__(self, actions=(SMALL, BIG, CONC), status=None, limits=(3, 3, 2), seed=3, gpu=True):
        ids, mem = np.arange(8), np.full(8, 512 * MB)
        st8 = np.zeros(8, np.uint8) if status is None else np.asarray(status, np.uint8)
        self.st = O.BalancerState(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=seed)
        self.st.update_invokers(ids, mem, st8)
        self.hs = [self.st.register_action(a.namespace, a.path, k, a.mem_mb, a.max_concurrent, a.blackbox)
                   for k, a in enumerate(actions)]
        self.m = InvokeModel(PublishModel(self.st, dict(zip(self.hs, actions)), H), limits)
        self.ns = np.arange(5, dtype=np.int32)
        self.b = None
        if gpu:
            b = self.b = GpuShardingContainerPoolBalancer(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=seed)
            b.update_invokers_arrays(ids, mem, st8)
            hs, _ = b.register_actions(list(actions))
            assert list(hs) == self.hs
            b.set_health_tid(H)
            b.set_throttle_limits(*limits)
            assert b.register_templates(TA, TB) == 0
            b.set_root_controller(RCI)
            assert b.register_namespaces([0xC0DE << 64 | k for k in range(5)]).tolist() == self.ns.tolist()

    @classmethod
    def around(cls, b, st, hs, actions, limits=(3, 3, 2), cluster=1):
        """The model beside a balancer b and its oracle state st that already hold invokers and the actions `hs`
        (tests/test_gpu_lifetime.py): sets up b's message and throttle state as the constructor does."""
        self = cls.__new__(cls)
        self.st, self.b, self.hs, self.ns = st, b, list(hs), np.arange(5, dtype=np.int32)
        self.m = InvokeModel(PublishModel(st, dict(zip(self.hs, actions)), H), limits, cluster)
        b.set_health_tid(H)
        b.set_throttle_limits(*limits)
        assert b.register_templates(TA, TB) == 0
        b.set_root_controller(RCI)
        assert b.register_namespaces([0xC0DE << 64 | k for k in range(5)]).tolist() == self.ns.tolist()
        return self


class Batch:
    """n items.  reject: positions that are rate-rejected for certain (rate override 0: limit 0).  forced: every other
    item is an action that passes for certain (both overrides huge); else a mix of triggers, items on the low default
    limits and items with overrides."""

    def __init__(self, rng, n, hs, t0, reject=(), forced=True):
        self.n = n
        self.ns = rng.integers(0, 5, n).astype(np.int32)
        self.acts = np.asarray(hs, np.int32)[rng.integers(0, len(hs), n)]
        self.t = t0 + np.arange(n, dtype=np.int64)
        self.ro = np.full(n, BIGLIM, np.int32)
        self.co = np.full(n, BIGLIM, np.int32)
        if forced:
            self.kind = np.full(n, RO | CO, np.uint8)
        else:
            over = rng.random(n) < 0.7
            self.kind = (np.where(over, RO | CO, 0) | np.where(rng.random(n) < 0.15, TRIG, 0)).astype(np.uint8)
        for i in reject:
            self.kind[i] |= RO
            self.ro[i] = 0
        self.aids = fresh_ids(n)
        self.tks = (np.arange(n) + 1000 * int(rng.integers(1, 1000))).astype(np.int32)
        self.lims = np.array([100, 61_000, 300_000])[rng.integers(0, 3, n)]
        tids = ["sid_%d" % k for k in range(n)]
        tids[n // 2] = "café € \U0001F600 \"q\"\n"
        self.M = dict(tmpl=np.arange(n, dtype=np.int32) % 3, tids=tids,
                      tid_start=np.arange(n) + 1_700_000_000_000, flags=rng.integers(0, 32, n).astype(np.uint8),
                      contents=['{"p":"%s"}' % ("x" * int(rng.integers(0, 60))) for _ in range(n)],
                      causes=rng.integers(0, 2**62, size=(n, 2)).astype(np.uint64),
                      traces=['{"t":"%d"}' % k for k in range(n)])

    def sub_msgs(self, idx):
        M = self.M
        return dict(tmpl=M["tmpl"][idx], tids=[M["tids"][i] for i in idx], tid_start=M["tid_start"][idx],
                    flags=M["flags"][idx], contents=[M["contents"][i] for i in idx], causes=M["causes"][idx],
                    traces=[M["traces"][i] for i in idx])


def state_of(b, handles):
    return (b.permits().tolist(), b.active_activations_for(handles).tolist(), b.activation_totals(),
            b.activations_live(), [x.tolist() for w in (0, 1) for x in b.rate_state(handles, w)])


def check_state(cx, twin=None):
    """permits, books, totals, live entries and both rate records against the model (and the twin)."""
    b, m = cx.b, cx.m
    assert np.array_equal(b.permits(), cx.st.permits())
    assert (b.active_activations_for(cx.ns).tolist(), b.activation_totals()) == m.pm.t.books(cx.ns)
    assert b.activations_live() == m.pm.t.live()
    for which in (0, 1):
        last, cnt = b.rate_state(cx.ns, which)
        assert (last.tolist(), cnt.tolist()) == m.rate_records(cx.ns, which)
    if twin is not None:
        assert state_of(b, cx.ns) == state_of(twin.b, cx.ns)


def sweep(b, now):
    aids, tk, inv, dl, fl, rem = b.expire_activations(now)
    return [(a, int(t), int(i), int(d), int(f)) for a, t, i, d, f in zip(aids, tk, inv, dl, fl)], rem


def check_sweep(cx, now, twin=None):
    """the order of an expiry sweep ten minutes on (the arm order across the skipped items)"""
    got = sweep(cx.b, now + 600_000)
    assert got == cx.m.pm.t.expire(now + 600_000)
    if twin is not None:
        assert got == sweep(twin.b, now + 600_000)
    check_state(cx, twin)
    return got


def run(cx, B, now, seq=None, seq_base=0, twin=None, waits=1, n_topics=N_TOPICS):
    """One call on the model, the device and (optionally) the twin context's separate calls; everything must agree.
    Returns the device's outputs."""
    want = cx.m.invoke(B.ns, B.kind, B.t, B.acts, B.aids, B.tks, B.lims, now, B.ro, B.co, seq, seq_base)
    words = np.array([O.aid_words(a) for a in B.aids], dtype=np.uint64)
    M = B.M
    wmsg = O.serialize_activations(TA, TB, RCI, np.where(want[5] >= 0, want[5], -1).astype(np.int32), M["tmpl"], words,
                                   M["tids"], M["tid_start"], M["flags"], M["contents"], M["causes"], M["traces"],
                                   n_topics=n_topics)
    got = cx.b.invoke_activations(B.ns, B.kind, B.t, B.acts, B.aids, B.tks, B.lims, now, rate_override=B.ro,
                                  conc_override=B.co, seq=seq, seq_base=seq_base,
                                  msgs=dict(M, n_topics=n_topics, cap=len(wmsg[0])))
    names = ("verdict", "rate_count", "rate_limit", "conc_count", "conc_limit", "invoker", "flags", "ticket", "existed")
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), name
        assert got[k].dtype == want[k].dtype, name
    summ = got[9].tolist()
    assert summ[:6] == want[9][:6] and summ[6] == 3 and summ[7] == 0 and summ[8:12] == want[9][8:12]
    assert summ[12] == waits and summ[13:] == [0, 0, 0]
    assert got[10][0] == wmsg[0]
    for k in (1, 2, 3):
        assert np.array_equal(got[10][k], wmsg[k]), k
    if twin is not None:
        tb = twin.b
        gate = tb.admit_batch(B.ns, B.kind, B.t, B.ro, B.co)
        for k in range(5):
            assert np.array_equal(gate[k], got[k]), names[k]
        adm = np.nonzero(((B.kind & TRIG) == 0) & (gate[0] == ADMIT_OK))[0]
        assert len(adm) == summ[8]
        if len(adm):
            p = tb.publish_activations(B.acts[adm], [B.aids[i] for i in adm], B.tks[adm], B.lims[adm], now,
                                       ns=B.ns[adm], seq=None if seq is None else np.asarray(seq, np.uint64)[adm],
                                       seq_base=seq_base, msgs=dict(B.sub_msgs(adm), n_topics=n_topics,
                                                                    cap=len(wmsg[0])))
            for k in range(4):
                assert np.array_equal(p[k], got[5 + k][adm]), names[5 + k]
            assert p[4].tolist()[:6] == summ[:6]
            assert p[5][0] == got[10][0] and np.array_equal(p[5][1], got[10][1])
            assert np.array_equal(adm[p[5][2]], got[10][2]) and np.array_equal(p[5][3], got[10][3])
        rest = np.setdiff1d(np.arange(B.n), adm)
        assert np.all(got[5][rest] == NOT_PUBLISHED) and not got[6][rest].any()
        assert np.all(got[7][rest] == -1) and not got[8][rest].any()
    check_state(cx, twin)
    return got


def boundary_positions(n):
    """0, n - 1 and each side of every multiple of 64 (those of 256 among them)"""
    pos = {0, n - 1}
    for edge in range(64, n, 64):
        pos |= {edge - 1, edge}
    return sorted(p for p in pos if 0 <= p < n)


# ------------------------------------------------------------------------------------------- compaction boundaries
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_compaction_boundaries(n):
    cx, tw = Ctx(), Ctx()
    rng = np.random.default_rng(100 + n)
    rej = boundary_positions(n)
    g = run(cx, Batch(rng, n, cx.hs, 600_000, rej), 1_000, seq_base=7, twin=tw)
    assert np.all(g[0][rej] == ADMIT_RATE) and g[9][8] == n - len(rej) and g[9][9] == len(rej)
    # ... and a random 30 % rejected, on the state the first call left
    rej2 = np.nonzero(rng.random(n) < 0.3)[0]
    g = run(cx, Batch(rng, n, cx.hs, 720_000, rej2), 2_000, seq_base=7 + n, twin=tw)
    assert g[9][8] == n - len(rej2)
    if n >= 65:
        assert g[9][2] > 0                                   # the pool is full: overload fallbacks after rejected items
    check_sweep(cx, 2_000, tw)


def test_mixed_verdicts_on_the_default_limits():
    cx, tw = Ctx(), Ctx()
    rng = np.random.default_rng(5)
    g = run(cx, Batch(rng, 300, cx.hs, 600_000, forced=False), 500, twin=tw)
    assert g[9][9] > 0 and g[9][10] > 0 and g[9][11] > 0 and g[9][8] > 0     # all three verdicts, and a trigger
    assert {ADMIT_OK, ADMIT_RATE, ADMIT_CONCURRENT} == set(g[0].tolist())
    check_sweep(cx, 500, tw)


# ------------------------------------------------------------------------------------------- m == 0, m == n
def test_nothing_admitted_changes_nothing_but_the_rate_records():
    cx, tw = Ctx(), Ctx()
    rng = np.random.default_rng(6)
    run(cx, Batch(rng, 40, cx.hs, 600_000), 100, twin=tw)     # some state first: entries, a concurrency map
    key = cx.b.key_id(cx.hs[2])
    before = state_of(cx.b, cx.ns)
    conc = [cx.b.concurrent_state(i, key) for i in range(8)]
    assert any(c is not None for c in conc)
    B = Batch(rng, 130, cx.hs, 660_000, reject=range(0, 130, 2))
    B.kind[1::2] |= TRIG                                      # every other item a trigger (their action is never read)
    B.acts[1::2] = -5
    g = run(cx, B, 200, twin=tw)                              # the twin runs admit_batch alone
    assert g[9][8] == 0 and g[9][0] == 0 and g[9][9] == 65 and g[9][11] == 65
    assert np.all(g[5] == NOT_PUBLISHED)
    after = state_of(cx.b, cx.ns)
    assert after[:4] == before[:4]                            # permits, books, totals, live entries
    assert after[4] != before[4]                              # the rate records are charged
    assert [cx.b.concurrent_state(i, key) for i in range(8)] == conc
    inv, fl = cx.b.publish([cx.hs[0]], seq_base=5)            # the next decision is the one the oracle makes
    assert (int(inv[0]), int(fl[0])) == cx.st.publish(cx.hs[0], 5)
    tinv, tfl = tw.b.publish([cx.hs[0]], seq_base=5)
    assert (int(tinv[0]), int(tfl[0])) == (int(inv[0]), int(fl[0]))
    check_sweep(cx, 200, tw)


def test_everything_admitted_equals_publish_activations():
    cx, tw = Ctx(), Ctx()
    g = run(cx, Batch(np.random.default_rng(7), 200, cx.hs, 600_000), 300, seq_base=11, twin=tw)
    assert g[9][8] == 200 and not g[0].any()
    check_sweep(cx, 300, tw)


# ------------------------------------------------------------------------------------------- sequence numbers
def test_fallbacks_follow_the_rank_among_the_admitted():
    rng = np.random.default_rng(8)
    fill = Batch(rng, 60, [0, 1, 2], 600_000)
    B = Batch(rng, 130, [0, 1, 2], 660_000, reject=[0, 3, 64, 65, 100])
    seq = rng.integers(0, 2**63, 130).astype(np.uint64)
    for explicit in (False, True):
        cx, tw = Ctx(), Ctx()
        run(cx, fill, 100, seq_base=0, twin=tw)               # the pool is full from here on
        g = run(cx, B, 200, seq=seq if explicit else None, seq_base=5_000, twin=tw)
        ovl = np.nonzero(g[6] & 1)[0]
        assert len(ovl) > 0 and ovl.max() > 0                 # a fallback after the rejected item 0 ...
        assert any(i > 3 for i in ovl) and g[0][3] == ADMIT_RATE
        # ... whose invoker depends on the sequence number: seq_base + the array index (for seq = None), or seq indexed
        # by rank instead of by item (for an explicit seq), gives other invokers
        adm = np.nonzero(g[0] == ADMIT_OK)[0]
        swapped = np.zeros(130, np.uint64)
        swapped[adm] = seq[:len(adm)]
        wrong = Ctx(gpu=False)
        wrong.m.invoke(fill.ns, fill.kind, fill.t, fill.acts, fill.aids, fill.tks, fill.lims, 100, fill.ro, fill.co)
        w = wrong.m.invoke(B.ns, B.kind, B.t, B.acts, B.aids, B.tks, B.lims, 200, B.ro, B.co,
                           seq=swapped if explicit else 5_000 + np.arange(130))
        assert np.array_equal(w[0], g[0]) and not np.array_equal(w[5], g[5])
        check_sweep(cx, 200, tw)


# ------------------------------------------------------------------------------------------- duplicate ids
def test_duplicate_ids():
    cx, tw = Ctx(), Ctx()
    B = Batch(np.random.default_rng(9), 6, cx.hs, 600_000, reject=[0])
    X, Y = fresh_ids(2)
    B.aids[0] = B.aids[1] = X                                 # rejected, then admitted: the admitted one creates it
    B.aids[2] = B.aids[4] = Y                                 # two admitted duplicates: as in publish
    g = run(cx, B, 100, twin=tw)
    assert g[0].tolist() == [ADMIT_RATE, 0, 0, 0, 0, 0] and np.all(g[5][1:] >= 0)
    assert (g[7][0], g[8][0]) == (-1, 0) and (g[7][1], g[8][1]) == (B.tks[1], 0)
    assert (g[7][2], g[8][2]) == (B.tks[2], 0) and (g[7][4], g[8][4]) == (B.tks[2], 1)
    assert g[9][0] == 5 and g[9][1] == 4 and cx.b.activations_live() == 4
    check_sweep(cx, 100, tw)


# ------------------------------------------------------------------------------------------- triggers
def test_triggers_get_rate_verdicts_only():
    cx, tw = Ctx(limits=(1000, 5, 1000)), Ctx(limits=(1000, 5, 1000))
    B = Batch(np.random.default_rng(10), 200, cx.hs, 600_000, forced=False)
    B.kind[:] = np.where(np.arange(200) % 2 == 0, TRIG, ACT)  # alternating, all on the defaults
    B.acts[0::2] = 77                                         # no such handle: a trigger's is never read
    g = run(cx, B, 100, twin=tw)
    trig = np.arange(0, 200, 2)
    assert set(g[0][trig].tolist()) == {ADMIT_OK, ADMIT_RATE} and g[9][11] == 25          # 5 fires in each namespace
    assert np.all(g[5][trig] == NOT_PUBLISHED) and np.all(g[3][trig] == -1) and not g[4][trig].any()
    assert not g[0][1::2].any() and g[9][8] == 100
    check_sweep(cx, 100, tw)


# ------------------------------------------------------------------------------------------- no usable invoker
def test_no_usable_invoker_is_reported():
    cx, tw = Ctx(status=[OFFLINE] * 8, limits=(1000, 1000, 2)), Ctx(status=[OFFLINE] * 8, limits=(1000, 1000, 2))
    B = Batch(np.random.default_rng(11), 40, cx.hs, 600_000, forced=False)
    B.kind[:] = ACT
    g = run(cx, B, 100, twin=tw)
    adm = np.nonzero(g[0] == ADMIT_OK)[0]
    assert len(adm) == 10 and np.all(g[5][adm] == NONE)       # 2 per namespace pass the gate, none gets an invoker
    assert g[9][4] == g[9][8] == 10 and g[9][0] == 0 and g[9][10] == 30
    # the gate counted them all the same (its stated assumption): the later items of each namespace see 2 in flight
    assert set(g[3][g[0] == ADMIT_CONCURRENT].tolist()) == {2}
    assert cx.b.activation_totals() == (0, 0, 0) and not cx.b.active_activations_for(cx.ns).any()
    assert cx.b.activations_live() == 0
    assert check_sweep(cx, 100, tw) == ([], 0)


# ------------------------------------------------------------------------------------------- errors change nothing
def test_rejected_calls_change_nothing():
    cx, tw = Ctx(), Ctx()                                     # the twin takes only the two calls that are accepted
    rng = np.random.default_rng(12)
    run(cx, Batch(rng, 30, cx.hs, 600_000), 100, twin=tw)
    before = state_of(cx.b, cx.ns)
    B = Batch(rng, 20, cx.hs, 660_000)

    def call(**over):
        a = dict(ns=B.ns, kind=B.kind, t_ms=B.t, actions=B.acts, aids=B.aids, tickets=B.tks, time_limit_ms=B.lims,
                 now_ms=200, rate_override=B.ro, conc_override=B.co)
        a.update(over)
        return cx.b.invoke_activations(**a)

    def bad(arr, i, v):
        x = np.array(arr).copy()
        x[i] = v
        return x

    for code, over in [(EINVAL, dict(time_limit_ms=bad(B.lims, 7, 2**40))),     # item 0's rate must not be charged
                       (EINVAL, dict(time_limit_ms=bad(B.lims, 7, -1))),
                       (ENOENT, dict(actions=bad(B.acts, 19, 99))),
                       (ENOENT, dict(ns=bad(B.ns, 3, 5))),
                       (EINVAL, dict(ns=bad(B.ns, 3, NONE))),
                       (EINVAL, dict(t_ms=bad(B.t, 9, -1))),
                       (EINVAL, dict(kind=bad(B.kind, 2, 8))),
                       (EINVAL, dict(now_ms=2**60))]:
        with pytest.raises(OwgsError) as e:
            call(**over)
        assert e.value.code == code, over
        assert state_of(cx.b, cx.ns) == before
    # msgs->n != n, through the raw entry point
    n = B.n
    words = np.array([O.aid_words(a) for a in B.aids], dtype=np.uint64).reshape(-1)
    outs = [np.zeros(n, np.uint8) for _ in range(3)] + [np.zeros(n, np.int32) for _ in range(6)]
    lims = np.ascontiguousarray(B.lims, np.int64)
    io = _lib.owgs_invoke_io(n, _p(B.ns), _p(B.kind), _p(B.t), _p(B.ro), _p(B.co), _p(B.acts), None, 0, _p(words),
                             _p(B.tks), _p(lims), 200, _p(outs[0]), _p(outs[3]),
                             _p(outs[4]), _p(outs[5]), _p(outs[6]), _p(outs[7]), _p(outs[1]), _p(outs[8]), _p(outs[2]))
    mb, mo, keep, _ = _msg_io(n, dict(B.M, n_topics=N_TOPICS, cap=1 << 16), "test")
    mb.n = n - 1
    summ = np.zeros(16, np.int64)
    assert _lib.lib().owgs_invoke_activations(cx.b._h, C.byref(io), C.byref(mb), C.byref(mo), _p(summ)) == EINVAL
    assert state_of(cx.b, cx.ns) == before and not summ.any()
    # an unknown handle on an item that is a trigger is not an error
    B.kind[5] |= TRIG
    B.acts[5] = 99
    g = run(cx, B, 200, twin=tw)
    assert g[5][5] == NOT_PUBLISHED and g[9][8] == 19
    check_sweep(cx, 200, tw)


# ------------------------------------------------------------------------------------------- two calls, then acks
def test_second_call_sees_the_releases():
    cx, tw = Ctx(), Ctx()
    rng = np.random.default_rng(13)
    B1 = Batch(rng, 60, cx.hs, 600_000, forced=False)
    B1.kind[:] = RO                                           # actions, rate limit lifted, 2 concurrent per namespace
    g1 = run(cx, B1, 100, twin=tw)
    placed = np.nonzero(g1[5] >= 0)[0]
    assert len(placed) == 10 and g1[9][10] == 50
    half = placed[::2]
    acks = [W.completion_message(B1.aids[i], int(g1[5][i])) for i in half]
    for side in (cx.b, tw.b):
        side.process_acks(acks)
    cx.m.pm.t.process_acks(acks)
    check_state(cx, tw)
    B2 = Batch(rng, 60, cx.hs, 660_000, forced=False)
    B2.kind[:] = RO
    g2 = run(cx, B2, 200, seq_base=60, twin=tw)
    freed = np.bincount(B1.ns[half], minlength=5)
    for h in range(5):                                        # the first action of a namespace sees what is in flight
        i = int(np.nonzero(B2.ns == h)[0][0])
        assert g2[3][i] == 2 - freed[h]
    assert g2[9][8] == len(half)                              # exactly the released slots are admitted again
    check_sweep(cx, 200, tw)


# ------------------------------------------------------------------------------------------- watched pairs
def test_watched_pairs_after_a_cluster_change():
    """After updateCluster with concurrent activations in flight the engine's decisions update the watched pairs over
    all n items of the call: the entries past the admitted count are padding that update must ignore."""
    cx, tw = Ctx(), Ctx()
    rng = np.random.default_rng(16)
    B1 = Batch(rng, 30, [cx.hs[2]], 600_000)                  # concurrent activations only
    g1 = run(cx, B1, 100, twin=tw)
    assert np.all(g1[5] >= 0)
    for c in (cx, tw):
        c.b.update_cluster(2)
        c.st.update_cluster(2)
        c.m.cluster = 2                                       # the limits are divided by the cluster size
    n = 200
    g2 = run(cx, Batch(rng, n, cx.hs, 660_000, np.nonzero(rng.random(n) < 0.4)[0]), 200, seq_base=30, twin=tw)
    assert 0 < g2[9][8] < n
    acks = [W.completion_message(B1.aids[i], int(g1[5][i])) for i in range(0, 30, 2)]
    want = cx.m.pm.t.process_acks(acks)
    for side in (cx.b, tw.b):
        got = side.process_acks(acks)
        assert all(np.array_equal(got[k], want[k]) for k in (0, 2, 3))
    run(cx, Batch(rng, n, cx.hs, 720_000, boundary_positions(n)), 300, seq_base=30 + n, twin=tw)
    check_sweep(cx, 300, tw)


# ------------------------------------------------------------------------------------------- large-state context
def test_large_state_context_reads_the_verdicts_back_once():
    acts = (SMALL, BIG, WIDE)
    cx, tw = Ctx(actions=acts), Ctx(actions=acts)
    assert cx.b.large_stats() is not None                     # maxConcurrent 4,096: the large-state engine
    rng = np.random.default_rng(14)
    n = 257
    g = run(cx, Batch(rng, n, cx.hs, 600_000, boundary_positions(n)), 100, twin=tw, waits=2)
    assert g[9][8] == n - len(boundary_positions(n))
    g = run(cx, Batch(rng, n, cx.hs, 660_000, np.nonzero(rng.random(n) < 0.3)[0]), 200, seq_base=n, twin=tw, waits=2)
    assert g[9][2] > 0
    B = Batch(rng, 10, cx.hs, 720_000, reject=range(10))      # nothing admitted: the engine is not run at all
    g = run(cx, B, 300, twin=tw, waits=2)
    assert g[9][8] == 0
    check_sweep(cx, 300, tw)


def test_on_chip_context_waits_once():
    """No host wait between the gate and the engine: the admitted count never comes to the host before the outputs."""
    cx, tw = Ctx(), Ctx()
    assert cx.b.large_stats() is None
    rng = np.random.default_rng(15)
    for n, seq in ((4, None), (513, rng.integers(0, 2**62, 513).astype(np.uint64))):
        g = run(cx, Batch(rng, n, cx.hs, 600_000, [0]), 100, seq=seq, twin=tw)
        assert g[9][12] == 1
    check_sweep(cx, 100, tw)
