"""The completion-ack timeout model (tests/timeout_model.py) against numbers written out by hand from
CommonLoadBalancer.scala:103-105 with the reference's defaults (TimeLimit.STD_DURATION 1 minute, timeout-factor 2,
timeout-addon 1 minute), and against the reference's rules for arming, cancelling and firing (CLB:148-152, 289,
329-337)."""
import types

import numpy as np

import oracle as O
from openwhisk_amd import workload as W
from timeout_model import NO_DEADLINE, TimeoutModel

ACT = types.SimpleNamespace(mem_mb=256, blackbox=False)


def _model():
    st = O.BalancerState(managed_fraction=1.0, blackbox_fraction=0.0)
    st.update_invokers(np.arange(3), np.full(3, 1024 * 2**20), np.zeros(3, np.uint8))
    a = st.register_action("ns", "ns/a", 0, 256)
    return TimeoutModel(O.AckFlow(st, health_start_ms=77, cap=1 << 8), {a: ACT}), st, a


def aid(k):
    return "%032x" % (0xE0 << 96 | k)


def test_deadlines_by_hand():
    m, _, _ = _model()
    assert m.deadline(100, 1_000) == 181_000          # max(100, 60000) * 2 + 60000 = 180000, armed at 1000
    assert m.deadline(60_000, 1_000) == 181_000       # the standard limit itself
    assert m.deadline(300_000, 1_000) == 661_000      # 300000 * 2 + 60000 = 660000
    m.set_ack_timeout(60_000, 3, 0)
    assert m.deadline(300_000, 0) == 900_000


def test_a_duplicate_arms_nothing():
    m, st, a = _model()
    inv, _ = st.publish(a, 0)
    assert m.track(aid(1), a, 5, inv, 300_000, 1_000) == (5, 0)
    assert m.track(aid(1), a, 6, inv, 100, 1_000) == (5, 1)   # shorter limit, later message: no new timer
    assert m.armed[aid(1)][0] == 661_000 and m.next_deadline() == 661_000
    assert m.books([]) == ([], (2, 512, 0))                    # the duplicate is counted all the same (CLB:121-127)
    assert m.expire(660_999) == ([], 0)
    out, rem = m.expire(661_000)
    assert out == [(aid(1), 5, inv, 661_000, 0)] and rem == 0
    assert m.books([]) == ([], (1, 256, 0)) and m.live() == 0 and m.next_deadline() == NO_DEADLINE


def test_regular_ack_then_sweep_gives_nothing():
    m, st, a = _model()
    inv, _ = st.publish(a, 0)
    m.track(aid(2), a, 7, inv, 100, 0)
    k, _, t, _ = m.process_acks([W.completion_message(aid(2), inv)])
    assert (k[0], t[0]) == (O.OUT_RELEASED, 7)
    assert m.expire(2**59) == ([], 0) and m.live() == 0


def test_sweep_then_regular_ack_is_noentry():
    m, st, a = _model()
    inv, _ = st.publish(a, 0)
    before = st.permits().copy()
    m.track(aid(3), a, 8, inv, 100, 0)
    out, _ = m.expire(180_000)
    assert out == [(aid(3), 8, inv, 180_000, 0)]
    assert st.permits()[inv] == before[inv] + 256              # releaseInvoker ran with the entry's invoker
    k, _, t, _ = m.process_acks([W.completion_message(aid(3), inv)])
    assert (k[0], t[0]) == (O.OUT_NOENTRY, -1)
    assert m.complete(aid(3), inv, forced=True)[0] == O.OUT_FORCED_NOENTRY


def test_order_and_cap():
    m, st, a = _model()
    # deadlines 180000, 180000, 180001, 180000 (armed at 0, 0, 1, 0): ties fire in arm order
    for k, now in enumerate([0, 0, 1, 0]):
        m.track(aid(10 + k), a, k, 0, 100, now)
    m.track(aid(20), a, 9)                                     # untimed: never expires
    out, rem = m.expire(180_001, cap=3)
    assert [o[1] for o in out] == [0, 1, 3] and rem == 1
    out, rem = m.expire(180_001, cap=0)
    assert out == [] and rem == 1
    out, rem = m.expire(2**59)
    assert [o[1] for o in out] == [2] and rem == 0 and m.live() == 1
