"""owgs_process_result_acks on the GPU (the RESULTS instantiation of the ack parser, the result-only lookups of the
table kernels, the one-block outputs) against the host model (tests/result_acks_model.py), whose completion half is the
frozen ack oracle's: every output array, and after each call the permits, activationSlots, the in-flight books, the
deadlines and the health vector."""
import ctypes as C

import numpy as np
import pytest

import large_state_cases as LC
import oracle as O
from feeds_model import ack_events
from openwhisk_amd import OwgsError, _lib
from openwhisk_amd import workload as W
from openwhisk_amd._lib import ACK_HEALTH, ACK_JVM, ACK_NOENTRY, ACK_RELEASED, ACK_RESULT, ACKF_RESULT, ACKF_RIGHT
from result_ack_cases import (activation_members, canonical, combined_message, fuzz_messages, print_object,
                              result_message)
from result_acks_model import ResultAckModel
from test_gpu_feeds import MB, Loop, register_all, same_health
from test_result_acks_cpu import FUZZ_SEED, vectors

pytestmark = pytest.mark.gpu
H = 1700000000123
NAMES = ("kind", "invoker", "ticket", "flags", "aid", "resp_off", "resp_len")


class RLoop(Loop):
    """test_gpu_feeds.Loop with the new call beside the model: the flow's table is read through ResultAckModel."""

    def __init__(self, w, zombies=False):
        super().__init__(w, zombies=zombies)
        self.md = ResultAckModel(self.flow)

    def track(self, aids, acts):
        tickets = np.arange(self.next_ticket, self.next_ticket + len(aids))
        self.next_ticket += len(aids)
        gt, gx = self.b.track_activations(aids, acts, tickets)
        for j, aid in enumerate(aids):
            t, x = self.md.track(aid, int(acts[j]), int(tickets[j]))
            assert (gt[j], gx[j]) == (t, x)
            self._count(acts[j], 1)
            if not x:
                self.entry[int(tickets[j])] = int(acts[j])
        return tickets

    def result_acks(self, msgs, now=None, apply=0):
        exp = list(self.md.process(msgs))
        off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])])[:-1]
        exp[5] = np.where(exp[3] & ACKF_RESULT, exp[5] + off, 0)
        before = self.hp.read()
        got = self.b.process_result_acks(msgs, now, apply)
        summ = got[7]
        bad = np.flatnonzero(exp[0] != got[0])
        assert len(bad) == 0, [(msgs[i][:300], int(got[0][i]), int(exp[0][i])) for i in bad[:3]]
        acc = exp[0] >= ACK_RELEASED
        assert np.array_equal(exp[1][acc], got[1][acc]), "invoker"
        for k in range(2, 7):
            d = np.flatnonzero(np.asarray(exp[k] != got[k]).reshape(len(msgs), -1).any(axis=1))
            assert len(d) == 0, (NAMES[k], [(msgs[i][:300], got[k][i], exp[k][i]) for i in d[:3]])
        for t in exp[2][exp[0] == ACK_RELEASED]:
            self._count(self.entry.pop(int(t)), -1)
        if now is None:
            assert summ is None
            same_health(self.b.health_read(), before)
            fed = None
        else:
            ev_inv, ev_kind = ack_events(exp[0], exp[1], exp[3])
            fed = self._feed(ev_inv, ev_kind, now, apply, summ, before)
        self.same_books()
        return got, fed


def _small():
    return W.config("c4", n_activations=6_000, n_invokers=40)


@pytest.fixture(scope="module")
def small():
    return _small()


def started(w, n_track, seed=3, zombies=False):
    """A loop with every invoker Healthy and the first n_track publishes of the stream tracked: (loop, ids, invokers)."""
    lp = RLoop(w, zombies=zombies)
    register_all(lp, len(w.inv_ids), w.inv_mem // MB)
    if n_track == 0:
        return lp, [], np.zeros(0, np.int32)
    acts = w.stream.act[:n_track]
    inv = lp.publish(acts)
    ok = np.flatnonzero(inv >= 0)
    aids = W.activation_ids(np.random.default_rng(seed), len(ok))
    lp.track(aids, acts[ok])
    return lp, aids, inv[ok]


# ----------------------------------------------------------------------------------------------- 1. golden vectors
def test_golden_vectors(small):
    vs = vectors()
    lp, aids, inv = started(small, 8)
    msgs = [v["msg"].encode("utf-8") for v in vs]
    (gk, gi, gt, gf, ga, go, gl, _), _ = lp.result_acks(msgs)
    for i, v in enumerate(vs):
        if v["kind"] == 3:  # an accepted Combined message: a completion, whatever the table says
            assert gk[i] in (ACK_RELEASED, ACK_HEALTH, ACK_NOENTRY), v["name"]
        else:
            assert int(gk[i]) == v["kind"], v["name"]
        if v["kind"] in (3, 7):
            assert "%016x%016x" % (int(ga[i][0]), int(ga[i][1])) == v["aid"], v["name"]
            assert bool(gf[i] & ACKF_RIGHT) == bool(v["right"]) and gf[i] & ACKF_RESULT, v["name"]
        else:
            assert (int(ga[i][0]), int(ga[i][1]), int(go[i]), int(gl[i]), int(gf[i])) == (0, 0, 0, 0, 0), v["name"]


# ------------------------------------------------------------------------------------------------------- 2. fuzz
def test_fuzz_in_batches(small):
    lp, aids, inv = started(small, 700)
    msgs = fuzz_messages(FUZZ_SEED, 2000, aids, inv)
    seen, now, at = set(), 10, 0
    sizes = [1, 63, 64, 65, 255, 256, 257, 1025]
    assert sum(sizes) <= len(msgs)
    for k, n in enumerate(sizes + [len(msgs) - sum(sizes)]):
        (gk, *_), _ = lp.result_acks(msgs[at:at + n], now if k % 2 else None, apply=2 if k % 2 else 0)
        seen |= set(gk.tolist())
        at += n
        now += 5
    assert {0, ACK_JVM, 2, ACK_RELEASED, ACK_NOENTRY, ACK_RESULT} <= seen


# ------------------------------------------------------------------------------------------ 3. placement and size
def test_placement_and_size(small):
    lp, aids, inv = started(small, 80)
    assert len(aids) >= 45
    rng = np.random.default_rng(5)
    msgs = []
    for pad in range(17):  # the response value starts (and, with the id's fixed length, ends) at every window offset
        msgs.append(b" " * pad + result_message('"%s"' % aids[pad]))
        body = print_object(activation_members(rng, aids[17 + pad], 40 + pad))
        msgs.append(b" " * pad + combined_message(body, int(inv[17 + pad])))
    big = activation_members(rng, aids[40], 9_000)
    msgs.append(combined_message(print_object(big), int(inv[40])))
    m200 = [(k, "[%s]" % ",".join('{"key":"k%d","value":%d}' % (q, q) for q in range(200)) if k == "annotations" else v)
            for k, v in activation_members(rng, aids[41], 50)]
    msgs.append(combined_message(print_object(m200), int(inv[41])))
    for j, depth in enumerate((63, 64, 65)):  # message, activation and response are containers 1-3
        k = depth - 3
        mm = [(a, '{"statusCode":0,"result":%s}' % ("[" * k + "]" * k) if a == "response" else v)
              for a, v in activation_members(rng, aids[42 + j], 30)]
        msgs.append(combined_message(print_object(mm), int(inv[42 + j])))
    (gk, _, _, gf, _, go, gl, _), _ = lp.result_acks(msgs, 50, apply=2)
    assert gk[-3:].tolist() == [ACK_RELEASED, ACK_RELEASED, 2] and gk[-5] == gk[-4] == ACK_RELEASED
    assert gl[-5] > 9_000 and (gk[:34:2] == ACK_RESULT).all() and (gk[1:34:2] == ACK_RELEASED).all()
    blob = b"".join(msgs)
    assert blob[go[0]:go[0] + gl[0]] == b'"%s"' % aids[0].encode()
    assert blob[go[-5]:go[-5] + gl[-5]].decode() == print_object(big)


# ------------------------------------------------------------------------------------------ 4. order in one batch
def test_order_inside_one_batch(small):
    lp, aids, inv = started(small, 12)
    tk = {a: t for (t, a) in zip(sorted(lp.entry), aids)}
    rng = np.random.default_rng(6)
    R = lambda j: canonical(rng, aids[j], 0, "result", 40)                  # noqa: E731
    Cb = lambda j: canonical(rng, aids[j], int(inv[j]), "combined", 40)     # noqa: E731
    Cp = lambda j: canonical(rng, aids[j], int(inv[j]), "completion")       # noqa: E731
    msgs = [R(0), Cp(0), R(0),        # Result before and after its Completion
            Cb(1), R(1),              # Result after a Combined of the same id
            Cb(2), Cb(2),             # two Combined of one id
            R(3), R(3)]               # a duplicate Result
    (gk, _, gt, *_), _ = lp.result_acks(msgs, 20, apply=2)
    assert gk.tolist() == [7, 3, 7, 3, 7, 3, 5, 7, 7]
    assert gt.tolist() == [tk[aids[0]], tk[aids[0]], -1, tk[aids[1]], -1, tk[aids[2]], -1, tk[aids[3]], tk[aids[3]]]
    assert lp.b.activations_live() == len(aids) - 3


# ------------------------------------------------------------------------------- 5. against today's two calls
def test_first_batch_equals_the_two_call_path():
    w = W.config("c4", n_activations=6_000, n_invokers=40)
    a1 = int(w.stream.acq_off[1])
    lp, aids, inv = started(w, a1)
    twin, aids2, inv2 = started(w, a1)
    assert aids == aids2 and np.array_equal(inv, inv2)
    rng = np.random.default_rng(11)
    msgs, comb = [], []  # comb: (message index, id index) of the Combined messages
    for j in rng.permutation(len(aids)):
        i = int(inv[j])
        if j % 3 == 0:
            msgs.append(W.completion_message(aids[j], i))
        elif j % 3 == 1:
            comb.append((len(msgs), int(j)))
            msgs.append(canonical(rng, aids[j], i, "combined", 120))
        else:
            msgs += [canonical(rng, aids[j], i, "result", 120), W.completion_message(aids[j], i)]
    (gk, gi, gt, gf, ga, _, _, _), fed = lp.result_acks(msgs, 100, apply=2)
    assert (gk == ACK_RELEASED).sum() == len(aids)
    assert (gk == ACK_RESULT).sum() == sum(1 for j in range(len(aids)) if j % 3 == 2)
    # the twin: the old parser, then the JVM's parse of the kind-1 messages and the second call
    tk, ti, tt, tf, s1 = twin.b.process_acks_supervised(msgs, 100, apply=2)
    assert (tk == ACK_JVM).sum() == len(comb) + (gk == ACK_RESULT).sum()
    ids = [aids[j] for _, j in comb]
    ck, ct, cf, s2 = twin.b.complete_activations_supervised(ids, [int(inv[j]) for _, j in comb], 100, apply=2)
    comb = [q for q, _ in comb]
    assert (ck == ACK_RELEASED).all() and s1[0] + s2[0] == fed[0]
    assert np.array_equal(ct, gt[comb])
    same = tk != ACK_JVM
    assert np.array_equal(tk[same], gk[same]) and np.array_equal(tt[same], gt[same])
    assert np.array_equal(lp.b.permits(), twin.b.permits())
    assert lp.b.activations_live() == twin.b.activations_live() == 0
    assert tuple(lp.b.activation_totals()) == tuple(twin.b.activation_totals())
    # the feed order differs in one respect: the twin's events of the Combined messages come after all the others
    # (its second call).  Every event here is a Success at one time, so the vectors the two orders leave are equal.
    same_health(lp.b.health_read(), twin.b.health_read())


# --------------------------------------------------------------------------------------------------- 6. timed entry
def test_timed_entry_and_the_sweep(small):
    lp, _, _ = started(small, 0)
    b = lp.b
    acts = small.stream.act[:2]
    inv = lp.publish(acts)
    assert (inv >= 0).all()
    x, y = W.activation_ids(np.random.default_rng(8), 2)
    t, e = b.track_activations_timed([x, y], acts, [70, 71], inv, [1_000, 1_000], 1_000)
    assert t.tolist() == [70, 71] and e.tolist() == [0, 0]
    for j, a in enumerate((x, y)):
        lp.md.track(a, int(acts[j]), 70 + j)
        lp._count(acts[j], 1)
        lp.entry[70 + j] = int(acts[j])
    dl = 1_000 + 60_000 * 2 + 60_000
    assert b.next_deadline() == dl
    rng = np.random.default_rng(9)
    # y's Combined before the sweep leaves only x to expire
    (gk, _, gt, *_), _ = lp.result_acks([canonical(rng, y, int(inv[1]), "combined", 40)], 2_000, apply=2)
    assert (gk[0], gt[0]) == (ACK_RELEASED, 71)
    aids, tk, ei, d, fl, rem = b.expire_activations(dl, None, False)
    assert list(aids) == [x] and tk.tolist() == [70] and rem == 0
    o, ot, oa, rf = lp.flow.complete(*O.aid_words(x), int(ei[0]), True, False)
    assert o == ACK_RELEASED
    lp.md.forget(x)
    lp._count(lp.entry.pop(70), -1)
    lp.same_books()
    assert b.next_deadline() == _lib.NO_DEADLINE
    # x's Combined after the sweep: NOENTRY, ticket -1, the id reported
    (gk, _, gt, gf, ga, _, gl, _), _ = lp.result_acks([canonical(rng, x, int(inv[0]), "combined", 40)], dl + 1, apply=2)
    assert (gk[0], gt[0]) == (ACK_NOENTRY, -1) and gf[0] & ACKF_RESULT and gl[0] > 0
    assert "%016x%016x" % (int(ga[0][0]), int(ga[0][1])) == x
    assert b.expiry_stats()[3] == 1


# --------------------------------------------------------------------------------------------------- 7. large state
def test_large_state_context():
    w = LC.workload("p17")
    lp, aids, inv = started(w, 200, zombies=True)
    assert lp.b.large_stats() is not None
    msgs = fuzz_messages(17, 300, aids, inv)
    (gk, *_), _ = lp.result_acks(msgs, 30, apply=2)
    assert {ACK_RELEASED, ACK_RESULT, ACK_JVM} <= set(gk.tolist())
    lp.publish(w.stream.act[200:400])
    lp.same_books()


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_argument_errors_change_nothing(small):
    lp, aids, inv = started(small, 30)
    register = lp.b
    rng = np.random.default_rng(4)
    msgs = [canonical(rng, aids[j], int(inv[j]), "combined", 40, system_error=True) for j in range(len(aids))]
    health, permits, live, totals = register.health_read(), register.permits(), register.activations_live(), \
        tuple(register.activation_totals())

    def unchanged():
        same_health(register.health_read(), health)
        assert np.array_equal(register.permits(), permits) and register.activations_live() == live
        assert tuple(register.activation_totals()) == totals

    clock = 1  # register_all fed the FSM at times 0 and 1
    for now, apply in ((clock - 1, 1), (-1, 0), (1 << 60, 0), (clock + 5, 3)):
        with pytest.raises(OwgsError) as e:
            register.process_result_acks(msgs, now, apply)
        assert e.value.code == _lib.EINVAL
        unchanged()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = len(msgs)
    buf = np.frombuffer(b"".join(msgs) + b"\0", np.uint8)
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.int64)
    arrs = [np.zeros(4 * n, np.int64) for _ in range(7)]
    L, h = register._L, register._h
    s = np.zeros(3, np.int32)
    assert L.owgs_process_result_acks(h, n, P(buf), P(off), None, 0, 0, None) == _lib.EINVAL
    for miss in range(7):
        out = _lib.owgs_ack_out(*[None if q == miss else P(a) for q, a in enumerate(arrs)])
        assert L.owgs_process_result_acks(h, n, P(buf), P(off), C.byref(out), clock + 5, 0, P(s)) == _lib.EINVAL
    out = _lib.owgs_ack_out(*[P(a) for a in arrs])
    assert L.owgs_process_result_acks(h, n, P(buf), P(off), C.byref(out), clock + 5, 0, None) == _lib.EINVAL  # now
    assert L.owgs_process_result_acks(h, n, P(buf), P(off), C.byref(out), 0, 1, None) == _lib.EINVAL          # apply
    unchanged()
    (gk, *_), fed = lp.result_acks(msgs, clock, apply=2)  # and the batch still goes through at the clock's own time
    assert (gk == ACK_RELEASED).all() and fed[0] == n


# -------------------------------------------------------------------------------- 9. no response member anywhere
def test_plain_batch_equals_process_acks_supervised(small):
    lp, aids, inv = started(small, 300)
    twin, _, _ = started(small, 300)
    rng = np.random.default_rng(12)
    msgs = W.ack_batch(rng, aids, inv, H, combined=0.0)
    assert not any(b'"response"' in m for m in msgs)
    (gk, gi, gt, gf, ga, go, gl, gs), _ = lp.result_acks(msgs, 40, apply=2)
    tk, ti, tt, tf, ts = twin.b.process_acks_supervised(msgs, 40, apply=2)
    assert np.array_equal(gk, tk) and np.array_equal(gi, ti) and np.array_equal(gt, tt) and np.array_equal(gf, tf)
    assert gs == ts and not go.any() and not gl.any()
    same_health(lp.b.health_read(), twin.b.health_read())
    assert np.array_equal(lp.b.permits(), twin.b.permits())
