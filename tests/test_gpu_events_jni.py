"""The throttle-gate event natives of the JNI binding (integration/owgs_jni.c: setEventSource, registerEventIdentities,
invokeActivationsEvents) executed through the JNIEnv stand-in of tests/jni_stub (tests/jni_events/events_harness.c adds
their ctypes wrappers), the way tests/test_gpu_invoke_jni.py drives invokeActivations.  The CPU test checks the binding's
argument handling; the GPU test compares one mixed batch with the ctypes path on a twin context."""
import ctypes as C
import os

import numpy as np
import pytest

import events_cases as EC
from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd import workload as W
from openwhisk_amd.balancer import Action, _blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "integration", "build", "libowgs_jni_events_harness.so")
K_INTS, K_LONGS, K_BYTES, K_STRING, K_DIRECT = 1, 2, 3, 4, 5
MB = 1 << 20
TRIG, RO, CO = 1, 2, 4
ACTIONS = [Action("ns", "ns/small", "0.0.1", 128), Action("ns", "ns/big", "0.0.1", 256),
           Action("ns", "ns/conc", "0.0.1", 128, 3)]


class Jvm:
    def __init__(self):
        _lib.lib()  # the engine first: the harness links against the same libowgs.so
        assert os.path.exists(HARNESS), "integration/build/libowgs_jni_events_harness.so not built (make -C integration)"
        L = C.CDLL(HARNESS)
        P, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, res, args in [("h_obj", P, [C.c_int, P, i64]), ("h_free", None, [P]), ("h_oob", C.c_long, []),
                                ("h_create", i64, [C.c_double, C.c_double, i64, i32, i32, i64]),
                                ("h_destroy", None, [i64]), ("h_update_invokers", i32, [i64, P, P, P]),
                                ("h_register_action", i32, [i64, P, P, P, i32, i32, i32]),
                                ("h_set_event_source", i32, [i64, P]),
                                ("h_register_event_identities", i32, [i64, P, P, P, P, i32]),
                                ("h_invoke_activations_events", i32, [i64, P, P, P, P, i32, i64, i64, i64, i64]),
                                ("h_last_error", C.c_char_p, [i64])]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        self.L, self.keep, self.objs = L, [], []

    def obj(self, kind, arr):
        self.keep.append(arr)
        o = self.L.h_obj(kind, arr.ctypes.data_as(C.c_void_p), arr.nbytes if kind in (K_DIRECT, K_STRING) else len(arr))
        self.objs.append(o)
        return o

    def string(self, s):
        return self.obj(K_STRING, np.frombuffer(s.encode("ascii") + b"\0", np.uint8)[:len(s)].copy())

    def close(self):
        for o in self.objs:
            self.L.h_free(o)
        self.objs.clear()


@pytest.fixture
def jvm():
    j = Jvm()
    yield j
    j.close()


def buffers(n, aids, lims, t_ms, acts, ns, tks, ro, co, kind, ident, ev_cap, rej_cap):
    """InvokeBuffers' layout (tests/test_gpu_invoke_jni.py) plus EventBuffers': ev_in = ident[n] (int32); ev_out = four
    int64 words, ev_off[n + 1], rej_off[n + 1], ev_cap + rej_cap bytes."""
    w = np.zeros(2 * n, np.uint64)
    w[0::2] = [int(a[:16], 16) for a in aids]
    w[1::2] = [int(a[16:], 16) for a in aids]
    parts = [w, np.asarray(lims, np.int64), np.asarray(t_ms, np.int64)]
    parts += [np.asarray(x, np.int32) for x in (acts, ns, tks, ro, co)] + [np.asarray(kind, np.uint8)]
    inb = np.concatenate([p.view(np.uint8) for p in parts]).copy()
    assert inb.nbytes == 53 * n
    ev_in = np.asarray(ident, np.int32).view(np.uint8).copy()
    ev_out = np.full(32 + 16 * (n + 1) + ev_cap + rej_cap, 0xEE, np.uint8)
    return inb, np.full(128 + 27 * n, 0xEE, np.uint8), ev_in, ev_out


def test_event_natives_reject_bad_shapes_without_a_device(jvm):
    L = jvm.L
    n = 4
    z = [0] * n
    inb, outb, evi, evo = buffers(n, ["%032x" % k for k in range(n)], z, z, z, z, z, z, z, z, z, 64, 32)
    din, dout, dei, deo = (jvm.obj(K_DIRECT, x) for x in (inb, outb, evi, evo))
    f = L.h_invoke_activations_events
    for bad in ((None, dout, dei, deo), (din, None, dei, deo), (din, dout, None, deo), (din, dout, dei, None)):
        assert f(0, *bad, n, 64, 32, 0, 0) == _lib.EINVAL
    assert f(0, din, dout, dei, deo, -1, 64, 32, 0, 0) == _lib.EINVAL
    assert f(0, din, dout, dei, deo, n, -1, 32, 0, 0) == _lib.EINVAL
    assert f(0, din, dout, dei, deo, n, 64, -1, 0, 0) == _lib.EINVAL
    assert f(0, din, dout, dei, deo, n + 1, 64, 32, 0, 0) == _lib.EINVAL             # beyond the buffers
    assert f(0, din, dout, dei, deo, n, 65, 32, 0, 0) == _lib.EINVAL                 # caps beyond ev_out
    assert f(0, din, dout, dei, deo, n, 2**63 - 1, 2**63 - 1, 0, 0) == _lib.EINVAL   # ... in 64-bit arithmetic
    assert f(0, din, dout, jvm.obj(K_DIRECT, evi[:-1]), deo, n, 64, 32, 0, 0) == _lib.EINVAL
    assert f(0, din, dout, jvm.obj(K_BYTES, evi.view(np.int8)), deo, n, 64, 32, 0, 0) == _lib.EINVAL  # not direct
    assert f(0, din, dout, dei, deo, n, 64, 32, 0, 0) == _lib.EINVAL                 # null context: the engine's
    assert L.h_set_event_source(0, None) == _lib.EINVAL
    src = jvm.obj(K_BYTES, np.frombuffer(b'"c"', np.int8).copy())
    assert L.h_set_event_source(0, src) == _lib.EINVAL                               # null context
    off = jvm.obj(K_LONGS, np.array([0, 1], np.int64))
    short = jvm.obj(K_LONGS, np.array([0], np.int64))
    far = jvm.obj(K_LONGS, np.array([0, 9], np.int64))
    by = jvm.obj(K_BYTES, np.frombuffer(b"ab", np.int8).copy())
    g = L.h_register_event_identities
    assert g(0, None, off, by, off, 1) == _lib.EINVAL
    assert g(0, by, short, by, off, 1) == _lib.EINVAL                                # offsets shorter than n + 1
    assert g(0, by, far, by, off, 1) == _lib.EINVAL                                  # offsets beyond the bytes
    assert g(0, by, off, by, off, -2) == _lib.EINVAL
    assert g(0, by, off, by, off, 1) == _lib.EINVAL                                  # null context
    assert np.all(outb == 0xEE) and np.all(evo == 0xEE) and L.h_oob() == 0


@pytest.mark.gpu
def test_event_natives_match_the_ctypes_path(jvm):
    L = jvm.L
    h = L.h_create(0.75, 0.25, 128 * MB, 1, 0, 7)
    assert h != 0
    ref = GpuShardingContainerPoolBalancer(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=7)
    try:
        ids, mem, st8 = np.arange(8, dtype=np.int32), np.full(8, 512 * MB, np.int64), np.zeros(8, np.int8)
        assert L.h_update_invokers(h, jvm.obj(K_INTS, ids), jvm.obj(K_LONGS, mem), jvm.obj(K_BYTES, st8)) == 0
        ref.update_invokers_arrays(ids, mem, st8.view(np.uint8))
        hs, _ = ref.register_actions(ACTIONS)
        for k, a in enumerate(ACTIONS):
            assert L.h_register_action(h, jvm.string(a.namespace), jvm.string(a.path), jvm.string(a.key), a.mem_mb,
                                       a.max_concurrent, int(a.blackbox)) == hs[k]
        hctx = C.c_void_p(h)
        uu = np.array([0, 77, 0, 78], np.uint64)
        o2 = np.zeros(2, np.int32)
        assert _lib.lib().owgs_register_namespaces(hctx, 2, uu.ctypes.data_as(C.c_void_p),
                                                   o2.ctypes.data_as(C.c_void_p)) == 0
        rns = ref.register_namespaces([77, 78])
        assert o2.tolist() == rns.tolist()
        assert _lib.lib().owgs_set_throttle_limits(hctx, 20, 3, 6) == 0
        ref.set_throttle_limits(20, 3, 6)
        # the event state through the natives
        pieces = EC.identities()
        assert L.h_set_event_source(h, jvm.obj(K_BYTES, np.frombuffer(EC.SOURCE.encode(), np.int8).copy())) == 0
        ab, ao = _blob([a for a, _ in pieces])
        bb, bo = _blob([b for _, b in pieces])
        assert L.h_register_event_identities(h, jvm.obj(K_BYTES, ab.view(np.int8)), jvm.obj(K_LONGS, ao),
                                             jvm.obj(K_BYTES, bb.view(np.int8)), jvm.obj(K_LONGS, bo),
                                             len(pieces)) == 0
        ref.set_event_source(EC.SOURCE)
        assert ref.register_event_identities([a for a, _ in pieces], [b for _, b in pieces]) == 0
        n = 130
        rng = np.random.default_rng(4)
        acts = hs[np.arange(n) % 3].astype(np.int32)
        aids = W.activation_ids(rng, n)
        lims = np.array([100, 300_000])[rng.integers(0, 2, n)]
        ns = rns[np.arange(n) % 2].astype(np.int32)
        tks = np.arange(n) + 500
        t_ms = 600_000 + np.arange(n)
        # every seventh item a trigger; every fifth item carries overrides that let it through
        kind = np.where(np.arange(n) % 7 == 3, TRIG, 0) | np.where(np.arange(n) % 5 == 0, RO | CO, 0)
        ro, co = np.full(n, 1000, np.int32), np.full(n, 1000, np.int32)
        ident = rng.integers(0, len(pieces), n).astype(np.int32)
        r = ref.invoke_activations(ns, kind.astype(np.uint8), t_ms, acts, aids, tks, lims, 42, rate_override=ro,
                                   conc_override=co, seq_base=1000, events={"ident": ident})
        ev, tx = r[-1]
        ev_cap, rej_cap = sum(map(len, ev)) + 3, sum(map(len, tx))
        inb, outb, evi, evo = buffers(n, aids, lims, t_ms, acts, ns, tks, ro, co, kind, ident, ev_cap, rej_cap)
        rc = L.h_invoke_activations_events(h, jvm.obj(K_DIRECT, inb), jvm.obj(K_DIRECT, outb), jvm.obj(K_DIRECT, evi),
                                           jvm.obj(K_DIRECT, evo), n, ev_cap, rej_cap, 1000, 42)
        assert rc == 0, L.h_last_error(h)
        assert outb[:128].view(np.int64).tolist() == r[9].tolist()
        ints = outb[128:128 + 24 * n].view(np.int32).reshape(6, n)
        for k, j in enumerate((1, 2, 3, 4, 5, 7)):           # rate count / limit, conc count / limit, invoker, ticket
            assert np.array_equal(ints[k], r[j]), j
        byts = outb[128 + 24 * n:].reshape(3, n)
        for k, j in enumerate((0, 6, 8)):                    # verdict, flags, existed
            assert np.array_equal(byts[k], r[j]), j
        head = evo[:32].view(np.int64).tolist()
        assert head == [ev_cap - 3, rej_cap, sum(1 for x in ev if x), sum(1 for x in tx if x)]
        offs = evo[32:32 + 16 * (n + 1)].view(np.int64).reshape(2, n + 1)
        base = 32 + 16 * (n + 1)
        evb, txb = evo[base:base + ev_cap].tobytes(), evo[base + ev_cap:].tobytes()
        assert [evb[offs[0][i]:offs[0][i + 1]] for i in range(n)] == ev
        assert [txb[offs[1][i]:offs[1][i + 1]] for i in range(n)] == tx
        assert np.all(evo[base + ev_cap - 3:base + ev_cap] == 0xEE)                    # the slack is untouched
        # the batch is what it was meant to be: all four rows, and the summary's event words
        assert all(s > 0 for s in EC.row_share(kind, r[0]))
        s = r[9]
        assert s[13] == head[2] == s[8] + s[9] + s[10] and s[14] == head[3] == s[9] + s[10] and s[15] == 1
        assert s[12] == 1
        # a region that does not fit: OWGS_ERANGE, the totals set, everything else done
        inb, outb, evi, evo = buffers(n, W.activation_ids(rng, n), lims, t_ms + 60_000, acts, ns, tks, ro, co, kind,
                                      ident, 10, n * _lib.REJECT_TEXT_MAX)
        rc = L.h_invoke_activations_events(h, jvm.obj(K_DIRECT, inb), jvm.obj(K_DIRECT, outb), jvm.obj(K_DIRECT, evi),
                                           jvm.obj(K_DIRECT, evo), n, 10, n * _lib.REJECT_TEXT_MAX, 2000, 43)
        assert rc == _lib.ERANGE
        summ = outb[:128].view(np.int64)
        assert summ[15] == 2 and summ[13] == 0 and summ[14] > 0 and summ[6] == 2
        assert evo[:8].view(np.int64)[0] > 10 and np.all(evo[base:base + 10] == 0xEE)
        assert L.h_oob() == 0
    finally:
        L.h_destroy(h)
