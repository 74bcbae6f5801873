"""The supervision-feed natives of the JNI binding (processPings, processAcksSupervised, completeActivationsSupervised
in integration/owgs_jni.c) executed through the JNIEnv stand-in of tests/jni_stub (tests/jni_feeds/feeds_harness.c adds
their ctypes wrappers), the way tests/test_gpu_jni.py drives the older natives.  The CPU test checks the binding's
argument handling; the GPU test compares a short loop with the ctypes path on a second context."""
import ctypes as C
import os

import numpy as np
import pytest

from feeds_model import FED, ping_model
from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "integration", "build", "libowgs_jni_feeds_harness.so")
K_INTS, K_LONGS, K_BYTES = 1, 2, 3
H = 1700000000123
MB = 1 << 20


class Jvm:
    def __init__(self):
        _lib.lib()  # the engine first: the harness links against the same libowgs.so
        if not os.path.exists(HARNESS):
            pytest.skip("integration/build/libowgs_jni_feeds_harness.so not built (make -C integration)")
        L = C.CDLL(HARNESS)
        P, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, res, args in [("h_obj", P, [C.c_int, P, i64]), ("h_free", None, [P]), ("h_oob", C.c_long, []),
                                ("h_create", i64, [C.c_double, C.c_double, i64, i32, i32, i64]),
                                ("h_destroy", None, [i64]),
                                ("h_process_pings", i32, [i64, P, P, P, i32, i64, i32, P, P, P, P]),
                                ("h_process_acks_supervised", i32, [i64, P, P, i32, P, P, P, P, i64, i32, P]),
                                ("h_complete_activations_supervised", i32,
                                 [i64, P, P, P, i32, P, P, P, i64, i32, P]),
                                ("h_last_error", C.c_char_p, [i64])]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        self.L, self.keep, self.objs = L, [], []

    def obj(self, kind, arr):
        self.keep.append(arr)
        o = self.L.h_obj(kind, arr.ctypes.data_as(C.c_void_p), len(arr))
        self.objs.append(o)
        return o

    def ints(self, a):
        return self.obj(K_INTS, np.ascontiguousarray(a, np.int32))

    def longs(self, a):
        return self.obj(K_LONGS, np.ascontiguousarray(a, np.int64))

    def bytes_(self, a):
        return self.obj(K_BYTES, np.ascontiguousarray(a).view(np.int8))

    def blob(self, msgs):
        off = np.zeros(len(msgs) + 1, np.int64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return self.bytes_(np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()), self.longs(off)

    def close(self):
        for o in self.objs:
            self.L.h_free(o)
        self.objs.clear()


@pytest.fixture
def jvm():
    j = Jvm()
    yield j
    j.close()


def test_feed_natives_reject_bad_shapes_without_a_device(jvm):
    L = jvm.L
    msgs = [W.ping_message(0, "1 MB"), W.ping_message(1, "1 MB")]
    by, off = jvm.blob(msgs)
    k, i, m, s = jvm.bytes_(np.zeros(2, np.uint8)), jvm.ints([0, 0]), jvm.longs([0, 0]), jvm.ints([0, 0, 0])
    t = jvm.longs([0, 0])
    assert L.h_process_pings(0, by, off, t, 3, 0, 0, k, i, m, s) == _lib.EINVAL            # n beyond the arrays
    assert L.h_process_pings(0, by, off, t, 2, 0, 0, k, i, m, jvm.ints([0, 0])) == _lib.EINVAL  # short summary
    assert L.h_process_pings(0, by, jvm.longs([0, 5, 10_000]), t, 2, 0, 0, k, i, m, s) == _lib.EINVAL  # past the bytes
    assert L.h_process_pings(0, None, off, t, 2, 0, 0, k, i, m, s) == _lib.EINVAL
    assert L.h_process_pings(0, by, off, t, 2, 0, 0, k, i, m, s) == _lib.EINVAL            # null context: the engine's
    tk, fl = jvm.ints([0, 0]), jvm.bytes_(np.zeros(2, np.uint8))
    assert L.h_process_acks_supervised(0, by, off, 2, k, i, tk, fl, 0, 0, None) == _lib.EINVAL
    assert L.h_process_acks_supervised(0, by, jvm.longs([0, 1]), 2, k, i, tk, fl, 0, 0, s) == _lib.EINVAL
    aid = jvm.bytes_(np.frombuffer(b"0" * 63, np.uint8).copy())
    assert L.h_complete_activations_supervised(0, aid, i, fl, 2, k, tk, fl, 0, 0, s) == _lib.EINVAL  # 63 < 2 * 32
    assert L.h_oob() == 0


@pytest.mark.gpu
def test_feed_natives_match_the_ctypes_path(jvm):
    L = jvm.L
    h = L.h_create(0.9, 0.1, 128 * MB, 1, 0, 7)
    assert h != 0
    ref = GpuShardingContainerPoolBalancer(managed_fraction=0.9, blackbox_fraction=0.1, rng_seed=7)
    lib = _lib.lib()
    try:
        ref.set_health_tid(H)
        assert lib.owgs_set_health_tid(C.c_void_p(h), H) == 0
        n = 70
        pings = [W.ping_message(i, "%d MB" % (1024 + i)) if i % 7 else b'{"name":' for i in range(n)]
        t = np.arange(n, dtype=np.int64)
        by, off = jvm.blob(pings)
        k, inst, mem, summ = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(3, np.int32)
        rc = L.h_process_pings(h, by, off, jvm.longs(t), n, n, 2, jvm.obj(K_BYTES, k), jvm.obj(K_INTS, inst),
                               jvm.obj(K_LONGS, mem), jvm.obj(K_INTS, summ))
        assert rc == 0, L.h_last_error(h)
        rk, ri, rm, rs = ref.process_pings(pings, t, n, apply=2)
        mk, mi, mm = ping_model(pings)
        assert np.array_equal(k.view(np.uint8), rk) and np.array_equal(inst, ri) and np.array_equal(mem, rm)
        assert np.array_equal(rk, mk) and np.array_equal(ri, mi) and np.array_equal(rm, mm)
        assert tuple(summ) == rs == (int((mk == FED).sum()), n, int((mk == FED).sum()))
        # health acks make the pinged invokers Healthy; one unparsable message in between
        rng = np.random.default_rng(1)
        acks = [W.completion_message(a, i, tid=("sid_invokerHealth", H))
                for i, a in enumerate(W.activation_ids(rng, n))]
        acks.insert(5, b"[1,")
        by, off = jvm.blob(acks)
        m = len(acks)
        k, inv, tk, fl = np.zeros(m, np.int8), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int8)
        rc = L.h_process_acks_supervised(h, by, off, m, jvm.obj(K_BYTES, k), jvm.obj(K_INTS, inv), jvm.obj(K_INTS, tk),
                                         jvm.obj(K_BYTES, fl), n + 1, 2, jvm.obj(K_INTS, summ))
        assert rc == 0, L.h_last_error(h)
        rk, ri, rt, rf, rs = ref.process_acks_supervised(acks, n + 1, apply=2)
        assert np.array_equal(k.view(np.uint8), rk) and np.array_equal(inv, ri) and np.array_equal(tk, rt)
        assert np.array_equal(fl.view(np.uint8), rf) and tuple(summ) == rs and rs[0] == n
        # forced completions without entries feed nothing; a health one feeds a Timeout
        aids = W.activation_ids(rng, 3)
        a32 = jvm.bytes_(np.frombuffer("".join(aids).encode("ascii"), np.uint8).copy())
        k3, t3, f3 = np.zeros(3, np.int8), np.zeros(3, np.int32), np.zeros(3, np.int8)
        rc = L.h_complete_activations_supervised(h, a32, jvm.ints([1, 2, 3]), jvm.bytes_(np.array([1, 1, 5], np.uint8)),
                                                 3, jvm.obj(K_BYTES, k3), jvm.obj(K_INTS, t3), jvm.obj(K_BYTES, f3),
                                                 n + 2, 1, jvm.obj(K_INTS, summ))
        assert rc == 0, L.h_last_error(h)
        rk, rt, rf, rs = ref.complete_activations_supervised(aids, [1, 2, 3], n + 2, apply=1, forced=[1, 1, 1],
                                                             health=[0, 0, 1])
        assert np.array_equal(k3.view(np.uint8), rk) and np.array_equal(t3, rt) and tuple(summ) == rs == (1, 0, 0)
        # both contexts hold the same FSM state
        cap = n
        st, um, te = np.zeros(cap, np.uint8), np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        sz = C.c_int32()
        assert lib.owgs_health_read(C.c_void_p(h), cap, C.byref(sz), st.ctypes.data_as(C.c_void_p),
                                    um.ctypes.data_as(C.c_void_p), te.ctypes.data_as(C.c_void_p), None, None) == 0
        g = ref.health_read()
        assert sz.value == len(g[0]) == n
        assert np.array_equal(st, g[0]) and np.array_equal(um, g[1]) and np.array_equal(te, g[2])
        assert L.h_oob() == 0
    finally:
        L.h_destroy(h)
