"""The invokeActivations native of the JNI binding (integration/owgs_jni.c) executed through the JNIEnv stand-in of
tests/jni_stub (tests/jni_invoke/invoke_harness.c adds its ctypes wrapper), the way tests/test_gpu_publish_jni.py drives
publishActivations.  The CPU test checks the binding's argument handling; the GPU test compares one mixed batch with
the ctypes path on a twin context."""
import ctypes as C
import os

import numpy as np
import pytest

from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd import workload as W
from openwhisk_amd._lib import ADMIT_CONCURRENT, ADMIT_OK, ADMIT_RATE, NOT_PUBLISHED
from openwhisk_amd.balancer import Action

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "integration", "build", "libowgs_jni_invoke_harness.so")
K_INTS, K_BYTES, K_STRING, K_DIRECT = 1, 3, 4, 5
MB = 1 << 20
TRIG, RO, CO = 1, 2, 4
ACTIONS = [Action("ns", "ns/small", "0.0.1", 128), Action("ns", "ns/big", "0.0.1", 256),
           Action("ns", "ns/conc", "0.0.1", 128, 3)]


class Jvm:
    def __init__(self):
        _lib.lib()  # the engine first: the harness links against the same libowgs.so
        assert os.path.exists(HARNESS), "integration/build/libowgs_jni_invoke_harness.so not built (make -C integration)"
        L = C.CDLL(HARNESS)
        P, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, res, args in [("h_obj", P, [C.c_int, P, i64]), ("h_free", None, [P]), ("h_oob", C.c_long, []),
                                ("h_create", i64, [C.c_double, C.c_double, i64, i32, i32, i64]),
                                ("h_destroy", None, [i64]), ("h_update_invokers", i32, [i64, P, P, P]),
                                ("h_register_action", i32, [i64, P, P, P, i32, i32, i32]),
                                ("h_invoke_activations", i32, [i64, P, P, i32, i64, i64]),
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


def buffers(n, aids, lims, t_ms, acts, ns, tks, ro, co, kind):
    """InvokeBuffers' layout: in = aid[2n], limit[n], t_ms[n] (int64), action, ns, ticket, rate / conc override [n]
    (int32), kind[n] (bytes)."""
    w = np.zeros(2 * n, np.uint64)
    w[0::2] = [int(a[:16], 16) for a in aids]
    w[1::2] = [int(a[16:], 16) for a in aids]
    parts = [w, np.asarray(lims, np.int64), np.asarray(t_ms, np.int64)]
    parts += [np.asarray(x, np.int32) for x in (acts, ns, tks, ro, co)] + [np.asarray(kind, np.uint8)]
    inb = np.concatenate([p.view(np.uint8) for p in parts]).copy()
    assert inb.nbytes == 53 * n
    return inb, np.full(128 + 27 * n, 0xEE, np.uint8)


def test_invoke_native_rejects_bad_shapes_without_a_device(jvm):
    L = jvm.L
    n = 4
    z = [0] * n
    inb, outb = buffers(n, ["%032x" % k for k in range(n)], z, z, z, z, z, z, z, z)
    din, dout = jvm.obj(K_DIRECT, inb), jvm.obj(K_DIRECT, outb)
    assert L.h_invoke_activations(0, None, dout, n, 0, 0) == _lib.EINVAL
    assert L.h_invoke_activations(0, din, None, n, 0, 0) == _lib.EINVAL
    assert L.h_invoke_activations(0, din, dout, -1, 0, 0) == _lib.EINVAL
    assert L.h_invoke_activations(0, din, dout, n + 1, 0, 0) == _lib.EINVAL               # beyond the buffers
    assert L.h_invoke_activations(0, din, jvm.obj(K_DIRECT, outb[:-1]), n, 0, 0) == _lib.EINVAL
    assert L.h_invoke_activations(0, jvm.obj(K_BYTES, inb.view(np.int8)), dout, n, 0, 0) == _lib.EINVAL  # not direct
    assert L.h_invoke_activations(0, din, dout, n, 0, 0) == _lib.EINVAL                   # null context: the engine's
    assert np.all(outb == 0xEE) and L.h_oob() == 0


@pytest.mark.gpu
def test_invoke_native_matches_the_ctypes_path(jvm):
    L = jvm.L
    h = L.h_create(0.75, 0.25, 128 * MB, 1, 0, 7)
    assert h != 0
    ref = GpuShardingContainerPoolBalancer(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=7)
    try:
        ids, mem, st8 = np.arange(8, dtype=np.int32), np.full(8, 512 * MB, np.int64), np.zeros(8, np.int8)
        assert L.h_update_invokers(h, jvm.obj(K_INTS, ids), jvm.obj(2, mem), jvm.obj(K_BYTES, st8)) == 0
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
        n = 130
        rng = np.random.default_rng(4)
        acts = hs[np.arange(n) % 3].astype(np.int32)
        aids = W.activation_ids(rng, n)
        aids[70] = aids[2]                                   # a duplicate of an admitted item
        lims = np.array([100, 300_000])[rng.integers(0, 2, n)]
        ns = rns[np.arange(n) % 2].astype(np.int32)
        tks = np.arange(n) + 500
        t_ms = 600_000 + np.arange(n)
        # every seventh item a trigger; every fifth item carries overrides that let it through
        kind = np.where(np.arange(n) % 7 == 3, TRIG, 0) | np.where(np.arange(n) % 5 == 0, RO | CO, 0)
        ro, co = np.full(n, 1000, np.int32), np.full(n, 1000, np.int32)
        inb, outb = buffers(n, aids, lims, t_ms, acts, ns, tks, ro, co, kind)
        rc = L.h_invoke_activations(h, jvm.obj(K_DIRECT, inb), jvm.obj(K_DIRECT, outb), n, 1000, 42)
        assert rc == 0, L.h_last_error(h)
        r = ref.invoke_activations(ns, kind.astype(np.uint8), t_ms, acts, aids, tks, lims, 42, rate_override=ro,
                                   conc_override=co, seq_base=1000)
        assert outb[:128].view(np.int64).tolist() == r[9].tolist()
        ints = outb[128:128 + 24 * n].view(np.int32).reshape(6, n)
        for k, j in enumerate((1, 2, 3, 4, 5, 7)):           # rate count / limit, conc count / limit, invoker, ticket
            assert np.array_equal(ints[k], r[j]), j
        byts = outb[128 + 24 * n:].reshape(3, n)
        for k, j in enumerate((0, 6, 8)):                    # verdict, flags, existed
            assert np.array_equal(byts[k], r[j]), j
        # the batch is what it was meant to be: all three verdicts, triggers, a duplicate of a placed item
        assert {ADMIT_OK, ADMIT_RATE, ADMIT_CONCURRENT} == set(r[0].tolist())
        s = r[9]
        assert s[8] > 0 and s[9] > 0 and s[10] > 0 and s[11] == 9 and s[0] == s[8] and s[6] == 2 and s[12] == 1
        assert np.all(r[5][(kind & TRIG) != 0] == NOT_PUBLISHED)
        assert r[0][2] == ADMIT_OK and r[0][70] == ADMIT_OK and (r[7][70], r[8][70]) == (502, 1)
        live = C.c_int64()
        assert _lib.lib().owgs_activations_live(hctx, C.byref(live)) == 0
        assert live.value == ref.activations_live() == s[1]
        tot = np.zeros(3, np.int64)
        assert _lib.lib().owgs_activation_totals(hctx, tot.ctypes.data_as(C.c_void_p)) == 0
        assert tuple(tot) == ref.activation_totals()
        assert L.h_oob() == 0
    finally:
        L.h_destroy(h)
