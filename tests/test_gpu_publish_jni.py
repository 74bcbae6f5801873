"""The publishActivations native of the JNI binding (integration/owgs_jni.c) executed through the JNIEnv stand-in of
tests/jni_stub (tests/jni_publish/publish_harness.c adds its ctypes wrapper), the way tests/test_gpu_feeds_jni.py
drives the feed natives.  The CPU test checks the binding's argument handling; the GPU test compares one batch with
the ctypes path on a twin context."""
import ctypes as C
import os

import numpy as np
import pytest

from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd import workload as W
from openwhisk_amd._lib import THROW_INDEX
from openwhisk_amd.balancer import Action

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "integration", "build", "libowgs_jni_publish_harness.so")
K_INTS, K_BYTES, K_STRING, K_DIRECT = 1, 3, 4, 5
MB = 1 << 20
ACTIONS = [Action("ns", "ns/managed", "0.0.1", 256), Action("ns", "ns/conc", "0.0.1", 128, 3),
           Action("", "polygenelubricants", "0.0.1", 256)]   # the last one's hash is Int.MinValue: schedule throws


class Jvm:
    def __init__(self):
        _lib.lib()  # the engine first: the harness links against the same libowgs.so
        if not os.path.exists(HARNESS):
            pytest.skip("integration/build/libowgs_jni_publish_harness.so not built (make -C integration)")
        L = C.CDLL(HARNESS)
        P, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, res, args in [("h_obj", P, [C.c_int, P, i64]), ("h_free", None, [P]), ("h_oob", C.c_long, []),
                                ("h_create", i64, [C.c_double, C.c_double, i64, i32, i32, i64]),
                                ("h_destroy", None, [i64]), ("h_update_invokers", i32, [i64, P, P, P]),
                                ("h_register_action", i32, [i64, P, P, P, i32, i32, i32]),
                                ("h_publish_activations", i32, [i64, P, P, i32, i32, i64, i64]),
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


def buffers(n, aids, lims, acts, ns, tks):
    """PublishBuffers' layout: in = aid[2n], limit[n] (int64), action[n], ns[n], ticket[n] (int32)."""
    w = np.zeros(2 * n, np.uint64)
    w[0::2] = [int(a[:16], 16) for a in aids]
    w[1::2] = [int(a[16:], 16) for a in aids]
    inb = np.concatenate([w.view(np.uint8), np.asarray(lims, np.int64).view(np.uint8),
                          np.asarray(acts, np.int32).view(np.uint8), np.asarray(ns, np.int32).view(np.uint8),
                          np.asarray(tks, np.int32).view(np.uint8)]).copy()
    assert inb.nbytes == 36 * n
    return inb, np.full(64 + 10 * n, 0xEE, np.uint8)


def test_publish_native_rejects_bad_shapes_without_a_device(jvm):
    L = jvm.L
    n = 4
    inb, outb = buffers(n, ["%032x" % k for k in range(n)], [0] * n, [0] * n, [0] * n, [0] * n)
    din, dout = jvm.obj(K_DIRECT, inb), jvm.obj(K_DIRECT, outb)
    assert L.h_publish_activations(0, None, dout, n, 0, 0, 0) == _lib.EINVAL
    assert L.h_publish_activations(0, din, None, n, 0, 0, 0) == _lib.EINVAL
    assert L.h_publish_activations(0, din, dout, -1, 0, 0, 0) == _lib.EINVAL
    assert L.h_publish_activations(0, din, dout, n + 1, 0, 0, 0) == _lib.EINVAL            # beyond the buffers
    assert L.h_publish_activations(0, din, jvm.obj(K_DIRECT, outb[:-1]), n, 0, 0, 0) == _lib.EINVAL
    assert L.h_publish_activations(0, jvm.obj(K_BYTES, inb.view(np.int8)), dout, n, 0, 0, 0) == _lib.EINVAL  # not direct
    assert L.h_publish_activations(0, din, dout, n, 0, 0, 0) == _lib.EINVAL                # null context: the engine's
    assert np.all(outb == 0xEE) and L.h_oob() == 0


@pytest.mark.gpu
def test_publish_native_matches_the_ctypes_path(jvm):
    L = jvm.L
    h = L.h_create(0.75, 0.25, 128 * MB, 1, 0, 7)
    assert h != 0
    ref = GpuShardingContainerPoolBalancer(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=7)
    try:
        ids, mem, st8 = np.arange(4, dtype=np.int32), np.full(4, 1024 * MB, np.int64), np.zeros(4, np.int8)
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
        n = 65
        rng = np.random.default_rng(3)
        acts = np.where(np.arange(n) % 7 == 3, hs[2], np.where(np.arange(n) % 2, hs[1], hs[0])).astype(np.int32)
        aids = W.activation_ids(rng, n)
        aids[64] = aids[3]                                   # a duplicate of a throwing item: it creates the entry
        aids[12] = aids[0]
        lims = np.array([100, 300_000])[rng.integers(0, 2, n)]
        ns = np.where(np.arange(n) % 5 == 0, -1, rns[np.arange(n) % 2]).astype(np.int32)
        tks = np.arange(n) + 500
        inb, outb = buffers(n, aids, lims, acts, ns, tks)
        rc = L.h_publish_activations(h, jvm.obj(K_DIRECT, inb), jvm.obj(K_DIRECT, outb), n, 1, 1000, 42)
        assert rc == 0, L.h_last_error(h)
        r_inv, r_fl, r_tk, r_ex, r_sum = ref.publish_activations(acts, aids, tks, lims, 42, ns=ns, seq_base=1000)
        assert outb[:64].view(np.int64).tolist() == r_sum.tolist()
        assert np.array_equal(outb[64:64 + 4 * n].view(np.int32), r_inv)
        assert np.array_equal(outb[64 + 4 * n:64 + 8 * n].view(np.int32), r_tk)
        assert np.array_equal(outb[64 + 8 * n:64 + 9 * n], r_fl)
        assert np.array_equal(outb[64 + 9 * n:], r_ex)
        # the batch is what it was meant to be: thrown items, their later duplicate creating the entry
        assert r_inv[3] == THROW_INDEX and r_tk[3] == -1 and (r_tk[64], r_ex[64]) == (564, 0)
        assert (r_tk[12], r_ex[12]) == (500, 1) and r_sum[5] == 9 and r_sum[0] == n - 9 and r_sum[6] == 2
        live = C.c_int64()
        assert _lib.lib().owgs_activations_live(hctx, C.byref(live)) == 0
        assert live.value == ref.activations_live() == r_sum[1]
        tot = np.zeros(3, np.int64)
        assert _lib.lib().owgs_activation_totals(hctx, tot.ctypes.data_as(C.c_void_p)) == 0
        assert tuple(tot) == ref.activation_totals()
        assert L.h_oob() == 0
    finally:
        L.h_destroy(h)
