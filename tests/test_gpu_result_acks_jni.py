"""The processResultAcks native of the JNI binding (integration/owgs_jni.c) executed through the JNIEnv stand-in of
tests/jni_stub (tests/jni_results/results_harness.c adds its ctypes wrapper), the way tests/test_gpu_feeds_jni.py drives
the feed natives.  The CPU test checks the binding's argument handling; the GPU test compares a batch of all three
message types with the ctypes path on a second context."""
import ctypes as C
import os

import numpy as np
import pytest

from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd import workload as W
from openwhisk_amd.balancer import Action
from result_ack_cases import canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "integration", "build", "libowgs_jni_results_harness.so")
K_INTS, K_LONGS, K_BYTES = 1, 2, 3
H = 1700000000123
MB = 1 << 20


class Jvm:
    def __init__(self):
        _lib.lib()  # the engine first: the harness links against the same libowgs.so
        assert os.path.exists(HARNESS), "integration/build/libowgs_jni_results_harness.so not built (make -C integration)"
        L = C.CDLL(HARNESS)
        P, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, res, args in [("h_obj", P, [C.c_int, P, i64]), ("h_free", None, [P]), ("h_oob", C.c_long, []),
                                ("h_create", i64, [C.c_double, C.c_double, i64, i32, i32, i64]),
                                ("h_destroy", None, [i64]),
                                ("h_process_result_acks", i32, [i64, P, P, i32, P, P, P, P, P, P, P, i64, i32, P]),
                                ("h_last_error", C.c_char_p, [i64])]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        self.L, self.keep, self.objs = L, [], []

    def obj(self, kind, arr):
        self.keep.append(arr)
        o = self.L.h_obj(kind, arr.ctypes.data_as(C.c_void_p), len(arr))
        self.objs.append(o)
        return o

    def blob(self, msgs):
        off = np.zeros(len(msgs) + 1, np.int64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return (self.obj(K_BYTES, np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy().view(np.int8)),
                self.obj(K_LONGS, off))

    def outputs(self, n, aid_words=None):
        a = [np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int8),
             np.zeros(2 * n if aid_words is None else aid_words, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)]
        return a, [self.obj(k, x) for k, x in zip((K_BYTES, K_INTS, K_INTS, K_BYTES, K_LONGS, K_LONGS, K_INTS), a)]

    def close(self):
        for o in self.objs:
            self.L.h_free(o)
        self.objs.clear()


@pytest.fixture
def jvm():
    j = Jvm()
    yield j
    j.close()


def test_native_rejects_bad_shapes_without_a_device(jvm):
    L = jvm.L
    msgs = [W.combined_message("0" * 32, 0), W.completion_message("1" * 32, 1)]
    by, off = jvm.blob(msgs)
    _, o = jvm.outputs(2)
    s = jvm.obj(K_INTS, np.zeros(3, np.int32))
    assert L.h_process_result_acks(0, by, off, 3, *o, 0, 0, s) == _lib.EINVAL                 # n beyond the arrays
    assert L.h_process_result_acks(0, by, off, 2, *jvm.outputs(2, aid_words=3)[1], 0, 0, s) == _lib.EINVAL  # short aid
    assert L.h_process_result_acks(0, by, off, 2, *o, 0, 0, jvm.obj(K_INTS, np.zeros(2, np.int32))) == _lib.EINVAL
    assert L.h_process_result_acks(0, by, jvm.obj(K_LONGS, np.array([0, 5, 10_000])), 2, *o, 0, 0, s) == _lib.EINVAL
    for miss in range(7):
        assert L.h_process_result_acks(0, by, off, 2, *[None if q == miss else x for q, x in enumerate(o)], 0, 0,
                                       s) == _lib.EINVAL
    assert L.h_process_result_acks(0, by, off, 2, *o, 0, 0, None) == _lib.EINVAL              # null context: the engine's
    assert L.h_oob() == 0


@pytest.mark.gpu
def test_native_matches_the_ctypes_path(jvm):
    L = jvm.L
    h = L.h_create(1.0, 0.0, 128 * MB, 1, 0, 7)
    assert h != 0
    ref = GpuShardingContainerPoolBalancer(managed_fraction=1.0, blackbox_fraction=0.0, rng_seed=7)
    lib = _lib.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        ids, mem, st8 = np.arange(4, dtype=np.int32), np.full(4, 1024 * MB, np.int64), np.zeros(4, np.uint8)
        ref.update_invokers_arrays(ids, mem, st8)
        assert lib.owgs_update_invokers(C.c_void_p(h), 4, P(ids), P(mem), P(st8)) == 0
        act = Action("ns", "ns/a", "0.0.1", 256)
        (a,), _ = ref.register_actions([act])
        ns, path, key = b"ns", b"ns/a", b"ns/a@0.0.1"
        o2 = np.array([0, 2], np.int32)
        assert lib.owgs_register_actions(
            C.c_void_p(h), 1, ns, P(o2), path, P(np.array([0, 4], np.int32)), key,
            P(np.array([0, len(key)], np.int32)), P(np.array([256], np.int32)), P(np.array([1], np.int32)),
            P(np.array([0], np.uint8)), P(np.zeros(1, np.int32)), None) == 0
        rng = np.random.default_rng(2)
        aids = W.activation_ids(rng, 6)
        a32 = np.frombuffer("".join(aids).encode(), np.uint8)
        acts, tks = np.full(6, a, np.int32), np.arange(50, 56, dtype=np.int32)
        ot, ox = np.zeros(6, np.int32), np.zeros(6, np.uint8)
        assert lib.owgs_track_activations(C.c_void_p(h), 6, P(a32), P(acts), P(tks), P(ot), P(ox)) == 0
        ref.track_activations(aids, acts, tks)
        msgs = [canonical(rng, aids[0], 0, "result", 80), canonical(rng, aids[0], 0, "combined", 80),
                canonical(rng, aids[1], 1, "combined-left"), canonical(rng, aids[2], 2, "completion"),
                canonical(rng, aids[2], 2, "result-left"), b'{"response":5}',
                canonical(rng, aids[3], 3, "combined", 80).replace(b'"publish":false', b'"publish":null')]
        n = len(msgs)
        by, off = jvm.blob(msgs)
        for now, apply, with_summary in ((0, 0, False), (5, 2, True)):
            arr, o = jvm.outputs(n)
            summ = np.zeros(3, np.int32)
            rc = L.h_process_result_acks(h, by, off, n, *o, now, apply, jvm.obj(K_INTS, summ) if with_summary else None)
            assert rc == 0, L.h_last_error(h)
            r = ref.process_result_acks(msgs, now if with_summary else None, apply)
            assert np.array_equal(arr[0].view(np.uint8), r[0]) and np.array_equal(arr[1], r[1])
            assert np.array_equal(arr[2], r[2]) and np.array_equal(arr[3].view(np.uint8), r[3])
            assert np.array_equal(arr[4].view(np.uint64).reshape(n, 2), r[4])
            assert np.array_equal(arr[5], r[5]) and np.array_equal(arr[6], r[6])
            if with_summary:
                assert tuple(summ) == r[7]
            else:  # the first pass: by the hand-written order rules
                assert r[0].tolist() == [7, 3, 3, 3, 7, 0, 1] and r[2].tolist() == [50, 50, 51, 52, -1, -1, -1]
        assert L.h_oob() == 0
    finally:
        L.h_destroy(h)
