"""CPU checks of the supervision feeds (include/owgs.h "supervision feeds"): the ping golden vectors against the host
model (tests/feeds_model.py), the model's InvokerInstanceId rules against the frozen ack oracle, the fuzz set's
coverage, the ping_message helper and the new entry points' argument checks (no device needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle as O
from feeds_model import FAIL, FED, RANGE, UNSUPPORTED, ack_events, instance_id, ping_model, ping_parts
from openwhisk_amd import _lib
from openwhisk_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AID = "0123456789abcdef0123456789abcdef"
FUZZ_SEEDS = (21, 22)


def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "ping_vectors.json"), encoding="utf-8") as f:
        return json.load(f)["vectors"]


def canonical_pings():
    return [W.ping_message(0, "16384 MB"), W.ping_message(17, "2048 MB", unique="u-17"),
            W.ping_message(123456, "1 GB", unique="a", displayed="invoker-b"), W.ping_message(-1, "512 MB"),
            W.ping_message(1 << 24, "512 MB"), W.ping_message(9, "1024  MB")]


def fuzz_messages(seed, n=1000):
    """n byte-level mutations (W.mutate, 1-3 edits) over the vectors and the canonical pings."""
    rng = np.random.default_rng(seed)
    base = [v["msg"].encode("utf-8") for v in vectors()] + canonical_pings()
    return [W.mutate(rng, base[int(rng.integers(0, len(base)))], int(rng.integers(1, 4))) for _ in range(n)]


def test_golden_file_is_what_the_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ping_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_ping_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.V == vectors()


def test_model_matches_the_golden_vectors():
    vs = vectors()
    kind, inst, mem = ping_model([v["msg"].encode("utf-8") for v in vs])
    for i, v in enumerate(vs):
        assert (int(kind[i]), int(inst[i]), int(mem[i])) == (v["kind"], v["instance"], v["bytes"]), v["name"]
    assert {FAIL, UNSUPPORTED, FED, RANGE} == {v["kind"] for v in vs}


def test_ping_message_is_the_reference_serialisation():
    # PingMessage(InvokerInstanceId(...)).serialize: compactPrint, declaration order, None options omitted
    assert W.ping_message(0, "16384 MB") == b'{"name":{"instance":0,"userMemory":"16384 MB"}}'
    assert W.ping_message(3, "2 GB", unique="u") == b'{"name":{"instance":3,"uniqueName":"u","userMemory":"2 GB"}}'
    assert W.ping_message(3, "2 GB", displayed="d") == \
        b'{"name":{"instance":3,"displayedName":"d","userMemory":"2 GB"}}'
    assert W.ping_message(4, "1 MB", "u", "d") == \
        b'{"name":{"instance":4,"uniqueName":"u","displayedName":"d","userMemory":"1 MB"}}'
    assert W.ping_message(5, "1 MB", unique='a"b') == b'{"name":{"instance":5,"uniqueName":"a\\"b","userMemory":"1 MB"}}'
    k, i, m = ping_model([W.ping_message(4, "1 MB", "u", "d")])
    assert (k[0], i[0], m[0]) == (FED, 4, 1 << 20)


def _oracle_agrees(msgs):
    """The name member's object, wrapped as the `invoker` of a CompletionMessage, through the frozen ack oracle."""
    wrapped, expect = [], []
    for msg in msgs:
        what, v = ping_parts(msg)
        if what != "name" or not (isinstance(v, tuple) and v[0] == "obj"):
            continue
        a, b = v[2]
        wrapped.append(b'{"transid":["sid_testing",1],"activationId":"' + AID.encode() + b'","invoker":' + msg[a:b]
                       + b"}")
        expect.append(instance_id(v))
    kind, inst, _, _, _ = O.parse_acks(wrapped, 1700000000123)
    for j, r in enumerate(expect):
        want = {"ok": O.ACK_COMPLETION, "fail": O.ACK_FAIL, "unsup": O.ACK_UNSUPPORTED}[r[0]]
        assert kind[j] == want, (wrapped[j], r, int(kind[j]))
        if r[0] == "ok":
            assert inst[j] == r[1], (wrapped[j], r, int(inst[j]))
    return len(expect)


def test_model_instance_id_agrees_with_the_ack_oracle_on_the_vectors():
    assert _oracle_agrees([v["msg"].encode("utf-8") for v in vectors()]) >= 40


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_set_covers_every_outcome_and_agrees_with_the_ack_oracle(seed):
    msgs = fuzz_messages(seed)
    kind, _, _ = ping_model(msgs)
    for k in (FAIL, FED, RANGE):
        assert (kind == k).sum() >= 1, k
    assert _oracle_agrees(msgs) >= 100


def test_ack_events_rule():
    kind = [3, 4, 5, 6, 0, 1, 2, 3, 3, 3, 4]
    inv = [7, 8, 9, 1, 2, 3, 4, -1, 1 << 24, 5, 6]
    fl = [0, 1, 1, 0, 0, 0, 0, 0, 0, 3, 0]
    i, k = ack_events(kind, inv, fl)
    assert i.tolist() == [7, 8, 5, 6] and k.tolist() == [1, 2, 2, 1]
    i, k = ack_events(kind, inv, fl, forced=[1] * 11)
    assert i.tolist() == [7, 8, 5, 6] and k.tolist() == [3, 3, 3, 3]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_null_arguments_return_einval_without_a_device(L):
    one = np.zeros(4, np.int64)
    p = one.ctypes.data_as(C.c_void_p)
    s = np.zeros(3, np.int32).ctypes.data_as(C.c_void_p)
    # no context: whatever the other arguments and times are (in or out of range), nothing is touched
    for now in (0, -1, 1 << 60, 5):
        assert L.owgs_process_pings(None, 1, p, p, p, now, 0, p, p, p, s) == _lib.EINVAL
        assert L.owgs_process_acks_supervised(None, 1, p, p, p, p, p, p, now, 0, s) == _lib.EINVAL
        assert L.owgs_complete_activations_supervised(None, 1, p, p, p, p, p, p, now, 2, s) == _lib.EINVAL
    assert L.owgs_process_pings(None, -1, None, None, None, 0, 0, None, None, None, None) == _lib.EINVAL
    assert L.owgs_process_acks_supervised(None, 0, None, None, None, None, None, None, 0, 0, None) == _lib.EINVAL
    assert L.owgs_complete_activations_supervised(None, 0, None, None, None, None, None, None, 0, 0, None) == \
        _lib.EINVAL
