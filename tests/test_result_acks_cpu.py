"""CPU checks of the result-carrying acks (include/owgs.h "result-carrying acks"): the hand-written golden vectors pin
the host model (tests/result_acks_model.py), the model's completion half goes through the frozen ack oracle, the two
message generators meet their conditions, and the entry point's no-context argument checks (no device needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle as O
from openwhisk_amd import _lib
from openwhisk_amd import workload as W
from result_ack_cases import canonical_messages, fuzz_messages
from result_acks_model import FAIL, JVM, RESULT, UNSUPPORTED, ResultAckModel, classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1700000000123
FUZZ_SEED = 31


def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "result_ack_vectors.json"), encoding="utf-8") as f:
        return json.load(f)["vectors"]


def model_kind(msg: bytes):
    """(kind, right, aid) as the vectors state them: 3 = an accepted Combined message whose CompletionMessage text the
    ack oracle parses as a completion."""
    c = classify(msg)
    if c[0] in ("fail", "jvm", "unsup"):
        return {"fail": FAIL, "jvm": JVM, "unsup": UNSUPPORTED}[c[0]], None, None
    if c[0] == "result":
        return RESULT, int(c[3]), "%016x%016x" % (c[1], c[2])
    assert c[0] == "combined"
    k = int(O.parse_acks([c[1]], H)[0][0])
    if k != O.ACK_COMPLETION:
        return k, None, None
    return 3, int(c[4]), "%016x%016x" % (c[2], c[3])


def test_golden_file_is_what_the_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_result_ack_golden", os.path.join(ROOT, "tests", "golden", "make_result_ack_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.V == vectors()


def test_model_matches_the_golden_vectors():
    vs = vectors()
    for v in vs:
        k, right, aid = model_kind(v["msg"].encode("utf-8"))
        assert k == v["kind"], (v["name"], k)
        if k in (3, RESULT):
            assert (right, aid) == (v["right"], v["aid"]), v["name"]
    assert {v["kind"] for v in vs} == {FAIL, JVM, UNSUPPORTED, 3, RESULT}
    # every subset rule has a message inside and one outside
    for rule in ("member names", "namespace", "name", "subject", "cause", "start / end", "duration", "response", "logs",
                 "version", "publish", "annotations", "presence"):
        assert any(v["name"].startswith("inside " + rule + " #") for v in vs), rule
        assert any(v["name"].startswith("outside " + rule + " #") for v in vs), rule


def test_a_message_without_response_is_not_the_models_business():
    assert classify(W.completion_message("0" * 32, 3)) == ("plain",)


def test_canonical_generator_is_always_accepted():
    """(a) what WhiskActivation.serdes.write + compactPrint prints lies inside the accepted subset: every message."""
    msgs = canonical_messages(7, 500)
    for m in msgs:
        k, _, _ = model_kind(m) if classify(m)[0] != "plain" else (3, None, None)
        assert k in (3, RESULT), m
    # member order of the case class, numeric times
    one = json.loads(msgs[0])["response"]
    assert list(one)[:6] == ["namespace", "name", "subject", "activationId", "start", "end"]
    assert isinstance(one["start"], int) and list(one["response"])[0] == "statusCode"


def test_fuzz_generator_covers_accepted_jvm_and_fail():
    """(b) by the model alone, at least a quarter of the fuzz set falls in each of accepted, JVM and FAIL."""
    msgs = fuzz_messages(FUZZ_SEED, 2000)
    kinds = np.array([3 if classify(m)[0] == "plain" else model_kind(m)[0] for m in msgs])
    n = len(msgs)
    assert (kinds >= 3).sum() >= n // 4
    assert (kinds == JVM).sum() >= n // 4
    assert (kinds == FAIL).sum() >= n // 4
    assert (kinds == UNSUPPORTED).sum() >= 1


def test_model_flow_order_inside_a_batch():
    """Result before / after its completion, two Combined of one id, a duplicate Result."""
    w = W.config("c4", n_activations=2_000, n_invokers=8)
    st = O.state_for(w)
    md = ResultAckModel(O.AckFlow(st, H))
    aids = W.activation_ids(np.random.default_rng(1), 3)
    for t, a in enumerate(aids):
        inv, _ = st.publish(int(w.stream.act[t]), t)
        assert inv >= 0
        md.track(a, int(w.stream.act[t]), 100 + t)
    r = lambda a: b'{"transid":["sid_testing",1],"response":"' + a.encode() + b'"}'  # noqa: E731
    c = lambda a: (b'{"transid":["sid_testing",1],"response":"' + a.encode()  # noqa: E731
                   + b'","invoker":{"instance":0,"userMemory":"1 MB"}}')
    kind, inv, tk, fl, aid, roff, rlen = md.process(
        [r(aids[0]), r(aids[0]), W.completion_message(aids[0], 0), r(aids[0]), c(aids[1]), c(aids[1]), r(aids[1])])
    assert kind.tolist() == [7, 7, 3, 7, 3, 5, 7]
    assert tk.tolist() == [100, 100, 100, -1, 101, -1, -1]
    assert fl[4] & 8 and not fl[4] & 16 and (rlen[4], roff[4]) == (34, 40)
    assert md.flow.live() == 1 and list(md.by_id.values()) == [102]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_null_context_returns_einval_without_a_device(L):
    p = np.zeros(8, np.int64).ctypes.data_as(C.c_void_p)
    out = _lib.owgs_ack_out(p, p, p, p, p, p, p)
    s = np.zeros(3, np.int32).ctypes.data_as(C.c_void_p)
    for now, apply, summ in ((0, 0, None), (5, 1, s), (-1, 3, s), (7, 0, None)):
        assert L.owgs_process_result_acks(None, 1, p, p, C.byref(out), now, apply, summ) == _lib.EINVAL
    assert L.owgs_process_result_acks(None, 0, None, None, None, 0, 0, None) == _lib.EINVAL
    assert L.owgs_process_result_acks(None, -1, None, None, None, 0, 0, None) == _lib.EINVAL
