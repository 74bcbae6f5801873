"""CPU-side checks of owgs_publish_activations: the ABI refuses NULLs without a device, and the model the GPU tests
compare against (tests/publish_model.py) reproduces hand-written vectors (tests/golden/publish_vectors.json, derived
from SCPB:292-316 and CLB:116-166 by hand in tests/golden/make_publish_golden.py)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import openwhisk_amd as ow
import oracle as O
from openwhisk_amd import _lib
from publish_model import PublishModel

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_publish_activations(L):
    assert "owgs_publish_activations" in ow.header_functions()
    assert hasattr(L, "owgs_publish_activations")
    assert L.owgs_abi_version() == 1  # additive change


def test_null_context_and_null_io_are_einval(L):
    summ = (C.c_int64 * 8)()
    io = _lib.owgs_publish_io()
    assert L.owgs_publish_activations(None, C.byref(io), None, None, summ) == _lib.EINVAL
    assert L.owgs_publish_activations(None, None, None, None, summ) == _lib.EINVAL
    # a non-NULL context pointer is never dereferenced before io is checked
    fake = C.create_string_buffer(64)
    assert L.owgs_publish_activations(C.cast(fake, C.c_void_p), None, None, None, summ) == _lib.EINVAL
    assert L.owgs_publish_activations(C.cast(fake, C.c_void_p), C.byref(io), None, None, None) == _lib.EINVAL


def test_struct_layouts_match_the_header():
    # LP64: int32 + padding, then pointers / 64-bit words in the header's order
    assert C.sizeof(_lib.owgs_publish_io) == 13 * 8
    assert _lib.owgs_publish_io.now_ms.offset == 64 and _lib.owgs_publish_io.out_existed.offset == 96
    assert C.sizeof(_lib.owgs_msg_out) == 8 * 8
    assert _lib.owgs_msg_out.total.offset == 48 and _lib.owgs_msg_out.m.offset == 56


def _cases():
    with open(os.path.join(HERE, "golden", "publish_vectors.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"][:40])
def test_model_reproduces_the_hand_written_vectors(case):
    st = O.BalancerState(managed_fraction=1.0, blackbox_fraction=0.0)
    st.update_invokers(np.arange(4), np.full(4, 1024 * 2**20), np.zeros(4, np.uint8))
    actions = {int(k): types.SimpleNamespace(mem_mb=v[0], blackbox=v[1]) for k, v in case["actions"].items()}
    m = PublishModel(st, actions)
    for e in case["before"]:
        assert m.t.track(e["aid"], e["action"], e["ticket"], e["invoker"], e["limit"], e["now"], e["ns"]) == \
            (e["ticket"], 0)
    it = case["items"]
    col = lambda k: [x[k] for x in it]  # noqa: E731
    ticket, existed, summ = m.setup(col("decision"), col("flag"), col("action"), col("aid"), col("ticket"),
                                    col("limit"), case["now"], col("ns"))
    assert ticket.tolist() == case["ticket"]
    assert existed.tolist() == case["existed"]
    assert summ == case["summary"]
    assert m.t.live() == case["live"]
    handles = sorted(int(k) for k in case["active"])
    active, totals = m.t.books(handles)
    assert active == [case["active"][str(h)] for h in handles]
    assert list(totals) == case["totals"]
    assert m.t.next_deadline() == case["next_deadline"]
    assert [list(x) for x in m.armed_order()] == case["armed"]


def test_vectors_cover_the_required_situations():
    it = _cases()[0]["items"]
    ids = [x["aid"] for x in it]
    dec = [x["decision"] for x in it]
    assert any(d >= 0 for d in dec) and -2 in dec and -1 in dec
    dup = [(i, ids.index(a)) for i, a in enumerate(ids) if ids.index(a) < i]
    assert any(dec[j] >= 0 and dec[i] >= 0 for i, j in dup)       # a duplicate of a placed item
    assert any(dec[j] == -2 and dec[i] >= 0 for i, j in dup)      # a duplicate of a thrown item, placed later
    before = {e["aid"] for e in _cases()[0]["before"]}
    assert any(a in before for a in ids)                          # a duplicate of a pre-existing entry
