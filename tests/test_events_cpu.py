"""The throttle gate's user events and rejection texts without a device: the model (tests/events_model.py) against
vectors written by hand and against the reference's own example, the header's size macros against the model at the
extreme values, the binding's layout and constants against the header, the argument errors that are refused before a
device is needed, and the inputs of the GPU tests (tests/events_cases.py) checked on the model."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import events_cases as EC
import events_model as EM
import openwhisk_amd as ow
import oracle as O
from invoke_model import InvokeModel
from openwhisk_amd import _lib
from openwhisk_amd.balancer import Action
from publish_model import PublishModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MB = 2**20
SMALL = Action("ns", "ns/small", "0.0.1", 128)
BIG = Action("ns", "ns/big", "0.0.1", 256)
CONC = Action("ns", "ns/conc", "0.0.1", 128, 3)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "event_vectors.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ the model
def test_golden_file_is_what_its_script_writes(vectors, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_event_golden", os.path.join(HERE, "golden", "make_event_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert vectors == json.loads(json.dumps({"cases": mod.CASES, "doc_example": mod.DOC_EXAMPLE}))


def test_model_equals_the_vectors_written_by_hand(vectors):
    rows = set()
    for c in vectors["cases"]:
        ev = EM.event(c["kind"], c["verdict"], c["conc_count"], c["ts"], c["source"].encode(), c["a"].encode(),
                      c["b"].encode())
        tx = EM.text(c["kind"], c["verdict"], c["rate_count"], c["rate_limit"], c["conc_count"], c["conc_limit"])
        assert ev == c["event"].encode(), c["name"]
        assert tx == c["text"].encode(), c["name"]
        rows.add(EM.row_of(c["kind"], c["verdict"]))
    assert rows == {0, 1, 2, 3}
    cases = vectors["cases"]
    assert any(c["conc_count"] == 2**31 - 1 and '"metricValue":-2147483648' in c["event"] for c in cases)
    assert {0, 9, 10, 2**60 - 1} <= {c["ts"] for c in cases}
    seen = {c[k] for c in cases if c["text"] for k in ("rate_count", "rate_limit", "conc_count", "conc_limit")}
    assert {0, 9, 10, 99, 100, -2**31} <= seen
    assert any(c["a"] == "" and c["b"] == "" and c["source"] == "" for c in cases)


def test_member_order_is_the_hash_maps_and_the_references_example(vectors):
    doc = vectors["doc_example"]
    # Scala 2.12 HashMap iteration over jsonFormat7's seven members, computed; the two-member body is a Map2
    assert EM.hash_order(EM.EVENT_MEMBERS) == doc["members"]
    assert sorted(EM.EVENT_MEMBERS) == sorted(doc["members"])
    a, b = EM.identity_pieces(doc["subject"], doc["userId"], doc["namespace"])
    ev = EM.event(0, EM.OK, doc["metricValue"] - 1, doc["timestamp"], json.dumps(doc["source"]).encode(), a, b)
    obj = json.loads(ev, object_pairs_hook=list)
    assert [k for k, _ in obj] == doc["members"]
    assert [k for k, _ in dict(obj)["body"]] == doc["body_members"]
    assert json.loads(ev) == {"body": {"metricName": doc["metricName"], "metricValue": doc["metricValue"]},
                              "eventType": doc["eventType"], "source": doc["source"], "subject": doc["subject"],
                              "timestamp": doc["timestamp"], "userId": doc["userId"], "namespace": doc["namespace"]}


def test_every_model_event_parses_to_the_expected_members():
    pieces = EC.readable_identities()
    items = EC.random_items(5, 400, len(pieces))
    ev, tx = EC.model_of(items, pieces)
    for i in range(400):
        cls = EM.item_class(int(items["kind"][i]), int(items["verdict"][i]))
        if cls is None:
            assert ev[i] == b"" and tx[i] == b""
            continue
        k = int(items["ident"][i])
        want_v = 1 if cls else (int(items["conc_count"][i]) + 1 + 2**31) % 2**32 - 2**31
        assert json.loads(ev[i]) == {
            "body": {"metricName": EM.NAMES[cls], "metricValue": want_v}, "eventType": "Metric",
            "source": "controller0", "subject": "subject-%d" % k, "timestamp": int(items["ts_ms"][i]),
            "userId": "23bc46b1-71f6-4ed5-8c54-816aa4f8c5%02d" % k, "namespace": "space %d" % k}
        assert (tx[i] != b"") == (cls != 0)
        if cls:
            m = re.fullmatch(rb"Too many (requests in the last minute|concurrent requests in flight) "
                             rb"\(count: (-?\d+), allowed: (-?\d+)\)\.", tx[i])
            which = ("rate", "conc")[cls - 1]
            assert m and (m.group(1) == b"requests in the last minute") == (cls == 1)
            assert (int(m.group(2)), int(m.group(3))) == (items[which + "_count"][i], items[which + "_limit"][i])


def test_header_macros_bound_the_model(vectors):
    """The macros are derived from the literals; the model reaches them exactly at the extreme values."""
    assert _lib.EVENT_MAX_FIXED == len(EM.EVENT_LITERALS) + max(map(len, EM.NAMES)) + 11 + 20
    assert _lib.EVENT_NAME_MAX == max(map(len, EM.NAMES))
    S, A, B = b'"controller0"', b'"subject":"x"', b'"userId":"u","namespace":"n"'
    extra = len(S) + len(A) + len(B)
    # the longest name carries an int32 value: -2147483648 after the wrap; the longest timestamp is INT64_MIN
    assert len(EM.event(0, EM.OK, 2**31 - 1, -2**63, S, A, B)) == _lib.EVENT_MAX_FIXED + extra
    assert len(EM.text(0, EM.CONC, 0, 0, -2**31, -2**31)) == _lib.REJECT_TEXT_MAX
    assert len(EM.text(0, EM.RATE, -2**31, -2**31, 0, 0)) < _lib.REJECT_TEXT_MAX
    for seed, pieces in ((1, EC.identities()), (2, EC.readable_identities())):
        items = EC.random_items(seed, 1_000, len(pieces))
        ev, tx = EC.model_of(items, pieces)
        for i, k in enumerate(items["ident"]):
            assert len(ev[i]) <= _lib.EVENT_MAX_FIXED + len(EC.SOURCE) + sum(map(len, pieces[k]))
            assert len(tx[i]) <= _lib.REJECT_TEXT_MAX
    for c in vectors["cases"]:
        assert len(c["event"]) <= _lib.EVENT_MAX_FIXED + len(c["source"]) + len(c["a"]) + len(c["b"])
        assert len(c["text"]) <= _lib.REJECT_TEXT_MAX


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_declares_the_event_functions(L):
    for name in ("owgs_set_event_source", "owgs_register_event_identities", "owgs_throttle_events",
                 "owgs_invoke_activations_events"):
        assert name in ow.header_functions()
        assert hasattr(L, name)
    assert L.owgs_abi_version() == 1  # additive change


def test_layout_and_constants_match_the_header(tmp_path):
    """openwhisk_amd/csrc/events_abi_check.cpp prints sizeof / offsetof / the constants as the C compiler sees them."""
    exe = str(tmp_path / "events_abi_layout")
    subprocess.run(["g++", "-std=c++17", "-o", exe, os.path.join(ROOT, "openwhisk_amd", "csrc", "events_abi_check.cpp")],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = dict(line.split() for line in out.splitlines())
    assert int(seen.pop("sizeof.owgs_event_io")) == C.sizeof(_lib.owgs_event_io)
    offs = {k[len("offset."):]: int(v) for k, v in seen.items() if k.startswith("offset.")}
    assert list(offs) == [f[0] for f in _lib.owgs_event_io._fields_]                   # the header's order
    assert offs == {f[0]: getattr(_lib.owgs_event_io, f[0]).offset for f in _lib.owgs_event_io._fields_}
    consts = {k[len("const.OWGS_"):]: int(v) for k, v in seen.items() if k.startswith("const.")}
    assert consts.pop("ABI_VERSION") == 1
    assert consts == {k: getattr(_lib, k) for k in ("EVENT_NAME_MAX", "EVENT_MAX_FIXED", "REJECT_TEXT_MAX", "ADMIT_OK",
                                                   "ADMIT_RATE", "ADMIT_CONCURRENT", "ADMIT_TRIGGER")}
    # the Scala shim restates the two bounds (EventBuffers)
    scala = open(os.path.join(ROOT, "integration", "GpuShardingContainerPoolBalancer.scala")).read()
    assert int(re.search(r"val EventMaxFixed = (\d+)L", scala).group(1)) == _lib.EVENT_MAX_FIXED
    assert int(re.search(r"val RejectTextMax = (\d+)L", scala).group(1)) == _lib.REJECT_TEXT_MAX


def _ev(n=1, null=(), **over):
    keep = np.zeros(8 * (n + 2), np.int64)
    p = keep.ctypes.data_as(C.c_void_p)
    ev = _lib.owgs_event_io()
    for name in ("ident", "ev_out", "ev_off", "rej_out", "rej_off"):
        if name not in null:
            setattr(ev, name, p)
    ev.ev_cap = ev.rej_cap = 8
    for k, v in over.items():
        setattr(ev, k, v)
    return ev, keep


def test_argument_errors_that_need_no_device(L):
    z = np.zeros(8, np.int64)
    p = z.ctypes.data_as(C.c_void_p)
    f = L.owgs_throttle_events
    ev, keep = _ev()
    arrays = [p] * 7
    assert f(None, 1, *arrays, C.byref(ev)) == _lib.EINVAL
    # a non-NULL context pointer is never dereferenced before these are checked
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert f(fake, 1, *arrays, None) == _lib.EINVAL
    assert f(fake, -1, *arrays, C.byref(ev)) == _lib.EINVAL
    for k in range(7):                                                        # a NULL among the seven arrays
        assert f(fake, 1, *[None if j == k else p for j in range(7)], C.byref(ev)) == _lib.EINVAL, k
    for name in ("ident", "ev_out", "ev_off", "rej_out", "rej_off"):          # ... or among ev's pointers
        bad, _ = _ev(null=(name,))
        assert f(fake, 1, *arrays, C.byref(bad)) == _lib.EINVAL, name
    for over in (dict(ev_cap=-1), dict(rej_cap=-1)):
        bad, _ = _ev(**over)
        assert f(fake, 1, *arrays, C.byref(bad)) == _lib.EINVAL, over
    assert L.owgs_set_event_source(None, b'"c"', 3) == _lib.EINVAL
    assert L.owgs_set_event_source(fake, b'"c"', -1) == _lib.EINVAL
    assert L.owgs_set_event_source(fake, None, 3) == _lib.EINVAL
    assert L.owgs_register_event_identities(None, 1, p, p, p, p, None) == _lib.EINVAL
    assert L.owgs_register_event_identities(fake, -1, p, p, p, p, None) == _lib.EINVAL
    assert L.owgs_register_event_identities(fake, 1, p, None, p, p, None) == _lib.EINVAL
    assert L.owgs_register_event_identities(fake, 1, p, p, p, None, None) == _lib.EINVAL
    # the integrated call: io's errors as owgs_invoke_activations', ev's before the context is looked at
    g = L.owgs_invoke_activations_events
    io = _lib.owgs_invoke_io()
    io.n = 1
    for name, _ in _lib.owgs_invoke_io._fields_:
        if name not in ("n", "seq_base", "now_ms", "seq", "rate_override", "conc_override"):
            setattr(io, name, p)
    summ = (C.c_int64 * 16)()
    assert g(None, C.byref(io), None, None, C.byref(ev), summ) == _lib.EINVAL
    assert g(fake, None, None, None, C.byref(ev), summ) == _lib.EINVAL
    assert g(fake, C.byref(io), None, None, C.byref(ev), None) == _lib.EINVAL
    mb = _lib.owgs_msg_batch()
    assert g(fake, C.byref(io), C.byref(mb), None, C.byref(ev), summ) == _lib.EINVAL      # msgs without mo
    for name in ("ident", "ev_out", "ev_off", "rej_out", "rej_off"):
        bad, _ = _ev(null=(name,))
        assert g(fake, C.byref(io), None, None, C.byref(bad), summ) == _lib.EINVAL, name
    for over in (dict(ev_cap=-1), dict(rej_cap=-1)):
        bad, _ = _ev(**over)
        assert g(fake, C.byref(io), None, None, C.byref(bad), summ) == _lib.EINVAL, over
    io.out_verdict = None
    assert g(fake, C.byref(io), None, None, C.byref(ev), summ) == _lib.EINVAL
    assert not any(summ) and not keep.any() and not z.any()
    assert (ev.ev_total, ev.rej_total, ev.n_events, ev.n_rejects) == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def oracle_state(actions, seed):
    st = O.BalancerState(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=seed)
    st.update_invokers(np.arange(8), np.full(8, 512 * MB), np.zeros(8, np.uint8))
    hs = [st.register_action(a.namespace, a.path, k, a.mem_mb, a.max_concurrent, a.blackbox)
          for k, a in enumerate(actions)]
    return st, hs


def test_the_twelve_item_batch_has_the_gate_outputs_written_by_hand():
    st, hs = oracle_state((SMALL, BIG), 11)
    m = InvokeModel(PublishModel(st, dict(zip(hs, (SMALL, BIG)))), limits=EC.LIMITS)
    args, gate = EC.twelve(*hs)
    a = dict(args)
    got = m.invoke(a.pop("ns"), a.pop("kind"), a.pop("t_ms"), a.pop("actions"), a.pop("aids"), a.pop("tickets"),
                   a.pop("time_limit_ms"), a.pop("now_ms"), **a)
    for k in range(5):
        assert got[k].tolist() == gate[k], k
    assert all(s > 0 for s in EC.row_share(args["kind"], got[0]))


def test_the_six_hundred_item_batch_has_all_four_rows():
    st, hs = oracle_state((SMALL, BIG, CONC), 3)
    m = InvokeModel(PublishModel(st, dict(zip(hs, (SMALL, BIG, CONC)))), limits=EC.LIMITS)
    a = EC.six_hundred(hs)
    assert len(a["ns"]) == 600 and set(a["ns"].tolist()) == {0, 1, 2, 3}
    got = m.invoke(a["ns"], a["kind"], a["t_ms"], a["actions"], a["aids"], a["tickets"], a["time_limit_ms"],
                   a["now_ms"], a["rate_override"], a["conc_override"], seq_base=a["seq_base"])
    share = EC.row_share(a["kind"], got[0])
    assert all(s >= 0.05 for s in share), share
    assert got[9][0] > 0 and got[9][10] > 0


@pytest.mark.parametrize("n", [64, 65, 256, 257, 1_000])
def test_random_items_have_a_tenth_of_every_row(n):
    items = EC.random_items(n, n, len(EC.identities()))
    assert all(s >= 0.10 for s in EC.row_share(items["kind"], items["verdict"]))
    assert set(items["ident"].tolist()) <= set(range(len(EC.identities())))


def test_identity_pieces_cover_the_lengths():
    pieces = EC.identities()
    assert {len(a) for a, _ in pieces} == set(EC.PIECE_LENGTHS) == {len(b) for _, b in pieces}
