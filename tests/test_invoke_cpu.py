"""owgs_invoke_activations without a device: the model (tests/invoke_model.py) against a case replayed by hand, the
struct layout and constants of the binding against the header, and the argument errors refused before the engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openwhisk_amd as ow
import oracle as O
from invoke_model import InvokeModel
from openwhisk_amd import _lib
from openwhisk_amd.balancer import Action
from publish_model import PublishModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MB = 2**20
ACT, TRIG, RO, CO = 0, 1, 2, 4
SMALL = Action("ns", "ns/small", "0.0.1", 128)
BIG = Action("ns", "ns/big", "0.0.1", 256)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def oracle_state():
    st = O.BalancerState(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=11)
    st.update_invokers(np.arange(8), np.full(8, 512 * MB), np.zeros(8, np.uint8))
    hs = [st.register_action(a.namespace, a.path, k, a.mem_mb, a.max_concurrent, a.blackbox)
          for k, a in enumerate((SMALL, BIG))]
    return st, hs


def test_model_equals_a_replay_by_hand():
    """Twelve items, limits 3 invokes / 3 fires per minute and 2 concurrent, one minute, two namespaces (0 and 1).
      i  ns kind        what happens, item by item
      0  0  action      invoke count 1 <= 3; in flight 0 < 2: admitted, rank 0
      1  0  action      count 2; 1 < 2: admitted, rank 1
      2  0  trigger     fire count 1 <= 3: OK, never published
      3  0  action      count 3 <= 3; 2 < 2 fails: CONCURRENT (count 2)
      4  0  action      count 4 > 3: RATE; it carries the id X
      5  1  action      count 1; 0 < 2: admitted, rank 2
      6  1  action CO=1 count 2; 1 < 1 fails: CONCURRENT (count 1, limit 1)
      7  1  action RO=10 count 3 <= 10; 1 < 2: admitted, rank 3; id X again: the rejected item 4 left no entry, this
                        one creates it
      8  1  trigger     fire count 1: OK
      9  1  action      count 4 > 3: RATE
     10  0  trigger RO=0 limit 0, fire count 2 > 0: RATE
     11  1  action RO=10 CO=5  count 5 <= 10; 2 < 5: admitted, rank 4; the id of item 0: existed, item 0's ticket
    The five admitted actions fit the pool (at most 256 MB each on 512 MB invokers), so each gets an invoker: the
    oracle's, asked in rank order with seq_base + rank."""
    st, (small, big) = oracle_state()
    m = InvokeModel(PublishModel(st, {small: SMALL, big: BIG}), limits=(3, 3, 2))
    ns = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1]
    kind = [ACT, ACT, TRIG, ACT, ACT, ACT, CO, RO, TRIG, ACT, TRIG | RO, RO | CO]
    ro = [0, 0, 0, 0, 0, 0, 0, 10, 0, 0, 0, 10]
    co = [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 5]
    t = [600_000 + i for i in range(12)]
    acts = [small, big, 99, small, big, small, big, big, -7, small, 12345, small]   # a trigger's handle is never read
    aids = ["%032x" % (0xA0 + i) for i in range(12)]
    aids[7] = aids[4]
    aids[11] = aids[0]
    tks = [50 + i for i in range(12)]
    got = m.invoke(ns, kind, t, acts, aids, tks, [100] * 12, 1_000, ro, co, seq_base=100)
    assert got[0].tolist() == [0, 0, 0, 2, 1, 0, 2, 0, 0, 1, 1, 0]
    assert got[1].tolist() == [1, 2, 1, 3, 4, 1, 2, 3, 1, 4, 2, 5]
    assert got[2].tolist() == [3, 3, 3, 3, 3, 3, 3, 10, 3, 3, 0, 10]
    assert got[3].tolist() == [0, 1, -1, 2, -1, 0, 1, 1, -1, -1, -1, 2]
    assert got[4].tolist() == [2, 2, 0, 2, 2, 2, 1, 2, 0, 2, 0, 5]
    twin, _ = oracle_state()
    dec = [twin.publish(a, 100 + k) for k, a in enumerate([small, big, small, big, small])]
    assert all(d[0] >= 0 for d in dec)
    want_inv = [_lib.NOT_PUBLISHED] * 12
    want_fl = [0] * 12
    for k, i in enumerate([0, 1, 5, 7, 11]):
        want_inv[i], want_fl[i] = dec[k]
    assert got[5].tolist() == want_inv and got[6].tolist() == want_fl
    assert got[7].tolist() == [50, 51, -1, -1, -1, 55, -1, 57, -1, -1, -1, 50]
    assert got[8].tolist() == [0] * 11 + [1]
    assert got[9] == [5, 4, 0, 0, 0, 0, 2, 0, 5, 3, 2, 2, 0, 0, 0, 0]
    assert m.pm.t.books([0, 1]) == ([2, 3], (5, 3 * 128 + 2 * 256, 0)) and m.pm.t.live() == 4
    assert m.rate == {(0, 0): [10, 4], (0, 1): [10, 2], (1, 0): [10, 5], (1, 1): [10, 1]}
    assert m.rate_records([0, 1, 2], 1) == ([10, 10, -2**63], [2, 1, 0])
    assert np.array_equal(st.permits(), twin.permits())


def test_header_declares_invoke_activations(L):
    assert "owgs_invoke_activations" in ow.header_functions()
    assert hasattr(L, "owgs_invoke_activations")
    assert L.owgs_abi_version() == 1  # additive change


def test_layout_and_constants_match_the_header(tmp_path):
    """openwhisk_amd/csrc/invoke_abi_check.cpp prints sizeof / offsetof / the constants as the C compiler sees them."""
    exe = str(tmp_path / "invoke_abi_layout")
    subprocess.run(["g++", "-std=c++17", "-o", exe, os.path.join(ROOT, "openwhisk_amd", "csrc", "invoke_abi_check.cpp")],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = dict(line.split() for line in out.splitlines())
    assert int(seen.pop("sizeof.owgs_invoke_io")) == C.sizeof(_lib.owgs_invoke_io)
    offs = {k[len("offset."):]: int(v) for k, v in seen.items() if k.startswith("offset.")}
    assert list(offs) == [f[0] for f in _lib.owgs_invoke_io._fields_]                  # the header's order
    assert offs == {f[0]: getattr(_lib.owgs_invoke_io, f[0]).offset for f in _lib.owgs_invoke_io._fields_}
    consts = {k[len("const.OWGS_"):]: int(v) for k, v in seen.items() if k.startswith("const.")}
    assert consts.pop("ABI_VERSION") == 1
    assert consts == {k: getattr(_lib, k) for k in (
        "NOT_PUBLISHED", "NONE", "THROW_INDEX", "ADMIT_OK", "ADMIT_RATE", "ADMIT_CONCURRENT", "ADMIT_TRIGGER",
        "ADMIT_RATE_OVERRIDE", "ADMIT_CONC_OVERRIDE")}
    assert _lib.NOT_PUBLISHED not in (_lib.NONE, _lib.THROW_INDEX) and _lib.NOT_PUBLISHED < 0


def _io(n=1, null=()):
    z = np.zeros(8, np.int64)
    p = z.ctypes.data_as(C.c_void_p)
    io = _lib.owgs_invoke_io()
    io.n = n
    for name, _ in _lib.owgs_invoke_io._fields_:
        if name not in ("n", "seq_base", "now_ms", "seq", "rate_override", "conc_override") and name not in null:
            setattr(io, name, p)
    return io, z


def test_argument_errors_that_need_no_device(L):
    summ = (C.c_int64 * 16)()
    io, keep = _io()
    f = L.owgs_invoke_activations
    assert f(None, C.byref(io), None, None, summ) == _lib.EINVAL
    assert f(None, None, None, None, summ) == _lib.EINVAL
    # a non-NULL context pointer is never dereferenced before these are checked
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert f(fake, None, None, None, summ) == _lib.EINVAL
    assert f(fake, C.byref(io), None, None, None) == _lib.EINVAL
    mb, mo = _lib.owgs_msg_batch(), _lib.owgs_msg_out()
    assert f(fake, C.byref(io), C.byref(mb), None, summ) == _lib.EINVAL      # msgs without mo
    assert f(fake, C.byref(io), None, C.byref(mo), summ) == _lib.EINVAL      # mo without msgs
    neg, _ = _io(n=-1)
    assert f(fake, C.byref(neg), None, None, summ) == _lib.EINVAL
    required = [name for name, _ in _lib.owgs_invoke_io._fields_
                if name not in ("n", "seq_base", "now_ms", "seq", "rate_override", "conc_override")]
    assert len(required) == 16
    for name in required:                                                    # a NULL among the required pointers
        bad, _ = _io(null=(name,))
        assert f(fake, C.byref(bad), None, None, summ) == _lib.EINVAL, name
    assert not any(summ) and not keep.any()
