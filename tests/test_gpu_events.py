"""The throttle gate's user events and rejection texts on the device: owgs_throttle_events against
vectors written by hand and against tests/events_model.py, its capacity contract, and owgs_invoke_activations_events
against owgs_invoke_activations on a twin context plus the model applied to the gate's outputs.  The inputs are those
tests/test_events_cpu.py checks on the model (tests/events_cases.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import events_cases as EC
import events_model as EM
from openwhisk_amd import GpuShardingContainerPoolBalancer, _lib
from openwhisk_amd._lib import ENOENT, EINVAL, ERANGE, OwgsError
from openwhisk_amd.balancer import Action, _p

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MB = 2**20
SMALL = Action("ns", "ns/small", "0.0.1", 128)
BIG = Action("ns", "ns/big", "0.0.1", 256)
CONC = Action("ns", "ns/conc", "0.0.1", 128, 3)
WIDE = Action("ns", "ns/wide", "0.0.1", 128, 4096)          # beyond the on-chip engine: a large-state context
TA = ['"action":{"path":"ns","name":"a%d"},"revision":null,"user":{"subject":"s%d"}' % (k, k) for k in range(3)]
TB = ["[]", '["x1"]', "[]"]
N_TOPICS = 8
NS = np.arange(4, dtype=np.int32)
GATE = ("verdict", "rate_count", "rate_limit", "conc_count", "conc_limit", "invoker", "flags", "ticket", "existed")


def balancer(actions=(SMALL, BIG), seed=11, pieces=None, source=EC.SOURCE):
    """A context set up for the gated publish (8 invokers of 512 MB, limits 3 / 3 / 2, four namespaces, templates)
    and, with pieces, for its events."""
    b = GpuShardingContainerPoolBalancer(managed_fraction=0.75, blackbox_fraction=0.25, rng_seed=seed)
    b.update_invokers_arrays(np.arange(8), np.full(8, 512 * MB), np.zeros(8, np.uint8))
    hs, _ = b.register_actions(list(actions))
    b.set_throttle_limits(*EC.LIMITS)
    assert b.register_templates(TA, TB) == 0
    assert b.register_namespaces([0xE7E7 << 64 | k for k in range(4)]).tolist() == NS.tolist()
    if pieces is not None:
        b.set_event_source(source)
        assert b.register_event_identities([a for a, _ in pieces], [x for _, x in pieces]) == 0
    return b, [int(h) for h in hs]


@pytest.fixture(scope="module")
def standalone():
    """One context for the stand-alone calls (they change no state) with the identities of events_cases."""
    pieces = EC.identities()
    b, _ = balancer(pieces=pieces)
    return b, pieces


def state_of(b):
    return (b.permits().tolist(), b.active_activations_for(NS).tolist(), b.activation_totals(), b.activations_live(),
            [x.tolist() for w in (0, 1) for x in b.rate_state(NS, w)])


# ------------------------------------------------------------------------------------------------ stand-alone
def test_golden_cases_byte_exact():
    with open(os.path.join(HERE, "golden", "event_vectors.json")) as f:
        cases = json.load(f)["cases"]
    groups = {}
    for c in cases:                                            # one context per event source
        groups.setdefault(c["source"], []).append(c)
    for source, cs in groups.items():
        b, _ = balancer(pieces=[(c["a"].encode(), c["b"].encode()) for c in cs], source=source)
        col = lambda k: [c[k] for c in cs]  # noqa: E731
        ev, tx = b.throttle_events(col("kind"), col("verdict"), col("rate_count"), col("rate_limit"), col("conc_count"),
                                   col("conc_limit"), col("ts"), np.arange(len(cs)))
        for i, c in enumerate(cs):
            assert ev[i] == c["event"].encode(), c["name"]
            assert tx[i] == c["text"].encode(), c["name"]
        for i, c in enumerate(cs):                             # ... and each alone: n = 1, offsets from 0
            e1, t1 = b.throttle_events([c["kind"]], [c["verdict"]], [c["rate_count"]], [c["rate_limit"]],
                                       [c["conc_count"]], [c["conc_limit"]], [c["ts"]], [i])
            assert (e1, t1) == ([c["event"].encode()], [c["text"].encode()]), c["name"]


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 1_000])
def test_standalone_equals_the_model(standalone, n):
    """n = 1 cannot hold a tenth of each of four rows: it runs once per row instead (four calls of one item); from 64 on
    the condition is asserted on the inputs."""
    b, pieces = standalone
    runs = [EC.random_items(n, n, len(pieces))] if n > 1 else [EC.random_items(10 + r, 1, len(pieces), row=r)
                                                                for r in range(4)]
    for items in runs:
        if n > 1:
            assert all(s >= 0.10 for s in EC.row_share(items["kind"], items["verdict"]))
        want = EC.model_of(items, pieces)
        got = b.throttle_events(**items)
        assert got[0] == want[0]
        assert got[1] == want[1]
    if n == 1_000:
        assert {len(a) for a, _ in pieces} == set(EC.PIECE_LENGTHS)
        assert any(int(c) == 2**31 - 1 and v == 0 and not k & 1
                   for c, v, k in zip(items["conc_count"], items["verdict"], items["kind"]))    # the wrapping value


def raw_events(b, items, ev_cap, rej_cap, fill=0xEE):
    """owgs_throttle_events through the raw entry point with sentinel-filled regions: (rc, struct, ev, rej, offsets)."""
    n = len(items["kind"])
    ev_buf = np.full(max(ev_cap, 1) + 16, fill, np.uint8)
    rej_buf = np.full(max(rej_cap, 1) + 16, fill, np.uint8)
    ev_off, rej_off = np.full(n + 1, -1, np.int64), np.full(n + 1, -1, np.int64)
    ident = np.ascontiguousarray(items["ident"], np.int32)
    E = _lib.owgs_event_io(_p(ident), _p(ev_buf), ev_cap, _p(ev_off), _p(rej_buf), rej_cap, _p(rej_off), -1, -1, -1, -1)
    arrs = [np.ascontiguousarray(items[k], dt) for k, dt in (
        ("kind", np.uint8), ("verdict", np.uint8), ("rate_count", np.int32), ("rate_limit", np.int32),
        ("conc_count", np.int32), ("conc_limit", np.int32), ("ts_ms", np.int64))]
    rc = _lib.lib().owgs_throttle_events(b._h, n, *[_p(a) for a in arrs], C.byref(E))
    return rc, E, ev_buf, rej_buf, ev_off, rej_off


def test_capacity(standalone):
    b, pieces = standalone
    items = EC.random_items(77, 130, len(pieces))
    want_ev, want_tx = EC.model_of(items, pieces)
    ev_all, tx_all = b"".join(want_ev), b"".join(want_tx)
    n_ev, n_tx = sum(1 for x in want_ev if x), sum(1 for x in want_tx if x)
    ev_offs = np.concatenate([[0], np.cumsum([len(x) for x in want_ev])])
    tx_offs = np.concatenate([[0], np.cumsum([len(x) for x in want_tx])])

    def check(rc, E, want_rc, ev_written, tx_written, bufs):
        ev_buf, rej_buf, ev_off, rej_off = bufs
        assert rc == want_rc
        assert (E.ev_total, E.rej_total, E.n_events, E.n_rejects) == (len(ev_all), len(tx_all), n_ev, n_tx)
        assert np.array_equal(ev_off, ev_offs) and np.array_equal(rej_off, tx_offs)
        if ev_written:
            assert ev_buf[:len(ev_all)].tobytes() == ev_all and np.all(ev_buf[len(ev_all):] == 0xEE)
        else:
            assert np.all(ev_buf == 0xEE)                      # the refused region's sentinel bytes are untouched
        if tx_written:
            assert rej_buf[:len(tx_all)].tobytes() == tx_all and np.all(rej_buf[len(tx_all):] == 0xEE)
        else:
            assert np.all(rej_buf == 0xEE)

    rc, E, *bufs = raw_events(b, items, len(ev_all), len(tx_all))              # cap == total
    check(rc, E, 0, True, True, bufs)
    rc, E, *bufs = raw_events(b, items, len(ev_all) - 1, len(tx_all))          # events one byte short
    check(rc, E, ERANGE, False, True, bufs)
    rc, E, *bufs = raw_events(b, items, len(ev_all), len(tx_all) - 1)          # texts one byte short
    check(rc, E, ERANGE, True, False, bufs)
    rc, E, *bufs = raw_events(b, items, 0, 0)
    check(rc, E, ERANGE, False, False, bufs)
    rc, E, *bufs = raw_events(b, items, len(ev_all) + 100, len(tx_all) + 7)    # a repeat with room, same context
    check(rc, E, 0, True, True, bufs)
    with pytest.raises(OwgsError) as e:                                         # ... and through the binding
        b.throttle_events(**items, ev_cap=len(ev_all) - 1)
    assert e.value.code == ERANGE and e.value.events == (None, want_tx)
    assert (e.value.ev_total, e.value.rej_total) == (len(ev_all), len(tx_all))
    assert b.throttle_events(**items) == (want_ev, want_tx)


def test_standalone_argument_errors(standalone):
    b, pieces = standalone
    items = EC.random_items(3, 20, len(pieces))

    def bad(key, i, v):
        x = dict(items)
        x[key] = np.array(items[key]).copy()
        x[key][i] = v
        return x

    for code, x in ((EINVAL, bad("verdict", 19, 3)), (EINVAL, bad("kind", 0, 8)), (ENOENT, bad("ident", 7, len(pieces))),
                    (ENOENT, bad("ident", 7, -1))):
        rc, E, ev_buf, rej_buf, ev_off, rej_off = raw_events(b, x, 1 << 16, 1 << 12)
        assert rc == code
        assert np.all(ev_buf == 0xEE) and np.all(rej_buf == 0xEE) and np.all(ev_off == -1) and E.ev_total == -1
    # an item without an event still needs a registered identity
    x = bad("ident", 0, 99)
    x["kind"], x["verdict"] = x["kind"].copy(), x["verdict"].copy()
    x["kind"][0], x["verdict"][0] = 1, 0
    assert raw_events(b, x, 1 << 16, 1 << 12)[0] == ENOENT
    nb, _ = balancer()                                                          # no event source set
    nb.register_event_identities([b"a"], [b"b"])
    rc, E, *_ = raw_events(nb, EC.random_items(3, 4, 1), 1 << 12, 1 << 12)
    assert rc == EINVAL and E.ev_total == -1
    nb.set_event_source('"c"')
    assert raw_events(nb, EC.random_items(3, 4, 1), 1 << 12, 1 << 12)[0] == 0
    assert b.throttle_events([], [], [], [], [], [], [], []) == ([], [])       # n == 0
    for ao, bo in (([1, 1], [0, 0]), ([0, 2, 1], [0, 0, 0])):                   # offsets not from 0 / decreasing
        a_off, b_off = np.array(ao, np.int64), np.array(bo + [0] * (len(ao) - len(bo)), np.int64)
        buf = np.zeros(8, np.uint8)
        assert _lib.lib().owgs_register_event_identities(nb._h, len(ao) - 1, _p(buf), _p(a_off), _p(buf), _p(b_off),
                                                         None) == EINVAL
    assert nb.register_event_identities([b"x"], [b"y"]) == 1                    # the refused calls registered nothing


# ------------------------------------------------------------------------------------------------ integrated
def integrated(actions, seed, args, pieces, ident, msgs=True, waits=1):
    """One owgs_invoke_activations_events call beside owgs_invoke_activations on a twin context: every output and the
    state afterwards equal, the events those of the model over the gate's outputs.  Returns (outputs, events, texts)."""
    b, hs = balancer(actions, seed, pieces)
    tw, _ = balancer(actions, seed)
    n = len(args["ns"])
    M = dict(EC.messages(n), n_topics=N_TOPICS, cap=1 << 20) if msgs else None
    got = b.invoke_activations(**args, msgs=M, events={"ident": ident})
    ref = tw.invoke_activations(**args, msgs=M)
    for k, name in enumerate(GATE):
        assert np.array_equal(got[k], ref[k]) and got[k].dtype == ref[k].dtype, name
    gs, rs = got[9].tolist(), ref[9].tolist()
    assert gs[:13] == rs[:13] and rs[13:] == [0, 0, 0] and gs[12] == waits
    if msgs:
        assert got[10][0] == ref[10][0] and all(np.array_equal(got[10][k], ref[10][k]) for k in (1, 2, 3))
    assert state_of(b) == state_of(tw)                          # permits, books, totals, entries, rate records
    want = EM.throttle_events(args["kind"], got[0], got[1], got[2], got[3], got[4], args["t_ms"], ident,
                              EC.SOURCE.encode(), pieces)
    ev, tx = got[-1]
    assert ev == want[0] and tx == want[1]
    assert gs[13:] == [sum(1 for x in ev if x), sum(1 for x in tx if x), 1]
    assert gs[13] == gs[8] + gs[9] + gs[10] and gs[14] == gs[9] + gs[10]
    return got, b, tw


def test_integrated_twelve_items():
    pieces = EC.readable_identities()
    b0, hs = balancer()
    args, gate = EC.twelve(*hs)
    ident = np.arange(12) % len(pieces)
    got, b, tw = integrated((SMALL, BIG), 11, args, pieces, ident)
    for k in range(5):
        assert got[k].tolist() == gate[k], GATE[k]
    assert got[9][12] == 1 and got[9][13:].tolist() == [10, 5, 1]
    ev, tx = got[-1]
    assert json.loads(ev[3])["body"] == {"metricName": "ConcurrentRateLimit", "metricValue": 1}
    assert tx[3] == b"Too many concurrent requests in flight (count: 2, allowed: 2)."
    assert tx[10] == b"Too many requests in the last minute (count: 2, allowed: 0)."
    assert json.loads(ev[11])["body"] == {"metricName": "ConcurrentInvocations", "metricValue": 3}
    assert ev[2] == b"" and ev[8] == b"" and json.loads(ev[0])["timestamp"] == 600_000
    # the two-stage form (no messages) gives the same events
    got2, _, _ = integrated((SMALL, BIG), 11, args, pieces, ident, msgs=False)
    assert got2[-1] == got[-1]


def test_integrated_six_hundred_items():
    pieces = EC.identities()
    _, hs = balancer((SMALL, BIG, CONC), 3)
    args = EC.six_hundred(hs)
    ident = np.random.default_rng(4).integers(0, len(pieces), 600).astype(np.int32)
    got, b, tw = integrated((SMALL, BIG, CONC), 3, args, pieces, ident)
    assert all(s > 0 for s in EC.row_share(args["kind"], got[0]))
    assert got[9][12] == 1 and got[9][15] == 1
    # a second call on the same contexts: the events follow the state the first one left
    args2 = EC.six_hundred(hs, seed=22)
    args2["t_ms"] = args2["t_ms"] + 3_600_000
    M = dict(EC.messages(600, 2), n_topics=N_TOPICS, cap=1 << 20)
    g2 = b.invoke_activations(**args2, msgs=M, events={"ident": ident})
    r2 = tw.invoke_activations(**args2, msgs=M)
    assert all(np.array_equal(g2[k], r2[k]) for k in range(9)) and g2[9][:13].tolist() == r2[9][:13].tolist()
    want = EM.throttle_events(args2["kind"], g2[0], g2[1], g2[2], g2[3], g2[4], args2["t_ms"], ident,
                              EC.SOURCE.encode(), pieces)
    assert g2[-1] == want and state_of(b) == state_of(tw)


def test_integrated_on_a_large_state_context():
    pieces = EC.readable_identities()
    acts = (SMALL, BIG, WIDE)
    b0, hs = balancer(acts, 3)
    assert b0.large_stats() is not None                        # maxConcurrent 4,096: the large-state engine
    args = EC.six_hundred(hs, seed=23, n=257)
    ident = np.arange(257) % len(pieces)
    got, b, tw = integrated(acts, 3, args, pieces, ident, waits=2)
    assert got[9][8] > 0 and got[9][9] > 0 and got[9][15] == 1


def test_null_events_equal_the_old_entry_point():
    _, hs = balancer((SMALL, BIG, CONC), 3)
    args = EC.six_hundred(hs, seed=24, n=130)
    n = 130
    outs = []
    for fn in ("owgs_invoke_activations_events", "owgs_invoke_activations"):
        b, _ = balancer((SMALL, BIG, CONC), 3)
        w = np.zeros(2 * n, np.uint64)
        w[0::2] = [int(a[:16], 16) for a in args["aids"]]
        w[1::2] = [int(a[16:], 16) for a in args["aids"]]
        o8 = [np.full(n, 0xEE, np.uint8) for _ in range(3)]
        o32 = [np.full(n, -9, np.int32) for _ in range(6)]
        lims = np.ascontiguousarray(args["time_limit_ms"], np.int64)
        io = _lib.owgs_invoke_io(n, _p(args["ns"]), _p(args["kind"]), _p(args["t_ms"]), _p(args["rate_override"]),
                                 _p(args["conc_override"]), _p(args["actions"]), None, args["seq_base"], _p(w),
                                 _p(args["tickets"]), _p(lims), args["now_ms"], _p(o8[0]), _p(o32[0]), _p(o32[1]),
                                 _p(o32[2]), _p(o32[3]), _p(o32[4]), _p(o8[1]), _p(o32[5]), _p(o8[2]))
        summ = np.full(16, -1, np.int64)
        f = getattr(_lib.lib(), fn)
        rc = f(b._h, C.byref(io), None, None, None, _p(summ)) if fn.endswith("events") else \
            f(b._h, C.byref(io), None, None, _p(summ))
        assert rc == 0
        outs.append(([x.tolist() for x in o8 + o32], summ.tolist(), state_of(b)))
    assert outs[0] == outs[1] and outs[0][1][13:] == [0, 0, 0] and outs[0][1][12] == 1


def test_integrated_capacity_and_errors():
    pieces = EC.readable_identities()
    b, hs = balancer((SMALL, BIG), 11, pieces)
    tw, _ = balancer((SMALL, BIG), 11)
    args, _ = EC.twelve(*hs)
    ident = np.arange(12) % len(pieces)
    before = state_of(b)
    for code, events in ((ENOENT, {"ident": np.where(np.arange(12) == 8, len(pieces), ident)}),
                         (EINVAL, {"ident": ident, "ev_cap": -1})):
        with pytest.raises(OwgsError) as e:                    # refused before any state changes, the rate records too
            b.invoke_activations(**args, events=events)
        assert e.value.code == code and state_of(b) == before
    nb, _ = balancer((SMALL, BIG), 11)
    nb.register_event_identities([a for a, _ in pieces], [x for _, x in pieces])
    with pytest.raises(OwgsError) as e:                        # the event source not set
        nb.invoke_activations(**args, events={"ident": ident})
    assert e.value.code == EINVAL and state_of(nb) == before
    # the event region one byte short: everything else is done and valid, the texts are written
    M = dict(EC.messages(12), n_topics=N_TOPICS, cap=1 << 16)
    ref = tw.invoke_activations(**args, msgs=M)
    want = EM.throttle_events(args["kind"], ref[0], ref[1], ref[2], ref[3], ref[4], args["t_ms"], ident,
                              EC.SOURCE.encode(), pieces)
    total = sum(map(len, want[0]))
    with pytest.raises(OwgsError) as e:
        b.invoke_activations(**args, msgs=M, events={"ident": ident, "ev_cap": total - 1})
    err = e.value
    assert err.code == ERANGE and (err.ev_total, err.rej_total) == (total, sum(map(len, want[1])))
    assert err.events == (None, want[1])
    for k in range(9):
        assert np.array_equal(err.partial[k], ref[k]), GATE[k]
    s = err.partial[9].tolist()
    assert s[:13] == ref[9][:13].tolist() and s[13:] == [0, 5, 2] and s[6] == 3
    assert err.partial[10][0] == ref[10][0]
    assert state_of(b) == state_of(tw)
    # the caller repeats only the events, from the outputs it holds
    again = b.throttle_events(args["kind"], *err.partial[:5], args["t_ms"], ident)
    assert again == want
