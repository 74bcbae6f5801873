"""Inputs the event tests share (tests/test_events_cpu.py checks them on the model before tests/test_gpu_events.py
hands them to a device): the twelve-item batch of tests/test_invoke_cpu.py::test_model_equals_a_replay_by_hand, the
600-item batch over four namespaces, random stand-alone items with every row of the table well represented, and
identities whose piece lengths cross a lane window (64) and go far beyond it."""
import numpy as np

import events_model as EM

ACT, TRIG, RO, CO = 0, 1, 2, 4
OK, RATE, CONC = 0, 1, 2
IMAX, IMIN = 2**31 - 1, -2**31
SOURCE = '"controller0"'
PIECE_LENGTHS = (0, 1, 63, 64, 65, 200, 5_000)
LIMITS = (3, 3, 2)                      # invokes / fires per minute, concurrent invocations
BIGLIM = 1_000_000


def twelve(small, big):
    """The twelve items of test_model_equals_a_replay_by_hand (its docstring replays them one by one) as keyword
    arguments of invoke_activations / InvokeModel.invoke, and the gate outputs written there by hand."""
    aids = ["%032x" % (0xA0 + i) for i in range(12)]
    aids[7] = aids[4]
    aids[11] = aids[0]
    args = dict(ns=[0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1],
                kind=[ACT, ACT, TRIG, ACT, ACT, ACT, CO, RO, TRIG, ACT, TRIG | RO, RO | CO],
                t_ms=[600_000 + i for i in range(12)],
                actions=[small, big, 99, small, big, small, big, big, -7, small, 12345, small],
                aids=aids, tickets=[50 + i for i in range(12)], time_limit_ms=[100] * 12, now_ms=1_000,
                rate_override=[0, 0, 0, 0, 0, 0, 0, 10, 0, 0, 0, 10],
                conc_override=[0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 5], seq_base=100)
    gate = ([0, 0, 0, 2, 1, 0, 2, 0, 0, 1, 1, 0], [1, 2, 1, 3, 4, 1, 2, 3, 1, 4, 2, 5],
            [3, 3, 3, 3, 3, 3, 3, 10, 3, 3, 0, 10], [0, 1, -1, 2, -1, 0, 1, 1, -1, -1, -1, 2],
            [2, 2, 0, 2, 2, 2, 1, 2, 0, 2, 0, 5])
    return args, gate


def six_hundred(handles, seed=21, n=600):
    """n items over four namespaces and twenty minutes (so the per-minute counts restart), limits 3 / 3 / 2: 30 %
    triggers, a fifth of the items with overrides that let them through."""
    rng = np.random.default_rng(seed)
    over = rng.random(n) < 0.2
    kind = (np.where(rng.random(n) < 0.3, TRIG, ACT) | np.where(over, RO | CO, 0)).astype(np.uint8)
    return dict(ns=rng.integers(0, 4, n).astype(np.int32), kind=kind,
                t_ms=600_000 + 2_000 * np.arange(n, dtype=np.int64),
                actions=np.asarray(handles, np.int32)[rng.integers(0, len(handles), n)],
                aids=["%032x" % (0xE5 << 100 | seed << 32 | i) for i in range(n)],
                tickets=(7_000 + np.arange(n)).astype(np.int32),
                time_limit_ms=np.array([100, 61_000, 300_000])[rng.integers(0, 3, n)], now_ms=2_000,
                rate_override=np.full(n, BIGLIM, np.int32), conc_override=np.full(n, BIGLIM, np.int32), seq_base=40)


def messages(n, seed=1):
    """The msgs argument (without n_topics and cap) for n items over the three templates of tests/test_gpu_invoke.py."""
    rng = np.random.default_rng(seed)
    return dict(tmpl=np.arange(n, dtype=np.int32) % 3, tids=["tid_%d" % k for k in range(n)],
                tid_start=np.arange(n) + 1_700_000_000_000, flags=rng.integers(0, 8, n).astype(np.uint8),
                contents=['{"p":"%s"}' % ("x" * int(rng.integers(0, 40))) for _ in range(n)])


def identities(seed=3):
    """One identity per (length of A, length of B) pair over PIECE_LENGTHS, diagonal and shifted: 14 identities whose
    pieces are opaque printable bytes of exactly those lengths."""
    rng = np.random.default_rng(seed)

    def piece(m):
        return bytes(rng.integers(0x23, 0x7F, m).astype(np.uint8))      # printable, no '"'

    L = PIECE_LENGTHS
    pairs = [(L[k], L[k]) for k in range(len(L))] + [(L[k], L[(k + 3) % len(L)]) for k in range(len(L))]
    return [(piece(a), piece(b)) for a, b in pairs]


def readable_identities(k=5):
    """Identities as a caller prints them: their events parse as JSON."""
    return [EM.identity_pieces("subject-%d" % i, "23bc46b1-71f6-4ed5-8c54-816aa4f8c5%02d" % i, "space %d" % i)
            for i in range(k)]


def row_share(kind, verdict):
    """Fraction of the items in each of the four rows of the table."""
    rows = np.array([EM.row_of(int(k), int(v)) for k, v in zip(kind, verdict)])
    return [float(np.mean(rows == r)) for r in range(4)]


def random_items(seed, n, n_ident, row=None):
    """n stand-alone items: the four rows dealt evenly (row = r: only that row), counts and timestamps random with
    the extremes mixed in.  Returns the keyword arguments of throttle_events."""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(np.arange(n) % 4) if row is None else np.full(n, row)
    kind = np.where(rows == 1, TRIG, ACT).astype(np.uint8)
    flip = (rows >= 2) & (rng.random(n) < 0.5)                 # a rejected item is an action or a trigger
    kind = np.where(flip, TRIG, kind).astype(np.uint8)
    kind |= (rng.integers(0, 4, n) << 1).astype(np.uint8)      # the override bits do not matter
    verdict = np.where(rows == 2, RATE, np.where(rows == 3, CONC, OK)).astype(np.uint8)
    edge32 = np.array([0, 9, 10, 99, 100, -1, IMAX, IMIN, IMAX - 1], np.int64)

    def counts():
        v = rng.integers(IMIN, IMAX + 1, n)
        small = rng.random(n) < 0.4
        v = np.where(small, rng.integers(0, 2_000, n), v)
        pick = rng.random(n) < 0.3
        return np.where(pick, edge32[rng.integers(0, len(edge32), n)], v).astype(np.int32)

    edge64 = np.array([0, 9, 10, 2**60 - 1, 999_999_999, 1_000_000_000, 10**18 - 1, 10**18], np.int64)
    ts = rng.integers(0, 2**60, n)
    ts = np.where(rng.random(n) < 0.3, edge64[rng.integers(0, len(edge64), n)], ts).astype(np.int64)
    return dict(kind=kind, verdict=verdict, rate_count=counts(), rate_limit=counts(), conc_count=counts(),
                conc_limit=counts(), ts_ms=ts, ident=rng.integers(0, n_ident, n).astype(np.int32))


def model_of(items, pieces, source=SOURCE):
    return EM.throttle_events(items["kind"], items["verdict"], items["rate_count"], items["rate_limit"],
                              items["conc_count"], items["conc_limit"], items["ts_ms"], items["ident"],
                              source.encode(), pieces)
