"""The throttle gate's user events and rejection texts as a model (owgs_throttle_events).

Written from the reference's Scala sources, not from the kernels:
  Entitlement.scala:383-420            checkThrottleOverload: for an admitted action invoke
                                       Metric("ConcurrentInvocations", count + 1) -- `count` is an Int, so the sum wraps
                                       before Metric widens it to Long; a trigger sends nothing (`case _ => // ignore`);
                                       a rejected request sends Metric(limit.limitName, 1) and fails with limit.errorMsg
  RateThrottler.scala / ActivationThrottler.scala:58-67
                                       limitName "TimedRateLimit" / "ConcurrentRateLimit"; errorMsg
                                       Messages.tooManyRequests(count, allowed) / tooManyConcurrentRequests(count, allowed)
  ErrorResponse.scala:70-75            the two texts
  Message.scala:404-418                EventMessage(source, body, subject, namespace, userId, eventType, timestamp),
                                       jsonFormat7, serialize = compactPrint
Member order: spray-json 1.3.5's JsObject(fields: _*) is Map(fields: _*); seven members make a Scala 2.12 immutable
HashMap, iterated in trie order.  hash_order() below computes it (String.hashCode, HashMap.improve, 5 bits per level
from the low end); the two-member body is a Map2 and keeps insertion order.
Nothing here reads a GPU output.
"""
OK, RATE, CONC = 0, 1, 2
TRIG = 1

# include/owgs.h: OWGS_EVENT_MAX_FIXED and OWGS_REJECT_TEXT_MAX are derived there from these literals
EVENT_LITERALS = '{"body":{"metricName":"","metricValue":},"eventType":"Metric","source":,,"timestamp":,}'
NAMES = ("ConcurrentInvocations", "TimedRateLimit", "ConcurrentRateLimit")
TEXT_RATE = "Too many requests in the last minute (count: %d, allowed: %d)."
TEXT_CONC = "Too many concurrent requests in flight (count: %d, allowed: %d)."


def _i32(x):
    return (int(x) + 2**31) % 2**32 - 2**31


def java_hash(s: str) -> int:
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return h


def improve(hc: int) -> int:
    """scala.collection.immutable.HashMap.improve (2.12): on 32-bit ints with wrapping, >>> unsigned."""
    h = (hc + (~(hc << 9) & 0xFFFFFFFF)) & 0xFFFFFFFF
    h ^= h >> 14
    h = (h + (h << 4)) & 0xFFFFFFFF
    return h ^ (h >> 10)


def hash_order(names):
    """Iteration order of an immutable.HashMap (a HashTrieMap) holding `names`: children by the 5-bit index of the
    improved hash, level by level from the low end."""
    def walk(items, level):
        if len(items) == 1:
            return [items[0][0]]
        buckets = {}
        for name, h in items:
            buckets.setdefault((h >> level) & 31, []).append((name, h))
        out = []
        for k in sorted(buckets):
            out += walk(buckets[k], level + 5)
        return out
    return walk([(n, improve(java_hash(n))) for n in names], 0)


EVENT_MEMBERS = ["source", "body", "subject", "namespace", "userId", "eventType", "timestamp"]   # jsonFormat7's order


def item_class(kind: int, verdict: int):
    """None, or the index into NAMES of the item's metric."""
    if verdict == RATE:
        return 1
    if verdict == CONC:
        return 2
    return None if kind & TRIG else 0


def event(kind, verdict, conc_count, ts, source: bytes, a: bytes, b: bytes) -> bytes:
    cls = item_class(int(kind), int(verdict))
    if cls is None:
        return b""
    value = _i32(int(conc_count) + 1) if cls == 0 else 1
    return (b'{"body":{"metricName":"%s","metricValue":%d},"eventType":"Metric","source":%s,%s,"timestamp":%d,%s}'
            % (NAMES[cls].encode(), value, source, a, int(ts), b))


def text(kind, verdict, rate_count, rate_limit, conc_count, conc_limit) -> bytes:
    if verdict == RATE:
        return (TEXT_RATE % (int(rate_count), int(rate_limit))).encode()
    if verdict == CONC:
        return (TEXT_CONC % (int(conc_count), int(conc_limit))).encode()
    return b""


def throttle_events(kind, verdict, rate_count, rate_limit, conc_count, conc_limit, ts, ident, source, pieces):
    """(events, texts): two lists of bytes by item.  pieces[id] = (A, B)."""
    ev, tx = [], []
    for i in range(len(kind)):
        a, b = pieces[int(ident[i])]
        ev.append(event(kind[i], verdict[i], conc_count[i], ts[i], source, a, b))
        tx.append(text(int(kind[i]), int(verdict[i]), rate_count[i], rate_limit[i], conc_count[i], conc_limit[i]))
    return ev, tx


def row_of(kind, verdict) -> int:
    """Row of the table in include/owgs.h: 0 admitted action, 1 admitted trigger, 2 rate-rejected, 3 concurrent-rejected."""
    return 2 if verdict == RATE else 3 if verdict == CONC else 1 if kind & TRIG else 0


def identity_pieces(subject: str, user_id: str, namespace: str):
    """The two pieces as a caller prints them (ASCII without characters that need escaping)."""
    return (b'"subject":"%s"' % subject.encode(), b'"userId":"%s","namespace":"%s"' % (user_id.encode(), namespace.encode()))
