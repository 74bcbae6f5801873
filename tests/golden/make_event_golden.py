"""Known-answer vectors for the throttle gate's user events and rejection texts (owgs_throttle_events).

Every expected string below is written BY HAND from the reference source (not computed by a model):
  - checkThrottleOverload (Entitlement.scala:383-420, "ENT"): an admitted action invoke sends
    Metric("ConcurrentInvocations", count + 1) -- `count` is an Int, the sum wraps before Metric widens it to Long; a
    trigger sends nothing (`case _ => // ignore`); a rejected invoke or fire sends Metric(limit.limitName, 1) and fails
    with limit.errorMsg
  - limitName / errorMsg (ActivationThrottler.scala:58-67, "AT"; ErrorResponse.scala:70-75, "ERR"):
    "ConcurrentRateLimit", s"Too many concurrent requests in flight (count: $count, allowed: $allowed)."
    "TimedRateLimit",      s"Too many requests in the last minute (count: $count, allowed: $allowed)."
  - EventMessage.serialize = compactPrint (Message.scala:404-418, "MSG"), members in the HashMap's order: body,
    eventType, source, subject, timestamp, userId, namespace -- the order of docs/metrics.md:353-364 ("DOC")
Case = one item: the event source S and the identity's pieces A, B as the caller prints them; kind bit 0 = trigger;
verdict OK 0, RATE 1, CONCURRENT 2; the gate's four numbers; ts.  `event` / `text` are "" where the item has none.
`doc_example` holds only the values of the reference's own example (DOC).
Run `python tests/golden/make_event_golden.py` to regenerate tests/golden/event_vectors.json.
"""
import json
import os

OK, RATE, CONC = 0, 1, 2
ACT, TRIG = 0, 1
S0 = '"controller0"'
A0 = '"subject":"guest"'
B0 = '"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"'
IMIN = -2**31
IMAX = 2**31 - 1

CASES = []


def case(name, cite, kind, verdict, rate_count, rate_limit, conc_count, conc_limit, ts, event, text, s=S0, a=A0, b=B0):
    CASES.append({"name": name, "cite": cite, "source": s, "a": a, "b": b, "kind": kind, "verdict": verdict,
                  "rate_count": rate_count, "rate_limit": rate_limit, "conc_count": conc_count,
                  "conc_limit": conc_limit, "ts": ts, "event": event, "text": text})


# ---- one case per row of the table
case("admitted action: ConcurrentInvocations, count + 1", "ENT:389-391", ACT, OK, 1, 60, 0, 30, 1524476104419,
     '{"body":{"metricName":"ConcurrentInvocations","metricValue":1},"eventType":"Metric","source":"controller0",'
     '"subject":"guest","timestamp":1524476104419,"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"}',
     "")
case("admitted trigger: nothing", "ENT:392 (case _ => // ignore)", TRIG, OK, 3, 60, -1, 0, 1524476104419, "", "")
case("rate-rejected action: TimedRateLimit", "ENT:405-415, AT:64-67, ERR:70-72", ACT, RATE, 61, 60, -1, 30, 1524476104420,
     '{"body":{"metricName":"TimedRateLimit","metricValue":1},"eventType":"Metric","source":"controller0",'
     '"subject":"guest","timestamp":1524476104420,"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"}',
     "Too many requests in the last minute (count: 61, allowed: 60).")
case("rate-rejected trigger: TimedRateLimit as well", "ENT:405-415", TRIG, RATE, 7, 6, -1, 0, 1524476104421,
     '{"body":{"metricName":"TimedRateLimit","metricValue":1},"eventType":"Metric","source":"controller0",'
     '"subject":"guest","timestamp":1524476104421,"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"}',
     "Too many requests in the last minute (count: 7, allowed: 6).")
case("concurrent-rejected action: ConcurrentRateLimit", "ENT:405-415, AT:58-62, ERR:73-75", ACT, CONC, 5, 60, 30, 30,
     1524476104422,
     '{"body":{"metricName":"ConcurrentRateLimit","metricValue":1},"eventType":"Metric","source":"controller0",'
     '"subject":"guest","timestamp":1524476104422,"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"}',
     "Too many concurrent requests in flight (count: 30, allowed: 30).")

# ---- the wrapping value: Int.MaxValue + 1 on an Int, then widened
case("count + 1 wraps on an Int", "ENT:389-391", ACT, OK, 1, 60, IMAX, IMAX, 5,
     '{"body":{"metricName":"ConcurrentInvocations","metricValue":-2147483648},"eventType":"Metric",'
     '"source":"controller0","subject":"guest","timestamp":5,'
     '"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"}', "")
case("count -1 gives value 0", "ENT:389-391", ACT, OK, 1, 60, -1, 30, 5,
     '{"body":{"metricName":"ConcurrentInvocations","metricValue":0},"eventType":"Metric",'
     '"source":"controller0","subject":"guest","timestamp":5,'
     '"userId":"23bc46b1-71f6-4ed5-8c54-816aa4f8c502","namespace":"guest"}', "")

# ---- timestamps 0, 9, 10, 2^60 - 1 (short pieces, so the strings stay readable)
for ts_, txt in ((0, "0"), (9, "9"), (10, "10"), (2**60 - 1, "1152921504606846975")):
    case(f"timestamp {txt}", "MSG:404-418", ACT, OK, 1, 60, 8, 30, ts_,
         '{"body":{"metricName":"ConcurrentInvocations","metricValue":9},"eventType":"Metric","source":"c",'
         '"subject":"s","timestamp":' + txt + ',"userId":"u","namespace":"n"}', "",
         s='"c"', a='"subject":"s"', b='"userId":"u","namespace":"n"')
case("a negative timestamp prints its sign", "MSG:404-418", ACT, OK, 1, 60, 9, 30, -1,
     '{"body":{"metricName":"ConcurrentInvocations","metricValue":10},"eventType":"Metric","source":"c",'
     '"subject":"s","timestamp":-1,"userId":"u","namespace":"n"}', "",
     s='"c"', a='"subject":"s"', b='"userId":"u","namespace":"n"')

# ---- counts 0, 9, 10, 99, 100 and Int.MinValue in the texts
EV_T = ('{"body":{"metricName":"TimedRateLimit","metricValue":1},"eventType":"Metric","source":"c",'
        '"subject":"s","timestamp":7,"userId":"u","namespace":"n"}')
EV_C = ('{"body":{"metricName":"ConcurrentRateLimit","metricValue":1},"eventType":"Metric","source":"c",'
        '"subject":"s","timestamp":7,"userId":"u","namespace":"n"}')
SHORT = dict(s='"c"', a='"subject":"s"', b='"userId":"u","namespace":"n"')
case("rate text 9 / 0", "ERR:70-72", ACT, RATE, 9, 0, -1, 30, 7, EV_T,
     "Too many requests in the last minute (count: 9, allowed: 0).", **SHORT)
case("rate text 10 / 9", "ERR:70-72", ACT, RATE, 10, 9, -1, 30, 7, EV_T,
     "Too many requests in the last minute (count: 10, allowed: 9).", **SHORT)
case("rate text 100 / 99", "ERR:70-72", TRIG, RATE, 100, 99, -1, 0, 7, EV_T,
     "Too many requests in the last minute (count: 100, allowed: 99).", **SHORT)
case("rate text with a wrapped count", "ERR:70-72", ACT, RATE, IMIN, IMAX, -1, 30, 7, EV_T,
     "Too many requests in the last minute (count: -2147483648, allowed: 2147483647).", **SHORT)
case("concurrent text 0 / 0", "ERR:73-75", ACT, CONC, 1, 60, 0, 0, 7, EV_C,
     "Too many concurrent requests in flight (count: 0, allowed: 0).", **SHORT)
case("concurrent text 10 / 9", "ERR:73-75", ACT, CONC, 1, 60, 10, 9, 7, EV_C,
     "Too many concurrent requests in flight (count: 10, allowed: 9).", **SHORT)
case("concurrent text 100 / 99", "ERR:73-75", ACT, CONC, 1, 60, 100, 99, 7, EV_C,
     "Too many concurrent requests in flight (count: 100, allowed: 99).", **SHORT)
case("concurrent text with extreme values", "ERR:73-75", ACT, CONC, 1, 60, IMIN, IMIN, 7, EV_C,
     "Too many concurrent requests in flight (count: -2147483648, allowed: -2147483648).", **SHORT)

# ---- empty pieces: the bytes are those of the format, whatever the pieces hold
case("empty source and pieces", "MSG:404-418", ACT, OK, 1, 60, 41, 60, 12,
     '{"body":{"metricName":"ConcurrentInvocations","metricValue":42},"eventType":"Metric","source":,,"timestamp":12,}',
     "", s="", a="", b="")
case("empty piece A only", "MSG:404-418", ACT, CONC, 1, 60, 3, 3, 12,
     '{"body":{"metricName":"ConcurrentRateLimit","metricValue":1},"eventType":"Metric","source":"c",,"timestamp":12,'
     '"userId":"u","namespace":"n"}',
     "Too many concurrent requests in flight (count: 3, allowed: 3).", s='"c"', a="", b='"userId":"u","namespace":"n"')

# docs/metrics.md:353-364 -- the values of the reference's example, nothing else
DOC_EXAMPLE = {
    "members": ["body", "eventType", "source", "subject", "timestamp", "userId", "namespace"],
    "body_members": ["metricName", "metricValue"],
    "metricName": "ConcurrentInvocations", "metricValue": 1, "eventType": "Metric", "source": "controller0",
    "subject": "guest", "timestamp": 1524476104419, "userId": "23bc46b1-71f6-4ed5-8c54-816aa4f8c502",
    "namespace": "guest",
}


def main():
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_vectors.json")
    with open(out, "w") as f:
        json.dump({"cases": CASES, "doc_example": DOC_EXAMPLE}, f, indent=1)
    print(f"wrote {len(CASES)} cases to {out}")


if __name__ == "__main__":
    main()
