"""Known-answer vectors for the entitlement throttle gate (owgs_admit_batch): the per-minute rate throttle
(RateThrottler.scala:47-86, "RT") followed, for actions that passed it, by the concurrent throttle
(ActivationThrottler.scala:41-62, "AT"), as EntitlementProvider.checkThrottles chains them (Entitlement.scala:197-202,
354-381, "ENT"), with every limit through calculateIndividualLimit (ENT:97-133).

Every expectation below is written BY HAND from the reference source (not computed by a model):
  - RateInfo.update: roll() -- curMin != lastMin resets the count to 0 -- then incrementAndGet (RT:72-83); a new
    RateInfo starts in the minute it is created in (RT:61); TimedRateLimit.ok = count <= allowed (AT:64-68)
  - ConcurrentRateLimit.ok = count < allowed (AT:58-62); only evaluated when the rate check passed (ENT:197-202) and
    never for triggers (ENT:378)
  - dilateLimit = Math.ceil(limit.toDouble * (clusterSize > 1 ? 1.2 : 1)).toInt (ENT:97-99), then
    0 if 0 else (dilated / clusterSize).max(1) (ENT:123-133)
The two RateThrottleTests cases (RateThrottleTests.scala:46-65, "T-RT") build RateThrottler with a raw limit function;
here the same numbers go in as system defaults / overrides with cluster size 1, where calculateIndividualLimit is the
identity for limits >= 0.

Item = [namespace index, kind, t_ms, rate override, concurrent override]; kind bit 0 trigger, bit 1 rate override
present, bit 2 concurrent override present.  Verdict: OK 0, RATE 1, CONCURRENT 2.  conc_count is -1 where the
concurrent check did not run.  `active` = activations in flight per namespace before the case; `final` = the rate
records [lastMin, count] per namespace afterwards (null: absent).
Run `python tests/golden/make_admit_golden.py` to regenerate tests/golden/admit_vectors.json.
"""
import json
import os

OK, RATE, CONC = 0, 1, 2
A, T, RO, CO = 0, 1, 2, 4
T0 = 1700000000123          # 20.123 s into minute 28333333
M = 28333333
MIN = 60000
IMAX = 2**31 - 1

CASES = []


def case(name, cite, cluster, limits, active, batches, final):
    CASES.append({"name": name, "cite": cite, "cluster": cluster, "limits": limits, "active": active,
                  "batches": batches, "final": final})


def b(items, verdict, rate_count, rate_limit, conc_count, conc_limit):
    assert len(items) == len(verdict) == len(rate_count) == len(rate_limit) == len(conc_count) == len(conc_limit)
    return {"items": items, "verdict": verdict, "rate_count": rate_count, "rate_limit": rate_limit,
            "conc_count": conc_count, "conc_limit": conc_limit}


# T-RT:47 -- limit 0: the first check is charged (count 1) and rejected
case("limit 0 rejects the first check", "T-RT:47", 1, [0, 60, 30], [0], [
    b([[0, A, T0, 0, 0]], [RATE], [1], [0], [-1], [30]),
], {"invoke": [[M, 1]], "fire": [None]})

# T-RT:48-53 -- limit 1: ok, reject, reject; one minute later the count restarts
case("limit 1: ok, reject, reject, ok a minute later", "T-RT:48-53", 1, [1, 60, 30], [0], [
    b([[0, A, T0, 0, 0], [0, A, T0 + 1, 0, 0], [0, A, T0 + 2, 0, 0]], [OK, RATE, RATE], [1, 2, 3], [1, 1, 1],
      [0, -1, -1], [30, 30, 30]),
    b([[0, A, T0 + MIN, 0, 0]], [OK], [1], [1], [0], [30]),
], {"invoke": [[M + 1, 1]], "fire": [None]})

# T-RT:56-65 -- default 1, the identity's own limit 5: five pass, the sixth does not.  Nothing is tracked in between,
# so the concurrent count grows only by the batch's own admitted actions.
case("default 1 with override 5", "T-RT:56-65", 1, [1, 60, 30], [0], [
    b([[0, A | RO, T0 + k, 5, 0] for k in range(6)], [OK] * 5 + [RATE], [1, 2, 3, 4, 5, 6], [5] * 6,
      [0, 1, 2, 3, 4, -1], [30] * 6),
], {"invoke": [[M, 6]], "fire": [None]})

# ENT:97-133 -- the limit table: both overrides = l, one namespace per l so that every count is 1 / 0.
#   cs = 1: no overcommit, l / 1; -5 -> max(-5, 1) = 1
#   cs = 2: ceil(1.2 l) = 0, 2, 3, 4, 6, 36, 72, 2576980377 -> saturates at 2^31-1, -6; halved, at least 1
#   cs = 3, 8: the same dilated values divided by 3 and by 8
LIMS = [0, 1, 2, 3, 5, 30, 60, IMAX, -5]
TABLE = {
    1: [0, 1, 2, 3, 5, 30, 60, IMAX, 1],
    2: [0, 1, 1, 2, 3, 18, 36, 1073741823, 1],
    3: [0, 1, 1, 1, 2, 12, 24, 715827882, 1],
    8: [0, 1, 1, 1, 1, 4, 9, 268435455, 1],
}
for cs, want in TABLE.items():
    # limit 0 rejects at the rate check (count 1 > 0); everything else passes both (1 <= limit, 0 < limit)
    case(f"limit table, cluster size {cs}", "ENT:97-133", cs, [60, 60, 30], [0] * len(LIMS), [
        b([[k, A | RO | CO, T0, l, l] for k, l in enumerate(LIMS)], [RATE] + [OK] * 8, [1] * 9, want,
          [-1] + [0] * 8, want),
    ], {"invoke": [[M, 1]] * 9, "fire": [None] * 9})

# RT:77-83 -- the test is !=, not >: a clock that steps back one minute resets, and so does the step forward again
case("clock stepping back resets", "RT:77-83", 1, [60, 60, 30], [0], [
    b([[0, A, T0, 0, 0], [0, A, T0 + 5, 0, 0], [0, A, T0 - MIN, 0, 0], [0, A, T0 - MIN + 9, 0, 0], [0, A, T0, 0, 0]],
      [OK] * 5, [1, 2, 1, 2, 1], [60] * 5, [0, 1, 2, 3, 4], [30] * 5),
], {"invoke": [[M, 1]], "fire": [None]})

# ENT:354-381 -- actions and triggers of one namespace interleaved: two independent counts (limit 3 each); triggers
# have no concurrent throttle and take no concurrent room: with 28 in flight the actions count 28, 29, 30
case("interleaved actions and triggers", "ENT:354-381", 1, [3, 3, 30], [28], [
    b([[0, k, T0 + i, 0, 0] for i, k in enumerate([A, T, A, T, T, A, T, T])],
      [OK, OK, OK, OK, OK, CONC, RATE, RATE], [1, 1, 2, 2, 3, 3, 4, 5], [3] * 8,
      [28, -1, 29, -1, -1, 30, -1, -1], [30, 0, 30, 0, 0, 30, 0, 0]),
], {"invoke": [[M, 3]], "fire": [[M, 5]]})

# ENT:197-202 -- the concurrent check runs only after a passed rate check: the rejected second action (its own limit 1,
# count 2) takes no concurrent room, so the fourth still sees 29 and only the fifth reaches 30
case("a rate-rejected action takes no concurrent room", "ENT:197-202", 1, [60, 60, 30], [27], [
    b([[0, A | RO, T0 + i, l, 0] for i, l in enumerate([10, 1, 10, 10, 10])], [OK, RATE, OK, OK, CONC],
      [1, 2, 3, 4, 5], [10, 1, 10, 10, 10], [27, -1, 28, 29, 30], [30] * 5),
], {"invoke": [[M, 5]], "fire": [None]})


def main():
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "admit_vectors.json")
    with open(out, "w") as f:
        json.dump(CASES, f, indent=1)
    print(f"wrote {len(CASES)} cases to {out}")


if __name__ == "__main__":
    main()
