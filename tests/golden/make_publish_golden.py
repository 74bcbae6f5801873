"""Writes publish_vectors.json: hand-derived expectations for `publish` over a drained batch.

Every number below was worked out by hand from the reference, not produced by any implementation:
  ShardingContainerPoolBalancer.scala:292-316  only an activation with an invoker reaches setupActivation
  CommonLoadBalancer.scala:116-166             setupActivation: books first (:121-127), then getOrElseUpdate (:148)
  CommonLoadBalancer.scala:103-105             timeout = max(limit, 60000) * 2 + 60000 with the default settings
The decisions are part of the input (they are the scheduler's business); the vectors pin what follows from them.

Run: python tests/golden/make_publish_golden.py
"""
import json
import os

A, B, C, X = ("%032x" % v for v in (0xA1, 0xB2, 0xC3, 0xD4 << 64 | 7))

CASES = [{
    "name": "placed, thrown, duplicates of a placed / a thrown / a pre-existing id, none",
    # handle -> (memory MB, blackbox)
    "actions": {"0": [256, False], "1": [128, True], "2": [256, False]},
    # tracked by an earlier call at now = 500: limit 100 -> 500 + 60000 * 2 + 60000 = 180500
    "before": [{"aid": X, "action": 0, "ticket": 90, "invoker": 1, "limit": 100, "now": 500, "ns": 5}],
    "now": 1000,
    "items": [
        # 0: placed on invoker 2, creates A: 1000 + 60000 * 2 + 60000 = 181000
        {"aid": A, "action": 0, "decision": 2, "flag": 0, "ticket": 10, "limit": 100, "ns": 5},
        # 1: schedule throws: no table access, no counter
        {"aid": B, "action": 2, "decision": -2, "flag": 0, "ticket": 11, "limit": 100, "ns": 5},
        # 2: a duplicate of item 0 (placed): A's ticket, counted by the books, arms nothing; a managed overload
        {"aid": A, "action": 0, "decision": 3, "flag": 1, "ticket": 12, "limit": 300000, "ns": 6},
        # 3: the id of item 1, which left no entry: this item creates it: 1000 + 300000 * 2 + 60000 = 661000
        {"aid": B, "action": 1, "decision": 0, "flag": 1, "ticket": 13, "limit": 300000, "ns": 6},
        # 4: a duplicate of the pre-existing X: its ticket 90; counted, no namespace
        {"aid": X, "action": 0, "decision": 1, "flag": 0, "ticket": 14, "limit": 100, "ns": -1},
        # 5: None: nothing
        {"aid": C, "action": 1, "decision": -1, "flag": 0, "ticket": 15, "limit": 100, "ns": 6},
    ],
    "ticket": [10, -1, 10, 13, 90, -1],
    "existed": [0, 0, 1, 0, 1, 0],
    # placed 0, 2, 3, 4; created A and B; overloads: item 2 managed, item 3 blackbox; one None; one throw; 2 stages
    "summary": [4, 2, 1, 1, 1, 1, 2, 0],
    "live": 3,
    # namespace 5: X + item 0; namespace 6: items 2 and 3 (the None item 5 is not counted)
    "active": {"5": 2, "6": 2},
    # total: X + 4 placed; managed MB: X, items 0, 2, 4 = 4 * 256; blackbox MB: item 3 = 128
    "totals": [5, 1024, 128],
    "next_deadline": 180500,
    # a sweep at 2^59 fires ascending (deadline, arm order): the entry's invoker is its creator's decision
    "armed": [[X, 180500, 1], [A, 181000, 2], [B, 661000, 0]],
}]

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "publish_vectors.json")
    with open(path, "w") as f:
        json.dump({"cases": CASES}, f, indent=1)
        f.write("\n")
    print(path)
