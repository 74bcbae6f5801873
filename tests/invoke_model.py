"""owgs_invoke_activations as a model: the entitlement throttle gate, then publish over what it admitted.

What it composes:
  Entitlement.scala:197-202, 354-381   the gate: tests/test_admit.py's admit_model over the model's own rate records
                                       and the in-flight books of the publish model (activationsPerNamespace)
  PrimitiveActions.scala:152-185       only an admitted action is published
  SCPB:257-317                         publish: tests/publish_model.py's PublishModel over the sub-batch of admitted
                                       actions, in array order; the k-th admitted action draws its overload fallback
                                       with seq[adm[k]], or seq_base + k
Every other item gets (NOT_PUBLISHED, 0, -1, 0).  The summary words are counted here.  Nothing here reads a GPU output.
"""
import numpy as np

from publish_model import PublishModel
from test_admit import admit_model

NOT_PUBLISHED = -3
OK, RATE, CONC = 0, 1, 2
TRIG = 1


class InvokeModel:
    def __init__(self, publish_model: PublishModel, limits=(60, 60, 30), cluster=1):
        self.pm = publish_model
        self.limits = tuple(limits)      # invokes / fires per minute, concurrent invocations
        self.cluster = cluster
        self.rate = {}                   # (handle, which) -> [lastMin, count]

    def invoke(self, ns, kind, t_ms, actions, aids, tickets, time_limit_ms, now_ms, rate_override=None,
               conc_override=None, seq=None, seq_base=0):
        """The nine arrays and the summary (a list of 16) of one call; summary[12] (the waits) is left 0."""
        n = len(ns)
        gate = admit_model(self.rate, self.limits, self.cluster, self.pm.t.active, ns, kind, t_ms, rate_override,
                           conc_override)
        verdict = gate[0]
        adm = [i for i in range(n) if not int(kind[i]) & TRIG and verdict[i] == OK]
        inv = np.full(n, NOT_PUBLISHED, np.int32)
        fl = np.zeros(n, np.uint8)
        tk = np.full(n, -1, np.int32)
        ex = np.zeros(n, np.uint8)
        sub = self.pm.publish([int(actions[i]) for i in adm], [aids[i] for i in adm], [int(tickets[i]) for i in adm],
                              [int(time_limit_ms[i]) for i in adm], now_ms, [int(ns[i]) for i in adm],
                              None if seq is None else [int(seq[i]) for i in adm], seq_base)
        for k, i in enumerate(adm):
            inv[i], fl[i], tk[i], ex[i] = sub[0][k], sub[1][k], sub[2][k], sub[3][k]
        s = list(sub[4]) + [0] * 8
        s[8] = len(adm)
        s[9] = int(np.sum(verdict == RATE))
        s[10] = int(np.sum(verdict == CONC))
        s[11] = sum(1 for i in range(n) if int(kind[i]) & TRIG and verdict[i] == OK)
        return gate + (inv, fl, tk, ex, s)

    def rate_records(self, handles, which):
        """(lastMin, count) as owgs_rate_state reads them: (INT64_MIN, 0) for an absent record."""
        r = [self.rate.get((int(h), which)) for h in handles]
        return [x[0] if x else -2**63 for x in r], [x[1] if x else 0 for x in r]
