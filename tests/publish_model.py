"""ShardingContainerPoolBalancer.publish for a drained batch as a model over the CPU oracle.

What it restates:
  SCPB:260-290  the decision: oracle.BalancerState.publish (an invoker id, -1 for None, -2 where schedule throws)
  SCPB:292-304  only an activation that got an invoker reaches setupActivation
  CLB:116-166   setupActivation: the books (CLB:121-127, before getOrElseUpdate), the entry of the first tracker with
                the chosen invoker, and its completion-ack timer -- tests/timeout_model.py's TimeoutModel.track
  SCPB:305-316  an activation without an invoker touches nothing: it cannot be the first tracker of its id
The summary words are counted here in Python.  Nothing here reads a GPU output.
"""
import numpy as np

import oracle as O
from timeout_model import TimeoutModel

NONE, THROW_INDEX = -1, -2


class PublishModel:
    def __init__(self, state: O.BalancerState, actions, health_start_ms=0, **timeouts):
        """actions: by action handle, objects with mem_mb / blackbox."""
        self.st = state
        self.actions = actions
        self.t = TimeoutModel(O.AckFlow(state, health_start_ms), actions, **timeouts)

    def setup(self, decisions, flags, actions, aids, tickets, time_limit_ms, now_ms, ns=None):
        """Steps 2 of every item in array order, given the decisions: (ticket, existed, summary)."""
        n = len(decisions)
        ticket = np.full(n, -1, np.int32)
        existed = np.zeros(n, np.uint8)
        s = [0] * 8
        for i in range(n):
            d = int(decisions[i])
            if d == NONE:
                s[4] += 1                                    # SCPB:305-316
                continue
            if d == THROW_INDEX:
                s[5] += 1                                    # schedule threw: publish never reaches setupActivation
                continue
            s[0] += 1
            a = int(actions[i])
            if int(flags[i]) & 1:                            # SCPB:277-286
                s[3 if self.actions[a].blackbox else 2] += 1
            t, x = self.t.track(aids[i], a, int(tickets[i]), d, int(time_limit_ms[i]), now_ms,
                                NONE if ns is None else int(ns[i]))
            ticket[i], existed[i] = t, x
            s[1] += 0 if x else 1
        s[6] = 2
        return ticket, existed, s

    def publish(self, actions, aids, tickets, time_limit_ms, now_ms, ns=None, seq=None, seq_base=0):
        """(invoker, flags, ticket, existed, summary) of one owgs_publish_activations call."""
        n = len(actions)
        inv = np.zeros(n, np.int32)
        fl = np.zeros(n, np.uint8)
        for i in range(n):                                   # step 1 never reads what step 2 writes
            inv[i], fl[i] = self.st.publish(int(actions[i]), int(seq[i]) if seq is not None else seq_base + i)
        ticket, existed, s = self.setup(inv, fl, actions, aids, tickets, time_limit_ms, now_ms, ns)
        return inv, fl, ticket, existed, s

    def armed_order(self):
        """[(aid, deadline, entry invoker)] in the order a sweep fires them: ascending (deadline, arm order)."""
        return [(aid, d, inv) for d, _, aid, inv in sorted((d, q, aid, inv) for aid, (d, q, inv) in
                                                          self.t.armed.items())]
