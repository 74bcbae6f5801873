"""The completion-ack timeout of CommonLoadBalancer as a model over the CPU oracle.

What it restates (CommonLoadBalancer.scala):
  :103-105  calculateCompletionAckTimeout = max(timeLimit, TimeLimit.STD_DURATION) * timeoutFactor + timeoutAddon
  :148-152  the timer is armed inside activationSlots.getOrElseUpdate: only the message that creates the entry arms one
  :289      a regular ack cancels it
  :150-152  a fired timer runs processCompletion(aid, tid, forced = true, isSystemError = false, invoker = entry.invoker)
  :121-127, :280-284  the in-flight books, counted per message and subtracted per removed entry
Which track creates an entry and which completion removes one comes from oracle.AckFlow; the slot state is the
oracle's BalancerState.  Timers due together fire in ascending (deadline, arm order) -- arm order = creation order --
which is this project's definition (the reference pins none).  Nothing here reads a GPU output.
"""
from collections import defaultdict

import numpy as np

import oracle as O

NONE = -1
NO_DEADLINE = 2**63 - 1


class TimeoutModel:
    def __init__(self, flow: O.AckFlow, actions, std_ms=60000, factor=2, addon_ms=60000):
        self.flow = flow
        self.actions = actions           # by action handle: objects with mem_mb / blackbox
        self.std, self.factor, self.addon = std_ms, factor, addon_ms
        self.armed = {}                  # aid -> (deadline, arm sequence, entry invoker)
        self.seq = 0
        self.entry = {}                  # aid of a live entry -> (ticket, namespace, action) of its first tracker
        self.active = defaultdict(int)   # activationsPerNamespace
        self.total = 0                   # totalActivations
        self.mem = [0, 0]                # totalManagedActivationMemory, totalBlackBoxActivationMemory

    def set_ack_timeout(self, std_ms, factor, addon_ms):
        self.std, self.factor, self.addon = std_ms, factor, addon_ms

    def deadline(self, time_limit_ms, now_ms):
        return now_ms + max(time_limit_ms, self.std) * self.factor + self.addon    # CLB:103-105

    # ------------------------------------------------------------------------------------------------ setupActivation
    def track(self, aid, action, ticket, invoker=None, time_limit_ms=None, now_ms=None, ns=NONE):
        """One message; invoker None = tracked through an untimed call (no timer).  (ticket, existed)."""
        a = self.actions[action]
        self.total += 1                                      # CLB:121
        self.mem[1 if a.blackbox else 0] += a.mem_mb         # CLB:122-125
        if ns != NONE:
            self.active[ns] += 1                             # CLB:127
        t, existed = self.flow.track(aid, action, ticket)
        if not existed:                                      # the by-name block of getOrElseUpdate runs (CLB:148-152)
            self.entry[aid] = (ticket, ns, action)
            if invoker is not None:
                self.armed[aid] = (self.deadline(time_limit_ms, now_ms), self.seq, invoker)
            self.seq += 1
        return t, existed

    def _removed(self, aid):
        _, ns, action = self.entry.pop(aid)                  # Some(entry), CLB:279
        a = self.actions[action]
        self.total -= 1                                      # CLB:280
        self.mem[1 if a.blackbox else 0] -= a.mem_mb         # CLB:281-283
        if ns != NONE:
            self.active[ns] -= 1                             # CLB:284
        self.armed.pop(aid, None)                            # the entry's timer goes with it (CLB:289)

    # ------------------------------------------------------------------------------------------------ completions
    def complete(self, aid, invoker, forced=False, health=False):
        hi, lo = O.aid_words(aid)
        out = self.flow.complete(hi, lo, invoker, forced, health)
        if out[0] == O.OUT_RELEASED:
            self._removed(aid)
        return out

    def process_acks(self, msgs):
        kind, inst, tick, fl = self.flow.process_acks(msgs)
        words = O.parse_acks(msgs, self.flow.h)[4]
        for i in np.nonzero(kind == O.OUT_RELEASED)[0]:
            self._removed("%016x%016x" % (int(words[i][0]), int(words[i][1])))
        return kind, inst, tick, fl

    # ------------------------------------------------------------------------------------------------ the timers
    def due(self, now_ms):
        d = [(dl, seq, aid) for aid, (dl, seq, _) in self.armed.items() if dl <= now_ms]
        d.sort()
        return d

    def expire(self, now_ms, cap=None):
        """(list of (aid, ticket, invoker, deadline, flags), remaining)."""
        d = self.due(now_ms)
        take = d if cap is None else d[:cap]
        out = []
        for dl, _, aid in take:
            inv = self.armed[aid][2]
            o, t, _, rf = self.complete(aid, inv, forced=True)
            assert o == O.OUT_RELEASED                       # an armed timer always has its entry
            out.append((aid, t, inv, dl, O._rel_bits(rf) << 1))
        return out, len(d) - len(take)

    def next_deadline(self):
        return min((v[0] for v in self.armed.values()), default=NO_DEADLINE)

    def live(self):
        return self.flow.live()

    def books(self, handles):
        return [self.active[int(h)] for h in handles], (self.total, self.mem[0], self.mem[1])
