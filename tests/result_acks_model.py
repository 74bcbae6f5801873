"""Host model of owgs_process_result_acks (include/owgs.h "result-carrying acks"), written from the reference's rules
over the raw text of each message, independently of the device parser:

classify(msg)       the message type and what its `response` is: a Left id (ActivationId.serdes), a Right object inside
                    the accepted subset, or neither; for a Combined message the text of the CompletionMessage with the
                    same id, invoker, isSystemError and transid, which the frozen ack oracle then judges
ResultAckModel      one controller's flow: oracle.AckFlow completes, this class keeps the id -> ticket view that
                    processResult (CLB:235-243) reads, and answers a batch as the device call reports it

The JSON scanner is feeds_model._Scan (spray-json's grammar and the device parser's limits); the subclass below only
adds the raw span of every value and member name.
"""
import re

import numpy as np

import oracle as O
from feeds_model import NONASCII, Num, _Err, _Scan, _Unsup

FAIL, JVM, UNSUPPORTED, RELEASED, HEALTH, NOENTRY, FORCED_NOENTRY, RESULT = range(8)
F_RESULT, F_RIGHT = 8, 16
DUMMY_AID = "0" * 32

_PART = re.compile(r"\A(\w|\w[\w@ .&-]{0,254}[\w@.&-])\Z", re.A)     # EntityName.REGEX, EntityPath.scala:206
_PLAIN = re.compile(rb'\A"[\x20\x21\x23-\x5b\x5d-\x7e]*"\Z')           # printable ASCII without '"' and '\'
_HEX32 = re.compile(rb'\A"[0-9a-f]{32}"\Z')
_LONG = re.compile(rb"\A-?(0|[1-9][0-9]{0,17})\Z")
_INT = re.compile(rb"\A-?(0|[1-9][0-9]{0,8})\Z")
_SEMVER = re.compile(rb'\A"(0|[1-9][0-9]{0,8})\.(0|[1-9][0-9]{0,8})\.(0|[1-9][0-9]{0,8})"\Z')  # SemVer.scala:52
WA_NAMES = ("namespace", "name", "subject", "activationId", "start", "end", "cause", "response", "logs", "version",
            "publish", "annotations", "duration")
WA_REQUIRED = tuple(n for n in WA_NAMES if n not in ("cause", "duration"))


class Node:
    """A scanned value with its raw span [a, b) in the message."""
    __slots__ = ("v", "a", "b")

    def __init__(self, v, a, b):
        self.v, self.a, self.b = v, a, b

    @property
    def kind(self):
        v = self.v
        if isinstance(v, tuple):
            return v[0]
        if isinstance(v, Num):
            return "num"
        if isinstance(v, str):
            return "str"
        return "null" if v is None else "bool"


class _Spans(_Scan):
    """_Scan with every value wrapped in a Node and every object member as (decoded name, raw name, Node)."""

    def value(self, depth):
        a = self.i
        v = super().value(depth)
        return Node(v, a, self.i)

    def obj(self, depth):
        self.i += 1
        self.ws()
        members = []
        if self.at() == 0x7D:
            self.i += 1
            return ("obj", members)
        while True:
            if self.at() != 0x22:
                raise _Err
            ka = self.i
            k = self.string()
            raw = self.b[ka:self.i]
            self.ws()
            if self.at() != 0x3A:
                raise _Err
            self.i += 1
            self.ws()
            members.append((k, raw, self.value(depth)))
            self.ws()
            c = self.at()
            self.i += 1
            if c == 0x7D:
                return ("obj", members)
            if c != 0x2C:
                raise _Err
            self.ws()


def _members(node, names):
    """{name: Node} of an object's members among names, or None: a raw name with an escape, or one of names twice."""
    out = {}
    for _, raw, val in node.v[1]:
        if b"\\" in raw:
            return None
        k = raw[1:-1].decode("latin-1")
        if k in names:
            if k in out:
                return None
            out[k] = val
    return out


def _entity_parts(raw, path):
    if not _PLAIN.match(raw):
        return False
    s = raw[1:-1].decode("ascii")
    parts = [p for p in s.split("/") if p] if path else [s]
    return len(parts) >= 1 and all(_PART.match(p) for p in parts)


def _absent_null_or(node, rx, msg):
    return node is None or node.kind == "null" or bool(rx.match(msg[node.a:node.b]))


def in_subset(node, msg):
    """The accepted subset of a `response` object, rule by rule as include/owgs.h lists it."""
    raw = lambda n: msg[n.a:n.b]  # noqa: E731
    m = _members(node, WA_NAMES)
    if m is None or any(k not in m for k in WA_REQUIRED):
        return False
    if not (_entity_parts(raw(m["namespace"]), True) and _entity_parts(raw(m["name"]), False)):
        return False
    s = raw(m["subject"])
    if not _PLAIN.match(s) or len(s) - 2 < 5 or s[1:2] == b" " or s[-2:-1] == b" ":
        return False
    if not _HEX32.match(raw(m["activationId"])) or not _absent_null_or(m.get("cause"), _HEX32, msg):
        return False
    if not (_LONG.match(raw(m["start"])) and _LONG.match(raw(m["end"]))):
        return False
    if not _absent_null_or(m.get("duration"), _LONG, msg):
        return False
    r = m["response"]
    if r.kind != "obj":
        return False
    rm = _members(r, ("statusCode", "result", "size"))
    if rm is None or "statusCode" not in rm or not _INT.match(raw(rm["statusCode"])):
        return False
    if not _absent_null_or(rm.get("size"), _INT, msg):
        return False
    logs = m["logs"]
    if logs.kind != "arr" or any(e.kind != "str" for e in logs.v[1]):
        return False
    v = raw(m["version"])
    if not _SEMVER.match(v) or v == b'"0.0.0"':
        return False
    if m["publish"].kind != "bool":
        return False
    ann = m["annotations"]
    if ann.kind != "arr":
        return False
    for e in ann.v[1]:
        if e.kind != "obj":
            return False
        em = _members(e, ("key", "value", "init"))
        if em is None or "key" not in em or "value" not in em:
            return False
        k = raw(em["key"])
        if not _PLAIN.match(k) or not k[1:-1].strip(b" "):
            return False
        if "init" in em and em["init"].kind != "bool":
            return False
    return True


def aid_words(raw_hex: bytes):
    return int(raw_hex[:16], 16), int(raw_hex[16:], 16)


def classify(msg: bytes):
    """What owgs_process_result_acks makes of one message before the table is consulted:
    ("plain",)                                  no `response` member: owgs_process_acks' business
    ("fail",) ("jvm",) ("unsup",)               outcomes the response or the grammar decides alone
    ("combined", completion text, hi, lo, right, (off, len))   the response is acceptable; the CompletionMessage text
                                                with the same id / transid / isSystemError / invoker decides the rest
    ("result", hi, lo, right, (off, len))       an accepted ResultMessage"""
    if b"\xef\xbf\xbf" in msg:
        return ("unsup",)
    try:
        root = _Spans(msg).root()
    except _Unsup:
        return ("unsup",)
    except _Err:
        return ("fail",)
    if root.kind != "obj":
        return ("fail",)
    top = {}
    for k, _, val in root.v[1]:  # member names compare after unescaping; the last of duplicates wins
        top[k] = val
    resp = top.get("response")
    if resp is None:
        return ("plain",)
    fail = unsup = right = False
    hi = lo = 0
    if resp.kind == "str":  # Left(ActivationId): Message.scala:231-233, ActivationId.scala:58-95
        s = resp.v
        if any(ord(ch) >= 0x80 for ch in s):
            unsup = True
        elif len(s) != 32 or any(ch not in "0123456789abcdef" for ch in s):
            fail = True
        else:
            hi, lo = aid_words(s.encode())
    elif resp.kind == "obj":  # Right(WhiskActivation): Message.scala:235
        if not in_subset(resp, msg):
            return ("jvm",)
        right = True
        for _, raw, val in resp.v[1]:
            if raw == b'"activationId"':
                hi, lo = aid_words(msg[val.a + 1:val.b - 1])
    else:
        fail = True  # Message.scala:236
    if "transid" not in top:
        fail = True
    span = (resp.a, resp.b - resp.a)
    if "invoker" not in top:  # ResultMessage, jsonFormat2
        return ("fail",) if fail else ("unsup",) if unsup else ("result", hi, lo, right, span)
    # Combined, jsonFormat4: the other three members as the CompletionMessage format reads them
    aid = DUMMY_AID if (fail or unsup) else "%016x%016x" % (hi, lo)
    tid = msg[top["transid"].a:top["transid"].b] if "transid" in top else b"[]"
    parts = [b'"transid":' + tid, b'"activationId":"' + aid.encode() + b'"']
    if "isSystemError" in top:
        parts.append(b'"isSystemError":' + msg[top["isSystemError"].a:top["isSystemError"].b])
    parts.append(b'"invoker":' + msg[top["invoker"].a:top["invoker"].b])
    text = b"{" + b",".join(parts) + b"}"
    if fail or unsup:
        k = int(O.parse_acks([text], 0)[0][0])
        return ("fail",) if (fail or k == O.ACK_FAIL) else ("unsup",)
    return ("combined", text, hi, lo, right, span)


class ResultAckModel:
    """The completion flow of one controller (oracle.AckFlow) with the id -> ticket view processResult reads."""

    def __init__(self, flow):
        self.flow = flow
        self.by_id = {}

    def track(self, aid: str, action: int, ticket: int):
        t, existed = self.flow.track(aid, action, ticket)
        if not existed:
            self.by_id[O.aid_words(aid)] = ticket
        return t, existed

    def forget(self, aid: str):
        """An entry removed by another path (a sweep, complete_activations)."""
        self.by_id.pop(O.aid_words(aid), None)

    def process(self, msgs):
        """(kind, invoker, ticket, flags, aid u64[n, 2], resp_off, resp_len) in array order; invoker is meaningful for
        kind >= RELEASED only (RESULT: -1), and resp_off counts inside the message (add the message's offset)."""
        n = len(msgs)
        kind, fl = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        inv, tk, rlen = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        aid, roff = np.zeros((n, 2), np.uint64), np.zeros(n, np.int64)
        for i, msg in enumerate(msgs):
            c = classify(msg)
            if c[0] in ("fail", "jvm", "unsup"):
                kind[i] = {"fail": FAIL, "jvm": JVM, "unsup": UNSUPPORTED}[c[0]]
                continue
            if c[0] == "result":
                _, hi, lo, right, span = c
                kind[i], inv[i], fl[i] = RESULT, -1, F_RESULT | (F_RIGHT if right else 0)
                tk[i] = self.by_id.get((hi, lo), -1)
                aid[i], roff[i], rlen[i] = (hi, lo), span[0], span[1]
                continue
            text = msg if c[0] == "plain" else c[1]
            k, oi, ot, of = self.flow.process_acks([text])
            kind[i], inv[i], tk[i], fl[i] = k[0], oi[0], ot[0], of[0]
            if k[0] >= RELEASED:
                hi, lo = (int(x) for x in O.parse_acks([text], self.flow.h)[4][0])
                aid[i] = (hi, lo)
                if k[0] == RELEASED:
                    del self.by_id[(hi, lo)]
                if c[0] == "combined":
                    fl[i] |= F_RESULT | (F_RIGHT if c[4] else 0)
                    roff[i], rlen[i] = c[5]
        return kind, inv, tk, fl, aid, roff, rlen
