"""Host model of the supervision feeds (include/owgs.h "supervision feeds"), written from the reference's rules:

ping_model(msgs)    PingMessage.parse (Message.scala:261-268) + the feed's outcome per raw message, with the device
                    parser's limits (the list of OWGS_ACK_UNSUPPORTED); an independent scanner in Python, pinned to
                    tests/golden/ping_vectors.json and cross-checked against the frozen ack oracle (test_feeds_cpu.py)
ack_events(...)     which InvocationFinishedMessage each completion outcome sends (CLB:266-276, 317, 327-345)
"""
import re

import numpy as np

FAIL, UNSUPPORTED, FED, RANGE = 0, 2, 3, 4
HEALTH_MAX_ID = 1 << 24
ACK_RELEASED, ACK_HEALTH = 3, 4
EV_SUCCESS, EV_SYSTEM_ERROR, EV_TIMEOUT = 1, 2, 3
NONASCII = "\U00010000"  # what a byte >= 0x80 inside a string decodes to: equal to nothing the rules look for
_WS = b" \t\n\r"
_ESC = {ord('"'): '"', ord("\\"): "\\", ord("/"): "/", ord("b"): "\b", ord("f"): "\f", ord("n"): "\n", ord("r"): "\r",
        ord("t"): "\t"}
_SIZE = re.compile(r"[ \t\n\x0b\f\r]?([0-9]+)[ \t\n\x0b\f\r]?(GB|MB|KB|B|G|M|K)[ \t\n\x0b\f\r]?", re.I | re.A)


class _Err(Exception):
    pass


class _Unsup(Exception):
    pass


class Num(str):
    """A number literal, kept as written."""


class _Scan:
    """JSON as spray-json 1.3.5 reads it (RFC 8259 grammar), the first violation or limit in byte order wins."""

    def __init__(self, b: bytes):
        self.b, self.i = b, 0

    def at(self, k=0):
        j = self.i + k
        return self.b[j] if j < len(self.b) else -1

    def ws(self):
        while self.i < len(self.b) and self.b[self.i] in _WS:
            self.i += 1

    def root(self):
        self.ws()
        v = self.value(0)
        self.ws()
        if self.i != len(self.b):
            raise _Err
        return v

    def value(self, depth):
        c = self.at()
        if c in (0x7B, 0x5B):  # { [
            if depth == 64:
                raise _Unsup
            return self.obj(depth + 1) if c == 0x7B else self.arr(depth + 1)
        if c == 0x22:
            return self.string()
        if c == 0x2D or 0x30 <= c <= 0x39:
            return self.number()
        for lit, val in ((b"true", True), (b"false", False), (b"null", None)):
            if c == lit[0]:
                if self.b[self.i:self.i + len(lit)] != lit:
                    raise _Err
                self.i += len(lit)
                return val
        raise _Err

    def obj(self, depth):
        start = self.i
        self.i += 1
        self.ws()
        pairs = []
        if self.at() == 0x7D:
            self.i += 1
            return ("obj", pairs, (start, self.i))
        while True:
            if self.at() != 0x22:
                raise _Err
            k = self.string()
            self.ws()
            if self.at() != 0x3A:
                raise _Err
            self.i += 1
            self.ws()
            pairs.append((k, self.value(depth)))
            self.ws()
            c = self.at()
            self.i += 1
            if c == 0x7D:
                return ("obj", pairs, (start, self.i))
            if c != 0x2C:
                raise _Err
            self.ws()

    def arr(self, depth):
        self.i += 1
        self.ws()
        items = []
        if self.at() == 0x5D:
            self.i += 1
            return ("arr", items)
        while True:
            items.append(self.value(depth))
            self.ws()
            c = self.at()
            self.i += 1
            if c == 0x5D:
                return ("arr", items)
            if c != 0x2C:
                raise _Err
            self.ws()

    def string(self):
        self.i += 1
        out = []
        while True:
            c = self.at()
            if c < 0x20:  # end of input or a raw control character
                raise _Err
            if c == 0x22:
                self.i += 1
                return "".join(out)
            if c == 0x5C:
                e = self.at(1)
                if e == 0x75:
                    h = self.b[self.i + 2:self.i + 6]
                    if len(h) != 4 or not re.fullmatch(rb"[0-9a-fA-F]{4}", h):
                        raise _Err
                    out.append(chr(int(h, 16)))
                    self.i += 6
                elif e in _ESC:
                    out.append(_ESC[e])
                    self.i += 2
                else:
                    raise _Err
            else:
                out.append(chr(c) if c < 0x80 else NONASCII)
                self.i += 1

    def number(self):
        m = re.match(rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?", self.b[self.i:])
        if not m:
            raise _Err
        # a fraction or exponent that starts and has no digit is an error where it stands
        rest = self.b[self.i + m.end():self.i + m.end() + 1]
        if m.group(3) is None and rest in (b"e", b"E"):
            raise _Err
        if m.group(2) is None and m.group(3) is None and rest == b".":
            raise _Err
        if m.group(3) is not None and len(m.group(3).lstrip(b"eE+-")) > 9:
            raise _Unsup
        self.i += m.end()
        return Num(m.group(0).decode("ascii"))


def _int_value(lit: str):
    """(BigDecimal(lit).intValue, significant digits as the device counts them)."""
    m = re.fullmatch(r"(-?)([0-9]+)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?", lit)
    neg, ip, fp, ex = m.group(1) == "-", m.group(2), m.group(3) or "", int(m.group(4) or 0)
    digits = ip + fp
    sig = len(digits.lstrip("0"))
    shift = ex - len(fp)
    if shift >= 0:
        v = 0 if shift >= 64 else int(digits) * 10 ** shift  # 10^64 has no low 64 bits
    else:
        keep = len(digits) + shift
        v = int(digits[:keep]) if keep > 0 else 0
    if neg:
        v = -v
    v &= 0xFFFFFFFF
    return (v - (1 << 32) if v >= 1 << 31 else v), sig


def instance_id(v):
    """InvokerInstanceId.serdes.read on a scanned value: ('ok', instance, bytes) | ('fail',) | ('unsup',)."""
    if not (isinstance(v, tuple) and v[0] == "obj"):
        return ("fail",)
    m = dict(v[1])  # the last of duplicate members
    fail = unsup = False
    inst = 0
    if not isinstance(m.get("instance"), Num):
        fail = True
    else:
        inst, sig = _int_value(m["instance"])
        unsup = sig > 34
    for k in ("uniqueName", "displayedName"):
        if k in m and m[k] is not None and not (isinstance(m[k], str) and not isinstance(m[k], Num)):
            fail = True
    um = m.get("userMemory")
    size = 0
    if not isinstance(um, str) or isinstance(um, Num):
        fail = True
    else:
        g = _SIZE.fullmatch(um)
        if not g or int(g.group(1)) > 2**63 - 1:
            fail = True
        else:
            size = int(g.group(1)) << {"B": 0, "K": 10, "M": 20, "G": 30}[g.group(2)[0].upper()]
            size &= (1 << 64) - 1
            if size >= 1 << 63:
                size -= 1 << 64
    return ("fail",) if fail else ("unsup",) if unsup else ("ok", inst, size)


def ping_parts(msg: bytes):
    """('fail' | 'unsup', None) or ('name', scanned value of the last top-level "name" member)."""
    if b"\xef\xbf\xbf" in msg:
        return "unsup", None
    try:
        root = _Scan(msg).root()
    except _Unsup:
        return "unsup", None
    except _Err:
        return "fail", None
    if not (isinstance(root, tuple) and root[0] == "obj"):
        return "fail", None
    names = [v for k, v in root[1] if k == "name"]
    if not names:
        return "fail", None
    return "name", names[-1]


def ping_model(msgs):
    """(kind u8, instance i32, bytes i64) per raw message, as owgs_process_pings reports them."""
    n = len(msgs)
    kind, inst, mem = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int64)
    for i, msg in enumerate(msgs):
        what, v = ping_parts(msg)
        if what != "name":
            kind[i] = UNSUPPORTED if what == "unsup" else FAIL
            continue
        r = instance_id(v)
        if r[0] != "ok":
            kind[i] = UNSUPPORTED if r[0] == "unsup" else FAIL
        elif 0 <= r[1] < HEALTH_MAX_ID:
            kind[i], inst[i], mem[i] = FED, r[1], r[2]
        else:
            kind[i], inst[i] = RANGE, r[1]
    return kind, inst, mem


def ack_events(kind, invoker, flags, forced=None):
    """The supervision events of a completion batch, in order: (invoker i32, kind u8).  kind / invoker / flags are the
    outputs of process_acks or complete_activations (flags bit0 = isSystemError), forced the call's forced bits."""
    kind, invoker, flags = np.asarray(kind), np.asarray(invoker), np.asarray(flags)
    forced = np.zeros(len(kind), bool) if forced is None else np.asarray(forced).astype(bool)
    feeds = ((kind == ACK_RELEASED) | (kind == ACK_HEALTH)) & (invoker >= 0) & (invoker < HEALTH_MAX_ID)
    ev = np.where(forced, EV_TIMEOUT, np.where(flags & 1, EV_SYSTEM_ERROR, EV_SUCCESS)).astype(np.uint8)
    return invoker[feeds].astype(np.int32), ev[feeds]
