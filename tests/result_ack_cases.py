"""Message generators for the result-carrying acks (owgs_process_result_acks): canonical messages as the reference
prints them, and a fuzz set of canonical messages with one defect each.  Shared by test_result_acks_cpu.py (which
checks the generators against the model) and test_gpu_result_acks.py."""
import json

import numpy as np

from openwhisk_amd import workload as W

_NS = ("guest", "whisk.system", "org_7/pkg-2", "team@example.org", "ns-31/utils")
_NAMES = ("hello", "resize image", "echo_v2", "a", "order-handler.prod")
_SUBJ = ("guest", "anon-9f3k2lQ8xT7bY1mZc4Vd6Ws0Rt5", "service account 7")
_KINDS = ("nodejs:20", "python:3.11", "blackbox")
_WORDS = ("alpha", "beta", "gamma", "delta", "He said \"hi\"", "line\nbreak", "tab\there", "café", "über")


def _js(x) -> str:
    """spray-json compactPrint of a value (no spaces; non-ASCII characters printed raw)."""
    return json.dumps(x, ensure_ascii=False, separators=(",", ":"))


def invoker_json(instance: int, mem_mb: int = 16384, unique=None) -> str:
    return '{"instance":%d%s,"userMemory":"%d MB"}' % (instance, (',"uniqueName":' + _js(unique)) if unique else "",
                                                      mem_mb)


def activation_members(rng, aid: str, result_bytes: int = 300):
    """WhiskActivation.serdes.write (jsonFormat13): the case class's members in order as (name, printed value); None
    options (cause, duration; the response's result and size) are omitted."""
    start = 1_700_000_000_000 + int(rng.integers(0, 10**9))
    dur = int(rng.integers(1, 60_000))
    payload, k = {}, 0
    while len(_js(payload)) < result_bytes:
        payload["f%d" % k] = [_WORDS[int(rng.integers(0, len(_WORDS)))], int(rng.integers(-10**6, 10**6)),
                              {"ok": bool(rng.integers(0, 2)), "v": None}]
        k += 1
    status = int(rng.choice([0, 0, 0, 1, 2, 3]))
    resp = {"statusCode": status, "result": payload}
    if rng.random() < 0.2:
        resp["size"] = int(rng.integers(1, 1 << 20))
    ann = [{"key": "path", "value": "guest/hello"}, {"key": "waitTime", "value": int(rng.integers(0, 5000))},
           {"key": "kind", "value": _KINDS[int(rng.integers(0, len(_KINDS)))]}, {"key": "timeout", "value": False},
           {"key": "limits", "value": {"concurrency": 1, "logs": 10, "memory": 256, "timeout": 60000}}]
    if rng.random() < 0.5:
        ann.append({"key": "initTime", "value": int(rng.integers(1, 900))})
    m = [("namespace", _js(_NS[int(rng.integers(0, len(_NS)))])), ("name", _js(_NAMES[int(rng.integers(0, len(_NAMES)))])),
         ("subject", _js(_SUBJ[int(rng.integers(0, len(_SUBJ)))])), ("activationId", _js(aid)), ("start", str(start)),
         ("end", str(start + dur))]
    if rng.random() < 0.3:
        m.append(("cause", _js(W.activation_ids(rng, 1)[0])))
    logs = [] if rng.random() < 0.7 else ["2023-11-14T22:13:20.1Z stdout: %s" % _WORDS[int(rng.integers(0, 4))]]
    m += [("response", _js(resp)), ("logs", _js(logs)), ("version", '"0.0.%d"' % int(rng.integers(1, 40))),
          ("publish", "false"), ("annotations", _js(ann))]
    if rng.random() < 0.8:
        m.append(("duration", str(dur)))
    return m


def print_object(members) -> str:
    return "{" + ",".join('"%s":%s' % kv for kv in members) + "}"


def combined_message(resp: str, instance: int, system_error: bool = False, tid=W.TESTING_TID) -> bytes:
    """CombinedCompletionAndResultMessage.serdes.write + compactPrint (jsonFormat4, Message.scala:191-193)."""
    return ('{"transid":["%s",%d],"response":%s,"isSystemError":%s,"invoker":%s}'
            % (tid[0], tid[1], resp, "true" if system_error else "false", invoker_json(instance))).encode("utf-8")


def result_message(resp: str, tid=W.TESTING_TID) -> bytes:
    """ResultMessage.serdes.write + compactPrint (jsonFormat2, Message.scala:221)."""
    return ('{"transid":["%s",%d],"response":%s}' % (tid[0], tid[1], resp)).encode("utf-8")


def canonical(rng, aid: str, instance: int, what: str, result_bytes: int = 300, system_error=False) -> bytes:
    """what: 'combined' / 'result' (Right), 'combined-left' / 'result-left' (after shrink), 'completion'."""
    if what == "completion":
        return W.completion_message(aid, instance, system_error=system_error)
    resp = _js(aid) if what.endswith("-left") else print_object(activation_members(rng, aid, result_bytes))
    if what.startswith("combined"):
        return combined_message(resp, instance, system_error)
    return result_message(resp)


def canonical_messages(seed: int, n: int):
    rng = np.random.default_rng(seed)
    aids = W.activation_ids(rng, n)
    kinds = ("combined", "result", "combined-left", "result-left", "completion")
    return [canonical(rng, aids[i], int(rng.integers(0, 40)), kinds[i % 5], system_error=i % 7 == 0) for i in range(n)]


# ---- one rule violation each: the object leaves the accepted subset (JVM)
_BAD = (("namespace", '""'), ("namespace", '"guest /x"'), ("name", '"a/b"'), ("subject", '"abc"'),
        ("subject", '"abcde "'), ("activationId", '"ABCDEF0123456789abcdef0123456789"'), ("start", "1.5"),
        ("end", '"2023-11-14T22:13:20Z"'), ("response", '{"result":1}'), ("response", '{"statusCode":1e1}'),
        ("logs", "[1]"), ("version", '"0.0.0"'), ("version", '"1.2"'), ("publish", "null"),
        ("annotations", '[{"key":"k"}]'), ("annotations", '[{"key":" ","value":1}]'), ("duration", "1e2"),
        ("cause", '"zz"'))


def _violate(rng, members):
    m = list(members)
    r = int(rng.integers(0, 4))
    if r == 0:  # a required member is missing
        req = [i for i, (k, _) in enumerate(m) if k not in ("cause", "duration")]
        del m[req[int(rng.integers(0, len(req)))]]
    elif r == 1:  # a member twice
        m.insert(int(rng.integers(0, len(m) + 1)), m[int(rng.integers(0, len(m)))])
    elif r == 2:  # a member name written with an escape
        i = int(rng.integers(0, len(m)))
        k = m[i][0]
        m[i] = (k[:1] + "\\u%04x" % ord(k[1]) + k[2:], m[i][1])
    else:
        k, v = _BAD[int(rng.integers(0, len(_BAD)))]
        m = [(a, v if a == k else b) for a, b in m]
        if k not in [a for a, _ in m]:
            m.append((k, v))
    return m


def fuzz_messages(seed: int, n: int, aids=None, invokers=None):
    """n messages: canonical ones (accepted), one rule violation inside the object (JVM), truncations and responses
    that are neither id nor object (FAIL), escapes and byte-level edits.  aids / invokers: ids (and their invokers)
    the messages draw from, so that a caller who tracked them sees completions; default: fresh ids."""
    rng = np.random.default_rng(seed)
    if aids is None:
        aids = W.activation_ids(rng, max(1, n // 2))
        invokers = rng.integers(0, 40, len(aids))
    out = []
    for _ in range(n):
        j = int(rng.integers(0, len(aids)))
        aid, inv = aids[j], int(invokers[j])
        comb = rng.random() < 0.6
        wrap = (lambda r: combined_message(r, inv, rng.random() < 0.1)) if comb else result_message
        u = rng.random()
        if u < 0.20:
            out.append(wrap(print_object(activation_members(rng, aid, int(rng.integers(20, 400))))))
        elif u < 0.27:
            out.append(wrap(_js(aid)))
        elif u < 0.31:
            out.append(W.completion_message(aid, inv, system_error=rng.random() < 0.1))
        elif u < 0.62:
            out.append(wrap(print_object(_violate(rng, activation_members(rng, aid, int(rng.integers(20, 200)))))))
        elif u < 0.80:
            m = wrap(print_object(activation_members(rng, aid, 60)))
            out.append(m[:int(rng.integers(1, len(m)))])
        elif u < 0.92:
            out.append(wrap(("17", "true", "null", '["%s"]' % aid, '"%s"' % aid[:31], '"%s"' % aid.upper(),
                             '"%sg"' % aid[:31])[int(rng.integers(0, 7))]))
        elif u < 0.95:
            out.append(wrap('"%s\\u0663"' % aid[:31]))  # a non-ASCII digit: UNSUPPORTED
        else:
            out.append(W.mutate(rng, wrap(print_object(activation_members(rng, aid, 40))), int(rng.integers(1, 3))))
    return out
