"""Known-answer vectors for owgs_process_result_acks (include/owgs.h "result-carrying acks").

Each message is written the way the reference serialises it or as a deliberate variant, and each expectation is
derived BY HAND from the reference source and the accepted subset listed in include/owgs.h (not from the model or the
device), citing the rule it follows:
  - dispatch (Message.scala:240-258): "invoker" + "response" -> CombinedCompletionAndResultMessage (jsonFormat4,
    Message.scala:191-193), "response" alone -> ResultMessage (jsonFormat2, Message.scala:221)
  - eitherResponse (Message.scala:227-238): a string is Left(ActivationId) through ActivationId.serdes
    (ActivationId.scala:58-95), an object Right(WhiskActivation), anything else a deserializationError
  - WhiskActivation.serdes = jsonFormat13 (WhiskActivation.scala:52-64, 182); the device takes an object only inside
    the accepted subset and reports every other object as JVM (1), never as FAIL
  - precedence: JVM over FAIL over UNSUPPORTED
Kinds: FAIL 0, JVM 1, UNSUPPORTED 2, 3 = an accepted Combined message (a completion: RELEASED / HEALTH / NOENTRY once
the table is consulted), 7 = an accepted ResultMessage.  For 3 and 7: right = the response is an object, aid = the id.
The vectors are data: run `python tests/golden/make_result_ack_golden.py` to regenerate result_ack_vectors.json.
"""
import json
import os

AID = "0123456789abcdef0123456789abcdef"
WAID = "fedcba9876543210fedcba9876543210"
TID = '["sid_testing",1700000000456]'
INV = '{"instance":%s,"userMemory":"1024 MB"}'
FAIL, JVM, UNSUP, COMBINED, RESULT = 0, 1, 2, 3, 7

# WhiskActivation.serdes.write + compactPrint: the case class's member order, None options omitted
WA = [("namespace", '"guest"'), ("name", '"hello"'), ("subject", '"guest-subject"'), ("activationId", '"%s"' % WAID),
      ("start", "1700000000000"), ("end", "1700000000123"),
      ("response", '{"statusCode":0,"result":{"greeting":"Hello, world"}}'), ("logs", "[]"), ("version", '"0.0.1"'),
      ("publish", "false"),
      ("annotations", '[{"key":"path","value":"guest/hello"},{"key":"waitTime","value":35},'
                      '{"key":"kind","value":"nodejs:20"},{"key":"timeout","value":false},'
                      '{"key":"limits","value":{"concurrency":1,"logs":10,"memory":256,"timeout":60000}}]'),
      ("duration", "123")]


def wa(drop=(), extra="", **repl):
    """The canonical activation with members replaced (name=value text), dropped, or text appended before '}'."""
    out = []
    for k, v in WA:
        if k in drop:
            continue
        out.append('"%s":%s' % (k, repl.get(k, v)))
    return "{" + ",".join(out) + extra + "}"


def combined(resp, sys="false", inv=INV % "0", tid=TID, extra=""):
    return '{"transid":%s,"response":%s,"isSystemError":%s,"invoker":%s%s}' % (tid, resp, sys, inv, extra)


def result(resp, tid=TID, extra=""):
    return '{"transid":%s,"response":%s%s}' % (tid, resp, extra)


V = []


def add(name, msg, kind, right=0, aid=None):
    e = {"name": name, "msg": msg, "kind": kind}
    if kind in (COMBINED, RESULT):
        e.update(right=right, aid=aid or (WAID if right else AID))
    V.append(e)


def both(name, resp, kind_c, kind_r=None, right=0, aid=None):
    add("combined: " + name, combined(resp), kind_c, right, aid)
    add("result: " + name, result(resp), kind_c if kind_r is None else kind_r, right, aid)


def rule(name, inside, outside):
    """One message just inside a subset rule (accepted as Right) and one just outside it (JVM)."""
    for i, r in enumerate(inside):
        add("inside %s #%d" % (name, i), combined(r), COMBINED, 1)
    for i, r in enumerate(outside):
        add("outside %s #%d" % (name, i), combined(r), JVM)


# ---- the two Left cases tests/golden/make_ack_golden.py lists as kind 1 (AcknowledgementMessageTests:57-64)
add("result message, Left", '{"transid":%s,"response":"%s"}' % (TID, AID), RESULT)
add("combined message, Left", '{"transid":%s,"response":"%s","isSystemError":false,"invoker":%s}'
    % (TID, AID, INV % "0"), COMBINED)
# ---- canonical Right
add("canonical combined, Right (ContainerProxy.scala:768-781)", combined(wa()), COMBINED, 1)
add("canonical result, Right", result(wa()), RESULT, 1)
add("result with cause, without duration", result(wa(drop=("duration",), extra=',"cause":"%s"' % AID)), RESULT, 1)

# ---- Left: ActivationId.serdes on a string
both("id of 31 characters", '"%s"' % AID[:31], FAIL)
both("id of 33 characters", '"%s0"' % AID, FAIL)
both("upper-case hex", '"%s"' % AID.upper(), FAIL)
both("escaped a decodes to a", '"0123456789\\u0061bcdef0123456789abcdef"', COMBINED, RESULT)
both("non-ASCII digit (Char.isDigit, ActivationId.scala:50)", '"0123456789abcdef0123456789abcde\\u0663"', UNSUP)
both("raw non-ASCII character", '"0123456789abcdef0123456789abcdeé"', UNSUP)
# ---- neither string nor object (Message.scala:236)
for lit in ("12345678901234567890123456789012", "true", "false", "null", '["%s"]' % AID, "1.5"):
    both("response " + lit[:12], lit, FAIL)

# ---- Combined: the other members
add("combined without transid", '{"response":"%s","invoker":%s}' % (AID, INV % "0"), FAIL)
add("combined, isSystemError null", combined('"%s"' % AID, sys="null"), COMBINED)
add("combined, isSystemError absent", '{"transid":%s,"response":"%s","invoker":%s}' % (TID, AID, INV % "3"), COMBINED)
add("combined, isSystemError a string", combined('"%s"' % AID, sys='"false"'), FAIL)
add("combined, invoker without userMemory", combined('"%s"' % AID, inv='{"instance":0}'), FAIL)
add("combined, top-level activationId is ignored (Message.scala:125)",
    combined(wa(), extra=',"activationId":"not an id"'), COMBINED, 1)
add("combined, last response wins", combined("17", extra=',"response":"%s"' % AID), COMBINED)
add("combined, escaped top-level member name", combined(wa()).replace('"response"', '"resp\\u006fnse"', 1), COMBINED, 1)
# ---- Result: jsonFormat2 ignores every other member
add("result without transid", '{"response":"%s"}' % AID, FAIL)
add("result, other members ignored", result('"%s"' % AID, extra=',"isSystemError":"x","activationId":5'), RESULT)
add("result, transid of another shape (TransactionId.scala:243-251)", result(wa(), tid='"x"'), RESULT, 1)

# ---- precedence
add("JVM over FAIL: object outside the subset, no transid", '{"response":%s,"invoker":%s}'
    % (wa(publish="null"), INV % "0"), JVM)
add("JVM over FAIL: object outside the subset, broken invoker", combined(wa(publish="null"), inv="[0]"), JVM)
add("JVM over UNSUPPORTED: instance of 35 digits", combined(wa(publish="null"), inv=INV % ("1" * 35)), JVM)
add("FAIL over UNSUPPORTED: non-ASCII id, isSystemError a string",
    combined('"0123456789abcdef0123456789abcde\\u0663"', sys='"x"'), FAIL)
add("FAIL over UNSUPPORTED: short id, instance of 35 digits", combined('"abc"', inv=INV % ("1" * 35)), FAIL)
add("UNSUPPORTED alone: good id, instance of 35 digits", combined('"%s"' % AID, inv=INV % ("1" * 35)), UNSUP)
add("in the subset but no transid: FAIL", '{"response":%s,"invoker":%s}' % (wa(), INV % "0"), FAIL)
add("grammar error inside the object: FAIL", combined(wa(logs="[,]")), FAIL)
# (the message, the activation and its response are containers 1-3: k brackets inside result reach depth 3 + k)
add("container depth 65 inside result: UNSUPPORTED",
    combined(wa(response='{"statusCode":0,"result":%s}' % ("[" * 62 + "]" * 62))), UNSUP)
add("container depth 64 inside result", combined(wa(response='{"statusCode":0,"result":%s}'
                                                    % ("[" * 61 + "]" * 61))), COMBINED, 1)

# ---- the accepted subset, rule by rule
rule("member names", [wa(extra=',"updated":1700000000999,"x":{"name":5}')],
     [wa().replace('"name"', '"n\\u0061me"', 1), wa(extra=',"publish":true'), wa(extra=',"x\\n":1')])
P256 = "a" * 256
rule("namespace", [wa(namespace='"guest/pkg"'), wa(namespace='"/guest//pkg/"'), wa(namespace='"%s"' % P256),
                   wa(namespace='"a b/_x@y.z&w-"')],
     [wa(namespace='"%sa"' % P256), wa(namespace='""'), wa(namespace='"//"'), wa(namespace='"guest /pkg"'),
      wa(namespace='"@guest"'), wa(namespace='"gu\\u0065st"'), wa(namespace='"guést"'), wa(namespace="5"),
      wa(namespace='"a+b"')])
rule("name", [wa(name='"a"'), wa(name='"hello world.v2"')], [wa(name='"a/b"'), wa(name='""'), wa(name='"a "'),
                                                            wa(name="null")])
rule("subject", [wa(subject='"abcde"'), wa(subject='"a b!~#"')],
     [wa(subject='"abcd"'), wa(subject='" abcde"'), wa(subject='"abcde "'), wa(subject='"abc\\tde"'),
      wa(subject='"abcdé"')])
rule("activationId", [], [wa(activationId='"%s"' % WAID[:31]), wa(activationId='"%s"' % WAID.upper()),
                         wa(activationId="12345678901234567890123456789012"),
                         wa(activationId='"\\u0066%s"' % WAID[1:])])
rule("cause", [wa(extra=',"cause":null'), wa(extra=',"cause":"%s"' % AID)],
     [wa(extra=',"cause":"%s"' % AID[:30]), wa(extra=',"cause":5')])
rule("start / end", [wa(start="0", end="-1"), wa(start="9" * 18), wa(end="-" + "9" * 18)],
     [wa(start="1" + "0" * 18), wa(end="1.5"), wa(start="1e3"), wa(start='"2023-11-14T22:13:20Z"'), wa(end="null")])
rule("duration", [wa(duration="null"), wa(duration="0")], [wa(duration="1.0"), wa(duration='"1"'),
                                                           wa(duration="1" + "0" * 18)])
rule("response", [wa(response='{"statusCode":-1}'), wa(response='{"statusCode":999999999,"size":null}'),
                  wa(response='{"statusCode":3,"result":[1,{"a":[]}],"size":12,"more":{}}'),
                  wa(response='{"size":7,"statusCode":1}')],
     [wa(response='{"statusCode":1000000000}'), wa(response='{"result":{}}'), wa(response='{"statusCode":0,"size":"x"}'),
      wa(response='{"status\\u0043ode":0}'), wa(response='{"statusCode":0,"statusCode":0}'), wa(response="[]"),
      wa(response='{"statusCode":0.0}'), wa(response='{"statusCode":0,"size":1e2}'), wa(response='{"statusCode":null}')])
rule("logs", [wa(logs='["a","2023 stdout: b\\n"]'), wa(logs='[ ]')], [wa(logs="[1]"), wa(logs='"x"'),
                                                                     wa(logs='["a",null]')])
rule("version", [wa(version='"999999999.0.10"'), wa(version='"0.1.0"')],
     [wa(version='"0.0.0"'), wa(version='"1.2"'), wa(version='"1.2.3.4"'), wa(version='"01.2.3"'),
      wa(version='"1000000000.0.0"'), wa(version='"1.2.x"'), wa(version="1")])
rule("publish", [wa(publish="true")], [wa(publish="null"), wa(publish='"true"'), wa(publish="0")])
rule("annotations", [wa(annotations="[]"), wa(annotations='[{"key":"k","value":null,"init":true}]'),
                     wa(annotations='[{"value":[{"key":1}],"key":" k ","other":0}]')],
     [wa(annotations='[{"key":" ","value":1}]'), wa(annotations='[{"key":"","value":1}]'),
      wa(annotations='[{"value":1}]'), wa(annotations='[{"key":"k"}]'),
      wa(annotations='[{"key":"k","key":"k","value":1}]'), wa(annotations='[{"key":"k","value":1,"value":1}]'),
      wa(annotations='[{"key":"k","value":1,"init":"x"}]'), wa(annotations='[{"key":"k","value":1,"init":null}]'),
      wa(annotations='[{"key":"k","value":1,"init":true,"init":true}]'), wa(annotations="[5]"),
      wa(annotations='[{"k\\u0065y":"k","value":1}]'), wa(annotations='[{"key":"k\\u0061","value":1}]'),
      wa(annotations='[{"key":5,"value":1}]'), wa(annotations='{"key":"k","value":1}'),
      wa(annotations='[{"key":"k","value":1},[]]')])
rule("presence", [wa(drop=("duration",))],
     [wa(drop=(k,)) for k, _ in WA if k != "duration"])

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "result_ack_vectors.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"vectors": V}, f, indent=1, ensure_ascii=False)
        f.write("\n")
    print(len(V), "vectors ->", path)
