"""Known-answer vectors for the ping feed (InvokerPool.processInvokerPing, InvokerSupervision.scala:174-185).

Each message is written the way the reference serialises it or as a deliberate variant, and each expectation is
derived BY HAND from the reference source (not from the model or the device), citing the rule it follows:
  - PingMessage.serdes = jsonFormat(PingMessage.apply _, "name") (Message.scala:261-268): the root must be an object
    with a member "name"; spray-json's JsObject keeps the LAST of duplicate members; member names are compared after
    unescaping; other members are ignored
  - InvokerInstanceId.serdes = jsonFormat4 (InstanceId.scala:31-49): instance Int (IntJsonFormat = BigDecimal.intValue:
    truncate, low 32 bits), uniqueName / displayedName Option[String] (absent or null -> None, anything but a string
    fails), userMemory ByteSize
  - ByteSize.fromString regex (?i)\\s?(\\d+)\\s?(GB|MB|KB|B|G|M|K)\\s? and group(1).toLong (Size.scala:119-138); \\d is
    [0-9] and \\s is [ \\t\\n\\x0B\\f\\r] (java.util.regex without UNICODE_CHARACTER_CLASS); toBytes = size * 1024^k
    in Long arithmetic, which wraps (Size.scala:28-62)
  - the device parser's limits are those of the ack parser (include/owgs.h, OWGS_ACK_UNSUPPORTED)
  - the FSM's status vector takes instances in [0, 2^24) (OWGS_HEALTH_MAX_ID); a parsed ping outside it is RANGE
The vectors are data: run `python tests/golden/make_ping_golden.py` to regenerate tests/golden/ping_vectors.json.
Kinds: FAIL 0, UNSUPPORTED 2, FED 3, RANGE 4.  instance is given for FED and RANGE, bytes for FED.
"""
import json
import os

KB, MB, GB = 1 << 10, 1 << 20, 1 << 30
FAIL, UNSUPPORTED, FED, RANGE = 0, 2, 3, 4
INV = '{"instance":%s,"userMemory":"%s"}'


def ping(inst="0", mem="16384 MB"):
    return '{"name":%s}' % (INV % (inst, mem))


V = []


def add(name, msg, kind, instance=0, mem=0):
    V.append({"name": name, "msg": msg, "kind": kind, "instance": instance if kind in (FED, RANGE) else 0,
              "bytes": mem if kind == FED else 0})


add("canonical ping (PingMessage(InvokerInstanceId(0, userMemory = 16384.MB)).serialize)", ping(), FED, 0, 16384 * MB)
add("canonical ping with both names", '{"name":{"instance":3,"uniqueName":"u1","displayedName":"d1",'
    '"userMemory":"16384 MB"}}', FED, 3, 16384 * MB)
add("unit MB with a space", ping("1", "2048 MB"), FED, 1, 2048 * MB)
add("unit g, lower case, no space", ping("1", "2g"), FED, 1, 2 * GB)
add("unit K between spaces", ping("1", " 1 K "), FED, 1, KB)
add("unit B without a space", ping("1", "512B"), FED, 1, 512)
add("unit kB, mixed case", ping("1", "7 kB"), FED, 1, 7 * KB)
add("unit Gb", ping("1", "4Gb"), FED, 1, 4 * GB)
add("unit M", ping("1", "3M"), FED, 1, 3 * MB)
add("form feed and vertical tab are \\s", ping("1", "\\f5\\u000bMB"), FED, 1, 5 * MB)
add("leading zeros", ping("2", "0002048 MB"), FED, 2, 2048 * MB)
add("zero bytes", ping("2", "0 B"), FED, 2, 0)
add("Long.MAX digits", ping("2", "9223372036854775807 B"), FED, 2, 2**63 - 1)
add("Long.MAX + 1 (toLong throws)", ping("2", "9223372036854775808 B"), FAIL)
add("one more digit than Long.MAX", ping("2", "92233720368547758070 B"), FAIL)
add("wrapping product 2^53 KB = 2^63 -> Long.MIN", ping("2", "9007199254740992 KB"), FED, 2, -2**63)
add("wrapping product Long.MAX GB -> -2^30", ping("2", "9223372036854775807 GB"), FED, 2, -GB)
add("two inner spaces", ping("2", "1024  MB"), FAIL)
add("no-break space, escaped", ping("2", "1024\\u00a0MB"), FAIL)
add("no-break space, raw", ping("2", "1024\xa0MB"), FAIL)
add("empty userMemory", ping("2", ""), FAIL)
add("userMemory a number", '{"name":{"instance":2,"userMemory":1024}}', FAIL)
add("userMemory missing", '{"name":{"instance":2}}', FAIL)
add("userMemory without a unit", ping("2", "1024"), FAIL)
add("userMemory negative", ping("2", "-1 MB"), FAIL)
add("userMemory digit escaped", ping("2", "\\u0031 MB"), FED, 2, MB)
add("unit Kelvin sign is not K", ping("2", "1 \u212aB"), FAIL)
add("instance 1e2", ping("1e2"), FED, 100, 16384 * MB)
add("instance 3.9 -> 3", ping("3.9"), FED, 3, 16384 * MB)
add("instance -1", ping("-1"), RANGE, -1)
add("instance -0.5 -> 0", ping("-0.5"), FED, 0, 16384 * MB)
add("instance 2^32 + 1 -> 1", ping("4294967297"), FED, 1, 16384 * MB)
add("instance 2^31 -> Int.MIN", ping("2147483648"), RANGE, -2**31)
add("instance 2^24 - 1", ping("16777215"), FED, 16777215, 16384 * MB)
add("instance 2^24", ping("16777216"), RANGE, 16777216)
add("instance a string", ping('"0"'), FAIL)
add("instance missing", '{"name":{"userMemory":"1 MB"}}', FAIL)
add("instance of 35 significant digits", ping("1" + "0" * 34), UNSUPPORTED)
add("uniqueName null", '{"name":{"instance":4,"uniqueName":null,"userMemory":"1 MB"}}', FED, 4, MB)
add("uniqueName 5", '{"name":{"instance":4,"uniqueName":5,"userMemory":"1 MB"}}', FAIL)
add("displayedName an object", '{"name":{"instance":4,"displayedName":{},"userMemory":"1 MB"}}', FAIL)
add("duplicate name member: the last wins", '{"name":%s,"name":%s}' % (INV % ("1", "1 MB"), INV % ("9", "2 MB")),
    FED, 9, 2 * MB)
add("duplicate name member: the last is bad", '{"name":%s,"name":7}' % (INV % ("1", "1 MB")), FAIL)
add("duplicate instance member: the last wins", '{"name":{"instance":1,"userMemory":"1 MB","instance":6}}', FED, 6,
    MB)
add("key spelt \\u006eame", '{"\\u006eame":%s}' % (INV % ("5", "1 MB")), FED, 5, MB)
add("key Name is another member", '{"Name":%s}' % (INV % ("5", "1 MB")), FAIL)
add("extra top-level members, a nested name is ignored",
    '{"x":[1,{"name":5}],"name":%s,"y":null,"z":{"name":"q"}}' % (INV % ("8", "1 MB")), FED, 8, MB)
add("extra members inside the instance id", '{"name":{"a":[],"instance":8,"b":{"instance":1},"userMemory":"1 MB"}}',
    FED, 8, MB)
add("whitespace around the root and inside", " \r\n\t" + ping("7", "1 MB").replace(":", " :\n").replace(",", " , ")
    + "\n ", FED, 7, MB)
add("root array", "[" + ping() + "]", FAIL)
add("root string", '"name"', FAIL)
add("missing name", '{"nam":%s}' % (INV % ("0", "1 MB")), FAIL)
add("name null", '{"name":null}', FAIL)
add("name a string", '{"name":"invoker0"}', FAIL)
add("name an array", '{"name":[%s]}' % (INV % ("0", "1 MB")), FAIL)
add("trailing garbage", ping() + "x", FAIL)
add("two roots", ping() + ping(), FAIL)
add("truncated", ping()[:-1], FAIL)
add("empty message", "", FAIL)
add("only whitespace", "  ", FAIL)
add("raw control character in a string", '{"name":%s,"x":"a\tb"}' % (INV % ("0", "1 MB")), FAIL)
add("leading zero number", ping("01"), FAIL)
add("U+FFFF in a string", '{"name":%s,"x":"\uffff"}' % (INV % ("0", "1 MB")), UNSUPPORTED)
add("65 levels of nesting", '{"name":%s,"x":%s}' % (INV % ("0", "1 MB"), "[" * 64 + "]" * 64), UNSUPPORTED)
add("64 levels of nesting", '{"name":%s,"x":%s}' % (INV % ("0", "1 MB"), "[" * 63 + "]" * 63), FED, 0, MB)
add("exponent of 10 digits", '{"name":%s,"x":1e1234567890}' % (INV % ("0", "1 MB")), UNSUPPORTED)
add("non-ASCII in the names", '{"name":{"instance":2,"uniqueName":"café","userMemory":"1 MB"}}', FED, 2, MB)

if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ping_vectors.json"), "w",
              encoding="utf-8") as f:
        json.dump({"vectors": V}, f, indent=1, ensure_ascii=False)
    print(len(V), "vectors")
