// owgs_acks.hip -- completion-ack path on the device.
//
// Replaces, for a batch of raw ack messages from the feed (LB:94-108: the activeAck topic, 128-message batches):
//   CommonLoadBalancer.processAcknowledgement   CLB:205-232   AcknowledegmentMessage.parse (Message.scala:224-256)
//   CommonLoadBalancer.processCompletion        CLB:260-346   activationSlots.remove + outcome + releaseInvoker
// and, at publish time, the activationSlots.getOrElseUpdate of setupActivation (CLB:148-166).
//
// Kernels
//   owgs_ack_parse_kernel    one thread per message: an iterative JSON scanner (explicit bit stack of containers,
//                            16-byte vector reads through a per-thread window) that validates the whole message
//                            (RFC 8259 grammar, as spray-json 1.3.5 parses it) and records the last occurrence of
//                            the top-level members transid / activationId / isSystemError / invoker / response;
//                            then converts the members CompletionMessage needs (jsonFormat4, Message.scala:204-216):
//                            ActivationId.parse (32 chars [0-9a-f] -> 128-bit key), InvokerInstanceId.instance
//                            (BigDecimal.intValue), userMemory (ByteSize regex + toLong), uniqueName/displayedName
//                            (Option[String]), isSystemError (Option[Boolean]), transid == invokerHealth.
//                            A template over RESULTS: <false> leaves a message with a `response` member to the JVM;
//                            <true> (owgs_process_result_acks) also takes CombinedCompletionAndResultMessage and
//                            ResultMessage: a `response` that is an id, or a WhiskActivation inside the accepted
//                            subset of include/owgs.h, checked by inlined functions over the byte window.
//   owgs_act_*_kernel        activationSlots as an open-addressing table in HBM: key = 128-bit activation id,
//                            value = {action handle, caller ticket} plus the entry's namespace, completion-ack
//                            deadline, invoker and arm sequence (owgs_expire.hip sweeps the deadlines, summarised per
//                            tile of 1,024 slots in tmin).  Inserts claim an empty slot by 64-bit CAS;
//                            same-key inserts of one batch resolve to the lowest batch index (getOrElseUpdate in
//                            array order); removals of one batch resolve to the lowest message index
//                            (activationSlots.remove in array order: later duplicates see None).
//   owgs_ack_resolve_kernel  processCompletion outcome per message + the release record of releaseInvoker
//                            (SCPB:327-331: invokerSlots.lift(invoker.toInt) -- out-of-range ids are no-ops),
//                            applied in message order by owgs_release_seq_kernel (owgs_kernels.hip).
// The fill and resolve kernels also keep the controller's in-flight books (totalActivations, the two memory totals,
// activationsPerNamespace: CLB:62-65), incremented at CLB:121-127 and decremented at CLB:280-284; see "in-flight
// books" below.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "owgs_internal.h"
#include "owgs_launch.h"

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------ byte window
// Reads the message through aligned 16-byte loads; the host pads the byte buffer by 16 bytes so the last block is
// readable.  at(i) returns -1 outside [b, e).
struct Win {
    const uint4* base;
    int64_t b, e, blk;
    uint4 v;
    __device__ Win(const uint8_t* bytes, int64_t b_, int64_t e_) : base((const uint4*)bytes), b(b_), e(e_), blk(-1) {}
    __device__ __forceinline__ int at(int64_t i) {
        if (i >= e || i < b) return -1;
        const int64_t k = i >> 4;
        if (k != blk) {
            v = base[k];
            blk = k;
        }
        const int q = (int)(i >> 2) & 3;
        const uint32_t w = q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
        return (int)((w >> ((i & 3) * 8)) & 0xFFu);
    }
};

__device__ __forceinline__ bool is_ws(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
__device__ __forceinline__ int hex_val(int c) {
    return (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : -1;
}

// one decoded UTF-16 code unit of a validated JSON string at i (i points inside the quotes); advances i.
// -1 at the closing quote; non-ASCII bytes decode to 0x10000 (never equal to an ASCII unit)
__device__ __forceinline__ int unit_at(Win& W, int64_t& i) {
    const int c = W.at(i);
    if (c == '"') return -1;
    if (c == '\\') {
        const int e = W.at(i + 1);
        if (e == 'u') {
            const int u = (hex_val(W.at(i + 2)) << 12) | (hex_val(W.at(i + 3)) << 8) | (hex_val(W.at(i + 4)) << 4) |
                          hex_val(W.at(i + 5));
            i += 6;
            return u;
        }
        i += 2;
        return e == 'b' ? 8 : e == 'f' ? 12 : e == 'n' ? 10 : e == 'r' ? 13 : e == 't' ? 9 : e;
    }
    i += 1;
    return c >= 0x80 ? 0x10000 : c;
}

// member names the path reads; decoded name compared against each (key at k = its opening quote)
#define K_AID 0
#define K_INV 1
#define K_SYS 2
#define K_RESP 3
#define K_TID 4
#define K_INSTANCE 5
#define K_UNIQUE 6
#define K_DISPLAYED 7
#define K_USERMEM 8
#define K_NAME 9
// the members of a `response` object (WhiskActivation, jsonFormat13), in the case class's order ...
#define K_WA_NAMESPACE 10
#define K_WA_NAME 11
#define K_WA_SUBJECT 12
#define K_WA_AID 13
#define K_WA_START 14
#define K_WA_END 15
#define K_WA_CAUSE 16
#define K_WA_RESPONSE 17
#define K_WA_LOGS 18
#define K_WA_VERSION 19
#define K_WA_PUBLISH 20
#define K_WA_ANNOTATIONS 21
#define K_WA_DURATION 22
// ... of its ActivationResponse (jsonFormat3) and of one annotation (Parameters.serdes)
#define K_AR_STATUS 23
#define K_AR_RESULT 24
#define K_AR_SIZE 25
#define K_P_KEY 26
#define K_P_VALUE 27
#define K_P_INIT 28
__constant__ char k_names[29][16] = {"activationId", "invoker",    "isSystemError", "response",   "transid",
                                     "instance",     "uniqueName", "displayedName", "userMemory", "name",
                                     "namespace",    "name",       "subject",       "activationId", "start",
                                     "end",          "cause",      "response",      "logs",       "version",
                                     "publish",      "annotations", "duration",     "statusCode", "result",
                                     "size",         "key",        "value",         "init"};
__constant__ int k_len[29] = {12, 7, 13, 8, 7, 8, 10, 13, 10, 4, 9, 4, 7, 12, 5, 3, 5, 8, 4, 7, 7, 11, 8, 10, 6, 4, 3, 5, 4};

// bitmask of the candidate names (lo..hi) the decoded key equals
__device__ __forceinline__ int key_match(Win& W, int64_t k, int lo, int hi) {
    int64_t i = k + 1;
    uint32_t alive = ((1u << (hi + 1)) - 1u) & ~((1u << lo) - 1u);
    int n = 0;
    for (;;) {
        const int u = unit_at(W, i);
        if (u < 0) break;
        for (int c = lo; c <= hi; ++c)
            if (((alive >> c) & 1u) && (n >= k_len[c] || u != k_names[c][n])) alive &= ~(1u << c);
        ++n;
        if (!alive) return -1;
    }
    for (int c = lo; c <= hi; ++c)
        if (((alive >> c) & 1u) && n == k_len[c]) return c;
    return -1;
}

#define EV_ERR 1
#define EV_UNSUP 2

// string starting at i (the opening quote); returns the index after the closing quote, or -1 on a grammar error
__device__ __forceinline__ int64_t scan_string(Win& W, int64_t i) {
    ++i;
    for (;;) {
        const int c = W.at(i);
        if (c < 0x20) return -1;  // end of message (-1) or a raw control character
        if (c == '"') return i + 1;
        if (c == '\\') {
            const int e = W.at(i + 1);
            if (e == 'u') {
                if (hex_val(W.at(i + 2)) < 0 || hex_val(W.at(i + 3)) < 0 || hex_val(W.at(i + 4)) < 0 ||
                    hex_val(W.at(i + 5)) < 0)
                    return -1;
                i += 6;
            } else if (e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't') {
                i += 2;
            } else {
                return -1;
            }
        } else {
            ++i;
        }
    }
}

// number at i; returns the index after it, -1 on a grammar error, -2 for an exponent of more than 9 digits
__device__ __forceinline__ int64_t scan_number(Win& W, int64_t i) {
    if (W.at(i) == '-') ++i;
    int c = W.at(i);
    if (c == '0') ++i;
    else if (c >= '1' && c <= '9') {
        while ((c = W.at(i)) >= '0' && c <= '9') ++i;
    } else return -1;
    if (W.at(i) == '.') {
        ++i;
        const int64_t f = i;
        while ((c = W.at(i)) >= '0' && c <= '9') ++i;
        if (i == f) return -1;
    }
    c = W.at(i);
    if (c == 'e' || c == 'E') {
        ++i;
        c = W.at(i);
        if (c == '+' || c == '-') ++i;
        const int64_t f = i;
        while ((c = W.at(i)) >= '0' && c <= '9') ++i;
        if (i == f) return -1;
        if (i - f > 9) return -2;
    }
    return i;
}

// low 64 bits of the integer part of a validated number literal (BigDecimal -> BigInteger.longValue), significant
// digit count in *sig
__device__ __forceinline__ u64 number_bits(Win& W, int64_t i, int* sig) {
    bool neg = false;
    if (W.at(i) == '-') neg = true, ++i;
    const int64_t ib = i;
    int c;
    while ((c = W.at(i)) >= '0' && c <= '9') ++i;
    const int64_t ie = i;
    int64_t fb = i, fe = i;
    if (W.at(i) == '.') {
        fb = ++i;
        while ((c = W.at(i)) >= '0' && c <= '9') ++i;
        fe = i;
    }
    int64_t ex = 0;
    c = W.at(i);
    if (c == 'e' || c == 'E') {
        ++i;
        bool en = false;
        c = W.at(i);
        if (c == '+') ++i;
        else if (c == '-') en = true, ++i;
        while ((c = W.at(i)) >= '0' && c <= '9') ex = ex * 10 + (c - '0'), ++i;
        if (en) ex = -ex;
    }
    const int64_t ni = ie - ib, nf = fe - fb, nd = ni + nf;
    const int64_t shift = ex - nf;
    const int64_t keep = shift >= 0 ? nd : nd + shift;
    u64 v = 0;
    int s = 0;
    bool started = false;
    for (int64_t k = 0; k < nd; ++k) {
        const int d = W.at(k < ni ? ib + k : fb + (k - ni)) - '0';
        started |= d != 0;
        s += started;
        if (k < keep) v = v * 10ull + (u64)d;
    }
    if (shift > 0 && keep > 0)
        for (int64_t k = 0; k < shift && k < 64; ++k) v *= 10ull;
    *sig = s;
    return neg ? 0ull - v : v;
}

// skip one validated value at i (containers by depth counting, strings by scan_string)
__device__ __forceinline__ int64_t skip_value(Win& W, int64_t i) {
    int depth = 0;
    for (;;) {
        const int c = W.at(i);
        if (c == '"') i = scan_string(W, i);
        else if (c == '{' || c == '[') ++depth, ++i;
        else if (c == '}' || c == ']') --depth, ++i;
        else if (c == '-' || (c >= '0' && c <= '9')) i = scan_number(W, i);
        else if (c == 't' || c == 'n') i += 4;
        else if (c == 'f') i += 5;
        else ++i;  // ',' ':' whitespace inside a container
        if (depth == 0) return i;
    }
}

// ByteSize.fromString over the decoded string at a (Size.scala:119-138); *bytes = toBytes (Size.scala:28-62: size times
// 1, 2^10, 2^20 or 2^30 in wrapping Long arithmetic)
__device__ __forceinline__ bool bytesize(Win& W, int64_t a, long long* bytes) {
    int64_t i = a + 1;
    int st = 0, sh = 0;
    u64 val = 0;
    bool ovf = false;
    for (;;) {
        const int u = unit_at(W, i);
        if (u < 0) break;
        const bool ws = u == ' ' || u == '\t' || u == '\n' || u == 0x0B || u == '\f' || u == '\r';
        const bool dg = u >= '0' && u <= '9';
        const int U = (u >= 'a' && u <= 'z') ? u - 32 : u;
        const bool gmk = U == 'G' || U == 'M' || U == 'K';
        switch (st) {
            case 0: st = ws ? 1 : dg ? 2 : 9; if (dg) val = (u64)(u - '0'); break;
            case 1: st = dg ? 2 : 9; if (dg) val = (u64)(u - '0'); break;
            case 2:
                if (dg) {
                    if (val > (u64)(0x7FFFFFFFFFFFFFFFull - (u64)(u - '0')) / 10ull) ovf = true;
                    else val = val * 10ull + (u64)(u - '0');
                } else st = ws ? 3 : gmk ? 4 : U == 'B' ? 5 : 9;
                if (gmk) sh = U == 'K' ? 10 : U == 'M' ? 20 : 30;
                break;
            case 3:
                st = gmk ? 4 : U == 'B' ? 5 : 9;
                if (gmk) sh = U == 'K' ? 10 : U == 'M' ? 20 : 30;
                break;
            case 4: st = U == 'B' ? 5 : ws ? 6 : 9; break;
            case 5: st = ws ? 6 : 9; break;
            default: st = 9;
        }
        if (st == 9) return false;
    }
    *bytes = (long long)(val << sh);
    return (st == 4 || st == 5 || st == 6) && !ovf;
}

__device__ __forceinline__ bool num_start(int c) { return c == '-' || (c >= '0' && c <= '9'); }

// U+FFFF (EF BF BF) reads as spray-json's end-of-input marker: left to the JVM
__device__ __forceinline__ bool has_ffff(Win& W, int64_t b, int64_t e) {
    bool ffff = false;
    for (int64_t i = b; i + 2 < e && !ffff; ++i)
        ffff = W.at(i) == 0xEF && W.at(i + 1) == 0xBF && W.at(i + 2) == 0xBF;
    return ffff;
}

// The whole message [b, e) against the grammar; v[q] = where the value of the LAST top-level member named
// k_names[LO + q] starts (-1: no such member), top_obj = the root is an object.  0, EV_ERR or EV_UNSUP.
template <int LO, int HI>
__device__ __forceinline__ int scan_message(Win& W, int64_t b, int64_t e, int64_t (&v)[HI - LO + 1], bool& top_obj) {
    u64 stk = 0;  // bit d-1: container at depth d is an object
    int d = 0, ev = 0;
    int64_t i = b;
    while (is_ws(W.at(i))) ++i;
    top_obj = W.at(i) == '{';
    enum { VALUE, KEY, AFTER } st = VALUE;
    for (;;) {
        if (st == VALUE) {
            const int c = W.at(i);
            if (c == '{' || c == '[') {
                if (d == 64) { ev = EV_UNSUP; break; }
                stk = (stk & ~(1ull << d)) | ((u64)(c == '{') << d);
                ++d;
                ++i;
                while (is_ws(W.at(i))) ++i;
                const int c2 = W.at(i);
                if (c2 == (c == '{' ? '}' : ']')) { --d; ++i; st = AFTER; }
                else st = c == '{' ? KEY : VALUE;
                continue;
            }
            int64_t j;
            if (c == '"') j = scan_string(W, i);
            else if (num_start(c)) j = scan_number(W, i);
            else if (c == 't') j = (W.at(i + 1) == 'r' && W.at(i + 2) == 'u' && W.at(i + 3) == 'e') ? i + 4 : -1;
            else if (c == 'f') j = (W.at(i + 1) == 'a' && W.at(i + 2) == 'l' && W.at(i + 3) == 's' && W.at(i + 4) == 'e') ? i + 5 : -1;
            else if (c == 'n') j = (W.at(i + 1) == 'u' && W.at(i + 2) == 'l' && W.at(i + 3) == 'l') ? i + 4 : -1;
            else j = -1;
            if (j == -2) { ev = EV_UNSUP; break; }
            if (j < 0) { ev = EV_ERR; break; }
            i = j;
            st = AFTER;
        } else if (st == KEY) {
            if (W.at(i) != '"') { ev = EV_ERR; break; }
            const int64_t k = i;
            i = scan_string(W, i);
            if (i < 0) { ev = EV_ERR; break; }
            while (is_ws(W.at(i))) ++i;
            if (W.at(i) != ':') { ev = EV_ERR; break; }
            ++i;
            while (is_ws(W.at(i))) ++i;
            if (d == 1) {
                const int id = key_match(W, k, LO, HI);
#pragma unroll
                for (int q = 0; q <= HI - LO; ++q)  // constant indices: v stays in registers (no scratch)
                    if (id - LO == q) v[q] = i;
            }
            st = VALUE;
        } else {  // AFTER a value
            while (is_ws(W.at(i))) ++i;
            if (d == 0) {
                if (i != e) ev = EV_ERR;
                break;
            }
            const int c = W.at(i);
            const bool obj = (stk >> (d - 1)) & 1ull;
            if (c == ',') {
                ++i;
                while (is_ws(W.at(i))) ++i;
                st = obj ? KEY : VALUE;
            } else if (c == (obj ? '}' : ']')) {
                --d;
                ++i;
            } else {
                ev = EV_ERR;
                break;
            }
        }
    }
    return ev;
}

// InvokerInstanceId (jsonFormat4, InstanceId.scala:31-49) from the validated value at a: instance through
// BigDecimal.intValue, uniqueName / displayedName as Option[String], userMemory through ByteSize.fromString, its
// toBytes in mem.  Sets fail (deserializationError) / unsup (beyond the parser's limits), never clears them.
__device__ __forceinline__ void instance_id(Win& W, int64_t a, int& inst, long long& mem, bool& fail, bool& unsup) {
    mem = 0;
    if (W.at(a) != '{') fail = true;
    else {
        int64_t w[4] = {-1, -1, -1, -1};
        int64_t j = a + 1;
        while (is_ws(W.at(j))) ++j;
        if (W.at(j) != '}') {
            for (;;) {
                while (is_ws(W.at(j))) ++j;
                const int64_t k = j;
                j = scan_string(W, j);
                while (is_ws(W.at(j))) ++j;
                ++j;  // ':'
                while (is_ws(W.at(j))) ++j;
                const int id = key_match(W, k, K_INSTANCE, K_USERMEM);
#pragma unroll
                for (int q = 0; q < 4; ++q)  // constant indices: w stays in registers
                    if (id - K_INSTANCE == q) w[q] = j;
                j = skip_value(W, j);
                while (is_ws(W.at(j))) ++j;
                if (W.at(j) != ',') break;
                ++j;
            }
        }
        if (w[0] < 0 || !num_start(W.at(w[0]))) fail = true;
        else {
            int sg;
            inst = (int32_t)(uint32_t)number_bits(W, w[0], &sg);
            if (sg > 34) unsup = true;
        }
        for (int q = 1; q <= 2; ++q)
            if (w[q] >= 0 && W.at(w[q]) != '"' && W.at(w[q]) != 'n') fail = true;
        if (w[3] < 0 || W.at(w[3]) != '"' || !bytesize(W, w[3], &mem)) fail = true;
    }
}

// ActivationId.serdes.read on the validated JSON string at a (ActivationId.scala:58-95): 32 decoded units of [0-9a-f]
// -> the 128-bit key.  A wrong length or another ASCII unit is a deserializationError (fail); a non-ASCII unit may be a
// digit of Char.isDigit (ActivationId.scala:50) and is left to the JVM (unsup).  Both the CompletionMessage's
// `activationId` and a `response` that is a string (Left, Message.scala:231-233) go through here.
__device__ __forceinline__ void activation_id(Win& W, int64_t a, u64& hi, u64& lo, bool& fail, bool& unsup) {
    int64_t j = a + 1;
    int len = 0;
    bool bad = false, nonascii = false;
    for (;;) {
        const int u = unit_at(W, j);
        if (u < 0) break;
        nonascii |= u >= 0x80;
        const int h = (u >= '0' && u <= '9') ? u - '0' : (u >= 'a' && u <= 'f') ? u - 'a' + 10 : -1;
        if (h < 0) bad = true;
        else if (len < 16) hi = (hi << 4) | (u64)h;
        else if (len < 32) lo = (lo << 4) | (u64)h;
        ++len;
    }
    if (nonascii) unsup = true;
    else if (len != 32 || bad) fail = true;
}

// ------------------------------------------------------------------------------------------ accepted subset
// A `response` object (Right(WhiskActivation), Message.scala:235) is taken on the device only inside the accepted
// subset of include/owgs.h ("accepted subset of a response object"): a sufficient condition for
// convertTo[WhiskActivation] to succeed, checked over the raw bytes of the already validated message.  Every function
// returns false for anything outside its rule; the caller then reports OWGS_ACK_JVM, never FAIL.

// the member name at k (its opening quote) among k_names[lo..hi], compared byte by byte; a name written with an escape
// sets esc (and matches nothing)
__device__ __forceinline__ int key_match_raw(Win& W, int64_t k, int lo, int hi, bool& esc) {
    int64_t i = k + 1;
    uint32_t alive = ((1u << (hi + 1)) - 1u) & ~((1u << lo) - 1u);
    int n = 0;
    for (;;) {
        const int u = W.at(i);
        if (u == '"') break;
        if (u == '\\') {
            esc = true;
            return -1;
        }
        for (int c = lo; c <= hi; ++c)
            if (((alive >> c) & 1u) && (n >= k_len[c] || u != k_names[c][n])) alive &= ~(1u << c);
        ++n;
        ++i;
    }
    for (int c = lo; c <= hi; ++c)
        if (((alive >> c) & 1u) && n == k_len[c]) return c;
    return -1;
}

// -?(0|[1-9][0-9]{0,maxd-1}) and nothing more: no fraction, no exponent (the grammar has excluded leading zeros)
__device__ __forceinline__ bool int_literal(Win& W, int64_t a, int maxd) {
    if (W.at(a) == '-') ++a;
    int nd = 0, c;
    while ((c = W.at(a)) >= '0' && c <= '9') ++a, ++nd;
    return nd >= 1 && nd <= maxd && c != '.' && c != 'e' && c != 'E';
}

// a string of exactly 32 raw [0-9a-f] -> hi, lo
__device__ __forceinline__ bool hex32(Win& W, int64_t a, u64& hi, u64& lo) {
    if (W.at(a) != '"') return false;
    u64 h = 0, l = 0;
    bool ok = true;
    for (int k = 0; k < 32; ++k) {
        const int c = W.at(a + 1 + k);
        const int x = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : -1;
        ok &= x >= 0;
        if (!ok) break;  // (a closing quote stops the walk inside the string)
        if (k < 16) h = (h << 4) | (u64)x;
        else l = (l << 4) | (u64)x;
    }
    hi = h;
    lo = l;
    return ok && W.at(a + 33) == '"';
}

// EntityPath / EntityName (EntityPath.scala:141-162, 206, 222-224): printable ASCII without '"' and '\', split at '/'
// (sep; EntityName has no separator: '/' is outside its class) with the empty parts dropped; every part matches
// EntityName.REGEX -- first [A-Za-z0-9_], then [\w@ .&-], no trailing blank, at most 256 characters.  A path needs one
// part or more, a name exactly one.
__device__ __forceinline__ bool entity_parts(Win& W, int64_t a, bool sep) {
    if (W.at(a) != '"') return false;
    int parts = 0, len = 0, last = 0;
    bool ok = true;
    for (int64_t i = a + 1;; ++i) {
        const int c = W.at(i);
        if (c == '"' || (sep && c == '/')) {
            if (len > 0) {
                ok &= last != ' ' && len <= 256;
                ++parts;
                len = 0;
            }
            if (c == '"') break;
            continue;
        }
        const bool w = (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_';
        const bool mid = w || c == '@' || c == ' ' || c == '.' || c == '&' || c == '-';
        if (len == 0 ? !w : !mid) return false;  // also '\', bytes >= 0x80 and the end of the window (-1)
        last = c;
        ++len;
    }
    return ok && (sep ? parts >= 1 : parts == 1);
}

// a string of printable ASCII (0x20-0x7E) without '"' and '\'; *n its length, *first / *last its end characters,
// *nonblank whether a character other than ' ' occurs
__device__ __forceinline__ bool plain_string(Win& W, int64_t a, int* n, int* first, int* last, bool* nonblank) {
    if (W.at(a) != '"') return false;
    int len = 0, f = 0, l = 0;
    bool nb = false;
    for (int64_t i = a + 1;; ++i) {
        const int c = W.at(i);
        if (c == '"') break;
        if (c < 0x20 || c > 0x7E || c == '\\') return false;
        if (len == 0) f = c;
        l = c;
        nb |= c != ' ';
        ++len;
    }
    *n = len, *first = f, *last = l, *nonblank = nb;
    return true;
}

// SemVer (SemVer.scala:52-101): "major.minor.patch", each (0|[1-9][0-9]{0,8}) so that toInt succeeds, not 0.0.0
__device__ __forceinline__ bool semver(Win& W, int64_t a) {
    if (W.at(a) != '"') return false;
    int64_t i = a + 1;
    bool nonzero = false;
    for (int part = 0; part < 3; ++part) {
        int nd = 0, c, c0 = W.at(i);
        while ((c = W.at(i)) >= '0' && c <= '9') ++i, ++nd;
        if (nd < 1 || nd > 9 || (c0 == '0' && nd > 1)) return false;
        nonzero |= c0 != '0';
        if (c != (part < 2 ? '.' : '"')) return false;
        ++i;
    }
    return nonzero;
}

// The checks of container values walk them once and return the index after the value (-1: outside the rule), so that
// the caller does not scan the value again to get past it.

// ActivationLogs (ActivationLogs.scala:35): an array whose elements are all strings
__device__ __forceinline__ int64_t string_array(Win& W, int64_t a) {
    if (W.at(a) != '[') return -1;
    int64_t j = a + 1;
    while (is_ws(W.at(j))) ++j;
    if (W.at(j) == ']') return j + 1;
    for (;;) {
        while (is_ws(W.at(j))) ++j;
        if (W.at(j) != '"') return -1;
        j = scan_string(W, j);
        while (is_ws(W.at(j))) ++j;
        if (W.at(j) != ',') return j + 1;  // ']'
        ++j;
    }
}

// the members of the validated object at a, one call of f(id, value index) per member whose raw name is
// k_names[lo..hi] (id) or another name (-1).  f returns -1 (outside the rule), 0 (the value is fine or of no interest
// and has not been walked) or the index after the value.  Returns the index after the object, or -1 as soon as a name
// is escaped, one of lo..hi occurs twice or f returns -1.  seen = the names met (bit id - lo).
template <class F>
__device__ __forceinline__ int64_t object_members(Win& W, int64_t a, int lo, int hi, uint32_t& seen, F f) {
    seen = 0;
    int64_t j = a + 1;
    while (is_ws(W.at(j))) ++j;
    if (W.at(j) == '}') return j + 1;
    for (;;) {
        while (is_ws(W.at(j))) ++j;
        const int64_t k = j;
        j = scan_string(W, j);
        while (is_ws(W.at(j))) ++j;
        ++j;  // ':'
        while (is_ws(W.at(j))) ++j;
        bool esc = false;
        const int id = key_match_raw(W, k, lo, hi, esc);
        if (esc) return -1;
        if (id >= 0) {
            const uint32_t bit = 1u << (id - lo);
            if (seen & bit) return -1;
            seen |= bit;
        }
        const int64_t r = f(id, j);
        if (r < 0) return -1;
        j = r > 0 ? r : skip_value(W, j);
        while (is_ws(W.at(j))) ++j;
        if (W.at(j) != ',') return j + 1;  // '}'
        ++j;
    }
}

// ActivationResponse (jsonFormat3, ActivationResult.scala:30-32, 249): statusCode an Int literal, size absent, null or
// one, result anything
__device__ __forceinline__ int64_t activation_response(Win& W, int64_t a) {
    if (W.at(a) != '{') return -1;
    uint32_t seen;
    const int64_t end = object_members(W, a, K_AR_STATUS, K_AR_SIZE, seen, [&](int id, int64_t j) -> int64_t {
        if (id == K_AR_STATUS) return int_literal(W, j, 9) ? 0 : -1;
        if (id == K_AR_SIZE) return (W.at(j) == 'n' || int_literal(W, j, 9)) ? 0 : -1;
        return 0;
    });
    return (seen & 1u) ? end : -1;
}

// Parameters.serdes.read (Parameter.scala:240-268): an array of objects, each with one "key" (a plain string with a
// non-blank character), one "value" and at most one "init", a boolean
__device__ __forceinline__ int64_t annotations(Win& W, int64_t a) {
    if (W.at(a) != '[') return -1;
    int64_t j = a + 1;
    while (is_ws(W.at(j))) ++j;
    if (W.at(j) == ']') return j + 1;
    for (;;) {
        while (is_ws(W.at(j))) ++j;
        if (W.at(j) != '{') return -1;
        uint32_t seen;
        j = object_members(W, j, K_P_KEY, K_P_INIT, seen, [&](int id, int64_t q) -> int64_t {
            if (id == K_P_KEY) {
                int n, f, l;
                bool nb;
                return (plain_string(W, q, &n, &f, &l, &nb) && nb) ? 0 : -1;
            }
            if (id == K_P_INIT) return (W.at(q) == 't' || W.at(q) == 'f') ? 0 : -1;
            return 0;
        });
        if (j < 0 || (seen & 3u) != 3u) return -1;
        while (is_ws(W.at(j))) ++j;
        if (W.at(j) != ',') return j + 1;  // ']'
        ++j;
    }
}

// WhiskActivation (jsonFormat13, WhiskActivation.scala:52-64, 182) inside the accepted subset: the index after the
// object (-1: outside the subset); hi / lo = its activationId
__device__ __forceinline__ int64_t whisk_activation(Win& W, int64_t a, u64& hi, u64& lo) {
    uint32_t seen;
    const int64_t end = object_members(W, a, K_WA_NAMESPACE, K_WA_DURATION, seen, [&](int id, int64_t j) -> int64_t {
        bool ok = true;
        if (id == K_WA_NAMESPACE) ok = entity_parts(W, j, true);
        else if (id == K_WA_NAME) ok = entity_parts(W, j, false);
        else if (id == K_WA_SUBJECT) {  // Subject.scala:46-67 behind ArgNormalizer.apply: trim is the identity
            int n, f, l;
            bool nb;
            ok = plain_string(W, j, &n, &f, &l, &nb) && n >= 5 && f != ' ' && l != ' ';
        } else if (id == K_WA_AID) ok = hex32(W, j, hi, lo);
        else if (id == K_WA_CAUSE) {
            u64 ch, cl;
            ok = W.at(j) == 'n' || hex32(W, j, ch, cl);
        } else if (id == K_WA_START || id == K_WA_END) ok = int_literal(W, j, 18);  // WhiskActivation.scala:161-168
        else if (id == K_WA_DURATION) ok = W.at(j) == 'n' || int_literal(W, j, 18);
        else if (id == K_WA_RESPONSE) return activation_response(W, j);
        else if (id == K_WA_LOGS) return string_array(W, j);
        else if (id == K_WA_VERSION) ok = semver(W, j);
        else if (id == K_WA_PUBLISH) ok = W.at(j) == 't' || W.at(j) == 'f';
        else if (id == K_WA_ANNOTATIONS) return annotations(W, j);
        return ok ? 0 : -1;
    });
    const uint32_t need = 0x1FFFu & ~(1u << (K_WA_CAUSE - K_WA_NAMESPACE)) & ~(1u << (K_WA_DURATION - K_WA_NAMESPACE));
    return (seen & need) == need ? end : -1;
}

template <bool RESULTS> struct OwgsAckParseSel { typedef OwgsAckParseArgs type; };
template <> struct OwgsAckParseSel<true> { typedef OwgsAckParseResultArgs type; };

// RESULTS = false: the parser of owgs_process_acks* (a `response` member: OWGS_ACK_JVM).  RESULTS = true:
// owgs_process_result_acks, which classifies those messages too (include/owgs.h).
template <bool RESULTS>
__global__ __launch_bounds__(256) void owgs_ack_parse_kernel(typename OwgsAckParseSel<RESULTS>::type A) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= A.n) return;
    const int64_t b = A.off[m], e = A.off[m + 1];
    Win W(A.bytes, b, e);
    int kind = OWGS_ACK_FAIL, inst = -1, sys = 0, health = 0;
    int result = 0, right = 0;  // RESULTS: the message has a `response` member; it is an object
    int64_t resp = 0, resp_end = 0;
    u64 hi = 0, lo = 0;
    if (has_ffff(W, b, e)) {
        kind = OWGS_ACK_UNSUPPORTED;
    } else {
        // ---------------------------------------------------------------- phase 1: grammar, top-level members
        int64_t v[5] = {-1, -1, -1, -1, -1};
        bool top_obj;
        const int ev = scan_message<K_AID, K_TID>(W, b, e, v, top_obj);
        if (ev == EV_UNSUP) kind = OWGS_ACK_UNSUPPORTED;
        else if (ev == EV_ERR || !top_obj) kind = OWGS_ACK_FAIL;
        else if (!RESULTS && v[K_RESP] >= 0) kind = OWGS_ACK_JVM;
        else if (v[K_INV] < 0 && (!RESULTS || v[K_RESP] < 0)) kind = OWGS_ACK_FAIL;
        else {
            // ------------------------------------------------------------ phase 2: the members of the message type
            // CompletionMessage (jsonFormat4, Message.scala:208-209); with RESULTS and a `response` member a
            // CombinedCompletionAndResultMessage (jsonFormat4, Message.scala:191-193: `invoker` present) or a
            // ResultMessage (jsonFormat2, Message.scala:221), whose id is the response's
            const bool has_resp = RESULTS && v[K_RESP] >= 0, has_inv = !RESULTS || v[K_INV] >= 0;
            bool fail = v[K_TID] < 0, unsup = false, jvm = false;
            if (has_resp) {
                const int c = W.at(v[K_RESP]);
                if (c == '"') {  // Left (Message.scala:231-233)
                    activation_id(W, v[K_RESP], hi, lo, fail, unsup);
                    resp_end = scan_string(W, v[K_RESP]);
                } else if (c == '{') {  // Right (Message.scala:235); the check's walk gives the value's end
                    right = 1;
                    resp_end = whisk_activation(W, v[K_RESP], hi, lo);
                    jvm = resp_end < 0;
                } else {
                    fail = true;  // Message.scala:236
                }
                result = 1;
            } else if (v[K_AID] >= 0) {
                const int64_t a = v[K_AID];
                const int c = W.at(a);
                if (c == '"') activation_id(W, a, hi, lo, fail, unsup);
                else if (num_start(c)) unsup = true;
                else fail = true;
            } else {
                fail = true;
            }
            if (has_inv && v[K_SYS] >= 0) {
                const int c = W.at(v[K_SYS]);
                if (c == 't') sys = 1;
                else if (c != 'f' && c != 'n') fail = true;
            }
            if (has_inv) {
                long long mem;
                instance_id(W, v[K_INV], inst, mem, fail, unsup);
            }
            if (has_inv && v[K_TID] >= 0 && W.at(v[K_TID]) == '[') {
                int64_t el[3] = {-1, -1, -1};
                int ne = 0;
                int64_t j = v[K_TID] + 1;
                while (is_ws(W.at(j))) ++j;
                if (W.at(j) != ']') {
                    for (;;) {
                        while (is_ws(W.at(j))) ++j;
#pragma unroll
                        for (int q = 0; q < 3; ++q)  // constant indices: el stays in registers
                            if (ne == q) el[q] = j;
                        ++ne;
                        j = skip_value(W, j);
                        while (is_ws(W.at(j))) ++j;
                        if (W.at(j) != ',') break;
                        ++j;
                    }
                }
                if ((ne == 2 || ne == 3) && W.at(el[0]) == '"' && num_start(W.at(el[1])) &&
                    (ne == 2 || W.at(el[2]) == 't' || W.at(el[2]) == 'f')) {
                    // "sid_invokerHealth"
                    int64_t q = el[0] + 1;
                    const char* H = "sid_invokerHealth";
                    bool eq = true;
                    int n = 0;
                    for (;;) {
                        const int u = unit_at(W, q);
                        if (u < 0) break;
                        if (n >= 17 || u != H[n]) eq = false;
                        ++n;
                    }
                    if (eq && n == 17) {
                        int sg;
                        const u64 s0 = number_bits(W, el[1], &sg);
                        if (sg > 34) unsup = true;
                        health = ((int64_t)s0 == A.health_start_ms) && (ne == 2 || W.at(el[2]) == 'f');
                    }
                }
            }
            // an object outside the subset stays the JVM's whatever else the message holds; then FAIL before UNSUPPORTED
            kind = jvm ? OWGS_ACK_JVM
                       : fail ? OWGS_ACK_FAIL
                              : unsup ? OWGS_ACK_UNSUPPORTED : has_inv ? OWGS_ACK_COMPLETION : OWGS_ACK_RESULT_MSG;
            if (RESULTS) resp = v[K_RESP];
        }
    }
    if (kind != OWGS_ACK_COMPLETION) sys = health = 0;  // only a parsed CompletionMessage carries them
    A.key[m] = make_ulonglong2(hi, lo);
    A.inst[m] = inst;
    if constexpr (RESULTS) {
        // an accepted message with a result: the span of its `response` value in the caller's bytes[], and the two
        // free bits of the record (3: carries a result, 7: the result is an object)
        const bool acc = result && (kind == OWGS_ACK_COMPLETION || kind == OWGS_ACK_RESULT_MSG);
        A.resp_off[m] = acc ? resp + A.off_base : 0;
        A.resp_len[m] = acc ? (int32_t)(resp_end - resp) : 0;
        A.info[m] = (uint8_t)(kind | (sys << 4) | (health << 5) | (acc ? 8 | (right << 7) : 0));
    } else {
        A.info[m] = (uint8_t)(kind | (sys << 4) | (health << 5) | (A.forced ? (A.forced[m] & 1) << 6 : 0));
    }
}

// PingMessage.parse (Message.scala:261-268: jsonFormat(PingMessage.apply _, "name")) for the raw messages of the
// `health` topic (InvokerPool.processInvokerPing, ISUP:174-185), one thread per message: the scanner and the
// InvokerInstanceId conversion of the ack parser above, with its limits.  kind = OWGS_PING_*; instance for FED / RANGE,
// userMemory.toBytes for FED, 0 otherwise.
__global__ __launch_bounds__(256) void owgs_ping_parse_kernel(const uint8_t* bytes, const int64_t* off, int32_t n,
                                                              uint8_t* out_kind, int32_t* out_inst,
                                                              long long* out_mem) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    const int64_t b = off[m], e = off[m + 1];
    Win W(bytes, b, e);
    int kind = OWGS_PING_FAIL, inst = 0;
    long long mem = 0;
    if (has_ffff(W, b, e)) {
        kind = OWGS_PING_UNSUPPORTED;
    } else {
        int64_t v[1] = {-1};
        bool top_obj;
        const int ev = scan_message<K_NAME, K_NAME>(W, b, e, v, top_obj);
        if (ev == EV_UNSUP) kind = OWGS_PING_UNSUPPORTED;
        else if (ev == EV_ERR || !top_obj || v[0] < 0) kind = OWGS_PING_FAIL;
        else {
            bool fail = false, unsup = false;
            instance_id(W, v[0], inst, mem, fail, unsup);
            kind = fail ? OWGS_PING_FAIL
                        : unsup ? OWGS_PING_UNSUPPORTED
                                : (inst >= 0 && inst < OWGS_HEALTH_MAX_ID_V) ? OWGS_PING_FED : OWGS_PING_RANGE;
        }
    }
    out_kind[m] = (uint8_t)kind;
    out_inst[m] = (kind == OWGS_PING_FED || kind == OWGS_PING_RANGE) ? inst : 0;
    out_mem[m] = kind == OWGS_PING_FED ? mem : 0;
}

// 32 hex chars per id (caller-side ActivationId strings) -> 128-bit keys; ids that are not 32 x [0-9a-f] get
// info = OWGS_ACK_FAIL (the caller's bug: ActivationId guarantees the format)
__global__ __launch_bounds__(256) void owgs_aid_decode_kernel(const char* aid32, int32_t n, const uint8_t* cflags,
                                                              ulonglong2* key, uint8_t* info, int32_t* inst,
                                                              const int32_t* inv) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    u64 hi = 0, lo = 0;
    bool bad = false;
    for (int k = 0; k < 32; ++k) {
        const int c = (uint8_t)aid32[(size_t)m * 32 + k];
        const int h = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : -1;
        bad |= h < 0;
        if (k < 16) hi = (hi << 4) | (u64)(h & 15);
        else lo = (lo << 4) | (u64)(h & 15);
    }
    key[m] = make_ulonglong2(hi, lo);
    if (info) {
        const uint8_t f = cflags ? cflags[m] : 0;  // bit0 forced, bit1 isSystemError, bit2 transid == invokerHealth
        info[m] = (uint8_t)((bad ? OWGS_ACK_FAIL : OWGS_ACK_COMPLETION) | ((f >> 1) & 1) << 4 | ((f >> 2) & 1) << 5 |
                            (f & 1) << 6);
        inst[m] = inv[m];
    }
}

// ------------------------------------------------------------------------------------------ activation table
__device__ __forceinline__ u64 aid_hash(ulonglong2 k) {
    u64 x = k.x * 0x9E3779B97F4A7C15ull ^ k.y;
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    return x;
}
__device__ __forceinline__ bool keq(ulonglong2 a, ulonglong2 b) { return a.x == b.x && a.y == b.y; }

#define TW_EMPTY 0ull
#define TW_READY OWGS_TW_READY
#define TW_TOMB 2ull
#define TW_CLAIM (1ull << 63)

// ------------------------------------------------------------------------------------------ in-flight books
// activationsPerNamespace(h) += delta (CLB:127 / CLB:283) for every lane whose h is a namespace handle; every lane of
// the wave calls it (lanes without an item pass OWGS_NONE_V).
// Wave-level aggregation: the lanes holding one handle elect their lowest lane, which adds the group's size (a hot
// namespace takes a large share of a batch: one atomic per wave on its word instead of one per item).  The plain
// form, one no-return atomic per lane, was measured beside it and dropped: on 50,000 ids of the headline draw (1,000
// namespaces, the hottest 10 % of the batch) it cost the completion call 48 us against 5 us.
__device__ __forceinline__ void ns_count(int32_t* active, int h, int delta) {
    const int lane = (int)(threadIdx.x & 63);
    u64 todo = __ballot(h != OWGS_NONE_V);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int hl = __shfl(h, leader);
        const u64 grp = __ballot(h == hl);
        if (lane == leader) atomicAdd(&active[hl], delta * __popcll(grp));
        todo &= ~grp;
    }
}

// the call's memory words: megabytes of the items it counted, managed and blackbox (CLB:123-125 / CLB:281-283), as a
// block reduction and one atomic per block and word; every thread of the block calls it (mb = 0 without an item)
__device__ __forceinline__ void mb_totals_add(unsigned long long* counters, int mb, bool bb) {
    __shared__ u64 red[2][4];
    u64 m = bb ? 0ull : (u64)(long long)mb, b = bb ? (u64)(long long)mb : 0ull;
    for (int o = 32; o; o >>= 1) {
        m += __shfl_xor(m, o);
        b += __shfl_xor(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = m;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (m) atomicAdd(&counters[OWGS_CNT_MANAGED_MB], m);
        if (b) atomicAdd(&counters[OWGS_CNT_BLACKBOX_MB], b);
    }
}

// track step 1: find or claim a slot for every id of the batch.  placed (null: every item) is the predicate of
// owgs_publish_activations: an item without an invoker skips setupActivation altogether (SCPB:292-304), so it claims
// nothing, owns no slot and -- unlike state 3 below -- is not counted by the fill kernel (state 4).
__global__ __launch_bounds__(256) void owgs_act_claim_kernel(OwgsActTable T, const ulonglong2* key, int32_t n,
                                                             const uint8_t* info, const uint8_t* placed,
                                                             int32_t* slot, uint8_t* state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (placed && !placed[i]) {
        slot[i] = -1;
        state[i] = 4;
        return;
    }
    if (info && (info[i] & 7) != OWGS_ACK_COMPLETION) {
        slot[i] = -1;
        state[i] = 3;
        return;
    }
    const ulonglong2 k = key[i];
    const u64 mask = (u64)T.cap - 1;
    u64 s = aid_hash(k) & mask;
    for (u64 probes = 0; probes <= mask; ++probes) {
        u64 w = __hip_atomic_load(&T.tw[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == TW_EMPTY) {
            const u64 old = atomicCAS(&T.tw[s], TW_EMPTY, TW_CLAIM | (u64)i);
            if (old == TW_EMPTY) {
                slot[i] = (int32_t)s;
                state[i] = 0;  // claimed in this batch
                atomicMin(&T.owner[s], i);
                return;
            }
            w = old;
        }
        if (w == TW_READY) {
            if (keq(T.tk[s], k)) {
                slot[i] = (int32_t)s;
                state[i] = 1;  // existed before the batch
                return;
            }
        } else if (w & TW_CLAIM) {
            const int j = (int)(w & 0x7FFFFFFFull);
            if (keq(key[j], k)) {
                slot[i] = (int32_t)s;
                state[i] = 0;
                atomicMin(&T.owner[s], i);
                return;
            }
        }
        s = (s + 1) & mask;
    }
    slot[i] = -1;  // table full: the host keeps the load under one half, so this is unreachable
    state[i] = 3;
}

// track step 2: the lowest batch index of each claimed slot writes the entry (getOrElseUpdate in array order), its
// namespace included: the entry keeps the namespace and action of its first tracker (CLB:148-166).
// Every item is counted, duplicates too: setupActivation increments totalActivations, the memory total of the action's
// pool and activationsPerNamespace (CLB:121-127) BEFORE activationSlots.getOrElseUpdate (CLB:148), so an id that
// already has an entry leaks one count in the reference -- and here.  (totalActivations += n is the host's.)
__global__ __launch_bounds__(256) void owgs_act_fill_kernel(OwgsActTable T, const ulonglong2* key, int32_t n,
                                                            const int32_t* action, const int32_t* ns,
                                                            const int32_t* ticket, const int32_t* slot,
                                                            const uint8_t* state, const uint8_t* placed,
                                                            int32_t* out_ticket, uint8_t* out_existed,
                                                            unsigned long long* counters, OwgsInflight F, OwgsArm A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int h = OWGS_NONE_V, mb = 0;
    bool bb = false;
    // an item the gate did not place moves no counter and keeps the outputs the gate wrote; its lane still takes part
    // in the wave / block reductions below with OWGS_NONE_V and 0 MB
    if (i < n && (!placed || placed[i])) {
        const int a = action[i];
        h = ns ? ns[i] : OWGS_NONE_V;  // msg.user.namespace.uuid's handle (CLB:127)
        mb = F.act_mem[a];           // action.limits.memory.megabytes (CLB:125)
        bb = F.act_bb[a] != 0;       // action.exec.pull (CLB:122)
        const int s = slot[i];
        if (s < 0) {
            out_existed[i] = 2;
            out_ticket[i] = -1;
        } else if (state[i] == 1) {
            out_existed[i] = 1;
            out_ticket[i] = T.tv[s].y;
        } else {
            const int o = T.owner[s];
            if (o == i) {
                T.tk[s] = key[i];
                T.tv[s] = make_int2(a, ticket[i]);
                T.tn[s] = h;
                // the item that creates the entry arms its timer (the by-name block of getOrElseUpdate, CLB:148-152)
                long long d = OWGS_NO_DEADLINE;
                if (A.inv) {
                    const long long tl = A.tl[i];
                    d = A.now + (tl > A.std_ms ? tl : A.std_ms) * A.factor + A.addon;  // CLB:103-105
                    atomicMin(&T.tmin[s >> OWGS_TILE_LOG2], d);
                }
                T.td[s] = d;
                T.ti[s] = A.inv ? A.inv[i] : -1;
                T.tq[s] = A.seq_base + (u64)i;
                out_existed[i] = 0;
                out_ticket[i] = ticket[i];
                atomicAdd(&counters[OWGS_CNT_INSERTED], 1ull);
            } else {
                out_existed[i] = 1;
                out_ticket[i] = ticket[o];
            }
        }
    }
    ns_count(F.active, h, 1);
    mb_totals_add(counters, mb, bb);
}

// track step 3: publish the claimed slots and reset the owner words
__global__ __launch_bounds__(256) void owgs_act_publish_kernel(OwgsActTable T, int32_t n, const int32_t* slot,
                                                               const uint8_t* state, const uint8_t* placed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (placed && !placed[i])) return;
    const int s = slot[i];
    if (s < 0 || state[i] != 0 || T.owner[s] != i) return;
    T.tw[s] = TW_READY;
    T.owner[s] = 0x7FFFFFFF;
}

// completion step 1: find each message's entry; the lowest message index of an entry removes it.  results != 0: a
// result-only record (OWGS_ACK_RESULT_MSG) finds its entry too, without a claim on it: it removes nothing
__global__ __launch_bounds__(256) void owgs_act_find_kernel(OwgsActTable T, const ulonglong2* key, int32_t n,
                                                            const uint8_t* info, int32_t* slot, int32_t results) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    const int kd = info[i] & 7;
    if (results && kd == OWGS_ACK_RESULT_MSG) {
        const ulonglong2 k = key[i];
        const u64 mask = (u64)T.cap - 1;
        u64 s = aid_hash(k) & mask;
        for (u64 probes = 0; probes <= mask; ++probes) {
            const u64 w = T.tw[s];
            if (w == TW_EMPTY) break;
            if (w == TW_READY && keq(T.tk[s], k)) {
                r = (int)s;
                break;
            }
            s = (s + 1) & mask;
        }
    } else if (kd == OWGS_ACK_COMPLETION) {
        const ulonglong2 k = key[i];
        const u64 mask = (u64)T.cap - 1;
        u64 s = aid_hash(k) & mask;
        for (u64 probes = 0; probes <= mask; ++probes) {
            const u64 w = T.tw[s];
            if (w == TW_EMPTY) break;
            if (w == TW_READY && keq(T.tk[s], k)) {
                r = (int)s;
                atomicMin(&T.owner[s], i);
                break;
            }
            s = (s + 1) & mask;
        }
    }
    slot[i] = r;
}

// completion step 2: processCompletion outcome + releaseInvoker record (CLB:286-345, SCPB:327-331).  A message that
// removes its entry (OWGS_ACK_RELEASED) also takes the entry out of the in-flight books with the ENTRY's values, not
// the message's (CLB:280-284: totalActivations.decrement, the memory total of entry.isBlackbox by entry.memoryLimit,
// activationsPerNamespace.get(entry.namespaceId).foreach(_.decrement())); no other outcome touches a counter.
// (totalActivations -= entries removed is the host's.)
__global__ __launch_bounds__(256) void owgs_ack_resolve_kernel(OwgsActTable T, int32_t n, const uint8_t* info,
                                                               const int32_t* inst, const int32_t* slot,
                                                               const int32_t* act_mem, const int32_t* act_maxc,
                                                               const int32_t* act_slot, int32_t n_slots,
                                                               int32_t* r_inv, int32_t* r_mem, int32_t* r_maxc,
                                                               int32_t* r_slot, uint8_t* out_kind,
                                                               int32_t* out_ticket, unsigned long long* counters,
                                                               OwgsInflight F, int32_t results) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int h = OWGS_NONE_V, mb = 0;
    bool bb = false;
    if (i < n) {
        const int k = info[i] & 7;
        const int s = slot[i];
        int outk = k, tk = -1, ri = 0x7FFFFFFF, rm = 1, rc = 1, rs = 0;
        if (results && k == OWGS_ACK_RESULT_MSG) {
            // processResult (CLB:235-243) looks the id up at the message's turn: the entry was there when the batch
            // began and no message before this one removes it (owner = the lowest index that does, INT_MAX: none).
            // Nothing is removed, released or counted: the lane enters the reductions below with the neutral values.
            if (s >= 0 && T.owner[s] > i) tk = T.tv[s].y;
        } else if (k == OWGS_ACK_COMPLETION) {
            if (s >= 0 && T.owner[s] == i) {
                const int2 v = T.tv[s];
                outk = OWGS_ACK_RELEASED;
                tk = v.y;
                const int inv = inst[i];
                ri = (inv >= 0 && inv < n_slots) ? inv : 0x7FFFFFFF;  // invokerSlots.lift(invoker.toInt)
                rm = act_mem[v.x];
                rc = act_maxc[v.x];
                rs = act_slot[v.x];
                atomicAdd(&counters[OWGS_CNT_REMOVED], 1ull);
                h = T.tn[s];               // entry.namespaceId (CLB:283)
                mb = rm;                   // entry.memoryLimit.toMB (CLB:282)
                bb = F.act_bb[v.x] != 0;   // entry.isBlackbox (CLB:281)
            } else if ((info[i] >> 5) & 1) {
                outk = OWGS_ACK_HEALTH;  // None if tid == TransactionId.invokerHealth (CLB:320-328)
            } else {
                outk = ((info[i] >> 6) & 1) ? OWGS_ACK_FORCED_NOENTRY : OWGS_ACK_NOENTRY;  // CLB:329-345
            }
        }
        r_inv[i] = ri;
        r_mem[i] = rm;
        r_maxc[i] = rc;
        r_slot[i] = rs;
        out_kind[i] = (uint8_t)outk;
        out_ticket[i] = tk;
    }
    ns_count(F.active, h, -1);
    mb_totals_add(counters, mb, bb);
}

// completion step 3: tombstone removed entries, reset owner words
__global__ __launch_bounds__(256) void owgs_act_remove_kernel(OwgsActTable T, int32_t n, const int32_t* slot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slot[i];
    if (s < 0 || T.owner[s] != i) return;
    T.tw[s] = TW_TOMB;
    T.owner[s] = 0x7FFFFFFF;
}

// out_flags = isSystemError | release flags << 1.  out_aid != null (owgs_process_result_acks): also the record's
// result bits as OWGS_ACKF_RESULT / OWGS_ACKF_RIGHT, and the id of every accepted message (hi, lo), 0 for the others
__global__ __launch_bounds__(256) void owgs_ack_flags_kernel(int32_t n, const uint8_t* info, const uint8_t* rflags,
                                                             const uint8_t* out_kind, uint8_t* out_flags,
                                                             const ulonglong2* key, unsigned long long* out_aid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool rel = out_kind[i] == OWGS_ACK_RELEASED;
    int f = ((info[i] >> 4) & 1) | (rel ? (rflags[i] & 3) << 1 : 0);
    if (out_aid) {
        f |= ((info[i] >> 3) & 1) << 3 | ((info[i] >> 7) & 1) << 4;
        const bool acc = out_kind[i] >= OWGS_ACK_RELEASED;
        const ulonglong2 k = key[i];
        out_aid[2 * (size_t)i] = acc ? k.x : 0ull;
        out_aid[2 * (size_t)i + 1] = acc ? k.y : 0ull;
    }
    out_flags[i] = (uint8_t)f;
}

// rehash live entries into a fresh table (all keys distinct: plain CAS insertion); the namespace, the deadline, the
// entry's invoker and the arm sequence travel with the entry, and the new table's deadline summary is built as arming
// builds it
__global__ __launch_bounds__(256) void owgs_act_rehash_kernel(OwgsActTable O, OwgsActTable T) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= O.cap || O.tw[s] != TW_READY) return;
    const ulonglong2 k = O.tk[s];
    const u64 mask = (u64)T.cap - 1;
    u64 t = aid_hash(k) & mask;
    for (;;) {
        if (atomicCAS(&T.tw[t], TW_EMPTY, TW_READY) == TW_EMPTY) {
            T.tk[t] = k;
            T.tv[t] = O.tv[s];
            T.tn[t] = O.tn[s];
            const long long d = O.td[s];
            T.td[t] = d;
            T.ti[t] = O.ti[s];
            T.tq[t] = O.tq[s];
            if (d != OWGS_NO_DEADLINE) atomicMin(&T.tmin[t >> OWGS_TILE_LOG2], d);
            return;
        }
        t = (t + 1) & mask;
    }
}

__global__ __launch_bounds__(256) void owgs_act_init_kernel(OwgsActTable T) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= T.cap) return;
    T.tw[s] = TW_EMPTY;
    T.owner[s] = 0x7FFFFFFF;
    if ((s & (OWGS_TILE - 1)) == 0) T.tmin[s >> OWGS_TILE_LOG2] = OWGS_NO_DEADLINE;
}

// ------------------------------------------------------------------------------------------ launchers
#define GRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st

extern "C" hipError_t owgs_launch_ack_parse(const OwgsAckParseArgs* a, hipStream_t st) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ack_parse_kernel<false>, GRID(a->n), *a);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_ack_parse_results(const OwgsAckParseResultArgs* a, hipStream_t st) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ack_parse_kernel<true>, GRID(a->n), *a);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_ping_parse(const uint8_t* bytes, const int64_t* off, int32_t n, uint8_t* out_kind,
                                             int32_t* out_inst, long long* out_mem, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ping_parse_kernel, GRID(n), bytes, off, n, out_kind, out_inst, out_mem);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_aid_decode(const char* aid32, int32_t n, const uint8_t* cflags, ulonglong2* key,
                                             uint8_t* info, int32_t* inst, const int32_t* inv, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_aid_decode_kernel, GRID(n), aid32, n, cflags, key, info, inst, inv);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_act_init(const OwgsActTable* T, hipStream_t st) {
    hipLaunchKernelGGL(owgs_act_init_kernel, GRID(T->cap), *T);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_act_rehash(const OwgsActTable* O, const OwgsActTable* T, hipStream_t st) {
    hipLaunchKernelGGL(owgs_act_rehash_kernel, GRID(O->cap), *O, *T);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_act_track(const OwgsActTable* T, const ulonglong2* key, int32_t n,
                                            const int32_t* action, const int32_t* ns, const int32_t* ticket,
                                            int32_t* slot, uint8_t* state, int32_t* out_ticket, uint8_t* out_existed,
                                            unsigned long long* counters, const OwgsInflight* F, const OwgsArm* arm,
                                            const uint8_t* placed, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_act_claim_kernel, GRID(n), *T, key, n, (const uint8_t*)nullptr, placed, slot, state);
    hipLaunchKernelGGL(owgs_act_fill_kernel, GRID(n), *T, key, n, action, ns, ticket, slot, state, placed, out_ticket,
                       out_existed, counters, *F, *arm);
    hipLaunchKernelGGL(owgs_act_publish_kernel, GRID(n), *T, n, slot, state, placed);
    return hipGetLastError();
}

// find + resolve: afterwards r_* hold the release records for owgs_release_seq_kernel (message order)
extern "C" hipError_t owgs_launch_ack_complete(const OwgsActTable* T, const OwgsAckCompleteArgs* a, hipStream_t st) {
    if (a->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_act_find_kernel, GRID(a->n), *T, a->key, a->n, a->info, a->slot, a->results);
    hipLaunchKernelGGL(owgs_ack_resolve_kernel, GRID(a->n), *T, a->n, a->info, a->inst, a->slot, a->act_mem,
                       a->act_maxc, a->act_slot, a->n_slots, a->r_inv, a->r_mem, a->r_maxc, a->r_slot, a->out_kind,
                       a->out_ticket, a->counters, a->fl, a->results);
    hipLaunchKernelGGL(owgs_act_remove_kernel, GRID(a->n), *T, a->n, a->slot);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_ack_flags(int32_t n, const uint8_t* info, const uint8_t* rflags,
                                            const uint8_t* out_kind, uint8_t* out_flags, const ulonglong2* key,
                                            unsigned long long* out_aid, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ack_flags_kernel, GRID(n), n, info, rflags, out_kind, out_flags, key, out_aid);
    return hipGetLastError();
}
