// owgs_events.hip -- the throttle gate's user events and rejection texts on the device.
//
// Replaces, for a drained batch, the two per-item outputs of checkThrottleOverload (Entitlement.scala:383-420):
//   EventMessage(source, Metric(name, value), subject, namespace, userId, "Metric", timestamp).serialize
//       Message.scala:404-418 (jsonFormat7 + compactPrint; the wire order of the seven members is the HashMap's)
//   limit.errorMsg = Messages.tooManyRequests / tooManyConcurrentRequests(count, allowed)
//       ActivationThrottler.scala:58-67, ErrorResponse.scala:70-75
// Both are pure functions of the gate's outputs for the item and of a timestamp; the pieces that do not change per
// item (the source, the identity's members) arrive printed, so there is no escaping work here, and the outputs are by
// item, so there is no sort.
//
// Kernels (HBM-bound byte work; no MFMA):
//   owgs_evt_size_kernel     one thread per item: class of the item, event length, text length, the two counts
//   hipcub exclusive sums    ev_off / rej_off over n + 1 lengths (entry n = the bytes needed)
//   owgs_evt_write_kernel    one wave per item: literals and pieces copied by the 64 lanes, numbers printed one
//                            character per lane; a region whose bytes exceed its cap is not written
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stdint.h>

#include "owgs_device.h"
#include "owgs_internal.h"
#include "owgs_launch.h"

#define LIT(s) (int)(sizeof(s) - 1)
#define E_HEAD "{\"body\":{\"metricName\":\""
#define E_VALUE "\",\"metricValue\":"
#define E_SOURCE "},\"eventType\":\"Metric\",\"source\":"
#define E_TIME ",\"timestamp\":"
#define N_INVOCATIONS "ConcurrentInvocations"
#define N_TIMED "TimedRateLimit"
#define N_CONCURRENT "ConcurrentRateLimit"
#define T_RATE "Too many requests in the last minute (count: "
#define T_CONC "Too many concurrent requests in flight (count: "
#define T_ALLOWED ", allowed: "
#define T_END ")."
// wlit hands one character to each lane
static_assert(LIT(E_HEAD) <= 64 && LIT(E_VALUE) <= 64 && LIT(E_SOURCE) <= 64 && LIT(E_TIME) <= 64 &&
              LIT(N_INVOCATIONS) <= 64 && LIT(T_RATE) <= 64 && LIT(T_CONC) <= 64 && LIT(T_ALLOWED) <= 64,
              "a literal longer than a wave");

// class of an item (the table in include/owgs.h): which event and text it has
enum { C_NONE = 0, C_INVOCATIONS = 1, C_TIMED = 2, C_CONCURRENT = 3 };
__device__ __forceinline__ int evt_class(uint8_t kind, uint8_t verdict) {
    if (verdict == 1) return C_TIMED;       // OWGS_ADMIT_RATE, action or trigger
    if (verdict == 2) return C_CONCURRENT;  // OWGS_ADMIT_CONCURRENT
    return (kind & 1) ? C_NONE : C_INVOCATIONS;  // OWGS_ADMIT_OK: a trigger sends nothing (`case _ => // ignore`)
}

// Metric value: count + 1 on an Int (wrapping), then widened (Entitlement.scala:389-391); 1 for a rejection
__device__ __forceinline__ int64_t evt_value(int cls, int32_t conc_count) {
    return cls == C_INVOCATIONS ? (int64_t)(int32_t)((uint32_t)conc_count + 1u) : 1;
}

__device__ __forceinline__ int evt_name_len(int cls) {
    return cls == C_INVOCATIONS ? LIT(N_INVOCATIONS) : cls == C_TIMED ? LIT(N_TIMED) : LIT(N_CONCURRENT);
}

// grid over n + 1: thread n writes the zero the exclusive sums turn into the totals
__global__ __launch_bounds__(256) void owgs_evt_size_kernel(OwgsEventArgs A) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    int64_t el = 0, rl = 0;
    if (i < A.n) {
        const int cls = evt_class(A.kind[i], A.verdict[i]);
        if (cls != C_NONE) {
            const int32_t id = A.ident[i];
            el = LIT(E_HEAD) + evt_name_len(cls) + LIT(E_VALUE) + digits(evt_value(cls, A.conc_count[i])) +
                 LIT(E_SOURCE) + A.src_len + 1 + (A.ia_off[id + 1] - A.ia_off[id]) + LIT(E_TIME) + digits(A.ts[i]) +
                 1 + (A.ib_off[id + 1] - A.ib_off[id]) + 1;
        }
        if (cls == C_TIMED)
            rl = LIT(T_RATE) + digits(A.rate_count[i]) + LIT(T_ALLOWED) + digits(A.rate_limit[i]) + LIT(T_END);
        else if (cls == C_CONCURRENT)
            rl = LIT(T_CONC) + digits(A.conc_count[i]) + LIT(T_ALLOWED) + digits(A.conc_limit[i]) + LIT(T_END);
    }
    if (i <= A.n) {
        A.ev_len[i] = el;
        A.rej_len[i] = rl;
    }
    // the counts: one atomic per wave and counter
    const unsigned long long be = __ballot(el != 0), br = __ballot(rl != 0);
    if ((threadIdx.x & 63) == 0) {
        if (be) atomicAdd(&A.cnt[0], __popcll(be));
        if (br) atomicAdd(&A.cnt[1], __popcll(br));
    }
}

// One wave per item.  ev_off[n] / rej_off[n] are the bytes needed: a region that does not fit is not written and is
// flagged in cnt[2] for the host, the other region is written all the same.
__global__ __launch_bounds__(256) void owgs_evt_write_kernel(OwgsEventArgs A) {
    const int32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= A.n) return;
    const bool ev_fits = A.ev_off[A.n] <= A.ev_cap, rej_fits = A.rej_off[A.n] <= A.rej_cap;
    if (i == 0 && lane == 0 && !(ev_fits && rej_fits))
        atomicOr(&A.cnt[2], (ev_fits ? 0 : OWGS_EVT_REFUSED_EV) | (rej_fits ? 0 : OWGS_EVT_REFUSED_REJ));
    const int cls = evt_class(A.kind[i], A.verdict[i]);
    if (cls == C_NONE) return;
    if (ev_fits) {
        char* d = A.ev_out + A.ev_off[i];
        const int32_t id = A.ident[i];
        int64_t o = 0;
        wlit(d + o, E_HEAD, LIT(E_HEAD), lane);
        o += LIT(E_HEAD);
        if (cls == C_INVOCATIONS) wlit(d + o, N_INVOCATIONS, LIT(N_INVOCATIONS), lane);
        else if (cls == C_TIMED) wlit(d + o, N_TIMED, LIT(N_TIMED), lane);
        else wlit(d + o, N_CONCURRENT, LIT(N_CONCURRENT), lane);
        o += evt_name_len(cls);
        wlit(d + o, E_VALUE, LIT(E_VALUE), lane);
        o += LIT(E_VALUE);
        o += wput_dec(d + o, evt_value(cls, A.conc_count[i]), lane);
        wlit(d + o, E_SOURCE, LIT(E_SOURCE), lane);
        o += LIT(E_SOURCE);
        wcopy(d + o, A.src, A.src_len, lane);
        o += A.src_len;
        if (lane == 0) d[o] = ',';
        o += 1;
        {
            const int64_t a0 = A.ia_off[id], al = A.ia_off[id + 1] - a0;
            wcopy(d + o, A.ia + a0, al, lane);
            o += al;
        }
        wlit(d + o, E_TIME, LIT(E_TIME), lane);
        o += LIT(E_TIME);
        o += wput_dec(d + o, A.ts[i], lane);
        if (lane == 0) d[o] = ',';
        o += 1;
        {
            const int64_t b0 = A.ib_off[id], bl = A.ib_off[id + 1] - b0;
            wcopy(d + o, A.ib + b0, bl, lane);
            o += bl;
        }
        if (lane == 0) d[o] = '}';
    }
    if (rej_fits && cls != C_INVOCATIONS) {
        char* d = A.rej_out + A.rej_off[i];
        const bool rate = cls == C_TIMED;
        int64_t o = 0;
        if (rate) wlit(d, T_RATE, LIT(T_RATE), lane);
        else wlit(d, T_CONC, LIT(T_CONC), lane);
        o += rate ? LIT(T_RATE) : LIT(T_CONC);
        o += wput_dec(d + o, rate ? A.rate_count[i] : A.conc_count[i], lane);
        wlit(d + o, T_ALLOWED, LIT(T_ALLOWED), lane);
        o += LIT(T_ALLOWED);
        o += wput_dec(d + o, rate ? A.rate_limit[i] : A.conc_limit[i], lane);
        wlit(d + o, T_END, LIT(T_END), lane);
    }
}

extern "C" size_t owgs_event_scratch_bytes(int32_t n) {
    size_t b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, n + 1);
    return b;
}

// sizes, offsets, bytes: queued on st without a wait.  a->cnt must be zero (the caller's memset on st).
extern "C" hipError_t owgs_launch_events(const OwgsEventArgs* a, void* temp, size_t temp_bytes, hipStream_t st) {
    const OwgsEventArgs& A = *a;
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_evt_size_kernel, dim3((unsigned)(((int64_t)A.n + 1 + 255) / 256)), dim3(256), 0, st, A);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(temp, tb, A.ev_len, A.ev_off, A.n + 1, st);
    if (e != hipSuccess) return e;
    tb = temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(temp, tb, A.rej_len, A.rej_off, A.n + 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(owgs_evt_write_kernel, dim3((unsigned)(((int64_t)A.n + 3) / 4)), dim3(256), 0, st, A);
    return hipGetLastError();
}
