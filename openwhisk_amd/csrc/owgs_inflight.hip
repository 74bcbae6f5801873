// owgs_inflight.hip -- reads of the per-namespace in-flight counters and the batched throttle check.
//
// The counters themselves move in the track / completion kernels (owgs_acks.hip, "in-flight books").  Here:
//   owgs_ns_gather_kernel        activeActivationsFor (CLB:83-84) for a batch of namespace handles
//   owgs_throttle_resolve_kernel sequential replay, in array order, of ActivationThrottler.check
//                                (ActivationThrottler.scala:41-49: ConcurrentRateLimit(activeActivationsFor(ns), limit),
//                                ok = count < allowed, :58-59) followed for admitted jobs by setupActivation's namespace
//                                count (CLB:127):
//                                    count_i = active[ns_i] + #{ j < i : ns_j == ns_i and ok_j },  ok_i = count_i < limit_i
//                                hipcub radix sort of (namespace, batch index) -- stable, so a namespace's jobs stay in
//                                array order -- then every segment is resolved in order by the wave that owns its first
//                                item.  No atomics: the results cannot depend on an arrival order.
//   owgs_admit_resolve_kernel    the whole entitlement throttle gate on the same plan: per job, in array order, the
//                                per-minute rate throttle (RateThrottler.scala:47-54, RateInfo :60-86) of its kind and,
//                                for an action that passed it, the concurrent throttle above restricted to such actions
//                                (Entitlement.scala:197-202, 354-381), with every limit through calculateIndividualLimit
//                                (Entitlement.scala:97-133)
//   owgs_rate_gather_kernel / owgs_rate_grow_kernel   reads and growth of the RateInfo records
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "owgs_internal.h"
#include "owgs_launch.h"

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void owgs_ns_iota_kernel(int32_t* idx, int32_t n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = i;
}

__global__ __launch_bounds__(256) void owgs_ns_gather_kernel(const int32_t* active, const int32_t* ns, int32_t n,
                                                             int32_t* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = active[ns[i]];
}

// key / idx: the batch sorted by namespace handle (stable), idx = the job's index in the batch.  Wave w owns the
// segments whose first item lies in [64 w, 64 w + 64) and walks each of them to its end, 64 jobs at a time, with the
// namespace's running count `a` wave-uniform.  A chunk whose limits are all equal takes the closed form
// ok <=> rank < limit - a; a chunk with mixed limits is a true in-order dependency and is replayed lane by lane.
__global__ __launch_bounds__(256) void owgs_throttle_resolve_kernel(const uint32_t* key, const int32_t* idx, int32_t n,
                                                                    const int32_t* limit, const int32_t* active,
                                                                    int32_t* out_count, uint8_t* out_ok) {
    const int lane = (int)(threadIdx.x & 63);
    const int p0 = (int)((blockIdx.x * 256 + threadIdx.x) >> 6) * 64;
    if (p0 >= n) return;  // (wave-uniform)
    const int p = p0 + lane;
    const uint32_t k = p < n ? key[p] : 0xFFFFFFFFu;
    const uint32_t kp = (p > 0 && p < n) ? key[p - 1] : 0xFFFFFFFFu;
    u64 heads = __ballot(p < n && (p == 0 || k != kp));
    while (heads) {
        const int hl = __ffsll((long long)heads) - 1;
        heads &= heads - 1;
        const uint32_t seg = (uint32_t)__shfl((int)k, hl);
        int a = active[seg];  // activeActivationsFor(namespace) before the batch (CLB:83-84)
        for (int q = p0 + hl;; q += 64) {
            const int j = q + lane;
            const u64 m = __ballot(j < n && key[j] == seg);  // the segment is contiguous from q: a run of low ones
            const int cnt = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
            if (cnt == 0) break;
            int id = 0, L = 0;
            if (lane < cnt) {
                id = idx[j];
                L = limit[id];
            }
            const int L0 = __shfl(L, 0);
            int c = 0, ok = 0;
            if (__ballot(lane < cnt && L != L0) == 0) {
                long long room = (long long)L0 - (long long)a;  // jobs this chunk can still admit
                room = room < 0 ? 0 : room > cnt ? cnt : room;
                const int r = (int)room;
                ok = lane < r;
                c = a + (lane < r ? lane : r);
                a += r;
            } else {
                for (int t = 0; t < cnt; ++t) {
                    const int Lt = __shfl(L, t);
                    const int o = a < Lt;  // ConcurrentRateLimit.ok: count < allowed
                    if (lane == t) {
                        c = a;
                        ok = o;
                    }
                    a += o;  // an admitted job is tracked: setupActivation's increment (CLB:127)
                }
            }
            if (lane < cnt) {
                out_count[id] = c;
                out_ok[id] = (uint8_t)ok;
            }
            if (cnt < 64) break;
        }
    }
}

// calculateIndividualLimit (Entitlement.scala:123-133) of dilateLimit (:99): the product and Math.ceil in IEEE double,
// Double.toInt saturating, the division truncating.
__device__ __forceinline__ int owgs_individual_limit(int abs, int cs) {
    const double d = ceil((double)abs * (cs > 1 ? 1.2 : 1.0));
    const int dil = d >= 2147483647.0 ? 2147483647 : d <= -2147483648.0 ? (-2147483647 - 1) : (int)d;
    if (dil == 0) return 0;
    const int q = dil / cs;
    return q > 1 ? q : 1;
}

__device__ __forceinline__ long long owgs_shfl64(long long v, int src) {
    const int lo = __shfl((int)(unsigned)((u64)v & 0xFFFFFFFFull), src);
    const int hi = __shfl((int)((u64)v >> 32), src);
    return (long long)(((u64)(unsigned)hi << 32) | (u64)(unsigned)lo);
}

// The walk of owgs_throttle_resolve_kernel with two more things per chunk of 64 jobs of one namespace.
//   rate: the count of a job does not depend on any verdict, so it is a closed form over the chunk: a job resets its
//     kind's RateInfo when its minute differs from that of the nearest earlier job of its kind (from the carried lastMin
//     when the chunk has none), and its count is its rank among its kind since the last reset at or before it, on top of
//     the carried count when there was no reset.  Two carries (invoke, fire), wave-uniform, written back by the owning
//     wave at the segment's end.
//   concurrent: only actions that passed the rate check take part; ranks are taken over THOSE lanes.  Equal limits among
//     them: ok <=> rank < limit - a; mixed limits: replayed lane by lane over them.
__global__ __launch_bounds__(256) void owgs_admit_resolve_kernel(const OwgsAdmitArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int n = A.n;
    const int p0 = (int)((blockIdx.x * 256 + threadIdx.x) >> 6) * 64;
    if (p0 >= n) return;  // (wave-uniform)
    const int p = p0 + lane;
    const uint32_t k = p < n ? A.key[p] : 0xFFFFFFFFu;
    const uint32_t kp = (p > 0 && p < n) ? A.key[p - 1] : 0xFFFFFFFFu;
    const u64 lt = (1ull << lane) - 1;  // the lanes before this one
    u64 heads = __ballot(p < n && (p == 0 || k != kp));
    while (heads) {
        const int hl = __ffsll((long long)heads) - 1;
        heads &= heads - 1;
        const uint32_t seg = (uint32_t)__shfl((int)k, hl);
        int a = A.active[seg];  // activeActivationsFor(namespace) before the batch (CLB:83-84)
        long long cm0 = A.rate_min[seg], cm1 = A.rate_min[(size_t)A.ns_cap + seg];  // RateInfo.lastMin: invoke, fire
        int cc0 = A.rate_cnt[seg], cc1 = A.rate_cnt[(size_t)A.ns_cap + seg];         // RateInfo.lastMinCount
        for (int q = p0 + hl;; q += 64) {
            const int j = q + lane;
            const u64 m = __ballot(j < n && A.key[j] == seg);  // the segment is contiguous from q: a run of low ones
            const int cnt = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
            if (cnt == 0) break;
            const bool v = lane < cnt;
            int id = 0, trig = 0, Lr = 0, Lc = 0;
            long long mn = 0;
            if (v) {
                id = A.idx[j];
                const int kd = A.kind[id];
                trig = kd & 1;
                mn = A.t_ms[id] / 60000;  // getCurrentMinute (RateThrottler.scala:85)
                Lr = owgs_individual_limit((kd & 2) ? A.rate_ov[id] : trig ? A.def_fire : A.def_invoke, A.cluster);
                Lc = trig ? 0 : owgs_individual_limit((kd & 4) ? A.conc_ov[id] : A.def_conc, A.cluster);
            }
            // ---- rate: roll() then incrementAndGet() (RateThrottler.scala:72-83)
            const u64 trg = __ballot(v && trig), act = __ballot(v && !trig);
            const u64 before = (trig ? trg : act) & lt;  // earlier jobs of my kind in the chunk
            const int pl = before ? 63 - __clzll((long long)before) : 0;
            const long long pm = owgs_shfl64(mn, pl);
            const long long ref = before ? pm : trig ? cm1 : cm0;
            const u64 rs = __ballot(v && mn != ref) & (trig ? trg : act) & (lt | (1ull << lane));  // resets up to me
            unsigned rcu;
            if (rs == 0) {
                rcu = (unsigned)(trig ? cc1 : cc0) + (unsigned)__popcll(before) + 1u;
            } else {
                const int lr = 63 - __clzll((long long)rs);  // the last reset at or before me
                rcu = (unsigned)__popcll(before >> lr) + 1u;
            }
            const int rc = (int)rcu;  // wrapping int32 (AtomicInteger)
            const int rate_ok = rc <= Lr;  // TimedRateLimit.ok: count <= allowed
            if (act) {  // (wave-uniform)
                const int ll = 63 - __clzll((long long)act);
                cm0 = owgs_shfl64(mn, ll);
                cc0 = __shfl(rc, ll);
            }
            if (trg) {
                const int ll = 63 - __clzll((long long)trg);
                cm1 = owgs_shfl64(mn, ll);
                cc1 = __shfl(rc, ll);
            }
            // ---- concurrent: only for actions the rate check let through (the flatMap of Entitlement.scala:197-202)
            const int elig = v && !trig && rate_ok;
            const u64 em = __ballot(elig);
            int c = -1, ok = 0;
            if (em) {  // (wave-uniform)
                const int L0 = __shfl(Lc, __ffsll((long long)em) - 1);
                if (__ballot(elig && Lc != L0) == 0) {
                    const int ne = __popcll(em);
                    long long room = (long long)L0 - (long long)a;  // actions this chunk can still admit
                    room = room < 0 ? 0 : room > ne ? ne : room;
                    const int r = (int)room;
                    const int rank = __popcll(em & lt);  // among the eligible lanes, not over the chunk
                    if (elig) {
                        ok = rank < r;
                        c = a + (rank < r ? rank : r);
                    }
                    a += r;
                } else {
                    for (u64 e = em; e; e &= e - 1) {
                        const int t = __ffsll((long long)e) - 1;
                        const int Lt = __shfl(Lc, t);
                        const int o = a < Lt;  // ConcurrentRateLimit.ok: count < allowed
                        if (lane == t) {
                            c = a;
                            ok = o;
                        }
                        a += o;  // an admitted action is tracked: setupActivation's increment (CLB:127)
                    }
                }
            }
            if (v) {
                // OWGS_ADMIT_RATE 1, OWGS_ADMIT_OK 0 (triggers have no concurrent throttle), OWGS_ADMIT_CONCURRENT 2
                A.out_verdict[id] = (uint8_t)(!rate_ok ? 1 : (trig || ok) ? 0 : 2);
                A.out_rate_count[id] = rc;
                A.out_rate_limit[id] = Lr;
                A.out_conc_count[id] = c;
                A.out_conc_limit[id] = Lc;
            }
            if (cnt < 64) break;
        }
        if (lane == 0) {
            A.rate_min[seg] = cm0;
            A.rate_cnt[seg] = cc0;
            A.rate_min[(size_t)A.ns_cap + seg] = cm1;
            A.rate_cnt[(size_t)A.ns_cap + seg] = cc1;
        }
    }
}

__global__ __launch_bounds__(256) void owgs_rate_gather_kernel(const long long* rate_min, const int32_t* rate_cnt,
                                                               size_t base, const int32_t* ns, int32_t n,
                                                               long long* out_min, int32_t* out_cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out_min[i] = rate_min[base + ns[i]];
        out_cnt[i] = rate_cnt[base + ns[i]];
    }
}

// the records of old_cap handles into arrays of new_cap handles (both throttlers); the new handles are absent
__global__ __launch_bounds__(256) void owgs_rate_grow_kernel(const long long* old_min, const int32_t* old_cnt,
                                                             int32_t old_cap, long long* new_min, int32_t* new_cnt,
                                                             int32_t new_cap) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2ll * new_cap) return;
    const int which = i >= new_cap;
    const long long h = i - (long long)which * new_cap;
    const bool old = h < old_cap;
    new_min[i] = old ? old_min[(long long)which * old_cap + h] : OWGS_RATE_ABSENT;
    new_cnt[i] = old ? old_cnt[(long long)which * old_cap + h] : 0;
}

#define GRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st

extern "C" hipError_t owgs_launch_ns_gather(const int32_t* active, const int32_t* ns, int32_t n, int32_t* out,
                                            hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ns_gather_kernel, GRID(n), active, ns, n, out);
    return hipGetLastError();
}

// temp bytes for the sort of n (namespace, index) pairs
extern "C" size_t owgs_throttle_sort_bytes(int32_t n, int32_t bits) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (const int32_t*)nullptr, (int32_t*)nullptr, n, 0, bits);
    return b;
}

// ns: handles in [0, 2^bits) (the host checked them); key_out / idx_in / idx_out: scratch [n]
extern "C" hipError_t owgs_launch_throttle(const int32_t* ns, const int32_t* limit, int32_t n, int32_t bits,
                                           void* temp, size_t temp_bytes, int32_t* key_out, int32_t* idx_in,
                                           int32_t* idx_out, const int32_t* active, int32_t* out_count,
                                           uint8_t* out_ok, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ns_iota_kernel, GRID(n), idx_in, n);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, tb, (const uint32_t*)ns, (uint32_t*)key_out, idx_in,
                                                      idx_out, n, 0, bits, st);  // handles are >= 0; LSD = stable
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(owgs_throttle_resolve_kernel, GRID(n), (const uint32_t*)key_out, idx_out, n, limit, active,
                       out_count, out_ok);
    return hipGetLastError();
}

// A: everything but key / idx, which are the sort's outputs; scratch as in owgs_launch_throttle
extern "C" hipError_t owgs_launch_admit(const int32_t* ns, int32_t bits, void* temp, size_t temp_bytes,
                                        int32_t* key_out, int32_t* idx_in, int32_t* idx_out, const OwgsAdmitArgs* args,
                                        hipStream_t st) {
    const int32_t n = args->n;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_ns_iota_kernel, GRID(n), idx_in, n);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, tb, (const uint32_t*)ns, (uint32_t*)key_out, idx_in,
                                                      idx_out, n, 0, bits, st);  // handles are >= 0; LSD = stable
    if (e != hipSuccess) return e;
    OwgsAdmitArgs A = *args;
    A.key = (const uint32_t*)key_out;
    A.idx = idx_out;
    hipLaunchKernelGGL(owgs_admit_resolve_kernel, GRID(n), A);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_rate_gather(const long long* rate_min, const int32_t* rate_cnt, int32_t ns_cap,
                                              int32_t which, const int32_t* ns, int32_t n, long long* out_min,
                                              int32_t* out_cnt, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_rate_gather_kernel, GRID(n), rate_min, rate_cnt, (size_t)which * (size_t)ns_cap, ns, n,
                       out_min, out_cnt);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_rate_grow(const long long* old_min, const int32_t* old_cnt, int32_t old_cap,
                                            long long* new_min, int32_t* new_cnt, int32_t new_cap, hipStream_t st) {
    hipLaunchKernelGGL(owgs_rate_grow_kernel, GRID(2ll * new_cap), old_min, old_cnt, old_cap, new_min, new_cnt,
                       new_cap);
    return hipGetLastError();
}
