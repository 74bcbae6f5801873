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
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "owgs_internal.h"

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
