// owgs_expire.hip -- completion-ack timeouts on the device.
//
// Replaces, for the entries of activationSlots that live in HBM (owgs_acks.hip):
//   CommonLoadBalancer.setupActivation      CLB:148-152   actorSystem.scheduler.scheduleOnce(completionAckTimeout)
//   calculateCompletionAckTimeout           CLB:103-105   (armed by owgs_act_fill_kernel, owgs_acks.hip)
//   the fired timer                         CLB:150-152   processCompletion(aid, tid, forced = true, ...)
// One akka timer per entry becomes one int64 deadline per slot (td) and one int64 per tile of OWGS_TILE slots (tmin), a
// lower bound of the tile's armed deadlines.  A sweep reads tmin; only tiles with tmin <= now are scanned.
//
// Kernels
//   owgs_expire_scan_kernel   one workgroup per tile: returns after one load when nothing in the tile can be due;
//                             otherwise appends the due live slots to a compact list (ballot within the wave, one atomic
//                             per workgroup on the list counter) and stores the exact minimum of the tile's other live
//                             deadlines as its new tmin.
//   (hipcub radix sort)       the due list ordered by (deadline, arm sequence): two stable passes, least significant
//                             key first.
//   owgs_expire_emit_kernel   the first `take` entries of the order become forced completions in the shared tail's
//                             input arrays (key, invoker, info = completion | forced); the others stay armed and put
//                             their deadlines back into tmin, so every scanned tile's word is exact after the removals.
//   owgs_deadline_min_kernel  min-reduction over tmin (owgs_next_deadline).
// The removal itself, the books, releaseInvoker and the large-state branch are the forced path's (ack_complete in
// owgs_host.cpp): the sweep only writes its input.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stdint.h>

#include "owgs_internal.h"
#include "owgs_launch.h"

typedef unsigned long long u64;

__device__ __forceinline__ long long wave_min(long long m) {
    for (int o = 32; o; o >>= 1) {
        const long long x = __shfl_xor(m, o);
        m = x < m ? x : m;
    }
    return m;
}

__global__ __launch_bounds__(256) void owgs_expire_scan_kernel(OwgsExpireArgs A) {
    const long long t = blockIdx.x;
    if (A.T.tmin[t] > A.now) return;  // nothing armed in this tile is due (block-uniform)
    __shared__ int wcnt[4][4];        // due slots per (round, wave), then their offsets in the block's range
    __shared__ long long wmin[4];
    __shared__ int base;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const long long s0 = t * OWGS_TILE + threadIdx.x;
    long long d[4], keep = OWGS_NO_DEADLINE;
    int rank[4];
    bool due[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long s = s0 + k * 256;
        const bool live = A.T.tw[s] == OWGS_TW_READY;
        d[k] = live ? A.T.td[s] : OWGS_NO_DEADLINE;
        due[k] = live && d[k] <= A.now;
        if (!due[k] && d[k] < keep) keep = d[k];
        const u64 b = __ballot(due[k]);
        rank[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[k][wave] = __popcll(b);
    }
    keep = wave_min(keep);
    if (lane == 0) wmin[wave] = keep;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < 4; ++k)
            for (int w = 0; w < 4; ++w) {
                const int c = wcnt[k][w];
                wcnt[k][w] = total;
                total += c;
            }
        base = total ? atomicAdd(&A.cnt[0], total) : 0;
        atomicAdd(&A.cnt[1], 1);
        long long m = wmin[0];
        for (int w = 1; w < 4; ++w) m = wmin[w] < m ? wmin[w] : m;
        A.T.tmin[t] = m;  // exact over the entries this sweep leaves alone; the emit step adds the due ones it keeps
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!due[k]) continue;
        const int p = base + wcnt[k][wave] + rank[k];
        if (p >= A.due_cap) continue;  // (the host sizes the list by the live entries: not reached)
        const long long s = s0 + k * 256;
        A.due_d[p] = d[k];
        A.due_q[p] = A.T.tq[s];
        A.due_slot[p] = (int32_t)s;
    }
}

__global__ __launch_bounds__(256) void owgs_expire_iota_kernel(int32_t* idx, int32_t n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = i;
}

// keys of the second pass: the deadlines in arm-sequence order
__global__ __launch_bounds__(256) void owgs_expire_gather_kernel(const long long* due_d, const int32_t* idx, int32_t n,
                                                                 u64* key) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) key[j] = (u64)due_d[idx[j]];  // deadlines are in [0, 2^62): unsigned order = signed order
}

// order[j] = due-list index of the j-th entry by (deadline, arm sequence)
__global__ __launch_bounds__(256) void owgs_expire_emit_kernel(OwgsActTable T, const long long* due_d,
                                                               const int32_t* due_slot, const int32_t* order,
                                                               int32_t n, int32_t take, ulonglong2* key, int32_t* inst,
                                                               uint8_t* info, long long* out_deadline) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int i = order[j];
    const int s = due_slot[i];
    const long long d = due_d[i];
    if (j < take) {
        key[j] = T.tk[s];
        inst[j] = T.ti[s];  // invoker = entry.invoker (CLB:150-152)
        info[j] = (uint8_t)(OWGS_ACK_COMPLETION | 1 << 6);  // forced = true, isSystemError = false
        out_deadline[j] = d;
    } else {
        atomicMin(&T.tmin[s >> OWGS_TILE_LOG2], d);  // left armed by cap
    }
}

__global__ __launch_bounds__(256) void owgs_deadline_min_kernel(const long long* tmin, long long n_tiles,
                                                                long long* out) {
    __shared__ long long wmin[4];
    long long m = OWGS_NO_DEADLINE;
    for (long long t = threadIdx.x; t < n_tiles; t += 256) {
        const long long x = tmin[t];
        m = x < m ? x : m;
    }
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = wmin[w] < m ? wmin[w] : m;
        *out = m;
    }
}

// ------------------------------------------------------------------------------------------ launchers
#define GRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st

extern "C" hipError_t owgs_launch_expire_scan(const OwgsExpireArgs* a, hipStream_t st) {
    const long long tiles = a->T.cap >> OWGS_TILE_LOG2;
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_expire_scan_kernel, dim3((unsigned)tiles), dim3(256), 0, st, *a);
    return hipGetLastError();
}

// temp bytes of the two sort passes over n due entries
extern "C" size_t owgs_expire_sort_bytes(int32_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (const int32_t*)nullptr,
                                             (int32_t*)nullptr, n, 0, 64);
    return b;
}

// a->due_*: the scan's list of n entries.  idx0 / idx1 / key / key_s: scratch [n]; afterwards idx0 holds the order and
// the first `take` entries are in key_out / inst / info / out_deadline (the shared completion tail's inputs).
extern "C" hipError_t owgs_launch_expire_order(const OwgsExpireArgs* a, int32_t n, int32_t take, int32_t seq_bits,
                                               void* temp, size_t temp_bytes, int32_t* idx0, int32_t* idx1,
                                               unsigned long long* key, unsigned long long* key_s, ulonglong2* key_out,
                                               int32_t* inst, uint8_t* info, long long* out_deadline, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_expire_iota_kernel, GRID(n), idx0, n);
    size_t tb = temp_bytes;
    // least significant key first: the arm sequence, then (stable) the deadline
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, tb, (const u64*)a->due_q, key_s, (const int32_t*)idx0, idx1,
                                                      n, 0, seq_bits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(owgs_expire_gather_kernel, GRID(n), a->due_d, idx1, n, key);
    tb = temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(temp, tb, (const u64*)key, key_s, (const int32_t*)idx1, idx0, n, 0, 62, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(owgs_expire_emit_kernel, GRID(n), a->T, a->due_d, a->due_slot, idx0, n, take, key_out, inst, info,
                       out_deadline);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_deadline_min(const OwgsActTable* T, long long* out, hipStream_t st) {
    hipLaunchKernelGGL(owgs_deadline_min_kernel, dim3(1), dim3(256), 0, st, T->tmin, T->cap >> OWGS_TILE_LOG2, out);
    return hipGetLastError();
}
