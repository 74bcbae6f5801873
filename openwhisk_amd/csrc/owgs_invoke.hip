// owgs_invoke.hip -- the seam between the entitlement throttle gate and publish.
//
// Replaces the host detour between the two steps every invoke takes in the reference:
//   EntitlementProvider.checkThrottles         Entitlement.scala:197-202, 354-381  (owgs_admit_resolve_kernel)
//   ShardingContainerPoolBalancer.publish      SCPB:257-317                        (the engine, the table kernels,
//                                                                                    the message stage)
// The gate leaves one verdict per item in HBM.  owgs_invoke_count_kernel / owgs_invoke_compact_kernel pack the admitted
// actions, in array order, into the engine's input and write the batch offsets {0, m} the engine and the pre-pass read
// on the device: the host launches them with the upper bound n and never learns m before the call's one copy back.
// owgs_invoke_gate_kernel is owgs_publish_gate_kernel with a scatter: the engine's decisions are indexed by the rank
// among the admitted actions, everything after it (table kernels, message stage, the caller) by item.
//
// Compaction: per wave64 one ballot and __popcll, the four wave counts through LDS, the block's base from the per-block
// counts of the count kernel (the pattern of owgs_feed_compact_kernel, over any number of blocks).  Every block of the
// scatter sums the counts of the blocks before it and of all blocks itself -- ceil(n / 256) words, 16 for a batch of
// 4,096 -- so there is no look-back chain and no ordering between blocks.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "owgs_internal.h"
#include "owgs_launch.h"

typedef unsigned long long u64;

__device__ __forceinline__ bool inv_admitted(const OwgsInvokeCompact& A, int i) {
    return i < A.n && !(A.kind[i] & 1u) && A.verdict[i] == 0;  // an action with OWGS_ADMIT_OK
}

__device__ __forceinline__ int inv_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(256) void owgs_invoke_count_kernel(OwgsInvokeCompact A) {
    __shared__ int32_t wcnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const u64 b = __ballot(inv_admitted(A, i));
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) A.bcnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(256) void owgs_invoke_compact_kernel(OwgsInvokeCompact A) {
    __shared__ int32_t wcnt[4], wbase[4], wtot[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    // admitted actions in the blocks before this one, and in all of them
    int before = 0, total = 0;
    for (int j = (int)threadIdx.x; j < (int)gridDim.x; j += 256) {
        const int c = A.bcnt[j];
        total += c;
        if (j < (int)blockIdx.x) before += c;
    }
    before = inv_wave_sum(before);
    total = inv_wave_sum(total);
    const bool adm = inv_admitted(A, i);
    const u64 b = __ballot(adm);
    if (lane == 0) {
        wcnt[wv] = __popcll(b);
        wbase[wv] = before;
        wtot[wv] = total;
    }
    __syncthreads();
    const int base = wbase[0] + wbase[1] + wbase[2] + wbase[3];
    const int m = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    int k = base + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) k += wcnt[w];
    if (i < A.n) {
        if (adm) {  // (k < m <= n)
            A.act_c[k] = A.action[i];
            if (A.seq) A.seq_c[k] = A.seq[i];
            A.map[k] = i;
        }
        A.rank[i] = adm ? k : -1;
        if (i >= m) {  // past the admitted actions: what the engine never writes and the watch update must ignore
            A.act_c[i] = 0;
            A.pad_out[i] = OWGS_NONE_V;
            A.pad_flags[i] = 0;
        }
    }
    if (i == 0) {
        A.off[0] = 0;
        A.off[1] = (int64_t)m;
    }
}

#define GATE_WORDS 5  // OWGS_PUB_PLACED .. OWGS_PUB_THROW

__global__ __launch_bounds__(256) void owgs_invoke_gate_kernel(OwgsInvokeGate G) {
    __shared__ int32_t wcnt[GATE_WORDS][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int32_t err = *G.err;  // (uniform: one scalar load)
    bool placed = false, ovl_m = false, ovl_b = false, none = false, thr = false;
    if (i < G.n) {
        const int k = G.rank[i];
        int32_t d = OWGS_NOT_PUBLISHED_V;
        uint8_t f = 0;
        if (k >= 0) {
            d = G.dec[k];
            f = G.dflags[k];
            if (!err) {
                placed = d >= 0;
                none = d == OWGS_NONE_V;
                thr = d == -2;  // OWGS_THROW_INDEX
                if (placed && (f & 1)) {  // MANAGED_ / BLACKBOX_SYSTEM_OVERLOAD (SCPB:277-286)
                    const bool bb = G.act_bb[G.action[i]] != 0;
                    ovl_m = !bb;
                    ovl_b = bb;
                }
            }
        }
        G.placed[i] = placed ? 1 : 0;
        if (G.msg_inv) G.msg_inv[i] = placed ? d : -1;
        G.out_inv[i] = d;
        G.out_flags[i] = f;
        if (!placed) {  // (a placed item's pair is the fill kernel's)
            G.out_ticket[i] = -1;
            G.out_existed[i] = 0;
        }
    }
    const u64 b0 = __ballot(placed), b1 = __ballot(ovl_m), b2 = __ballot(ovl_b), b3 = __ballot(none),
              b4 = __ballot(thr);
    if (lane == 0) {
        wcnt[OWGS_PUB_PLACED][wv] = __popcll(b0);
        wcnt[OWGS_PUB_OVL_MANAGED][wv] = __popcll(b1);
        wcnt[OWGS_PUB_OVL_BLACKBOX][wv] = __popcll(b2);
        wcnt[OWGS_PUB_NONE][wv] = __popcll(b3);
        wcnt[OWGS_PUB_THROW][wv] = __popcll(b4);
    }
    __syncthreads();
    if (threadIdx.x < GATE_WORDS) {
        const int w = (int)threadIdx.x;
        const int32_t s = wcnt[w][0] + wcnt[w][1] + wcnt[w][2] + wcnt[w][3];
        if (s) atomicAdd(&G.hdr[w], (u64)s);
    }
    if (i == 0) G.hdr[OWGS_PUB_ERR] = (u64)(uint32_t)err;
}

// bcnt holds ceil(n / 256) words
extern "C" hipError_t owgs_launch_invoke_compact(const OwgsInvokeCompact* a, hipStream_t st) {
    if (a->n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a->n + 255) / 256));
    hipLaunchKernelGGL(owgs_invoke_count_kernel, grid, dim3(256), 0, st, *a);
    hipLaunchKernelGGL(owgs_invoke_compact_kernel, grid, dim3(256), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_invoke_gate(const OwgsInvokeGate* g, hipStream_t st) {
    if (g->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_invoke_gate_kernel, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, st, *g);
    return hipGetLastError();
}
