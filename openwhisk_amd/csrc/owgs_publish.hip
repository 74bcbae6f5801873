// owgs_publish.hip -- the gate of owgs_publish_activations.
//
// Replaces the host detour between the three steps of ShardingContainerPoolBalancer.publish for a drained batch:
//   schedule                                   SCPB:260-290  (the engine: decisions in HBM)
//   if (invoker.isDefined) setupActivation     SCPB:292-304, CLB:116-166  (the table kernels, owgs_acks.hip)
//   sendActivationToInvoker                    SCPB:302-303, CLB:175-198  (the message stage, owgs_msgs.hip)
// The engine leaves one decision per item; owgs_publish_gate_kernel turns them into the per-item "placed" predicate
// the table kernels take (an item without an invoker touches neither the table nor a counter), into the message
// stage's invoker array, and into the call's summary words.  When the context's error word is set the predicate is
// all-false and every message invoker is -1: the later stages run and do nothing, without the host having looked.
//
// Summary words by wave64 ballot: one __popcll per wave and word, the four wave counts through LDS, one atomic per
// block and word (the pattern of mb_totals_add and owgs_feed_compact_kernel).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "owgs_internal.h"
#include "owgs_launch.h"

typedef unsigned long long u64;

#define GATE_WORDS 5  // OWGS_PUB_PLACED .. OWGS_PUB_THROW

__global__ __launch_bounds__(256) void owgs_publish_gate_kernel(OwgsPublishGate G) {
    __shared__ int32_t wcnt[GATE_WORDS][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int32_t err = *G.err;  // (uniform: one scalar load)
    bool placed = false, ovl_m = false, ovl_b = false, none = false, thr = false;
    if (i < G.n) {
        const int32_t d = G.dec[i];
        const uint8_t f = G.dflags[i];
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

// after the message stage: its three host-visible words join the block, so that one copy brings everything
__global__ void owgs_publish_collect_kernel(u64* hdr, const int32_t* bad, const int32_t* topic_start,
                                            int32_t n_topics, const int64_t* out_off, int32_t n) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    hdr[OWGS_PUB_MSG_BAD] = (u64)(uint32_t)*bad;
    hdr[OWGS_PUB_MSG_M] = (u64)(uint32_t)topic_start[n_topics];
    hdr[OWGS_PUB_MSG_TOTAL] = (u64)out_off[n];
}

extern "C" hipError_t owgs_launch_publish_gate(const OwgsPublishGate* g, hipStream_t st) {
    if (g->n <= 0) return hipSuccess;
    hipLaunchKernelGGL(owgs_publish_gate_kernel, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, st, *g);
    return hipGetLastError();
}

extern "C" hipError_t owgs_launch_publish_collect(unsigned long long* hdr, const int32_t* bad,
                                                  const int32_t* topic_start, int32_t n_topics,
                                                  const int64_t* out_off, int32_t n, hipStream_t st) {
    hipLaunchKernelGGL(owgs_publish_collect_kernel, dim3(1), dim3(64), 0, st, hdr, bad, topic_start, n_topics, out_off,
                       n);
    return hipGetLastError();
}
