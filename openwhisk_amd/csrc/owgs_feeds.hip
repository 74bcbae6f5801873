// owgs_feeds.hip -- the two supervision feeds on the device.
//
// Replaces the host detour between a topic's batch and the health FSM (owgs_health.hip):
//   InvokerPool.processInvokerPing -> self ! PingMessage          InvokerSupervision.scala (ISUP) 174-185
//   processCompletion -> invokerPool ! InvocationFinishedMessage  CommonLoadBalancer.scala (CLB) 266-276, 317, 327
// The ping parser (owgs_ping_parse_kernel, owgs_acks.hip) and the completion path leave one outcome per item in device
// buffers; owgs_feed_compact_kernel turns the items that produce a supervision message into the event arrays
// (invoker, kind, t, userMemory) that owgs_launch_health_batch takes, in item order (mailbox order).  No event array
// crosses the bus.
//
// One workgroup of 16 waves walks the items in tiles of 1,024: a wave ballot gives each feeding lane its rank inside
// the wave, the 16 wave counts go through LDS, the running total is carried from tile to tile.  The feeds' batches are
// the topics' (128 acks, LB:94-108; a ping per invoker and second), so one workgroup is the whole job and a second
// launch for a multi-block scan would cost more than it saves.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "owgs_internal.h"
#include "owgs_launch.h"

#define EV_PING 0
#define EV_SUCCESS 1
#define EV_SYSTEM_ERROR 2
#define EV_TIMEOUT 3

template <int MODE>
__global__ __launch_bounds__(1024) void owgs_feed_compact_kernel(OwgsFeedArgs A) {
    __shared__ int32_t wcnt[16];
    __shared__ int32_t total;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) total = 0;
    __syncthreads();
    for (int32_t i0 = 0; i0 < A.n; i0 += 1024) {
        const int32_t i = i0 + tid;
        bool feed = false;
        int32_t inv = 0;
        int kind = EV_PING;
        if (i < A.n) {
            const int k = A.kind[i];
            inv = A.inv[i];
            if (MODE == OWGS_FEED_PINGS) {
                feed = k == OWGS_PING_FED;
            } else {
                // InvocationFinishedMessage goes out where processCompletion found the entry or the ack is a health
                // test action's (CLB:317, 327); an id the status vector cannot hold has no actor (ISUP:135-137)
                feed = (k == OWGS_ACK_RELEASED || k == OWGS_ACK_HEALTH) && inv >= 0 && inv < OWGS_HEALTH_MAX_ID_V;
                const bool forced = A.info && ((A.info[i] >> 6) & 1);
                kind = forced ? EV_TIMEOUT : (A.flags[i] & 1) ? EV_SYSTEM_ERROR : EV_SUCCESS;  // CLB:266-276
            }
        }
        const unsigned long long bal = __ballot(feed);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        int32_t pos = total + rank;
        for (int w = 0; w < wv; ++w) pos += wcnt[w];
        if (feed) {  // pos < events so far <= i + 1 <= n: inside the arrays, which hold n entries
            A.ev_inv[pos] = inv;
            A.ev_kind[pos] = (uint8_t)kind;
            A.ev_t[pos] = MODE == OWGS_FEED_PINGS ? A.t[i] : A.now;
            A.ev_mem[pos] = MODE == OWGS_FEED_PINGS ? A.mem[i] : 0;
        }
        __syncthreads();
        if (tid == 0) {
            int32_t s = 0;
            for (int w = 0; w < 16; ++w) s += wcnt[w];
            total += s;
        }
        __syncthreads();
    }
}

extern "C" hipError_t owgs_launch_feed_compact(const OwgsFeedArgs* a, int mode, hipStream_t st) {
    if (a->n <= 0) return hipSuccess;
    if (mode == OWGS_FEED_PINGS)
        hipLaunchKernelGGL(owgs_feed_compact_kernel<OWGS_FEED_PINGS>, dim3(1), dim3(1024), 0, st, *a);
    else
        hipLaunchKernelGGL(owgs_feed_compact_kernel<OWGS_FEED_ACKS>, dim3(1), dim3(1024), 0, st, *a);
    return hipGetLastError();
}
