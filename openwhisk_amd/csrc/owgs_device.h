// owgs_device.h -- the device helpers that more than one kernel file uses, defined once: the counter RNG every engine
// shares with the oracle (a drifted copy would be a parity bug of one engine), bit and wave primitives, and the walk
// arithmetic of the chunked engine (owgs_kernels.hip), which the device self-test there checks against integer division.
#ifndef OWGS_DEVICE_H
#define OWGS_DEVICE_H

#include <hip/hip_runtime.h>

#include "owgs_divq.h"
#include "owgs_internal.h"

typedef unsigned long long u64;  // (every kernel file's name for it)

// ------------------------------------------------------------------------------------------------ every engine
__device__ __forceinline__ u64 splitmix64(u64 x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// Counter RNG replacing ThreadLocalRandom.nextInt(|H|) (SCPB:421); identical to oracle/owsched_oracle.c
__device__ __forceinline__ uint32_t rng_index(u64 seed, u64 seq, uint32_t n) {
    u64 u = splitmix64(seed ^ (seq * 0x9E3779B97F4A7C15ULL)) >> 32;
    return (uint32_t)((u * (u64)n) >> 32);
}

__device__ __forceinline__ int ffs64(u64 m) { return __ffsll((long long)m) - 1; }

// DPP (GFX9 row_shr / row_bcast) wave64 scans: no LDS round trip
template <int CTRL, int ROWM>
__device__ __forceinline__ int dpp_add_src(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWM, 0xf, true);  // out-of-row / masked lanes read 0
}
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += dpp_add_src<0x111, 0xf>(v);  // row_shr:1
    v += dpp_add_src<0x112, 0xf>(v);  // row_shr:2
    v += dpp_add_src<0x114, 0xf>(v);  // row_shr:4
    v += dpp_add_src<0x118, 0xf>(v);  // row_shr:8
    v += dpp_add_src<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
    v += dpp_add_src<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
    return v;
}
template <int CTRL, int ROWM>
__device__ __forceinline__ int dpp_keep(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWM, 0xf, false);  // invalid source lanes keep `old`
}
__device__ __forceinline__ int wave_incl_max(int v) {
    const int I = (int)0x80000000;
    v = max(v, dpp_keep<0x111, 0xf>(I, v));
    v = max(v, dpp_keep<0x112, 0xf>(I, v));
    v = max(v, dpp_keep<0x114, 0xf>(I, v));
    v = max(v, dpp_keep<0x118, 0xf>(I, v));
    v = max(v, dpp_keep<0x142, 0xa>(I, v));
    v = max(v, dpp_keep<0x143, 0xc>(I, v));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    const int I = (int)0x80000000;
    v = max(v, dpp_keep<0x111, 0xf>(I, v));
    v = max(v, dpp_keep<0x112, 0xf>(I, v));
    v = max(v, dpp_keep<0x114, 0xf>(I, v));
    v = max(v, dpp_keep<0x118, 0xf>(I, v));
    v = max(v, dpp_keep<0x142, 0xa>(I, v));
    v = max(v, dpp_keep<0x143, 0xc>(I, v));
    return __builtin_amdgcn_readlane(v, 63);
}

// position of the need-th set bit (0-based) of m, need < popc(m): halving by popcounts, no loop over the bits
__device__ __forceinline__ int select_in_word(uint32_t m, int need) {
    int pos = 0;
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        const int c = __popc(m & ((1u << w) - 1u));
        const bool up = need >= c;
        need -= up ? c : 0;
        m = up ? m >> w : m;
        pos += up ? w : 0;
    }
    return pos;
}

// x mod n for 0 <= x < 2^31, 1 <= n < 2^15 without an integer division: float reciprocal, then exact correction
__device__ __forceinline__ int mod_fast(int x, int n, float rn) {
    const int q = (int)((float)x * rn);  // |q - x / n| <= 2 for x < 2^31, n < 2^15
    int r = x - q * n;
    r += r < 0 ? n : 0;
    r += r < 0 ? n : 0;
    r -= r >= n ? n : 0;
    r -= r >= n ? n : 0;
    return r;
}

// ------------------------------------------------------------------------------------------------ chunked engine only
// (the resident and the large-state engine use nothing below; it is here for the engine and the self-test that checks it)
#define OWGS_CAPMAX 1024  // capacities are clamped: a lane's rank is < OWGS_WL

// The walk arithmetic of the chunked engine: the exact forms of owgs_divq.h, whose per-divisor
// constants are computed where the divisor is fixed (the lane decode, the kernel prologue).  DivCap: capacities by one
// memory limit; DivPos: positions in one pool.
struct DivCap {
    int m;
    float rm, hrm;
};
struct DivPos {
    int n;
    uint32_t M;
};
__device__ __forceinline__ DivCap div_cap_of(int m, float rm) { return DivCap{m, rm, 0.5f * rm}; }
// from the correctly rounded reciprocal a DivCap needs
__device__ __forceinline__ DivCap div_cap(int m) { return div_cap_of(m, owgs_divq_rm(m)); }
// min(floor(pv / m), OWGS_CAPMAX), 0 for pv < m (negative permits included); usable permits are below 2^22
__device__ __forceinline__ int cap_q(int pv, const DivCap& d) { return owgs_divq_cap(pv, d.rm, d.hrm, OWGS_CAPMAX); }
__device__ __forceinline__ DivPos div_pos(int n, uint32_t M) { return DivPos{n, M}; }
// x mod n for 0 <= x < 2^31, 1 <= n < 2^15
__device__ __forceinline__ int pos_mod(int x, const DivPos& d) { return owgs_divq_mod(x, d.n, d.M); }
// x mod n for ranks (< 2^10) against maxConcurrent (< 2^12): owgs_divq.h's small remainder takes the hardware's
// reciprocal estimate, so no division per lane
static_assert(OWGS_CAPMAX == OWGS_DIVQ_CAPMAX && OWGS_MAX_MEM_MB == OWGS_DIVQ_MAX_MEM, "owgs_divq.h mirrors the engine's bounds");
__device__ __forceinline__ int small_mod(int x, int n) { return owgs_divq_small_mod(x, n, __builtin_amdgcn_rcpf((float)n)); }

#endif
