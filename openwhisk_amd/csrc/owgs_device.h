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

// ------------------------------------------------------------------------------------------------ the serialisers
// (owgs_msgs.hip, owgs_events.hip: decimal printing and the wave-cooperative copies)
__device__ __forceinline__ unsigned long long pow10_at(int t) {  // 10^t, 0 <= t < 20
    constexpr unsigned long long P[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull,
        10000000ull, 100000000ull, 1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull,
        100000000000000ull, 1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull,
        10000000000000000000ull};
    return P[t];
}

__device__ __forceinline__ uint64_t magnitude(int64_t v) { return v < 0 ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v; }

// decimal digits of |v| (+1 for the sign): t = floor(bit length * log10(2)) is the digit count or one less
__device__ __forceinline__ int digits(int64_t v) {
    const uint64_t u = magnitude(v);
    const int t = ((64 - __clzll(u | 1)) * 1233) >> 12;
    return max(t + (u >= pow10_at(t) ? 1 : 0), 1) + (v < 0);
}

// decimal digit of u at power r (0 = units): u split into three base-1e9 limbs by two constant divisions, then one
// 32-bit division
__device__ __forceinline__ int digit_at(uint64_t u, int r) {
    const uint64_t q = u / 1000000000ull;
    const uint32_t lo = (uint32_t)(u - q * 1000000000ull);
    const uint64_t q2 = q / 1000000000ull;
    const uint32_t mid = (uint32_t)(q - q2 * 1000000000ull), top = (uint32_t)q2;
    const uint32_t x = r < 9 ? lo : r < 18 ? mid : top;
    const uint32_t p = (uint32_t)pow10_at(r < 9 ? r : r < 18 ? r - 9 : r - 18);
    return (int)((x / p) % 10u);
}

// wave-cooperative copy of len bytes
__device__ __forceinline__ void wcopy(char* dst, const char* src, int64_t len, int lane) {
    const int n = (int)len;  // a piece of one message: < 2^31 bytes
    for (int j = lane; j < n; j += 64) dst[j] = src[j];
}
__device__ __forceinline__ void wlit(char* dst, const char* lit, int len, int lane) {
    if (lane < len) dst[lane] = lit[lane];
}

// lane k of a wave writes character k (from the left) of v's decimal form at d; returns its length
__device__ __forceinline__ int wput_dec(char* d, int64_t v, int lane) {
    const int nd = digits(v);
    if (lane < nd) {
        if (v < 0 && lane == 0) d[0] = '-';
        else d[lane] = (char)('0' + digit_at(magnitude(v), nd - 1 - lane));
    }
    return nd;
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
