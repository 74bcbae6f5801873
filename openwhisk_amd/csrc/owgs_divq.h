// owgs_divq.h -- exact quotients and remainders by invariant divisors, without an integer division and without
// correction chains.  Plain inline functions for host and device code: no HIP builtins, so the host
// reproduces the device bit for bit (tests/divq_check.cpp, run by tests/test_divq_cpu.py, drives this header alone).
//
// Capacity:  floor(x / mem) for 0 <= x < 2^22 and 1 <= mem <= OWGS_MAX_MEM_MB.
//   rm = 1.0f / (float)mem, correctly rounded (a plain division, not a hardware reciprocal estimate), hrm = 0.5f * rm.
//   fmaf(x, rm, hrm) is (x + 0.5) / mem with one rounding after the reciprocal's own: its error is below
//   2^-23 * (x + 0.5) / mem < 0.5 / mem for x < 2^22, and (x + 0.5) / mem is never closer than 0.5 / mem to an
//   integer, so the truncation is the floor.  From 2^23 on the form is wrong for some operands.
//   owgs_divq_cap clamps the operand into [0, 2^22) first and the quotient to qmax afterwards: negative operands give 0,
//   and an operand of 2^22 or more gives qmax exactly when floor((2^22 - 1) / mem) >= qmax, which for the engine's
//   qmax of 1024 is every mem up to OWGS_DIVQ_MEM_ANY.  So the clamped capacity is exact for x < 2^22 and any mem, and
//   for any x and mem <= OWGS_DIVQ_MEM_ANY; outside both it under-estimates.
//
// Position:  x mod n for 0 <= x < 2^31 and 1 <= n < 2^15.
//   M = floor((2^32 - 1) / n); q = hi32(x * M) under-estimates floor(x / n) by at most 1 (x * e / (n * 2^32) < 0.5
//   with e = 2^32 - M * n <= n), so r = x - q * n lies in [0, 2n) and one one-sided correction is exact.  As unsigned
//   numbers r - n wraps beyond r exactly when r < n, so the correction is min(r, r - n): no compare, no select.
//   (Rounding M down, not up, costs nothing and takes n = 1 in: M = 2^32 - 1 gives q = x - 1, r = 1, min(1, 0) = 0.)
//
// Small remainder:  x mod n for 0 <= x < 2^16 and 1 <= n < 2^13 (ranks against maxConcurrent) by the capacity form's
//   quotient with ANY reciprocal rn within 2 ulp of 1 / n, the hardware's estimate included: the error of
//   fmaf(x, rn, 0.5f * rn) is below 2^-21 * (x + 0.5) / n, far inside the 0.5 / n margin at this size, so no division
//   per lane is needed.  The host check perturbs the rounded reciprocal by an ulp either way.
#ifndef OWGS_DIVQ_H
#define OWGS_DIVQ_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OWGS_DIVQ_FN __host__ __device__ inline
#else
#define OWGS_DIVQ_FN inline
#endif

#define OWGS_DIVQ_XMAX (1 << 22)  // the capacity quotient is exact for operands below this
#define OWGS_DIVQ_MEM_ANY 4095    // ... and the capacity clamped to 1024 for any operand up to this divisor
#define OWGS_DIVQ_CAPMAX 1024     // the engine's capacity clamp (OWGS_CAPMAX; checked where the engine defines it)
#define OWGS_DIVQ_MAX_MEM 131071  // the largest memory limit (OWGS_MAX_MEM_MB; checked there too)

// the reciprocal of the capacity form (once per divisor); mem >= 1
OWGS_DIVQ_FN float owgs_divq_rm(int mem) { return 1.0f / (float)mem; }

// floor(x / mem) for 0 <= x < 2^22, with rm = owgs_divq_rm(mem), hrm = 0.5f * rm
OWGS_DIVQ_FN int owgs_divq_quot(int x, float rm, float hrm) { return (int)fmaf((float)x, rm, hrm); }

// min(floor(x / mem), qmax), 0 for x < 0 (domain: above)
OWGS_DIVQ_FN int owgs_divq_cap(int x, float rm, float hrm, int qmax) {
    const int xc = x < 0 ? 0 : (x < OWGS_DIVQ_XMAX ? x : OWGS_DIVQ_XMAX - 1);
    const int q = owgs_divq_quot(xc, rm, hrm);
    return q < qmax ? q : qmax;
}

// x mod n for 0 <= x < 2^16, 1 <= n < 2^13, rn within 2 ulp of 1 / n
OWGS_DIVQ_FN int owgs_divq_small_mod(int x, int n, float rn) { return x - n * (int)fmaf((float)x, rn, 0.5f * rn); }

// the multiplier of the position form (once per divisor: one 32-bit division); n >= 1
OWGS_DIVQ_FN uint32_t owgs_divq_magic(uint32_t n) { return 0xFFFFFFFFu / n; }

// (the compiler turns the high half of the 64-bit product into one mul_hi)
OWGS_DIVQ_FN uint32_t owgs_divq_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// x mod n with M = owgs_divq_magic(n)
OWGS_DIVQ_FN int owgs_divq_mod(int x, int n, uint32_t M) {
    const uint32_t q = owgs_divq_mulhi((uint32_t)x, M);
    const uint32_t r = (uint32_t)x - q * (uint32_t)n, rn = r - (uint32_t)n;
    return (int)(r < rn ? r : rn);
}

#endif
