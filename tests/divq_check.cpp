// divq_check.cpp -- stand-alone host check of openwhisk_amd/csrc/owgs_divq.h against the integer / and %
// (tests/test_divq_cpu.py builds and runs it with the system C++ compiler; no device, no library).  Prints one line per section and exits non-zero on
// the first mismatch.
#include <cstdio>
#include <cstdlib>

#include "owgs_divq.h"

static const int CAPMAX = OWGS_DIVQ_CAPMAX;       // (the engine asserts that these are its own)
static const int MAX_MEM_MB = OWGS_DIVQ_MAX_MEM;
static long long g_points = 0;

static int cap_ref(long long x, int mem, int qmax) {
    if (x < 0) x = 0;
    const long long q = x / mem;
    return (int)(q < qmax ? q : qmax);
}

static bool cap_check(int x, int mem, float rm, float hrm) {
    ++g_points;
    // unclamped (the quotient itself) and with the engine's clamp
    const int big = 0x7FFFFFFF;
    if (owgs_divq_cap(x, rm, hrm, big) != cap_ref(x, mem, big) || owgs_divq_cap(x, rm, hrm, CAPMAX) != cap_ref(x, mem, CAPMAX)) {
        std::printf("capacity mismatch: x=%d mem=%d got %d want %d\n", x, mem, owgs_divq_cap(x, rm, hrm, big),
                    cap_ref(x, mem, big));
        return false;
    }
    return true;
}

static bool mod_check(int x, int n, uint32_t M) {
    ++g_points;
    const int r = owgs_divq_mod(x, n, M);
    if (r != x % n) {
        std::printf("position mismatch: x=%d n=%d got %d want %d\n", x, n, r, x % n);
        return false;
    }
    return true;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng_next() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    // ---- capacity: every mem, every multiple boundary below 2^22, negative operands, the clamp
    for (int mem = 1; mem <= MAX_MEM_MB; ++mem) {
        const float rm = owgs_divq_rm(mem), hrm = 0.5f * rm;
        for (long long km = 0; km <= OWGS_DIVQ_XMAX; km += mem) {
            for (long long x = km - 1; x <= km + 1; ++x)
                if (x >= 0 && x < OWGS_DIVQ_XMAX && !cap_check((int)x, mem, rm, hrm)) return 1;
            const long long xh = km + mem / 2;
            if (xh < OWGS_DIVQ_XMAX && !cap_check((int)xh, mem, rm, hrm)) return 1;
        }
        if (!cap_check(OWGS_DIVQ_XMAX - 1, mem, rm, hrm)) return 1;
        const int neg[] = {-1, -mem, -mem - 1, -OWGS_DIVQ_XMAX, -(1 << 29), (int)0x80000000};
        for (int x : neg)
            if (!cap_check(x, mem, rm, hrm)) return 1;
        // the clamp's edge: CAPMAX * mem - 1, CAPMAX * mem, where the domain reaches it
        const long long ce = (long long)CAPMAX * mem;
        for (long long x = ce - 1; x <= ce + 1; ++x)
            if (x < OWGS_DIVQ_XMAX && !cap_check((int)x, mem, rm, hrm)) return 1;
    }
    std::printf("capacity: %lld points, 0 mismatches\n", g_points);

    // ---- capacity with the engine's clamp, operands of 2^22 and more: exact for every mem up to OWGS_DIVQ_MEM_ANY
    // (the clamped operand's quotient already reaches CAPMAX), and not beyond it
    g_points = 0;
    for (int mem = 1; mem <= OWGS_DIVQ_MEM_ANY + 1; ++mem) {
        const float rm = owgs_divq_rm(mem), hrm = 0.5f * rm;
        const long long xs[] = {OWGS_DIVQ_XMAX, OWGS_DIVQ_XMAX + 1, (1ll << 23) + 1, (1ll << 24) + 3, (1ll << 27) - 1,
                                (1ll << 29) - 1, (1ll << 30), 0x7FFFFFFFll, (long long)CAPMAX * mem + (1ll << 22)};
        for (long long x : xs) {
            ++g_points;
            const bool same = owgs_divq_cap((int)x, rm, hrm, CAPMAX) == cap_ref(x, mem, CAPMAX);
            if (same != (mem <= OWGS_DIVQ_MEM_ANY)) {
                std::printf("clamped capacity: x=%lld mem=%d %s\n", x, mem, same ? "exact beyond the bound" : "mismatch");
                return 1;
            }
        }
    }
    std::printf("clamped capacity: %lld points, exact up to mem %d, not at %d\n", g_points, OWGS_DIVQ_MEM_ANY,
                OWGS_DIVQ_MEM_ANY + 1);

    // ---- capacity beyond the domain: the form is wrong somewhere from 2^23 on (why the engine bounds its permits)
    {
        long long bad = 0;
        int bx = 0, bm = 0;
        for (int mem = 1; mem <= 4096 && !bad; ++mem) {
            const float rm = owgs_divq_rm(mem), hrm = 0.5f * rm;
            for (long long km = ((1ll << 23) / mem) * mem; km < (1ll << 25); km += mem) {
                for (long long x = km - 1; x <= km + 1; ++x) {
                    if (x < (1ll << 23)) continue;
                    if (owgs_divq_quot((int)x, rm, hrm) != cap_ref(x, mem, 0x7FFFFFFF)) {
                        if (!bad) bx = (int)x, bm = mem;
                        ++bad;
                    }
                }
            }
        }
        if (!bad) {
            std::printf("beyond: no mismatch found at x >= 2^23 (the documented limit does not hold)\n");
            return 1;
        }
        std::printf("beyond: first mismatch at x=%d mem=%d (x >= 2^23)\n", bx, bm);
    }

    // ---- position: every n, boundaries at a strided set of multiples with the first and the last, random operands
    g_points = 0;
    const long long XL = 1ll << 31;
    for (int n = 1; n < (1 << 15); ++n) {
        const uint32_t M = owgs_divq_magic((uint32_t)n);
        const long long kl = (XL - 1) / n;  // the last multiple below 2^31
        const long long stride = kl / 97 + 1;
        for (long long k = 0;; k += stride) {
            if (k > kl) k = kl;
            const long long km = k * n;
            for (long long x = km - 1; x <= km + 1; ++x)
                if (x >= 0 && x < XL && !mod_check((int)x, n, M)) return 1;
            if (k == kl) break;
        }
        // (the first multiples one by one: small operands are the common ones)
        for (int x = 0; x < 4 * n + 2; x += (x < 8 ? 1 : n - 1 > 0 ? n - 1 : 1))
            if (!mod_check(x, n, M)) return 1;
        if (!mod_check(0x7FFFFFFF, n, M)) return 1;
        for (int j = 0; j < 128; ++j)
            if (!mod_check((int)(rng_next() >> 33), n, M)) return 1;
    }
    for (int j = 0; j < 4000000; ++j) {
        const uint64_t z = rng_next();
        const int n = 1 + (int)((z & 0xFFFFFFFFu) % ((1u << 15) - 1));
        if (!mod_check((int)(z >> 33), n, owgs_divq_magic((uint32_t)n))) return 1;
    }
    std::printf("position: %lld points, 0 mismatches\n", g_points);

    // ---- small remainder: every n below 2^13, every multiple boundary below 2^16, the rounded reciprocal and its
    // neighbours one and two ulp away (what a hardware estimate may return)
    g_points = 0;
    for (int n = 1; n < (1 << 13); ++n) {
        const float r0 = owgs_divq_rm(n);
        float rs[5] = {r0, std::nextafterf(r0, 0.0f), std::nextafterf(r0, 2.0f), 0.0f, 0.0f};
        rs[3] = std::nextafterf(rs[1], 0.0f);
        rs[4] = std::nextafterf(rs[2], 2.0f);
        for (float rn : rs)
            for (int km = 0; km <= (1 << 16); km += n)
                for (int x = km - 1; x <= km + 1; ++x) {
                    if (x < 0 || x >= (1 << 16)) continue;
                    ++g_points;
                    if (owgs_divq_small_mod(x, n, rn) != x % n) {
                        std::printf("small remainder mismatch: x=%d n=%d\n", x, n);
                        return 1;
                    }
                }
    }
    std::printf("small remainder: %lld points, 0 mismatches\n", g_points);
    std::printf("OK\n");
    return 0;
}
