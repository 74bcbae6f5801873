// invoke_abi_check.cpp -- owgs_invoke_activations' share of the C ABI (include/owgs.h) as a stand-alone host program.
//
// Always: prints the layout of owgs_invoke_io and the constants the Python binding restates, one `name value` pair per
// line (tests/test_invoke_cpu.py compiles this file alone with the host compiler and compares with openwhisk_amd/_lib.py).
// With -DOWGS_ABI_LINKED (make -C openwhisk_amd abicheck: linked with the host code under ASan/UBSan, no device needed):
// the argument errors that are refused before the engine is touched.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/owgs.h"

#define SHOW_OFF(f) std::printf("offset.%s %zu\n", #f, offsetof(owgs_invoke_io, f))
#define SHOW_CONST(c) std::printf("const.%s %d\n", #c, (int)(c))

#ifdef OWGS_ABI_LINKED
static int g_bad = 0;
#define EXPECT(call, want)                                                            \
    do {                                                                              \
        const int got_ = (call);                                                      \
        if (got_ != (want)) {                                                         \
            std::printf("FAIL line %d: %s = %d, want %d\n", __LINE__, #call, got_, (want)); \
            ++g_bad;                                                                  \
        }                                                                             \
    } while (0)
#endif

int main() {
    std::printf("sizeof.owgs_invoke_io %zu\n", sizeof(owgs_invoke_io));
    SHOW_OFF(n);
    SHOW_OFF(ns);
    SHOW_OFF(kind);
    SHOW_OFF(t_ms);
    SHOW_OFF(rate_override);
    SHOW_OFF(conc_override);
    SHOW_OFF(action);
    SHOW_OFF(seq);
    SHOW_OFF(seq_base);
    SHOW_OFF(aid);
    SHOW_OFF(ticket);
    SHOW_OFF(time_limit_ms);
    SHOW_OFF(now_ms);
    SHOW_OFF(out_verdict);
    SHOW_OFF(out_rate_count);
    SHOW_OFF(out_rate_limit);
    SHOW_OFF(out_conc_count);
    SHOW_OFF(out_conc_limit);
    SHOW_OFF(out_invoker);
    SHOW_OFF(out_flags);
    SHOW_OFF(out_ticket);
    SHOW_OFF(out_existed);
    SHOW_CONST(OWGS_ABI_VERSION);
    SHOW_CONST(OWGS_NOT_PUBLISHED);
    SHOW_CONST(OWGS_NONE);
    SHOW_CONST(OWGS_THROW_INDEX);
    SHOW_CONST(OWGS_ADMIT_OK);
    SHOW_CONST(OWGS_ADMIT_RATE);
    SHOW_CONST(OWGS_ADMIT_CONCURRENT);
    SHOW_CONST(OWGS_ADMIT_TRIGGER);
    SHOW_CONST(OWGS_ADMIT_RATE_OVERRIDE);
    SHOW_CONST(OWGS_ADMIT_CONC_OVERRIDE);
#ifdef OWGS_ABI_LINKED
    const int32_t ns[1] = {0}, act[1] = {0}, tick[1] = {7};
    const uint8_t kind[1] = {0};
    const int64_t t[1] = {5}, lim[1] = {100};
    const uint64_t words[2] = {1, 2};
    uint8_t ver[1], fl[1], ex[1];
    int32_t rc[1], rl[1], cc[1], cl[1], inv[1], ot[1];
    int64_t summ[16];
    owgs_invoke_io io;
    std::memset(&io, 0, sizeof io);
    io.n = 1;
    io.ns = ns;
    io.kind = kind;
    io.t_ms = t;
    io.action = act;
    io.aid = words;
    io.ticket = tick;
    io.time_limit_ms = lim;
    io.out_verdict = ver;
    io.out_rate_count = rc;
    io.out_rate_limit = rl;
    io.out_conc_count = cc;
    io.out_conc_limit = cl;
    io.out_invoker = inv;
    io.out_flags = fl;
    io.out_ticket = ot;
    io.out_existed = ex;
    owgs_msg_batch mb;
    std::memset(&mb, 0, sizeof mb);
    owgs_msg_out mo;
    std::memset(&mo, 0, sizeof mo);
    // no context, no io, no summary
    EXPECT(owgs_invoke_activations(nullptr, &io, nullptr, nullptr, summ), OWGS_EINVAL);
    EXPECT(owgs_invoke_activations(nullptr, nullptr, nullptr, nullptr, summ), OWGS_EINVAL);
    EXPECT(owgs_invoke_activations(nullptr, &io, nullptr, nullptr, nullptr), OWGS_EINVAL);
    // refused before the context is looked at: a stand-in that is never dereferenced
    alignas(16) static char fake[64];
    owgs_ctx* fc = (owgs_ctx*)fake;
    EXPECT(owgs_invoke_activations(fc, nullptr, nullptr, nullptr, summ), OWGS_EINVAL);
    EXPECT(owgs_invoke_activations(fc, &io, &mb, nullptr, summ), OWGS_EINVAL);  // msgs without mo
    EXPECT(owgs_invoke_activations(fc, &io, nullptr, &mo, summ), OWGS_EINVAL);  // mo without msgs
    io.n = -1;
    EXPECT(owgs_invoke_activations(fc, &io, nullptr, nullptr, summ), OWGS_EINVAL);
    io.n = 1;
    const void** req[] = {(const void**)&io.ns, (const void**)&io.kind, (const void**)&io.t_ms, (const void**)&io.action,
                          (const void**)&io.aid, (const void**)&io.ticket, (const void**)&io.time_limit_ms,
                          (const void**)&io.out_verdict, (const void**)&io.out_rate_count,
                          (const void**)&io.out_rate_limit, (const void**)&io.out_conc_count,
                          (const void**)&io.out_conc_limit, (const void**)&io.out_invoker, (const void**)&io.out_flags,
                          (const void**)&io.out_ticket, (const void**)&io.out_existed};
    for (const void** p : req) {  // a NULL among the required pointers
        const void* keep = *p;
        *p = nullptr;
        EXPECT(owgs_invoke_activations(fc, &io, nullptr, nullptr, summ), OWGS_EINVAL);
        *p = keep;
    }
    std::printf(g_bad ? "invoke_abi_check: %d failures\n" : "invoke_abi_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
#else
    return 0;
#endif
}
