// events_abi_check.cpp -- the throttle-gate events' share of the C ABI (include/owgs.h) as a stand-alone host program.
//
// Always: prints the layout of owgs_event_io and the constants the Python binding restates, one `name value` pair per
// line (tests/test_events_cpu.py compiles this file alone with the host compiler and compares with openwhisk_amd/_lib.py).
// With -DOWGS_ABI_LINKED (make -C openwhisk_amd abicheck: linked with the host code under ASan/UBSan, no device needed):
// the argument errors of owgs_set_event_source, owgs_register_event_identities, owgs_throttle_events and
// owgs_invoke_activations_events that are refused before the context is looked at.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/owgs.h"

#define SHOW_OFF(f) std::printf("offset.%s %zu\n", #f, offsetof(owgs_event_io, f))
#define SHOW_CONST(c) std::printf("const.%s %lld\n", #c, (long long)(c))

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
    std::printf("sizeof.owgs_event_io %zu\n", sizeof(owgs_event_io));
    SHOW_OFF(ident);
    SHOW_OFF(ev_out);
    SHOW_OFF(ev_cap);
    SHOW_OFF(ev_off);
    SHOW_OFF(rej_out);
    SHOW_OFF(rej_cap);
    SHOW_OFF(rej_off);
    SHOW_OFF(ev_total);
    SHOW_OFF(rej_total);
    SHOW_OFF(n_events);
    SHOW_OFF(n_rejects);
    SHOW_CONST(OWGS_ABI_VERSION);
    SHOW_CONST(OWGS_EVENT_NAME_MAX);
    SHOW_CONST(OWGS_EVENT_MAX_FIXED);
    SHOW_CONST(OWGS_REJECT_TEXT_MAX);
    SHOW_CONST(OWGS_ADMIT_OK);
    SHOW_CONST(OWGS_ADMIT_RATE);
    SHOW_CONST(OWGS_ADMIT_CONCURRENT);
    SHOW_CONST(OWGS_ADMIT_TRIGGER);
#ifdef OWGS_ABI_LINKED
    const uint8_t kind[1] = {0}, ver[1] = {0};
    const int32_t cnt[1] = {1}, ident[1] = {0};
    const int64_t ts[1] = {5};
    int64_t ev_off[2] = {-7, -7}, rej_off[2] = {-7, -7}, summ[16];
    char ev_out[8], rej_out[8];
    owgs_event_io ev;
    std::memset(&ev, 0, sizeof ev);
    ev.ident = ident;
    ev.ev_out = ev_out;
    ev.ev_cap = sizeof ev_out;
    ev.ev_off = ev_off;
    ev.rej_out = rej_out;
    ev.rej_cap = sizeof rej_out;
    ev.rej_off = rej_off;
    const int64_t off2[2] = {0, 0};
    // no context
    EXPECT(owgs_set_event_source(nullptr, "\"c\"", 3), OWGS_EINVAL);
    EXPECT(owgs_register_event_identities(nullptr, 1, "", off2, "", off2, nullptr), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(nullptr, 1, kind, ver, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    // refused before the context is looked at: a stand-in that is never dereferenced
    alignas(16) static char fake[64];
    owgs_ctx* fc = (owgs_ctx*)fake;
    EXPECT(owgs_set_event_source(fc, "\"c\"", -1), OWGS_EINVAL);
    EXPECT(owgs_set_event_source(fc, nullptr, 3), OWGS_EINVAL);
    EXPECT(owgs_register_event_identities(fc, -1, "", off2, "", off2, nullptr), OWGS_EINVAL);
    EXPECT(owgs_register_event_identities(fc, 1, "", nullptr, "", off2, nullptr), OWGS_EINVAL);
    EXPECT(owgs_register_event_identities(fc, 1, "", off2, "", nullptr, nullptr), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, cnt, cnt, ts, nullptr), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, -1, kind, ver, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, nullptr, ver, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, nullptr, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, nullptr, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, nullptr, cnt, cnt, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, nullptr, cnt, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, cnt, nullptr, ts, &ev), OWGS_EINVAL);
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, cnt, cnt, nullptr, &ev), OWGS_EINVAL);
    const void** req[] = {(const void**)&ev.ident, (const void**)&ev.ev_out, (const void**)&ev.ev_off,
                          (const void**)&ev.rej_out, (const void**)&ev.rej_off};
    for (const void** p : req) {  // a NULL among the required pointers of ev
        const void* keep = *p;
        *p = nullptr;
        EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
        *p = keep;
    }
    ev.ev_cap = -1;
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    ev.ev_cap = sizeof ev_out;
    ev.rej_cap = -1;
    EXPECT(owgs_throttle_events(fc, 1, kind, ver, cnt, cnt, cnt, cnt, ts, &ev), OWGS_EINVAL);
    // the integrated call: ev's own errors come before the context is looked at, as io's do
    const int32_t ns[1] = {0}, act[1] = {0}, tick[1] = {7};
    const int64_t lim[1] = {100};
    const uint64_t words[2] = {1, 2};
    uint8_t o8[3][1];
    int32_t o32[6][1];
    owgs_invoke_io io;
    std::memset(&io, 0, sizeof io);
    io.n = 1;
    io.ns = ns;
    io.kind = kind;
    io.t_ms = ts;
    io.action = act;
    io.aid = words;
    io.ticket = tick;
    io.time_limit_ms = lim;
    io.out_verdict = o8[0];
    io.out_flags = o8[1];
    io.out_existed = o8[2];
    io.out_rate_count = o32[0];
    io.out_rate_limit = o32[1];
    io.out_conc_count = o32[2];
    io.out_conc_limit = o32[3];
    io.out_invoker = o32[4];
    io.out_ticket = o32[5];
    EXPECT(owgs_invoke_activations_events(fc, &io, nullptr, nullptr, &ev, summ), OWGS_EINVAL);  // rej_cap < 0
    ev.rej_cap = sizeof rej_out;
    ev.ident = nullptr;
    EXPECT(owgs_invoke_activations_events(fc, &io, nullptr, nullptr, &ev, summ), OWGS_EINVAL);
    ev.ident = ident;
    EXPECT(owgs_invoke_activations_events(nullptr, &io, nullptr, nullptr, &ev, summ), OWGS_EINVAL);
    EXPECT(owgs_invoke_activations_events(fc, nullptr, nullptr, nullptr, &ev, summ), OWGS_EINVAL);
    EXPECT(owgs_invoke_activations_events(fc, &io, nullptr, nullptr, &ev, nullptr), OWGS_EINVAL);
    io.out_verdict = nullptr;
    EXPECT(owgs_invoke_activations_events(fc, &io, nullptr, nullptr, &ev, summ), OWGS_EINVAL);
    if (ev_off[0] != -7 || rej_off[0] != -7 || ev.ev_total || ev.n_events) {
        std::printf("FAIL: a refused call wrote an output\n");
        ++g_bad;
    }
    std::printf(g_bad ? "events_abi_check: %d failures\n" : "events_abi_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
#else
    return 0;
#endif
}
