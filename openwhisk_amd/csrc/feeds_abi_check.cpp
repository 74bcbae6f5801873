// feeds_abi_check.cpp -- the argument checks of the supervision-feed entry points (include/owgs.h) as a stand-alone
// host program, built with the host code under ASan/UBSan (make -C openwhisk_amd abicheck).  It needs no device: every
// call here must be refused before the engine is touched (the checks that need a context are in
// tests/test_gpu_feeds.py).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/owgs.h"

static int g_bad = 0;
#define EXPECT(call, want)                                                            \
    do {                                                                              \
        const int got_ = (call);                                                      \
        if (got_ != (want)) {                                                         \
            std::printf("FAIL line %d: %s = %d, want %d\n", __LINE__, #call, got_, (want)); \
            ++g_bad;                                                                  \
        }                                                                             \
    } while (0)

int main() {
    const char ping[] = "{\"name\":{\"instance\":1,\"userMemory\":\"1 MB\"}}";
    const int64_t off[2] = {0, (int64_t)std::strlen(ping)};
    const int64_t t[1] = {5};
    uint8_t kind[1], flags[1];
    int32_t inst[1], ticket[1], summary[3];
    int64_t mem[1];
    const char aid[33] = "0123456789abcdef0123456789abcdef";
    const int32_t inv[1] = {1};
    const uint8_t cfl[1] = {1};

    // no context
    EXPECT(owgs_process_pings(nullptr, 1, ping, off, t, 5, 0, kind, inst, mem, summary), OWGS_EINVAL);
    EXPECT(owgs_process_pings(nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr), OWGS_EINVAL);
    EXPECT(owgs_process_pings(nullptr, -1, ping, off, t, -1, 9, kind, inst, mem, summary), OWGS_EINVAL);
    EXPECT(owgs_process_acks_supervised(nullptr, 1, ping, off, kind, inst, ticket, flags, 5, 0, summary), OWGS_EINVAL);
    EXPECT(owgs_process_acks_supervised(nullptr, 1, ping, off, kind, inst, ticket, flags, -1, 3, nullptr), OWGS_EINVAL);
    EXPECT(owgs_complete_activations_supervised(nullptr, 1, aid, inv, cfl, kind, ticket, flags, 5, 0, summary), OWGS_EINVAL);
    EXPECT(owgs_complete_activations_supervised(nullptr, 1, aid, inv, cfl, kind, ticket, flags, int64_t(1) << 60, 2, summary),
           OWGS_EINVAL);

    // owgs_process_result_acks: no context, with and without a summary, a NULL out, a NULL member
    uint64_t aid2[2];
    int64_t roff[1];
    int32_t rlen[1];
    owgs_ack_out ao = {kind, inst, ticket, flags, aid2, roff, rlen};
    EXPECT(owgs_process_result_acks(nullptr, 1, ping, off, &ao, 5, 0, summary), OWGS_EINVAL);
    EXPECT(owgs_process_result_acks(nullptr, 1, ping, off, &ao, 0, 0, nullptr), OWGS_EINVAL);
    EXPECT(owgs_process_result_acks(nullptr, 1, ping, off, &ao, 7, 2, nullptr), OWGS_EINVAL);
    EXPECT(owgs_process_result_acks(nullptr, 1, ping, off, nullptr, -1, 3, summary), OWGS_EINVAL);
    EXPECT(owgs_process_result_acks(nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr), OWGS_EINVAL);
    EXPECT(owgs_process_result_acks(nullptr, -1, ping, off, &ao, 0, 0, nullptr), OWGS_EINVAL);
    ao.aid = nullptr;
    EXPECT(owgs_process_result_acks(nullptr, 1, ping, off, &ao, 0, 0, nullptr), OWGS_EINVAL);

    // owgs_publish_activations: no context, no io, no summary
    const int32_t act[1] = {0};
    const uint64_t words[2] = {1, 2};
    const int64_t lim[1] = {100};
    uint8_t existed[1];
    int64_t psum[8];
    owgs_publish_io io;
    std::memset(&io, 0, sizeof io);
    io.n = 1;
    io.action = act;
    io.aid = words;
    io.ticket = inv;
    io.time_limit_ms = lim;
    io.out_invoker = inst;
    io.out_flags = flags;
    io.out_ticket = ticket;
    io.out_existed = existed;
    EXPECT(owgs_publish_activations(nullptr, &io, nullptr, nullptr, psum), OWGS_EINVAL);
    EXPECT(owgs_publish_activations(nullptr, nullptr, nullptr, nullptr, psum), OWGS_EINVAL);
    EXPECT(owgs_publish_activations(nullptr, &io, nullptr, nullptr, nullptr), OWGS_EINVAL);

    std::printf(g_bad ? "feeds_abi_check: %d failures\n" : "feeds_abi_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
