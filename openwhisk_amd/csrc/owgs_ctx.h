// owgs_ctx.h -- the host runtime's context (struct owgs_ctx), the types that own its GPU resources, and the helpers
// the owgs_host*.cpp files share.  Host side only; the device-side layout is owgs_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/owgs.h"
#include "owgs_internal.h"
#include "owgs_launch.h"

typedef unsigned long long u64;

// diagnostic environment switches, read once per process (not on every call)
struct EnvOpts {
    int opts = 0, cw = 0, deal = -1, variant = -1;
    bool trace = false, feat_all = false;
    // owgs_process_batch through the resident engine: on/off, the largest call (releases + publishes) it takes, and
    // its idle time before it writes the state back and exits (OWGS_RESIDENT=0 sends every call down the chain)
    int res = 1, res_max = 1024;
    long long res_idle_us = 20000;
    // ... and its lifetime: it exits between calls once this long after its launch even when busy (it holds a hardware
    // queue that another context's stream may share; GPU_MAX_HW_QUEUES is 4), the next call relaunches it
    long long res_life_us = 100000;
    // watched pairs (after updateCluster) on the resident engine (0: such calls take the launch chain, as in round 4)
    int res_watch = 1;
    int res_eager = 1;  // OWGS_RES_EAGER=0: after a chained call the engine is relaunched by the next small call only
    // (tests) the doorbell's and the walk-cursor generation's values at the context's first launch: start a context
    // just below their wrap limits
    long long res_call_base = 0, res_gen_base = 0;
    // the resident engine's speculative walks: walk steps each publish probes on its own before the in-order
    // validation (0: every decision walked one at a time)
    int res_spec = 16;
    int res_cspec = 0;  // OWGS_RES_CSPEC: walk steps a concurrent publish speculates (0: max(4, res_spec / 4))
    int res_cspec_pre = 0;  // OWGS_RES_CSPEC_PRE: ... when the helper speculates the next chunk ahead (0: as above)
    int res_split = 1;  // OWGS_RES_SPLIT: helper waves (0-3) for the concurrent speculation; 0 = wave 0 itself
    // OWGS_RES_PRE=0: the helper wave does not speculate a run's next chunk while wave 0 decides the current one
    int res_pre = 1;
    // owgs_replay_device through the resident engine's stream mode (one wave deciding, speculative walks) instead of
    // the chunked engine, where it applies (identity pools, no watched pairs)
    int spec_replay = 0;
    EnvOpts() {
        if (const char* e = getenv("OWGS_SPEC_REPLAY")) spec_replay = atoi(e);
        if (const char* e = getenv("OWGS_RESIDENT")) res = atoi(e);
        if (const char* e = getenv("OWGS_RES_SPEC")) res_spec = atoi(e);
        if (const char* e = getenv("OWGS_RES_CSPEC")) res_cspec = atoi(e);
        if (const char* e = getenv("OWGS_RES_CSPEC_PRE")) res_cspec_pre = atoi(e);
        if (const char* e = getenv("OWGS_RES_SPLIT")) res_split = atoi(e);
        if (const char* e = getenv("OWGS_RES_PRE")) res_pre = atoi(e);
        if (const char* e = getenv("OWGS_RES_MAX")) res_max = atoi(e);
        if (const char* e = getenv("OWGS_RES_IDLE_US")) res_idle_us = atoll(e);
        if (const char* e = getenv("OWGS_RES_LIFE_US")) res_life_us = atoll(e);
        if (const char* e = getenv("OWGS_RES_WATCH")) res_watch = atoi(e);
        if (const char* e = getenv("OWGS_RES_EAGER")) res_eager = atoi(e);
        if (const char* e = getenv("OWGS_RES_CALL_BASE")) res_call_base = atoll(e);
        if (const char* e = getenv("OWGS_RES_GEN_BASE")) res_gen_base = atoll(e);
        feat_all = getenv("OWGS_FEAT_ALL") != nullptr;  // the general engine for every launch (A/B diagnostics)
        if (const char* e = getenv("OWGS_VARIANT")) variant = atoi(e);  // force an engine geometry (diagnostics)
        if (const char* o = getenv("OWGS_OPTS")) opts = atoi(o);
        if (const char* e = getenv("OWGS_CW")) cw = atoi(e);
        if (const char* e = getenv("OWGS_DEAL")) deal = atoi(e);
        trace = getenv("OWGS_TRACE_FILE") != nullptr;
    }
};
inline const EnvOpts& env_opts() {  // (inline: one instance for every file of the library)
    static const EnvOpts e;
    return e;
}

// ------------------------------------------------------------------------------------------------ owning types
// Every device allocation, pinned host block, event and stream of the library belongs to one of the four types
// below and is freed by its destructor.  live_resources counts what exists, process-wide, for owgs_live_resources
// (diagnostics): one relaxed atomic step where a resource is made or freed, never on a per-call path.
enum { LIVE_DEVICE = 0, LIVE_PINNED = 1, LIVE_SYNC = 2 };
inline std::atomic<int64_t> live_resources[3];
inline void live_step(int kind, int64_t d) { live_resources[kind].fetch_add(d, std::memory_order_relaxed); }

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf& operator=(DevBuf&& o) noexcept {  // takes o's allocation (a grown table replacing the old one)
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t m) {
        if (m <= n && p) return hipSuccess;
        release();
        size_t bytes = (m ? m : 1) * sizeof(T);
        hipError_t e = hipMalloc((void**)&p, bytes);
        if (e == hipSuccess) {
            n = m ? m : 1;
            live_step(LIVE_DEVICE, 1);
        } else {
            p = nullptr;
        }
        return e;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            live_step(LIVE_DEVICE, -1);
        }
        p = nullptr;
        n = 0;
    }
};

// a pinned host block (hipHostMalloc).  reserve allocates exactly `bytes` unless the block already holds as many:
// how far ahead a block grows (usually twice the call's need) and its flags are each call site's choice.
template <class T = void>
struct Pinned {
    T* p = nullptr;
    size_t bytes = 0;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { release(); }
    hipError_t reserve(size_t b, unsigned flags) {
        if (p && b <= bytes) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void**)&p, b, flags);
        if (e == hipSuccess) {
            bytes = b;
            live_step(LIVE_PINNED, 1);
        } else {
            p = nullptr;
        }
        return e;
    }
    void release() {
        if (p) {
            (void)hipHostFree(p);
            live_step(LIVE_PINNED, -1);
        }
        p = nullptr;
        bytes = 0;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) {
            (void)hipEventDestroy(e);
            live_step(LIVE_SYNC, -1);
        }
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r == hipSuccess) live_step(LIVE_SYNC, 1);
        else e = nullptr;
        return r;
    }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) {
            (void)hipStreamDestroy(s);
            live_step(LIVE_SYNC, -1);
        }
    }
    hipError_t create(unsigned flags) {
        hipError_t r = hipStreamCreateWithFlags(&s, flags);
        if (r == hipSuccess) live_step(LIVE_SYNC, 1);
        else s = nullptr;
        return r;
    }
    operator hipStream_t() const { return s; }
};

struct owgs_ctx {
    // Destruction order comes from member order: C++ destroys members last to first, so the streams (declared first)
    // go last, the events before them, and every buffer and pinned block (all declared further down) before the
    // events.  owgs_destroy quiesces the resident engine and drains the stream, then deletes the context.
    Stream stream;
    // owgs_process_batch through the resident engine (owgs_resident.hip): its stream
    Stream res_stream;
    static constexpr int OVF_PROBES = 4;
    Event ev_ovf[OVF_PROBES];   // the overflow's entry-count probes (h_ovf_cnt below)
    Event ev_status;            // owgs_update_health_device's copy of the status bytes (status_stale below)
    // calls on one context are ordered as issued, whatever stream each names: ev_tail marks the end of the last
    // asynchronous call's work (on tail_stream); later work on another stream waits for it (order_on / tail_mark)
    Event ev_tail;
    Event ev_margs;             // recorded after the last engine launch that reads d_margs / h_margs
    Event ev_engine[2];         // around the last owgs_engine_kernel launch
    Event ev_res;               // the resident engine's launch

    owgs_config cfg{};
    double mf = 0, bf = 0;
    std::string err;

    // ShardingContainerPoolBalancerState mirror
    std::vector<int32_t> ids;
    std::vector<int64_t> mem;
    std::vector<uint8_t> status;
    int32_t managed = 0, blackboxes = 0;
    std::vector<int32_t> msteps, bsteps;
    int32_t cluster = 1;
    int32_t n_slots = 0;
    bool pool_override[2] = {false, false};
    std::vector<int32_t> ov_ids[2];
    std::vector<uint8_t> ov_status[2];

    // derived pools
    int32_t nm = 0, nb = 0, hm = 0, hb = 0, shortcut_ok = 3;
    int32_t pool_mode = 0, n_ids = 0;  // 0: pool position p -> id p (managed) / N - nb + p (blackbox)

    // actions
    std::vector<int32_t> a_mem, a_maxc, a_slot, a_hash;
    std::vector<uint8_t> a_bb, a_cok, a_live;
    std::vector<int32_t> free_handles;  // released action handles (owgs_release_actions), reused by registrations
    std::vector<int32_t> slot_uses, slot_maxc, slot_mem;  // per fqn@version key: live handles naming it, its limits
    std::vector<std::string> slot_name;
    std::unordered_map<std::string, int32_t> slot_ids;
    // keys no live handle names: recycled (slot id reused) once no map entry and no watched pair names them any more,
    // checked on the device when registrations run out of ids (reclaim_slots); slot_epoch counts recycled keys
    std::vector<int32_t> pending_slots, free_slots;
    int64_t slot_epoch = 0, snap_slot_epoch = 0;
    DevBuf<uint32_t> d_cand;

    // device state
    DevBuf<int32_t> d_permits, d_pool_words, d_hlist, d_act_slot, d_act_hash, d_act_mem, d_act_maxc, d_steps,
        d_cpx, d_err;
    // the primary table's entries right after the chunked engine's last rebuild of it, kept across launches (a
    // launch rebuilds once its entries grew by OWGS_CTC / 8 since then; 0 after a restore: as if never rebuilt)
    DevBuf<int32_t> d_clast;
    int32_t steps_stride = 0;  // d_steps = [managed list | blackbox list], each steps_stride entries
    DevBuf<int64_t> d_mem_bytes;  // userMemory of every invoker (updateCluster recomputes all slots from it)
    DevBuf<uint8_t> d_status;
    DevBuf<uint32_t> d_usable, d_ct_keys, d_ct_vals, d_ct_tmp;
    DevBuf<uint8_t> d_act_bb, d_act_cok;
    DevBuf<uint2> d_act_meta;
    DevBuf<u64> d_stats;
    // NestedSemaphore map overflow (keys beyond the LDS-sized primary table, owgs_internal.h OwgsOvf)
    DevBuf<uint2> d_ovf, s_ovf;
    DevBuf<uint32_t> d_ovf_rc;
    DevBuf<int32_t> d_ovf_touched, d_ovf_cnt;  // d_ovf_cnt = {entries (live + deleted), touched count}
    int32_t ovf_cap = 0;
    int64_t ovf_used_ub = 0;  // host upper bound of the overflow's entries (exact after a read-back)
    // the overflow's entry count copied back after engine launches without waiting (a ring of pinned words +
    // events, ev_ovf): read when the bound above runs out.  A probe that has arrived replaces the bound; otherwise the
    // host waits for an OLDER probe than the newest -- the launches after it keep the GPU busy meanwhile -- instead of
    // draining the stream (a batch-by-batch replay then never idles the engine stream on this bound)
    Pinned<int32_t> h_ovf_cnt;                      // [OVF_PROBES]
    bool ovf_probe[OVF_PROBES] = {};                // slot recorded and not yet consumed
    int64_t ovf_probe_added[OVF_PROBES] = {};       // ovf_added at the slot's recording (its launch included)
    int64_t ovf_added = 0;                          // activations ever added to the bound
    int ovf_probe_next = 0;
    // owgs_update_health_device on identity pools: the status bytes and usable bitmap are updated on the device only;
    // the host mirror (status, healthy counts) is downloaded when a host path needs it (ev_status: the copy)
    bool status_stale = false;
    hipStream_t tail_stream = nullptr;  // (not owned: the stream ev_tail was recorded on)
    bool tail_valid = false;
    int32_t s_ovf_cnt = 0;    // snapshot: overflow entries (0: the snapshot had none)
    int32_t s_ovf_cap = 0;
    DevBuf<uint32_t> d_margs;  // owgs_replay_device_multi: shard argument blocks beyond the kernarg segment
    Pinned<> h_margs;          // pinned staging of d_margs
    bool ev_margs_valid = false;
    // per-call scratch
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_a, d_b, d_c, d_d, d_out, d_cstart, d_relx, d_relcnt, d_xslot;
    DevBuf<uint8_t> d_flags, d_rflags;
    DevBuf<u64> d_seq;
    DevBuf<int64_t> d_rel;
    DevBuf<uint4> d_rec;
    DevBuf<uint32_t> d_lix;
    DevBuf<uint32_t> d_gcur;  // per-action walk cursors (tagged by batch)
    DevBuf<unsigned long long> d_trace;  // barrier timeline (diagnostic builds, env OWGS_TRACE_FILE)
    int32_t cur_tag = 0;      // tags used so far (wraps with a clear of d_gcur)
    DevBuf<uint2> d_rel_rec, d_xmeta;
    // activationSlots (owgs_acks.hip)
    DevBuf<unsigned long long> t_tw;
    DevBuf<ulonglong2> t_tk;
    DevBuf<int2> t_tv;
    DevBuf<int32_t> t_tn, t_owner;
    long long t_cap = 0, t_used = 0, t_live = 0;
    // completion-ack timeouts (owgs_expire.hip): per-slot deadline / entry invoker / arm sequence, the per-tile summary,
    // calculateCompletionAckTimeout's three settings (CLB:103-105), the arm-sequence counter, the sweep's scratch and
    // its counters (owgs_expiry_stats)
    DevBuf<long long> t_td, t_tmin, x_d, x_tl, x_outd;
    DevBuf<int32_t> t_ti, x_slot, x_idx0, x_idx1, x_cnt, x_inv;
    DevBuf<unsigned long long> t_tq, x_q, x_key, x_key_s;
    DevBuf<uint8_t> x_temp;
    long long a_std = 60000, a_factor = 2, a_addon = 60000;
    unsigned long long arm_seq = 0;
    long long x_sweeps = 0, x_tiles = 0, x_tiles_last = 0, x_expired = 0;
    // the in-flight books (CLB:62-65): namespace uuid -> dense handle, the per-namespace counters on the device
    // (int32, ns_cap entries, zero beyond the registered handles), the three totals on the host (folded in from each
    // call's counter words at the synchronisation the call ends with)
    std::map<std::pair<uint64_t, uint64_t>, int32_t> ns_map;
    DevBuf<int32_t> d_ns_active, q_key, q_idx0, q_idx1;
    DevBuf<uint8_t> q_temp;
    int32_t ns_cap = 0;
    // the entitlement throttle gate (owgs_admit_batch): the RateInfo records of the two rate throttlers, entry
    // which * ns_cap + handle (lastMin OWGS_RATE_ABSENT, count 0: never checked), grown with d_ns_active; the three
    // system defaults (Entitlement.scala:138, 142, 153; ansible/group_vars/all:73-75); its output block on the device
    // ([4 n] int32 then [n] verdict bytes) and the pinned host block it is read back into with one copy
    DevBuf<long long> d_rate_min, g_min;
    DevBuf<int32_t> d_rate_cnt, g_out;
    Pinned<> g_pin;
    int32_t lim_invoke = 60, lim_fire = 60, lim_conc = 30;
    long long f_total = 0, f_mb_managed = 0, f_mb_blackbox = 0;
    long long health_ms = 0;
    DevBuf<ulonglong2> k_key;
    DevBuf<uint8_t> k_info, k_state, k_kind, k_oflags, k_bytes, k_cfl;
    DevBuf<int32_t> k_inst, k_slot, k_tick, k_r0, k_r1, k_r2, k_r3, k_act;
    DevBuf<int64_t> k_off;
    DevBuf<char> k_aid;
    DevBuf<unsigned long long> k_cnt;
    // owgs_publish_activations (owgs_publish.hip): the placed predicate, the message stage's invoker array, the output
    // block on the device and the pinned host block it is read back into with one copy
    DevBuf<uint8_t> p_placed, p_blk;
    DevBuf<int32_t> p_minv;
    Pinned<> p_pin;
    // owgs_invoke_activations (owgs_invoke.hip): the items' action handles, sequence numbers and override arrays as
    // uploaded, the maps between an item and its rank among the admitted actions, the compaction's per-block counts
    // (its output block and pinned block are p_blk / p_pin)
    DevBuf<int32_t> v_act, v_map, v_rank, v_bcnt, v_ov0, v_ov1;
    DevBuf<u64> v_seq;
    // owgs_process_result_acks: its seven output arrays as one device block, and the pinned block they come back in
    DevBuf<uint8_t> r_blk;
    Pinned<> r_pin;
    // invoker health supervision (owgs_health.hip): persistent SoA by invoker id + per-batch scratch
    DevBuf<uint8_t> h_st, he_kind, he_temp;
    DevBuf<uint32_t> h_ring;
    DevBuf<int64_t> h_last, h_tick, h_mem, he_t, he_mem, he_packed;
    DevBuf<int32_t> h_tests, he_inv, he_key, he_idx0, he_idx1, he_beg, he_end, he_reg, he_pad;
    int32_t h_cap = 0, h_size = 0;
    // the supervision feeds (owgs_feeds.hip): the FSM kernel's summary words, the pings' receive times and parsed
    // userMemory, and the largest batch whose feed buffers are reserved (feed_n) with its sort scratch (feed_tb)
    DevBuf<int32_t> he_sum;
    DevBuf<int64_t> pg_t, pg_mem;
    int32_t feed_n = 0;
    size_t feed_tb = 0;
    DevBuf<unsigned long long> r_bound;  // release front end scratch (owgs_launch_release_seq)
    DevBuf<int32_t> r_idx, r_cnt, r_cval, r_cval_s, r_cbeg;
    DevBuf<uint32_t> r_ckey, r_ckey_s;
    DevBuf<uint8_t> r_sel, r_temp;
    bool ev_engine_valid = false;
    // ActivationMessage templates + serialisation scratch (owgs_msgs.hip)
    std::vector<char> ta, tb;
    std::vector<int64_t> ta_off{0}, tb_off{0};
    std::string rci = "{\"asString\":\"0\"}";  // ControllerInstanceId("0"), jsonFormat1 (InstanceId.scala:40, 59)
    bool tmpl_dirty = true;
    DevBuf<char> m_ta, m_tb, m_rci, m_tid, m_content, m_trace, m_out;
    DevBuf<int64_t> m_ta_off, m_tb_off, m_tid_off, m_tid_start, m_content_off, m_trace_off, m_len, m_len_sorted,
        m_out_off;
    DevBuf<int32_t> m_inv, m_tmpl, m_bad, m_order, m_iota, m_cnt, m_topic;
    DevBuf<uint32_t> m_key, m_key_sorted;
    DevBuf<ulonglong2> m_aid, m_cause;
    DevBuf<uint8_t> m_flags, m_temp;
    // the throttle gate's user events (owgs_events.hip): the event source (a printed JSON string; unset until
    // owgs_set_event_source), the identities' two pieces with their offsets, their device copies, the per-call scratch
    // and byte regions, and the stand-alone call's inputs, output block and the pinned block it comes back in
    std::string ev_src;
    bool ev_src_set = false, ev_dirty = true;
    std::vector<char> ei_a, ei_b;
    std::vector<int64_t> ei_a_off{0}, ei_b_off{0};
    DevBuf<char> e_src, e_ia, e_ib, e_ev_out, e_rej_out;
    DevBuf<int64_t> e_ia_off, e_ib_off, e_ev_len, e_rej_len, e_ts;
    DevBuf<int32_t> e_ident, e_i32;
    DevBuf<uint8_t> e_kind, e_ver, e_temp, e_blk;
    Pinned<> e_pin;
    int64_t h_now = INT64_MIN;
    // watched (invoker, fqn) pairs after a slot-state reset (owgs_watch.hip; w_cap == 0: none)
    DevBuf<uint32_t> w_keys, w_vals;
    DevBuf<int32_t> w_cnt, w_wkey, w_D, w_L, w_Lcnt, w_rel;
    DevBuf<uint4> w_L2;
    DevBuf<int64_t> w_off;
    // owgs_replay_device_group: its batch offsets, the usable bitmap of each batch's health, and (during the call) the
    // first activation of the group (releases of earlier ones get their records from those decisions)
    DevBuf<int64_t> g_off;
    // large-state engine (owgs_seq.hip): a state beyond every on-chip geometry (owgs_limits) or maxConcurrent beyond
    // OWGS_MAX_CONC runs there -- permits in HBM, the NestedSemaphore maps in one HBM table q_map
    bool large = false, big_conc = false;
    // the chunked engine's capacities (owgs_divq.h) are exact while every slot is below 2^22 MB or every memory limit
    // at most OWGS_DIVQ_MEM_ANY MB: a context that has seen both (sticky) runs on the large-state engine as well
    bool wide_slots = false, wide_mem = false;
    DevBuf<uint4> q_map;
    int32_t q_cap = 0;
    DevBuf<int32_t> q_filled, q_state, q_look;
    DevBuf<uint4> q_cur;   // walk cursors of the large-state engine, per action {generation, step, position, 0}
    uint32_t q_gen = 1;    // the next call's first generation: cursors never outlive the call that wrote them
    int64_t q_spec = 0, q_alone = 0;  // its decisions: kept from the group speculation / decided alone
    int64_t q_path[OWGS_SEQ_NPATH] = {};  // ... by path (the kernel's state[16..], owgs_large_stats' [2..11])
    int64_t q_launches = 0, q_resumes = 0;  // its launches / those that stopped for the map to grow
    uint64_t q_cyc[4] = {0, 0, 0, 0};  // its cycles: releases, group speculation, kept decisions, decided alone
    DevBuf<uint32_t> d_hwords;
    const uint32_t* grp_hwords = nullptr;
    int32_t grp_hstride = 0;
    int64_t grp_a0 = 0;
    DevBuf<uint8_t> w_rfl;
    int32_t w_cap = 0, w_live = 0;
    int32_t stats_par = 0, stats_last = 0;  // d_stats holds two counter blocks: the next launch's, the last one's
    int32_t cw_cache = 0;  // chunk width of the current state and actions (0: recompute)
    bool any_conc = false;  // some registered action has maxConcurrent > 1 (the engine needs its map code)
    int32_t variant = 0;   // engine geometry: 0 wide chunks, 1 narrow (large pools, owgs_engine_narrow.hip)
    // owgs_process_batch: pinned staging (inputs, outputs) and their device copies
    Pinned<> h_pin, h_pout;
    DevBuf<uint8_t> d_pin, d_pout;
    DevBuf<int32_t> f_src, f_cnt, f_tile;
    DevBuf<uint2> f_rec;
    // owgs_process_batch through the resident engine (owgs_resident.hip, stream and event above): the pinned control
    // block and call buffers, the call counter (the doorbell), whether a launch is live, and counters for
    // owgs_resident_stats
    Pinned<int32_t> res_ctl, res_in;
    Pinned<char> res_out;
    int32_t res_call = 0;
    bool res_alive = false;
    bool res_last_served = false;  // the previous owgs_process_batch call was served by the resident engine
    int32_t res_stage = 0;
    int64_t res_n_calls = 0, res_n_launches = 0, res_n_bails = 0, res_n_chained = 0, res_n_life = 0;
    int64_t res_n_watch_calls = 0;  // served calls while watched pairs existed
    int64_t res_prof[OWGS_RES_NPROF] = {};
    int64_t res_used_max = 0, res_tombs_max = 0;  // the primary table's fill after served calls (largest seen)
    int64_t res_host_ns[2] = {};    // served calls: host time building the call (records, ranks), bell-to-answer wait
    DevBuf<uint4> d_w_sidx;         // resident engine: watched pairs by fqn@version key (built at its launch)
    DevBuf<uint2> d_w_list;
    int32_t w_scap = 0;
    uint64_t res_cache_epoch = 1, res_cache_seen = 0;  // res_meta / the watched-pair index are current when equal
    DevBuf<uint2> d_res_cur;        // per action: {cursor generation, first walk step that may fit}
    std::vector<uint2> res_meta;    // act_meta as of the live launch (every change of it stops the engine first)
    uint32_t res_gen_seen = 0;      // the last cursor generation the engine reported
    int64_t last_call_ns = 0;       // duration of the last publish / release / process_batch call, timed inside the library
    DevBuf<unsigned long long> d_spec_stats;  // stream-mode replays: summed resident-engine counters (owgs_resident_stats)
    DevBuf<uint32_t> d_claim;       // stream-mode replays: released activations (a second release is a malformed stream)
    bool spec_last = false;         // the last replay ran in stream mode
    DevBuf<unsigned long long> f_bound;  // per slot: what a fused call's releases can return (zero between calls)
    DevBuf<uint32_t> s_w_keys, s_w_vals;
    DevBuf<int32_t> s_w_wkey;
    int32_t s_w_cap = 0, s_w_live = 0;
    // snapshot
    DevBuf<int32_t> s_permits;
    DevBuf<uint32_t> s_ct_keys, s_ct_vals;
    bool has_snap = false;
    int32_t snap_slots = 0;

    int fail(int code, const char* what, hipError_t e = hipSuccess) {
        err = what;
        if (e != hipSuccess) {
            err += ": ";
            err += hipGetErrorString(e);
        }
        return code;
    }
};

#define HIPCHK(ctx, call)                                                     \
    do {                                                                      \
        hipError_t _e = (call);                                               \
        if (_e != hipSuccess) return (ctx)->fail(OWGS_EDEVICE, #call, _e);    \
    } while (0)

template <class T>
static hipError_t upload(DevBuf<T>& d, const T* h, size_t n, hipStream_t s) {
    hipError_t e = d.reserve(n);
    if (e != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    return hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, s);
}

// times one ABI call, entry to return, into c->last_call_ns (the latency the JNI shim sees, without the host
// language's call overhead)
struct CallTimer {
    owgs_ctx* c;
    std::chrono::steady_clock::time_point t0;
    explicit CallTimer(owgs_ctx* c_) : c(c_), t0(std::chrono::steady_clock::now()) {}
    ~CallTimer() {
        if (c) c->last_call_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    }
};

// ---------------------------------------------------------------- helpers called across files, by defining file
// owgs_host.cpp
int order_on(owgs_ctx* c, hipStream_t s);
OwgsOvf ovf_args(const owgs_ctx* c);
void ovf_add(owgs_ctx* c, int64_t n);
int ensure_ovf(owgs_ctx* c, int64_t n_new, hipStream_t s);
OwgsWatch watch_args(const owgs_ctx* c);
int w_refresh(owgs_ctx* c, hipStream_t s);
void base_args(owgs_ctx* c, OwgsEngineArgs& A);
int run_prepass(owgs_ctx* c, OwgsEngineArgs& A, int32_t n_batches, const int64_t* acq_off, const int32_t* act,
                int64_t n_act, hipStream_t s);
int run_engine(owgs_ctx* c, OwgsEngineArgs& A, hipStream_t s, bool launch = true);
int w_update(owgs_ctx* c, int32_t n, const int32_t* d_act, const int32_t* d_out, const uint8_t* d_fl,
             hipStream_t s);
int check_err_word(owgs_ctx* c);
bool registered(const owgs_ctx* c, int32_t n, const int32_t* action);
int res_quiesce(owgs_ctx* c);
OwgsSeqArgs seq_args(owgs_ctx* c);
int seq_run(owgs_ctx* c, const OwgsSeqArgs& S0, hipStream_t s);
int publish_device(owgs_ctx* c, int32_t n, const int32_t* action, const uint64_t* seq, uint64_t seq_base,
                   int32_t* h_out, uint8_t* h_flags);
int release_scratch(owgs_ctx* c, OwgsReleaseArgs& R, int32_t n);
// owgs_host_acks.cpp
int act_reserve(owgs_ctx* c, long long n);
int track_device(owgs_ctx* c, int32_t n, const ulonglong2* key, const int32_t* action, const int32_t* ns,
                 const int32_t* ticket, const int32_t* inv, const long long* tl, int64_t now_ms,
                 const uint8_t* placed, int32_t* out_ticket, uint8_t* out_existed,
                 unsigned long long* counters, hipStream_t st);
struct AckResultTail {  // owgs_process_result_acks: where ack_complete copies the result block
    unsigned long long* d_aid;  // [2n] in the block
    void* pin;                  // pinned destination
    const void* blk;            // the block
    size_t bytes;
};
int ack_complete(owgs_ctx* c, int32_t n, uint8_t* d_kind, int32_t* d_ticket, uint8_t* d_flags,
                 hipStream_t st, const AckResultTail* rt = nullptr);
bool ns_known(const owgs_ctx* c, int32_t n, const int32_t* ns);
OwgsAdmitArgs admit_args(const owgs_ctx* c, int32_t n);

// Every entry point but owgs_process_batch reads or replaces the state a live resident engine holds in LDS, so it
// stops the engine first (the engine writes the state back to HBM and exits); the next eligible call launches it again.
#define OWGS_ENTER(c)                             \
    do {                                          \
        (void)hipSetDevice((c)->cfg.device);      \
        const int q_ = res_quiesce(c);            \
        if (q_) return q_;                        \
    } while (0)

#define OWGS_NOT_LARGE(c)                                                                                   \
    do {                                                                                                  \
        if ((c)->large)                                                                                   \
            return (c)->fail(OWGS_ERANGE, "not available for a state beyond owgs_limits (large-state engine)"); \
    } while (0)
