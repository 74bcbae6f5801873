// owgs_host_acks.cpp -- activation table, completion acks, expiry, the in-flight books and the throttle gate.
#include "owgs_ctx.h"

// ============================================================================================== completion acks
// activationSlots (CLB:60) on the device; see owgs_acks.hip.

static OwgsActTable act_table(owgs_ctx* c) {
    OwgsActTable T;
    T.tw = c->t_tw.p;
    T.tk = c->t_tk.p;
    T.tv = c->t_tv.p;
    T.tn = c->t_tn.p;
    T.owner = c->t_owner.p;
    T.cap = c->t_cap;
    T.td = c->t_td.p;
    T.ti = c->t_ti.p;
    T.tq = c->t_tq.p;
    T.tmin = c->t_tmin.p;
    return T;
}

// keep used slots (live + deleted) under half the capacity: rehash the live entries into a table of
// max(cap, 4 * (live + n)) slots when n more inserts could cross it
int act_reserve(owgs_ctx* c, long long n) {
    if (c->t_cap > 0 && c->t_used + n <= c->t_cap / 2) return OWGS_OK;
    long long cap = 1 << 16;
    while (cap < 4 * (c->t_live + n)) cap <<= 1;
    if (cap < c->t_cap) cap = c->t_cap;
    DevBuf<unsigned long long> tw;
    DevBuf<ulonglong2> tk;
    DevBuf<int2> tv;
    DevBuf<int32_t> tn, ow, ti;
    DevBuf<long long> td, tmin;
    DevBuf<unsigned long long> tq;
    HIPCHK(c, td.reserve((size_t)cap));
    HIPCHK(c, ti.reserve((size_t)cap));
    HIPCHK(c, tq.reserve((size_t)cap));
    HIPCHK(c, tmin.reserve((size_t)(cap >> OWGS_TILE_LOG2)));
    HIPCHK(c, tw.reserve((size_t)cap));
    HIPCHK(c, tk.reserve((size_t)cap));
    HIPCHK(c, tv.reserve((size_t)cap));
    HIPCHK(c, tn.reserve((size_t)cap));
    HIPCHK(c, ow.reserve((size_t)cap));
    OwgsActTable T{tw.p, tk.p, tv.p, tn.p, ow.p, cap, td.p, ti.p, tq.p, tmin.p};
    HIPCHK(c, owgs_launch_act_init(&T, c->stream));
    if (c->t_cap > 0) {
        OwgsActTable O = act_table(c);
        HIPCHK(c, owgs_launch_act_rehash(&O, &T, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->t_td = std::move(td);
    c->t_ti = std::move(ti);
    c->t_tq = std::move(tq);
    c->t_tmin = std::move(tmin);
    c->t_tw = std::move(tw);
    c->t_tk = std::move(tk);
    c->t_tv = std::move(tv);
    c->t_tn = std::move(tn);
    c->t_owner = std::move(ow);
    c->t_cap = cap;
    c->t_used = c->t_live;
    return OWGS_OK;
}

int owgs_set_health_tid(owgs_ctx* c, int64_t start_ms) {
    if (!c) return OWGS_EINVAL;
    c->health_ms = start_ms;
    return OWGS_OK;
}

int owgs_activations_live(owgs_ctx* c, int64_t* live) {
    if (!c || !live) return OWGS_EINVAL;
    *live = c->t_live;
    return OWGS_OK;
}

static OwgsInflight inflight_args(owgs_ctx* c) {
    OwgsInflight F;
    F.active = c->d_ns_active.p;
    F.act_mem = c->d_act_mem.p;
    F.act_bb = c->d_act_bb.p;
    return F;
}

// The device half of setupActivation (CLB:116-166) over device arrays: claim / fill / publish for n ids with their
// action, namespace (null: none), ticket, entry invoker and time limit (inv null: an untimed call, nothing armed),
// shared by the track entry points and owgs_publish_activations.  placed (null: every item) is the latter's predicate:
// an item it clears touches neither the table nor a counter and keeps the out_ticket / out_existed already there.
// The caller has run act_reserve(c, n) and zeroed counters; queued on st, no wait.  The arm counter advances by n.
int track_device(owgs_ctx* c, int32_t n, const ulonglong2* key, const int32_t* action, const int32_t* ns,
                 const int32_t* ticket, const int32_t* inv, const long long* tl, int64_t now_ms,
                 const uint8_t* placed, int32_t* out_ticket, uint8_t* out_existed,
                 unsigned long long* counters, hipStream_t st) {
    HIPCHK(c, c->k_slot.reserve((size_t)n));
    HIPCHK(c, c->k_state.reserve((size_t)n));
    OwgsArm arm{};
    arm.seq_base = c->arm_seq;
    if (inv) {
        arm.inv = inv;
        arm.tl = tl;
        arm.now = now_ms;
        arm.std_ms = c->a_std;
        arm.factor = c->a_factor;
        arm.addon = c->a_addon;
    }
    OwgsActTable T = act_table(c);
    const OwgsInflight F = inflight_args(c);
    HIPCHK(c, owgs_launch_act_track(&T, key, n, action, ns, ticket, c->k_slot.p, c->k_state.p, out_ticket,
                                    out_existed, counters, &F, &arm, placed, st));
    c->arm_seq += (unsigned long long)n;  // arm order = track call order, then array index
    return OWGS_OK;
}

// ns = null: every item without a namespace (owgs_track_activations); invoker = null: nothing armed (the untimed calls)
static int track_impl(owgs_ctx* c, int32_t n, const char* aid32, const int32_t* action, const int32_t* ns,
                      const int32_t* ticket, int32_t* out_ticket, uint8_t* out_existed,
                      const int32_t* invoker = nullptr, const int64_t* time_limit_ms = nullptr, int64_t now_ms = 0) {
    if (!c || n < 0 || (n > 0 && (!aid32 || !action || !ticket || !out_ticket || !out_existed))) return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    if (invoker) {
        if (now_ms < 0 || now_ms >= (1LL << 60)) return c->fail(OWGS_EINVAL, "track: now outside [0, 2^60)");
        for (int32_t i = 0; i < n; ++i)
            if (invoker[i] < 0 || time_limit_ms[i] < 0 || time_limit_ms[i] >= (1LL << 40))
                return c->fail(OWGS_EINVAL, "track: negative invoker or time limit outside [0, 2^40)");
    }
    if (!registered(c, n, action)) return c->fail(OWGS_ENOENT, "unknown action");
    if (ns) {
        const int32_t nn = (int32_t)c->ns_map.size();
        for (int32_t i = 0; i < n; ++i)
            if (ns[i] != OWGS_NONE && (ns[i] < 0 || ns[i] >= nn)) return c->fail(OWGS_ENOENT, "unknown namespace");
    }
    // ActivationId.asString is 32 chars of [0-9a-f]; reject a malformed batch before any entry is created
    for (size_t k = 0; k < (size_t)n * 32; ++k) {
        const char ch = aid32[k];
        if (!((ch >= '0' && ch <= '9') || (ch >= 'a' && ch <= 'f')))
            return c->fail(OWGS_EINVAL, "activation id is not 32 characters of [0-9a-f]");
    }
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    int rc = act_reserve(c, n);
    if (rc) return rc;
    HIPCHK(c, upload(c->k_aid, aid32, (size_t)n * 32, c->stream));
    HIPCHK(c, upload(c->k_act, action, (size_t)n, c->stream));
    HIPCHK(c, upload(c->k_r0, ticket, (size_t)n, c->stream));
    HIPCHK(c, c->k_key.reserve((size_t)n));
    HIPCHK(c, c->k_tick.reserve((size_t)n));
    HIPCHK(c, c->k_oflags.reserve((size_t)n));
    if (ns) HIPCHK(c, upload(c->k_r1, ns, (size_t)n, c->stream));
    if (invoker) {
        HIPCHK(c, upload(c->x_inv, invoker, (size_t)n, c->stream));
        HIPCHK(c, upload(c->x_tl, (const long long*)time_limit_ms, (size_t)n, c->stream));
    }
    HIPCHK(c, c->k_cnt.reserve(OWGS_CNT_WORDS));
    HIPCHK(c, hipMemsetAsync(c->k_cnt.p, 0, OWGS_CNT_WORDS * 8, c->stream));
    HIPCHK(c, owgs_launch_aid_decode(c->k_aid.p, n, nullptr, c->k_key.p, nullptr, nullptr, nullptr, c->stream));
    rc = track_device(c, n, c->k_key.p, c->k_act.p, ns ? c->k_r1.p : nullptr, c->k_r0.p,
                      invoker ? c->x_inv.p : nullptr, invoker ? c->x_tl.p : nullptr, now_ms, nullptr, c->k_tick.p,
                      c->k_oflags.p, c->k_cnt.p, c->stream);
    if (rc) return rc;
    unsigned long long cnt[OWGS_CNT_WORDS];
    HIPCHK(c, hipMemcpyAsync(out_ticket, c->k_tick.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_existed, c->k_oflags.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt, c->k_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->t_used += (long long)cnt[OWGS_CNT_INSERTED];
    c->t_live += (long long)cnt[OWGS_CNT_INSERTED];
    // CLB:121-125 for every item of the batch, duplicates included (they run before getOrElseUpdate, CLB:148)
    c->f_total += n;
    c->f_mb_managed += (long long)cnt[OWGS_CNT_MANAGED_MB];
    c->f_mb_blackbox += (long long)cnt[OWGS_CNT_BLACKBOX_MB];
    for (int32_t i = 0; i < n; ++i)
        if (out_existed[i] == 2) return c->fail(OWGS_EINVAL, "activation id is not 32 characters of [0-9a-f]");
    return OWGS_OK;
}

int owgs_track_activations(owgs_ctx* c, int32_t n, const char* aid32, const int32_t* action, const int32_t* ticket,
                           int32_t* out_ticket, uint8_t* out_existed) {
    return track_impl(c, n, aid32, action, nullptr, ticket, out_ticket, out_existed);
}

int owgs_track_activations_ns(owgs_ctx* c, int32_t n, const char* aid32, const int32_t* action, const int32_t* ns,
                              const int32_t* ticket, int32_t* out_ticket, uint8_t* out_existed) {
    if (n > 0 && !ns) return OWGS_EINVAL;
    return track_impl(c, n, aid32, action, ns, ticket, out_ticket, out_existed);
}

int owgs_set_ack_timeout(owgs_ctx* c, int64_t std_ms, int32_t factor, int64_t addon_ms) {
    if (!c) return OWGS_EINVAL;
    if (std_ms < 0 || std_ms >= (1LL << 40) || addon_ms < 0 || addon_ms >= (1LL << 40) || factor < 1 ||
        factor >= (1 << 16))
        return c->fail(OWGS_EINVAL, "ack timeout: std / addon outside [0, 2^40) or factor outside [1, 2^16)");
    c->a_std = std_ms;
    c->a_factor = factor;
    c->a_addon = addon_ms;
    return OWGS_OK;
}

int owgs_track_activations_timed(owgs_ctx* c, int32_t n, const char* aid32, const int32_t* action, const int32_t* ns,
                                 const int32_t* ticket, const int32_t* invoker, const int64_t* time_limit_ms,
                                 int64_t now_ms, int32_t* out_ticket, uint8_t* out_existed) {
    if (n > 0 && (!invoker || !time_limit_ms)) return OWGS_EINVAL;
    return track_impl(c, n, aid32, action, ns, ticket, out_ticket, out_existed, invoker, time_limit_ms, now_ms);
}

// the completion's share of the books (CLB:280-284): one decrement per removed entry, the entries' megabytes
static void inflight_release(owgs_ctx* c, const unsigned long long* cnt) {
    c->f_total -= (long long)cnt[OWGS_CNT_REMOVED];
    c->f_mb_managed -= (long long)cnt[OWGS_CNT_MANAGED_MB];
    c->f_mb_blackbox -= (long long)cnt[OWGS_CNT_BLACKBOX_MB];
}

// owgs_process_result_acks' share of the tail: result-only records look their entry up, the flags kernel adds the result
// bits and the ids, and the output block's copy is queued before the tail's one synchronisation
// shared tail: info/key/inst of n messages are in k_info/k_key/k_inst; resolve, release in order, flags
int ack_complete(owgs_ctx* c, int32_t n, uint8_t* d_kind, int32_t* d_ticket, uint8_t* d_flags,
                 hipStream_t st, const AckResultTail* rt) {
    if (c->t_cap == 0) {
        int rc = act_reserve(c, 0);
        if (rc) return rc;
    }
    HIPCHK(c, c->k_slot.reserve((size_t)n));
    HIPCHK(c, c->k_r0.reserve((size_t)n));
    HIPCHK(c, c->k_r1.reserve((size_t)n));
    HIPCHK(c, c->k_r2.reserve((size_t)n));
    HIPCHK(c, c->k_r3.reserve((size_t)n));
    HIPCHK(c, c->d_rflags.reserve((size_t)n));
    HIPCHK(c, c->k_cnt.reserve(OWGS_CNT_WORDS));
    HIPCHK(c, hipMemsetAsync(c->k_cnt.p, 0, OWGS_CNT_WORDS * 8, st));
    if (!c->d_act_mem.p) {  // no actions registered: every lookup misses, the records are never read
        HIPCHK(c, c->d_act_mem.reserve(1));
        HIPCHK(c, c->d_act_maxc.reserve(1));
        HIPCHK(c, c->d_act_slot.reserve(1));
        HIPCHK(c, c->d_act_bb.reserve(1));
    }
    OwgsActTable T = act_table(c);
    OwgsAckCompleteArgs a{};
    a.key = c->k_key.p;
    a.info = c->k_info.p;
    a.inst = c->k_inst.p;
    a.n = n;
    a.slot = c->k_slot.p;
    a.act_mem = c->d_act_mem.p;
    a.act_maxc = c->d_act_maxc.p;
    a.act_slot = c->d_act_slot.p;
    a.n_slots = c->n_slots;
    a.r_inv = c->k_r0.p;
    a.r_mem = c->k_r1.p;
    a.r_maxc = c->k_r2.p;
    a.r_slot = c->k_r3.p;
    a.out_kind = d_kind;
    a.out_ticket = d_ticket;
    a.counters = c->k_cnt.p;
    a.fl = inflight_args(c);
    a.results = rt ? 1 : 0;
    HIPCHK(c, owgs_launch_ack_complete(&T, &a, st));
    if (c->large) {  // the large-state engine applies the records in message order (owgs_seq.hip)
        const int64_t offs[4] = {0, (int64_t)n, 0, 0};
        HIPCHK(c, upload(c->g_off, offs, 4, st));
        OwgsSeqArgs S = seq_args(c);
        S.n_runs = 1;
        S.rel_off = c->g_off.p;
        S.pub_off = c->g_off.p + 2;
        S.rel_inv = c->k_r0.p;
        S.rel_mem = c->k_r1.p;
        S.rel_maxc = c->k_r2.p;
        S.rel_slot = c->k_r3.p;
        S.rel_flags = c->d_rflags.p;
        int rs = seq_run(c, S, st);
        if (rs) return rs;
        HIPCHK(c, owgs_launch_ack_flags(n, c->k_info.p, c->d_rflags.p, d_kind, d_flags, c->k_key.p,
                                        rt ? rt->d_aid : nullptr, st));
        if (rt) HIPCHK(c, hipMemcpyAsync(rt->pin, rt->blk, rt->bytes, hipMemcpyDeviceToHost, st));
        unsigned long long cnt[OWGS_CNT_WORDS];
        HIPCHK(c, hipMemcpyAsync(cnt, c->k_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->t_live -= (long long)cnt[OWGS_CNT_REMOVED];
        inflight_release(c, cnt);
        return check_err_word(c);
    }
    OwgsReleaseArgs R{};
    R.permits = c->d_permits.p;
    R.n_slots = c->n_slots;
    R.ct_keys = c->d_ct_keys.p;
    R.ct_vals = c->d_ct_vals.p;
    R.ovf = ovf_args(c);
    R.n = n;
    R.inv = c->k_r0.p;
    R.mem = c->k_r1.p;
    R.maxc = c->k_r2.p;
    R.slot = c->k_r3.p;
    R.flags = c->d_rflags.p;
    R.err = c->d_err.p;
    int rs = release_scratch(c, R, n);
    if (!rs && c->w_cap > 0) {
        rs = ensure_ovf(c, n, st);
        ovf_add(c, n);
    }
    if (rs) return rs;
    R.ovf = ovf_args(c);
    R.w = watch_args(c);
    HIPCHK(c, owgs_launch_release_seq(&R, st));
    HIPCHK(c, owgs_launch_ack_flags(n, c->k_info.p, c->d_rflags.p, d_kind, d_flags, c->k_key.p,
                                    rt ? rt->d_aid : nullptr, st));
    if (rt) HIPCHK(c, hipMemcpyAsync(rt->pin, rt->blk, rt->bytes, hipMemcpyDeviceToHost, st));
    unsigned long long cnt[OWGS_CNT_WORDS];
    HIPCHK(c, hipMemcpyAsync(cnt, c->k_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->t_live -= (long long)cnt[OWGS_CNT_REMOVED];
    inflight_release(c, cnt);
    rs = w_refresh(c, st);
    return rs ? rs : check_err_word(c);
}

int owgs_process_acks_device(owgs_ctx* c, int32_t n, const uint8_t* bytes, const int64_t* off, uint8_t* out_kind,
                             int32_t* out_invoker, int32_t* out_ticket, uint8_t* out_flags, void* stream) {
    if (!c || n < 0 || (n > 0 && (!bytes || !off || !out_kind || !out_invoker || !out_ticket || !out_flags)))
        return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, stream ? (hipStream_t)stream : c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, c->k_key.reserve((size_t)n));
    HIPCHK(c, c->k_info.reserve((size_t)n));
    OwgsAckParseArgs p{};
    p.bytes = bytes;
    p.off = off;
    p.n = n;
    p.health_start_ms = c->health_ms;
    p.forced = nullptr;
    p.key = c->k_key.p;
    p.inst = out_invoker;
    p.info = c->k_info.p;
    HIPCHK(c, owgs_launch_ack_parse(&p, st));
    // the resolve step reads the instance from k_inst
    HIPCHK(c, c->k_inst.reserve((size_t)n));
    HIPCHK(c, hipMemcpyAsync(c->k_inst.p, out_invoker, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return ack_complete(c, n, out_kind, out_ticket, out_flags, st);
}

int owgs_process_acks(owgs_ctx* c, int32_t n, const char* bytes, const int64_t* off, uint8_t* out_kind,
                      int32_t* out_invoker, int32_t* out_ticket, uint8_t* out_flags) {
    if (!c || n < 0 || (n > 0 && (!bytes || !off || !out_kind || !out_invoker || !out_ticket || !out_flags)))
        return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i] || off[i] < 0) return c->fail(OWGS_EINVAL, "offsets");
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    const size_t nb = (size_t)(off[n] - off[0]);
    std::vector<int64_t> o((size_t)n + 1);
    for (int32_t i = 0; i <= n; ++i) o[i] = off[i] - off[0];
    HIPCHK(c, c->k_bytes.reserve(nb + 32));
    HIPCHK(c, hipMemsetAsync(c->k_bytes.p + nb, 0, 32, c->stream));
    if (nb) HIPCHK(c, hipMemcpyAsync(c->k_bytes.p, bytes + off[0], nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, upload(c->k_off, o.data(), o.size(), c->stream));
    HIPCHK(c, c->k_kind.reserve((size_t)n));
    HIPCHK(c, c->k_tick.reserve((size_t)n));
    HIPCHK(c, c->k_oflags.reserve((size_t)n));
    HIPCHK(c, c->k_act.reserve((size_t)n));
    int rc = owgs_process_acks_device(c, n, c->k_bytes.p, c->k_off.p, c->k_kind.p, c->k_act.p, c->k_tick.p,
                                      c->k_oflags.p, nullptr);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out_kind, c->k_kind.p, (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_invoker, c->k_act.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_ticket, c->k_tick.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_flags, c->k_oflags.p, (size_t)n, hipMemcpyDeviceToHost));
    return OWGS_OK;
}

int owgs_complete_activations(owgs_ctx* c, int32_t n, const char* aid32, const int32_t* invoker, const uint8_t* flags,
                              uint8_t* out_kind, int32_t* out_ticket, uint8_t* out_flags) {
    if (!c || n < 0 || (n > 0 && (!aid32 || !invoker || !flags || !out_kind || !out_ticket || !out_flags)))
        return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    HIPCHK(c, upload(c->k_aid, aid32, (size_t)n * 32, c->stream));
    HIPCHK(c, upload(c->k_cfl, flags, (size_t)n, c->stream));
    HIPCHK(c, upload(c->k_act, invoker, (size_t)n, c->stream));
    HIPCHK(c, c->k_key.reserve((size_t)n));
    HIPCHK(c, c->k_info.reserve((size_t)n));
    HIPCHK(c, c->k_inst.reserve((size_t)n));
    HIPCHK(c, c->k_kind.reserve((size_t)n));
    HIPCHK(c, c->k_tick.reserve((size_t)n));
    HIPCHK(c, c->k_oflags.reserve((size_t)n));
    HIPCHK(c, owgs_launch_aid_decode(c->k_aid.p, n, c->k_cfl.p, c->k_key.p, c->k_info.p, c->k_inst.p, c->k_act.p,
                                     c->stream));
    int rc = ack_complete(c, n, c->k_kind.p, c->k_tick.p, c->k_oflags.p, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out_kind, c->k_kind.p, (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_ticket, c->k_tick.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_flags, c->k_oflags.p, (size_t)n, hipMemcpyDeviceToHost));
    return OWGS_OK;
}

// ------------------------------------------------------------------------------------------ completion-ack timeouts
// owgs_expire.hip finds and orders the due entries; the removal, the books and releaseInvoker are ack_complete's.
int owgs_expire_activations(owgs_ctx* c, int64_t now_ms, int32_t cap, int32_t feed_health, int32_t* out_n,
                            int64_t* out_remaining, uint64_t* out_aid, int32_t* out_ticket, int32_t* out_invoker,
                            int64_t* out_deadline, uint8_t* out_flags) {
    if (!c || !out_n || !out_remaining || cap < 0 ||
        (cap > 0 && (!out_aid || !out_ticket || !out_invoker || !out_deadline || !out_flags)))
        return OWGS_EINVAL;
    if (now_ms < 0 || now_ms >= (1LL << 60)) return c->fail(OWGS_EINVAL, "expire: now outside [0, 2^60)");
    if (feed_health && now_ms < c->h_now)
        return c->fail(OWGS_EINVAL, "expire: now before the health supervision's last batch");
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = c->stream;
    if (c->t_cap == 0) {
        int rc = act_reserve(c, 0);
        if (rc) return rc;
    }
    // every buffer the sweep needs before its first kernel: the scan rewrites the summary words of the tiles it reads
    // and the emit step completes them, so nothing between the two may fail for want of memory
    const size_t live = (size_t)std::max<long long>(c->t_live, 1);
    const size_t tb = owgs_expire_sort_bytes((int32_t)live);
    HIPCHK(c, c->x_cnt.reserve(2));
    HIPCHK(c, c->x_d.reserve(live));
    HIPCHK(c, c->x_q.reserve(live));
    HIPCHK(c, c->x_slot.reserve(live));
    HIPCHK(c, c->x_idx0.reserve(live));
    HIPCHK(c, c->x_idx1.reserve(live));
    HIPCHK(c, c->x_key.reserve(live));
    HIPCHK(c, c->x_key_s.reserve(live));
    HIPCHK(c, c->x_outd.reserve(live));
    HIPCHK(c, c->x_temp.reserve(tb));
    HIPCHK(c, c->k_key.reserve(live));
    HIPCHK(c, c->k_inst.reserve(live));
    HIPCHK(c, c->k_info.reserve(live));
    HIPCHK(c, c->k_kind.reserve(live));
    HIPCHK(c, c->k_tick.reserve(live));
    HIPCHK(c, c->k_oflags.reserve(live));
    OwgsExpireArgs a{};
    a.T = act_table(c);
    a.now = now_ms;
    a.cnt = c->x_cnt.p;
    a.due_cap = (int32_t)live;
    a.due_d = c->x_d.p;
    a.due_q = c->x_q.p;
    a.due_slot = c->x_slot.p;
    HIPCHK(c, hipMemsetAsync(c->x_cnt.p, 0, 2 * sizeof(int32_t), st));
    HIPCHK(c, owgs_launch_expire_scan(&a, st));
    int32_t cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt, c->x_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->x_sweeps += 1;
    c->x_tiles += cnt[1];
    c->x_tiles_last = cnt[1];
    const int32_t due = cnt[0];
    if ((long long)due > c->t_live) return c->fail(OWGS_EDEVICE, "expire: more due entries than live ones");
    const int32_t take = std::min(due, cap);
    *out_n = take;
    *out_remaining = (int64_t)due - take;
    if (due == 0) return OWGS_OK;
    int32_t seq_bits = 1;
    while (seq_bits < 64 && (c->arm_seq >> seq_bits) != 0) ++seq_bits;
    HIPCHK(c, owgs_launch_expire_order(&a, due, take, seq_bits, c->x_temp.p, tb, c->x_idx0.p, c->x_idx1.p, c->x_key.p,
                                       c->x_key_s.p, c->k_key.p, c->k_inst.p, c->k_info.p, c->x_outd.p, st));
    if (take == 0) {
        HIPCHK(c, hipStreamSynchronize(st));
        return OWGS_OK;
    }
    // processCompletion(aid, tid, forced = true, isSystemError = false, invoker = entry.invoker) for each, in order
    int rc = ack_complete(c, take, c->k_kind.p, c->k_tick.p, c->k_oflags.p, st);
    if (rc) return rc;
    c->x_expired += take;
    HIPCHK(c, hipMemcpy(out_aid, c->k_key.p, (size_t)take * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_ticket, c->k_tick.p, (size_t)take * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_invoker, c->k_inst.p, (size_t)take * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_deadline, c->x_outd.p, (size_t)take * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_flags, c->k_oflags.p, (size_t)take, hipMemcpyDeviceToHost));
    if (!feed_health) return OWGS_OK;
    // InvocationFinishedMessage(invoker, Timeout) of each expired entry (CLB:317) in the same order; ids the status
    // vector cannot hold were never registered, and the pool ignores a message for an unregistered invoker
    std::vector<int32_t> inv;
    inv.reserve((size_t)take);
    for (int32_t i = 0; i < take; ++i)
        if (out_invoker[i] >= 0 && out_invoker[i] < OWGS_HEALTH_MAX_ID) inv.push_back(out_invoker[i]);
    if (inv.empty()) return OWGS_OK;
    const std::vector<uint8_t> kind(inv.size(), (uint8_t)OWGS_EV_TIMEOUT);
    const std::vector<int64_t> t(inv.size(), now_ms), mem(inv.size(), 0);
    return owgs_health_events(c, (int32_t)inv.size(), inv.data(), kind.data(), t.data(), mem.data(), now_ms, 0);
}

int owgs_next_deadline(owgs_ctx* c, int64_t* t_ms) {
    if (!c || !t_ms) return OWGS_EINVAL;
    *t_ms = INT64_MAX;
    if (c->t_cap == 0) return OWGS_OK;
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    HIPCHK(c, c->x_outd.reserve(1));
    const OwgsActTable T = act_table(c);
    HIPCHK(c, owgs_launch_deadline_min(&T, c->x_outd.p, c->stream));
    long long v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->x_outd.p, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *t_ms = (int64_t)v;
    return OWGS_OK;
}

int owgs_expiry_stats(owgs_ctx* c, int64_t out[5]) {
    if (!c || !out) return OWGS_EINVAL;
    out[0] = c->x_sweeps;
    out[1] = c->x_tiles;
    out[2] = c->x_tiles_last;
    out[3] = c->x_expired;
    out[4] = c->t_cap >> OWGS_TILE_LOG2;
    return OWGS_OK;
}

// ------------------------------------------------------------------------------------------ in-flight books
// activationsPerNamespace (CLB:62) on the device, the three totals (CLB:63-65) on the host; see owgs_acks.hip for the
// counting and owgs_inflight.hip for the reads and the throttle check.
int owgs_register_namespaces(owgs_ctx* c, int32_t n, const uint64_t* uuid128, int32_t* out_ns) {
    if (!c || n < 0 || (n > 0 && (!uuid128 || !out_ns))) return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    // handles of the call: a uuid already registered (before or earlier in this call) keeps its handle
    std::map<std::pair<uint64_t, uint64_t>, int32_t> fresh;
    const int64_t have = (int64_t)c->ns_map.size();
    for (int32_t i = 0; i < n; ++i) {
        const std::pair<uint64_t, uint64_t> u(uuid128[2 * (size_t)i], uuid128[2 * (size_t)i + 1]);
        if (!c->ns_map.count(u) && !fresh.count(u)) {
            const int32_t h = (int32_t)(have + (int64_t)fresh.size());
            fresh[u] = h;
        }
    }
    const int64_t need = have + (int64_t)fresh.size();
    if (need > (1 << 30)) return c->fail(OWGS_ERANGE, "more than 2^30 namespaces");
    if (need > c->ns_cap) {  // grow geometrically on the context's stream; the old counters are copied, the rest zero
        OWGS_ENTER(c);
        {
            const int ro_ = order_on(c, c->stream);
            if (ro_) return ro_;
        }
        int64_t cap = std::max<int64_t>(c->ns_cap, OWGS_NS_INITIAL_CAP);
        while (cap < need) cap *= 2;
        DevBuf<int32_t> nb, rc;
        DevBuf<long long> rm;  // the rate records grow with the counters: old records copied, new handles absent
        hipError_t e = nb.reserve((size_t)cap);
        if (e == hipSuccess) e = rm.reserve(2 * (size_t)cap);
        if (e == hipSuccess) e = rc.reserve(2 * (size_t)cap);
        if (e == hipSuccess) e = hipMemsetAsync(nb.p, 0, (size_t)cap * 4, c->stream);
        if (e == hipSuccess && c->ns_cap > 0)
            e = hipMemcpyAsync(nb.p, c->d_ns_active.p, (size_t)c->ns_cap * 4, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess)
            e = owgs_launch_rate_grow(c->d_rate_min.p, c->d_rate_cnt.p, c->ns_cap, rm.p, rc.p, (int32_t)cap, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (the old arrays are freed below)
        if (e != hipSuccess) return c->fail(OWGS_EDEVICE, "namespace counters", e);
        c->d_ns_active = std::move(nb);
        c->d_rate_min = std::move(rm);
        c->d_rate_cnt = std::move(rc);
        c->ns_cap = (int32_t)cap;
    }
    for (const auto& kv : fresh) c->ns_map[kv.first] = kv.second;
    for (int32_t i = 0; i < n; ++i)
        out_ns[i] = c->ns_map[std::make_pair(uuid128[2 * (size_t)i], uuid128[2 * (size_t)i + 1])];
    return OWGS_OK;
}

bool ns_known(const owgs_ctx* c, int32_t n, const int32_t* ns) {
    const int32_t nn = (int32_t)c->ns_map.size();
    for (int32_t i = 0; i < n; ++i)
        if (ns[i] < 0 || ns[i] >= nn) return false;
    return true;
}

int owgs_active_activations(owgs_ctx* c, int32_t n, const int32_t* ns, int32_t* out) {
    if (!c || n < 0 || (n > 0 && (!ns || !out))) return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    if (!ns_known(c, n, ns)) return c->fail(OWGS_ENOENT, "unknown namespace");
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    HIPCHK(c, upload(c->k_act, ns, (size_t)n, c->stream));
    HIPCHK(c, c->k_tick.reserve((size_t)n));
    HIPCHK(c, owgs_launch_ns_gather(c->d_ns_active.p, c->k_act.p, n, c->k_tick.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->k_tick.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OWGS_OK;
}

// (every call that moves the totals ends with a synchronisation and folds its words in there: the host values are
// ordered after all earlier calls)
int owgs_activation_totals(owgs_ctx* c, int64_t out[3]) {
    if (!c || !out) return OWGS_EINVAL;
    out[0] = c->f_total;
    out[1] = c->f_mb_managed;
    out[2] = c->f_mb_blackbox;
    return OWGS_OK;
}

int owgs_throttle_batch(owgs_ctx* c, int32_t n, const int32_t* ns, const int32_t* limit, int32_t* out_count,
                        uint8_t* out_ok) {
    if (!c || n < 0 || (n > 0 && (!ns || !limit || !out_count || !out_ok))) return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    for (int32_t i = 0; i < n; ++i)
        if (ns[i] == OWGS_NONE) return c->fail(OWGS_EINVAL, "throttle check without a namespace");
    if (!ns_known(c, n, ns)) return c->fail(OWGS_ENOENT, "unknown namespace");
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    int32_t bits = 1;
    while (((int64_t)1 << bits) < (int64_t)c->ns_map.size()) ++bits;
    const size_t tb = owgs_throttle_sort_bytes(n, bits);
    HIPCHK(c, c->q_temp.reserve(tb));
    HIPCHK(c, c->q_key.reserve((size_t)n));
    HIPCHK(c, c->q_idx0.reserve((size_t)n));
    HIPCHK(c, c->q_idx1.reserve((size_t)n));
    HIPCHK(c, upload(c->k_act, ns, (size_t)n, c->stream));
    HIPCHK(c, upload(c->k_r0, limit, (size_t)n, c->stream));
    HIPCHK(c, c->k_tick.reserve((size_t)n));
    HIPCHK(c, c->k_oflags.reserve((size_t)n));
    HIPCHK(c, owgs_launch_throttle(c->k_act.p, c->k_r0.p, n, bits, c->q_temp.p, tb, c->q_key.p, c->q_idx0.p,
                                   c->q_idx1.p, c->d_ns_active.p, c->k_tick.p, c->k_oflags.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_count, c->k_tick.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_ok, c->k_oflags.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OWGS_OK;
}

// ------------------------------------------------------------------------------------------ entitlement throttle gate
// checkUserThrottle + checkConcurrentUserThrottle (Entitlement.scala:197-202, 354-381) for a drained batch; the
// semantics are in include/owgs.h, the kernel in owgs_inflight.hip.
int owgs_set_throttle_limits(owgs_ctx* c, int32_t invokes_per_minute, int32_t fires_per_minute,
                             int32_t concurrent_invocations) {
    if (!c) return OWGS_EINVAL;
    c->lim_invoke = invokes_per_minute;
    c->lim_fire = fires_per_minute;
    c->lim_conc = concurrent_invocations;
    return OWGS_OK;
}

// The gate's arguments that come from the context: the system defaults, the cluster size, the books and the rate
// records.  The caller adds the batch's inputs (kind, t_ms, overrides) and where the five outputs go; shared by
// owgs_admit_batch and owgs_invoke_activations.
OwgsAdmitArgs admit_args(const owgs_ctx* c, int32_t n) {
    OwgsAdmitArgs A{};
    A.n = n;
    A.def_invoke = c->lim_invoke;
    A.def_fire = c->lim_fire;
    A.def_conc = c->lim_conc;
    A.cluster = c->cluster;  // loadBalancer.clusterSize (SCPB:254)
    A.active = c->d_ns_active.p;
    A.rate_min = c->d_rate_min.p;
    A.rate_cnt = c->d_rate_cnt.p;
    A.ns_cap = c->ns_cap;
    return A;
}

int owgs_admit_batch(owgs_ctx* c, int32_t n, const int32_t* ns, const uint8_t* kind, const int64_t* t_ms,
                     const int32_t* rate_override, const int32_t* conc_override, uint8_t* out_verdict,
                     int32_t* out_rate_count, int32_t* out_rate_limit, int32_t* out_conc_count,
                     int32_t* out_conc_limit) {
    if (!c || n < 0 ||
        (n > 0 && (!ns || !kind || !t_ms || !out_verdict || !out_rate_count || !out_rate_limit || !out_conc_count ||
                   !out_conc_limit)))
        return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    // argument contract: validated before any state changes
    for (int32_t i = 0; i < n; ++i) {
        if (ns[i] == OWGS_NONE) return c->fail(OWGS_EINVAL, "throttle gate without a namespace");
        if (kind[i] & ~(OWGS_ADMIT_TRIGGER | OWGS_ADMIT_RATE_OVERRIDE | OWGS_ADMIT_CONC_OVERRIDE))
            return c->fail(OWGS_EINVAL, "throttle gate: reserved kind bits");
        if (((kind[i] & OWGS_ADMIT_RATE_OVERRIDE) && !rate_override) ||
            ((kind[i] & OWGS_ADMIT_CONC_OVERRIDE) && !conc_override))
            return c->fail(OWGS_EINVAL, "throttle gate: an override bit without its array");
        if (t_ms[i] < 0 || t_ms[i] >= (1LL << 60)) return c->fail(OWGS_EINVAL, "throttle gate: time outside [0, 2^60)");
    }
    if (!ns_known(c, n, ns)) return c->fail(OWGS_ENOENT, "unknown namespace");
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    int32_t bits = 1;
    while (((int64_t)1 << bits) < (int64_t)c->ns_map.size()) ++bits;
    const size_t tb = owgs_throttle_sort_bytes(n, bits);
    const size_t N = (size_t)n;
    HIPCHK(c, c->q_temp.reserve(tb));
    HIPCHK(c, c->q_key.reserve(N));
    HIPCHK(c, c->q_idx0.reserve(N));
    HIPCHK(c, c->q_idx1.reserve(N));
    HIPCHK(c, upload(c->k_act, ns, N, c->stream));
    HIPCHK(c, upload(c->k_kind, kind, N, c->stream));
    HIPCHK(c, upload(c->k_off, t_ms, N, c->stream));
    if (rate_override) HIPCHK(c, upload(c->k_r0, rate_override, N, c->stream));
    if (conc_override) HIPCHK(c, upload(c->k_r1, conc_override, N, c->stream));
    const size_t out_bytes = 17 * N;
    HIPCHK(c, c->g_out.reserve(4 * N + (N + 3) / 4));
    if (c->g_pin.bytes < out_bytes) HIPCHK(c, c->g_pin.reserve(out_bytes * 2, hipHostMallocDefault));
    OwgsAdmitArgs A = admit_args(c, n);
    A.kind = c->k_kind.p;
    A.t_ms = c->k_off.p;
    A.rate_ov = rate_override ? c->k_r0.p : nullptr;
    A.conc_ov = conc_override ? c->k_r1.p : nullptr;
    A.out_verdict = (uint8_t*)(c->g_out.p + 4 * N);
    A.out_rate_count = c->g_out.p;
    A.out_rate_limit = c->g_out.p + N;
    A.out_conc_count = c->g_out.p + 2 * N;
    A.out_conc_limit = c->g_out.p + 3 * N;
    HIPCHK(c, owgs_launch_admit(c->k_act.p, bits, c->q_temp.p, tb, c->q_key.p, c->q_idx0.p, c->q_idx1.p, &A,
                                c->stream));
    // the five outputs come back with one copy into pinned memory (five copies into the caller's pageable arrays
    // cost the call 55-71 us more) and are handed out on the host
    HIPCHK(c, hipMemcpyAsync(c->g_pin.p, c->g_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const char* HO = (const char*)c->g_pin.p;
    memcpy(out_rate_count, HO, 4 * N);
    memcpy(out_rate_limit, HO + 4 * N, 4 * N);
    memcpy(out_conc_count, HO + 8 * N, 4 * N);
    memcpy(out_conc_limit, HO + 12 * N, 4 * N);
    memcpy(out_verdict, HO + 16 * N, N);
    return OWGS_OK;
}

int owgs_rate_state(owgs_ctx* c, int32_t n, const int32_t* ns, int32_t which, int64_t* out_last_min,
                    int32_t* out_count) {
    if (!c || n < 0 || which < 0 || which > 1 || (n > 0 && (!ns || !out_last_min || !out_count))) return OWGS_EINVAL;
    if (n == 0) return OWGS_OK;
    if (!ns_known(c, n, ns)) return c->fail(OWGS_ENOENT, "unknown namespace");
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    HIPCHK(c, upload(c->k_act, ns, (size_t)n, c->stream));
    HIPCHK(c, c->g_min.reserve((size_t)n));
    HIPCHK(c, c->k_tick.reserve((size_t)n));
    HIPCHK(c, owgs_launch_rate_gather(c->d_rate_min.p, c->d_rate_cnt.p, c->ns_cap, which, c->k_act.p, n, c->g_min.p,
                                      c->k_tick.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_last_min, c->g_min.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_count, c->k_tick.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OWGS_OK;
}
