// owgs_host_msgs.cpp -- ActivationMessage templates and serialisation, publish and gated publish end to end.
#include "owgs_ctx.h"

// ------------------------------------------------------------------------------------------ ActivationMessage output
int owgs_register_templates(owgs_ctx* c, int32_t n, const char* a_bytes, const int64_t* a_off, const char* b_bytes,
                            const int64_t* b_off, int32_t* out_first_id) {
    if (!c || n < 0 || (n > 0 && (!a_bytes || !a_off || !b_bytes || !b_off))) return OWGS_EINVAL;
    for (int32_t i = 0; i < n; ++i)
        if (a_off[i + 1] < a_off[i] || b_off[i + 1] < b_off[i] || a_off[0] < 0 || b_off[0] < 0)
            return c->fail(OWGS_EINVAL, "template offsets must be non-decreasing");
    if ((int64_t)c->ta_off.size() - 1 + n > INT32_MAX) return c->fail(OWGS_ERANGE, "too many templates");
    if (out_first_id) *out_first_id = (int32_t)c->ta_off.size() - 1;
    for (int32_t i = 0; i < n; ++i) {
        c->ta.insert(c->ta.end(), a_bytes + a_off[i], a_bytes + a_off[i + 1]);
        c->ta_off.push_back((int64_t)c->ta.size());
        c->tb.insert(c->tb.end(), b_bytes + b_off[i], b_bytes + b_off[i + 1]);
        c->tb_off.push_back((int64_t)c->tb.size());
    }
    c->tmpl_dirty = true;
    return OWGS_OK;
}

int owgs_set_root_controller(owgs_ctx* c, const char* json, int32_t len) {
    if (!c || len < 0 || (len > 0 && !json)) return OWGS_EINVAL;
    c->rci.assign(json, json + len);
    c->tmpl_dirty = true;
    return OWGS_OK;
}

static int msg_templates_upload(owgs_ctx* c, hipStream_t st) {
    if (!c->tmpl_dirty) return OWGS_OK;
    HIPCHK(c, upload(c->m_ta, c->ta.data(), c->ta.size(), st));
    HIPCHK(c, upload(c->m_tb, c->tb.data(), c->tb.size(), st));
    HIPCHK(c, upload(c->m_ta_off, c->ta_off.data(), c->ta_off.size(), st));
    HIPCHK(c, upload(c->m_tb_off, c->tb_off.data(), c->tb_off.size(), st));
    HIPCHK(c, upload(c->m_rci, c->rci.data(), c->rci.size(), st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->tmpl_dirty = false;
    return OWGS_OK;
}

// plan + write with device pointers, queued on st without a wait.  The templates are on the device already
// (msg_templates_upload, which may wait).
static int msg_queue(owgs_ctx* c, OwgsMsgArgs& A, int32_t n_topics, hipStream_t st) {
    const int32_t n = A.n;
    A.ta = c->m_ta.p;
    A.ta_off = c->m_ta_off.p;
    A.tb = c->m_tb.p;
    A.tb_off = c->m_tb_off.p;
    A.n_templates = (int32_t)c->ta_off.size() - 1;
    A.rci = c->m_rci.p;
    A.rci_len = (int32_t)c->rci.size();
    A.n_topics = n_topics;
    int32_t bits = 1;
    while (bits < 31 && ((int64_t)n_topics >> bits) != 0) ++bits;
    HIPCHK(c, c->m_key.reserve((size_t)n));
    HIPCHK(c, c->m_key_sorted.reserve((size_t)n));
    HIPCHK(c, c->m_len.reserve((size_t)n));
    HIPCHK(c, c->m_len_sorted.reserve((size_t)n + 1));
    HIPCHK(c, c->m_iota.reserve((size_t)n));
    HIPCHK(c, c->m_cnt.reserve((size_t)n_topics + 1));
    HIPCHK(c, c->m_bad.reserve(1));
    const size_t tb = owgs_msg_scratch_bytes(n, n_topics, bits);
    HIPCHK(c, c->m_temp.reserve(tb));
    A.key = c->m_key.p;
    A.len = c->m_len.p;
    A.bad = c->m_bad.p;
    HIPCHK(c, hipMemsetAsync(c->m_bad.p, 0, 4, st));
    HIPCHK(c, owgs_launch_msg_plan(&A, bits, c->m_temp.p, tb, c->m_key_sorted.p, c->m_iota.p, c->m_len_sorted.p,
                                   c->m_cnt.p, st));
    HIPCHK(c, owgs_launch_msg_write(&A, st));
    return OWGS_OK;
}

// the message stage's verdict from its bad-input word
static int msg_verdict(owgs_ctx* c, int32_t bad) {
    if (bad & 1) return c->fail(OWGS_EINVAL, "serialize: invoker >= n_topics or unknown template");
    if (bad & 2) return c->fail(OWGS_EINVAL, "serialize: transaction id is not valid UTF-8");
    if (bad & 4) return c->fail(OWGS_ERANGE, "serialize: output capacity below the batch's bytes (see *total)");
    return OWGS_OK;
}

// queue + finish: host-visible *total / *m (one wait)
static int msg_run(owgs_ctx* c, OwgsMsgArgs& A, int32_t n_topics, hipStream_t st, int64_t* total, int32_t* m) {
    int rc = msg_templates_upload(c, st);
    if (!rc) rc = msg_queue(c, A, n_topics, st);
    if (rc) return rc;
    int32_t bad = 0, mm = 0;
    int64_t tot = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, c->m_bad.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&mm, A.topic_start + n_topics, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&tot, A.out_off + A.n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (total) *total = tot;
    if (m) *m = mm;
    return msg_verdict(c, bad);
}

// fused: the batch of owgs_publish_activations, whose invoker and aid are the call's own (both must be NULL)
static bool msg_batch_ok(const owgs_msg_batch* b, int32_t n_topics, bool fused = false) {
    if (!b || b->n < 0 || n_topics < 0 || n_topics >= INT32_MAX) return false;
    if (fused && (b->invoker || b->aid)) return false;
    if (b->n == 0) return true;
    return (fused || (b->invoker && b->aid)) && b->tmpl && b->tid_off && b->tid_start && b->flags;
}

struct MsgNeeds {
    bool c = false, r = false, x = false;  // some flag asks for content / traceContext / cause
};

// the host-side checks of a batch in host buffers and of its outputs, before anything is touched
static int msg_host_check(owgs_ctx* c, const owgs_msg_batch* b, int32_t n_topics, const char* out, int64_t cap,
                          const int64_t* out_off, const int32_t* out_order, const int32_t* topic_start, bool fused,
                          MsgNeeds& need) {
    if (!c || !msg_batch_ok(b, n_topics, fused) || cap < 0 || !out_off || !topic_start || (b->n > 0 && !out_order) ||
        (cap > 0 && !out))
        return OWGS_EINVAL;
    const int32_t n = b->n;
    if (n > 0 && b->tid_off[n] > b->tid_off[0] && !b->tid)
        return c->fail(OWGS_EINVAL, "serialize: transaction id bytes missing");
    for (int32_t i = 0; i < n; ++i) {
        need.c |= (b->flags[i] & OWGS_MSG_HAS_CONTENT) != 0;
        need.x |= (b->flags[i] & OWGS_MSG_HAS_CAUSE) != 0;
        need.r |= (b->flags[i] & OWGS_MSG_HAS_TRACE) != 0;
    }
    if ((need.c && (!b->content || !b->content_off)) || (need.x && !b->cause) ||
        (need.r && (!b->trace || !b->trace_off)))
        return c->fail(OWGS_EINVAL, "serialize: a flag asks for content / cause / traceContext that is missing");
    for (int32_t i = 0; i < n; ++i)
        if (b->tid_off[i + 1] < b->tid_off[i] || (need.c && b->content_off[i + 1] < b->content_off[i]) ||
            (need.r && b->trace_off[i + 1] < b->trace_off[i]))
            return c->fail(OWGS_EINVAL, "serialize: offsets must be non-decreasing");
    return OWGS_OK;
}

// a checked host batch -> the context's device buffers, outputs reserved; A is complete but for invoker and aid
static int msg_upload(owgs_ctx* c, const owgs_msg_batch* b, const MsgNeeds& need, int32_t n_topics, int64_t cap,
                      OwgsMsgArgs& A, hipStream_t st) {
    const int32_t n = b->n;
    const int64_t tid0 = n ? b->tid_off[0] : 0, tidn = n ? b->tid_off[n] : 0;
    HIPCHK(c, upload(c->m_tmpl, b->tmpl, (size_t)n, st));
    HIPCHK(c, upload(c->m_tid, b->tid + tid0, (size_t)(tidn - tid0), st));
    std::vector<int64_t> off((size_t)n + 1);
    for (int32_t i = 0; i <= n; ++i) off[i] = n ? b->tid_off[i] - tid0 : 0;
    HIPCHK(c, upload(c->m_tid_off, off.data(), off.size(), st));
    HIPCHK(c, upload(c->m_tid_start, b->tid_start, (size_t)n, st));
    HIPCHK(c, upload(c->m_flags, b->flags, (size_t)n, st));
    std::vector<int64_t> coff((size_t)n + 1, 0), roff((size_t)n + 1, 0);
    if (need.c) {
        for (int32_t i = 0; i <= n; ++i) coff[i] = b->content_off[i] - b->content_off[0];
        HIPCHK(c, upload(c->m_content, b->content + b->content_off[0], (size_t)coff[n], st));
    }
    if (need.r) {
        for (int32_t i = 0; i <= n; ++i) roff[i] = b->trace_off[i] - b->trace_off[0];
        HIPCHK(c, upload(c->m_trace, b->trace + b->trace_off[0], (size_t)roff[n], st));
    }
    HIPCHK(c, upload(c->m_content_off, coff.data(), coff.size(), st));
    HIPCHK(c, upload(c->m_trace_off, roff.data(), roff.size(), st));
    if (need.x) HIPCHK(c, upload(c->m_cause, (const ulonglong2*)b->cause, (size_t)n, st));
    else HIPCHK(c, c->m_cause.reserve(1));
    HIPCHK(c, c->m_content.reserve(1));
    HIPCHK(c, c->m_trace.reserve(1));
    HIPCHK(c, c->m_order.reserve((size_t)n));
    HIPCHK(c, c->m_out_off.reserve((size_t)n + 1));
    HIPCHK(c, c->m_topic.reserve((size_t)n_topics + 1));
    HIPCHK(c, c->m_out.reserve((size_t)std::max<int64_t>(cap, 1)));
    A.n = n;
    A.tmpl = c->m_tmpl.p;
    A.tid = c->m_tid.p;
    A.tid_off = c->m_tid_off.p;
    A.tid_start = c->m_tid_start.p;
    A.flags = c->m_flags.p;
    A.content = c->m_content.p;
    A.content_off = c->m_content_off.p;
    A.cause = c->m_cause.p;
    A.trace = c->m_trace.p;
    A.trace_off = c->m_trace_off.p;
    A.order = c->m_order.p;
    A.out_off = c->m_out_off.p;
    A.topic_start = c->m_topic.p;
    A.out = c->m_out.p;
    A.cap = cap;
    return OWGS_OK;
}

// the serialised batch (tot bytes, mm messages) from the context's device buffers into the caller's; waits
static int msg_download(owgs_ctx* c, int32_t n_topics, int64_t tot, int32_t mm, char* out, int64_t* out_off,
                        int32_t* out_order, int32_t* topic_start, hipStream_t st) {
    if (tot) HIPCHK(c, hipMemcpyAsync(out, c->m_out.p, (size_t)tot, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out_off, c->m_out_off.p, (size_t)(mm + 1) * 8, hipMemcpyDeviceToHost, st));
    if (mm) HIPCHK(c, hipMemcpyAsync(out_order, c->m_order.p, (size_t)mm * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(topic_start, c->m_topic.p, (size_t)(n_topics + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return OWGS_OK;
}

int owgs_serialize_activations(owgs_ctx* c, const owgs_msg_batch* b, int32_t n_topics, char* out, int64_t cap,
                               int64_t* out_off, int32_t* out_order, int32_t* topic_start, int64_t* total,
                               int32_t* m) {
    MsgNeeds need;
    int rc = msg_host_check(c, b, n_topics, out, cap, out_off, out_order, topic_start, false, need);
    if (rc) return rc;
    const int32_t n = b->n;
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = c->stream;
    HIPCHK(c, upload(c->m_inv, b->invoker, (size_t)n, st));
    HIPCHK(c, upload(c->m_aid, (const ulonglong2*)b->aid, (size_t)n, st));
    OwgsMsgArgs A{};
    rc = msg_upload(c, b, need, n_topics, cap, A, st);
    if (rc) return rc;
    A.invoker = c->m_inv.p;
    A.aid = c->m_aid.p;
    int64_t tot = 0;
    int32_t mm = 0;
    rc = msg_run(c, A, n_topics, st, &tot, &mm);
    if (total) *total = tot;
    if (m) *m = mm;
    if (rc) return rc;
    return msg_download(c, n_topics, tot, mm, out, out_off, out_order, topic_start, st);
}

int owgs_serialize_activations_device(owgs_ctx* c, const owgs_msg_batch* b, int32_t n_topics, char* out,
                                      int64_t cap, int64_t* out_off, int32_t* out_order, int32_t* topic_start,
                                      int64_t* total, int32_t* m, void* stream) {
    if (!c || !msg_batch_ok(b, n_topics) || cap < 0 || !out_off || !topic_start || (b->n > 0 && !out_order) ||
        (cap > 0 && !out) || (b->n > 0 && (!b->content_off || !b->trace_off)))
        return OWGS_EINVAL;
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, stream ? (hipStream_t)stream : c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, c->m_content.reserve(1));
    HIPCHK(c, c->m_trace.reserve(1));
    HIPCHK(c, c->m_cause.reserve(1));
    OwgsMsgArgs A{};
    A.n = b->n;
    A.invoker = b->invoker;
    A.tmpl = b->tmpl;
    A.aid = (const ulonglong2*)b->aid;
    A.tid = b->tid;
    A.tid_off = b->tid_off;
    A.tid_start = b->tid_start;
    A.flags = b->flags;
    A.content = b->content ? b->content : c->m_content.p;
    A.content_off = b->content_off;
    A.cause = b->cause ? (const ulonglong2*)b->cause : c->m_cause.p;
    A.trace = b->trace ? b->trace : c->m_trace.p;
    A.trace_off = b->trace_off;
    A.order = out_order;
    A.out_off = out_off;
    A.topic_start = topic_start;
    A.out = out;
    A.cap = cap;
    return msg_run(c, A, n_topics, st, total, m);
}

// ------------------------------------------------------------------------------------------ publish end to end
// Where the four publish arrays of an output block lie in pinned memory (the header is at c->p_pin).
struct PublishBlock {
    const char *inv, *ticket, *flags, *existed;
};

// What owgs_publish_activations and owgs_invoke_activations do once their output block has arrived in c->p_pin: the
// engine's error word as the gate kernel saw it, the four publish outputs handed out, the host's share of the books
// (the table's fill, CLB:121-125 for every placed item), out_summary[0..6], the table-full scan and, with msgs, the
// message stage's verdict and the download of its bytes.  who names the entry point in the error texts.
static int publish_tail(owgs_ctx* c, const char* who, int32_t n, const PublishBlock& B, int32_t* out_invoker,
                        uint8_t* out_flags, int32_t* out_ticket, uint8_t* out_existed, const owgs_msg_batch* msgs,
                        owgs_msg_out* mo, int64_t* out_summary, hipStream_t st) {
    const unsigned long long* H = (const unsigned long long*)c->p_pin.p;
    if (H[OWGS_PUB_ERR]) {  // the engine failed: the gate placed nothing, the table and the books are untouched
        const int rc = check_err_word(c);
        return rc ? rc : c->fail(OWGS_EDEVICE, (std::string(who) + ": the engine's error word was set").c_str());
    }
    memcpy(out_invoker, B.inv, (size_t)n * 4);
    memcpy(out_ticket, B.ticket, (size_t)n * 4);
    memcpy(out_flags, B.flags, (size_t)n);
    memcpy(out_existed, B.existed, (size_t)n);
    const long long placed = (long long)H[OWGS_PUB_PLACED], inserted = (long long)H[OWGS_PUB_CNT + OWGS_CNT_INSERTED];
    c->t_used += inserted;
    c->t_live += inserted;
    // CLB:121-125 for every placed item, duplicates included; an item without an invoker never reaches them
    c->f_total += placed;
    c->f_mb_managed += (long long)H[OWGS_PUB_CNT + OWGS_CNT_MANAGED_MB];
    c->f_mb_blackbox += (long long)H[OWGS_PUB_CNT + OWGS_CNT_BLACKBOX_MB];
    out_summary[0] = placed;
    out_summary[1] = inserted;
    out_summary[2] = (int64_t)H[OWGS_PUB_OVL_MANAGED];
    out_summary[3] = (int64_t)H[OWGS_PUB_OVL_BLACKBOX];
    out_summary[4] = (int64_t)H[OWGS_PUB_NONE];
    out_summary[5] = (int64_t)H[OWGS_PUB_THROW];
    out_summary[6] = 2;
    for (int32_t i = 0; i < n; ++i)
        if (out_existed[i] == 2) return c->fail(OWGS_EDEVICE, (std::string(who) + ": activation table full").c_str());
    if (!msgs) return OWGS_OK;
    const int32_t mm = (int32_t)H[OWGS_PUB_MSG_M];
    const int64_t tot = (int64_t)H[OWGS_PUB_MSG_TOTAL];
    mo->total = tot;
    mo->m = mm;
    int rc = msg_verdict(c, (int32_t)H[OWGS_PUB_MSG_BAD]);
    if (!rc) rc = msg_download(c, mo->n_topics, tot, mm, mo->out, mo->out_off, mo->out_order, mo->topic_start, st);
    if (rc) return rc;  // the entries stay, left to their timeouts (SCPB:302-303): serialise again with out_invoker
    out_summary[6] = 3;
    return OWGS_OK;
}

// ShardingContainerPoolBalancer.publish (SCPB:257-317) for a drained batch: schedule, setupActivation for the placed
// items, the serialised messages -- the decisions never leave the device between the stages.  On an
// on-chip context nothing below waits between queueing the engine and the one block copy; the gate kernel reads the
// error word on the device, so an engine error leaves the later stages with nothing to do.
int owgs_publish_activations(owgs_ctx* c, const owgs_publish_io* io, const owgs_msg_batch* msgs, owgs_msg_out* mo,
                             int64_t out_summary[8]) {
    if (!c || !io || !out_summary) return OWGS_EINVAL;
    const int32_t n = io->n;
    if (n < 0 || (msgs == nullptr) != (mo == nullptr)) return OWGS_EINVAL;
    if (n > 0 && (!io->action || !io->aid || !io->ticket || !io->time_limit_ms || !io->out_invoker ||
                  !io->out_flags || !io->out_ticket || !io->out_existed))
        return OWGS_EINVAL;
    MsgNeeds need;
    if (msgs) {
        if (msgs->n != n) return c->fail(OWGS_EINVAL, "publish: msgs->n differs from io->n");
        const int rm = msg_host_check(c, msgs, mo->n_topics, mo->out, mo->cap, mo->out_off, mo->out_order,
                                      mo->topic_start, true, need);
        if (rm) return rm;
    }
    if (io->now_ms < 0 || io->now_ms >= (1LL << 60)) return c->fail(OWGS_EINVAL, "publish: now outside [0, 2^60)");
    for (int32_t i = 0; i < n; ++i)
        if (io->time_limit_ms[i] < 0 || io->time_limit_ms[i] >= (1LL << 40))
            return c->fail(OWGS_EINVAL, "publish: time limit outside [0, 2^40)");
    if (!registered(c, n, io->action)) return c->fail(OWGS_ENOENT, "unknown action");
    if (io->ns) {
        const int32_t nn = (int32_t)c->ns_map.size();
        for (int32_t i = 0; i < n; ++i)
            if (io->ns[i] != OWGS_NONE && (io->ns[i] < 0 || io->ns[i] >= nn))
                return c->fail(OWGS_ENOENT, "unknown namespace");
    }
    for (int k = 0; k < 8; ++k) out_summary[k] = 0;
    if (n == 0) {
        if (mo) {
            mo->total = 0;
            mo->m = 0;
            mo->out_off[0] = 0;
            for (int32_t k = 0; k <= mo->n_topics; ++k) mo->topic_start[k] = 0;
            out_summary[6] = 3;
        } else {
            out_summary[6] = 2;
        }
        return OWGS_OK;
    }
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = c->stream;
    // everything that may wait comes first: the table's rehash, the templates, the buffers
    int rc = act_reserve(c, n);
    if (!rc && msgs) rc = msg_templates_upload(c, st);
    if (rc) return rc;
    const size_t hdr_bytes = (size_t)OWGS_PUB_HDR * 8, blk_bytes = hdr_bytes + (size_t)n * 10;
    if (c->p_pin.bytes < blk_bytes) HIPCHK(c, c->p_pin.reserve(blk_bytes * 2, hipHostMallocDefault));
    HIPCHK(c, c->p_blk.reserve(blk_bytes));
    HIPCHK(c, c->p_placed.reserve((size_t)n));
    if (msgs) HIPCHK(c, c->p_minv.reserve((size_t)n));
    // stage 1: the decisions, left in d_out / d_flags (the action handles in d_a)
    rc = publish_device(c, n, io->action, io->seq, io->seq_base, nullptr, nullptr);
    if (rc) return rc;  // (only the large-state engine reports its own error here: nothing is tracked or written)
    // the inputs of stages 2 and 3 go up while the engine runs
    HIPCHK(c, upload(c->k_key, (const ulonglong2*)io->aid, (size_t)n, st));
    HIPCHK(c, upload(c->k_r0, io->ticket, (size_t)n, st));
    if (io->ns) HIPCHK(c, upload(c->k_r1, io->ns, (size_t)n, st));
    HIPCHK(c, upload(c->x_tl, (const long long*)io->time_limit_ms, (size_t)n, st));
    OwgsMsgArgs A{};
    if (msgs) {
        rc = msg_upload(c, msgs, need, mo->n_topics, mo->cap, A, st);
        if (rc) return rc;
    }
    unsigned long long* hdr = (unsigned long long*)c->p_blk.p;
    int32_t* b_inv = (int32_t*)(c->p_blk.p + hdr_bytes);
    int32_t* b_tick = b_inv + n;
    uint8_t* b_flags = (uint8_t*)(b_tick + n);
    uint8_t* b_ex = b_flags + n;
    HIPCHK(c, hipMemsetAsync(hdr, 0, hdr_bytes, st));
    OwgsPublishGate G{};
    G.n = n;
    G.err = c->d_err.p;
    G.dec = c->d_out.p;
    G.dflags = c->d_flags.p;
    G.action = c->d_a.p;
    G.act_bb = c->d_act_bb.p;
    G.placed = c->p_placed.p;
    G.msg_inv = msgs ? c->p_minv.p : nullptr;
    G.hdr = hdr;
    G.out_inv = b_inv;
    G.out_ticket = b_tick;
    G.out_flags = b_flags;
    G.out_existed = b_ex;
    HIPCHK(c, owgs_launch_publish_gate(&G, st));
    // stage 2: setupActivation of the placed items, the entry's invoker read from the decisions
    rc = track_device(c, n, c->k_key.p, c->d_a.p, io->ns ? c->k_r1.p : nullptr, c->k_r0.p, c->d_out.p, c->x_tl.p,
                      io->now_ms, c->p_placed.p, b_tick, b_ex, hdr + OWGS_PUB_CNT, st);
    if (rc) return rc;
    // stage 3: the messages of the placed items
    if (msgs) {
        A.invoker = c->p_minv.p;
        A.aid = c->k_key.p;
        rc = msg_queue(c, A, mo->n_topics, st);
        if (rc) return rc;
        HIPCHK(c, owgs_launch_publish_collect(hdr, c->m_bad.p, A.topic_start, mo->n_topics, A.out_off, n, st));
    }
    HIPCHK(c, hipMemcpyAsync(c->p_pin.p, c->p_blk.p, blk_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const char* P = (const char*)c->p_pin.p + hdr_bytes;
    const PublishBlock B{P, P + (size_t)n * 4, P + (size_t)n * 8, P + (size_t)n * 9};
    return publish_tail(c, "publish", n, B, io->out_invoker, io->out_flags, io->out_ticket, io->out_existed, msgs, mo,
                        out_summary, st);
}

// ------------------------------------------------------------------------------------------ throttle gate events
int owgs_set_event_source(owgs_ctx* c, const char* json, int32_t len) {
    if (!c || len < 0 || (len > 0 && !json)) return OWGS_EINVAL;
    c->ev_src.assign(json ? json : "", (size_t)len);
    c->ev_src_set = true;
    c->ev_dirty = true;
    return OWGS_OK;
}

int owgs_register_event_identities(owgs_ctx* c, int32_t n, const char* a_bytes, const int64_t* a_off,
                                   const char* b_bytes, const int64_t* b_off, int32_t* out_first_id) {
    if (!c || n < 0 || (n > 0 && (!a_off || !b_off))) return OWGS_EINVAL;
    if (n > 0 && (a_off[0] != 0 || b_off[0] != 0))
        return c->fail(OWGS_EINVAL, "event identities: offsets must start at 0");
    for (int32_t i = 0; i < n; ++i)
        if (a_off[i + 1] < a_off[i] || b_off[i + 1] < b_off[i])
            return c->fail(OWGS_EINVAL, "event identities: offsets must be non-decreasing");
    if (n > 0 && ((a_off[n] > 0 && !a_bytes) || (b_off[n] > 0 && !b_bytes)))
        return c->fail(OWGS_EINVAL, "event identities: piece bytes missing");
    if ((int64_t)c->ei_a_off.size() - 1 + n > INT32_MAX) return c->fail(OWGS_ERANGE, "too many event identities");
    if (out_first_id) *out_first_id = (int32_t)c->ei_a_off.size() - 1;
    for (int32_t i = 0; i < n; ++i) {
        c->ei_a.insert(c->ei_a.end(), a_bytes + a_off[i], a_bytes + a_off[i + 1]);
        c->ei_a_off.push_back((int64_t)c->ei_a.size());
        c->ei_b.insert(c->ei_b.end(), b_bytes + b_off[i], b_bytes + b_off[i + 1]);
        c->ei_b_off.push_back((int64_t)c->ei_b.size());
    }
    if (n > 0) c->ev_dirty = true;
    return OWGS_OK;
}

// the checks of an owgs_event_io that need no context (before the context is looked at) ...
static bool ev_io_ok(int32_t n, const owgs_event_io* ev) {
    if (ev->ev_cap < 0 || ev->rej_cap < 0 || (ev->ev_cap > 0 && !ev->ev_out) || (ev->rej_cap > 0 && !ev->rej_out))
        return false;
    return n <= 0 || (ev->ident && ev->ev_off && ev->rej_off);
}

// ... and those that do: the source is set, every item's identity is registered
static int ev_state_check(owgs_ctx* c, int32_t n, const owgs_event_io* ev) {
    if (!c->ev_src_set) return c->fail(OWGS_EINVAL, "events: the event source is not set (owgs_set_event_source)");
    const int32_t ni = (int32_t)c->ei_a_off.size() - 1;
    for (int32_t i = 0; i < n; ++i)
        if (ev->ident[i] < 0 || ev->ident[i] >= ni) return c->fail(OWGS_ENOENT, "events: unknown event identity");
    return OWGS_OK;
}

static void ev_empty(owgs_event_io* ev) {
    ev->ev_total = ev->rej_total = 0;
    ev->n_events = ev->n_rejects = 0;
    if (ev->ev_off) ev->ev_off[0] = 0;
    if (ev->rej_off) ev->rej_off[0] = 0;
}

// bytes of the event section of an output block: ev_off and rej_off [n + 1], then the four count words
static size_t ev_section_bytes(int32_t n) { return ((size_t)n + 1) * 16 + 16; }

// Everything of the event stage that may wait or allocate: the source and identities on the device, the scratch, the
// byte regions, the items' identities.  sec = the event section of the call's device block; A comes back complete but
// for the gate's arrays and the timestamps.
static int ev_prepare(owgs_ctx* c, int32_t n, const owgs_event_io* ev, uint8_t* sec, OwgsEventArgs& A, size_t& tb,
                      hipStream_t st) {
    if (c->ev_dirty) {
        HIPCHK(c, upload(c->e_src, c->ev_src.data(), c->ev_src.size(), st));
        HIPCHK(c, upload(c->e_ia, c->ei_a.data(), c->ei_a.size(), st));
        HIPCHK(c, upload(c->e_ib, c->ei_b.data(), c->ei_b.size(), st));
        HIPCHK(c, upload(c->e_ia_off, c->ei_a_off.data(), c->ei_a_off.size(), st));
        HIPCHK(c, upload(c->e_ib_off, c->ei_b_off.data(), c->ei_b_off.size(), st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->ev_dirty = false;
    }
    tb = owgs_event_scratch_bytes(n);
    HIPCHK(c, c->e_temp.reserve(tb));
    HIPCHK(c, c->e_ev_len.reserve((size_t)n + 1));
    HIPCHK(c, c->e_rej_len.reserve((size_t)n + 1));
    HIPCHK(c, c->e_ev_out.reserve((size_t)std::max<int64_t>(ev->ev_cap, 1)));
    HIPCHK(c, c->e_rej_out.reserve((size_t)std::max<int64_t>(ev->rej_cap, 1)));
    HIPCHK(c, upload(c->e_ident, ev->ident, (size_t)n, st));
    A.n = n;
    A.ident = c->e_ident.p;
    A.src = c->e_src.p;
    A.src_len = (int32_t)c->ev_src.size();
    A.ia = c->e_ia.p;
    A.ia_off = c->e_ia_off.p;
    A.ib = c->e_ib.p;
    A.ib_off = c->e_ib_off.p;
    A.ev_len = c->e_ev_len.p;
    A.rej_len = c->e_rej_len.p;
    A.ev_off = (int64_t*)sec;
    A.rej_off = A.ev_off + n + 1;
    A.cnt = (int32_t*)(A.rej_off + n + 1);
    A.ev_out = c->e_ev_out.p;
    A.ev_cap = ev->ev_cap;
    A.rej_out = c->e_rej_out.p;
    A.rej_cap = ev->rej_cap;
    return OWGS_OK;
}

// the three steps, queued on st without a wait
static int ev_queue(owgs_ctx* c, const OwgsEventArgs& A, size_t tb, hipStream_t st) {
    HIPCHK(c, hipMemsetAsync(A.cnt, 0, 16, st));
    HIPCHK(c, owgs_launch_events(&A, c->e_temp.p, tb, st));
    return OWGS_OK;
}

// Once the block is in pinned memory (sec = its event section): the offsets, totals and counts handed out, the bytes of
// every region that fitted queued for download (the caller waits).  stage = 1 done / 2 refused for capacity; written[2]
// = the events / texts written.  Returns OWGS_ERANGE for a refused region.
static int ev_collect(owgs_ctx* c, int32_t n, owgs_event_io* ev, const uint8_t* sec, int64_t* stage, int64_t* written,
                      hipStream_t st) {
    const size_t ob = ((size_t)n + 1) * 8;
    memcpy(ev->ev_off, sec, ob);
    memcpy(ev->rej_off, sec + ob, ob);
    int32_t cnt[4];
    memcpy(cnt, sec + 2 * ob, 16);
    ev->ev_total = ev->ev_off[n];
    ev->rej_total = ev->rej_off[n];
    ev->n_events = cnt[0];
    ev->n_rejects = cnt[1];
    const bool ev_fits = ev->ev_total <= ev->ev_cap, rej_fits = ev->rej_total <= ev->rej_cap;
    if (ev_fits && ev->ev_total)
        HIPCHK(c, hipMemcpyAsync(ev->ev_out, c->e_ev_out.p, (size_t)ev->ev_total, hipMemcpyDeviceToHost, st));
    if (rej_fits && ev->rej_total)
        HIPCHK(c, hipMemcpyAsync(ev->rej_out, c->e_rej_out.p, (size_t)ev->rej_total, hipMemcpyDeviceToHost, st));
    written[0] = ev_fits ? cnt[0] : 0;
    written[1] = rej_fits ? cnt[1] : 0;
    *stage = ev_fits && rej_fits ? 1 : 2;
    if (ev_fits && rej_fits) return OWGS_OK;
    return c->fail(OWGS_ERANGE, "events: a region's capacity is below the batch's bytes (see ev_total / rej_total)");
}

// checkThrottleOverload's event and error text (Entitlement.scala:383-420) for n items from the gate's outputs in host
// arrays: the pure function of include/owgs.h, no state change.
int owgs_throttle_events(owgs_ctx* c, int32_t n, const uint8_t* kind, const uint8_t* verdict,
                         const int32_t* rate_count, const int32_t* rate_limit, const int32_t* conc_count,
                         const int32_t* conc_limit, const int64_t* ts_ms, owgs_event_io* ev) {
    if (!c || !ev || n < 0 || !ev_io_ok(n, ev)) return OWGS_EINVAL;
    if (n > 0 && (!kind || !verdict || !rate_count || !rate_limit || !conc_count || !conc_limit || !ts_ms))
        return OWGS_EINVAL;
    for (int32_t i = 0; i < n; ++i) {
        if (verdict[i] > OWGS_ADMIT_CONCURRENT) return c->fail(OWGS_EINVAL, "events: verdict outside 0..2");
        if (kind[i] & ~(OWGS_ADMIT_TRIGGER | OWGS_ADMIT_RATE_OVERRIDE | OWGS_ADMIT_CONC_OVERRIDE))
            return c->fail(OWGS_EINVAL, "events: reserved kind bits");
    }
    int rc = ev_state_check(c, n, ev);
    if (rc) return rc;
    if (n == 0) {
        ev_empty(ev);
        return OWGS_OK;
    }
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = c->stream;
    const size_t N = (size_t)n, sec_bytes = ev_section_bytes(n);
    if (c->e_pin.bytes < sec_bytes) HIPCHK(c, c->e_pin.reserve(sec_bytes * 2, hipHostMallocDefault));
    HIPCHK(c, c->e_blk.reserve(sec_bytes));
    OwgsEventArgs A{};
    size_t tb = 0;
    rc = ev_prepare(c, n, ev, c->e_blk.p, A, tb, st);
    if (rc) return rc;
    HIPCHK(c, upload(c->e_kind, kind, N, st));
    HIPCHK(c, upload(c->e_ver, verdict, N, st));
    HIPCHK(c, c->e_i32.reserve(4 * N));
    const int32_t* src32[4] = {rate_count, rate_limit, conc_count, conc_limit};
    for (int k = 0; k < 4; ++k)
        HIPCHK(c, hipMemcpyAsync(c->e_i32.p + k * N, src32[k], N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, upload(c->e_ts, ts_ms, N, st));
    A.kind = c->e_kind.p;
    A.verdict = c->e_ver.p;
    A.rate_count = c->e_i32.p;
    A.rate_limit = c->e_i32.p + N;
    A.conc_count = c->e_i32.p + 2 * N;
    A.conc_limit = c->e_i32.p + 3 * N;
    A.ts = c->e_ts.p;
    rc = ev_queue(c, A, tb, st);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->e_pin.p, c->e_blk.p, sec_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    int64_t stage = 0, written[2];
    rc = ev_collect(c, n, ev, (const uint8_t*)c->e_pin.p, &stage, written, st);
    HIPCHK(c, hipStreamSynchronize(st));
    return rc;
}

// ------------------------------------------------------------------------------------------ gated publish
// The engine step of owgs_invoke_activations on an on-chip context: publish_device without its uploads.  The admitted
// actions are in d_a (and d_seq) and their count m only on the device, as the batch offsets {0, m} in d_off; n bounds
// it.  Checked against m on the device: the pre-pass and the engine take every bound from d_off, the
// host count sizes buffers (d_rec, d_lix, the pre-pass grid, the overflow's upper bound) and clamps the I/O wave's
// record prefetch; the watch update runs over n items, of which those from m on are padding it returns on.
static int invoke_engine(owgs_ctx* c, int32_t n, bool has_seq, uint64_t seq_base) {
    OwgsEngineArgs A;
    base_args(c, A);
    A.seq_base = seq_base;
    A.seq = has_seq ? c->d_seq.p : nullptr;
    A.out_inv = c->d_out.p;
    A.out_flags = c->d_flags.p;
    int rc = run_prepass(c, A, 1, c->d_off.p, c->d_a.p, n, c->stream);
    if (!rc) rc = run_engine(c, A, c->stream);
    if (!rc) rc = w_update(c, n, c->d_a.p, c->d_out.p, c->d_flags.p, c->stream);
    return rc;
}

// EntitlementProvider.checkThrottles (Entitlement.scala:197-202, 354-381) and, for what it admits,
// ShardingContainerPoolBalancer.publish (SCPB:257-317) for a drained batch (the semantics are in
// include/owgs.h).  On an on-chip context nothing below waits between queueing the gate and the one block copy.
// ev: the event stage of owgs_invoke_activations_events, or NULL.
static int invoke_run(owgs_ctx* c, const owgs_invoke_io* io, const owgs_msg_batch* msgs, owgs_msg_out* mo,
                      owgs_event_io* ev, int64_t out_summary[16]) {
    if (!c || !io || !out_summary) return OWGS_EINVAL;
    const int32_t n = io->n;
    if (n < 0 || (msgs == nullptr) != (mo == nullptr)) return OWGS_EINVAL;
    if (ev && !ev_io_ok(n, ev)) return OWGS_EINVAL;
    if (n > 0 && (!io->ns || !io->kind || !io->t_ms || !io->action || !io->aid || !io->ticket || !io->time_limit_ms ||
                  !io->out_verdict || !io->out_rate_count || !io->out_rate_limit || !io->out_conc_count ||
                  !io->out_conc_limit || !io->out_invoker || !io->out_flags || !io->out_ticket || !io->out_existed))
        return OWGS_EINVAL;
    // the gate's argument contract (owgs_admit_batch)
    for (int32_t i = 0; i < n; ++i) {
        const uint8_t kd = io->kind[i];
        if (io->ns[i] == OWGS_NONE) return c->fail(OWGS_EINVAL, "throttle gate without a namespace");
        if (kd & ~(OWGS_ADMIT_TRIGGER | OWGS_ADMIT_RATE_OVERRIDE | OWGS_ADMIT_CONC_OVERRIDE))
            return c->fail(OWGS_EINVAL, "throttle gate: reserved kind bits");
        if (((kd & OWGS_ADMIT_RATE_OVERRIDE) && !io->rate_override) ||
            ((kd & OWGS_ADMIT_CONC_OVERRIDE) && !io->conc_override))
            return c->fail(OWGS_EINVAL, "throttle gate: an override bit without its array");
        if (io->t_ms[i] < 0 || io->t_ms[i] >= (1LL << 60))
            return c->fail(OWGS_EINVAL, "throttle gate: time outside [0, 2^60)");
    }
    // ... and publish's (owgs_publish_activations), over the items that are actions
    MsgNeeds need;
    if (msgs) {
        if (msgs->n != n) return c->fail(OWGS_EINVAL, "invoke: msgs->n differs from io->n");
        const int rm = msg_host_check(c, msgs, mo->n_topics, mo->out, mo->cap, mo->out_off, mo->out_order,
                                      mo->topic_start, true, need);
        if (rm) return rm;
    }
    if (io->now_ms < 0 || io->now_ms >= (1LL << 60)) return c->fail(OWGS_EINVAL, "invoke: now outside [0, 2^60)");
    for (int32_t i = 0; i < n; ++i)
        if (!(io->kind[i] & OWGS_ADMIT_TRIGGER) && (io->time_limit_ms[i] < 0 || io->time_limit_ms[i] >= (1LL << 40)))
            return c->fail(OWGS_EINVAL, "invoke: time limit outside [0, 2^40)");
    for (int32_t i = 0; i < n; ++i)
        if (!(io->kind[i] & OWGS_ADMIT_TRIGGER) && !registered(c, 1, io->action + i))
            return c->fail(OWGS_ENOENT, "unknown action");
    if (!ns_known(c, n, io->ns)) return c->fail(OWGS_ENOENT, "unknown namespace");
    if (ev) {
        const int re = ev_state_check(c, n, ev);
        if (re) return re;
    }
    for (int k = 0; k < 16; ++k) out_summary[k] = 0;
    if (n == 0) {
        if (ev) {
            ev_empty(ev);
            out_summary[15] = 1;
        }
        if (mo) {
            mo->total = 0;
            mo->m = 0;
            mo->out_off[0] = 0;
            for (int32_t k = 0; k <= mo->n_topics; ++k) mo->topic_start[k] = 0;
            out_summary[6] = 3;
        } else {
            out_summary[6] = 2;
        }
        return OWGS_OK;
    }
    OWGS_ENTER(c);
    {
        const int ro_ = order_on(c, c->stream);
        if (ro_) return ro_;
    }
    hipStream_t st = c->stream;
    const size_t N = (size_t)n;
    // everything that may wait comes first: the table's rehash, the templates, the buffers
    int rc = act_reserve(c, n);
    if (!rc && msgs) rc = msg_templates_upload(c, st);
    if (rc) return rc;
    // with events the block carries their section behind the nine arrays: the same one copy brings both back
    const size_t hdr_bytes = (size_t)OWGS_PUB_HDR * 8, ev_at = (hdr_bytes + N * 27 + 7) & ~(size_t)7,
                 blk_bytes = ev ? ev_at + ev_section_bytes(n) : hdr_bytes + N * 27;
    if (c->p_pin.bytes < blk_bytes) HIPCHK(c, c->p_pin.reserve(blk_bytes * 2, hipHostMallocDefault));
    HIPCHK(c, c->p_blk.reserve(blk_bytes));
    OwgsEventArgs E{};
    size_t ev_tb = 0;
    if (ev) {
        rc = ev_prepare(c, n, ev, c->p_blk.p + ev_at, E, ev_tb, st);
        if (rc) return rc;
    }
    HIPCHK(c, c->p_placed.reserve(N));
    if (msgs) HIPCHK(c, c->p_minv.reserve(N));
    int32_t bits = 1;
    while (((int64_t)1 << bits) < (int64_t)c->ns_map.size()) ++bits;
    const size_t tb = owgs_throttle_sort_bytes(n, bits);
    HIPCHK(c, c->q_temp.reserve(tb));
    HIPCHK(c, c->q_key.reserve(N));
    HIPCHK(c, c->q_idx0.reserve(N));
    HIPCHK(c, c->q_idx1.reserve(N));
    HIPCHK(c, c->v_rank.reserve(N));
    HIPCHK(c, c->d_out.reserve(N));
    HIPCHK(c, c->d_flags.reserve(N));
    // the block: header, then the gate's four int32 arrays, out_invoker, out_ticket, then the three byte arrays
    unsigned long long* hdr = (unsigned long long*)c->p_blk.p;
    int32_t* b_rc = (int32_t*)(c->p_blk.p + hdr_bytes);
    int32_t *b_rl = b_rc + N, *b_cc = b_rc + 2 * N, *b_cl = b_rc + 3 * N, *b_inv = b_rc + 4 * N, *b_tick = b_rc + 5 * N;
    uint8_t *b_ver = (uint8_t*)(b_rc + 6 * N), *b_flags = b_ver + N, *b_ex = b_ver + 2 * N;
    HIPCHK(c, hipMemsetAsync(hdr, 0, hdr_bytes, st));
    // stage 0: the gate (owgs_admit_batch), its outputs written into the block
    HIPCHK(c, upload(c->k_act, io->ns, N, st));
    HIPCHK(c, upload(c->k_kind, io->kind, N, st));
    HIPCHK(c, upload(c->k_off, io->t_ms, N, st));
    if (io->rate_override) HIPCHK(c, upload(c->v_ov0, io->rate_override, N, st));
    if (io->conc_override) HIPCHK(c, upload(c->v_ov1, io->conc_override, N, st));
    OwgsAdmitArgs G = admit_args(c, n);
    G.kind = c->k_kind.p;
    G.t_ms = c->k_off.p;
    G.rate_ov = io->rate_override ? c->v_ov0.p : nullptr;
    G.conc_ov = io->conc_override ? c->v_ov1.p : nullptr;
    G.out_verdict = b_ver;
    G.out_rate_count = b_rc;
    G.out_rate_limit = b_rl;
    G.out_conc_count = b_cc;
    G.out_conc_limit = b_cl;
    HIPCHK(c, owgs_launch_admit(c->k_act.p, bits, c->q_temp.p, tb, c->q_key.p, c->q_idx0.p, c->q_idx1.p, &G, st));
    // the events read only the gate's outputs: queued right behind it, they do not wait for the engine
    if (ev) {
        E.kind = c->k_kind.p;
        E.verdict = b_ver;
        E.rate_count = b_rc;
        E.rate_limit = b_rl;
        E.conc_count = b_cc;
        E.conc_limit = b_cl;
        E.ts = c->k_off.p;
        rc = ev_queue(c, E, ev_tb, st);
        if (rc) return rc;
    }
    int64_t waits = 0;
    // the event section of the pinned block handed out and the regions' bytes downloaded (not counted in [12], like the
    // message bytes); wait = false leaves the wait for the download to the caller
    auto events_out = [&](bool wait) {
        int re = ev_collect(c, n, ev, (const uint8_t*)c->p_pin.p + ev_at, &out_summary[15], &out_summary[13], st);
        if (wait && hipStreamSynchronize(st) != hipSuccess && re != OWGS_EDEVICE)
            re = c->fail(OWGS_EDEVICE, "invoke: the download of the events failed");
        return re;
    };
    // the five gate outputs from the pinned block (valid whenever the gate ran, whatever happens after it)
    auto gate_out = [&]() {
        const char* P = (const char*)c->p_pin.p + hdr_bytes;
        memcpy(io->out_rate_count, P, 4 * N);
        memcpy(io->out_rate_limit, P + 4 * N, 4 * N);
        memcpy(io->out_conc_count, P + 8 * N, 4 * N);
        memcpy(io->out_conc_limit, P + 12 * N, 4 * N);
        memcpy(io->out_verdict, P + 24 * N, N);
        for (int32_t i = 0; i < n; ++i) {
            const bool trig = (io->kind[i] & OWGS_ADMIT_TRIGGER) != 0;
            const uint8_t v = io->out_verdict[i];
            out_summary[8] += !trig && v == OWGS_ADMIT_OK;
            out_summary[9] += v == OWGS_ADMIT_RATE;
            out_summary[10] += v == OWGS_ADMIT_CONCURRENT;
            out_summary[11] += trig && v == OWGS_ADMIT_OK;
        }
    };
    // the engine step failed on the host side or reported its own error: the rate records stay charged and the gate's
    // outputs are handed out (the reference charges the rate before publish can fail); nothing is tracked or written
    auto engine_failed = [&](int code) {
        if (hipMemcpyAsync(c->p_pin.p, c->p_blk.p, blk_bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess) {
            gate_out();
            out_summary[12] = waits + 1;
            if (ev) (void)events_out(true);
        }
        return code;
    };
    // stage 1: the admitted actions through the engine, the decisions left in d_out / d_flags by rank
    if (c->large) {
        // the large-state engine's run takes host arrays: the verdicts come back once before it
        std::vector<uint8_t> ver(N);
        HIPCHK(c, hipMemcpyAsync(ver.data(), b_ver, N, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        ++waits;
        std::vector<int32_t> rank(N), act_c;
        std::vector<uint64_t> seq_c;
        for (int32_t i = 0; i < n; ++i) {
            const bool adm = !(io->kind[i] & OWGS_ADMIT_TRIGGER) && ver[i] == OWGS_ADMIT_OK;
            rank[i] = adm ? (int32_t)act_c.size() : -1;
            if (adm) {
                act_c.push_back(io->action[i]);
                if (io->seq) seq_c.push_back(io->seq[i]);
            }
        }
        HIPCHK(c, upload(c->v_rank, rank.data(), N, st));
        if (!act_c.empty())
            rc = publish_device(c, (int32_t)act_c.size(), act_c.data(), io->seq ? seq_c.data() : nullptr, io->seq_base,
                                nullptr, nullptr);
        if (rc) return engine_failed(rc);
    } else {
        HIPCHK(c, c->d_off.reserve(2));
        HIPCHK(c, c->d_a.reserve(N));
        if (io->seq) HIPCHK(c, c->d_seq.reserve(N));
        HIPCHK(c, c->v_map.reserve(N));
        HIPCHK(c, c->v_bcnt.reserve((N + 255) / 256));
        HIPCHK(c, upload(c->v_act, io->action, N, st));
        if (io->seq) HIPCHK(c, upload(c->v_seq, (const u64*)io->seq, N, st));
        OwgsInvokeCompact K{};
        K.n = n;
        K.verdict = b_ver;
        K.kind = c->k_kind.p;
        K.action = c->v_act.p;
        K.seq = io->seq ? c->v_seq.p : nullptr;
        K.bcnt = c->v_bcnt.p;
        K.act_c = c->d_a.p;
        K.seq_c = io->seq ? c->d_seq.p : nullptr;
        K.map = c->v_map.p;
        K.rank = c->v_rank.p;
        K.off = c->d_off.p;
        K.pad_out = c->d_out.p;
        K.pad_flags = c->d_flags.p;
        HIPCHK(c, owgs_launch_invoke_compact(&K, st));
        rc = invoke_engine(c, n, io->seq != nullptr, io->seq_base);
        if (rc) return engine_failed(rc);
    }
    // the inputs of stages 2 and 3 go up while the engine runs
    if (c->large) HIPCHK(c, upload(c->v_act, io->action, N, st));
    HIPCHK(c, upload(c->k_key, (const ulonglong2*)io->aid, N, st));
    HIPCHK(c, upload(c->k_r0, io->ticket, N, st));
    HIPCHK(c, upload(c->x_tl, (const long long*)io->time_limit_ms, N, st));
    OwgsMsgArgs A{};
    if (msgs) {
        rc = msg_upload(c, msgs, need, mo->n_topics, mo->cap, A, st);
        if (rc) return rc;
    }
    OwgsInvokeGate Q{};
    Q.n = n;
    Q.err = c->d_err.p;
    Q.rank = c->v_rank.p;
    Q.dec = c->d_out.p;
    Q.dflags = c->d_flags.p;
    Q.action = c->v_act.p;
    Q.act_bb = c->d_act_bb.p;
    Q.placed = c->p_placed.p;
    Q.msg_inv = msgs ? c->p_minv.p : nullptr;
    Q.hdr = hdr;
    Q.out_inv = b_inv;
    Q.out_ticket = b_tick;
    Q.out_flags = b_flags;
    Q.out_existed = b_ex;
    HIPCHK(c, owgs_launch_invoke_gate(&Q, st));
    // stage 2: setupActivation of the placed items, by item: the entry's invoker from the scattered decisions, the
    // namespace the gate's
    rc = track_device(c, n, c->k_key.p, c->v_act.p, c->k_act.p, c->k_r0.p, b_inv, c->x_tl.p, io->now_ms,
                      c->p_placed.p, b_tick, b_ex, hdr + OWGS_PUB_CNT, st);
    if (rc) return rc;
    // stage 3: the messages of the placed items
    if (msgs) {
        A.invoker = c->p_minv.p;
        A.aid = c->k_key.p;
        rc = msg_queue(c, A, mo->n_topics, st);
        if (rc) return rc;
        HIPCHK(c, owgs_launch_publish_collect(hdr, c->m_bad.p, A.topic_start, mo->n_topics, A.out_off, n, st));
    }
    HIPCHK(c, hipMemcpyAsync(c->p_pin.p, c->p_blk.p, blk_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ++waits;
    gate_out();
    out_summary[12] = waits;
    const char* P = (const char*)c->p_pin.p + hdr_bytes;
    const PublishBlock B{P + 16 * N, P + 20 * N, P + 25 * N, P + 26 * N};
    const int re = ev ? events_out(false) : OWGS_OK;
    const std::string ev_err = re ? c->err : std::string();
    rc = publish_tail(c, "invoke", n, B, io->out_invoker, io->out_flags, io->out_ticket, io->out_existed, msgs, mo,
                      out_summary, st);
    if (!ev) return rc;
    // the event bytes were queued before the message bytes: one wait covers both.  The message stage's code wins.
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = c->fail(OWGS_EDEVICE, "invoke: the download of the events failed");
    if (rc || !re) return rc;
    c->err = ev_err;
    return re;
}

int owgs_invoke_activations(owgs_ctx* c, const owgs_invoke_io* io, const owgs_msg_batch* msgs, owgs_msg_out* mo,
                            int64_t out_summary[16]) {
    return invoke_run(c, io, msgs, mo, nullptr, out_summary);
}

int owgs_invoke_activations_events(owgs_ctx* c, const owgs_invoke_io* io, const owgs_msg_batch* msgs,
                                   owgs_msg_out* mo, owgs_event_io* ev, int64_t out_summary[16]) {
    return invoke_run(c, io, msgs, mo, ev, out_summary);
}
