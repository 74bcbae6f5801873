/*
 * owgs.h -- C ABI of the MI355X-native batched invoker scheduler ("GPU sharding" balancer).
 *
 * This is the drop-in boundary for OpenWhisk's controller-side invoker assignment hot path.  A JVM shim
 * (GpuShardingContainerPoolBalancer) binds these symbols over JNI and keeps everything
 * else of CommonLoadBalancer (activation bookkeeping, Kafka send, ack feed) on the JVM side.
 * Paths below are relative to the reference repository root; abbreviations:
 *   SCPB = core/controller/src/main/scala/org/apache/openwhisk/core/loadBalancer/ShardingContainerPoolBalancer.scala
 *   CLB  = core/controller/src/main/scala/org/apache/openwhisk/core/loadBalancer/CommonLoadBalancer.scala
 *   LB   = core/controller/src/main/scala/org/apache/openwhisk/core/loadBalancer/LoadBalancer.scala
 *   NS   = common/scala/src/main/scala/org/apache/openwhisk/common/NestedSemaphore.scala
 *
 * Conventions
 *   - Every entry point returns 0 on success or a negative OWGS_E* code; nothing throws or aborts across the ABI.
 *     owgs_last_error() describes the last failure of a context.
 *   - Buffers are owned by the caller.  Functions without a _device suffix take HOST pointers; *_device functions
 *     take HIP device pointers (HBM-resident) and an optional hipStream_t passed as void*.
 *   - Per-activation outcome: out_invoker >= 0 is the chosen invoker id; OWGS_NONE (-1) is the reference's None
 *     ("No invokers available", SCPB:305-316); OWGS_THROW_INDEX (-2) marks an input for which the reference's
 *     schedule() throws IndexOutOfBoundsException (Int.MinValue hash, SCPB:266-268/411, or an invoker id outside
 *     invokerSlots, SCPB:413/422).  out_flags bit0 (OWGS_FLAG_OVERLOAD) = overload random fallback + forceAcquire
 *     (SCPB:417-424); the JVM shim turns it into the MANAGED/BLACKBOX_SYSTEM_OVERLOAD counter (SCPB:277-286).
 *   - Release flags: bit0 NoSuchElementException (NS:103), bit1 permit overflow Error (ForcibleSemaphore.scala:48-50),
 *     bit2 activation has no entry (it was never scheduled: CLB:278-279 finds no ActivationEntry).
 *   - Sequential semantics: a batch is equivalent to the reference executing, in array order, one schedule()
 *     (or releaseInvoker()) per element against the single-writer context.  The random overload fallback draws
 *     its index with the counter RNG keyed by (rng_seed, seq) documented in DESIGN.md (replaces ThreadLocalRandom,
 *     SCPB:421).
 *   - One context = one controller shard (SCPB horizontal sharding, SCPB:126-133); contexts are single-writer.
 *   - Calls on one context take effect in the order they are issued, whatever stream each names: an asynchronous call
 *     (the *_device functions, owgs_restore, owgs_update_health_device) leaves its work as the context's tail, and
 *     the next call -- on any stream, or a synchronous one -- is ordered after it on the device.  Device buffers the
 *     caller passes to an asynchronous call are read when `stream` reaches the call's work: keep them valid (and
 *     unmodified) until then.
 */
#ifndef OWGS_H
#define OWGS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OWGS_ABI_VERSION 1

#define OWGS_OK 0
#define OWGS_EINVAL (-22)  /* bad argument */
#define OWGS_ENOMEM (-12)  /* allocation failed (host or device) */
#define OWGS_EDEVICE (-5)  /* HIP runtime error */
#define OWGS_ERANGE (-34)  /* state too large for the engine (see owgs_limits) */
#define OWGS_ENOENT (-2)   /* unknown action / invoker */

#define OWGS_NONE (-1)
#define OWGS_THROW_INDEX (-2)
#define OWGS_FLAG_OVERLOAD 1u

#define OWGS_REL_NOSUCHELEMENT 1u
#define OWGS_REL_OVERFLOW 2u
#define OWGS_REL_NOENTRY 4u

/* InvokerState (core/controller/.../loadBalancer/InvokerSupervision.scala:47-66): only HEALTHY is usable. */
#define OWGS_HEALTHY 0
#define OWGS_UNHEALTHY 1
#define OWGS_UNRESPONSIVE 2
#define OWGS_OFFLINE 3

typedef struct owgs_ctx owgs_ctx;

typedef struct owgs_config {
    double managed_fraction;  /* whisk.loadbalancer.managed-fraction  (core/controller/src/main/resources/reference.conf:22-32) */
    double blackbox_fraction; /* whisk.loadbalancer.blackbox-fraction */
    int64_t min_memory_bytes; /* MemoryLimit.MIN_MEMORY (common/scala/src/main/resources/application.conf:377) */
    int32_t cluster_size;     /* initial cluster size (SCPB:457 default 1) */
    int32_t device;           /* HIP device ordinal */
    uint64_t rng_seed;        /* overload-fallback RNG seed (DESIGN.md "Counter RNG") */
} owgs_config;

/* Replaces: object ShardingContainerPoolBalancer.instance(...) building the balancer (SCPB:336-365) and
 * ShardingContainerPoolBalancerState() (SCPB:449-470). */
int owgs_create(const owgs_config* cfg, owgs_ctx** out);
void owgs_destroy(owgs_ctx* ctx);
const char* owgs_last_error(const owgs_ctx* ctx);
int owgs_abi_version(void);
/* Diagnostics (runs without a GPU): each engine object (wide / narrow geometry) refuses a launch prepared for the other
 * geometry before anything runs -- the launch wrappers compare the host's geometry tag with their own, and the kernels
 * check it again before their first barrier (a mismatch fails the call with OWGS_EDEVICE, "engine geometry").
 * OWGS_OK when every wrapper refused. */
int owgs_geometry_selfcheck(void);
/* max invokers / slots the engine holds on chip (LDS); beyond them the large-state engine runs the context (DESIGN.md
 * section 9), as it does one that has both a slot of 2^22 MB or more and a memory limit above 4095 MB: the on-chip
 * engine's capacities floor(permits / mem) are exact below either bound (csrc/owgs_divq.h), and it refuses a state
 * beyond both (OWGS_ERANGE).  States no engine holds return OWGS_ERANGE from update_invokers. */
int owgs_limits(int32_t* max_invokers, int32_t* max_slots);

/* Replaces: ShardingContainerPoolBalancerState.updateInvokers(newInvokers: IndexedSeq[InvokerHealth]) (SCPB:512-551),
 * driven by the monitor actor on CurrentInvokerPoolState (SCPB:226-227).  status: OWGS_HEALTHY..OWGS_OFFLINE. */
int owgs_update_invokers(owgs_ctx* ctx, int32_t n, const int32_t* ids, const int64_t* user_memory_bytes,
                         const uint8_t* status);

/* Replaces: ShardingContainerPoolBalancerState.updateCluster(newSize) (SCPB:561-584), driven by the Akka cluster
 * membership events in the monitor actor (SCPB:230-248). */
int owgs_update_cluster(owgs_ctx* ctx, int32_t new_size);

/* Registers actions (the per-activation inputs of publish, SCPB:260-276).  For action i:
 *   namespace  = msg.user.namespace.name.asString   (SCPB:266, hashed)
 *   path       = action.fullyQualifiedName(false).asString, e.g. "ns/pkg/name" (SCPB:266, hashed)
 *   key        = action.fullyQualifiedName(true).asString ("ns/pkg/name@0.0.1"): the NestedSemaphore map key (SCPB:271)
 *   mem_mb     = action.limits.memory.megabytes (SCPB:274);  max_conc = action.limits.concurrency.maxConcurrent (SCPB:270)
 *   blackbox   = action.exec.pull (SCPB:260)
 * Strings are concatenated in *_bytes with offsets *_off[0..n] (n+1 entries).  generateHash (SCPB:370-372) runs on the
 * GPU; out_hash (optional) receives it, out_action receives the action handle used by the batch calls. */
int owgs_register_actions(owgs_ctx* ctx, int32_t n, const char* ns_bytes, const int32_t* ns_off,
                          const char* path_bytes, const int32_t* path_off, const char* key_bytes,
                          const int32_t* key_off, const int32_t* mem_mb, const int32_t* max_conc,
                          const uint8_t* blackbox, int32_t* out_action, int32_t* out_hash);

/* Replaces the reference's NestedSemaphore map lifetime (NestedSemaphore.scala:109-111: an entry exists only while
 * activations of its fqn@version are in flight; nothing else is keyed by it).  The caller drops action handles it will
 * not name again (a cold action, a superseded fqn@version): none of their activations may still be in flight and no
 * later call may name them.  Handle ids are reused by later owgs_register_actions calls; an fqn@version key that no
 * live handle names is recycled when registrations run out of key ids, once no map entry and no watched pair holds it
 * (a device scan; keys still held stay pending).  A restore of a snapshot taken before a key was recycled returns
 * OWGS_EINVAL.  With this a long-running controller never runs out of the 131,070 key / 131,070 handle ids. */
int owgs_release_actions(owgs_ctx* ctx, int32_t n, const int32_t* actions);

/* Replaces: the scheduling half of ShardingContainerPoolBalancer.publish (SCPB:257-290) -- pool selection, hash,
 * home invoker, step size and ShardingContainerPoolBalancer.schedule (SCPB:398-436) with NestedSemaphore
 * tryAcquireConcurrent / forceAcquireConcurrent (NS:32-91) -- for n activations in array order.
 * seq[i] keys the overload RNG (may be NULL: seq = seq_base + i). */
int owgs_publish_batch(owgs_ctx* ctx, int32_t n, const int32_t* action, const uint64_t* seq, uint64_t seq_base,
                       int32_t* out_invoker, uint8_t* out_flags);

/* Replaces: ShardingContainerPoolBalancer.releaseInvoker (SCPB:327-331) reached from CommonLoadBalancer
 * .processCompletion (CLB:260-346): invokerSlots.lift(invoker).foreach(_.releaseConcurrent(fqn, maxConcurrent, mem)).
 * invoker < 0 means "no ActivationEntry" (flag OWGS_REL_NOENTRY, no state change). out_flags may be NULL. */
int owgs_release_batch(owgs_ctx* ctx, int32_t n, const int32_t* invoker, const int32_t* action, uint8_t* out_flags);

/* Replaces: one drained batch of the JVM shim's batching thread -- for each run r in order, releaseInvoker for the
 * completions [rel_off[r], rel_off[r+1]) (SCPB:327-331 via CommonLoadBalancer.processCompletion, CLB:260-346; invoker
 * and action handle of the ActivationEntry, invoker < 0 = no entry) and then the scheduling half of publish
 * (SCPB:257-290) for the activations [pub_off[r], pub_off[r+1]).  Same results as alternating owgs_release_batch and
 * owgs_publish_batch calls.  Small calls on identity pools without watched pairs (at most OWGS_RES_MAX = 1024
 * releases + publishes by default) are served by a resident engine that keeps the slot state on chip between calls:
 * inputs and outputs through pinned host memory, a doorbell, no launch or synchronisation per call; it writes the
 * state back and exits when any other entry point of the context is called, or after 20 ms without a call
 * (OWGS_RES_IDLE_US; OWGS_RESIDENT=0 disables it).  Other calls: one pinned copy in, one launch chain, one pinned copy
 * out, one synchronisation.  rel_off / pub_off have n_runs + 1 entries starting at 0; seq may be NULL (seq = seq_base
 * + publish index); rel_flags may be NULL. */
int owgs_process_batch(owgs_ctx* ctx, int32_t n_runs, const int32_t* rel_off, const int32_t* rel_invoker,
                       const int32_t* rel_action, uint8_t* rel_flags, const int32_t* pub_off,
                       const int32_t* pub_action, const uint64_t* seq, uint64_t seq_base, int32_t* out_invoker,
                       uint8_t* out_flags);

/* Replaces: ShardingContainerPoolBalancer.schedule(maxConcurrent, fqn, invokers, dispatched, slots, index, step)
 * (SCPB:398-436) called directly with an explicit walk, as the reference unit tests do (ShardingContainerPoolBalancer
 * Tests.scala:244-412).  pool = 0 managed / 1 blackbox pool of the context; key = slot-key id (see owgs_key_id). */
int owgs_schedule_walks(owgs_ctx* ctx, int32_t n, const uint8_t* pool, const int32_t* index, const int32_t* step,
                        const int32_t* mem_mb, const int32_t* max_conc, const int32_t* key, const uint64_t* seq,
                        int32_t* out_invoker, uint8_t* out_flags);

/* Test seam mirroring `protected[loadBalancer] var _invokerSlots` (SCPB:455): replace the slot vector with n fresh
 * NestedSemaphores of the given memory permits (concurrency maps emptied). */
int owgs_set_slots(owgs_ctx* ctx, int32_t n, const int32_t* permits);
/* Replaces the pool vectors for the explicit-walk tests: managed pool = (ids, status) as given. */
int owgs_set_pool(owgs_ctx* ctx, int32_t pool, int32_t n, const int32_t* ids, const uint8_t* status);

/* Introspection (ForcibleSemaphore.availablePermits / NestedSemaphore.concurrentState / state getters). */
int owgs_read_permits(owgs_ctx* ctx, int32_t* out, int32_t cap, int32_t* n_slots);
int owgs_read_concurrent(owgs_ctx* ctx, int32_t invoker, int32_t key, int32_t* permits, int32_t* op_count);
int owgs_key_id(owgs_ctx* ctx, int32_t action);
/* Diagnostics (synchronises): the NestedSemaphore map's fill -- live and deleted entries of the on-chip primary table,
 * entries (live + deleted) and capacity of the HBM overflow. */
int owgs_map_fill(owgs_ctx* ctx, int32_t* primary_live, int32_t* primary_deleted, int32_t* overflow_entries,
                  int32_t* overflow_cap);
int owgs_state_info(owgs_ctx* ctx, int32_t* n_invokers, int32_t* managed, int32_t* blackbox, int32_t* cluster_size);
int owgs_step_sizes(owgs_ctx* ctx, int32_t pool, int32_t* out, int32_t cap, int32_t* n);

/* Replaces: ShardingContainerPoolBalancer.pairwiseCoprimeNumbersUntil(x) (SCPB:379-384), the step-size table that
 * updateInvokers (SCPB:525-527) rebuilds on the device; exposed for the reference's unit test
 * (ShardingContainerPoolBalancerTests.scala:371-384).  Writes min(cap, n) values to out (may be NULL), n = list length.
 * x > owgs_limits' pool range returns OWGS_ERANGE. */
int owgs_pairwise_coprime(owgs_ctx* ctx, int32_t x, int32_t* out, int32_t cap, int32_t* n);

/* Stream replay with HBM-resident buffers (bench / batching thread).  Batch b first releases the activations
 * rel_aid[rel_off[b]..rel_off[b+1]) (ids into this stream; their invoker is this stream's own earlier output),
 * then publishes activations [acq_off[b], acq_off[b+1]) with action act[i] and seq = seq_base + i.
 * n_activations = acq_off[n_batches], n_releases = rel_off[n_batches] (given so no device read is needed).
 * All pointers are device pointers; stream is a hipStream_t (NULL = the context's stream).  Asynchronous, with one
 * exception: when the call's activations could fill the HBM overflow of the NestedSemaphore map past half its capacity
 * (its upper bound: the entries it holds plus one per activation), the call first synchronises `stream`, reads the
 * exact entry count back and, if still needed, grows and rehashes the table before launching. */
int owgs_replay_device(owgs_ctx* ctx, int32_t n_batches, const int64_t* acq_off, const int32_t* act,
                       int64_t n_activations, const int64_t* rel_off, const int64_t* rel_aid, int64_t n_releases,
                       uint64_t seq_base, int32_t* out_invoker, uint8_t* out_flags, uint8_t* rel_flags, void* stream);
/* One batch of a stream replayed batch by batch, so that state updates can come in between (configs[4]: the health
 * all-gather between batches feeding owgs_update_health_device, i.e. updateInvokers, SCPB:512-551): releases
 * rel_aid[r_beg, r_end) -- activations of this stream decided by EARLIER calls, their invoker read from out_invoker --
 * then publishes act[a_beg, a_end) with seq = seq_base + i; every index is into the whole stream's arrays (device
 * pointers).  Same results as the batch inside one owgs_replay_device call of the whole stream with the same state
 * updates between batches.  Asynchronous on `stream` (same exception as owgs_replay_device). */
int owgs_replay_device_span(owgs_ctx* ctx, int64_t a_beg, int64_t a_end, int64_t r_beg, int64_t r_end,
                            const int32_t* act, const int64_t* rel_aid, uint64_t seq_base, int32_t* out_invoker,
                            uint8_t* out_flags, uint8_t* rel_flags, void* stream);
/* Consecutive batches of a stream replayed batch by batch in ONE engine launch, with a health vector applied before
 * each batch (configs[4]'s cadence: the health all-gathered between batches, applied as updateInvokers with a new
 * status vector, SCPB:512-551, before the batch's releases).  acq_off / rel_off are HOST arrays [n_batches + 1] of
 * indices into the whole stream's device arrays (as owgs_replay_device_span's a_beg..r_end, per batch); releases may
 * name activations decided by earlier calls or by earlier batches of this group.  status_dev (device, nullable):
 * row b = status_dev + b * status_stride holds n_status InvokerState codes (n_status = the context's invokers);
 * after the call the context's health is the last row's.  Same results as owgs_update_health_device(row b) +
 * owgs_replay_device_span(batch b) for every b.  Identity pools without watched pairs run one launch; otherwise the
 * call takes exactly that batch-by-batch sequence.  Asynchronous on `stream` (same exception as owgs_replay_device). */
int owgs_replay_device_group(owgs_ctx* ctx, int32_t n_batches, const int64_t* acq_off, const int64_t* rel_off,
                             const int32_t* act, const int64_t* rel_aid, uint64_t seq_base, int32_t* out_invoker,
                             uint8_t* out_flags, uint8_t* rel_flags, const uint8_t* status_dev, int64_t status_stride,
                             int32_t n_status, void* stream);
/* Several controller shards (clusterSize > 1, one context each, same device) replayed by ONE engine launch, one
 * workgroup per shard: the reference runs one ShardingContainerPoolBalancer per controller (SCPB:126-133,
 * 485-499); this hosts up to 64 of them on one GPU (up to 8 argument blocks travel in the kernarg segment, more
 * through a pinned host buffer and HBM owned by ctxs[0]).  io[i] holds owgs_replay_device's arguments for ctxs[i];
 * every shard needs n_batches > 0.  Same results as k separate owgs_replay_device calls.  Asynchronous on `stream`
 * (same exception as owgs_replay_device, per shard). */
typedef struct owgs_replay_io {
    int32_t n_batches;
    const int64_t* acq_off;
    const int32_t* act;
    int64_t n_activations;
    const int64_t* rel_off;
    const int64_t* rel_aid;
    int64_t n_releases;
    uint64_t seq_base;
    int32_t* out_invoker;
    uint8_t* out_flags;
    uint8_t* rel_flags;
} owgs_replay_io;
int owgs_replay_device_multi(owgs_ctx** ctxs, int32_t k, const owgs_replay_io* io, void* stream);
/* Same with host buffers (copies in and out, synchronous). */
int owgs_replay(owgs_ctx* ctx, int32_t n_batches, const int64_t* acq_off, const int32_t* act, const int64_t* rel_off,
                const int64_t* rel_aid, uint64_t seq_base, int32_t* out_invoker, uint8_t* out_flags,
                uint8_t* rel_flags);

/* ---- completion path (CommonLoadBalancer.processAcknowledgement / processCompletion, CLB:205-346) ----------------
 * activationSlots (CLB:60) lives on the device: an activation is tracked when it is published and removed by its
 * completion ack.  Per-message outcome codes (out_kind): */
#define OWGS_ACK_FAIL 0           /* AcknowledegmentMessage.parse fails (CLB:226-228): the shim logs the raw message */
#define OWGS_ACK_JVM 1            /* the message has a "response" member (ResultMessage / Combined...): its
                                     WhiskActivation is deserialised by the JVM, which completes the slot with
                                     owgs_complete_activations.  From owgs_process_result_acks: only a message whose
                                     `response` object lies outside the accepted subset */
#define OWGS_ACK_UNSUPPORTED 2    /* outside the device parser's limits (container depth > 64, an exponent of more
                                     than 9 digits, a non-ASCII or numeric activation id, U+FFFF, a number of more
                                     than 34 significant digits in instance / transid): the JVM parses it */
#define OWGS_ACK_RELEASED 3       /* processCompletion found the entry: releaseInvoker ran (CLB:286-319) */
#define OWGS_ACK_HEALTH 4         /* no entry, transid == TransactionId.invokerHealth (CLB:320-328) */
#define OWGS_ACK_NOENTRY 5        /* no entry, regular ack after a forced one (CLB:329-337) */
#define OWGS_ACK_FORCED_NOENTRY 6 /* no entry, forced (timeout) after a regular ack (CLB:338-345) */

/* TransactionId.invokerHealth's start (TransactionId.scala:225) of this controller: health acks echo it. */
int owgs_set_health_tid(owgs_ctx* ctx, int64_t start_ms);

/* Replaces: activationSlots.getOrElseUpdate(msg.activationId, ActivationEntry(...)) in setupActivation (CLB:148-166),
 * in array order.  aid32 = n activation ids of 32 chars [0-9a-f] (ActivationId.asString, no terminator); action =
 * the action handle (its limits and fqn@version are the entry's); ticket = the caller's handle for its own per-
 * activation state (promise, timeout handler).  out_ticket = the ticket of the entry now in the map (the existing
 * one when out_existed = 1). */
int owgs_track_activations(owgs_ctx* ctx, int32_t n, const char* aid32, const int32_t* action, const int32_t* ticket,
                           int32_t* out_ticket, uint8_t* out_existed);

/* Replaces: processAcknowledgement (CLB:205-232) for n raw ack messages (UTF-8 bytes, offsets off[0..n]) processed
 * in array order: AcknowledegmentMessage.parse (Message.scala:237-256) on the device, then for every
 * CompletionMessage processCompletion(aid, tid, forced = false, isSystemError, invoker) (CLB:260-346): the entry is
 * removed and releaseInvoker(invoker, entry) (SCPB:327-331) applied.  out_invoker = the message's invoker instance,
 * out_ticket = the removed entry's ticket (-1 otherwise), out_flags bit0 = isSystemError, bits1-2 = the release
 * flags (OWGS_REL_NOSUCHELEMENT, OWGS_REL_OVERFLOW) of releaseInvoker.  The shim sends InvocationFinishedMessage
 * for RELEASED / HEALTH outcomes and completes promises for OWGS_ACK_JVM messages. */
int owgs_process_acks(owgs_ctx* ctx, int32_t n, const char* bytes, const int64_t* off, uint8_t* out_kind,
                      int32_t* out_invoker, int32_t* out_ticket, uint8_t* out_flags);
/* Same with device buffers (bytes padded by 16 readable bytes past off[n]); stream as in owgs_replay_device. */
int owgs_process_acks_device(owgs_ctx* ctx, int32_t n, const uint8_t* bytes, const int64_t* off, uint8_t* out_kind,
                             int32_t* out_invoker, int32_t* out_ticket, uint8_t* out_flags, void* stream);

/* Replaces: processCompletion (CLB:260-346) called directly -- the completion-ack timeout (forced, CLB:150-152) and
 * the completion half of messages the JVM parsed itself (OWGS_ACK_JVM).  flags bit0 forced, bit1 isSystemError,
 * bit2 transid == invokerHealth.  Outcomes and out_flags as in owgs_process_acks. */
int owgs_complete_activations(owgs_ctx* ctx, int32_t n, const char* aid32, const int32_t* invoker,
                              const uint8_t* flags, uint8_t* out_kind, int32_t* out_ticket, uint8_t* out_flags);
/* activationSlots.size */
int owgs_activations_live(owgs_ctx* ctx, int64_t* live);

/* ---- in-flight books (CLB:62-65) ----
 * totalActivations, totalBlackBoxActivationMemory, totalManagedActivationMemory and activationsPerNamespace, which
 * setupActivation increments (CLB:121-127) and processCompletion decrements for the entry it removed (CLB:280-284).
 * They are what LoadBalancer.activeActivationsFor / totalActiveActivations return (CLB:83-85), what the in-flight
 * gauges emit (CLB:68-79) and what ActivationThrottler.check reads.  The track and completion calls above keep them:
 *   - tracking counts EVERY item, an id that already has an entry included (CLB:121-127 run before getOrElseUpdate,
 *     CLB:148): total += 1, the memory total of the action's pool += its megabytes, the item's namespace += 1.  A
 *     duplicate id so leaks one count, as in the reference.  The entry keeps the namespace and action of its first
 *     tracker in array order.  A batch rejected with an error counts nothing.
 *   - a completion whose outcome is OWGS_ACK_RELEASED subtracts the removed ENTRY's values (its action's megabytes
 *     and pool, its namespace), not the message's.  No other outcome touches a counter.
 * Per-namespace counters are int32 with wrapping arithmetic (LongAdder.intValue, CLB:84), the totals int64.
 * owgs_snapshot / owgs_restore leave them alone, as they leave activationSlots alone. */

#define OWGS_NS_INITIAL_CAP 1024 /* namespaces the device counter array holds before its first growth */
/* msg.user.namespace.uuid (CLB:127, 157) -> dense handle.  uuid128 = 2n words (hi, lo).  Idempotent: a uuid already
 * registered returns its handle.  Handles are never reused in this version. */
int owgs_register_namespaces(owgs_ctx* ctx, int32_t n, const uint64_t* uuid128, int32_t* out_ns);

/* owgs_track_activations with msg.user.namespace.uuid per item: ns[i] is a namespace handle or OWGS_NONE (the item
 * moves the totals and no namespace).  An unknown handle returns OWGS_ENOENT before any state changes.  Outputs and
 * table behaviour are those of owgs_track_activations, which behaves as ns = OWGS_NONE for every item. */
int owgs_track_activations_ns(owgs_ctx* ctx, int32_t n, const char* aid32, const int32_t* action, const int32_t* ns,
                              const int32_t* ticket, int32_t* out_ticket, uint8_t* out_existed);

/* Replaces: activeActivationsFor(namespace) (CLB:83-84) for n namespace handles; ordered after earlier calls. */
int owgs_active_activations(owgs_ctx* ctx, int32_t n, const int32_t* ns, int32_t* out);
/* out[0] totalActivations, out[1] totalManagedActivationMemory (MB), out[2] totalBlackBoxActivationMemory (MB)
 * (CLB:63-65); totalActiveActivations (CLB:85) is (int32_t)out[0].  Ordered after earlier calls. */
int owgs_activation_totals(owgs_ctx* ctx, int64_t out[3]);

/* Sequential replay, in array order, of ActivationThrottler.check (ActivationThrottler.scala:41-49, ConcurrentRateLimit
 * :58-59) followed, for admitted jobs, by setupActivation's namespace count (CLB:127):
 *   count_i = active[ns_i] + #{ j < i : ns_j == ns_i and ok_j };   ok_i = count_i < limit_i
 * Read-only: no counter changes (they move when the admitted jobs are tracked).
 * Assumption: an admitted job is tracked afterwards.  That holds whenever the pool has a usable invoker: schedule
 * returns None only with no healthy invoker (SCPB:398-436), and only then does publish skip setupActivation; a batch
 * checked while no invoker is usable counts admitted jobs that will not be tracked against the later jobs of their
 * namespace.  ns[i] = OWGS_NONE returns OWGS_EINVAL, an unknown handle OWGS_ENOENT. */
int owgs_throttle_batch(owgs_ctx* ctx, int32_t n, const int32_t* ns, const int32_t* limit, int32_t* out_count,
                        uint8_t* out_ok);

/* ---- entitlement throttle gate (Entitlement.scala:197-202, 354-381) ----
 * The two throttles every invoke and fire passes before publish, for a drained batch in array order: the per-minute
 * rate throttle (invokeRateThrottler / triggerRateThrottler: RateThrottler.scala:47-54, RateInfo :60-86) and, only for
 * an action that passed it, the concurrent throttle (ActivationThrottler.scala:41-49) over the in-flight books.
 *
 * State: per namespace handle two independent rate records (invoke, fire), each absent or (lastMin int64, count
 * int32).  They persist across calls, grow with the namespace counters and, like the books, are left alone by
 * owgs_snapshot / owgs_restore.
 *
 * Limit of an item: all three limits go through calculateIndividualLimit (Entitlement.scala:97-133, 144-149), with
 * cs = the context's cluster size (owgs_update_cluster) at the time of the call:
 *   abs   = override present ? override : system default
 *   dil   = (int) ceil((double)abs * (cs > 1 ? 1.2 : 1.0))     IEEE double; the conversion saturates to int32
 *   limit = dil == 0 ? 0 : max(dil / cs, 1)                     truncating division
 * so a negative override yields 1.
 *
 * Item i with namespace h, kind, t_ms[i] (the System.currentTimeMillis of its check), m = t_ms[i] / 60000:
 *   1. r = the record of (h, kind).  Absent: r = (m, 0).  m != r.lastMin: r = (m, 0) -- a clock that steps back
 *      resets too (RateThrottler.scala:77-83).  Then r.count += 1 (wrapping int32), rate_count[i] = r.count,
 *      rate_ok = rate_count[i] <= rate_limit[i].  The count is charged whether or not the item passes.
 *   2. not rate_ok: verdict OWGS_ADMIT_RATE; the concurrent check is not evaluated, conc_count[i] = -1.
 *   3. trigger: verdict OWGS_ADMIT_OK (no concurrent throttle, Entitlement.scala:378), conc_count[i] = -1,
 *      conc_limit[i] = 0.
 *   4. action: conc_count[i] = active[h] + #{ j < i : ns_j == h, verdict_j == OK, j an action };
 *      verdict = conc_count[i] < conc_limit[i] ? OWGS_ADMIT_OK : OWGS_ADMIT_CONCURRENT.
 * Step 4 is owgs_throttle_batch's rule restricted to the actions that passed the rate check, with its assumption (an
 * admitted action is tracked afterwards); the in-flight counters are only read. */
#define OWGS_ADMIT_OK 0
#define OWGS_ADMIT_RATE 1
#define OWGS_ADMIT_CONCURRENT 2
#define OWGS_ADMIT_TRIGGER 1       /* kind bit 0: a trigger fire (else an action invoke) */
#define OWGS_ADMIT_RATE_OVERRIDE 2 /* kind bit 1: rate_override[i] is limits.invocationsPerMinute / firesPerMinute */
#define OWGS_ADMIT_CONC_OVERRIDE 4 /* kind bit 2: conc_override[i] is limits.concurrentInvocations */

/* actionInvokePerMinuteLimit, triggerFirePerMinuteLimit, actionInvokeConcurrentLimit (Entitlement.scala:138, 142,
 * 153).  Until set: 60, 60, 30.  Applies from the next owgs_admit_batch call. */
int owgs_set_throttle_limits(owgs_ctx* ctx, int32_t invokes_per_minute, int32_t fires_per_minute,
                             int32_t concurrent_invocations);

/* The gate over n items.  An override array may be NULL when no item sets its kind bit.  t_ms in [0, 2^60).
 * out_rate_limit / out_conc_limit are the computed limits (Messages.tooManyRequests(count, allowed); the
 * ConcurrentInvocations metric is conc_count + 1, Entitlement.scala:389-391; owgs_throttle_events below prints both
 * from these outputs); out_conc_limit is written for every action, also when its concurrent check was skipped.
 * ns[i] = OWGS_NONE, a reserved kind bit, a kind bit without its array or a t_ms outside the range return
 * OWGS_EINVAL, an unknown handle OWGS_ENOENT, all before any state changes. */
int owgs_admit_batch(owgs_ctx* ctx, int32_t n, const int32_t* ns, const uint8_t* kind, const int64_t* t_ms,
                     const int32_t* rate_override, const int32_t* conc_override, uint8_t* out_verdict,
                     int32_t* out_rate_count, int32_t* out_rate_limit, int32_t* out_conc_count,
                     int32_t* out_conc_limit);

/* The rate records of n namespace handles: which = 0 the invoke throttler's, 1 the fire throttler's.  An absent record
 * reads out_last_min = INT64_MIN, out_count = 0.  For tests and gauges; ordered after earlier calls. */
int owgs_rate_state(owgs_ctx* ctx, int32_t n, const int32_t* ns, int32_t which, int64_t* out_last_min,
                    int32_t* out_count);

/* ---- completion-ack timeouts (CLB:103-105, 148-152) ----
 * setupActivation arms one timer per ActivationEntry inside getOrElseUpdate (CLB:148-152); a regular ack cancels it
 * (CLB:289); a fired timer runs processCompletion(aid, tid, forced = true, isSystemError = false, invoker =
 * entry.invoker), which removes the entry, takes it out of the books, releases the invoker and sends
 * InvocationFinishedMessage(invoker, Timeout) (CLB:266-267, 278-317).  Here the deadline and the entry's invoker are
 * stored with the entry, and one call fires everything that is due.  An entry a regular ack removed has no deadline
 * left, so a sweep never produces OWGS_ACK_FORCED_NOENTRY; a regular ack that arrives after the sweep gets
 * OWGS_ACK_NOENTRY (CLB:329-337).  Entries tracked through owgs_track_activations / owgs_track_activations_ns never
 * expire; owgs_complete_activations with the forced bit keeps working for callers that keep their own timers.
 *
 * Order.  The reference pins no order among akka timers that are due together.  This project defines one: ascending
 * (deadline, arm order), where arm order is the order in which the entries were created -- track call order, then
 * array index within a call.  Within one sweep it shows in the output arrays, in which release sees a
 * ForcibleSemaphore overflow, and in the rank-dependent concurrent releases. */

/* calculateCompletionAckTimeout (CLB:103-105): TimeLimit.STD_DURATION, lbConfig.timeoutFactor, lbConfig.timeoutAddon.
 * Defaults 60000, 2, 60000 (TimeLimit std 1 minute; reference.conf timeout-factor 2, timeout-addon 1m).  std_ms and
 * addon_ms in [0, 2^40), factor in [1, 2^16), else OWGS_EINVAL.  Applies to entries armed afterwards. */
int owgs_set_ack_timeout(owgs_ctx* ctx, int64_t std_ms, int32_t factor, int64_t addon_ms);

/* owgs_track_activations_ns plus the entry's invoker (ActivationEntry.invoker, CLB:158) and its action time limit
 * (ActivationEntry.timeLimit, CLB:160).  The item that CREATES an entry arms its deadline
 *   now_ms + max(time_limit_ms[i], std_ms) * factor + addon_ms
 * An item whose id already has an entry arms nothing (the by-name block of getOrElseUpdate does not run, CLB:148-152);
 * it is still counted by the books, as today.  ns may be NULL (every item OWGS_NONE).  now_ms in [0, 2^60),
 * time_limit_ms[i] in [0, 2^40), invoker[i] >= 0, else OWGS_EINVAL; unknown handles and malformed ids as in
 * owgs_track_activations_ns; a rejected batch changes nothing. */
int owgs_track_activations_timed(owgs_ctx* ctx, int32_t n, const char* aid32, const int32_t* action,
                                 const int32_t* ns, const int32_t* ticket, const int32_t* invoker,
                                 const int64_t* time_limit_ms, int64_t now_ms, int32_t* out_ticket,
                                 uint8_t* out_existed);

/* Every timer due at or before now_ms fires: processCompletion(aid, tid, forced = true, isSystemError = false,
 * invoker = entry.invoker) (CLB:150-152, 260-317) for each live entry with deadline <= now_ms, in ascending
 * (deadline, arm order), at most cap of them.  *out_n = entries expired by this call, *out_remaining = due entries left
 * armed because of cap (cap = 0: the due count, nothing expires; the output arrays may then be NULL).  out_aid = 2
 * words (hi, lo) per entry; out_flags = the release flags of releaseInvoker << 1 as in owgs_process_acks.  An entry
 * invoker beyond invokerSlots is a no-op release (lift, SCPB:329).  feed_health != 0: the expired entries'
 * InvocationFinishedMessage(invoker, Timeout) (CLB:317) go to the device health FSM as OWGS_EV_TIMEOUT events at time
 * now_ms in the same order, with apply = 0 (a sweep that expires nothing feeds nothing and leaves the FSM's clock
 * alone); now_ms before the FSM's last now_ms is then OWGS_EINVAL with nothing expired.  now_ms in [0, 2^60),
 * cap >= 0. */
int owgs_expire_activations(owgs_ctx* ctx, int64_t now_ms, int32_t cap, int32_t feed_health, int32_t* out_n,
                            int64_t* out_remaining, uint64_t* out_aid, int32_t* out_ticket, int32_t* out_invoker,
                            int64_t* out_deadline, uint8_t* out_flags);

/* A lower bound of the earliest armed deadline (INT64_MAX: none): what the shim sleeps until.  It may be earlier than
 * the true minimum after regular acks removed entries; a sweep makes it exact for every tile it scanned. */
int owgs_next_deadline(owgs_ctx* ctx, int64_t* t_ms);

/* out[0] sweeps, [1] tiles scanned over all sweeps, [2] tiles scanned by the last sweep, [3] entries expired over all
 * sweeps, [4] tiles of the current table (1,024 slots each; 0 before the table exists). */
int owgs_expiry_stats(owgs_ctx* ctx, int64_t out[5]);

/* ---- invoker health supervision ----
 * Replaces: InvokerPool (InvokerSupervision.scala:95-210: registerInvoker on the first ping, padToIndexed with Offline
 * entries, InvocationFinishedMessage forwarding) and one InvokerActor FSM per invoker (InvokerSupervision.scala:
 * 285-440: Offline / Unhealthy / Unresponsive / Healthy, 10 s state timeout, 1-minute Tick sending test actions
 * while Unhealthy or Unresponsive, a ring buffer of the last 10 results with tolerance 3).
 * Events are in mailbox order with non-decreasing times (ms, in [0, 2^60)) that never go back before the previous
 * batch's now_ms;
 * timers due at or before an event's time fire before it, and all timers due at or before now_ms fire at the end.
 * user_memory_bytes = the pinging InvokerInstanceId's userMemory (ignored for other kinds).  apply != 0 hands the
 * resulting status vector to owgs_update_invokers (the monitor's CurrentInvokerPoolState -> updateInvokers,
 * SCPB:226-227).  Bad kinds, negative ids or times out of order: OWGS_EINVAL with no state change. */
#define OWGS_HEALTH_MAX_ID (1 << 24) /* invoker ids accepted by owgs_health_events (the status vector is dense) */
#define OWGS_EV_PING 0          /* PingMessage (InvokerSupervision.scala:120-131) */
#define OWGS_EV_SUCCESS 1       /* InvocationFinishedMessage(InvocationFinishedResult.Success) */
#define OWGS_EV_SYSTEM_ERROR 2  /* ... SystemError */
#define OWGS_EV_TIMEOUT 3       /* ... Timeout */
#define OWGS_EV_STATE_TIMEOUT 4 /* an FSM.StateTimeout message to the invoker's actor */
int owgs_health_events(owgs_ctx* ctx, int32_t n, const int32_t* invoker, const uint8_t* kind, const int64_t* t_ms,
                       const int64_t* user_memory_bytes, int64_t now_ms, int32_t apply);
/* Replaces: InvokerPool's GetStatus (status vector, InvokerSupervision.scala:132) plus per-invoker detail: userMemory
 * of the instance in the status vector, test actions sent during the last batch (invokeTestAction,
 * InvokerSupervision.scala:416-434), the ring buffer (2 bits per result oldest first: 1 Success, 2 SystemError,
 * 3 Timeout; count << 20) and the next Tick (-1: none).  *n = the status vector's length; any output may be NULL. */
int owgs_health_read(owgs_ctx* ctx, int32_t cap, int32_t* n, uint8_t* status, int64_t* user_memory_bytes,
                     int32_t* test_actions, uint32_t* ring, int64_t* next_tick);

/* ---- supervision feeds: raw pings and ack results drive the FSM ----
 * The two inputs of the health FSM without a host detour.  The events are built on the device from what the ping
 * parser / the completion path left there, in array order (mailbox order), and go through the batch launch of
 * owgs_health_events; no event array is uploaded.
 *
 * out_summary (all three calls): [0] events fed; [1] entries of the status vector (below its new size) whose stored
 * state or userMemory differs from before the call, entries the vector grew by included; [2] test actions this batch
 * sent (the sum of owgs_health_read's test_actions).  The shim reads the vectors only when [1] or [2] is non-zero.
 * apply: 0 hands nothing to owgs_update_invokers; 1 hands the status vector over as owgs_health_events does; 2 hands
 * it over only if out_summary[1] > 0 -- the reference sends CurrentInvokerPoolState only on CurrentState / Transition
 * (ISUP:139-149), and updateInvokers with an unchanged vector changes nothing (SCPB:512-551).  apply = 2 compares
 * with the vector before THIS call: a caller that mixes it with apply = 0 calls hands over late. */

/* Per-message outcome of owgs_process_pings (out_kind): */
#define OWGS_PING_FAIL 0        /* PingMessage.parse fails (ISUP:181-183): the shim logs the raw message */
#define OWGS_PING_UNSUPPORTED 2 /* outside the device parser's limits (the list of OWGS_ACK_UNSUPPORTED): JVM parses */
#define OWGS_PING_FED 3         /* parsed; fed to the FSM as OWGS_EV_PING at t_ms[i] */
#define OWGS_PING_RANGE 4       /* parsed, instance outside [0, OWGS_HEALTH_MAX_ID): reported, not fed */

/* Replaces: InvokerPool.processInvokerPing (ISUP:174-185) for n raw messages of the `health` topic (UTF-8 bytes,
 * offsets off[0..n]) received at t_ms[i]: PingMessage.parse (Message.scala:261-268) on the device, then
 * `self ! p` for every parsed ping (ISUP:120-131).
 * Parse: the whole message must be valid JSON as spray-json 1.3.5 reads it (the scanner and limits of
 * owgs_process_acks).  The root must be an object; the last top-level member whose decoded name is "name" is the
 * InvokerInstanceId (jsonFormat4, InstanceId.scala:31-49), read exactly as the `invoker` member of an ack: instance a
 * JSON number through BigDecimal.intValue; uniqueName / displayedName absent, null or a string; userMemory a string
 * matching (?i)\s?(\d+)\s?(GB|MB|KB|B|G|M|K)\s? with \d = [0-9], \s = [ \t\n\x0B\f\r] and digits that fit a Long
 * (Size.scala:119-138).  A non-object root or no "name" member is OWGS_PING_FAIL.
 * out_user_memory_bytes = size * {1, 2^10, 2^20, 2^30} in wrapping int64 arithmetic (ByteSize.toBytes, Size.scala:
 * 28-62, 166-172): what the shim passes to updateInvokers.  out_instance is written for FED and RANGE; every other
 * output of a message that is not FED is 0.
 * Feed: the FED messages, in array order, are OWGS_EV_PING events (instance, t_ms[i], bytes); the rest drop out.  The
 * time contract is owgs_health_events': t_ms non-decreasing and not before the previous batch's now_ms, now_ms not
 * before the last t_ms, all in [0, 2^60) -- checked over all n entries, whatever they parse to, before anything runs;
 * a violation is OWGS_EINVAL with no state change.  Timers due up to now_ms fire also when nothing is FED.
 * A negative instance makes the reference's actor throw (status(-1), ISUP:125); here it is OWGS_PING_RANGE, as is an
 * instance the dense status vector does not accept.  An UNSUPPORTED ping the JVM parses itself reaches the FSM later,
 * through owgs_health_events at the JVM's current time. */
int owgs_process_pings(owgs_ctx* ctx, int32_t n, const char* bytes, const int64_t* off, const int64_t* t_ms,
                       int64_t now_ms, int32_t apply, uint8_t* out_kind, int32_t* out_instance,
                       int64_t* out_user_memory_bytes, int32_t out_summary[3]);

/* owgs_process_acks / owgs_complete_activations -- outcomes, outputs, releases and books exactly theirs -- followed by
 * `invokerPool ! InvocationFinishedMessage(invoker, result)` (CLB:317, 327) on the device: for each item in array
 * order whose outcome is OWGS_ACK_RELEASED or OWGS_ACK_HEALTH and whose invoker is in [0, OWGS_HEALTH_MAX_ID) one
 * event at time now_ms: OWGS_EV_TIMEOUT if forced (owgs_complete_activations_supervised, flag bit 0), else
 * OWGS_EV_SYSTEM_ERROR if isSystemError, else OWGS_EV_SUCCESS (CLB:266-276).  The invoker is the call's / the
 * message's (CLB:317, 327), not the entry's.  NOENTRY, FORCED_NOENTRY, FAIL, JVM and UNSUPPORTED feed nothing
 * (CLB:328-345); an id without an actor is ignored by the FSM as by InvokerPool (ISUP:135-137).  now_ms before the
 * FSM's last now_ms or outside [0, 2^60) is OWGS_EINVAL before any ack is processed.  A batch that feeds no event
 * leaves the FSM's clock alone, as the expiry sweep does.  Messages reported OWGS_ACK_JVM are completed by the shim
 * through owgs_complete_activations_supervised once the JVM has parsed them (owgs_process_result_acks below completes
 * most of them in the batch itself). */
int owgs_process_acks_supervised(owgs_ctx* ctx, int32_t n, const char* bytes, const int64_t* off, uint8_t* out_kind,
                                 int32_t* out_invoker, int32_t* out_ticket, uint8_t* out_flags, int64_t now_ms,
                                 int32_t apply, int32_t out_summary[3]);
int owgs_complete_activations_supervised(owgs_ctx* ctx, int32_t n, const char* aid32, const int32_t* invoker,
                                         const uint8_t* flags, uint8_t* out_kind, int32_t* out_ticket,
                                         uint8_t* out_flags, int64_t now_ms, int32_t apply, int32_t out_summary[3]);

/* ---- result-carrying acks: CombinedCompletionAndResultMessage and ResultMessage on the device -------------------
 * Completes the dispatch of AcknowledegmentMessage.serdes.read (Message.scala:240-258): owgs_process_acks* hand every
 * message with a `response` member to the JVM (OWGS_ACK_JVM); this call classifies them too, so that a controller
 * serving blocking invokes (ContainerProxy.scala:768-781 sends a Combined message for each unless split acks are
 * configured) needs one device call per ack batch and no ActivationId -> Promise map beside activationSlots. */
#define OWGS_ACK_RESULT 7    /* out_kind: an accepted ResultMessage: processResult only, nothing completed */
#define OWGS_ACKF_RESULT 8   /* out_flags bit3: the message carries a result (processResult runs, CLB:218-220) */
#define OWGS_ACKF_RIGHT 16   /* out_flags bit4: response is a WhiskActivation object (Right); clear: an id (Left) */
typedef struct owgs_ack_out {
    uint8_t* kind; int32_t* invoker; int32_t* ticket; uint8_t* flags;
    uint64_t* aid;        /* 2n words (hi, lo) of acknowledgement.activationId, 0 when not parsed */
    int64_t* resp_off;    /* start of the `response` value in bytes[], 0 when OWGS_ACKF_RESULT is clear */
    int32_t* resp_len;    /* its length in bytes */
} owgs_ack_out;
/* With out_summary != NULL the feed, now_ms, apply and failure atomicity are those of owgs_process_acks_supervised.
 * With out_summary == NULL nothing is fed; now_ms and apply must then be 0, else OWGS_EINVAL.  Argument errors (a NULL
 * out or member with n > 0, offsets out of order, the feed's checks) return before anything runs.
 *
 * Messages are classified in array order, one per message; the grammar, its limits (OWGS_ACK_UNSUPPORTED) and the
 * U+FFFF rule are those of owgs_process_acks.
 *  1. No `response` member: exactly as by owgs_process_acks.  aid = the CompletionMessage's id when it is accepted
 *     (RELEASED / HEALTH / NOENTRY), 0 otherwise.
 *  2. A `response` member (the last top-level member of that name):
 *     - a JSON string is Left(ActivationId) through ActivationId.serdes (ActivationId.scala:58-95) with the rules of
 *       `activationId`: a wrong length or a non-hex character is OWGS_ACK_FAIL, a non-ASCII character
 *       OWGS_ACK_UNSUPPORTED;
 *     - a JSON object is Right(WhiskActivation) only inside the accepted subset below; any other object is
 *       OWGS_ACK_JVM, as from owgs_process_acks: the device never reports an object as FAIL;
 *     - any other value is OWGS_ACK_FAIL (Message.scala:236).
 *  3. With an `invoker` member the message is a CombinedCompletionAndResultMessage (jsonFormat4: transid, response,
 *     isSystemError, invoker; Message.scala:191-193).  transid must be present (TransactionId.serdes.read itself never
 *     fails, TransactionId.scala:243-251), isSystemError is absent, null or a boolean, invoker an InvokerInstanceId as
 *     in a CompletionMessage; health-transid detection is the CompletionMessage's.  A top-level `activationId` is
 *     ignored: the id is the response's (Message.scala:125), the string or the object's `activationId`.  FAIL takes
 *     precedence over UNSUPPORTED, JVM (an object outside the subset) over both.  An accepted Combined message is a
 *     completion: outcome (RELEASED / HEALTH / NOENTRY), release flags, books, timeouts, watch refresh, large-state
 *     branch and health event are exactly those of a CompletionMessage with the same id, invoker, isSystemError and
 *     transid at the same array position.  In addition OWGS_ACKF_RESULT is set, OWGS_ACKF_RIGHT for an object, and
 *     aid, resp_off and resp_len are written.
 *  4. Without an `invoker` member the message is a ResultMessage (jsonFormat2: transid, response; Message.scala:221;
 *     every other member is ignored).  Accepted: out_kind = OWGS_ACK_RESULT, invoker = -1, flags = OWGS_ACKF_RESULT
 *     (| OWGS_ACKF_RIGHT), aid / resp_off / resp_len written; nothing is removed, released, counted or fed.
 *     out_ticket = the ticket of the id's entry if that entry is live at the message's turn -- ready when the batch
 *     starts and removed by no message at a lower index of this batch -- and -1 otherwise.  It is what processResult
 *     (CLB:235-243) needs: a shim that keeps its promises by ticket needs no id map; out_aid covers the -1 cases.
 *
 * Accepted subset of a `response` object -- a sufficient condition for convertTo[WhiskActivation] (jsonFormat13,
 * WhiskActivation.scala:52-64, 182) to succeed, not an exact one; the authoritative list:
 *  - member names: no member name of the object, of its `response` object or of an annotation is written with an
 *    escape; none of the 13 names below occurs twice (nor statusCode / result / size, nor key / value / init inside
 *    their objects); unknown names are ignored (spray-json's product formats read members by name).
 *  - namespace (EntityPath.scala:141-178): a string of bytes 0x20-0x7E without '"' and '\'; split at '/', empty parts
 *    dropped, at least one part left; each part matches EntityName.REGEX (EntityPath.scala:206) with \w =
 *    [A-Za-z0-9_] and is at most 256 characters.
 *  - name (EntityPath.scala:222-234): one such part.
 *  - subject (Subject.scala:46-67 behind ArgNormalizer.apply): the same character class, no leading or trailing
 *    blank, at least 5 characters.
 *  - activationId: a string of 32 characters [0-9a-f], written without escapes.
 *  - cause: absent, null, or such a string.
 *  - start, end (WhiskActivation.scala:161-168): a literal -?(0|[1-9][0-9]{0,17}).
 *  - duration: absent, null, or a literal of that form.
 *  - response (ActivationResult.scala:30-32, 249): an object; statusCode a literal -?(0|[1-9][0-9]{0,8}); size
 *    absent, null or of that form; result any value.
 *  - logs (ActivationLogs.scala:35): an array of strings.
 *  - version (SemVer.scala:52-101): a string matching SemVer.REGEX, each part of at most 9 digits, not "0.0.0".
 *  - publish: true or false.
 *  - annotations (Parameter.scala:240-268): an array of objects; each has exactly one `key`, an unescaped string of
 *    bytes 0x20-0x7E with a non-blank character, exactly one `value` (any), and at most one `init`, a boolean.
 *  - presence: namespace, name, subject, activationId, start, end, response, logs, version, publish and annotations
 *    are all present (spray-json applies no case-class defaults). */
int owgs_process_result_acks(owgs_ctx* ctx, int32_t n, const char* bytes, const int64_t* off,
                             const owgs_ack_out* out, int64_t now_ms, int32_t apply, int32_t out_summary[3]);

/* ---- ActivationMessage serialisation + per-invoker topic fan-out ----
 * Replaces: ActivationMessage.serialize (jsonFormat11 + spray-json compactPrint, Message.scala:51-70, 170-175) and
 * the per-activation producer.send to topic "invoker<N>" (sendActivationToInvoker, CommonLoadBalancer.scala:175-198)
 * for a batch of publishes.  The invariant members are templates printed once per (action, identity) by the caller:
 * part A = the three members `"action":<fqn>,"revision":<rev>,"user":<identity>` (no surrounding commas), part B =
 * the initArgs array value; rootControllerIndex is one JSON value per context.  Templates append; returns the id
 * of the first new one. */
int owgs_register_templates(owgs_ctx* ctx, int32_t n, const char* a_bytes, const int64_t* a_off, const char* b_bytes,
                            const int64_t* b_off, int32_t* out_first_id);
int owgs_set_root_controller(owgs_ctx* ctx, const char* json, int32_t len);

#define OWGS_MSG_BLOCKING 1       /* ActivationMessage.blocking */
#define OWGS_MSG_EXTRA_LOGGING 2  /* transid.meta.extraLogging: ["id", start, true] */
#define OWGS_MSG_HAS_CONTENT 4    /* content = Some(JsObject) (printed, in content/content_off) */
#define OWGS_MSG_HAS_CAUSE 8      /* cause = Some(ActivationId) */
#define OWGS_MSG_HAS_TRACE 16     /* traceContext = Some(Map) (printed, in trace/trace_off) */
typedef struct owgs_msg_batch {
    int32_t n;
    const int32_t* invoker;      /* the publish decisions (owgs_publish_batch out_invoker); < 0: no message */
    const int32_t* tmpl;         /* template id per activation */
    const uint64_t* aid;         /* 2 per activation: the 32 hex digits of ActivationId as (hi, lo) */
    const char* tid;             /* TransactionId.meta.id strings, UTF-8, offsets tid_off[0..n] */
    const int64_t* tid_off;
    const int64_t* tid_start;    /* TransactionId.meta.start, epoch ms */
    const uint8_t* flags;        /* OWGS_MSG_* */
    const char* content;         /* may be NULL when no flag asks for it */
    const int64_t* content_off;
    const uint64_t* cause;       /* 2 per activation */
    const char* trace;
    const int64_t* trace_off;
} owgs_msg_batch;
/* Host buffers.  Output: the m messages (activations with invoker >= 0) grouped by invoker id ascending, publish order
 * within a topic: bytes out[out_off[j] .. out_off[j+1]), out_order[j] = activation index, topic_start[k] ..
 * topic_start[k+1] = the messages of topic "invoker<k>" for k < n_topics.  out_off has n + 1 entries, out_order n,
 * topic_start n_topics + 1.  *total = bytes needed; OWGS_ERANGE (nothing written) when it exceeds cap; OWGS_EINVAL
 * for an invoker >= n_topics, an unknown template or a malformed UTF-8 transaction id. */
int owgs_serialize_activations(owgs_ctx* ctx, const owgs_msg_batch* batch, int32_t n_topics, char* out, int64_t cap,
                               int64_t* out_off, int32_t* out_order, int32_t* topic_start, int64_t* total,
                               int32_t* m);
/* Same with every pointer of batch and the outputs in device memory (e.g. invoker = owgs_replay_device's out_invoker),
 * on `stream`; content_off and trace_off are required (n + 1 zeros when unused); no host-side argument check beyond
 * NULLs (the device flags bad templates / invokers / UTF-8 as above); *total and *m are host values (the call
 * synchronises once). */
int owgs_serialize_activations_device(owgs_ctx* ctx, const owgs_msg_batch* batch, int32_t n_topics, char* out,
                                      int64_t cap, int64_t* out_off, int32_t* out_order, int32_t* topic_start,
                                      int64_t* total, int32_t* m, void* stream);

/* ---- publish end to end: schedule, setupActivation, serialise ----
 * Replaces: ShardingContainerPoolBalancer.publish (SCPB:257-317) for a drained batch -- schedule (SCPB:260-290), then
 * for the activations that got an invoker setupActivation (SCPB:292-304, CLB:116-166) and sendActivationToInvoker
 * (SCPB:302-303, CLB:175-198) -- as one call.  The decisions stay on the device from the engine through the
 * activationSlots table into the serialiser; they come back once, with every other output.
 *
 * Sequential definition.  Item i, in array order:
 *   1. Decision (SCPB:260-290): exactly owgs_publish_batch's for the same action, seq and seq_base.  out_invoker[i]
 *      >= 0, OWGS_NONE or OWGS_THROW_INDEX; out_flags[i] bit 0 the overload flag.
 *   2. Only if out_invoker[i] >= 0 (SCPB:292-304): setupActivation (CLB:116-166), exactly owgs_track_activations_timed
 *      for the item with invoker = out_invoker[i] and now_ms = io->now_ms.  The books count the item whether or not its
 *      id already has an entry (CLB:121-127 run before getOrElseUpdate, CLB:148).  The item that creates the entry
 *      stores namespace, action, ticket and invoker and arms now + max(time_limit, std) * factor + addon (CLB:103-105,
 *      148-152).  A duplicate of an earlier PLACED item of the batch, or of an existing entry, gets that entry's ticket,
 *      out_existed = 1, and arms nothing.  An item without an invoker touches neither the table nor any counter and
 *      cannot be the first tracker of an id (SCPB:305-316 never reach setupActivation): out_ticket = -1, out_existed =
 *      0.  Arm order among the placed items is array order; the context's arm counter advances by n.
 *   3. With msgs: the item's message is written under topic "invoker<out_invoker[i]>" exactly as
 *      owgs_serialize_activations would with invoker = out_invoker; an item without an invoker gets no message.
 * Step 1 never reads what steps 2 and 3 write, so running the stages batch-wise equals running them item by item.
 * Only placed jobs are counted: for callers of this entry point the "assumption" of owgs_throttle_batch /
 * owgs_admit_batch (an admitted job is tracked afterwards) is no longer a hazard -- a job without an invoker is not
 * counted against the later jobs of its namespace once this call has run.
 *
 * The ids are (hi, lo) words (owgs_msg_batch.aid; hi = the first 16 hex digits): the entry is the one a raw ack with
 * the 32-hex id finds and the one owgs_expire_activations reports in out_aid.
 *
 * msgs and mo are both NULL (stages 1 and 2 only) or both set.  With them: msgs->n == io->n; msgs->invoker and
 * msgs->aid must be NULL (the call uses its own decisions and io->aid); everything else as owgs_serialize_activations.
 *
 * out_summary: [0] placed items, [1] entries created, [2] overload fallbacks of managed actions
 * (MANAGED_SYSTEM_OVERLOAD, SCPB:277-286), [3] of blackbox actions (BLACKBOX_SYSTEM_OVERLOAD), [4] items with
 * OWGS_NONE, [5] items with OWGS_THROW_INDEX, [6] stages completed (0, 2 or 3), [7] 0.
 *
 * Failures.  Argument errors are refused before any state changes, the slot state included, with the code of the
 * corresponding call: a NULL among the required pointers (every io pointer but seq and ns; out_summary), n < 0, msgs
 * without mo or mo without msgs, msgs->n != io->n, msgs->invoker or msgs->aid set, now_ms outside [0, 2^60), a time
 * limit outside [0, 2^40) and every host-side check of owgs_serialize_activations: OWGS_EINVAL; an unknown action or
 * namespace handle: OWGS_ENOENT.  n == 0 is OWGS_OK and changes nothing.  An engine error (the codes of
 * owgs_publish_batch) means nothing is tracked and nothing is written.  A failure the message stage finds on the device
 * -- an unknown template, an invoker >= n_topics, a transaction id that is not valid UTF-8 (OWGS_EINVAL), total > cap
 * (OWGS_ERANGE, mo->total set) -- does not undo stages 1 and 2, as the reference's setupActivation precedes a
 * producer.send that may fail (SCPB:302-303; the entry is left to its timeout): the four io outputs and out_summary
 * are valid, out_summary[6] = 2, and the caller serialises again with owgs_serialize_activations(invoker = out_invoker).
 */
typedef struct owgs_publish_io {
    int32_t n;
    const int32_t* action;         /* [n] action handles (owgs_register_actions) */
    const uint64_t* seq;           /* [n] overload-RNG sequence numbers, or NULL: seq_base + i */
    uint64_t seq_base;
    const uint64_t* aid;           /* [2n] ActivationId as (hi, lo), the form of owgs_msg_batch.aid */
    const int32_t* ns;             /* [n] namespace handles or OWGS_NONE; NULL: every item OWGS_NONE */
    const int32_t* ticket;         /* [n] */
    const int64_t* time_limit_ms;  /* [n] action.limits.timeout */
    int64_t now_ms;
    int32_t* out_invoker;          /* as owgs_publish_batch */
    uint8_t* out_flags;            /* as owgs_publish_batch */
    int32_t* out_ticket;           /* as owgs_track_activations_timed; -1 for an item without an invoker */
    uint8_t* out_existed;          /* 0 / 1 as there; 0 for an item without an invoker */
} owgs_publish_io;

typedef struct owgs_msg_out {      /* the outputs of owgs_serialize_activations, host buffers */
    int32_t n_topics;
    char* out;
    int64_t cap;
    int64_t* out_off;
    int32_t* out_order;
    int32_t* topic_start;
    int64_t total;                 /* written by the call */
    int32_t m;
} owgs_msg_out;

int owgs_publish_activations(owgs_ctx* ctx, const owgs_publish_io* io, const owgs_msg_batch* msgs, owgs_msg_out* mo,
                             int64_t out_summary[8]);

/* ---- gated publish: the throttle gate feeds schedule in one call ----
 * Replaces: the two steps every invoke takes -- EntitlementProvider.checkThrottles (Entitlement.scala:197-202, 354-381)
 * and, for what it lets through, ShardingContainerPoolBalancer.publish (PrimitiveActions.scala:152-185, SCPB:257-317)
 * -- for a drained batch, as one call: owgs_admit_batch followed by owgs_publish_activations over the admitted actions,
 * without the verdicts coming back to the host in between.
 *
 * Sequential definition.
 *   1. Gate: out_verdict, out_rate_count, out_rate_limit, out_conc_count, out_conc_limit and the rate records are exactly
 *      what owgs_admit_batch gives for (n, ns, kind, t_ms, rate_override, conc_override), its assumption included: an
 *      admitted action counts against the later actions of its namespace in this batch.
 *   2. Publish: let adm be the indices, in array order, of the items that are actions (kind bit 0 clear) with verdict
 *      OWGS_ADMIT_OK, m = |adm|.  out_invoker, out_flags, out_ticket, out_existed at those indices, the activationSlots
 *      entries, the in-flight books, the armed deadlines and (with msgs) the messages are exactly those of
 *      owgs_publish_activations over the sub-batch action[adm], aid[adm], ns[adm], ticket[adm], time_limit_ms[adm] with
 *      the same now_ms.  The RNG sequence of the k-th admitted action is seq[adm[k]] when seq is given and seq_base + k
 *      otherwise: the rank among the admitted actions, not the array index.  The namespace of the books is the item's
 *      gate namespace.
 *   3. Every other item -- a trigger, a rate-rejected or a concurrent-rejected item -- has out_invoker =
 *      OWGS_NOT_PUBLISHED, out_flags = 0, out_ticket = -1, out_existed = 0.  It touches neither the slot state, the table,
 *      the books nor the messages and cannot be the first tracker of an id; its action, aid, ticket and time_limit_ms
 *      entries are not interpreted (time_limit_ms is still range-checked for every item that is an action).
 * Arm order among the placed items is array order; the context's arm counter advances by n.
 * Messages: msgs is indexed by item, msgs->n == n, msgs->invoker and msgs->aid must be NULL; only placed items produce
 * a message, and out_order holds item indices.
 *
 * The gate's assumption.  An admitted action that gets no invoker (OWGS_NONE, OWGS_THROW_INDEX) is not tracked, yet
 * step 1 has already counted it: conc_count of the later items of its namespace IN THIS BATCH includes it, so such an
 * item may come back OWGS_ADMIT_CONCURRENT where the reference, running item by item, would have admitted it.
 * out_summary[4] + out_summary[5] is the number of admitted actions for which this happened; 0 means the verdicts are
 * the reference's.  The books themselves are exact (only placed items are counted), so the next call starts right.
 *
 * out_summary: [0..7] as owgs_publish_activations ([0] placed, [1] entries created, [2] / [3] overload fallbacks of
 * managed / blackbox actions, [4] admitted actions with OWGS_NONE, [5] with OWGS_THROW_INDEX, [6] stages completed (0,
 * 2 or 3), [7] 0); [8] admitted actions (m); [9] items with verdict OWGS_ADMIT_RATE; [10] items with verdict
 * OWGS_ADMIT_CONCURRENT; [11] triggers with verdict OWGS_ADMIT_OK; [12] how often the call waited on its stream before
 * its outputs were on the host: 1 on an on-chip context (the one block copy: m never comes to the host before it), 2 on
 * a large-state context (the verdicts come back before the engine, whose run takes host arrays).  Not counted, both as
 * in owgs_publish_activations: the waits inside the large-state engine's run and the download of the message bytes,
 * and the rare growth of a table -- the activationSlots rehash, or the NestedSemaphore map's overflow, whose size bound
 * this call advances by n rather than m, so that a context whose batches are mostly rejected reads the exact entry
 * count back (one synchronisation) somewhat earlier than owgs_publish_activations would.  When the engine step fails
 * and the gate outputs are handed out (below), [12] counts the wait that brought them.  [13..15] 0.
 *
 * Failures.  Every argument error of owgs_admit_batch and of owgs_publish_activations is refused before any device
 * state changes -- the rate records included -- with that call's code; the action handle is checked only for items
 * that are actions.  n == 0 is OWGS_OK and changes nothing.  An engine error leaves the rate records charged and the
 * five gate outputs valid (the reference charges the rate before publish can fail); nothing is tracked or written.
 * Any other failure after the gate was queued -- a HIP runtime error (OWGS_EDEVICE) or a failed allocation -- also
 * leaves the rate records charged, but hands out no output at all: the caller reads the records with owgs_rate_state.
 * Failures the message stage finds on the device behave as in owgs_publish_activations: out_summary[6] = 2, the
 * entries stay, and the caller serialises again with owgs_serialize_activations(invoker = out_invoker with the
 * negative values as they are). */
#define OWGS_NOT_PUBLISHED (-3)   /* out_invoker of an item the gate did not hand to publish */
typedef struct owgs_invoke_io {
    int32_t n;
    /* gate inputs, exactly those of owgs_admit_batch */
    const int32_t* ns;
    const uint8_t* kind;
    const int64_t* t_ms;
    const int32_t* rate_override;  /* may be NULL as there */
    const int32_t* conc_override;
    /* publish inputs, exactly those of owgs_publish_io; read only for items that are actions */
    const int32_t* action;
    const uint64_t* seq;           /* [n] by item, or NULL: seq_base + rank among the admitted actions */
    uint64_t seq_base;
    const uint64_t* aid;           /* [2n] */
    const int32_t* ticket;
    const int64_t* time_limit_ms;
    int64_t now_ms;
    /* outputs, all [n] */
    uint8_t* out_verdict;
    int32_t* out_rate_count;
    int32_t* out_rate_limit;
    int32_t* out_conc_count;
    int32_t* out_conc_limit;
    int32_t* out_invoker;
    uint8_t* out_flags;
    int32_t* out_ticket;
    uint8_t* out_existed;
} owgs_invoke_io;

int owgs_invoke_activations(owgs_ctx* ctx, const owgs_invoke_io* io, const owgs_msg_batch* msgs, owgs_msg_out* mo,
                            int64_t out_summary[16]);

/* ---- throttle gate: user-event messages and rejection texts ----
 * Replaces: the two per-item outputs of checkThrottleOverload (Entitlement.scala:383-420) for a drained batch -- the
 * EventMessage it sends to the topic `events` for every admitted action invoke (Metric("ConcurrentInvocations", count
 * + 1)) and for every rejected invoke or fire (Metric(limit.limitName, 1)), and the text the rejected request fails with
 * (limit.errorMsg: ActivationThrottler.scala:58-67, ErrorResponse.scala:70-75).  Both are pure functions of the gate's
 * outputs for the item (owgs_admit_batch, unchanged) and of a timestamp.
 *
 * Setup state of a context, both additive:
 *   - the event source: one printed JSON string value with its quotes, e.g. "controller0"
 *     (s"controller${controllerInstance.asString}", Entitlement.scala:395, 411); unset until owgs_set_event_source.
 *   - event identities, append-only, ids from 0: two opaque byte pieces the caller prints once per Identity with
 *     spray-json (escaping is the caller's): piece A = `"subject":<string>`, piece B =
 *     `"userId":<string>,"namespace":<string>`.  Any length >= 0.
 *
 * Item i, in array order, with S the source, A / B the pieces of ident[i] and ts = ts_ms[i]:
 *   action,  verdict OWGS_ADMIT_OK          event ConcurrentInvocations, value (int64)(int32)(conc_count[i] + 1) -- the
 *                                           reference adds 1 to an Int (wrapping) and then widens; no text
 *   trigger, verdict OWGS_ADMIT_OK          no event (`case _ => // ignore`), no text
 *   verdict OWGS_ADMIT_RATE (either kind)   event TimedRateLimit, value 1; text
 *                                           `Too many requests in the last minute (count: <rate_count>, allowed: <rate_limit>).`
 *   verdict OWGS_ADMIT_CONCURRENT           event ConcurrentRateLimit, value 1; text
 *                                           `Too many concurrent requests in flight (count: <conc_count>, allowed: <conc_limit>).`
 * Event bytes (EventMessage.serialize = format.write(this).compactPrint, Message.scala:404-418):
 *   {"body":{"metricName":"<name>","metricValue":<v>},"eventType":"Metric","source":S,A,"timestamp":<ts>,B}
 * Numbers are plain decimal with a leading '-' when negative; the texts print signed 32-bit values, <v> and <ts> signed
 * 64-bit ones.  Member order: spray-json 1.3.5 builds a JsObject from Map(fields: _*); seven members make a Scala 2.12
 * immutable HashMap, whose iteration order (String.hashCode, improve, 5 bits per trie level from the low end) is body,
 * eventType, source, subject, timestamp, userId, namespace -- the order of the reference's own example
 * (docs/metrics.md:353-364); the two-member body keeps insertion order (Map2).
 * Timestamp: the reference takes System.currentTimeMillis() when it constructs the message, right after the check;
 * here it is ts_ms[i], which the integrated call takes from t_ms[i], the time of the item's check.
 *
 * Outputs are BY ITEM: event i is ev_out[ev_off[i] .. ev_off[i+1]), text i is rej_out[rej_off[i] .. rej_off[i+1]); an
 * item without an event or text has an empty range.  There is one topic, and item order is send order. */
#define OWGS_EVENT_NAME_MAX 21 /* strlen("ConcurrentInvocations"), the longest metric name */
/* The largest event without S, A and B: the literals, the longest name, an int32 value with its sign (the int64 value
 * is a widened int32, or 1) and an int64 timestamp with its sign. */
#define OWGS_EVENT_MAX_FIXED                                                                                         \
    ((int64_t)(sizeof("{\"body\":{\"metricName\":\"\",\"metricValue\":},\"eventType\":\"Metric\",\"source\":,,"      \
                      "\"timestamp\":,}") - 1) + OWGS_EVENT_NAME_MAX + 11 + 20)
/* The largest rejection text: the longer literal and two int32 values with their signs. */
#define OWGS_REJECT_TEXT_MAX \
    ((int64_t)(sizeof("Too many concurrent requests in flight (count: , allowed: ).") - 1) + 11 + 11)
/* So ev_cap = n * (OWGS_EVENT_MAX_FIXED + |S| + max |A| + max |B|) and rej_cap = n * OWGS_REJECT_TEXT_MAX always
 * suffice. */

int owgs_set_event_source(owgs_ctx* ctx, const char* json, int32_t len);
/* Identities append; returns the id of the first new one.  Offsets that do not start at 0 or that decrease:
 * OWGS_EINVAL. */
int owgs_register_event_identities(owgs_ctx* ctx, int32_t n, const char* a_bytes, const int64_t* a_off,
                                   const char* b_bytes, const int64_t* b_off, int32_t* out_first_id);

typedef struct owgs_event_io {
    const int32_t* ident;          /* [n] event identity per item */
    char* ev_out;                  /* host buffers */
    int64_t ev_cap;
    int64_t* ev_off;               /* [n + 1] */
    char* rej_out;
    int64_t rej_cap;
    int64_t* rej_off;              /* [n + 1] */
    int64_t ev_total, rej_total;   /* written by the call: bytes needed */
    int32_t n_events, n_rejects;   /* ... and items with an event / a text */
} owgs_event_io;

/* The pure function above over host arrays (the outputs of owgs_admit_batch, or of an earlier
 * owgs_invoke_activations_events whose event stage was refused for capacity); no state changes.  kind: only bit 0
 * (OWGS_ADMIT_TRIGGER) matters, the override bits are accepted.  rate_count / rate_limit are read for OWGS_ADMIT_RATE
 * items, conc_count for admitted actions and OWGS_ADMIT_CONCURRENT items, conc_limit for the latter.
 * OWGS_EINVAL: a NULL among ctx, ev, and with n > 0 the nine arrays, ev->ident, ev->ev_off, ev->rej_off (ev_out /
 * rej_out may be NULL with a cap of 0); n < 0; a negative cap; the event source not set; a verdict outside 0..2; a
 * reserved kind bit.  OWGS_ENOENT: an ident[i] outside the registered range (every item is checked, whether or not it
 * has an event).  n == 0 is OWGS_OK with totals 0.
 * Capacity: ev_total > ev_cap or rej_total > rej_cap leaves THAT region (its bytes) untouched, the other region is still
 * written; both offset arrays, both totals and both counts are set, and the call returns OWGS_ERANGE. */
int owgs_throttle_events(owgs_ctx* ctx, int32_t n, const uint8_t* kind, const uint8_t* verdict,
                         const int32_t* rate_count, const int32_t* rate_limit, const int32_t* conc_count,
                         const int32_t* conc_limit, const int64_t* ts_ms, owgs_event_io* ev);

/* owgs_invoke_activations -- everything it does and returns, unchanged -- plus the events and texts of the batch, built
 * on the device from the gate's outputs (ts = io->t_ms) right after the gate; the two offset arrays, totals and counts
 * come back in the call's one block copy, the bytes are downloaded like the message bytes (not counted in [12]).
 * ev == NULL behaves exactly as owgs_invoke_activations.
 * out_summary: [0..12] as owgs_invoke_activations; [13] events written, [14] rejection texts written (each 0 when its
 * region was refused); [15] the event stage: 0 not asked, 1 done, 2 refused for capacity.
 * Failures: every argument error of owgs_invoke_activations and of owgs_throttle_events' ev (NULLs, a negative cap, the
 * source not set: OWGS_EINVAL; an unknown ident[i]: OWGS_ENOENT) is refused before any state changes, the rate records
 * included.  A region over its cap is left untouched and the other is written, as in owgs_throttle_events: [15] = 2 and
 * OWGS_ERANGE, while every gate and publish output is valid and every state change stands; the caller repeats only
 * owgs_throttle_events with larger buffers.  If the message stage fails too its code wins; [6] and [15] carry both
 * facts.  When the engine step fails and only the gate outputs are handed out, the events are handed out with them. */
int owgs_invoke_activations_events(owgs_ctx* ctx, const owgs_invoke_io* io, const owgs_msg_batch* msgs,
                                   owgs_msg_out* mo, owgs_event_io* ev, int64_t out_summary[16]);

/* Duration of the last owgs_engine_kernel launch (HIP events recorded on its stream right before and after it);
 * waits for it to finish.  Measurement hook for bench.py's roofline. */
int owgs_engine_ms(owgs_ctx* ctx, float* ms);

/* Diagnostics (leak tests): what the library holds in this process, over every context: out[0] device allocations,
 * [1] pinned host blocks, [2] events and streams it created.  All three are back at their earlier values once the
 * contexts created since have been destroyed.  No device work; needs no context. */
int owgs_live_resources(int64_t out[3]);

/* Counters of owgs_process_batch's two paths: out[0] calls the resident engine served, [1] its launches, [2] calls it
 * refused untouched (a release that could leave the on-chip permit range; the chain took them), [3] calls the launch
 * chain took, [4] 1 while a resident engine is live; then, summed over the served calls: [5] walk rounds, [6]
 * decisions, [7] staging cycles, [8] release cycles, [9] publish cycles, [10] overflow lookups, [11] walks that
 * started at a cursor, [12] walks skipped by the pool permit bound, [13] decisions committed from speculative walks,
 * [14] validation passes, [15] decisions decided alone, [16] their cycles, [17] speculation cycles, [18] validation
 * cycles (the decisions decided alone included), [19..23] cycles of the speculation's rank matching, plain walks and
 * concurrent walks, of the validation's map inserts and of the releases' concurrent part; [24] chunks whose
 * concurrent decisions the helper wave speculated while wave 0 finished the chunk before, [25] the helper wave's
 * cycles in its concurrent walks; [26] the duration in ns of the last owgs_publish_batch / owgs_release_batch /
 * owgs_process_batch call, entry to return, timed inside the library; [27] 1 when the last owgs_replay /
 * owgs_replay_device(_span) ran through the resident engine's stream mode (OWGS_SPEC_REPLAY), [28..48] that replay's
 * counters [5..25] summed over its launch (waits for the context's stream, not for a live resident engine); [49],
 * [50] the largest primary-table fill (live + deleted entries) and deleted entries after a served call; [51], [52]
 * host nanoseconds over the served calls: building the call (records, chunk ranks), bell to answer; [53] launches
 * that ended at the engine's lifetime bound (OWGS_RES_LIFE_US, default 100 ms: it exits between calls so that
 * launches of other streams sharing its hardware queue are not held back); [54] served calls while watched pairs
 * existed (after owgs_update_cluster with activations in flight).  Returns the number of counters (55). */
int owgs_resident_stats(owgs_ctx* ctx, int64_t* out, int32_t cap);

/* Which path of the large-state engine (a pool beyond owgs_limits, or a maxConcurrent beyond
 * 4095) decided what.  Totals since the context was created, summed on the host after every launch (no device work
 * here): out[0] decisions kept from a group's speculation, [1] decisions decided alone (the two owgs_read_stats also
 * reports, below); then out[0] split by branch: [2] plain (maxConcurrent == 1) and [3] concurrent decisions kept
 * inside a run committed at once, [4] plain and [5] concurrent decisions kept one at a time in queue order, [6]
 * speculated walks that fail everywhere and were forced (SCPB:417-424) -- [0] == [2] + ... + [6]; [7] decisions that
 * had a speculation but were decided alone (it no longer held at their turn, or an earlier decision of their action
 * / key was decided alone; counted in [1] too); [8] None outcomes of an empty pool (SCPB:288-290) and [9]
 * IndexOutOfBounds outcomes (SCPB:266-268), counted in neither [0] nor [1] -- every publish is in exactly one of
 * [2..6], [1], [8], [9]; [10] groups of up to 64 releases whose plain releases were applied at once, [11] groups
 * applied in queue order (a permit count could leave the int range, FS:48-50); [12] launches of the engine, [13]
 * launches that stopped for the NestedSemaphore map to grow and were resumed.  Returns the number of counters (14),
 * or 0 with nothing written while the context runs on the on-chip engines. */
int owgs_large_stats(owgs_ctx* ctx, int64_t* out, int32_t cap);

/* Restore the slot state captured by owgs_snapshot (bench: every timed step starts from the same state). */
int owgs_snapshot(owgs_ctx* ctx);
int owgs_restore(owgs_ctx* ctx, void* stream);

/* Health all-gather hook (RCCL over xGMI, done by the caller): overwrite the status vector from a device buffer of
 * n bytes (InvokerState codes), e.g. the rank-0 row of an all_gather of CurrentInvokerPoolState.  Asynchronous on
 * `stream` for identity pools (the status bytes are copied and the usable bitmap rebuilt there; status_dev must stay
 * valid until `stream` reaches the copy); later calls on any stream see the new health (see Conventions). */
int owgs_update_health_device(owgs_ctx* ctx, int32_t n, const uint8_t* status_dev, void* stream);

/* Device self-test of the engine's wave primitives (DPP scans/reductions vs a serial computation); 0 = pass. */
int owgs_selftest(owgs_ctx* ctx);

/* Engine counters of the last engine launch (diagnostics): [0] resolution passes, [1] walk probes, [2] overload
 * fallbacks, [3] wave-cooperative long walks, [4] chunks, [5] passes that stopped before the chunk end,
 * [31] lanes re-decided inside their pass; [32] NestedSemaphore entries, absent when their lanes speculated, that the
 * I/O wave found or inserted ahead of the commit, [33] committing lanes that found or inserted theirs themselves
 * (the entry pre-find); [8..15] per-phase shader cycles in the diagnostic build
 * (libowgs_prof.so).  On a context that runs on the large-state engine the slots [40..43] (cycles of its releases,
 * group speculation, kept decisions, decisions decided alone) and [46], [47] (decisions kept from the speculation /
 * decided alone) are not the last launch's: they are totals since the context was created (owgs_large_stats). */
int owgs_read_stats(owgs_ctx* ctx, uint64_t* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
