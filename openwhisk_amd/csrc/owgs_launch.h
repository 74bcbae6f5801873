// owgs_launch.h -- the launch wrappers the .hip files define and the host runtime calls (C linkage).  Included by
// both sides: a definition whose parameters disagree with its declaration here does not compile, where the linker
// alone would only have compared names.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "owgs_internal.h"

extern "C" hipError_t owgs_launch_hash(const OwgsHashArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_lookup(const OwgsLookupArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_selftest(int* bad, int trials, hipStream_t s);
extern "C" hipError_t owgs_launch_prepare(const OwgsPrepArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_prepass(const OwgsPrepassArgs* a, int32_t* cstart, int64_t max_chunks,
                                          hipStream_t s);
extern "C" hipError_t owgs_launch_ovf_clear(const OwgsOvf* O, hipStream_t s);
extern "C" hipError_t owgs_launch_ovf_rehash(const uint2* old_t, int32_t old_cap, const OwgsOvf* O, int32_t* err,
                                            hipStream_t s);
extern "C" hipError_t owgs_launch_relpos(const OwgsRelposArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_relflags(const int64_t* rel_aid, int64_t n_rel, const int32_t* out_inv,
                                           uint8_t* rel_flags, hipStream_t s);
extern "C" hipError_t owgs_launch_release_seq(const OwgsReleaseArgs* a, hipStream_t s);
extern "C" size_t owgs_release_scratch_bytes(int32_t n);
extern "C" hipError_t owgs_launch_engine(const OwgsEngineArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_engine_multi(const OwgsEngineArgs* a, int k, hipStream_t s);
extern "C" hipError_t owgs_launch_engine_multi_dev(const OwgsEngineArgs* a_host, const OwgsEngineArgs* a_dev, int k,
                                                   hipStream_t s);
extern "C" int32_t owgs_coprime_max(void);
extern "C" hipError_t owgs_launch_coprime(const int32_t* xs, int32_t n_pools, int32_t* out, int32_t out_stride,
                                          int32_t* counts, hipStream_t s);
extern "C" hipError_t owgs_launch_slots(const int64_t* mem_bytes, int32_t from, int32_t n, int32_t cluster,
                                       int64_t min_bytes, int32_t* permits, hipStream_t s);
extern "C" hipError_t owgs_launch_seq(const OwgsSeqArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_seq_rehash(const uint4* old, int32_t old_cap, const OwgsSeqArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_seq_migrate(const uint32_t* ct_keys, const uint32_t* ct_vals, int32_t n_ct,
                                              const uint2* ovf, int32_t ovf_cap, const uint32_t* w_keys,
                                              const uint32_t* w_vals, int32_t w_cap, const OwgsSeqArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_seq_lookup(const OwgsSeqArgs* a, int32_t inv, int32_t slot, int32_t* out, hipStream_t s);
extern "C" hipError_t owgs_launch_usable_rows(const uint8_t* status, int64_t stride, int32_t n, int32_t rows,
                                              uint32_t* bits, int32_t n_words, hipStream_t s);
extern "C" hipError_t owgs_launch_usable(const uint8_t* status, int32_t n, uint32_t* bits, int32_t n_words,
                                        hipStream_t s);
extern "C" hipError_t owgs_launch_slot_scan(const uint32_t* ct_keys, const uint2* ovf, int32_t ovf_cap,
                                           const uint32_t* w_keys, int32_t w_cap, const int32_t* wkey, uint32_t* cand,
                                           hipStream_t s);
extern "C" hipError_t owgs_launch_ack_parse(const OwgsAckParseArgs* a, hipStream_t st);
extern "C" hipError_t owgs_launch_aid_decode(const char* aid32, int32_t n, const uint8_t* cflags, ulonglong2* key,
                                             uint8_t* info, int32_t* inst, const int32_t* inv, hipStream_t st);
extern "C" hipError_t owgs_launch_act_init(const OwgsActTable* T, hipStream_t st);
extern "C" hipError_t owgs_launch_act_rehash(const OwgsActTable* O, const OwgsActTable* T, hipStream_t st);
extern "C" hipError_t owgs_launch_act_track(const OwgsActTable* T, const ulonglong2* key, int32_t n,
                                            const int32_t* action, const int32_t* ns, const int32_t* ticket,
                                            int32_t* slot, uint8_t* state, int32_t* out_ticket, uint8_t* out_existed,
                                            unsigned long long* counters, const OwgsInflight* F, const OwgsArm* arm,
                                            const uint8_t* placed, hipStream_t st);
extern "C" hipError_t owgs_launch_publish_gate(const OwgsPublishGate* g, hipStream_t st);
extern "C" hipError_t owgs_launch_publish_collect(unsigned long long* hdr, const int32_t* bad,
                                                  const int32_t* topic_start, int32_t n_topics,
                                                  const int64_t* out_off, int32_t n, hipStream_t st);
extern "C" hipError_t owgs_launch_expire_scan(const OwgsExpireArgs* a, hipStream_t st);
extern "C" size_t owgs_expire_sort_bytes(int32_t n);
extern "C" hipError_t owgs_launch_expire_order(const OwgsExpireArgs* a, int32_t n, int32_t take, int32_t seq_bits,
                                               void* temp, size_t temp_bytes, int32_t* idx0, int32_t* idx1,
                                               unsigned long long* key, unsigned long long* key_s, ulonglong2* key_out,
                                               int32_t* inst, uint8_t* info, long long* out_deadline, hipStream_t st);
extern "C" hipError_t owgs_launch_deadline_min(const OwgsActTable* T, long long* out, hipStream_t st);
extern "C" hipError_t owgs_launch_ns_gather(const int32_t* active, const int32_t* ns, int32_t n, int32_t* out,
                                            hipStream_t st);
extern "C" size_t owgs_throttle_sort_bytes(int32_t n, int32_t bits);
extern "C" hipError_t owgs_launch_throttle(const int32_t* ns, const int32_t* limit, int32_t n, int32_t bits,
                                           void* temp, size_t temp_bytes, int32_t* key_out, int32_t* idx_in,
                                           int32_t* idx_out, const int32_t* active, int32_t* out_count,
                                           uint8_t* out_ok, hipStream_t st);
extern "C" hipError_t owgs_launch_admit(const int32_t* ns, int32_t bits, void* temp, size_t temp_bytes,
                                        int32_t* key_out, int32_t* idx_in, int32_t* idx_out, const OwgsAdmitArgs* args,
                                        hipStream_t st);
extern "C" hipError_t owgs_launch_rate_gather(const long long* rate_min, const int32_t* rate_cnt, int32_t ns_cap,
                                              int32_t which, const int32_t* ns, int32_t n, long long* out_min,
                                              int32_t* out_cnt, hipStream_t st);
extern "C" hipError_t owgs_launch_rate_grow(const long long* old_min, const int32_t* old_cnt, int32_t old_cap,
                                            long long* new_min, int32_t* new_cnt, int32_t new_cap, hipStream_t st);
extern "C" hipError_t owgs_launch_ack_complete(const OwgsActTable* T, const OwgsAckCompleteArgs* a, hipStream_t st);
extern "C" hipError_t owgs_launch_ack_flags(int32_t n, const uint8_t* info, const uint8_t* rflags,
                                            const uint8_t* out_kind, uint8_t* out_flags, const ulonglong2* key,
                                            unsigned long long* out_aid, hipStream_t st);
extern "C" hipError_t owgs_launch_ack_parse_results(const OwgsAckParseResultArgs* a, hipStream_t st);
extern "C" hipError_t owgs_launch_health_init(uint8_t* s, uint32_t* ring, int64_t* last, int64_t* tick, int64_t* mem,
                                              int32_t* tests, int32_t from, int32_t to, hipStream_t st);
extern "C" size_t owgs_health_sort_bytes(int32_t n, int32_t bits);
extern "C" hipError_t owgs_launch_health_batch(const int32_t* ev_inv, const uint8_t* ev_kind, const int64_t* ev_t,
                                               const int64_t* ev_mem, int32_t n, int32_t bits, void* temp,
                                               size_t temp_bytes, int32_t* key_out, int32_t* idx_in,
                                               int32_t* idx_out, int64_t* packed, int32_t* seg_beg, int32_t* seg_end,
                                               int32_t* reg_first, int32_t* pad_src, uint8_t* s, uint32_t* ring,
                                               int64_t* last, int64_t* tick, int64_t* mem, int32_t* tests,
                                               int32_t old_size, int32_t new_size, int64_t now, int32_t* sum,
                                               hipStream_t st);
extern "C" hipError_t owgs_launch_ping_parse(const uint8_t* bytes, const int64_t* off, int32_t n, uint8_t* out_kind,
                                             int32_t* out_inst, long long* out_mem, hipStream_t st);
extern "C" hipError_t owgs_launch_feed_compact(const OwgsFeedArgs* a, int mode, hipStream_t st);
extern "C" size_t owgs_msg_scratch_bytes(int32_t n, int32_t n_topics, int32_t bits);
extern "C" hipError_t owgs_launch_msg_plan(const OwgsMsgArgs* a, int32_t bits, void* temp, size_t temp_bytes,
                                           uint32_t* key_sorted, int32_t* iota, int64_t* len_sorted, int32_t* cnt,
                                           hipStream_t st);
extern "C" hipError_t owgs_launch_msg_write(const OwgsMsgArgs* a, hipStream_t st);
extern "C" size_t owgs_event_scratch_bytes(int32_t n);
extern "C" hipError_t owgs_launch_events(const OwgsEventArgs* a, void* temp, size_t temp_bytes, hipStream_t st);
extern "C" size_t owgs_engine_lds_bytes(int n_slots, int pool_mode, int n_ids, int nm, int nb, int n_actions);
// the narrow geometry (owgs_engine_narrow.hip): same ABI, 7 x 32-lane chunks
extern "C" size_t owgs_engine_lds_bytes_narrow(int n_slots, int pool_mode, int n_ids, int nm, int nb, int n_actions);
extern "C" hipError_t owgs_launch_prepass_narrow(const OwgsPrepassArgs* a, int32_t* cstart, int64_t max_chunks,
                                                 hipStream_t s);
extern "C" hipError_t owgs_launch_engine_narrow(const OwgsEngineArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_engine_multi_narrow(const OwgsEngineArgs* a, int k, hipStream_t s);
extern "C" hipError_t owgs_launch_engine_multi_dev_narrow(const OwgsEngineArgs* a_host, const OwgsEngineArgs* a_dev,
                                                          int k, hipStream_t s);
#define OWGS_WL_NARROW (OWGS_EW * 32)
extern "C" hipError_t owgs_launch_w_rebuild(const OwgsWRebuildArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_stage_releases(const OwgsStageArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_relmeta(int32_t n, const int32_t* act, const int32_t* act_mem,
                                          const int32_t* act_maxc, const int32_t* act_slot, int32_t* mem,
                                          int32_t* maxc, int32_t* slot, hipStream_t s);
extern "C" hipError_t owgs_launch_w_update(const OwgsWUpdateArgs* a, hipStream_t s);
extern "C" hipError_t owgs_launch_invoke_compact(const OwgsInvokeCompact* a, hipStream_t st);
extern "C" hipError_t owgs_launch_invoke_gate(const OwgsInvokeGate* g, hipStream_t st);
extern "C" size_t owgs_resident_image_bytes(int32_t n_slots, int32_t n_ids);
extern "C" hipError_t owgs_launch_resident(const OwgsResArgs* a, size_t lds_bytes, hipStream_t s);
extern "C" hipError_t owgs_launch_w_relgather(const int64_t* rel_aid, int32_t n, const int32_t* out_inv,
                                              const int32_t* act, const int32_t* act_mem, const int32_t* act_maxc,
                                              const int32_t* act_slot, int32_t* inv, int32_t* mem, int32_t* maxc,
                                              int32_t* slot, hipStream_t s);
