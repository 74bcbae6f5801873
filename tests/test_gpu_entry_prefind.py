"""The engine's entry pre-find (openwhisk_amd/csrc/owgs_kernels.hip): lanes whose NestedSemaphore entry
was absent when they speculated queue its key, the I/O wave finds or inserts it during validation, and the commit
stores the new value at the index it left.  An entry inserted for a lane that does not commit stays a zero-valued
placeholder, which must read as absent everywhere and never leave a launch.

Every case is bit-exact against the oracle on the assignment vector, the decision flags, the release flags and the
final permits, and takes a few seconds at most.  The workloads are those of entry_prefind_cases.py;
test_entry_prefind_inputs.py shows on the CPU that each still meets the condition it is here for."""
import numpy as np
import pytest

import entry_prefind_cases as PC
import oracle as O
from openwhisk_amd import GpuShardingContainerPoolBalancer
from openwhisk_amd import workload as W

pytestmark = pytest.mark.gpu


def gpu_for(w):
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, w.inv_status)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    return b


def check(w, b=None, st=None):
    st = st or O.state_for(w)
    o_inv, o_fl, o_rf = st.replay(w.stream)
    b = b or gpu_for(w)
    g_inv, g_fl, g_rf = b.replay(w.stream)
    bad = np.nonzero(o_inv != g_inv)[0]
    assert len(bad) == 0, f"first mismatch at {bad[:5]} oracle={o_inv[bad[:5]]} gpu={g_inv[bad[:5]]}"
    assert np.array_equal(o_fl, g_fl)
    assert np.array_equal(o_rf, g_rf)
    assert np.array_equal(st.permits(), b.permits())
    return b, o_inv


def check_case(name):
    """A case of entry_prefind_cases.py against its (shared) oracle run."""
    w = PC.workload(name)
    o_perm, o_inv, o_fl, o_rf = PC.oracle_run(name)
    b = gpu_for(w)
    g_inv, g_fl, g_rf = b.replay(w.stream)
    bad = np.nonzero(o_inv != g_inv)[0]
    assert len(bad) == 0, f"first mismatch at {bad[:5]} oracle={o_inv[bad[:5]]} gpu={g_inv[bad[:5]]}"
    assert np.array_equal(o_fl, g_fl)
    assert np.array_equal(o_rf, g_rf)
    assert np.array_equal(o_perm, b.permits())
    assert b.large_stats() is None
    return b


def test_many_keys_cap_and_lane_path():
    # A: over 64 absent-entry lanes in every chunk -- the I/O wave takes its round, the rest find or insert themselves
    b = check_case("A")
    es = b.entry_stats()
    print(es)
    assert es["prefound"] > 0 and es["lane_found"] > 0, es


def test_one_key_many_lanes():
    # B: dozens of lanes of a chunk on one absent key -- equal keys in one round of the I/O wave (CAS losers rescan)
    b = check_case("B")
    es = b.entry_stats()
    print(es)
    assert es["prefound"] > 0, es


def test_table_beyond_its_fill():
    # C: more live entries than the on-chip table takes -- the fill gate, the overflow table (pre-find off while it
    # holds entries) and a rebuild with placeholders around
    b = check_case("C")
    print(b.entry_stats())


def test_stops_and_forced_acquires():
    # D: lanes behind a stop speculate again elsewhere and leave placeholders; forced acquires write their entries
    b = check_case("D")
    print(b.entry_stats(), b.stats())
    assert b.stats()["stops"] > 0


def test_second_replay_and_resident_call_after_placeholders():
    # after case A's stream: a second stream on the same context without restore, then one owgs_process_batch call
    # of 64 jobs (32 releases, 32 publishes) -- both read the table the first launch wrote back (placeholders leave a
    # launch as deleted entries), against the oracle continuing from the same state
    w = PC.workload("A")
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, w.inv_status)
    b.update_cluster(w.cluster_size)
    gh, _ = b.register_actions(w.actions)
    st = O.BalancerState(w.managed_fraction, w.blackbox_fraction, rng_seed=w.rng_seed, zombies=True)
    st.update_invokers(w.inv_ids, w.inv_mem, w.inv_status)
    keys = {}
    oh = [st.register_action(a.namespace, a.path, keys.setdefault(a.key, len(keys)), a.mem_mb, a.max_concurrent,
                             a.blackbox) for a in w.actions]
    check(w, b, st)
    assert b.entry_stats()["prefound"] > 0
    w2 = W.config(PC.CASES["A"][0], shard=1, **PC.CASES["A"][1])  # (the same cluster and actions, another stream)
    assert [a.key for a in w2.actions] == [a.key for a in w.actions] and not np.array_equal(w2.stream.act, w.stream.act)
    _, o_inv2 = check(w2, b, st)
    # the shim's call: completions of 32 activations of the second stream that it left in flight, then 32 publishes
    s2 = w2.stream
    flying = np.setdiff1d(np.nonzero(o_inv2 >= 0)[0], s2.rel_aid)[:32]
    assert len(flying) == 32
    ri = [int(o_inv2[i]) for i in flying]
    pubs = [int(a) for a in w.stream.act[:32]]
    seq = 2 * len(s2.act)
    o_rf = [O._rel_bits(st.release(x, oh[s2.act[i]])) for x, i in zip(ri, flying)]
    o_dec = [st.publish(oh[a], seq + k) for k, a in enumerate(pubs)]
    gi, gf, grf = b.process_batch([0, 32], ri, [int(gh[s2.act[i]]) for i in flying], [0, 32],
                                  [int(gh[a]) for a in pubs], seq_base=seq)
    assert grf.tolist() == o_rf
    assert [(int(x), int(f)) for x, f in zip(gi, gf)] == [(int(x), int(f)) for x, f in o_dec]
    assert np.array_equal(st.permits(), b.permits())


def test_narrow_geometry():
    # 12,007 invokers (over the wide geometry's 11,656 ids): the 7 x 32 geometry compiles the same body
    w = W.config("headline", n_invokers=12_007, n_activations=30_000, user_memory_mb=1024, mem_choices=(128, 256),
                 conc_frac=1.0, conc_range=(2, 4), n_actions=4000, n_namespaces=50, zipf_s=0.0, unhealthy_frac=0.0,
                 delay_mean=1.5, load=1.0)
    b, _ = check(w)
    assert b.large_stats() is None  # (an on-chip engine ran it)
    es = b.entry_stats()
    print(es)
    assert es["prefound"] > 0, es


def test_multi_shard_launch():
    # two shards of case A's cluster in one launch: the multi-shard kernel's bodies
    import torch

    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    shards = []
    for g in (0, 1):
        w = W.config("headline", shard=g, n_shards=2, **dict(PC.CASES["A"][1], n_activations=4000,
                                                             user_memory_mb=8192))
        b = gpu_for(w)
        s = w.stream
        d = [t(s.acq_off, np.int64), t(s.act, np.int32), t(s.rel_off, np.int64),
             t(s.rel_aid if len(s.rel_aid) else np.zeros(1), np.int64),
             torch.empty(len(s.act), dtype=torch.int32, device=dev),
             torch.empty(len(s.act), dtype=torch.uint8, device=dev),
             torch.zeros(max(len(s.rel_aid), 1), dtype=torch.uint8, device=dev)]
        io = (s.n_batches, d[0].data_ptr(), d[1].data_ptr(), len(s.act), d[2].data_ptr(), d[3].data_ptr(),
              len(s.rel_aid), s.seq_base, d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr())
        shards.append((w, b, d, io))
    GpuShardingContainerPoolBalancer.replay_device_multi([(b, io) for _, b, _, io in shards])
    torch.cuda.synchronize()
    for w, b, d, _ in shards:
        st = O.state_for(w)
        o_inv, o_fl, o_rf = st.replay(w.stream)
        assert np.array_equal(o_inv, d[4].cpu().numpy())
        assert np.array_equal(o_fl, d[5].cpu().numpy())
        assert np.array_equal(o_rf, d[6].cpu().numpy()[: len(o_rf)])
        assert np.array_equal(st.permits(), b.permits())


def test_group_replay_with_health_rows():
    # the batches of case A's pool in one engine launch, each with its own health row
    import torch
    from openwhisk_amd import cluster

    w = W.config("headline", **dict(PC.CASES["A"][1], n_activations=4000, batch=1000))
    s = w.stream
    sched = cluster.health_schedule(w.inv_status, s.n_batches, churn=0.05)
    b = gpu_for(w)
    st = O.state_for(w)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    d_act, d_aid = t(s.act, np.int32), t(s.rel_aid, np.int64)
    d_out = torch.full((len(s.act),), -9, dtype=torch.int32, device=dev)
    d_fl = torch.zeros(len(s.act), dtype=torch.uint8, device=dev)
    d_rf = torch.zeros(max(len(s.rel_aid), 1), dtype=torch.uint8, device=dev)
    nid = len(w.inv_status)
    d_h = t(np.stack(sched), np.uint8)
    b.replay_device_group(s.acq_off, s.rel_off, d_act.data_ptr(), d_aid.data_ptr(), s.seq_base, d_out.data_ptr(),
                          d_fl.data_ptr(), d_rf.data_ptr(), d_h.data_ptr(), nid, nid)
    torch.cuda.synchronize()
    o_inv, o_fl, o_rf = O.replay_with_health(st, s, w.inv_ids, w.inv_mem, sched)
    assert np.array_equal(d_out.cpu().numpy(), o_inv)
    assert np.array_equal(d_fl.cpu().numpy(), o_fl)
    assert np.array_equal(d_rf.cpu().numpy()[: len(s.rel_aid)], o_rf)
    assert np.array_equal(b.permits(), st.permits())
