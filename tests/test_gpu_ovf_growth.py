"""The concurrency map's HBM overflow across calls on one context (openwhisk_amd/csrc/owgs_host.cpp: ensure_ovf's
growth path with owgs_ovf_rehash_kernel, the entry-count bound and its probes, restore_impl over a captured overflow,
reset_ctab on a filled one, and growth inside a multi-shard launch).  Every other test that reaches the overflow
replays once on a fresh context: the table is allocated empty and keeps its size.

Every case runs one sequence of calls on a context and on one oracle state and is bit-exact after each call on the
assignment vector, the decision flags, the release flags and the permits; at its end NestedSemaphore.concurrentState
of a seeded sample of 200 invokers x 40 keys agrees too, with at least one entry present.  The streams are those of
ovf_growth_cases.py; test_ovf_growth_inputs.py shows on the CPU what each of them reaches."""
import time

import numpy as np
import pytest

import ovf_growth_cases as G
from openwhisk_amd import GpuShardingContainerPoolBalancer

pytestmark = pytest.mark.gpu


def gpu_for(w):
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, w.inv_status)
    b.update_cluster(w.cluster_size)
    gh, _ = b.register_actions(w.actions)
    assert np.array_equal(gh, np.arange(len(w.actions)))  # (a stream's action indices are the context's handles)
    return b


def fill(b):
    """map_fill() of a context on the on-chip engine."""
    assert b.large_stats() is None
    f = b.map_fill()
    assert 0 <= f["primary_live"] + f["primary_deleted"] <= G.OWGS_CTC
    assert 0 <= f["overflow_entries"] <= f["overflow_cap"]
    return f


def same(got, want, what):
    """One call's three arrays and the permits after it against the oracle's step."""
    o_inv, o_fl, o_rf, o_perm, _ = want
    g_inv, g_fl, g_rf, g_perm = got
    bad = np.nonzero(o_inv != g_inv)[0]
    assert len(bad) == 0, f"{what}: first mismatch at {bad[:5]} oracle={o_inv[bad[:5]]} gpu={g_inv[bad[:5]]}"
    assert np.array_equal(o_fl, g_fl), what
    assert np.array_equal(o_rf, g_rf[: len(o_rf)]), what
    assert np.array_equal(o_perm, g_perm), what


def call(b, stream):
    t0 = time.perf_counter()
    got = (*b.replay(stream), b.permits())
    print(f"replay of {len(stream.act)} activations: {time.perf_counter() - t0:.2f} s")
    return got


def same_entries(b, st):
    sl = st.invoker_slots
    present = 0
    for inv, k in G.sample_pairs(len(sl), G.n_keys(G.s1())):
        o = sl[inv].concurrent_state(k)
        g = b.concurrent_state(inv, k)
        assert o == g, (inv, k, o, g)
        present += o is not None
    assert present > 0


def same_permanent_entries(b, st):
    """Every entry S1 leaves for good, one by one: a table that was rebuilt elsewhere has to hold each of them with
    the oracle's value (the calls of this file never release them, and need not walk to them)."""
    sl = st.invoker_slots
    for inv, k in G.s1_live_pairs():
        o = sl[inv].concurrent_state(k)
        g = b.concurrent_state(inv, k)
        assert o is not None and o == g, (inv, k, o, g)


def after_s1():
    """A fresh context that replayed S1: entries in the overflow, its capacity, S2 for that capacity."""
    b = gpu_for(G.s1())
    same(call(b, G.s1().stream), G.oracle_run(("S1",))[0][0], "S1")
    f = fill(b)
    assert f["overflow_entries"] > 0, f
    cap0 = f["overflow_cap"]
    assert cap0 >= 1 << 19 and cap0 & (cap0 - 1) == 0
    w2 = G.s2(cap0)
    assert w2.actions == G.s1().actions
    assert G.ovf_need(0, len(w2.stream.act)) == 2 * cap0  # no entry count lets this call fit
    return b, cap0, w2


def device_io(s, dev):
    """A stream's arrays on the device and the tuple replay_device_multi takes."""
    import torch

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    d = [t(s.acq_off, np.int64), t(s.act, np.int32), t(s.rel_off, np.int64),
         t(s.rel_aid if len(s.rel_aid) else np.zeros(1), np.int64),
         torch.full((len(s.act),), -9, dtype=torch.int32, device=dev),
         torch.zeros(len(s.act), dtype=torch.uint8, device=dev),
         torch.zeros(max(len(s.rel_aid), 1), dtype=torch.uint8, device=dev)]
    io = (s.n_batches, d[0].data_ptr(), d[1].data_ptr(), len(s.act), d[2].data_ptr(), d[3].data_ptr(), len(s.rel_aid),
          s.seq_base, d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr())
    return d, io


def test_growth_with_live_entries():
    # A: the second call cannot fit the table the first one left entries in -- exact count, a table twice as large,
    # every live entry rehashed into it, then S2's 25 batches release and acquire on the grown table.  S2 need not
    # walk to an entry S1 left, so each of those is read back too
    b, cap0, w2 = after_s1()
    res, st = G.oracle_run(("S1", "S2:%d" % cap0))
    same(call(b, w2.stream), res[1], "S2")
    f = fill(b)
    print(cap0, f, [r[4] for r in res])
    assert f["overflow_cap"] == 2 * cap0 and f["overflow_entries"] > 0, f
    # an entry is in one table or the other, live or deleted: never fewer than the oracle's live ones
    assert f["primary_live"] + f["overflow_entries"] >= res[1][4], (f, res[1][4])
    same_permanent_entries(b, st)
    same_entries(b, st)


def test_snapshot_and_restore_over_a_filled_overflow():
    # B: a snapshot that holds overflow entries, restored into a table of its size (a copy), then into one that grew
    # since (cleared, the snapshot's live entries rehashed).  A restore before the first S2 too, so that both S2
    # replays start from the snapshot's state (S1) and must agree
    b, cap0, w2 = after_s1()
    f_snap = fill(b)
    b.snapshot()
    res11, _ = G.oracle_run(("S1", "S1"))
    res12, st12 = G.oracle_run(("S1", "S2:%d" % cap0))
    second = call(b, G.s1().stream)
    same(second, res11[1], "S1 after the snapshot")
    b.restore()
    assert fill(b) == f_snap
    assert np.array_equal(b.permits(), res11[0][3])
    third = call(b, G.s1().stream)
    same(third, res11[1], "S1 after the restore")
    for g2, g3 in zip(second, third):
        assert np.array_equal(g2, g3)
    assert fill(b)["overflow_cap"] == cap0
    b.restore()
    assert fill(b) == f_snap
    first2 = call(b, w2.stream)
    same(first2, res12[1], "S2 after the restore")
    grown = fill(b)
    assert grown["overflow_cap"] == 2 * cap0 and grown["overflow_entries"] > 0, grown
    b.restore()  # the table is larger than the captured one
    f = fill(b)
    print(f_snap, grown, f, res12[0][4])
    assert f["overflow_cap"] == 2 * cap0
    assert (f["primary_live"], f["primary_deleted"]) == (f_snap["primary_live"], f_snap["primary_deleted"])
    # the rehash counts live entries only: all the oracle has beyond the primary table's
    assert f["overflow_entries"] == res12[0][4] - f_snap["primary_live"], (f, res12[0][4])
    assert 0 < f["overflow_entries"] <= f_snap["overflow_entries"]
    assert np.array_equal(b.permits(), res12[0][3])
    same_permanent_entries(b, G.oracle_run(("S1",))[1])
    again2 = call(b, w2.stream)
    same(again2, res12[1], "S2 after the restore into the grown table")
    for g1, g2 in zip(first2, again2):
        assert np.array_equal(g1, g2)
    assert fill(b)["overflow_cap"] == 2 * cap0
    same_entries(b, st12)


def spans(b, every=25):
    """Case C on context b (after S1): S3 one batch per replay_device_span call on device-resident buffers; map_fill
    before the first call, every 25 calls and at the end."""
    import torch

    dev = torch.device("cuda", 0)
    s = G.s3().stream
    d, _ = device_io(s, dev)
    fills = [(0, fill(b))]
    for k in range(s.n_batches):
        b.replay_device_span(s.acq_off[k], s.acq_off[k + 1], s.rel_off[k], s.rel_off[k + 1], d[1].data_ptr(),
                             d[3].data_ptr(), s.seq_base, d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr())
        if (k + 1) % every == 0 or k + 1 == s.n_batches:
            fills.append((k + 1, fill(b)))
    torch.cuda.synchronize()
    return (d[4].cpu().numpy(), d[5].cpu().numpy(), d[6].cpu().numpy()[: len(s.rel_aid)], b.permits()), fills


def test_entry_bound_runs_out_without_a_reason_to_grow():
    # C: 150 calls of 2,000 activations each.  The host's bound of the entry count grows by every call's activations
    # and is lowered from the counts the engine leaves behind (or an exact read-back); the entries stay a few thousand.
    # Whenever the capacity changes it is what ovf_need gives for an entry count the table had between the two checks,
    # never what the bound alone (60,000 + 2,000 per call, never refreshed) would ask for.  Twice, on two fresh
    # contexts: the same outputs
    res, st = G.oracle_run(("S1", "S3"))
    runs = []
    for rep in range(2):
        b = after_s1()[0]
        got, fills = spans(b)
        print(rep, fills)
        same(got, res[1], f"S3 span by span (run {rep})")
        assert len(fills) == 1 + 150 // 25 and fills[-1][0] == 150
        for (k0, f0), (k1, f1) in zip(fills, fills[1:]):
            if f1["overflow_cap"] == f0["overflow_cap"]:
                continue
            lo, hi = sorted((f0["overflow_entries"], f1["overflow_entries"]))
            assert G.ovf_need(lo, G.BATCH3) <= f1["overflow_cap"] <= G.ovf_need(hi, G.BATCH3), (k0, f0, k1, f1)
            stale = G.ovf_need(G.N1 + (k1 - 1) * G.BATCH3, G.BATCH3)
            assert stale == G.ovf_need(hi, G.BATCH3) or f1["overflow_cap"] != stale, (k0, f0, k1, f1)
        if rep:
            same_entries(b, st)
        runs.append((got, fills))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert [f["overflow_cap"] for _, f in runs[0][1]] == [f["overflow_cap"] for _, f in runs[1][1]]


def test_reset_of_a_filled_overflow():
    # D: updateCluster discards the map -- the overflow is cleared and the cleared table used again
    b, cap0, _ = after_s1()
    res, st = G.oracle_run(("S1", "cluster2", "S1"))
    _, st1 = G.oracle_run(("S1",))
    sl1 = st1.invoker_slots
    was_live = [(i, k) for i, k in G.sample_pairs(len(sl1), G.n_keys(G.s1()))
                if sl1[i].concurrent_state(k) is not None][:16]
    assert was_live and all(b.concurrent_state(i, k) == sl1[i].concurrent_state(k) for i, k in was_live)
    b.update_cluster(2)
    f = fill(b)
    assert f["overflow_entries"] == 0 and f["primary_live"] == 0 and f["overflow_cap"] == cap0, f
    assert np.array_equal(b.permits(), res[1][3])
    assert all(b.concurrent_state(i, k) is None for i, k in was_live)
    same(call(b, G.s1().stream), res[2], "S1 after updateCluster(2)")
    f = fill(b)
    print(f, res[2][4])
    assert f["overflow_cap"] == cap0 and f["primary_live"] + f["overflow_entries"] >= res[2][4], f
    same_entries(b, st)


def test_growth_inside_a_multi_shard_launch():
    # E: two shards in one launch, only the first has to grow its table (run_engine without a launch of its own)
    import torch

    dev = torch.device("cuda", 0)
    b0, cap0, w2 = after_s1()
    b1, cap1, _ = after_s1()
    assert cap1 == cap0
    (d0, io0), (d1, io1) = device_io(w2.stream, dev), device_io(G.s1().stream, dev)
    torch.cuda.synchronize()
    GpuShardingContainerPoolBalancer.replay_device_multi([(b0, io0), (b1, io1)])
    torch.cuda.synchronize()
    res0, st0 = G.oracle_run(("S1", "S2:%d" % cap0))
    res1, st1 = G.oracle_run(("S1", "S1"))
    for b, d, want, what in ((b0, d0, res0[1], "shard 0 (S2)"), (b1, d1, res1[1], "shard 1 (S1)")):
        same((d[4].cpu().numpy(), d[5].cpu().numpy(), d[6].cpu().numpy(), b.permits()), want, what)
    f0, f1 = fill(b0), fill(b1)
    print(f0, f1)
    assert f0["overflow_cap"] == 2 * cap0 and f0["overflow_entries"] > 0, f0
    assert f0["primary_live"] + f0["overflow_entries"] >= res0[1][4], (f0, res0[1][4])
    assert f1["overflow_cap"] == cap0 and f1["overflow_entries"] > 0, f1
    same_permanent_entries(b0, st0)
    same_entries(b0, st0)
    same_entries(b1, st1)
