"""In-pass re-decisions with their per-lane work on the engine lanes: before the I/O wave re-decides a
stopping lane, the engine lanes give their own tentative takes back and meet it at a barrier of their own; after the
last re-decision each lane that would keep its speculation tests its own target and action against the re-decided sets,
which the I/O wave leaves in LDS.

Every case is bit-exact against the oracle: assignment vector, decision flags, release flags and final permits.  The
cases are small (each generates and replays through the CPU oracle in well under a second): the three chunk widths with
partly empty waves at the new barriers, mixed classes with new containers created in commit, several re-decisions in
one pass, the narrow geometry, and the other two kernels' dispatch.
"""
import numpy as np
import pytest

import oracle as O
from openwhisk_amd import GpuShardingContainerPoolBalancer
from openwhisk_amd import workload as W

pytestmark = pytest.mark.gpu

SMALL = dict(user_memory_mb=1024, n_actions=400, n_namespaces=40)
# 200 invokers kept near full, maxConcurrent 1 (chunk width 192): passes stop on lanes whose invoker an earlier lane
# filled, and the I/O wave re-decides them inside the pass
FULL192 = dict(n_invokers=200, batch=2000, delay_mean=1.2, conc_frac=0.0, blackbox_frac=0.0, unhealthy_frac=0.0,
               user_memory_mb=8192, n_actions=400, n_namespaces=40)


def gpu_for(w):
    b = GpuShardingContainerPoolBalancer(managed_fraction=w.managed_fraction, blackbox_fraction=w.blackbox_fraction,
                                         rng_seed=w.rng_seed)
    b.update_invokers_arrays(w.inv_ids, w.inv_mem, w.inv_status)
    b.update_cluster(w.cluster_size)
    b.register_actions(w.actions)
    return b


def check(w, b=None):
    st = O.state_for(w)
    o_inv, o_fl, o_rf = st.replay(w.stream)
    b = b or gpu_for(w)
    g_inv, g_fl, g_rf = b.replay(w.stream)
    bad = np.nonzero(o_inv != g_inv)[0]
    assert len(bad) == 0, f"first mismatch at {bad[:5]} oracle={o_inv[bad[:5]]} gpu={g_inv[bad[:5]]}"
    assert np.array_equal(o_fl, g_fl)
    assert np.array_equal(o_rf, g_rf)
    assert np.array_equal(st.permits(), b.permits())
    return b, o_fl


def _units(w):
    """Capacity units as the library's chunk_width counts them: managed slot MB over the mean action MB."""
    return w.info["usable"] * w.managed_fraction * w.info["slot_mb"] / np.mean([a.mem_mb for a in w.actions])


def test_width_448():
    # 80,640 units: the widest chunks; overloaded, so the mem > U forced re-decision runs too
    w = W.config("c2", n_invokers=700, n_activations=150_000, mem_choices=(128,), load=1.2, delay_mean=1.5,
                 n_actions=400, n_namespaces=40)
    assert _units(w) >= 60_000 and w.stream.n_batches == 3
    b, fl = check(w)
    assert np.any(fl & 1)
    assert b.stats()["redecided"] > 0


def test_width_256():
    w = W.config("c2", n_invokers=400, n_activations=60_000, mem_choices=(128, 256), load=1.0, delay_mean=1.5,
                 n_actions=400, n_namespaces=40)
    assert 30_000 <= _units(w) < 60_000
    b, _ = check(w)
    assert b.stats()["redecided"] > 0


@pytest.mark.parametrize("n_act", [4000, 4201])
def test_width_192(n_act):
    # 4,201 activations in batches of 2,000: the last chunks hold 201 lanes and then 1 -- partly empty waves (and
    # whole waves without a lane) at every barrier of the re-decision and commit phases
    w = W.config("headline", n_activations=n_act, **FULL192)
    assert _units(w) < 30_000
    b, fl = check(w)
    assert np.any(fl & 1)
    assert b.stats()["redecided"] > 0


def test_mixed_classes():
    # a quarter of the actions concurrent on a near-full small pool: stops that are not re-decidable end the pass,
    # exempt lanes (forced decisions) sit between the stops and are never dropped for a clash, and new containers are
    # created in commit
    w = W.config("headline", n_invokers=203, n_activations=6000, delay_mean=1.5, conc_frac=0.25, load=1.2, **SMALL)
    assert any(a.max_concurrent > 1 for a in w.actions)
    b, fl = check(w)
    assert np.any(fl & 1)
    assert b.stats()["redecided"] > 0


def test_several_redecisions_per_pass():
    # 60 invokers kept full by 40 actions, maxConcurrent 1: one pass re-decides several lanes (each one's takes given
    # back once, re-applied lane by lane), and the next lane of a re-decided action ends it
    w = W.config("c2", n_invokers=60, n_activations=6000, load=1.1, delay_mean=1.5, n_actions=40, n_namespaces=8,
                 user_memory_mb=8192)
    b, _ = check(w)
    st = b.stats()
    assert st["redecided"] > st["stops"], st


def test_narrow_geometry():
    # 12,000 invokers: the 7 x 32 geometry compiles the same body
    w = W.config("c2", n_invokers=12_000, n_activations=40_000, user_memory_mb=1024, mem_choices=(256, 512), load=1.0,
                 delay_mean=1.5, n_actions=400, n_namespaces=40)
    b, _ = check(w)
    assert b.large_stats() is None  # (an on-chip engine ran it)


def test_multi_shard_launch():
    # two shards of the near-full pool in one launch: the multi-shard kernel's two bodies
    import torch

    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    shards = []
    for g in (0, 1):
        w = W.config("headline", shard=g, n_shards=2, n_activations=4000, **FULL192)
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
        assert b.stats()["redecided"] > 0


def test_group_replay_with_health_rows():
    # the batches of the near-full pool in one engine launch, each with its own health row
    import torch
    from openwhisk_amd import cluster

    w = W.config("headline", n_activations=4000, **FULL192)
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
    assert b.stats()["redecided"] > 0
