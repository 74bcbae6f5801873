"""The chunked engine after its split by wave role (one body for the I/O wave, one for the engine waves) and with the
compile-time LDS layout (fixed regions first, permits / pool / prefix counts last).

Every case is bit-exact against the oracle: assignment vector, decision flags, release flags and final permits.  The
cases are small: they aim at the regions that now sit at variable offsets behind the permits, at a full image, at both
pool modes, at the I/O wave's own work (in-pass re-decisions) and at each of the three kernels' dispatch.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from openwhisk_amd import GpuShardingContainerPoolBalancer
from openwhisk_amd import _lib
from openwhisk_amd import workload as W

pytestmark = pytest.mark.gpu

# invokers of 1 GB with actions up to 2 GB: the 2 GB actions fit nowhere, so each takes the overload fallback (the
# usable bitmap and its prefix counts: the regions behind the permits)
SMALL = dict(user_memory_mb=1024, n_actions=400, n_namespaces=40)


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


@pytest.mark.parametrize("n_inv", [1001, 1002, 1003])
def test_pool_sizes_off_a_multiple_of_four(n_inv):
    # n_slots % 4 = 1, 2, 3: the tail slots of the 16-byte permit load, and the bitmap / prefix counts start behind a
    # padded permit region
    w = W.config("headline", n_invokers=n_inv, n_activations=4500, batch=1500, delay_mean=1.5, conc_frac=0.25,
                 unhealthy_frac=0.02, **SMALL)
    assert w.stream.n_batches == 3 and len(w.stream.rel_aid) > 0
    _, fl = check(w)
    assert np.any(fl & 1)  # forced (overload fallback) decisions


def _largest_pools():
    """The largest identity pool of the wide geometry (the library picks it while its image fits 160 KB) and of the
    narrow one (owgs_limits)."""
    L = _lib.lib()
    L.owgs_engine_lds_bytes.restype = C.c_size_t
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if L.owgs_engine_lds_bytes(mid, 0, mid, mid, mid, 0) <= 160 * 1024:
            lo = mid
        else:
            hi = mid - 1
    mi, ms = C.c_int32(), C.c_int32()
    assert L.owgs_limits(C.byref(mi), C.byref(ms)) == 0
    assert lo < mi.value
    return lo, mi.value


@pytest.mark.parametrize("geometry", ["wide", "narrow"])
def test_full_image(geometry):
    # the image is full: an off-by-one of the layout corrupts the last permits (the blackbox pool's, at the end of the
    # ids) or the prefix counts
    n_inv = _largest_pools()[0 if geometry == "wide" else 1]
    w = W.config("headline", n_invokers=n_inv, n_activations=2000, batch=1000, delay_mean=1.2, blackbox_frac=0.3,
                 unhealthy_frac=0.02, **SMALL)
    b, fl = check(w)
    assert np.any(fl & 1)
    assert b.large_stats() is None  # (an on-chip engine ran it)


def test_explicit_pools():
    # pool words instead of the bitmap, concurrent actions: the OWGS_F_ALL instantiation.  The explicit pools name the
    # invokers the identity pools would, so the oracle's decisions are the same
    w = W.config("headline", n_invokers=301, n_activations=2000, batch=1000, delay_mean=1.2, conc_frac=0.3,
                 unhealthy_frac=0.02, **SMALL)
    b = gpu_for(w)
    nm, nb, n = b.managed_size, b.blackbox_size, len(w.inv_ids)
    b.set_pool(0, [(int(w.inv_ids[i]), int(w.inv_status[i])) for i in range(nm)])
    b.set_pool(1, [(int(w.inv_ids[i]), int(w.inv_status[i])) for i in range(n - nb, n)])
    _, fl = check(w, b)
    assert np.any(fl & 1)


def test_io_wave_redecides():
    # 200 invokers kept near full, maxConcurrent 1: passes stop on lanes whose invoker an earlier lane filled, and the
    # I/O wave re-decides them inside the pass
    w = W.config("headline", n_invokers=200, n_activations=4000, batch=2000, delay_mean=1.2, conc_frac=0.0,
                 blackbox_frac=0.0, unhealthy_frac=0.0, user_memory_mb=8192, n_actions=400, n_namespaces=40)
    b, _ = check(w)
    assert b.stats()["redecided"] > 0


def test_multi_shard_launch():
    # two small shards in one launch: the multi-shard kernel's dispatch into the two bodies
    import torch

    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    shards = []
    for g in (0, 1):
        w = W.config("headline", shard=g, n_shards=2, n_invokers=203, n_activations=3000, batch=1000, delay_mean=1.5,
                     conc_frac=0.25, **SMALL)
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
    # three batches in one engine launch, each with its own health row: the engine rebuilds the bitmap and the prefix
    # counts (behind the permits) before every batch
    import torch
    from openwhisk_amd import cluster

    w = W.config("headline", n_invokers=203, n_activations=3000, batch=1000, delay_mean=1.5, conc_frac=0.25, **SMALL)
    s = w.stream
    assert s.n_batches == 3
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
