"""owgs_destroy frees everything a context ever owned: owgs_live_resources (device allocations, pinned blocks, events
+ streams, process-wide) reads the same before a context is created and after it is closed, for one context driven
through every path that reserves a buffer of its own -- replays on the chunked engine and in the resident engine's
stream mode, a group replay, drained batches on the resident engine with watched pairs, key recycling, the gated
publish with messages and result-carrying acks.  Each step is checked against the oracle as in the neighbouring tests
(test_gpu_parity, test_gpu_resident, test_gpu_invoke), so the paths are known to have run.  Stream mode is selected by
OWGS_SPEC_REPLAY, read once per process, so the scenario runs in a child process (this file as a script)."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_KEYS = 131_070  # OWGS_MAX_SLOTKEYS: the fqn@version key ids are 0..MAX_KEYS


def scenario():
    import torch

    import oracle as O
    from openwhisk_amd import Action, _lib
    from openwhisk_amd import workload as W
    from openwhisk_amd._lib import ACK_RELEASED, ACKF_RESULT
    from result_ack_cases import canonical
    from test_gpu_invoke import Batch, Ctx, check_state, run
    from test_gpu_resident import Shim

    gc.collect()
    before = _lib.live_resources()

    def cfg(n, shard):  # one cluster (64 invokers, 40 actions, 30 % of them concurrent), a stream of its own per shard
        return W.config("c4", n_activations=n, n_invokers=64, n_actions=40, shard=shard)

    sh = Shim(cfg(1500, 0))
    g, o, w = sh.g, sh.o, sh.w
    assert len(w.actions) == 40 and any(a.max_concurrent > 1 for a in w.actions)
    assert list(sh.gh) == list(sh.oh) == list(range(40))
    assert _lib.live_resources()[0] > before[0]

    def same_replay(stream):
        got, want = g.replay(stream), o.replay(stream)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert np.array_equal(g.permits(), o.permits())

    # 1. a 2,000-activation replay: the chunked engine, or the resident engine's stream mode under OWGS_SPEC_REPLAY=1
    same_replay(cfg(2000, 1).stream)
    assert (g.stream_mode_stats() is not None) == (os.environ.get("OWGS_SPEC_REPLAY") == "1")

    # 2. owgs_replay_device_group: three batches per launch, each with its health row (test_gpu_parity's group test)
    s = cfg(600, 2).stream
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    d_act, d_aid = t(s.act, np.int32), t(s.rel_aid, np.int64)
    d_out = torch.full((len(s.act),), -9, dtype=torch.int32, device=dev)
    d_fl = torch.zeros(len(s.act), dtype=torch.uint8, device=dev)
    d_rf = torch.zeros(max(len(s.rel_aid), 1), dtype=torch.uint8, device=dev)
    d_h = t(np.stack([w.inv_status] * s.n_batches), np.uint8)
    acq, rel = np.ascontiguousarray(s.acq_off, np.int64), np.ascontiguousarray(s.rel_off, np.int64)
    nid = len(w.inv_status)
    for g0 in range(0, s.n_batches, 3):
        g1 = min(g0 + 3, s.n_batches)
        g.replay_device_group(acq[g0:g1 + 1], rel[g0:g1 + 1], d_act.data_ptr(), d_aid.data_ptr(), s.seq_base,
                              d_out.data_ptr(), d_fl.data_ptr(), d_rf.data_ptr(), d_h[g0].data_ptr(), nid, nid)
    torch.cuda.synchronize()
    o_inv, o_fl, o_rf = O.replay_with_health(o, s, w.inv_ids, w.inv_mem, [w.inv_status] * s.n_batches)
    assert np.array_equal(d_out.cpu().numpy(), o_inv) and np.array_equal(d_fl.cpu().numpy(), o_fl)
    assert np.array_equal(d_rf.cpu().numpy()[:len(s.rel_aid)], o_rf[:len(s.rel_aid)])
    assert np.array_equal(g.permits(), o.permits())

    # 3. updateCluster with concurrent activations in flight: watched pairs; a replay then goes batch by batch
    g.update_cluster(2)
    o.update_cluster(2)
    same_replay(cfg(2000, 3).stream)

    # 4. twenty drained batches of 1-64 jobs on the resident engine (its watched-pair index)
    rng = np.random.default_rng(7)
    for _ in range(20):
        sh.call(int(rng.integers(1, 65)))
    st = g.resident_stats()
    assert st["served"] > 0 and st["watch_calls"] > 0, st
    assert np.array_equal(g.permits(), o.permits())

    # 5. the gated publish with messages, then result-carrying acks for what it placed (test_gpu_invoke's model)
    cx = Ctx.around(g, o, sh.oh, w.actions, cluster=2)
    B = Batch(rng, 48, cx.hs, 600_000, reject=(3, 17))
    got = run(cx, B, 100, seq_base=sh.seq, n_topics=len(w.inv_ids))  # (one topic per invoker)
    placed = [i for i in range(B.n) if got[5][i] >= 0][:12]
    assert placed
    msgs = [canonical(rng, B.aids[i], int(got[5][i]), "combined") for i in placed]
    want = cx.m.pm.t.process_acks([W.completion_message(B.aids[i], int(got[5][i])) for i in placed])
    r = g.process_result_acks(msgs)
    assert np.array_equal(r[0], want[0]) and np.all(r[0] == ACK_RELEASED) and np.array_equal(r[2], want[2])
    assert r[1].tolist() == [int(got[5][i]) for i in placed] and np.all(r[3] & ACKF_RESULT)
    check_state(cx)

    # 6. key recycling: fillers take every key id left (their handles are dropped round by round), so the next new key
    # makes the context scan its tables for ids nothing holds any more (reclaim_slots)
    left, k0 = MAX_KEYS + 1 - 40, 0
    while left:
        n = min(left, 8000)
        hs, _ = g.register_actions([Action("fill", f"fill/a{k0 + k}", "0.0.1", 128) for k in range(n)])
        g.release_actions([int(h) for h in hs])
        left, k0 = left - n, k0 + n
    new = Action("fresh", "fresh/action", "0.0.1", 256, 3)
    (gh,), _ = g.register_actions([new])
    assert 0 <= g.key_id(int(gh)) <= MAX_KEYS
    oh = o.register_action(new.namespace, new.path, 40, new.mem_mb, new.max_concurrent, new.blackbox)
    seq = sh.seq + B.n
    gi, gf, _ = g.process_batch([0, 0], [], [], [0, 6], [int(gh)] * 6, seq_base=seq)
    assert [(int(a), int(b)) for a, b in zip(gi, gf)] == [tuple(int(v) for v in o.publish(oh, seq + j)) for j in range(6)]
    assert np.array_equal(g.permits(), o.permits())

    g.close()
    gc.collect()
    assert _lib.live_resources() == before, (_lib.live_resources(), before)


def test_destroy_frees_every_resource_of_a_context_that_used_every_path():
    env = dict(os.environ, OWGS_SPEC_REPLAY="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(HERE))
    assert r.returncode == 0 and "lifetime scenario ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_failed_create_leaves_nothing_behind():
    from openwhisk_amd import GpuShardingContainerPoolBalancer, OwgsError, _lib
    gc.collect()
    before = _lib.live_resources()
    # (a device index beyond every device count: owgs_create gives up at its range check, BEFORE it owns a stream or a
    # buffer.  Its later failure paths -- an allocation or a launch that fails once the stream exists -- end in
    # owgs_destroy on a partly built context; no argument reaches them, so they are covered only in so far as that is
    # the call the second half below makes on a whole context.)
    with pytest.raises(OwgsError):
        GpuShardingContainerPoolBalancer(device=1_000_000)
    gc.collect()
    assert _lib.live_resources() == before
    # ... and a context that did come up goes away whole
    GpuShardingContainerPoolBalancer().close()
    assert _lib.live_resources() == before


if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]
    scenario()
    print("lifetime scenario ok")
