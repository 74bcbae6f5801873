"""The large-state engine (openwhisk_amd/csrc/owgs_seq.hip) on hot small pools, with its path counters.

The engine's other streams run on 25k to 100k invokers, where two decisions of a 64-decision group almost never meet on
one invoker and its group speculation is nearly always kept.  Here the pools hold 1 to 600 invokers (the context is
moved to the engine by an action with maxConcurrent 5000, never invoked): speculations collide and are rejected, walks
fail and are forced, the map grows inside a replay, and the pool sizes sit on the engine's numeric thresholds.  Every
comparison is bit-exact against the literal oracle (decisions, overload flags, release flags, final permits, a sample
of the NestedSemaphore entries); `large_stats()` (owgs_large_stats) then shows that the branch a case exists for was
taken, and that every publish is counted on exactly one path."""
import numpy as np
import pytest

import large_state_cases as LC
import oracle as O
import test_gpu_parity as P
import test_gpu_resident as R
from openwhisk_amd.balancer import Action, HEALTHY, UNHEALTHY

pytestmark = pytest.mark.gpu
MB = 1024 * 1024
TOP = 2**31 - 1
KEPT = ("run_plain", "run_conc", "kept_plain", "kept_conc", "forced_spec")


def check_accounting(b, n_publishes):
    """every publish on exactly one path; the older two counters agree with the split ones"""
    st = b.large_stats()
    assert st is not None, "the context does not run on the large-state engine"
    assert st["large_spec"] == sum(st[k] for k in KEPT), st
    assert st["large_spec"] + st["alone"] + st["none_kind"] + st["throw_kind"] == n_publishes, st
    assert st["rejected"] <= st["alone"] and st["resumes"] < st["launches"], st
    old = b.stats()
    assert old.get("large_spec", 0) == st["large_spec"] and old.get("large_alone", 0) == st["alone"]
    return st


def check_entries(b, st, w, pairs):
    """concurrent_state of (invoker, action) pairs against the oracle's end state (empty entries included)"""
    slots = st.invoker_slots
    for inv, a in pairs:
        got = b.concurrent_state(int(inv), b.key_id(int(a)))
        assert got == slots[int(inv)].concurrent_state(st.keys[w.actions[int(a)].key]), (inv, a, got)


# ------------------------------------------------------------------------------------------- A: whole-stream sweep
# the counters a case exists for; observed values of large_stats() on an MI355X next to each case
NONZERO = {
    # run_plain 891, run_conc 981, kept_plain 2,358, kept_conc 1,151, forced_spec 10,077, alone 4,542 (rejected 3,041),
    # 327 release groups, all parallel, 1 launch
    "p40": ("forced_spec", "rejected"),
    # run_plain 1,604, kept_plain 1,405, forced_spec 2,185, alone 14,806 (rejected 2,403); run_conc = kept_conc = 0:
    # neither pool has more than SEQ_SPEC_C positions; 999 release groups, 1 launch
    "p17": ("rejected",),
    # run_plain 5,368, kept_plain 6,847, forced_spec 2,251, alone 5,534 (rejected 4,878), 318 release groups, 1 launch
    "p64": ("forced_spec",),
    # run_plain 3,885, run_conc 897, kept_plain 4,980, kept_conc 2,958, forced_spec 3,152, alone 4,128 (rejected 2,635)
    "p65": (),
    # run_conc 13,671, kept_conc 14,216, alone 32,113 (rejected 1,025), 938 release groups, 2 launches, 1 resume
    "p300": ("resumes",),
    # run_plain 13,714, run_conc 5,379, kept_plain 1,217, kept_conc 8,594, forced_spec 1,793, alone 9,303 (rejected 903)
    "p600": ("run_plain", "run_conc", "kept_conc"),
}
# Case B, the same streams call by call (p17 in 280 launches, p300 in 810, p600 in 550): p17 run_plain 1,692,
# kept_plain 1,364, forced_spec 2,244, alone 14,700; p300 run_conc 15,298, kept_conc 14,722, alone 29,980, no resume
# (the host grows the map between calls); p600 run_plain 13,831, run_conc 5,585, kept_plain 1,170, kept_conc 8,490,
# forced_spec 1,085, alone 9,839.


@pytest.mark.parametrize("name", list(LC.CASES))
def test_small_pool_stream_matches_oracle_and_counts_its_paths(name):
    """Case A: every table case through the whole-stream entry point (owgs_replay)."""
    w = LC.workload(name)
    st, o_inv, o_fl, o_rf = LC.oracle_run(name)
    b = P.gpu_for(w)
    assert b.large_stats() is not None
    g_inv, g_fl, g_rf = b.replay(w.stream)
    bad = np.nonzero(o_inv != g_inv)[0]
    assert len(bad) == 0, f"{name}: first mismatch at {bad[:5]} oracle={o_inv[bad[:5]]} gpu={g_inv[bad[:5]]}"
    assert np.array_equal(o_fl, g_fl)
    assert np.array_equal(o_rf, g_rf)
    assert np.array_equal(st.permits(), b.permits())
    ls = check_accounting(b, len(w.stream.act))
    print(name, ls)
    for k in NONZERO[name] + ("alone", "large_spec"):
        assert ls[k] > 0, (name, k, ls)
    assert ls["none_kind"] == 0 and ls["throw_kind"] == 0 and ls["rel_groups_ordered"] == 0
    if name == "p17":  # pools of 16 and 1 positions: concurrent decisions never speculate (n > SEQ_SPEC_C fails)
        assert ls["run_conc"] == 0 and ls["kept_conc"] == 0, ls
    if name == "p64":  # no concurrent action at all
        assert ls["run_conc"] == 0 and ls["kept_conc"] == 0, ls
    # entries: where concurrent activations of the last batches went, and random pairs (mostly absent or empty)
    rng = np.random.default_rng(5)
    conc = np.nonzero(np.array([a.max_concurrent > 1 for a in w.actions])[w.stream.act])[0]
    pairs = [(g_inv[i], w.stream.act[i]) for i in conc[-150:]]
    ca = np.unique(w.stream.act[conc]) if len(conc) else np.zeros(0, int)
    pairs += [(rng.integers(0, len(w.inv_ids)), rng.choice(ca)) for _ in range(150 if len(ca) else 0)]
    check_entries(b, st, w, pairs)


# ------------------------------------------------------------------------------------------- B: call by call
@pytest.mark.parametrize("name", ["p17", "p300", "p600"])
def test_small_pool_shim_sequence_matches_oracle(name):
    """Case B: the same streams as the shim's owgs_process_batch sequence, drains of 1..300 jobs: one launch per call
    (cursor generations start over, the map and its deleted entries carry over from call to call), on p300 with
    updateCluster halfway."""
    w = LC.workload(name)
    sh = R.Shim(w, shadow=True)
    rng = np.random.default_rng(17)
    half = len(sh.jobs) // 2
    changed = name != "p300"
    while not sh.done():
        if not changed and sh.pos >= half:
            for x in (sh.g, sh.o, sh.z):
                x.update_cluster(2)
            changed = True
        sh.call(int(rng.integers(1, 301)))
    assert np.array_equal(sh.g.permits(), sh.o.permits())
    assert sh.g.resident_stats()["served"] == 0
    ls = check_accounting(sh.g, sh.seq)
    print(name, ls)
    assert sh.seq == len(w.stream.act) and ls["launches"] >= sh.calls
    assert ls["alone"] > 0 and ls["large_spec"] > 0


# ------------------------------------------------------------------------------------------- C: pool-size boundaries
def _boundary_script(n, managed=1.0, blackbox=0.0, unhealthy_every=0, seed=21):
    """3,000 activations in 20 calls of 150 publishes on n uniform 1,024 MB invokers, each call first releasing 75
    activations in flight (so the pool fills up and walks fail): the oracle's answers, call by call."""
    rng = np.random.default_rng(seed)
    o = O.BalancerState(managed, blackbox, rng_seed=seed, zombies=True)
    ids, mem = np.arange(n, dtype=np.int32), np.full(n, 1024 * MB, np.int64)
    status = np.zeros(n, np.uint8)
    if unhealthy_every:
        status[::unhealthy_every] = UNHEALTHY
    o.update_invokers(ids, mem, status)
    acts = [Action(f"ns{a % 3}", f"ns{a % 3}/p/a{a}", "0.0.1", (128, 256, 512)[a % 3], 1 if a < 4 else 3,
                   blackbox > 0 and a % 4 == 3) for a in range(8)] + [LC.WIDE]
    oh = [o.register_action(a.namespace, a.path, k, a.mem_mb, a.max_concurrent, a.blackbox) for k, a in enumerate(acts)]
    live, seq, calls = [], 0, []
    for _ in range(20):
        pick = rng.choice(len(live), size=min(75, len(live)), replace=False) if live else np.zeros(0, int)
        rel = [live[j] for j in sorted(pick)]
        gone = set(pick.tolist())
        live = [x for j, x in enumerate(live) if j not in gone]
        pubs = rng.integers(0, 8, size=150)
        orf = [O._rel_bits(o.release(x, oh[a])) for x, a in rel]
        oi = [o.publish(oh[a], seq + k) for k, a in enumerate(pubs)]
        calls.append((rel, pubs, seq, orf, oi))
        seq += len(pubs)
        live += [(int(x), int(a)) for (x, _), a in zip(oi, pubs) if x >= 0]
    return o, acts, (ids, mem, status), calls


def _run_boundary(n, **kw):
    o, acts, (ids, mem, status), calls = _boundary_script(n, **kw)
    forced = sum(f & 1 for _, _, _, _, oi in calls for _, f in oi)
    assert forced > 0, "the pool never fills: no walk fails"
    g = P.gpu(managed_fraction=kw.get("managed", 1.0), blackbox_fraction=kw.get("blackbox", 0.0),
              rng_seed=kw.get("seed", 21))
    g.update_invokers_arrays(ids, mem, status)
    gh, _ = g.register_actions(acts)
    assert g.managed_size == o.managed_size and g.blackbox_size == o.blackbox_size
    for c, (rel, pubs, seq, orf, oi) in enumerate(calls):
        gi, gf, grf = g.process_batch([0, len(rel)], [x for x, _ in rel], [gh[a] for _, a in rel], [0, len(pubs)],
                                      [gh[a] for a in pubs], seq_base=seq)
        assert grf.tolist() == orf, c
        assert [(int(x), int(f)) for x, f in zip(gi, gf)] == oi, c
    assert np.array_equal(g.permits(), o.permits())
    check_accounting(g, 3000)
    slots = o.invoker_slots
    rng = np.random.default_rng(1)
    for inv in (range(n) if n <= 80 else rng.choice(n, 80, replace=False)):
        for a in range(4, 8):
            assert g.concurrent_state(int(inv), g.key_id(int(gh[a]))) == slots[int(inv)].concurrent_state(a), (inv, a)
    return g, o


@pytest.mark.parametrize("nm", [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 254, 255, 256, 257, 258])
def test_pool_size_boundaries(nm):
    """Case C: managed pools of exactly nm positions around SEQ_SPEC_C = 16 (concurrent speculation needs n > 16),
    SEQ_SPEC = 64 (the plain speculation's budget; `sx + u >= n` ends a walk inside it) and the 256-probe round of a
    walk decided alone (n + 2 probes: 256 at n = 254, 257 at n = 255, one probe into a second round)."""
    g, o = _run_boundary(nm)
    assert g.managed_size == nm


def test_blackbox_pool_at_an_odd_first_id():
    """77 invokers at 0.9 / 0.1: the blackbox pool's ids start inside a word of the usable bitmap."""
    g, o = _run_boundary(77, managed=0.9, blackbox=0.1)
    assert (77 - g.blackbox_size) % 32 != 0 and g.blackbox_size > 1


def test_pool_with_a_quarter_of_the_invokers_unhealthy():
    """Unusable positions inside the walks and the forced acquire's choice among the healthy ones only."""
    _run_boundary(66, unhealthy_every=4)


# ------------------------------------------------------------------------------------------- D: capacity arithmetic
def _pair(permits_mb):
    n = len(permits_mb)
    g = P.gpu(managed_fraction=1.0, blackbox_fraction=0.0, rng_seed=9)
    o = O.BalancerState(1.0, 0.0, rng_seed=9, zombies=True)
    ids, mem = np.arange(n, dtype=np.int32), np.array(permits_mb, np.int64) * MB
    g.update_invokers_arrays(ids, mem, np.zeros(n, np.uint8))
    o.update_invokers(ids, mem, np.zeros(n, np.uint8))
    assert g.permits().tolist() == o.permits().tolist() == list(permits_mb)
    return g, o


def _register(g, o, acts):
    acts = list(acts) + [LC.WIDE]
    gh, _ = g.register_actions(acts)
    oh = [o.register_action(a.namespace, a.path, k, a.mem_mb, a.max_concurrent, a.blackbox) for k, a in enumerate(acts)]
    assert g.large_stats() is not None
    return gh, oh


def _publish_groups(g, o, gh, oh, sizes=(64, 130)):
    seq = 0
    for n in sizes:
        gi, gf = g.publish([gh] * n, seq_base=seq)
        oi = [o.publish(oh, seq + k) for k in range(n)]
        assert [(int(x), int(f)) for x, f in zip(gi, gf)] == oi, (n, seq)
        seq += n
    assert np.array_equal(g.permits(), o.permits())
    check_accounting(g, seq)


@pytest.mark.parametrize("maxc", [1, 3])
@pytest.mark.parametrize("mem", [129, 1000, 4097])
def test_capacity_quotient_at_its_boundaries(mem, maxc):
    """Case D: the speculation's floor(permits / mem) (a float estimate and one correction, clamped to 64) where it is
    exactly k - 1, k and k + 1 for k around 1, 2 and the clamp: three invokers holding k * mem - 1, k * mem and
    k * mem + 1 MB, memories that are no power of two, one group of 64 and one call of 130 decisions of one action
    (ranks 0..63, then groups that start from the first one's cursor)."""
    for k in (1, 2, 63, 64, 65):
        g, o = _pair([max(k * mem - 1, 128), k * mem, k * mem + 1])
        gh, oh = _register(g, o, [Action("ns", "ns/p/a", "0.0.1", mem, maxc)])
        _publish_groups(g, o, gh[0], oh[0])
        if maxc > 1:
            for inv in range(3):
                assert g.concurrent_state(inv, g.key_id(int(gh[0]))) == o.invoker_slots[inv].concurrent_state(0)


@pytest.mark.parametrize("maxc", [1, 3])
@pytest.mark.parametrize("mem", [128, 129])
def test_capacity_quotient_far_beyond_the_clamp(mem, maxc):
    """An invoker holding 2**31 - 1 MB: the quotient (16.7 M) is far beyond the clamp and its float estimate is off by
    more than the one correction; a second, nearly full invoker makes the walks pass or land there by one MB."""
    g, o = _pair([TOP, 2 * mem - 1, 3 * mem])
    gh, oh = _register(g, o, [Action("ns", "ns/p/a", "0.0.1", mem, maxc)])
    _publish_groups(g, o, gh[0], oh[0])


def test_none_and_index_out_of_bounds_outcomes_are_counted_apart():
    """The two outcomes that are no decision (an empty pool's None, SCPB:288-290; the Int.MinValue hash, SCPB:266-268)
    count as neither kept nor alone, so the accounting identity needs their counters."""
    g = P.gpu(managed_fraction=1.0, blackbox_fraction=0.0)
    gh, _ = g.register_actions([Action("ns", "ns/p/a", "0.0.1", 256), LC.WIDE])
    assert g.publish([gh[0]] * 70)[0].tolist() == [-1] * 70
    st = check_accounting(g, 70)
    assert st["none_kind"] == 70 and st["throw_kind"] == 0 and st["alone"] == 0 and st["large_spec"] == 0
    g, o = _pair([1024] * 3)
    gh, oh = _register(g, o, [Action("", "polygenelubricants", "0.0.1", 256), Action("ns", "ns/p/a", "0.0.1", 256)])
    gi, gf = g.publish([gh[0], gh[1]] * 5)
    assert gi[0::2].tolist() == [-2] * 5
    assert [(int(x), int(f)) for x, f in zip(gi[1::2], gf[1::2])] == [o.publish(oh[1], 2 * k + 1) for k in range(5)]
    st = check_accounting(g, 10)
    assert st["throw_kind"] == 5 and st["none_kind"] == 0 and st["large_spec"] + st["alone"] == 5


# ------------------------------------------------------------------------------------------- E: release groups
def _release(g, o, gh, oh, rels):
    """one owgs_release_batch call against the oracle release by release; the groups it took by path"""
    before = g.large_stats()
    grf = g.release_invoker([x for x, _ in rels], [gh[a] for _, a in rels])
    orf = [O._rel_bits(o.release(x, oh[a])) for x, a in rels]
    assert grf.tolist() == orf
    assert np.array_equal(g.permits(), o.permits())
    after = g.large_stats()
    return orf, after["rel_groups_par"] - before["rel_groups_par"], \
        after["rel_groups_ordered"] - before["rel_groups_ordered"]


def test_plain_release_groups_are_applied_in_parallel():
    """Case E (a): 200 maxConcurrent == 1 releases in one call, no invoker near the int range: four groups, each
    applied at once."""
    g, o = _pair([4096] * 10)
    gh, oh = _register(g, o, [Action("ns", "ns/p/a", "0.0.1", 128, 1)])
    gi, _ = g.publish([gh[0]] * 200)
    oi = [o.publish(oh[0], k)[0] for k in range(200)]
    assert gi.tolist() == oi and min(oi) >= 0
    orf, par, ordered = _release(g, o, gh, oh, [(x, 0) for x in oi])
    assert orf == [0] * 200 and (par, ordered) == (4, 0)
    assert g.permits().tolist() == [4096] * 10


def test_release_group_at_the_int_range_exactly_and_one_past():
    """Case E (b): a 64-release group after which one invoker holds 2**31 - 1 MB exactly is still applied at once, no
    flag; one MB more and the group is applied in queue order, ForcibleSemaphore's overflow Error (FS:48-50) on the
    release where the oracle has it -- in the same call as a group applied at once."""
    acts = [Action("ns", "ns/p/a", "0.0.1", 256, 1)]
    g, o = _pair([TOP - 64 * 256, 1000])
    gh, oh = _register(g, o, acts)
    orf, par, ordered = _release(g, o, gh, oh, [(0, 0)] * 64)
    assert orf == [0] * 64 and (par, ordered) == (1, 0) and g.permits().tolist() == [TOP, 1000]
    g, o = _pair([TOP - 64 * 256 + 1, 1000])
    gh, oh = _register(g, o, acts)
    orf, par, ordered = _release(g, o, gh, oh, [(1, 0)] * 64 + [(0, 0)] * 64)
    assert orf == [0] * 127 + [2] and (par, ordered) == (1, 1)
    assert g.permits().tolist() == [TOP - 255, 1000 + 64 * 256]
    # the bound counts everything the group returns, to any invoker: here nothing overflows, in queue order all the same
    g, o = _pair([TOP - 64 * 256 + 1, 1000])
    gh, oh = _register(g, o, acts)
    orf, par, ordered = _release(g, o, gh, oh, [(0, 0), (1, 0)] * 32)
    assert orf == [0] * 64 and (par, ordered) == (0, 1)


def test_mixed_release_group_at_a_near_limit_invoker():
    """Case E (c): plain and concurrent releases to one invoker near the int range in one group; a concurrent release
    empties a container (its memory returns: the Error comes after the ResizableSemaphore update, the entry stays)."""
    acts = [Action("ns", "ns/p/a", "0.0.1", 128, 1), Action("ns", "ns/p/c", "0.0.1", 256, 3)]
    g, o = _pair([TOP - 44])
    gh, oh = _register(g, o, acts)
    gi, gf = g.publish([gh[1]] * 6)  # two containers of three
    oi = [o.publish(oh[1], k) for k in range(6)]
    assert [(int(x), int(f)) for x, f in zip(gi, gf)] == oi and g.permits().tolist() == [TOP - 44 - 512]
    rels = [(0, 0), (0, 1), (0, 1), (0, 1), (0, 0), (0, 0), (0, 1), (0, 1), (0, 1), (0, 0), (0, 1)]
    orf, par, ordered = _release(g, o, gh, oh, rels)
    # 128 + (256: the first container) + 128 fit; the third plain release and the second container's memory do not, and
    # the entry that Error left behind ({0 free, 0 operations}) takes the eleventh release: no NoSuchElementException
    assert orf == [0, 0, 0, 0, 0, 2, 0, 0, 2, 2, 0] and (par, ordered) == (0, 1)
    assert g.permits().tolist() == [TOP - 44]
    assert g.concurrent_state(0, g.key_id(int(gh[1]))) == o.invoker_slots[0].concurrent_state(1) == (1, -1)
