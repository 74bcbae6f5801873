"""owgs_process_batch on drained batches in arrival order (tests/arrival_cases.py): completions and publishes
interleaved as a controller's queue holds them, so that one call holds dozens to a thousand runs and many of its
completions name an activation published earlier in the same call.  The queue of every other test is each stream
batch's completions, then its publishes, in stream batches of thousands of jobs: one to three runs per call.

Part 1 drives the three cases of arrival_cases.py through each of the call's four routes -- the resident engine
(owgs_resident.hip), the fused launch chain (owgs_fused.hip and the pre-pass of owgs_kernels.hip), the per-run path
(process_runs in owgs_host.cpp, taken while watched pairs exist) and the large-state engine (owgs_seq.hip) -- and
part 2 adds hand-made run shapes on a pool of seven invokers.  Every comparison is bit-exact against the literal
oracle, call by call (decisions and flags, release flags: Shim.call / Pool.call assert them) and on the final permits.
The route of every call is read as the difference of resident_stats() (`served`, `chained`) and large_stats()
(`launches`) around it, so a call that quietly takes another route fails its test.  Routes are chosen by call size and
context state alone; tests/test_arrival_inputs.py checks the shape of the same calls on the CPU."""
import collections

import numpy as np
import pytest

import arrival_cases as AC
import oracle as O
from large_state_cases import WIDE
from openwhisk_amd import Action, GpuShardingContainerPoolBalancer
from test_gpu_resident import Shim

pytestmark = pytest.mark.gpu
MB = 1024 * 1024
RES_MAX = 1024  # OWGS_RES_MAX: the largest call (releases + publishes) the resident engine takes


# ------------------------------------------------------------------------------------------- part 1: the four routes
def _shim(name, wide=False, shadow=False):
    w = AC.workload(name, wide)
    sh = Shim(w, shadow=shadow)
    sh.jobs = AC.jobs(w)  # (Shim.call takes any job order; it resolves same-call releases through the oracle)
    return sh


def _call(sh, n):
    """one drained batch of n jobs: Shim.call's checks, and the route the library took"""
    runs = AC.n_runs(sh.jobs[sh.pos:sh.pos + n])
    r0, l0 = sh.g.resident_stats(), sh.g.large_stats()
    pubs, rels = sh.call(n)
    r1, l1 = sh.g.resident_stats(), sh.g.large_stats()
    rec = dict(jobs=n, runs=runs, pubs=pubs, rels=rels, large=(l1["launches"] - l0["launches"]) if l1 else 0)
    rec.update({k: r1[k] - r0[k] for k in ("served", "chained", "refused", "watch_calls")})
    return rec


def _drive(sh, lo, hi, seed, limit=None, before=None):
    """drains of lo..hi jobs over the first `limit` jobs (the cuts of arrival_cases.drains)"""
    rng = np.random.default_rng(seed)
    end = len(sh.jobs) if limit is None else min(limit, len(sh.jobs))
    recs = []
    while sh.pos < end:
        if before:
            before(sh, recs)
        n = min(int(rng.integers(lo, hi + 1)), end - sh.pos)
        if n > 0:
            recs.append(_call(sh, n))
    return recs


@pytest.mark.parametrize("name", list(AC.CASES))
def test_resident_engine_serves_arrival_order(name):
    """Drains of 1..600 jobs: every call on the resident engine, up to ~155 runs in one call.  A call with k runs that
    hold releases bumps the walk-cursor generation k times, so the sequence passes dozens of generation bumps per call
    (median 74 to 77 runs) where the stream-batch order of test_gpu_resident.py passes one to three; the helper waves'
    speculation of the next chunk crosses a run boundary in nearly every chunk."""
    sh = _shim(name)
    recs = _drive(sh, *AC.SMALL_DRAINS)
    assert sh.done() and sum(r["pubs"] for r in recs) == len(sh.w.stream.act)
    off = [r for r in recs if (r["served"], r["chained"], r["large"]) != (1, 0, 0)]
    assert not off, off[:3]  # (every call is eligible: identity pools, no watched pairs, at most 600 jobs)
    f = AC.facts(name, *AC.SMALL_DRAINS)
    assert [r["runs"] for r in recs].count(f["runs_max"]) >= 1 and len(recs) == f["calls"]  # the calls the CPU test saw
    assert max(r["runs"] for r in recs if r["served"]) >= 100
    assert min(r["runs"] for r in recs if r["served"]) <= 8 < np.median([r["runs"] for r in recs])
    st = sh.g.resident_stats()
    assert st["refused"] == 0, st
    assert np.array_equal(sh.g.permits(), sh.o.permits())


@pytest.mark.parametrize("name", list(AC.CASES))
def test_fused_chain_takes_arrival_order(name):
    """Drains of 1,025..4,095 jobs: beyond OWGS_RES_MAX, so the launch chain takes every call in one engine launch
    (no watched pairs, publishes in every call: the fused branch, not the per-run one) -- one staging workgroup per
    run, f_cnt of 2 x runs, and with more than PP_INLINE = 8 runs the chunk table and its binary search in the
    pre-pass, which no other test reaches through owgs_process_batch."""
    sh = _shim(name)
    recs = _drive(sh, *AC.LARGE_DRAINS)
    assert sh.done()
    big = [r for r in recs if r["jobs"] > RES_MAX]
    assert len(big) >= len(recs) - 1  # (only the queue's remainder can be a small call)
    off = [r for r in big if (r["served"], r["chained"], r["refused"], r["large"]) != (0, 1, 0, 0)]
    assert not off, off[:3]
    assert all(r["pubs"] > 0 and r["runs"] > 8 for r in big)
    assert max(r["runs"] for r in big) >= 512
    assert max(r["runs"] for r in recs) == AC.facts(name, *AC.LARGE_DRAINS)["runs_max"]
    assert np.array_equal(sh.g.permits(), sh.o.permits())


@pytest.mark.parametrize("name", ["a40", "b100"])
def test_per_run_path_takes_arrival_order(name):
    """The first 12,000 jobs in drains of 1,025..4,095, updateCluster(2) on both sides after a third of them: the
    concurrent activations in flight become watched pairs, and while any is left the chain takes a call run by run
    (process_runs: the exact release kernels, one engine launch and one watch update per run) -- here with hundreds
    of runs per call instead of at most three.

    The library exports no count of the watched pairs; `watch_calls` of resident_stats() counts the calls the
    resident engine served while there were any.  So a probe call of 24 jobs follows the change and every large call
    after it: watched pairs are only created by the change, so a large call between two probes that both counted is
    known to have run with watched pairs, that is on the per-run path."""
    sh = _shim(name, shadow=True)
    limit, at = 12_000, 4_000
    state = dict(changed=False, probes=[])

    def before(sh, recs):
        if not state["changed"] and sh.pos >= at:
            for b in (sh.g, sh.o, sh.z):
                b.update_cluster(2)
            state["changed"] = True
        if state["changed"]:
            state["probes"].append((len(recs), _call(sh, 24)["watch_calls"]))

    recs = _drive(sh, *AC.LARGE_DRAINS, limit=limit - 24, before=before)
    state["probes"].append((len(recs), _call(sh, 24)["watch_calls"]))
    probes = state["probes"]
    assert state["changed"] and probes[0][1] == 1, probes  # watched pairs exist after the change
    watched = [recs[i] for (i, a), (j, b) in zip(probes, probes[1:])
               if i < j and a == 1 and b == 1 and recs[i]["jobs"] > RES_MAX]
    print(name, "calls", [(r["jobs"], r["runs"], r["chained"]) for r in recs], "probes", probes)
    assert all((r["served"], r["chained"]) == (0, 1) for r in recs if r["jobs"] > RES_MAX), recs
    assert watched, probes
    assert max(r["runs"] for r in watched) >= 100, watched
    assert np.array_equal(sh.g.permits(), sh.o.permits())
    assert sh.z_rf != sh.o_rf  # releases that only the reference's empty entries explain were reached


@pytest.mark.parametrize("drains", [AC.SMALL_DRAINS, AC.LARGE_DRAINS], ids=["small", "large"])
@pytest.mark.parametrize("name", ["a40", "b100"])
def test_large_state_engine_takes_arrival_order(name, drains):
    """The same queues on a context that the never-invoked maxConcurrent 5000 action moves to the large-state engine
    (seq_host_runs): its groups of 64 decisions span the run boundaries, which come every two to four jobs."""
    sh = _shim(name, wide=True)
    assert sh.g.large_stats() is not None
    recs = _drive(sh, *drains)
    assert sh.done()
    off = [r for r in recs if r["served"] or r["chained"] or r["large"] < 1]
    assert not off, off[:3]
    assert max(r["runs"] for r in recs) >= (512 if drains is AC.LARGE_DRAINS else 100)
    ls = sh.g.large_stats()
    old = sh.g.stats()
    print(name, ls)
    assert ls["large_spec"] > 0 and ls["alone"] > 0, ls
    assert old["large_spec"] == ls["large_spec"] and old["large_alone"] == ls["alone"] > 0
    assert ls["large_spec"] + ls["alone"] + ls["none_kind"] + ls["throw_kind"] == sh.seq == len(sh.w.stream.act), ls
    assert np.array_equal(sh.g.permits(), sh.o.permits())


# ----------------------------------------------------------------------------------------- part 2: directed run shapes
# seven invokers, no blackbox pool; plain and concurrent actions, two of them under one fqn@version key.  About 217 MB
# per activation: 32 GB invokers hold about 1,000 of them, so that the calls of a test meet walks that find room at
# once, walks past full invokers and forced acquires; the tests with fewer activations in flight take smaller invokers.
N_INV, INV_MB = 7, 32_768
ACTS = [Action("ns0", "ns0/p/a0", "0.0.1", 128, 1), Action("ns1", "ns1/p/a1", "0.0.1", 256, 1),
        Action("ns2", "ns2/p/a2", "0.0.1", 512, 1), Action("ns0", "ns0/p/c3", "0.0.1", 256, 3),
        Action("ns1", "ns1/p/c4", "0.0.1", 512, 2), Action("ns2", "ns1/p/c4", "0.0.1", 512, 2),
        Action("ns2", "ns2/p/c6", "0.0.1", 128, 5)]


def _chunk_width(acts, inv_mb):
    """The chain's chunk width for this pool, from the capacity units as test_gpu_redecide_coop.py counts them
    (managed slot MB over the mean action MB; 448 from 60,000 units, 256 from 30,000, else 192)."""
    units = N_INV * inv_mb / np.mean([a.mem_mb for a in acts])
    return 448 if units >= 60_000 else 256 if units >= 30_000 else 192


class Pool:
    """The library and the literal oracle on the small pool.  call(runs) is one owgs_process_batch: runs =
    [(releases, publishes)], releases = a count (that many of the oldest activations in flight, those published
    earlier in the same call included) or a list of (invoker, action) taken as it is; publishes = action indices."""

    def __init__(self, large=False, inv_mb=INV_MB, seed=3):
        self.acts = ACTS + ([WIDE] if large else [])
        self.g = GpuShardingContainerPoolBalancer(managed_fraction=1.0, blackbox_fraction=0.0, rng_seed=seed)
        self.o = O.BalancerState(1.0, 0.0, rng_seed=seed, zombies=True)
        ids, mem = np.arange(N_INV, dtype=np.int32), np.full(N_INV, inv_mb * MB, np.int64)
        self.g.update_invokers_arrays(ids, mem, np.zeros(N_INV, np.uint8))
        self.o.update_invokers(ids, mem, np.zeros(N_INV, np.uint8))
        self.gh, _ = self.g.register_actions(self.acts)
        keys = {}
        self.key = [keys.setdefault(a.key, len(keys)) for a in self.acts]
        self.oh = [self.o.register_action(a.namespace, a.path, k, a.mem_mb, a.max_concurrent, a.blackbox)
                   for a, k in zip(self.acts, self.key)]
        self.large = large
        assert (self.g.large_stats() is not None) == large
        self.live = collections.deque()  # (invoker, action) of the activations in flight, oldest first
        self.forced = self.placed = 0    # publishes by the oracle's overload flag
        self.seq = 0
        self.rng = np.random.default_rng(seed)
        self.routes = []

    def pubs(self, n):
        return self.rng.integers(0, len(ACTS), size=n).tolist()

    def call(self, runs, seq_stride=1):
        ro, po, ri, ra, pa, sq, orf, oi = [0], [0], [], [], [], [], [], []
        for rels, pubs in runs:
            if isinstance(rels, int):
                assert len(self.live) >= rels, "the shape releases more than is in flight"
                rels = [self.live.popleft() for _ in range(rels)]
            for x, a in rels:
                ri.append(x)
                ra.append(int(self.gh[a]))
                orf.append(O._rel_bits(self.o.release(x, self.oh[a])) if x >= 0 else 4)  # OWGS_REL_NOENTRY
            for a in pubs:
                s = self.seq + seq_stride * len(pa)
                pa.append(int(self.gh[a]))
                sq.append(s)
                x, f = self.o.publish(self.oh[a], s)
                oi.append((int(x), int(f)))
                assert x >= 0
                self.live.append((int(x), a))
                self.forced += f & 1
                self.placed += not f & 1
            ro.append(len(ri))
            po.append(len(pa))
        r0, l0 = self.g.resident_stats(), self.g.large_stats()
        gi, gf, grf = self.g.process_batch(ro, ri, ra, po, pa, seq=None if seq_stride == 1 else np.array(sq, np.uint64),
                                           seq_base=self.seq)
        r1, l1 = self.g.resident_stats(), self.g.large_stats()
        self.seq += seq_stride * len(pa)
        assert grf.tolist() == orf, len(self.routes)
        assert [(int(x), int(f)) for x, f in zip(gi, gf)] == oi, len(self.routes)
        d = {k: r1[k] - r0[k] for k in ("served", "chained")}
        route = "large" if l1 and l1["launches"] > l0["launches"] else "resident" if d["served"] else "chain"
        assert (d["served"], d["chained"]) == {"large": (0, 0), "resident": (1, 0), "chain": (0, 1)}[route], d
        assert self.large == (route == "large")
        self.routes.append(route)
        return route

    def check_state(self):
        assert np.array_equal(self.g.permits(), self.o.permits())
        slots = self.o.invoker_slots
        for inv in range(N_INV):
            for a, act in enumerate(ACTS):
                if act.max_concurrent > 1:
                    got = self.g.concurrent_state(inv, self.g.key_id(int(self.gh[a])))
                    want = slots[inv].concurrent_state(self.key[a])
                    # the reference leaves an empty entry {0 free, 0 operations} where a concurrent try failed
                    # (NS:61-62).  The large-state engine keeps it; the on-chip engines keep none, since it only
                    # matters to a release after updateCluster, which the watched pairs stand for
                    if not self.large and want == (0, 0) and got is None:
                        continue
                    assert got == want, (inv, a, got, want)


def _expect(p, route, want):
    """on-chip contexts: the route the call's size asks for; a large-state context has one route"""
    assert route == ("large" if p.large else want), (route, want, p.routes)


NOENTRY = [(-1, 0), (-1, 3), (-1, 5)]
# shape -> (the small call, the same shape beyond OWGS_RES_MAX); p.pubs(n) draws n actions
SHAPES = {
    "one_run_of_releases_only": lambda p: ([(5, [])], [(1030, [])]),
    "one_run_of_publishes_only": lambda p: ([(0, p.pubs(7))], [(0, p.pubs(1030))]),
    "five_runs_first_middle_last_empty": lambda p: (
        [(0, []), (3, p.pubs(4)), (0, []), (2, p.pubs(3)), (0, [])],
        [(0, []), (400, p.pubs(400)), (0, []), (200, p.pubs(300)), (0, [])]),
    "releases_only_then_publishes_only": lambda p: ([(4, []), (0, p.pubs(5))], [(600, []), (0, p.pubs(600))]),
    "every_release_without_an_entry": lambda p: (
        [(NOENTRY, p.pubs(4)), (NOENTRY[:2], p.pubs(3))],
        [(NOENTRY * 200, p.pubs(300)), (NOENTRY * 70, p.pubs(100))]),
}


@pytest.mark.parametrize("large", [False, True], ids=["onchip", "large"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_run_shapes(shape, large):
    """Each shape as a small call (the resident engine takes it) and beyond 1,024 jobs (the chain takes it: fused, or
    run by run for a call without publishes), with activations in flight before and an ordinary call after."""
    p = Pool(large)
    p.call([(0, p.pubs(300))])
    small, padded = SHAPES[shape](p)
    _expect(p, p.call(small), "resident")
    p.check_state()
    p.call([(0, p.pubs(900))])  # (enough in flight for the padded call's releases)
    assert sum((r if isinstance(r, int) else len(r)) + len(q) for r, q in padded) > RES_MAX
    _expect(p, p.call(padded), "chain")
    p.check_state()
    p.call([(40, p.pubs(30)), (20, p.pubs(50))])
    p.check_state()
    assert p.placed > 300, (p.placed, p.forced)


@pytest.mark.parametrize("large", [False, True], ids=["onchip", "large"])
@pytest.mark.parametrize("n_runs", [8, 9])
def test_prepass_threshold(n_runs, large):
    """Exactly 8 and exactly 9 runs in a call beyond 1,024 jobs: with up to PP_INLINE = 8 batches every pre-pass
    workgroup walks the chunk counts itself, with more it searches the chunk table owgs_chunks_kernel built."""
    p = Pool(large, inv_mb=6144)  # (about 200 activations fit: the calls run on a full pool)
    p.call([(0, p.pubs(200))])
    runs = [(65, p.pubs(70)) for _ in range(n_runs)]
    assert len(runs) == n_runs and 135 * n_runs > RES_MAX
    _expect(p, p.call(runs), "chain")
    p.check_state()
    # ... and the same number of runs with empty ones among them (batches without a chunk on either side)
    runs = [(65, p.pubs(140)) if r % 2 else (70, []) for r in range(n_runs)]
    assert sum(r + len(q) for r, q in runs) > RES_MAX
    _expect(p, p.call(runs), "chain")
    p.check_state()
    assert p.placed > 100 and p.forced > 100, (p.placed, p.forced)


@pytest.mark.parametrize("large", [False, True], ids=["onchip", "large"])
@pytest.mark.parametrize("extra", [0, 1])
def test_chunk_width_edges(extra, large):
    """A run of exactly one chunk width of publishes, and of one more, as the second of three runs: small (resident
    engine, whose speculation unit of 64 divides the width) and beyond 1,024 jobs (the chain's pre-pass, whose chunk
    count shows the width the library used)."""
    inv_mb = 6144  # (the run of one width fills the pool)
    cw = _chunk_width(ACTS + ([WIDE] if large else []), inv_mb)
    p = Pool(large, inv_mb=inv_mb)
    p.call([(0, p.pubs(20))])
    _expect(p, p.call([(2, p.pubs(3)), (3, p.pubs(cw + extra)), (2, p.pubs(3))]), "resident")
    p.check_state()
    p.call([(0, p.pubs(500))])
    _expect(p, p.call([(400, p.pubs(450)), (3, p.pubs(cw + extra)), (2, p.pubs(3))]), "chain")
    if not large:  # the last engine launch's chunks: ceil(450 / cw) + 1 (+ 1 past the width) + 1
        chunks = p.g.stats()["chunks"]
        print("chunk width", cw, "chunks", chunks)
        assert chunks == -(-450 // cw) + 1 + extra + 1, (cw, chunks)
    p.check_state()
    assert p.placed > 100 and p.forced > 100, (p.placed, p.forced)


@pytest.mark.parametrize("large", [False, True], ids=["onchip", "large"])
def test_largest_resident_block(large):
    """1,024 jobs as 512 runs of one release and one publish, each release naming the publish two runs before it: the
    offset arrays alone take 8 x 516 bytes of the call block, past the resident engine's first 4 KB read, and every
    run bumps the cursor generation.  The call is within OWGS_RES_MAX and its block fits the staging area, so the
    resident engine serves it (route asserted below); then once more with explicit sequence numbers three apart."""
    p = Pool(large, inv_mb=256)  # (the 512 MB actions never fit, the others meet two or three activations in flight)
    p.call([(0, p.pubs(2))])
    _expect(p, p.call([(1, [a]) for a in p.pubs(512)]), "resident")
    assert len(p.live) == 2
    p.check_state()
    _expect(p, p.call([(1, [a]) for a in p.pubs(512)], seq_stride=3), "resident")
    p.check_state()
    p.call([(2, p.pubs(40))])
    p.check_state()
    assert p.placed > 100 and p.forced > 100, (p.placed, p.forced)
