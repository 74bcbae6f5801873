"""The inputs of the arrival-order parity tests (tests/arrival_cases.py), checked on the CPU: the literal oracle alone,
driven through the same drains as test_gpu_arrival_order.py, shows that the calls have the shape those tests exist for
-- dozens to hundreds of runs per call, completions that name an activation published earlier in the same call, forced
acquires of both kinds.  These are conditions on the inputs, not measurements of the code under test: a change to
openwhisk_amd/workload.py that flattens a case fails here, on a machine without a GPU.

Observed with the default headline seed, interleave seed 7, drains of 1..600 jobs from seed 1 and of 1,025..4,095 jobs
from seed 2 (batch = the capacity-calibrated stream batch; same-call = releases naming an activation published earlier
in the same call; no case has a rejected release):

| case | batch | small: calls, runs median / max / min, share > 8 | same-call (conc.) | forced (conc.) | large: calls, runs median / max |
|------|-------|--------------------------------------------------|-------------------|----------------|---------------------------------|
| a40  | 61    | 129, 75 / 153 / 2, 0.96                          | 4,441 (848)       | 6,250 (464)    | 16, 589 / 1,018                 |
| b100 | 90    | 129, 77 / 155 / 2, 0.94                          | 2,348 (1,272)     | 1,893 (465)    | 16, 585 / 1,022                 |
| c200 | 147   | 128, 74 / 157 / 2, 0.96                          | 664 (0)           | 3,825 (0)      | 16, 595 / 1,005                 |

`pytest -s` prints every case's figures (the first test below)."""
import pytest

import arrival_cases as AC

IDS = list(AC.CASES)


@pytest.fixture(scope="module", params=IDS)
def case(request):
    return request.param, AC.facts(request.param, *AC.SMALL_DRAINS), AC.facts(request.param, *AC.LARGE_DRAINS)


def test_the_stream_batch_is_small_and_a_drain_spans_several(case):
    name, small, large = case
    print(name, "small drains", small)  # (pytest -s: the figures of the table above)
    print(name, "large drains", large)
    assert 60 <= small["batch"] <= 150, (name, small)
    assert small["jobs"] > 30_000 and small["releases"] > 15_000, (name, small)


def test_the_interleave_keeps_the_order_inside_each_kind_and_stays_causal():
    for name in IDS:
        w = AC.workload(name)
        q = AC.jobs(w)
        s = w.stream
        assert [a for k, a in q if k == 1] == list(range(len(s.act)))
        assert [a for k, a in q if k == 0] == s.rel_aid.tolist()
        published = set()
        for k, a in q:
            if k == 1:
                published.add(a)
            else:
                assert a in published, (name, a)
        # ... and it is an interleave: neither kind stands in one block per stream batch
        b0 = q[:int(s.acq_off[3] + s.rel_off[3])]
        assert AC.n_runs(b0) > 12, name
        assert AC.jobs(w) == q and AC.jobs(w, seed=8) != q  # seeded


def test_small_drains_hold_dozens_of_runs(case):
    name, f, _ = case
    assert f["runs_median"] >= 32, (name, f)
    assert f["runs_max"] >= 128, (name, f)
    assert f["share_over_8"] >= 0.90, (name, f)
    assert f["runs_min"] <= 8, (name, f)  # at least one call on the pre-pass's inline side (PP_INLINE = 8)


def test_large_drains_hold_hundreds_of_runs(case):
    name, _, f = case
    assert f["runs_max"] >= 512, (name, f)
    assert f["calls"] >= 10, (name, f)


def test_releases_name_activations_of_the_same_call(case):
    name, f, _ = case
    assert f["same_call"] >= 500, (name, f)
    if name in ("a40", "b100"):
        assert f["same_call_conc"] >= 100, (name, f)


def test_forced_acquires_of_both_kinds(case):
    name, f, _ = case
    assert f["forced"] >= 1000, (name, f)
    if name in ("a40", "b100"):
        assert f["forced_conc"] >= 100, (name, f)
    else:
        assert f["forced_conc"] == 0 and f["same_call_conc"] == 0, (name, f)  # c200: plain actions only


def test_n_runs_counts_as_the_shim_cuts():
    r, p = (0, 0), (1, 0)
    assert AC.n_runs([]) == 0
    assert AC.n_runs([r, r, r]) == 1 and AC.n_runs([p, p]) == 1 and AC.n_runs([r, p]) == 1
    assert AC.n_runs([p, r]) == 2 and AC.n_runs([r, p, r, p, p, r]) == 3
