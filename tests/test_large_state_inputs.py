"""The inputs of the large-state engine's small-pool sweep (tests/large_state_cases.py), checked on the CPU: for every
case the literal oracle alone shows the condition that makes the case worth running on the GPU -- pool sizes on the
engine's thresholds, forced acquires of the kind the case is about, a map that must grow inside one replay.  A change
to openwhisk_amd/workload.py that quietly empties a case fails here, on a machine without a GPU.

Oracle figures observed with the default headline seed (nm / nb = managed / blackbox pool positions; entries = the
NestedSemaphore maps' entries at the end, empty ones included, summed with concurrent_size()):

| id   | pools         | batches     | releases | forced (plain / concurrent; on the blackbox pool) | entries |
|------|---------------|-------------|----------|---------------------------------------------------|---------|
| p40  | nm 36, nb 4   | 69 of 291   | 18,893   | 11,978 (11,576 / 402; 0)                          | 1,857   |
| p17  | nm 16, nb 1   | 1,000 of 20 | 19,929   | 5,626 (3,317 / 2,309; 2,082)                      | 1,157   |
| p64  | nm 64, nb 7   | 56 of 360   | 18,709   | 4,136 (4,136 / 0; 0)                              | 0       |
| p65  | nm 66, nb 7   | 36 of 559   | 17,880   | 5,005 (4,985 / 20; 0)                             | 758     |
| p300 | nm 270, nb 30 | 83 of 725   | 57,243   | 4,295 (0 / 4,295; 612)                            | 91,165  |
| p600 | nm 540, nb 60 | 142 of 283  | 39,073   | 4,875 (4,479 / 396; 483)                          | 14,854  |

No case has a None outcome.  `pytest -s` prints every case's figures (the first test below)."""
import pytest

import large_state_cases as LC

IDS = list(LC.CASES)


@pytest.fixture(scope="module", params=IDS)
def case(request):
    return request.param, LC.facts(request.param)


def test_every_case_has_batches_and_releases(case):
    name, f = case
    print(name, f)  # (pytest -s: the figures of the table above)
    assert f["batches"] >= 3 and f["releases"] > 10_000, (name, f)


def test_the_wide_action_is_registered_last_and_never_invoked(case):
    name, _ = case
    w = LC.workload(name)
    assert w.actions[-1] == LC.WIDE and w.actions[-1].max_concurrent > 4095
    assert int(w.stream.act.max()) < len(w.actions) - 1


def test_pool_sizes_sit_on_the_engine_thresholds():
    # SEQ_SPEC_C = 16: concurrent speculation needs a pool of more than 16 positions; SEQ_SPEC = 64: the plain budget
    assert LC.facts("p17")["nm"] == 16 and LC.facts("p17")["nb"] == 1
    assert LC.facts("p64")["nm"] == 64
    assert LC.facts("p65")["nm"] > 64 and (LC.facts("p65")["nm"] % 32) != 0  # (the blackbox pool's first id)
    assert LC.facts("p40")["nm"] > 16 and LC.facts("p40")["nb"] > 0


def test_forced_acquires_of_the_kind_each_case_is_about():
    assert LC.facts("p40")["forced_plain"] > 0 and LC.facts("p40")["forced_conc"] > 0
    assert LC.facts("p64")["forced_plain"] > 0 and LC.facts("p64")["forced_conc"] == 0
    assert LC.facts("p17")["forced_conc"] > 0 and LC.facts("p17")["forced_blackbox"] > 0
    assert LC.facts("p65")["forced"] > 0
    assert LC.facts("p300")["forced_conc"] > 0 and LC.facts("p300")["forced_plain"] == 0
    assert LC.facts("p600")["forced"] > 0


def test_p300_map_must_grow_inside_one_replay():
    # the large map starts at 65,536 entries and is kept under half full: more than 40,000 entries at the end means
    # the engine stopped for it to grow, and resumed, inside the replay
    assert LC.facts("p300")["entries"] > 40_000
