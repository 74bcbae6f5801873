"""The inputs of the entry pre-find's GPU cases (tests/entry_prefind_cases.py), checked on the CPU: for every case the
oracle's decisions alone show the condition that makes the case worth running on the GPU.  A change to
openwhisk_amd/workload.py that quietly empties a case fails here, on a machine without a GPU.

Figures observed with the default seeds (192-lane chunks; `pytest -s` prints them):

| id | batches | chunks | absent-entry lanes per chunk (mean) | chunks over 64 | most lanes on one absent key | live entries (max) | forced |
|----|---------|--------|-------------------------------------|----------------|------------------------------|--------------------|--------|
| A  | 4       | 32     | 151                                 | 32             |                              |                    |        |
| B  | 4       | 32     |                                     |                | 72                           |                    |        |
| C  | 3       |        |                                     |                |                              | 7,943              |        |
| D  |         |        |                                     |                |                              |                    | 734    |
"""
import pytest

import entry_prefind_cases as PC


@pytest.fixture(scope="module", params=list(PC.CASES))
def case(request):
    return request.param, PC.facts(request.param)


def test_every_case_has_concurrent_decisions_on_absent_entries(case):
    name, f = case
    print(name, f)  # (pytest -s: the figures of the table above)
    assert f["batches"] >= 3 and f["absent_mean"] > 0, (name, f)


def test_a_fills_more_than_one_round_in_most_chunks():
    f = PC.facts("A")
    assert 2 * f["chunks_over_64"] >= f["chunks"], f  # over PF_CAP = 64 lanes in at least half the chunks


def test_b_puts_many_lanes_on_one_absent_key():
    assert PC.facts("B")["same_key_max"] >= 65, PC.facts("B")  # more than one round's lanes on one key


def test_c_outgrows_the_on_chip_table():
    assert PC.facts("C")["live_max"] > 3840, PC.facts("C")  # OWGS_CT_LDS_FILL = 4096 - 256


def test_d_has_forced_acquires():
    f = PC.facts("D")
    assert f["forced"] > 0 and f["forced_conc"] > 0, f
