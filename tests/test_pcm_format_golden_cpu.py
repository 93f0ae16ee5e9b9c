"""The host functions of the PCM format section (csrc/dsm_pcm_format.h; no GPU) against tests/golden/pcm_format.json: the
SHA-256 digests tools/make_pcm_format_golden.py recorded from the library of the commit before ingest and egress were folded
into one definition.  dsm_ingest_host and dsm_egress_host over seeded frames — every common rate, three odd ones, every format,
the extremes, a format change — the descriptor words of every admitted rate, the return codes of refused ones and dsm_resample:
not a bit of them has moved.  The GPU tests then carry that over to the two kernels, which they compare with the host."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pcm_format_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def recomputed(lib):
    return G.compute(G.load(lib._name))


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden):
    assert len(golden["ingest"]) == 4 * len(G.INGEST_RATES) == 44
    assert len(golden["egress"]) == 4 * len(G.EGRESS_RATES) + 1 == 41 and "switch" in golden["egress"]
    assert set(golden["describe"]) == set(golden["refused"]) == {"ingest", "egress"}
    assert all(len(r) == len(G.REFUSED) and all(rc == -1 for rc in r.values()) for r in golden["refused"].values())
    assert len(golden["resample"]) == 14
    assert golden["describe"]["ingest"] != golden["describe"]["egress"]  # the two directions are not each other's words


@pytest.mark.parametrize("part", ["ingest", "egress", "describe", "refused", "resample"])
def test_host_functions_give_the_recorded_bits(golden, recomputed, part):
    assert G.differences(golden[part], recomputed[part], part) == []
