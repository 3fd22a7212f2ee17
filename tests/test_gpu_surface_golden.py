"""Every configuration of surface_golden.py -- one compress and one decompress of a 19-frame clip each -- gives the recorded container
(canonical hash, length, record types), last_* attributes, decoded frames and integrity report (tests/golden/surface_containers.json,
written by tools/gen_surface_golden.py on the commit before the surface was split into options, rules and stages)."""
import pytest

import surface_golden as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return sg.load(sg.CONTAINERS)["entries"]


def test_the_fixture_names_exactly_the_configurations(recorded):
    assert sorted(recorded) == sorted(name for name, _, _, _ in sg.CONFIGS)
    for a, b in sg.SAME_BYTES:
        assert recorded[a]["canonical_sha256"] == recorded[b]["canonical_sha256"], (a, b)


@pytest.mark.parametrize("name", [c[0] for c in sg.CONFIGS])
def test_configuration_equals_the_recorded_entry(recorded, name):
    got = sg.run_config(name)
    assert got == recorded[name]
