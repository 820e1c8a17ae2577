"""GPU: every kernel instance of the planar FCN engine against the oracle and its plain twins (bodies and the table:
tests/fcn_instance_checks.py).  One parameter per configuration and frame size, so that a fault names the instance's configuration:
40x56 is three and a half 16-column tiles (a 16 x 32 tile overhangs the frame), 67x131 is odd at every pyramid level with several workgroups per layer."""
import pytest

import fcn_instance_checks as ic

pytestmark = pytest.mark.gpu

SIZES = ((40, 56), (67, 131))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", [c.name for c in ic.configurations()])
def test_configuration_vs_oracle_and_twins(hip_lib, monkeypatch, name, size):
    cfg = {c.name: c for c in ic.configurations()}[name]
    ic.check_config(hip_lib, cfg, *size, monkeypatch)
