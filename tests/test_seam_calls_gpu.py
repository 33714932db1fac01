"""The Python seam above the C ABI (srlz/ops.py, srlz/hotpath.py) enqueues what it enqueued when tests/golden/seam_calls.json was
recorded (tools/seam_trace.py: the scenarios, what is logged of a call and what is not): the same entry points in the same order with
the same descriptors, sizes, scalars and null / non-null pointers, on every route — the default step on bytes and on floats with its
timer report, the plain chain under hotpath.TAPS, each fusion switch cleared, the VAE + perceptual step, an eval forward, the ResNet-18
trunk on both 64 -> 64 kernels, and two kernel-level cases for entry points no model-level step reaches.  Equality is exact.

The workspace sizes in the trace depend on the number of compute units: the fixture is valid on MI355X only.  It is a record of the
sources it was taken from and is never re-recorded to make a change of the seam pass; a change that means to alter a launch sequence
states the difference it expects."""
import json

import pytest
import torch  # noqa: F401  (before srlz._cabi, as in every GPU test: one HIP runtime per process)

from tools import seam_trace as ST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(ST.FIXTURE) as f:
        return ST.unpack(json.load(f))


def test_fixture_covers_every_entry_point_of_the_seam(recorded):
    assert sorted(recorded) == sorted(name for name, _ in ST.SCENARIOS)
    seen = {call[0] for res in recorded.values() for call in res["calls"]}
    assert set(ST.SEAM_ENTRY_POINTS) <= set(ST.enqueueing())
    assert not set(ST.SEAM_ENTRY_POINTS) - seen, sorted(set(ST.SEAM_ENTRY_POINTS) - seen)


@pytest.mark.parametrize("name", [name for name, _ in ST.SCENARIOS])
def test_seam_enqueues_the_recorded_calls(recorded, name):
    got, want = ST.plain(dict(ST.SCENARIOS)[name]()), recorded[name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, "call %d of %s:\n got  %s\n want %s" % (i, name, g, w)
    assert len(got["calls"]) == len(want["calls"])
    assert got.get("timers") == want.get("timers")
