"""How many machine streams a run keeps in rotation (h2g_mstreams_policy in h2g_kernels.hip, a pure host function): its table of cases, through the library.
No GPU: the function touches no device."""
import pytest

from hisat2_amd import api

MAX = 8


@pytest.mark.parametrize("units, bails, linear, pinned, light, want", [
    # pinned: the value itself, whatever the load and the index
    (1_000_000, 0, True, 8, 2, 8),
    (1_000_000, 500_000, True, 1, 2, 1),
    (1_000_000, 0, False, 3, 2, 3),
    (1_000_000, 0, True, 99, 2, MAX),
    # a graph index: every lane its own stream
    (1_000_000, 0, False, 0, 2, MAX),
    (10, 0, False, 0, 1, MAX),
    # a linear index, light: nothing finished yet, the headline's 0.8 %, exactly 1.5 % (the regime is "more than")
    (1_000_000, 0, True, 0, 2, 2),
    (1_000_000, 8_000, True, 0, 2, 2),
    (1_000_000, 15_000, True, 0, 2, 2),
    (1_000_000, 15_000, True, 0, 1, 1),
    (1_000_000, 15_000, True, 0, 3, 3),
    (0, 0, True, 0, 2, 2),
    # ... heavy from the first hand-on beyond 1.5 %; the count is weighed against THIS batch's units
    (1_000_000, 15_001, True, 0, 2, MAX),
    (1_000_000, 27_000, True, 0, 1, MAX),
    (60_000, 901, True, 0, 2, MAX),
    (60_000, 900, True, 0, 2, 2),
    (0, 1, True, 0, 2, MAX),
    # no 32-bit wrap in the comparison: 2^32 - 1 hand-ons against 2^33 units is 50 %
    (1 << 33, (1 << 32) - 1, True, 0, 2, MAX),
    ((1 << 40), (1 << 32) - 1, True, 0, 2, 2),
    # the light value is kept inside 1 .. 8
    (1_000_000, 0, True, 0, 0, 1),
    (1_000_000, 0, True, 0, 99, MAX),
])
def test_policy_table(units, bails, linear, pinned, light, want):
    assert api.mstreams_policy(units, bails, linear, pinned, light) == want
