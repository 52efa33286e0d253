"""The LDS rules of `trs_adjoint_fits`, `trs_recover_cases_fits`, `trs_effects_fits` and `trs_modes_fits` to the byte
(no GPU): what each kernel keeps in LDS, written out here, rounded up to 16 bytes, against the 160 KB of a CU - on
shapes on both sides of the limit.  (The other analyses pin theirs in their own test files.)"""
import pytest

from python_stable_3d_truss_analysis_amd import _capi

BUDGET = 160 * 1024
round16 = lambda nbytes: (nbytes + 15) // 16 * 16
# the member-end lists of every joint: cnt [nJ], start [nJ + 1], ends [2 nM], int32
end_lists = lambda nJ, nM: 4 * (2 * nJ + 1 + 2 * nM)
RULES = {
    # two DOF vectors, one double per member, the end lists
    "trs_adjoint_fits": lambda nJ, nM: round16(8 * (6 * nJ + nM) + end_lists(nJ, nM)),
    # one DOF vector, the end lists
    "trs_recover_cases_fits": lambda nJ, nM: round16(8 * 3 * nJ + end_lists(nJ, nM)),
    # one DOF vector, one double per member, the end lists
    "trs_effects_fits": lambda nJ, nM: round16(8 * (3 * nJ + nM) + end_lists(nJ, nM)),
    # one double and one pair of end joints per member, one counter; no joint table
    "trs_modes_fits": lambda nJ, nM: 16 * nM + 16,
}


def largest(fits):
    """The largest n >= 0 with fits(n), for a monotone rule that holds at 0."""
    lo, hi = 0, 1
    while fits(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("name", sorted(RULES))
def test_fits_rule_in_bytes(name):
    lib, rule = _capi.load(), RULES[name]
    fits = getattr(lib, name)
    assert fits(244, 942) == 1 and rule(244, 942) <= BUDGET
    assert fits(-1, 4) == 0 and fits(4, -1) == 0
    seen = set()
    # the last member that fits beside nJ joints, and its neighbours
    for nJ in (0, 1, 7, 100, 244, 1000, 2000, 2925, 4000):
        if rule(nJ, 0) > BUDGET:   # (the joints alone are too many)
            assert fits(nJ, 0) == 0
            continue
        top = largest(lambda nM: rule(nJ, nM) <= BUDGET)
        assert rule(nJ, top) <= BUDGET < rule(nJ, top + 1)
        for nM in range(max(top - 3, 0), top + 5):
            assert fits(nJ, nM) == int(rule(nJ, nM) <= BUDGET), (nJ, nM, rule(nJ, nM))
            seen.add(fits(nJ, nM))
    # the last joint that fits beside nM members (the mass kernel keeps nothing per joint)
    for nM in (0, 1, 5, 942, 3000, 7000):
        if rule(0, nM) == rule(1 << 16, nM):
            assert fits(1 << 16, nM) == 1
            continue
        top = largest(lambda nJ: rule(nJ, nM) <= BUDGET)
        assert rule(top, nM) <= BUDGET < rule(top + 1, nM)
        for nJ in range(max(top - 3, 0), top + 5):
            assert fits(nJ, nM) == int(rule(nJ, nM) <= BUDGET), (nJ, nM, rule(nJ, nM))
            seen.add(fits(nJ, nM))
    assert seen == {0, 1}
