"""Host side of the tile plan's row-end tables (csrc/pair_plan.hpp, no GPU): how many buffer shells a displacement bound
selects."""
import math

import pytest

from azplugins_amd import _lib


def _brute(width, has_bound, bound, shells):
    """The statement: without a usable bound or width every shell; else the smallest n with n x width >= 2 x bound,
    at most all of them."""
    if not has_bound or math.isnan(bound) or bound < 0.0:
        return shells
    if bound == 0.0:
        return 0
    if not width > 0.0:
        return shells
    n = 0
    while n < shells and n * width < 2.0 * bound:
        n += 1
    return n


@pytest.mark.parametrize("width", [0.05, 0.025, 0.4 / 8, 0.3 / 16, 1e-3, 7.0])
def test_plan_shells_for_matches_the_statement(width):
    f = _lib.lib().azp_pair_plan_shells_for
    S = int(_lib.lib().azp_pair_plan_shells())
    for n in range(0, S + 3):
        # inside shell n's range, just below and just above its upper edge (the library's own guard against a rounded
        # quotient is 1e-12, far inside these offsets)
        for k in (n - 0.5, n - 1e-6, n + 1e-6):
            bound = 0.5 * k * width
            if bound <= 0.0:
                continue
            assert f(width, 1, bound) == _brute(width, True, bound, S), (width, n, k)
    assert f(width, 1, 0.0) == 0
    assert f(width, 1, 1e-300) == 1
    assert f(width, 1, 1e300) == S and f(width, 1, math.inf) == S


def test_plan_shells_for_without_a_usable_bound_or_width():
    f = _lib.lib().azp_pair_plan_shells_for
    S = int(_lib.lib().azp_pair_plan_shells())
    for width in (0.05, 0.0, -1.0, math.nan):
        assert f(width, 0, 0.01) == S            # no bound given
        assert f(width, 1, math.nan) == S
        assert f(width, 1, -0.01) == S and f(width, 1, -math.inf) == S
        assert f(width, 1, 0.0) == 0             # nothing moved: no buffer entry can be in range, whatever the width
        assert f(width, 1, -0.0) == 0
    for width in (0.0, -1.0, math.nan):          # no shells (no r_list_max hint at build time): whole rows once anything moved
        assert f(width, 1, 1e-9) == S == _brute(width, True, 1e-9, S)
