"""The bounds of _lstm_seq_cases.py do not pass vacuously (CPU): an fp32
emulation of both whole-sequence LSTM routes fits them at every case, and
every mutant of that emulation breaks them wherever something recurs."""

import pytest

import _lstm_seq_cases as C
from _bf16_bounds import assert_within, violations

_cache = {}


def _inputs(shape):
    if shape not in _cache:
        _cache[shape] = C.inputs(*shape)
    return _cache[shape]


@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_seq_bounds_hold_for_the_emulation(run):
    shape, route, forced = run
    route = C.run_route(route, forced)
    inp = _inputs(shape)
    out = C.emulate(inp, route)
    assert_within(out, C.oracle(inp, out, route), f"emulated {C.run_id(run)}")


# T = 1 and T = 2 are left out: at T = 1 nothing recurs, and the T = 2
# cases have no mid-sequence reset (cont[2] does not exist), so the cont
# gates on c and dh act on nothing there.
RECURRENT = [r for r in C.RUNS if r[0][0] >= 3]


def test_enough_recurrent_cases():
    assert len({r[0] for r in RECURRENT}) >= 5


@pytest.mark.parametrize("mutant", C.MUTANTS)
@pytest.mark.parametrize("run", RECURRENT, ids=C.run_id)
def test_seq_bounds_catch_mutants(run, mutant):
    shape, route, forced = run
    route = C.run_route(route, forced)
    inp = _inputs(shape)
    out = C.emulate(inp, route, mutant)
    bad = violations(out, C.oracle(inp, out, route))
    if C.tail_is_empty(mutant, shape[2]):
        # H a multiple of the tile: the dropped tail holds nothing, the
        # mutant is the honest emulation and must still fit
        assert not bad, bad
    else:
        assert bad, f"{mutant} fits the bounds at {C.run_id(run)}"


@pytest.mark.parametrize("mutant", ["k_tail_dropped", "slice_tail_dropped"])
def test_tail_mutants_at_the_full_window_widths(mutant):
    """H = 1024 has no tail, H = 1032 has both; T = 2 is enough for these
    two, which do not depend on a reset."""
    inp = _inputs((2, 2, 1024))
    out = C.emulate(inp, "persist", mutant)
    assert not violations(out, C.oracle(inp, out, "persist"))
    inp = _inputs((2, 2, 1032))
    out = C.emulate(inp, "loop", mutant)
    assert violations(out, C.oracle(inp, out, "loop"))
