"""CPU checks of the yardstick test_fc_stream_gpu.py holds gemm_fc_kernel
to: the fp32 emulation of the slab split-K scheme sits inside the float64
derived bound for every case and class, and each mutant of it falls outside
in at least one case (so the bound can tell them apart)."""

import pytest

import _fc_stream_cases as FC
from _bf16_bounds import violations
from _gemm_bounds import within

_cache = {}


def _case(name, cls):
    """(inputs, oracle) of a case, computed once and shared."""
    key = (name, cls)
    if key not in _cache:
        c = FC.FC_CASES[name]
        seed = 900 + 2 * list(FC.FC_CASES).index(name) + \
            FC.CLASSES.index(cls)
        inp = FC.fc_inputs(c, cls, seed)
        orc, peak = FC.fc_oracle(c, inp)
        if cls == "exact":
            assert peak <= 256, "exact-class precondition"
        _cache[key] = (inp, orc)
    return _cache[key]


@pytest.mark.parametrize("cls", FC.CLASSES)
@pytest.mark.parametrize("name", list(FC.FC_CASES))
def test_emulation_within_bound(name, cls):
    inp, orc = _case(name, cls)
    within(FC.fc_emulate(FC.FC_CASES[name], inp), orc, f"{name}/{cls}")


@pytest.mark.parametrize("mutant", FC.FC_MUTANTS)
def test_mutant_falls_outside(mutant):
    caught = []
    for name, c in FC.FC_CASES.items():
        for cls in FC.CLASSES:
            inp, orc = _case(name, cls)
            if violations(FC.fc_emulate(c, inp, mutant=mutant), orc):
                caught.append(f"{name}/{cls}")
    print(f"{mutant}: caught in {len(caught)} cases")
    assert caught, f"mutant {mutant} passes every case"


def test_table_covers_the_axes():
    cs = FC.FC_CASES.values()
    assert {c["M"] for c in cs} == set(FC.MS)
    assert {c["N"] for c in cs} == set(FC.NS) | {10, 500}
    assert {c["K"] for c in cs} == set(FC.KS) | {800}
    assert {c["sk"] for c in cs} == set(FC.SKS)
    assert {(c["bias"], c["relu"]) for c in cs} == \
        {(a, b) for a in (False, True) for b in (False, True)}
    # a ragged last split and a split of a single K tile
    ks, z = FC.split_k(1000, 7)
    assert z == 7 and 1000 - 6 * ks not in (0, ks)
    assert FC.split_k(64, 7) == (32, 2)
