"""
The table of device entry points (``tests/device_cases.py``) names every one of them.

Membership is decided by the source-text rule of ``device_cases.symbols_reached``, the rule of
``test_the_table_names_every_device_entry_point_of_the_binding`` in tests/test_gpu_scribble.py
followed one step further: not "the name of the Python function stands in the file" but "the
functions a case's ``run`` calls, followed through the package by their names, hold the C symbol".
No library is loaded and no device is needed.  A ``_dev`` symbol that is added to
``backend.SIGNATURES`` without a case and without an entry in ``device_cases.ALLOWED`` fails
``test_every_device_symbol_of_the_binding_is_reached_by_a_case``.
"""
import device_cases as D
from hydrodem_amd import backend as B


def device_symbols(signatures):
    return {name for name in signatures if name.endswith("_dev")}


def unreached(signatures, entries, allowed):
    reached = set()
    for entry in entries:
        reached |= D.symbols_reached(entry.case)
    return sorted(device_symbols(signatures) - reached - set(allowed))


def test_case_names_are_unique_and_every_case_is_whole():
    names = [entry.case.name for entry in D.ENTRIES]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    for entry in D.ENTRIES:
        case = entry.case
        assert callable(case.build) and callable(case.run) and callable(case.check), case.name
        assert entry.shapes and all(len(shape) == 2 for shape in entry.shapes), case.name
    assert len(D.PARAMS) == len(set(D.IDS))


def test_every_device_symbol_of_the_binding_is_reached_by_a_case():
    assert len(device_symbols(B.SIGNATURES)) >= 50          # (the rule sees the table at all)
    assert unreached(B.SIGNATURES, D.ENTRIES, D.ALLOWED) == []


def test_the_allowlist_holds_only_symbols_that_exist_and_that_no_case_reaches():
    for name, reason in D.ALLOWED.items():
        assert name in B.SIGNATURES and reason.strip(), name
    assert unreached(B.SIGNATURES, D.ENTRIES, {}) == sorted(D.ALLOWED)


def test_a_symbol_added_without_a_case_is_found():
    later = dict(B.SIGNATURES, hdem_something_new_u8_dev=[])
    assert unreached(later, D.ENTRIES, D.ALLOWED) == ["hdem_something_new_u8_dev"]
    # and a case that is taken out leaves its symbols behind
    without = [entry for entry in D.ENTRIES if not entry.case.name.startswith("quadratic-")]
    assert unreached(B.SIGNATURES, without, D.ALLOWED) == ["hdem_quadratic_f32_dev"]


def test_each_case_reaches_a_device_symbol_of_its_own_operator():
    """The rule follows names, so it can only claim too much through a name that many functions
    share; a case that reached no ``_dev`` symbol at all, or every one, would show that."""
    everything = device_symbols(B.SIGNATURES)
    for entry in D.ENTRIES:
        mine = D.symbols_reached(entry.case) & everything
        assert 1 <= len(mine) <= 6, (entry.case.name, sorted(mine))
