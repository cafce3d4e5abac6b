"""
The drop-in seam (SURVEY 8b "What calls it"): every import statement the
reference's own modules and tests make against ``filters``, ``sliding_window``
and ``exceptions`` -- listed, with file:line, in
tests/golden/reference_imports.json (made by parsing the reference,
tests/golden/make_golden_imports.py) -- is executed in a fresh interpreter with
``hydrodem_amd/dropin`` first on ``sys.path`` and must bind objects of this
package.  No GPU, no library load: importing the operators is free.
"""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "hydrodem_amd", "dropin")
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_imports.json"),
                      encoding="utf-8"))


def run(code, *extra_path):
    head = "import sys\n" + "".join(f"sys.path.insert(0, {p!r})\n"
                                    for p in reversed((DROPIN, ROOT) + extra_path))
    return subprocess.run([sys.executable, "-c", head + textwrap.dedent(code)],
                          capture_output=True, text=True, cwd="/")


def test_the_fixture_holds_the_three_caller_lines_of_the_verdict():
    by_where = {r["where"]: r for r in ROWS}
    assert by_where["hydrodem/image_srtm.py:7"]["names"] == [
        "DetectApplyFourier", "BinaryClosing", "GrovesCorrectionsIter"]
    assert by_where["hydrodem/image_hsheds.py:6"]["names"] == [
        "LagoonsDetection", "ClipLagoonsRivers", "ProcessRivers"]
    assert by_where["hydrodem/hydro_dem_process.py:20"]["names"] == [
        "SubtractionFilter", "ProductFilter", "AdditionFilter", "PostProcessingFinal"]


@pytest.mark.parametrize("row", ROWS, ids=[r["where"] for r in ROWS])
def test_reference_import_statement_resolves_to_this_package(row):
    stmt = f"from {row['module']} import ({', '.join(row['names'])})"
    code = stmt + "\n" + "\n".join(
        f"assert {n}.__module__.startswith('hydrodem_amd.'), ({n!r}, {n}.__module__)"
        for n in row["names"]) + "\nprint('ok')\n"
    out = run(code)
    assert out.returncode == 0 and out.stdout.strip() == "ok", f"{stmt}\n{out.stderr}"


def test_all_statements_in_one_interpreter_share_one_set_of_classes():
    lines = []
    for row in ROWS:
        lines.append(f"from {row['module']} import ({', '.join(row['names'])})")
        lines += [f"seen.setdefault({n!r}, {n}); assert seen[{n!r}] is {n}, {n!r}"
                  for n in row["names"]]
    out = run("seen = {}\n" + "\n".join(lines) + "\nimport hydrodem_amd\n"
              "assert seen['GrovesCorrectionsIter'] is hydrodem_amd.GrovesCorrectionsIter\n"
              "assert seen['Filter'] is hydrodem_amd.Filter\nprint(len(seen))\n")
    assert out.returncode == 0 and int(out.stdout) >= 45, out.stderr


def test_other_cguerrero_modules_still_come_from_the_reference_tree(tmp_path):
    """``cguerrero.hydrodem.utils_dem`` (GDAL I/O, not rebuilt) must keep
    resolving to the tree behind the drop-in; a stand-in tree plays the
    reference here (the GPU box has none)."""
    pkg = tmp_path / "cguerrero" / "hydrodem"
    (pkg / "filters").mkdir(parents=True)
    (tmp_path / "cguerrero" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "utils_dem.py").write_text("WHO = 'reference tree'\n")
    (pkg / "sliding_window.py").write_text("raise ImportError('shadowed module was imported')\n")
    (pkg / "filters" / "__init__.py").write_text("raise ImportError('shadowed package')\n")
    out = run("""
        from cguerrero.hydrodem.utils_dem import WHO
        from cguerrero.hydrodem.filters.custom_filters import RouteRivers, QuadraticFilter
        from cguerrero.hydrodem.sliding_window import SlidingWindow
        from cguerrero.hydrodem.exceptions import WindowSizeEvenError
        import hydrodem_amd
        assert WHO == 'reference tree'
        assert QuadraticFilter is hydrodem_amd.QuadraticFilter
        assert SlidingWindow is hydrodem_amd.sliding_window.SlidingWindow
        print('ok')
        """, str(tmp_path))
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_custom_filters_namespace_covers_the_reference_module():
    """Every public class the reference's custom_filters binds at module level
    (its own 22 + what custom_filters.py:9-19 imports) exists here."""
    names = sorted({n for r in ROWS if r["where"].startswith("hydrodem/filters/custom_filters.py")
                    for n in r["names"]})
    own = ["MajorityFilter", "ExpandFilter", "RouteRivers", "QuadraticFilter", "CorrectNANValues",
           "IsolatedPoints", "BlanksFourier", "DetectBlanksFourier", "MaskNegatives",
           "MaskPositives", "MaskTallGroves", "MaskFourier", "TidyingLagoons", "LagoonsDetection",
           "GrovesCorrection", "GrovesCorrectionsIter", "ProcessRivers", "ClipLagoonsRivers",
           "FourierInitial", "FourierProcessQuarters", "DetectApplyFourier", "PostProcessingFinal"]
    out = run("import filters.custom_filters as m\n"
              f"missing = [n for n in {names + own!r} if not hasattr(m, n)]\n"
              "assert not missing, missing\nprint('ok')\n")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


SLIDING_SMALL = os.path.join(ROOT, "tests", "golden", "sliding_small.npz")

# what the checks below share: build a case of tests/golden/sliding_small.npz with the
# classes the import statement of the caller bound (``classes``)
_CASE_HELPERS = f"""
import json
import numpy as np
from numpy import testing
g = np.load({SLIDING_SMALL!r})
cases = {{c["name"]: c for c in json.loads(str(g["cases"]))}}

def make(name):
    c = cases[name]
    grid = np.arange(c["rows"] * c["cols"]).reshape((c["rows"], c["cols"]))
    kw = {{"window_size": c["window_size"]}}
    if c["inner_size"]:
        kw["inner_size"] = c["inner_size"]
    return classes[c["class"]](grid, **kw)
"""


def test_the_references_own_sliding_window_tests_behave_the_same_against_the_dropin():
    """The known answers of the reference's `cguerrero/tests/test_sliding_window.py` -- the
    literals of its `tests/constants.py`, committed as data with the case and position each
    is checked at (tests/golden/sliding_small.npz, tests/golden/make_golden_sliding_small.py)
    -- hold for the classes its import statement `from cguerrero.hydrodem.sliding_window
    import ...` binds in a fresh interpreter with `dropin/` first on `sys.path`: the windows
    and centres of the iterations over 4 x 4, 3 x 3, 3 x 4, 6 x 6 and 9 x 9 grids and the
    __getitem__ windows, NaN positions included."""
    code = """
        from cguerrero.hydrodem.sliding_window import (SlidingWindow, InnerWindow,
                                                       SlidingIgnoreBorder, CircularWindow,
                                                       NoCenterWindow, IgnoreBorderInnerSliding)
        classes = {c.__name__: c for c in (SlidingWindow, InnerWindow, SlidingIgnoreBorder,
                                           CircularWindow, NoCenterWindow,
                                           IgnoreBorderInnerSliding)}
        assert all(c.__module__ == 'hydrodem_amd.sliding_window' for c in classes.values())
        """
    code = textwrap.dedent(code) + _CASE_HELPERS + textwrap.dedent("""
        known = json.loads(str(g["known"]))
        for k in known:
            sliding = make(k["case"])
            if k["position"] is not None:
                testing.assert_array_equal(sliding[tuple(k["position"])], g["known_" + k["const"]],
                                           err_msg=k["const"])
                continue
            got = list(sliding)
            want_w = g["known_" + k["const"] + "_windows"]
            first = k.get("nth", 0)
            got = got[first:first + len(want_w)]
            assert len(got) == len(want_w), k["const"]
            for (win, centre), w, c in zip(got, want_w, g["known_" + k["const"] + "_centres"]):
                testing.assert_array_equal(win, w, err_msg=k["const"])
                if "nth" not in k:
                    assert tuple(centre) == tuple(c), (k["const"], centre, c)
        print('checked', len(known))
        """)
    out = run(code)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["checked", "24"]


def test_the_88_doctest_examples_of_the_references_sliding_window_hold_for_the_dropin():
    """The results the docstring examples of the reference's `sliding_window.py` show --
    for each class the first windows of `iter(sliding)` on its first grid, every window of
    the loop over its `grid_2` (3 x 3, 3 x 4, 4 x 4, 6 x 6) and `sliding[1, 1]`,
    `sliding[3, 3]`, `sliding[1, 3]` -- recorded from the reference as data
    (tests/golden/sliding_small.npz), hold for the classes the examples' own
    `from sliding_window import ...` binds with `dropin/` first on `sys.path`."""
    code = """
        import sliding_window
        from sliding_window import (SlidingWindow, SlidingIgnoreBorder, CircularWindow,
                                    InnerWindow, NoCenterWindow, IgnoreBorderInnerSliding)
        assert sliding_window.SlidingWindow.__module__ == 'hydrodem_amd.sliding_window'
        classes = {c.__name__: c for c in (SlidingWindow, SlidingIgnoreBorder, CircularWindow,
                                           InnerWindow, NoCenterWindow,
                                           IgnoreBorderInnerSliding)}
        """
    code = textwrap.dedent(code) + _CASE_HELPERS + textwrap.dedent("""
        names = json.loads(str(g["doctest_cases"]))
        for name in names:
            got = list(make(name))
            assert len(got) == len(g[name + "_windows"]), name
            for (win, centre), w, c in zip(got, g[name + "_windows"], g[name + "_centres"]):
                testing.assert_array_equal(win, w, err_msg=name)
                assert tuple(centre) == tuple(c), (name, centre, c)
        s = make("SlidingWindow_5x5_3")
        pos = [tuple(p) for p in cases["SlidingWindow_5x5_3"]["positions"]]
        for p in [(1, 1), (3, 3), (1, 3)]:
            testing.assert_array_equal(s[p], g["SlidingWindow_5x5_3_getitem"][pos.index(p)])
        print('checked', len(names))
        """)
    out = run(code)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["checked", "11"]
