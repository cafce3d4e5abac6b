"""
Regenerates tests/golden/sliding_small.npz from a checkout of the reference (its
cguerrero/ directory), so that the window classes are pinned without the reference tree:

  cases   every window and centre the imported reference's classes yield on the grids of
          its unit tests and docstring examples (np.arange(r * c) as 3 x 3, 3 x 4, 4 x 4,
          5 x 5, 6 x 6 and 9 x 9), and what __getitem__ returns at the positions those tests
          index and at every centre of the iteration;
  known   the known-answer literals of the reference's tests/constants.py, each with the case
          and the position (or the iteration) the reference's test_sliding_window.py checks
          it against -- data only: the generator checks that the reference reproduces them.

    python tests/golden/make_golden_sliding_small.py <reference>/cguerrero
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (class name, window size, inner size or None)
SHAPES = [("SlidingWindow", 3, None), ("SlidingIgnoreBorder", 3, None),
          ("CircularWindow", 3, None), ("NoCenterWindow", 3, None),
          ("InnerWindow", 5, 3), ("IgnoreBorderInnerSliding", 5, 3)]
GRIDS = [(3, 3), (3, 4), (4, 4), (5, 5), (6, 6), (9, 9)]
# positions the reference's unit tests and docstrings index, besides the iteration's centres
POSITIONS = {("SlidingWindow", 5, 5): [(1, 1), (3, 3), (1, 3)],
             ("SlidingIgnoreBorder", 5, 5): [(1, 1), (3, 3), (5, 4)],
             ("CircularWindow", 5, 5): [(1, 1), (3, 3), (2, 3), (1, 2)],
             ("InnerWindow", 6, 6): [(2, 2), (3, 3)],
             ("NoCenterWindow", 3, 4): [(1, 1), (1, 2)],
             ("IgnoreBorderInnerSliding", 9, 9): [(4, 5), (4, 9), (4, 6)]}
# constants.py name -> (case, position); a position of None: the first windows of the iteration
KNOWN = {"sliding_window_3x3": ("SlidingWindow_4x4_3", None),
         "sliding_window_element_1_1": ("SlidingWindow_5x5_3", (1, 1)),
         "sliding_window_element_3_3": ("SlidingWindow_5x5_3", (3, 3)),
         "sliding_window_element_1_3": ("SlidingWindow_5x5_3", (1, 3)),
         "sliding_window_ignore_border_3x3": ("SlidingIgnoreBorder_3x3_3", None),
         "ignore_border_element_1_1": ("SlidingIgnoreBorder_5x5_3", (1, 1)),
         "ignore_border_element_3_3": ("SlidingIgnoreBorder_5x5_3", (3, 3)),
         "ignore_border_element_5_4": ("SlidingIgnoreBorder_5x5_3", (5, 4)),
         "circular_window_3x4": ("CircularWindow_3x4_3", None),
         "circular_window_element_1_1": ("CircularWindow_5x5_3", (1, 1)),
         "circular_window_element_3_3": ("CircularWindow_5x5_3", (3, 3)),
         "circular_window_element_2_3": ("CircularWindow_5x5_3", (2, 3)),
         "inner_window_6x6": ("InnerWindow_6x6_5_3", None),
         "inner_window_element_2_2": ("InnerWindow_6x6_5_3", (2, 2)),
         "inner_window_element_3_3": ("InnerWindow_6x6_5_3", (3, 3)),
         "no_center_sliding_window_3x4": ("NoCenterWindow_3x4_3", None),
         "no_center_sliding_window_1_1": ("NoCenterWindow_3x4_3", (1, 1)),
         "no_center_sliding_window_1_2": ("NoCenterWindow_3x4_3", (1, 2)),
         "mixing_sliding_element_4_5": ("IgnoreBorderInnerSliding_9x9_5_3", (4, 5)),
         "mixing_sliding_element_4_9": ("IgnoreBorderInnerSliding_9x9_5_3", (4, 9))}
# the first four windows of the combined class's iteration, one constant each
KNOWN_NTH = {"first_element_test": 0, "second_element_test": 1, "third_element_test": 2,
             "fourth_element_test": 3}
# the cases of the docstring examples: the first grid of each class and its `grid_2`
DOCTEST_CASES = ["SlidingWindow_5x5_3", "SlidingWindow_4x4_3", "SlidingIgnoreBorder_5x5_3",
                 "SlidingIgnoreBorder_3x3_3", "CircularWindow_5x5_3", "CircularWindow_3x4_3",
                 "InnerWindow_9x9_5_3", "InnerWindow_6x6_5_3", "NoCenterWindow_5x5_3",
                 "NoCenterWindow_3x4_3", "IgnoreBorderInnerSliding_9x9_5_3"]


def case_name(cls_name, rows, cols, ws, inner):
    return f"{cls_name}_{rows}x{cols}_{ws}" + (f"_{inner}" if inner else "")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(sys.argv[1], "hydrodem"))
    sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import sliding_window as ref_sw
    import constants
    out, cases = {}, []
    for rows, cols in GRIDS:
        grid = np.arange(rows * cols).reshape((rows, cols))
        for cls_name, ws, inner in SHAPES:
            if ws > min(rows, cols):
                continue
            cls = getattr(ref_sw, cls_name)
            kw = {"window_size": ws} if inner is None else {"window_size": ws, "inner_size": inner}
            wins, centres = [], []
            for w, c in cls(grid, **kw):
                wins.append(np.asarray(w, dtype=np.float32))
                centres.append(tuple(int(v) for v in c))
            sliding = cls(grid, **kw)
            positions, items = [], []
            for pos in POSITIONS.get((cls_name, rows, cols), []) + centres:
                if pos in positions:
                    continue
                try:
                    item = sliding[pos]
                except Exception:  # pylint: disable=broad-except
                    continue                    # the reference refuses it: nothing to pin
                positions.append(pos)
                items.append(np.asarray(item, dtype=np.float32))
            name = case_name(cls_name, rows, cols, ws, inner)
            cases.append({"name": name, "class": cls_name, "rows": rows, "cols": cols,
                          "window_size": ws, "inner_size": inner,
                          "positions": [list(p) for p in positions]})
            out[name + "_windows"] = np.stack(wins) if wins else np.zeros((0, ws, ws), np.float32)
            out[name + "_centres"] = np.array(centres, dtype=np.int64).reshape(-1, 2)
            out[name + "_getitem"] = np.stack(items) if items else np.zeros((0, ws, ws), np.float32)
            print(name, len(wins), "windows,", len(positions), "positions")
    by_name = {c["name"]: c for c in cases}
    known = []
    for const, (name, pos) in KNOWN.items():
        value = getattr(constants, const)
        entry = {"const": const, "case": name, "position": list(pos) if pos else None}
        if pos is None:
            out["known_" + const + "_windows"] = np.stack([np.asarray(w, np.float32)
                                                           for w, _ in value])
            out["known_" + const + "_centres"] = np.array([c for _, c in value], np.int64)
            assert np.array_equal(out[name + "_windows"][:len(value)],
                                  out["known_" + const + "_windows"], equal_nan=True), const
        else:
            out["known_" + const] = np.asarray(value, np.float32)
            k = by_name[name]["positions"].index(list(pos))
            assert np.array_equal(out[name + "_getitem"][k], out["known_" + const],
                                  equal_nan=True), const
        known.append(entry)
    for const, nth in KNOWN_NTH.items():
        w, c = getattr(constants, const)
        name = "IgnoreBorderInnerSliding_9x9_5_3"
        out["known_" + const + "_windows"] = np.asarray(w, np.float32)[None]
        out["known_" + const + "_centres"] = np.array([c], np.int64)
        assert np.array_equal(out[name + "_windows"][nth], np.asarray(w, np.float32),
                              equal_nan=True), const
        known.append({"const": const, "case": name, "position": None, "nth": nth})
    assert all(c in by_name for c in DOCTEST_CASES)
    out["cases"] = np.array(json.dumps(cases))
    out["known"] = np.array(json.dumps(known))
    out["doctest_cases"] = np.array(json.dumps(DOCTEST_CASES))
    np.savez_compressed(os.path.join(HERE, "sliding_small.npz"), **out)


if __name__ == "__main__":
    main()
