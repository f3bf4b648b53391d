"""Throw-away: slice tests/golden/wgrad_classes.json to the cells with x3_occ == 3 and prove the slice against the parent's file.  Not a tool:
the table is sliced once, at the commit that removes TNR_WG_X3_OCC (profiles/r34a_wgrad_env_cleanout.txt, section 3).

    python profiles/r34a_wgrad_golden_slice.py --parent <commit> --write     # slice the parent's file into the working tree
    python profiles/r34a_wgrad_golden_slice.py --parent <commit>             # compare the working tree's file with the parent's, value for value

The parent's file is read with `git show <commit>:tests/golden/wgrad_classes.json`, never from the working tree, and nothing here loads the
library: the sliced table is the recorded one, not a new record of the code under test.  classes and records are re-indexed in the order of their
first use over the kept cells, the order tools/record_wgrad_classes.py's walk would give them.
"""
import argparse
import itertools
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = "tests/golden/wgrad_classes.json"
KEEP = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    old = json.loads(subprocess.run(["git", "show", "%s:%s" % (a.parent, PATH)], cwd=ROOT, check=True, capture_output=True).stdout)
    names = list(old["dims"])
    grid = list(itertools.product(*old["dims"].values()))
    assert len(grid) == len(old["cells"]) == 1944 and names[4] == "x3_occ"
    kept = [(cell[:4] + cell[5:], row) for cell, row in zip(grid, old["cells"]) if cell[4] == KEEP]
    if a.write:
        classes, records, cells = {}, {}, []
        for _, row in kept:
            out = []
            for ri in row:
                rec = old["records"][ri]
                cls = old["classes"][rec[0]]
                new = (classes.setdefault(None if cls is None else tuple(cls), len(classes)),) + tuple(rec[1:])
                out.append(records.setdefault(new, len(records)))
            cells.append(out)
        doc = {"recorded_at_commit": old["recorded_at_commit"],
               "sliced": "the 648 cells with x3_occ == 3 of the 1944 recorded ones, re-indexed, by the commit after %s "
                         "(profiles/r34a_wgrad_golden_slice.py)" % a.parent,
               "dims": {k: v for k, v in old["dims"].items() if k != "x3_occ"},
               "sizes": old["sizes"], "group_jobs": old["group_jobs"],
               "classes": [None if c is None else list(c) for c in classes], "records": [list(r) for r in records], "cells": cells}
        with open(os.path.join(ROOT, PATH), "w") as f:
            f.write(json.dumps(doc, separators=(",", ":")).replace('],"', '],\n"').replace("]],[[", "]],\n[[") + "\n")
    with open(os.path.join(ROOT, PATH)) as f:
        new = json.load(f)
    assert new["recorded_at_commit"] == old["recorded_at_commit"] and "x3_occ" not in new["dims"]
    assert list(new["dims"].items()) == [(k, v) for k, v in old["dims"].items() if k != "x3_occ"]
    assert new["sizes"] == old["sizes"] and new["group_jobs"] == old["group_jobs"]
    new_grid = list(itertools.product(*new["dims"].values()))
    assert new_grid == [cell for cell, _ in kept] and len(new["cells"]) == len(kept) == 648
    n = 0
    for (cell, old_row), new_row in zip(kept, new["cells"]):
        assert len(old_row) == len(new_row) == len(old["sizes"])
        for oi, ni in zip(old_row, new_row):
            orec, nrec = old["records"][oi], new["records"][ni]
            assert old["classes"][orec[0]] == new["classes"][nrec[0]] and orec[1:] == nrec[1:], (cell, orec, nrec)
            n += 1
    used_r = {ri for row in new["cells"] for ri in row}
    used_c = {new["records"][ri][0] for ri in used_r}
    assert used_r == set(range(len(new["records"]))) and used_c == set(range(len(new["classes"]))), "an entry no kept cell references"
    assert len({tuple(r) for r in new["records"]}) == len(new["records"]) and len({tuple(c) for c in new["classes"]}) == len(new["classes"])
    live = [c for c in new["classes"] if c is not None]
    assert len(live) == 44, len(live)
    dropped = sorted(tuple(c) for c in old["classes"] if c is not None and c not in live)
    print("parent %s: %d cells, %d records, %d classes, %d bytes" % (a.parent, len(old["cells"]), len(old["records"]), len(old["classes"]),
                                                                   len(subprocess.run(["git", "show", "%s:%s" % (a.parent, PATH)], cwd=ROOT,
                                                                                      check=True, capture_output=True).stdout)))
    print("sliced: %d cells, %d records, %d classes (%d non-null), %d bytes" % (len(new["cells"]), len(new["records"]), len(new["classes"]), len(live),
                                                                                os.path.getsize(os.path.join(ROOT, PATH))))
    print("%d (cell, size) entries equal the parent's, class tuple and record values" % n)
    print("classes of the parent no kept cell reaches (%d):" % len(dropped), " ".join("{%s}" % ",".join(map(str, c)) for c in dropped))


if __name__ == "__main__":
    main()
