"""Write the fixture tests/golden/g27_neuron_coords.npz: coordinate files written by cwfa_amd.CWFA.write_neural_coordinates_to_file and
what the REFERENCE's own read_neural_coordinates_from_file (CWFA.py:223-238, imported by oracle.make_golden's recipe) returns from
them.  The CSV texts and the returned lists only.  Run from the repository root:  python tools/make_neuron_golden.py

Two sets: one with a negative relative z (a peak below the central planes), one with a `score` column.  For a list of files the
reference returns the first file's rows (it drops the result of dataframe.append; under pandas 2, which has no such method, the
call raises and the generator records that instead)."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import dump, import_reference  # noqa: E402

SETS = {"plain": ([[17, 40, -9], [101, 7, 3], [5, 5, 0], [60, 88, 11]], None),
        "scored": ([[30, 31, 2], [12, 90, -1], [77, 45, 6]], [1.5, 0.4375, 0.25])}


def main():
    from cwfa_amd.CWFA import write_neural_coordinates_to_file
    ref = import_reference()[-1]
    arrs = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for name, (coords, scores) in SETS.items():
            path = os.path.join(tmp, name + ".csv")
            write_neural_coordinates_to_file(coords, path, scores)
            got = ref.read_neural_coordinates_from_file(path)
            assert got == coords and all(type(v) is int for row in got for v in row), (name, got)
            arrs[name + "/csv"] = np.array(open(path).read())
            arrs[name + "/coords"] = np.array(got, dtype=np.int64)
            if scores is not None:
                arrs[name + "/scores"] = np.array(scores, dtype=np.float64)
            paths.append(path)
        try:
            both = ref.read_neural_coordinates_from_file(paths)
            arrs["list/raised"] = np.int64(0)
            arrs["list/coords"] = np.array(both, dtype=np.int64)
            assert both == SETS["plain"][0], "the reference returns the first file's rows"
        except AttributeError:                       # pandas 2: DataFrame.append is gone
            arrs["list/raised"] = np.int64(1)
    arrs["sets"] = np.array(list(SETS))
    dump("g27_neuron_coords", **arrs)


if __name__ == "__main__":
    main()
