"""Reader of tests/golden/reference_answers.npz: answers of the reference's own C code (oracle/_ref/libmifi_ref.so), recorded by
scripts/record_reference_answers.py.  Keys are "<group>.<case>.<field>"; inputs are stored as they were passed, outputs as bit
patterns (uint32 of float32, uint64 of float64) next to return codes and nChanged.  Reads tests/golden/ only."""
import os

import numpy as np

FILE = "reference_answers.npz"


class Fixture:
    def __init__(self, path):
        with np.load(path, allow_pickle=False) as z:
            self.arrays = {k: z[k] for k in z.files}

    def names(self, group):
        """sorted "<group>.<case>" names of one group."""
        return sorted({".".join(k.split(".")[:2]) for k in self.arrays if k.split(".")[0] == group})

    def case(self, name):
        return {k[len(name) + 1:]: v for k, v in self.arrays.items() if k.startswith(name + ".")}


def load(golden_dir):
    return Fixture(os.path.join(golden_dir, FILE))


def levels_of(Levels, c):
    """The vertical_ref.Levels (or capi.VerticalLevels: same keywords) of a "levels" case."""
    kw = {k: c[k] for k in ("sigma", "a", "ap", "b") if k in c}
    return Levels(int(c["kind"]), int(c["nz"]), p0=float(c["p0"]), ptop=float(c["ptop"]), ps=c["ps"], **kw)
