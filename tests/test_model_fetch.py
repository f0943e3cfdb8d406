"""scripts/model_fetch.py, the CPU model of what the staged bilinear launch stages and fetches: it cuts the bench plans' tiles with the
library's own rules and must keep reproducing the staged cells per slice that the library reports for the two bench variants
(BENCH_r03.json: plan.info()["stagedCells"] of the default and the one_percent workload), which it does exactly; the fetch figures
of DESIGN.md 6.2 stand on that."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.mark.parametrize("variant,staged", [("default", 12082148), ("one_percent", 9673512)])
def test_model_reproduces_the_staged_cells_of_the_bench_plans(variant, staged):
    import model_fetch
    m = model_fetch.model(variant, 512, 8, 200)
    assert m["staged_cells_per_slice"] == staged
    lines = m["lines_summed_over_tiles"]["cells_per_slice"]
    # lines are whole and hold every staged cell; every order fetches between the floor and the sum over tiles
    assert lines >= m["staged_cells_per_slice"] and lines % 32 == 0
    floor = m["distinct_lines"]["cells_per_slice"]
    assert lines == floor + m["duplicates_x"]["cells_per_slice"] + m["duplicates_y"]["cells_per_slice"]
    for name, o in m["orders"].items():
        assert floor <= o["cells_per_slice"] <= lines, name
