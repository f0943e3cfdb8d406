"""The chunk-per-XCD launch order of the second staged form's float kernel (staged2.hip; the order itself: staged_layout.hpp,
tests/test_staged_layout_chunk_xcd.py) on the GPU: XCD x runs z chunk x of every tile instead of all chunks of its own tiles.  The
results must not know: every case is compared bit for bit with the oracle through the C ABI, identical NaN positions included
(bicubic in float arithmetic: within its stated 1e-5 of the stencil's magnitude, and bit-equal between the orders).

The tuning build forces the order (FIMEX_AMD_STAGE2_ORDER 2) at a small shape: source 320 x 240 onto 192 x 160 with positions that
overshoot the source on every side, 256 threads on 64 x 16 tiles.  That is 10 bands of 3 tiles, so cohorts of 8 bands x 4 tiles
give one full band group and a last cohort of two bands; band 9 lies below the source (tiles without chunks, every output
undefined), and one cell of band 0 points 200 source rows away from its neighbours, so its tile is split and the piece that holds
it is a gather tile -- both inside a cohort.  plan.launch_order(nz) says which order a batch takes, so a case that silently ran
the old order fails.

Batch lengths, with the chunk length (FIMEX_AMD_STAGE2_ZPB) that makes the rule of chunk_xcd_chunk_count give them 8 chunks:
8 slices (chunks of 1: shorter than the ring), 17 (chunks of 2 and 3), 24 (3 each), 35 (4 and 5: the ring's tail path after its
steady state in every chunk); 35 slices in 16 chunks; 5 and 7 slices fall back to the tile-major order."""
import numpy as np
import pytest

import cases
import oracle

gpu = pytest.mark.gpu

IN_X, IN_Y, OUT_X, OUT_Y = 320, 240, 192, 160
NZ_MAX = 35
TILE_MAJOR, CHUNK_PER_XCD = 1, 2
# nz, STAGE2_ZPB, chunks the order takes (0: the batch falls back to the tile-major order)
BATCHES = [(8, 1, 8), (17, 3, 8), (24, 3, 8), (35, 5, 8), (35, 2, 16), (5, 3, 0), (7, 1, 0)]
SHAPE_ENV = {"STAGE2_NT": "256", "STAGE2_TW": "64", "STAGED_MIN_NZ": "1"}
KINDS = {"nearest": (oracle.NEAREST, None), "bilinear": (oracle.BILINEAR, None), "bicubic_float": (oracle.BICUBIC, "BICUBIC_FAST")}


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


def positions(outlier=True):
    y, x = np.meshgrid(np.arange(OUT_Y, dtype=np.float64), np.arange(OUT_X, dtype=np.float64), indexing="ij")
    px, py = (x * 1.7 - 2.5).ravel(), (y * 1.7 - 1.7).ravel()
    if outlier:
        px[2 * OUT_X + 10], py[2 * OUT_X + 10] = 150.3, 205.4  # the outlier of band 0
    assert px.max() > IN_X and py.reshape(OUT_Y, OUT_X)[144:].min() > IN_Y  # band 9 (rows 144 .. 159) lies below the source
    return px, py


class Case:
    """one kind: positions, field and the oracle's answer, computed once and shared by the variants"""
    _made = {}

    def __new__(cls, kind):
        if kind not in cls._made:
            self = super().__new__(cls)
            self.kind = kind
            self.method, self.arith = KINDS[kind]
            self.px, self.py = positions()
            self.f = cases.field(NZ_MAX, IN_Y, IN_X, seed=len(kind), extremes=False)
            self.want = oracle.interpolate_values(self.method, self.px, self.py, self.f, IN_X, IN_Y, OUT_X, OUT_Y)
            self.tile_major = {}  # nz -> the tile-major launch's result (float bicubic is compared with it)
            cls._made[kind] = self
        return cls._made[kind]

    def plan(self, fa, monkeypatch, env):
        for k, v in dict(SHAPE_ENV, **env).items():
            monkeypatch.setenv("FIMEX_AMD_" + k, v)
        plan = fa.RegridPlan(self.method, self.px, self.py, IN_X, IN_Y, OUT_X, OUT_Y, bicubic=getattr(fa, self.arith) if self.arith else None)
        info = plan.info()
        assert info["stagedCells"] > 0 and (info["tileW"], info["tileH"]) == (64, 16), info
        return plan

    def run(self, plan, nz):
        import torch
        d_in = torch.from_numpy(np.ascontiguousarray(self.f[:nz])).cuda()
        out = torch.full((nz, OUT_Y, OUT_X), 7.0, dtype=torch.float32, device="cuda")
        plan.apply_device(d_in.data_ptr(), nz, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def check(self, got, nz, what):
        want = self.want[:nz]
        if self.kind != "bicubic_float":
            assert cases.same(got, want), (what, cases.describe_mismatch(got, want))
            return
        # float arithmetic: 1e-5 of the stencil's magnitude (BASELINE.json), NaN exactly where the oracle has them
        from numpy.lib.stride_tricks import sliding_window_view
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        x0, y0 = np.floor(self.px).astype(np.int64) - 1, np.floor(self.py).astype(np.int64) - 1
        ok = (x0 >= 0) & (x0 + 3 < IN_X) & (y0 >= 0) & (y0 + 3 < IN_Y)
        for z in range(nz):
            mag = np.zeros(self.px.size, np.float32)
            mag[ok] = sliding_window_view(np.abs(np.nan_to_num(self.f[z])), (4, 4)).max(axis=(2, 3))[y0[ok], x0[ok]]
            d = np.abs(got[z].ravel().astype(np.float64) - want[z].ravel())
            fin = np.isfinite(want[z].ravel())
            assert fin.any() and (d[fin] <= 1e-5 * mag[fin]).all(), (what, float((d[fin] / mag[fin]).max()))


def test_the_case_has_a_gather_tile_an_undefined_band_and_a_ragged_last_cohort():
    """what the docstring promises of the geometry, from the positions alone: 10 bands of 16 rows; the outlier's tile spans more
    source rows than a tile may (160), every other tile of band 0 does not; band 9 reads nothing"""
    px, py = positions()
    py2 = py.reshape(OUT_Y, OUT_X)
    assert OUT_Y // 16 == 10 and OUT_X // 64 == 3
    band0 = py2[:16]
    assert band0[:, :64].max() - band0[:, :64].min() > 160 and band0[:, 64:].max() - band0[:, 64:].min() < 40
    assert (py2[144:] > IN_Y - 0.5).all()
    assert np.isfinite(oracle.interpolate_values(oracle.BILINEAR, px, py, np.ones((1, IN_Y, IN_X), np.float32), IN_X, IN_Y, OUT_X, OUT_Y)).mean() > 0.7


@gpu
def test_the_plan_itself_holds_the_gather_tile_and_the_undefined_band(fa, tuning_build, monkeypatch):
    """The same two facts from the plan, so that a change of the cutting rules that loses them fails here.  Against a plan of the
    same positions without the outlier: a gather tile stages nothing, so the plan with the outlier streams fewer source cells -- the
    piece that turns into a gather tile is 32 columns wide (tile_width_step of a 64-column shape), 32 * 1.7 = 54 cells of every source
    row of its footprint, while the one cut that leads to it adds at most one 16-byte chunk and one shared stencil column per row, 5
    cells; every other tile is the same in both plans.  And the target cells of band 9, a whole row of tiles, are all counted undefined."""
    case = Case("bilinear")
    with_outlier = case.plan(fa, monkeypatch, {}).info()
    px, py = positions(outlier=False)
    plain = fa.RegridPlan(oracle.BILINEAR, px, py, IN_X, IN_Y, OUT_X, OUT_Y).info()
    print("stagedCells with / without the outlier:", with_outlier["stagedCells"], plain["stagedCells"],
          "planBytes:", with_outlier["planBytes"], plain["planBytes"], "undefinedCells:", with_outlier["undefinedCells"])
    assert (plain["tileW"], plain["tileH"]) == (64, 16) and 0 < with_outlier["stagedCells"] < plain["stagedCells"]
    assert with_outlier["undefinedCells"] >= 16 * OUT_X and with_outlier["undefinedCells"] >= plain["undefinedCells"]


@gpu
@pytest.mark.parametrize("depth", ["2", "3"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_chunk_per_xcd_order_matches_the_oracle(fa, tuning_build, monkeypatch, kind, depth):
    case = Case(kind)
    plan = case.plan(fa, monkeypatch, {"STAGE2_DEPTH": depth})
    for nz, zpb, chunks in BATCHES:
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ZPB", str(zpb))
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ORDER", "1")
        assert plan.launch_order(nz) == TILE_MAJOR
        before = case.run(plan, nz)
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ORDER", "2")
        assert plan.launch_order(nz) == (CHUNK_PER_XCD if chunks else TILE_MAJOR), (nz, zpb)
        got = case.run(plan, nz)
        case.check(got, nz, (kind, depth, nz, zpb))
        assert cases.same(got, before), ("the two orders differ", kind, depth, nz, zpb, cases.describe_mismatch(got, before))


@gpu
@pytest.mark.parametrize("cohort", [("16", "2"), ("32", "1"), ("2", "1")])
def test_other_cohort_shapes(fa, tuning_build, monkeypatch, cohort):
    """STAGE2_COHORT_BANDS / _TILES, read when the plan is built: the sweeps' cohorts, and one so small that the sequence is cut into
    many"""
    case = Case("bilinear")
    plan = case.plan(fa, monkeypatch, {"STAGE2_COHORT_BANDS": cohort[0], "STAGE2_COHORT_TILES": cohort[1], "STAGE2_ORDER": "2", "STAGE2_ZPB": "3"})
    assert plan.launch_order(17) == CHUNK_PER_XCD
    case.check(case.run(plan, 17), 17, cohort)


def product_case():
    """the product's shapes need a target of some size for more than one cohort: 40 bands of two tiles (1024 threads on 512 x 8)"""
    inX, inY, outX, outY = 721, 361, 900, 320
    px, py = cases.coherent_positions(inX, inY, outX, outY, seed=51, outliers=3)
    return px, py, inX, inY, outX, outY


@gpu
def test_product_build_takes_the_order_from_104_slices_on_once_tuning_chose_it(fa, monkeypatch):
    """The product library: a plan that was never tuned runs the tile-major order at every batch length.  tune_device at 104
    slices -- the shortest batch the rule gives 8 chunks of at least 13 slices -- times the second order too, returns, and leaves a
    valid choice that info() and launch_order() agree on; tuned again on one slice less, where only the shapes can be chosen, the plan
    keeps that order.  Whatever it chose, the result is the oracle's; the other order gives the same bits (forced in the tuning build
    on the same plan geometry)."""
    import torch
    px, py, inX, inY, outX, outY = product_case()
    nz = 104
    f = np.ascontiguousarray(np.broadcast_to(cases.field(8, inY, inX, seed=52), (13, 8, inY, inX)).reshape(nz, inY, inX))
    f += np.arange(nz, dtype=np.float32)[:, None, None]  # no two slices alike
    want = oracle.interpolate_values(oracle.BILINEAR, px, py, f, inX, inY, outX, outY)
    st = torch.cuda.current_stream().cuda_stream
    d_in = torch.from_numpy(f).cuda()
    d_out = torch.full((nz, outY, outX), 7.0, device="cuda")
    was = fa.use_tuning_build(False)
    try:
        plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
        assert plan.info()["stagedCells"] > 0 and plan.info()["launchOrder"] == 0
        assert [plan.launch_order(n) for n in (3, 4, 103, 104, 500)] == [-1, TILE_MAJOR, TILE_MAJOR, TILE_MAJOR, TILE_MAJOR]
        shape = plan.tune_device(d_in.data_ptr(), nz, d_out.data_ptr(), st)
        order = plan.info()["launchOrder"]
        assert shape in (0, 1) and order in (0, 1)
        # The tuning launches leave the regridded slices behind, and the last of them ran the chunk-per-XCD order on the shape kept.
        # This comparison is therefore the product library's own coverage of the new order whatever the rule then chose (the forced
        # comparisons below run the tuning build): tune_device has to go on timing that order last, into d_out.
        assert cases.same(d_out.cpu().numpy(), want)
        assert plan.launch_order(104) == (CHUNK_PER_XCD if order else TILE_MAJOR) and plan.launch_order(103) == TILE_MAJOR
        d_out.fill_(7.0)
        plan.apply_device(d_in.data_ptr(), nz, d_out.data_ptr(), st)
        torch.cuda.synchronize()
        assert cases.same(d_out.cpu().numpy(), want)
        # one slice less: the shapes are timed again, the order chosen on the longer batch stays
        assert plan.tune_device(d_in.data_ptr(), 103, d_out.data_ptr(), st) in (0, 1) and plan.info()["launchOrder"] == order
        assert plan.launch_order(104) == (CHUNK_PER_XCD if order else TILE_MAJOR) and plan.launch_order(103) == TILE_MAJOR
        near = fa.RegridPlan(oracle.NEAREST, px, py, inX, inY, outX, outY)  # one shape, two orders
        assert near.tune_device(d_in.data_ptr(), nz, d_out.data_ptr(), st) == 0 and near.info()["launchOrder"] in (0, 1)
        assert cases.same(d_out.cpu().numpy(), oracle.interpolate_values(oracle.NEAREST, px, py, f, inX, inY, outX, outY))
        del plan, near
        fa.use_tuning_build(True)
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ORDER", "2")
        for alt in ("0", "1"):
            monkeypatch.setenv("FIMEX_AMD_STAGE2_USE_ALT", alt)
            plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
            assert plan.launch_order(nz) == CHUNK_PER_XCD and plan.launch_order(103) == TILE_MAJOR
            d_out.fill_(7.0)
            plan.apply_device(d_in.data_ptr(), nz, d_out.data_ptr(), st)
            torch.cuda.synchronize()
            assert cases.same(d_out.cpu().numpy(), want), ("forced order, shape " + alt, cases.describe_mismatch(d_out.cpu().numpy(), want))
            del plan
    finally:
        fa.use_tuning_build(was)
