"""A list of variables regridded in one call (fimex_amd_regrid_apply_multi_device / _typed_device / _host): the list kernels of the
second staged form (staged2_list.hip, staged2_list_typed.hip: path 1) and the per-variable calls inside the entry (path 0).

Every result is compared bit for bit, with identical NaN positions (cases.same; byte equality on stored types), with the oracle AND
with the per-variable device calls on the same buffers -- except bicubic in float arithmetic, which meets the oracle within the
tolerance rule of test_gpu_staged2_shapes.FloatCase and its per-variable calls bit for bit.

How the variables lie in memory (DeviceList): every variable is an allocation of its own, in an address order that is not the
list's; two variables are carved from one pool at offsets that are multiples of 4 bytes and not of 16; every output is pre-filled
with a sentinel and has guard elements before and after it, which must survive.
"""
import numpy as np
import pytest

import cases
import oracle
import test_gpu_staged2_shapes as shapes

pytestmark = pytest.mark.gpu

GUARD = 64       # guard elements on either side of an output
SENTINEL = 0xA5  # every byte of an output and its guards before the call
K = 64           # FIMEX_AMD_REGRID_MULTI_MAX_VARS


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert capi.REGRID_MULTI_MAX_VARS == K
    return capi


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class DeviceList:
    """Device copies of the variables `fields` ([nz_i][inY][inX] arrays of one dtype, nz_i may be 0) and their outputs of
    outLayer elements per slice.  pooled: two variables that share one allocation.  in_shift: variable -> bytes its source is
    moved behind a 4-byte boundary; out_shift: the same for its output (a variable with an allocation of its own), with whole
    guards on both sides still."""

    def __init__(self, fields, outLayer, seed, pooled=(1, 2), in_shift=None, out_shift=None):
        import torch
        self.dtype = fields[0].dtype
        es = self.dtype.itemsize
        self.nz = [int(f.shape[0]) for f in fields]
        n = len(fields)
        in_shift = in_shift or {}
        out_shift = out_shift or {}
        live = [i for i in range(n) if self.nz[i]]
        pooled = tuple(i for i in pooled if i in live) if len([i for i in pooled if i in live]) == 2 else ()
        inBytes = [f.nbytes for f in fields]
        self.outBytes = [z * outLayer * es for z in self.nz]
        guard = GUARD * es
        self.ins, self.outs = [0] * n, [0] * n
        self.out_tensors, self.regions, self.keep = [], [], []  # regions: (tensor index, first byte, variable)

        def off16(o):  # the next offset from o on that is a multiple of 4 and not of 16
            o = (o + 3) // 4 * 4
            return o + 4 if o % 16 == 0 else o

        # separate allocations of one size, handed out in an address order that is not the list's
        single = [i for i in live if i not in pooled]
        if single:
            sizeIn = max(inBytes[i] for i in single) + 16
            sizeOut = max(self.outBytes[i] for i in single) + 2 * guard + max(out_shift.values(), default=0)
            rng = np.random.default_rng(seed)
            for size, isOut in ((sizeIn, False), (sizeOut, True)):
                blocks = sorted((torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in single), key=lambda t: t.data_ptr())
                perm = rng.permutation(len(single))
                while len(single) > 1 and np.array_equal(perm, np.arange(len(single))):
                    perm = rng.permutation(len(single))
                for i, k in zip(single, perm):
                    t = blocks[k]
                    if isOut:
                        s = out_shift.get(i, 0)
                        assert t.data_ptr() % 4 == 0 and guard % 4 == 0
                        self.out_tensors.append(t)
                        self.regions.append((len(self.out_tensors) - 1, guard + s, i))
                        self.outs[i] = t.data_ptr() + guard + s
                    else:
                        s = in_shift.get(i, 0)
                        t[s:s + inBytes[i]] = torch.from_numpy(np.ascontiguousarray(fields[i]).view(np.uint8).ravel()).cuda()
                        self.keep.append(t)
                        self.ins[i] = t.data_ptr() + s
            if len(single) > 1:
                for ptrs in ([self.ins[i] for i in single], [self.outs[i] for i in single]):
                    assert ptrs != sorted(ptrs)
        assert all(i in single for i in out_shift), "out_shift: variables with an allocation of their own"
        if pooled:
            a, b = pooled
            oa = off16(0)
            ob = off16(oa + inBytes[a])
            pool = torch.zeros(ob + inBytes[b] + 16, dtype=torch.uint8, device="cuda")
            for i, o in ((a, oa), (b, ob)):
                pool[o:o + inBytes[i]] = torch.from_numpy(np.ascontiguousarray(fields[i]).view(np.uint8).ravel()).cuda()
                self.ins[i] = pool.data_ptr() + o
            self.keep.append(pool)
            oa = off16(guard)
            ob = off16(oa + self.outBytes[a] + guard)
            opool = torch.full((ob + self.outBytes[b] + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
            self.out_tensors.append(opool)
            for i, o in ((a, oa), (b, ob)):
                self.regions.append((len(self.out_tensors) - 1, o, i))
                self.outs[i] = opool.data_ptr() + o
            for i in pooled:
                assert self.ins[i] % 4 == 0 and self.ins[i] % 16 != 0 and self.outs[i] % 4 == 0 and self.outs[i] % 16 != 0
        self.outLayer = outLayer

    def results(self, shape2d):
        """the outputs per variable; asserts that every byte outside them still holds the sentinel"""
        import torch
        torch.cuda.synchronize()
        host = [t.cpu().numpy() for t in self.out_tensors]
        got = [np.zeros((0,) + shape2d, self.dtype) for _ in self.nz]
        outside = [np.ones(h.size, bool) for h in host]
        for k, o, i in self.regions:
            got[i] = host[k][o:o + self.outBytes[i]].view(self.dtype).reshape((self.nz[i],) + shape2d).copy()
            outside[k][o:o + self.outBytes[i]] = False
        for h, m in zip(host, outside):
            assert (h[m] == SENTINEL).all(), "a guard element was overwritten"
        return got

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out_tensors)


def run_list(fa, plan, fields, shape2d, seed, cdm=None, bads=None, **placing):
    """The list through the multi entry, and every variable through the plain entry on the same sources: the two must agree byte
    for byte.  Returns (results per variable, path)."""
    import torch
    outY, outX = shape2d
    dl = DeviceList(fields, outX * outY, seed, **placing)
    path = plan.apply_multi_device(dl.ins, dl.nz, dl.outs, _stream(), cdmType=cdm, badValue=bads)
    got = dl.results(shape2d)
    for i, z in enumerate(dl.nz):
        if z == 0:
            continue
        ref = torch.zeros(dl.outBytes[i], dtype=torch.uint8, device="cuda")
        if cdm is None:
            plan.apply_device(dl.ins[i], z, ref.data_ptr(), _stream())
        else:
            fa.regrid_apply_typed_device(plan, dl.ins[i], cdm, z, float(np.broadcast_to(bads, (len(dl.nz),))[i]), ref.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert np.array_equal(ref.cpu().numpy(), got[i].view(np.uint8).ravel()), "variable %d differs from its own call" % i
    return got, path


def split(f, nz):
    ends = np.cumsum(nz)
    return [f[e - z:e] for e, z in zip(ends, nz)]


def same_as_oracle(got, want, nz):
    for i, (g, w) in enumerate(zip(got, split(want, nz))):
        assert cases.same(g, w), (i, cases.describe_mismatch(g, w))


# ------------------------------------------------------------------------------------------------- 1. float lists, product build
GEOMETRY = (320, 18, 256, 16)  # 1.3 source cells per target cell, overshooting every side: undefined and border cells
NZ = (1, 5, 1, 12, 1, 7)


def float_case(kind, nz):
    return shapes.FloatCase(kind, *GEOMETRY, 1.3, -2.5, -1.7, nz=nz)


def plan_of(fa, case):
    plan = fa.RegridPlan(case.method, case.px, case.py, *case.shape, bicubic=getattr(fa, case.arith) if case.arith else None)
    assert plan.info()["stagedCells"] > 0
    return plan


def within_float_bicubic_tolerance(case, got, nz):
    """the rule of shapes.FloatCase.check: same NaN positions, within 1e-5 of the stencil's magnitude"""
    from numpy.lib.stride_tricks import sliding_window_view
    inX, inY, outX, outY = case.shape
    got = np.concatenate(got)
    assert np.array_equal(np.isnan(got), np.isnan(case.want[:nz]))
    x0, y0 = np.floor(case.px).astype(np.int64) - 1, np.floor(case.py).astype(np.int64) - 1
    ok = (x0 >= 0) & (x0 + 3 < inX) & (y0 >= 0) & (y0 + 3 < inY)
    for z in range(nz):
        mag = np.zeros(case.px.size, np.float32)
        mag[ok] = sliding_window_view(np.abs(np.nan_to_num(case.f[z])), (4, 4)).max(axis=(2, 3))[y0[ok], x0[ok]]
        d = np.abs(got[z].ravel().astype(np.float64) - case.want[z].ravel())
        fin = np.isfinite(case.want[z].ravel())
        assert fin.any() and (d[fin] <= 1e-5 * mag[fin]).all(), (z, float((d[fin] / mag[fin]).max()))


@pytest.mark.parametrize("kind", ["nearest", "bilinear", "bicubic_float"])
def test_float_lists_on_the_product_build(fa, kind):
    """27 slices in six variables.  The launch rule restated (staged2_z_chunks: tile-major order, chunks of about 25 slices of one
    size): two chunks, [0, 14) and [14, 27), whose boundary lies inside the fourth variable, slices [7, 19)."""
    total = sum(NZ)
    chunks = -(-total // 25)
    assert chunks == 2
    boundary = total // chunks + (1 if total % chunks else 0)
    begin = sum(NZ[:3])
    assert boundary == 14 and begin < boundary < begin + NZ[3]
    case = float_case(kind, total)
    plan = plan_of(fa, case)
    assert plan.launch_order(total) == 1  # tile-major: the split above is the launch's
    got, path = run_list(fa, plan, split(case.f, NZ), (GEOMETRY[3], GEOMETRY[2]), seed=1)
    assert path == 1
    if kind == "bicubic_float":
        within_float_bicubic_tolerance(case, got, total)
    else:
        same_as_oracle(got, case.want, NZ)


# ------------------------------------------------------------------------------------------------- 2. special tiles
@pytest.mark.parametrize("method", [oracle.BILINEAR, oracle.NEAREST])
def test_float_list_with_a_gather_tile_and_a_tile_row_without_chunks(fa, method):
    nz = (1, 1, 1, 1, 3)
    px, py, inX, inY, outY = shapes.typed_case(np.int16, method, 384)[:5]
    f = cases.field(sum(nz), inY, inX, seed=41, extremes=False)
    want = oracle.interpolate_values(method, px, py, f, inX, inY, 384, outY)
    plan = fa.RegridPlan(method, px, py, inX, inY, 384, outY)
    assert plan.info()["stagedCells"] > 0
    got, path = run_list(fa, plan, split(f, nz), (outY, 384), seed=2)
    assert path == 1
    same_as_oracle(got, want, nz)


def typed_fields(dt, inX, inY, nz, seed):
    """variables of the whole range of dt, each with a fill value of its own: one that occurs in the data, the ends of the range
    (the upper one occurs, the lower one does not), none at all (NaN)"""
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    choice = [float(info.min + 3), float(info.max), float("nan"), float(info.min)]
    fields, bads = [], []
    for i, z in enumerate(nz):
        f = rng.integers(info.min + 1, int(info.max) + 1, (z, inY, inX)).astype(dt)
        bad = choice[i % len(choice)]
        if bad == bad and bad != info.min:
            f.reshape(-1)[rng.random(f.size) < 0.03] = dt(bad)
        fields.append(f)
        bads.append(bad)
    return fields, bads


def typed_same_as_oracle(got, fields, bads, method, px, py, inX, inY, outX, outY):
    code = oracle.cdm_type_of(fields[0].dtype)
    for i, (g, f, bad) in enumerate(zip(got, fields, bads)):
        if f.shape[0] == 0:
            continue
        fl = oracle.interpolate_values(method, px, py, oracle.data2interpolation_array(f, bad), inX, inY, outX, outY)
        want = oracle.interpolation_array2data(fl, code, bad)
        # without a fill value an undefined result becomes (T)NaN, which C leaves undefined: those cells are not compared
        defined = np.ones(fl.shape, bool) if bad == bad else ~np.isnan(fl)
        assert np.array_equal(g[defined], want[defined]), (i, bad, int((g != want)[defined].sum()))


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR])
@pytest.mark.parametrize("dt", [np.int16, np.uint8])
@pytest.mark.parametrize("outX", [384, 383])
def test_stored_type_lists_with_a_fill_value_per_variable(fa, method, dt, outX):
    """even row lengths (two results per store: the pooled outputs are 4-byte aligned) and odd ones, on the tiles of
    shapes.typed_case: a gather tile and a tile row without chunks"""
    nz = (1, 1, 1, 1, 3)
    px, py, inX, inY, outY = shapes.typed_case(dt, method, outX)[:5]
    fields, bads = typed_fields(dt, inX, inY, nz, seed=outX + np.dtype(dt).itemsize)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    got, path = run_list(fa, plan, fields, (outY, outX), seed=3, cdm=oracle.cdm_type_of(dt), bads=bads)
    assert path == 1
    typed_same_as_oracle(got, fields, bads, method, px, py, inX, inY, outX, outY)


# ------------------------------------------------------------------------------------------------- 3. dispatch
def test_short_lists_zeros_single_variables_and_repeated_inputs(fa):
    case = float_case("bilinear", 12)
    plan = plan_of(fa, case)
    shape2d = (GEOMETRY[3], GEOMETRY[2])
    empty = case.f[:0]
    # three slices in all: the per-variable calls
    got, path = run_list(fa, plan, [case.f[0:1], empty, case.f[1:3]], shape2d, seed=4)
    assert path == 0
    same_as_oracle([got[0], got[2]], case.want[:3], (1, 2))
    # variables without slices inside a list that runs the list kernel
    nz = (1, 0, 5, 0, 1)
    got, path = run_list(fa, plan, split(case.f[:7], nz), shape2d, seed=5, pooled=(0, 2))
    assert path == 1
    same_as_oracle(got, case.want[:7], nz)
    # one variable: the plain entry
    got, path = run_list(fa, plan, [case.f[:6]], shape2d, seed=6)
    assert path == 1
    same_as_oracle(got, case.want[:6], (6,))
    # one input given twice, with two outputs
    dl = DeviceList([case.f[:4], case.f[4:8]], shape2d[0] * shape2d[1], seed=7, pooled=())
    assert plan.apply_multi_device([dl.ins[0], dl.ins[0]], dl.nz, dl.outs, _stream()) == 1
    got = dl.results(shape2d)
    same_as_oracle(got, np.concatenate([case.want[:4], case.want[:4]]), (4, 4))


def test_a_stored_type_source_that_is_not_4_byte_aligned_takes_the_per_variable_calls(fa):
    nz = (1, 2, 3)
    outX = 384
    px, py, inX, inY, outY = shapes.typed_case(np.int16, oracle.BILINEAR, outX)[:5]
    fields, bads = typed_fields(np.int16, inX, inY, nz, seed=77)
    plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
    got, path = run_list(fa, plan, fields, (outY, outX), seed=8, cdm=oracle.cdm_type_of(np.int16), bads=bads, pooled=(), in_shift={1: 2})
    assert path == 0
    typed_same_as_oracle(got, fields, bads, oracle.BILINEAR, px, py, inX, inY, outX, outY)
    got, path = run_list(fa, plan, fields, (outY, outX), seed=8, cdm=oracle.cdm_type_of(np.int16), bads=bads, pooled=())
    assert path == 1


def test_plans_without_a_list_kernel_take_the_per_variable_calls(fa):
    """bicubic in the reference's arithmetic (first staged form), a forward plan, and a coord-NN plan on positions without spatial
    coherence (no staged form at all); a 4-byte stored type on a plan that has the list kernel for floats"""
    nz = (1, 5, 1, 2)
    total = sum(nz)
    shape2d = (GEOMETRY[3], GEOMETRY[2])
    case = float_case("bicubic", total)
    plan = fa.RegridPlan(case.method, case.px, case.py, *case.shape, bicubic=fa.BICUBIC_REFERENCE)
    got, path = run_list(fa, plan, split(case.f, nz), shape2d, seed=9)
    assert path == 0
    same_as_oracle(got, case.want, nz)

    inX, inY, outX, outY = GEOMETRY
    rng = np.random.default_rng(5)
    px, py = rng.uniform(-1, outX, inX * inY), rng.uniform(-1, outY, inX * inY)
    plan = fa.RegridPlan(fa.FORWARD_MEAN, px, py, inX, inY, outX, outY)
    got, path = run_list(fa, plan, split(case.f, nz), shape2d, seed=10)
    assert path == 0  # (run_list has compared every variable with its own call)

    # scattered positions on a source of 400 rows: every tile spans more source rows than a tile may, no staged form is kept
    cx, cy = 600, 400
    px, py = rng.uniform(-1, cx, outX * outY), rng.uniform(-1, cy, outX * outY)
    plan = fa.RegridPlan(oracle.COORD_NN, px, py, cx, cy, outX, outY)
    assert plan.launch_order(total) == -1
    f = cases.field(total, cy, cx, seed=21, extremes=False)
    got, path = run_list(fa, plan, split(f, nz), shape2d, seed=11)
    assert path == 0
    same_as_oracle(got, oracle.interpolate_values(oracle.COORD_NN, px, py, f, cx, cy, outX, outY), nz)

    near = float_case("nearest", total)
    plan = plan_of(fa, near)
    f32 = np.random.default_rng(6).integers(-2 ** 31 + 1, 2 ** 31, near.f.shape).astype(np.int32)
    got, path = run_list(fa, plan, split(f32, nz), shape2d, seed=12, cdm=oracle.cdm_type_of(np.int32), bads=-7.0)
    assert path == 0


# ------------------------------------------------------------------------------------------------- 4. more variables than one launch takes
def test_one_variable_more_than_a_launch_takes(fa):
    nz = (1,) * (K + 1)
    case = float_case("bilinear", K + 1)
    plan = plan_of(fa, case)
    got, path = run_list(fa, plan, split(case.f, nz), (GEOMETRY[3], GEOMETRY[2]), seed=13, pooled=(K - 1, K))
    assert path == 1
    same_as_oracle(got, case.want, nz)


# ------------------------------------------------------------------------------------------------- 5. tuning build
NZ_TUNING = (1,) * 7 + (3,)


@pytest.mark.parametrize("kind", ["nearest", "bilinear", "bicubic_float"])
def test_ring_depths_with_chunks_of_two_slices(fa, tuning_build, monkeypatch, kind):
    """STAGE2_DEPTH 2 and 3, STAGE2_ZPB 2: five chunks of two slices; with three slots the source cursor is two variables ahead of
    the result cursor.  Then STAGED_MIN_NZ 1 with a list of one slice."""
    total = sum(NZ_TUNING)
    case = float_case(kind, total)
    shape2d = (GEOMETRY[3], GEOMETRY[2])
    first = None
    for depth in ("2", "3"):
        monkeypatch.setenv("FIMEX_AMD_STAGE2_DEPTH", depth)
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ZPB", "2")
        plan = plan_of(fa, case)
        got, path = run_list(fa, plan, split(case.f, NZ_TUNING), shape2d, seed=14)
        assert path == 1
        if kind == "bicubic_float":
            within_float_bicubic_tolerance(case, got, total)
            first = first or got
            assert all(cases.same(g, h) for g, h in zip(got, first))
        else:
            same_as_oracle(got, case.want, NZ_TUNING)
        monkeypatch.setenv("FIMEX_AMD_STAGED_MIN_NZ", "1")
        got, path = run_list(fa, plan, [case.f[:1]], shape2d, seed=15)
        assert path == 1
        if kind != "bicubic_float":
            same_as_oracle(got, case.want[:1], (1,))
        monkeypatch.delenv("FIMEX_AMD_STAGED_MIN_NZ")


@pytest.mark.parametrize("dt,method", [(np.int16, oracle.BILINEAR), (np.uint8, oracle.NEAREST)])
def test_stored_type_ring_depths_with_chunks_of_two_slices(fa, tuning_build, monkeypatch, dt, method):
    outX = 384
    px, py, inX, inY, outY = shapes.typed_case(dt, method, outX)[:5]
    fields, bads = typed_fields(dt, inX, inY, NZ_TUNING, seed=91)
    code = oracle.cdm_type_of(dt)
    for depth in ("2", "3"):
        monkeypatch.setenv("FIMEX_AMD_STAGE2T_DEPTH", depth)
        monkeypatch.setenv("FIMEX_AMD_STAGE2T_ZPB", "2")
        plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
        got, path = run_list(fa, plan, fields, (outY, outX), seed=16, cdm=code, bads=bads)
        assert path == 1
        typed_same_as_oracle(got, fields, bads, method, px, py, inX, inY, outX, outY)
        monkeypatch.setenv("FIMEX_AMD_STAGED_MIN_NZ", "1")
        got, path = run_list(fa, plan, fields[:1], (outY, outX), seed=17, cdm=code, bads=bads[:1])
        assert path == 1
        typed_same_as_oracle(got, fields[:1], bads[:1], method, px, py, inX, inY, outX, outY)
        monkeypatch.delenv("FIMEX_AMD_STAGED_MIN_NZ")


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_overlapping_outputs_are_refused_and_nothing_is_written(fa):
    case = float_case("bilinear", 8)
    plan = plan_of(fa, case)
    shape2d = (GEOMETRY[3], GEOMETRY[2])
    dl = DeviceList([case.f[:4], case.f[4:8]], shape2d[0] * shape2d[1], seed=18, pooled=())
    with pytest.raises(fa.FimexAmdError, match="an output overlaps another array of the list"):
        plan.apply_multi_device(dl.ins, dl.nz, [dl.outs[0], dl.outs[0] + 4], _stream())
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        plan.apply_multi_device(dl.ins, dl.nz, [dl.outs[0], dl.ins[0] + 8], _stream())
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        plan.apply_multi_device(dl.ins, dl.nz, [dl.ins[1] + 8, dl.outs[1]], _stream())
    code = oracle.cdm_type_of(np.float32)
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        plan.apply_multi_device(dl.ins, dl.nz, [dl.outs[1] + 4, dl.outs[1]], _stream(), cdmType=code, badValue=0.0)
    assert dl.untouched()


# ------------------------------------------------------------------------------------------------- 7. host form
def test_host_forms_equal_the_device_forms(fa):
    case = float_case("bilinear", sum(NZ))
    plan = plan_of(fa, case)
    got, path = plan.apply_multi_host(split(case.f, NZ))
    assert path == 1
    same_as_oracle(got, case.want, NZ)
    got, path = plan.apply_multi_host([case.f[:1], case.f[:0], case.f[1:3]])
    assert path == 0
    same_as_oracle([got[0], got[2]], case.want[:3], (1, 2))

    nz = (1, 1, 0, 3)
    outX = 384
    px, py, inX, inY, outY = shapes.typed_case(np.int16, oracle.BILINEAR, outX)[:5]
    fields, bads = typed_fields(np.int16, inX, inY, nz, seed=55)
    plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
    dev, path = run_list(fa, plan, fields, (outY, outX), seed=19, cdm=oracle.cdm_type_of(np.int16), bads=bads, pooled=())
    assert path == 1
    got, path = plan.apply_multi_host(fields, badValue=bads)
    assert path == 1
    assert all(np.array_equal(g, d) for g, d in zip(got, dev))
