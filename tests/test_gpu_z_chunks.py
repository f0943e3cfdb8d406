"""The multi-slice loops of the gather, vector and border-smoothing kernels against the CPU oracle.

Every streaming kernel cuts a batch into z chunks of zPerBlock slices per workgroup and walks a chunk with an unrolled main loop
(several slices in flight: one buffer descriptor over ZC slices with the slice index in the scalar offset, or a pointer advanced
by several slices per pass) followed by a one-slice tail.  The launch rules give zPerBlock > 1 only where the grid alone already
fills the chip, so at the small shapes of the other modules every chunk is one slice and only the tails run.  Here the main loops
run, at least twice in one workgroup and with a tail behind them, in two ways: on the tuning build with zPerBlock forced
(FIMEX_AMD_ZPB for the gather kernels, FIMEX_AMD_VECTOR_ZPB for the rotations) at small shapes, and on the product build at the
smallest shapes at which the launch rule itself chooses zPerBlock > 1.  The product-build tests restate the launch rule and assert
the zPerBlock it gives: a retuned launcher must fail them, not turn them back into one-slice tests.

Passes of the main loop per chunk (tail slices behind them), by (zPerBlock, nz):
  gather_apply<STENCIL, ZC, T> (csrc/gather.hip):
  <1, 16, float>               (16, 16) 1; (17, 35) 1 + 1; (40, 83) 2 + 8; product (17, 17) 1 + 1
  <2, 8, float>                (16, 16) 2; (17, 35) 2 + 1; (8, 20) 1; (40, 83) 5; product (17, 17) 2 + 1
  <2, 16 / 4 / 2, float>       (17, 35) 1 + 1 / 4 + 1 / 8 + 1
  <4, 2, float>                (16, 16) 8; (17, 35) 8 + 1; (8, 20) 4; (3, 7) 1 + 1; (40, 83) 20
  <1 | 2, 8, stored types>     (8, 19) 1, last chunk 3 tail slices; (17, 19) 2 + 1
  apply_few<1 | 2, 2 / 4 / 8>  one slice, FEW_CELLS cells per lane
  rotate_values_vec4           VECTOR_ZPB 2 / 3 / 4 / 5 / 9: 1 / 1 + 1 / 2 / 2 + 1 / 4 + 1; product (3, 80) 1 + 1
  rotate_direction_vec4        the same
  rotate_direction             VECTOR_ZPB 4 / 5 / 9: 1 / 1 + 1 / 2 + 1; product (5, 80) 1 + 1
  border_smooth_kernel         product (12, 17): 3 in one workgroup, 1 + 1 in the other

Comparisons are bit for bit with identical NaN positions (cases.same, np.array_equal on the bytes of stored types).  The inputs
hold NaN, infinities, -0.0 and denormals, and the positions overshoot the source, so undefined cells and bilinear border cells lie
inside multi-slice chunks too.
"""
import functools

import numpy as np
import pytest

import cases
import merge_ref as mr
import oracle

pytestmark = pytest.mark.gpu

METHODS = [oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC]
METHOD_IDS = ["nearest", "bilinear", "bicubic"]


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


def _ceil_div(a, b):
    return -(-a // b)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)  # shared between tests
    return arrays


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared inputs are read-only


def _check_plan_info(plan, method):
    info = plan.info()
    assert info["undefinedCells"] > 0  # write_undefined over a multi-slice chunk
    if method == oracle.BILINEAR:
        assert info["borderCells"] > 0  # border entries (zero steps for the neighbours they lack) inside a multi-slice chunk


# ------------------------------------------------------------------------------------------- 1. gather kernels on floats, forced ZPB
GATHER_GEOMETRY = (120, 90, 100, 70)  # 36 tiles: the launch rule alone gives one slice per workgroup
ZPB_NZ = [(16, 16), (17, 35), (8, 20), (3, 7), (40, 83)]


@functools.lru_cache(maxsize=None)
def _gather_case(method, nz):
    inX, inY, outX, outY = GATHER_GEOMETRY
    px, py = cases.backward_positions(inX, inY, outX, outY, seed=5)
    f = cases.field(nz, inY, inX, seed=300 + nz)
    want = oracle.interpolate_values(method, px, py, f, inX, inY, outX, outY)
    return _frozen(px, py, f, want)


def _gather_on_device(fa, method, px, py, f, geometry):
    import torch
    inX, inY, outX, outY = geometry
    nz = f.shape[0]
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    d_in = _dev(f)
    d_out = torch.full((nz, outY, outX), -7.0, dtype=torch.float32, device="cuda")
    plan.apply_gather_device(d_in.data_ptr(), nz, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check_plan_info(plan, method)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("zpb,nz", ZPB_NZ)
def test_gather_main_loops_with_forced_chunks(fa, monkeypatch, method, zpb, nz, tuning_build):
    """gather_apply<1, 16>, <2, 8> and <4, 2> on floats with chunks of several slices: a chunk of 17 is 16 + 1, 2 x 8 + 1 and
    8 x 2 + 1 slices; where ZPB does not divide nz the last chunk is shorter than the others"""
    monkeypatch.setenv("FIMEX_AMD_ZPB", str(zpb))
    px, py, f, want = _gather_case(method, nz)
    got = _gather_on_device(fa, method, px, py, f, GATHER_GEOMETRY)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


@pytest.mark.parametrize("knobs", [{"BILINEAR_ZC": "16"}, {"BILINEAR_ZC": "4"}, {"BILINEAR_ZC": "2"}, {"BILINEAR_ZC": "1"}, {"NT": "0"},
                                   {"BILINEAR_ZC": "16", "NT": "0"}, {"BILINEAR_ZC": "4", "NT": "0"}],
                         ids=lambda k: "-".join("%s%s" % kv for kv in sorted(k.items())))
def test_bilinear_gather_other_instantiations(fa, monkeypatch, knobs, tuning_build):
    """the other gather_apply<2, ZC, float, NT> kernels that the sweeps launch, on chunks of 17 slices and a last chunk of one"""
    monkeypatch.setenv("FIMEX_AMD_ZPB", "17")
    for k, v in knobs.items():
        monkeypatch.setenv("FIMEX_AMD_" + k, v)
    px, py, f, want = _gather_case(oracle.BILINEAR, 35)
    got = _gather_on_device(fa, oracle.BILINEAR, px, py, f, GATHER_GEOMETRY)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("cells", [2, 4, 8])
def test_one_slice_kernels_with_every_cells_per_lane(fa, monkeypatch, method, cells, tuning_build):
    """apply_few<1 | 2, CELLS> on one slice: 64 x (4 * CELLS) tiles on a 100 x 70 target, so every shape has lanes beyond the slice and
    partly filled tiles (100 % 64 != 0; 70 is no multiple of 8, 16 or 32); undefined entries (their loads are dropped) and bilinear
    border entries lie among the cells of one lane"""
    monkeypatch.setenv("FIMEX_AMD_FEW_CELLS", str(cells))
    px, py, f, want = _gather_case(method, 1)
    got = _gather_on_device(fa, method, px, py, f, GATHER_GEOMETRY)  # asserts the plan's undefined and border cells
    assert cases.same(got, want), cases.describe_mismatch(got, want)


# ------------------------------------------------------------------------------------- 2. gather kernels on stored types, forced ZPB
# outX odd and inX * inY odd: the slices of the byte types start on odd addresses inside a descriptor over 8 slices
TYPED_GEOMETRY = (97, 71, 151, 110)
TYPED_NZ = 19
TYPED = [(np.int16, -32767.0), (np.uint16, 65535.0), (np.int8, -127.0), (np.uint8, 255.0), (np.int32, -2147483647.0), (np.int16, float("nan"))]


@functools.lru_cache(maxsize=None)
def _typed_case(method, dt, bad):
    inX, inY, outX, outY = TYPED_GEOMETRY
    px, py = cases.backward_positions(inX, inY, outX, outY, seed=12)
    rng = np.random.default_rng(3)
    info = np.iinfo(dt)
    f = rng.integers(max(info.min, -30000) // 2, min(info.max, 30000) // 2 + 1, (TYPED_NZ, inY, inX)).astype(dt)
    if bad == bad:  # a NaN fill value marks nothing in integer data
        f.reshape(-1)[rng.choice(f.size, f.size // 25, replace=False)] = dt(bad)
    want = oracle.interpolation_array2data(
        oracle.interpolate_values(method, px, py, oracle.data2interpolation_array(f, bad), inX, inY, outX, outY), oracle.cdm_type_of(dt), bad)
    return _frozen(px, py, f, want)


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("dt,bad", TYPED, ids=lambda p: p.__name__ if isinstance(p, type) else "bad%g" % p)
@pytest.mark.parametrize("zpb", [8, 17])
def test_typed_gather_main_loops_with_forced_chunks(fa, monkeypatch, method, dt, bad, zpb, tuning_build):
    """gather_apply on the stored type with 8 slices behind one descriptor: chunks of 8, 8 and 3 slices, and of 2 x 8 + 1 and 2
    (bicubic: one slice at a time); against the oracle's three steps"""
    import torch
    monkeypatch.setenv("FIMEX_AMD_TYPED_STAGED", "0")
    monkeypatch.setenv("FIMEX_AMD_TYPED_FUSED", "2")
    monkeypatch.setenv("FIMEX_AMD_ZPB", str(zpb))
    inX, inY, outX, outY = TYPED_GEOMETRY
    assert (inX * inY) % 4 != 0 and outX % 2 == 1
    px, py, f, want = _typed_case(method, dt, bad)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    _check_plan_info(plan, method)
    t = _dev(f.view(np.uint8))
    out = torch.full((TYPED_NZ * outY * outX * np.dtype(dt).itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    fa.regrid_apply_typed_device(plan, t.data_ptr(), oracle.cdm_type_of(dt), TYPED_NZ, bad, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(dt).reshape(want.shape)
    differ = np.argwhere(got != want)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "%d cells differ; first (z, y, x): %s" % (len(differ), differ[:5].tolist())


# -------------------------------------------------------------------------------------------- 3. gather kernels, the launch rule itself
def _gather_z_per_block(outX, outY, nz):
    """make_args of csrc/gather.hip at its defaults: 64 x 4 tiles, chunks so that 256 * 8 * 4 workgroups exist, at most 40
    slices per workgroup"""
    tiles = _ceil_div(outX, 64) * _ceil_div(outY, 4)
    chunks = max(1, min(nz, _ceil_div(256 * 8 * 4, tiles)))
    return min(_ceil_div(nz, chunks), 40, nz)


PRODUCT_GEOMETRY = (96, 64, 1024, 2048)  # 16 x 512 = 8192 tiles: the smallest grid at which one workgroup takes the whole batch
PRODUCT_NZ = 17


@functools.lru_cache(maxsize=None)
def _product_inputs():
    inX, inY, outX, outY = PRODUCT_GEOMETRY
    px, py = cases.backward_positions(inX, inY, outX, outY, seed=21)
    f = cases.field(PRODUCT_NZ, inY, inX, seed=22)
    return _frozen(px, py, f)


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
def test_gather_main_loops_under_the_launch_rule(fa, method):
    """the product library at the smallest shape at which its own rule gives zPerBlock > 1: 17 slices in one workgroup, 16 + 1 for
    gather_apply<1, 16, float> and 2 x 8 + 1 for gather_apply<2, 8, float>"""
    import torch
    inX, inY, outX, outY = PRODUCT_GEOMETRY
    assert _gather_z_per_block(outX, outY, PRODUCT_NZ) == 17
    px, py, f = _product_inputs()
    want = oracle.interpolate_values(method, px, py, f, inX, inY, outX, outY, nthreads=16)
    got = _gather_on_device(fa, method, px, py, f, PRODUCT_GEOMETRY)
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    del got, want
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ 4. vector kernels
SENTINEL = np.float32(-12345.678)
SCALE, OFFSET = 0.1, 5.0  # of the packed directions
PAD = 16  # floats of sentinel on either side of the data (one more on the side the data is shifted away from)


class _Padded:
    """a [oz][oy][ox] float32 field inside a larger device allocation: 16 floats of sentinel in front, 16-byte aligned data
    (shift 0) or data that starts 4 bytes later (shift 1), sentinel behind"""

    def __init__(self, a, shift):
        host = np.full(a.size + 2 * PAD + 1, SENTINEL, np.float32)
        self.lo, self.shape = PAD + shift, a.shape
        host[self.lo:self.lo + a.size] = a.reshape(-1)
        self.t = _dev(host)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * self.lo

    def result(self):
        """the data after the call; the sentinels on both sides must have survived it"""
        h = self.t.cpu().numpy()
        n = int(np.prod(self.shape))
        pad = np.concatenate([h[:self.lo], h[self.lo + n:]])
        assert pad.size == 2 * PAD + 1 and np.all(pad.view(np.uint32) == SENTINEL.view(np.uint32)), "the call wrote outside its field"
        return h[self.lo:self.lo + n].reshape(self.shape)


def _stream(side):
    import torch
    return torch.cuda.Stream() if side else torch.cuda.current_stream()


@functools.lru_cache(maxsize=None)
def _vector_case(ox, oy, oz):
    m = cases.rotation_matrix(ox, oy, seed=ox)
    u = cases.field(oz, oy, ox, seed=1)
    v = cases.field(oz, oy, ox, seed=2) - 280
    wu, wv = oracle.vector_reproject_values(m, u, v, ox, oy)
    rng = np.random.default_rng(3)
    ang = rng.uniform(-30, 400, (oz, oy, ox)).astype(np.float32)
    ang.reshape(-1)[rng.choice(ang.size, 6, replace=False)] = [np.nan, np.inf, -np.inf, 0.0, 360.0, -0.0]
    wa = oracle.vector_reproject_direction(m, ang, ox, oy)
    # packed directions: unpack in double, the oracle's rotation, pack again (src/CDMProcessor.cc:621-636)
    packed = rng.integers(0, 3600, (oz, oy, ox)).astype(np.float32)
    packed[0, 0, :3] = np.nan
    unpacked = (SCALE * packed.astype(np.float64) + OFFSET).astype(np.float32)
    rotated = oracle.vector_reproject_direction(m, unpacked, ox, oy)
    wp = ((1 / SCALE) * (rotated.astype(np.float64) - OFFSET)).astype(np.float32)
    return _frozen(m, u, v, wu, wv, ang, wa, packed, wp)


VECTOR_LAYERS = [(64, 48), (101, 37), (16, 4)]
VECTOR_ZPB = [2, 3, 4, 5, 9]
# (shift of u, shift of v): both aligned takes the vec4 kernel where layer % 4 == 0, every other pair the scalar kernel
VALUE_SHIFTS = [(0, 0), (1, 1), (1, 0), (0, 1)]


def _layer_shifts(shifts):
    """every layer on aligned tensors; the layers with layer % 4 == 0, which choose their kernel by the alignment, on the others too"""
    return [pytest.param(layer, s, id="%dx%d-shift%s" % (layer + ("".join(map(str, np.atleast_1d(s))),)))
            for layer in VECTOR_LAYERS for s in shifts if (layer[0] * layer[1]) % 4 == 0 or s == shifts[0]]


def _rotate_values(plan, u, v, shifts, side):
    import torch
    s = _stream(side)
    with torch.cuda.stream(s):
        du, dv = _Padded(u, shifts[0]), _Padded(v, shifts[1])
        plan.reproject_values_device(du.ptr, dv.ptr, u.shape[0], s.cuda_stream)
        s.synchronize()
        return du.result(), dv.result()


def _rotate_angles(plan, ang, shift, side, scaled=False):
    import torch
    s = _stream(side)
    with torch.cuda.stream(s):
        d = _Padded(ang, shift)
        if scaled:
            plan.reproject_direction_scaled_device(d.ptr, ang.shape[0], SCALE, OFFSET, s.cuda_stream)
        else:
            plan.reproject_direction_device(d.ptr, ang.shape[0], s.cuda_stream)
        s.synchronize()
        return d.result()


@pytest.mark.parametrize("layer,shifts", _layer_shifts(VALUE_SHIFTS))
@pytest.mark.parametrize("zpb", VECTOR_ZPB)
def test_vector_values_with_forced_chunks(fa, monkeypatch, layer, shifts, zpb, tuning_build):
    """rotate_values_vec4 (two slices in flight) and rotate_values_scalar on chunks of zpb, zpb and 1 slices; a u or v that is not
    16-byte aligned takes the scalar kernel although layer % 4 == 0"""
    monkeypatch.setenv("FIMEX_AMD_VECTOR_ZPB", str(zpb))
    (ox, oy), oz = layer, 2 * zpb + 1
    m, u, v, wu, wv = _vector_case(ox, oy, oz)[:5]
    gu, gv = _rotate_values(fa.VectorPlan(m, ox, oy), u, v, shifts, side=zpb in (3, 9))
    assert cases.same(gu, wu), cases.describe_mismatch(gu, wu)
    assert cases.same(gv, wv), cases.describe_mismatch(gv, wv)


@pytest.mark.parametrize("layer,shift", _layer_shifts([0, 1]))
@pytest.mark.parametrize("zpb", VECTOR_ZPB)
@pytest.mark.parametrize("scaled", [False, True], ids=["direction", "direction_scaled"])
def test_vector_directions_with_forced_chunks(fa, monkeypatch, layer, shift, zpb, scaled, tuning_build):
    """rotate_direction_vec4 (two slices in flight), rotate_direction (four) and rotate_direction_scaled on chunks of zpb, zpb and 1
    slices"""
    monkeypatch.setenv("FIMEX_AMD_VECTOR_ZPB", str(zpb))
    (ox, oy), oz = layer, 2 * zpb + 1
    case = _vector_case(ox, oy, oz)
    m, (ang, want) = case[0], (case[7:9] if scaled else case[5:7])
    got = _rotate_angles(fa.VectorPlan(m, ox, oy), ang, shift, side=zpb in (2, 5), scaled=scaled)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


def _vector_z_per_block(layer, oz, cells_per_lane):
    """make_args of csrc/vector.hip (:168-173) with VECTOR_ZPB at its default: chunks so that 256 * 8 * 2 workgroups exist"""
    blocks_x = _ceil_div(_ceil_div(layer, cells_per_lane), 256)
    chunks = max(1, min(oz, _ceil_div(256 * 8 * 2, blocks_x)))
    return _ceil_div(oz, chunks)


@pytest.mark.parametrize("ox,oy,shift,cells_per_lane,z_per_block", [(512, 256, 0, 4, 3), (256, 256, 1, 1, 5)], ids=["vec4_3_slices", "scalar_5_slices"])
def test_vector_main_loops_under_the_launch_rule(fa, ox, oy, shift, cells_per_lane, z_per_block):
    """the product library at the smallest layers at which its own rule gives zPerBlock > 1 for 80 slices: 27 chunks of 3 (the last
    of 2) for the vec4 kernels on aligned tensors, 16 chunks of 5 (four slices in flight plus one) for the scalar kernels on tensors
    that start 4 bytes off"""
    import torch
    oz = 80
    assert _vector_z_per_block(ox * oy, oz, cells_per_lane) == z_per_block
    m, u, v, wu, wv, ang, wa = _vector_case(ox, oy, oz)[:7]
    plan = fa.VectorPlan(m, ox, oy)
    gu, gv = _rotate_values(plan, u, v, (shift, shift), side=False)
    assert cases.same(gu, wu), cases.describe_mismatch(gu, wu)
    assert cases.same(gv, wv), cases.describe_mismatch(gv, wv)
    del gu, gv
    ga = _rotate_angles(plan, ang, shift, side=True)
    assert cases.same(ga, wa), cases.describe_mismatch(ga, wa)
    del ga
    _vector_case.cache_clear()  # the small cases above are done; these two hold 0.4 GB
    torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------- 5. border smoothing, the launch rule itself
def _smooth_z_per_block(nx, ny, nz):
    """tile_grid of csrc/merge.hip (:322-336): 64 x 4 tiles, chunks so that 256 * 8 * 4 workgroups exist, zPerBlock rounded up to the
    4 slices in flight; -> (zPerBlock, chunks)"""
    tiles = _ceil_div(nx, 64) * _ceil_div(ny, 4)
    chunks = min(nz, _ceil_div(256 * 8 * 4, tiles))
    zpb = _ceil_div(_ceil_div(nz, chunks), 4) * 4
    if _ceil_div(nz, zpb) > 65535:
        zpb = _ceil_div(nz, 65535)
    return zpb, _ceil_div(nz, zpb)


def _smooth_fields(nx, ny, nz, seed):
    """(I, O) [nz][ny][nx]: two random planes, shifted and offset from slice to slice so that no two slices are alike; about 10 % NaN in
    each, and infinities, zeros of either sign and equal values in every slice"""
    rng = np.random.default_rng(seed)
    planes = rng.normal(280, 5, (2, ny * nx)).astype(np.float32)
    holes = rng.random((2, ny * nx)) < 0.1
    special = [(np.inf, 1.), (1., -np.inf), (np.inf, np.inf), (-np.inf, np.inf), (0., -0.), (-0., 0.), (0., 0.), (3.5, 3.5), (0., 1.), (-0., 2.)]
    I, O = np.empty((nz, ny * nx), np.float32), np.empty((nz, ny * nx), np.float32)
    for z in range(nz):
        I[z] = np.roll(planes[0], 1009 * z) + np.float32(0.25 * z)
        O[z] = np.roll(planes[1], -733 * z) - np.float32(0.25 * z)
        for p, (vi, vo) in zip(rng.integers(0, ny * nx, len(special)), special):
            I[z, p], O[z, p] = vi, vo
        I[z][np.roll(holes[0], 517 * z)] = np.nan
        O[z][np.roll(holes[1], -389 * z)] = np.nan
    return I.reshape(nz, ny, nx), O.reshape(nz, ny, nx)


def test_border_smooth_main_loop_under_the_launch_rule(fa):
    """border_smooth_kernel on 1024 x 1024 x 17: 4096 tiles, two z chunks of 12 slices; the workgroups of the first make three passes
    of the four-slice loop, those of the second one pass and a one-slice tail.  Out of place and in place on the inner."""
    import torch
    from test_gpu_merge import _identical
    nx, ny, nz, tw, bw = 1024, 1024, 17, 40, 3
    assert _smooth_z_per_block(nx, ny, nz) == (12, 2)
    I, O = _smooth_fields(nx, ny, nz, 9)
    want = mr.border_smooth(I, O, tw, bw, True)
    stream = torch.cuda.current_stream().cuda_stream
    dI, dO = _dev(I), _dev(O)
    out = torch.full((nz, ny, nx), -7.0, dtype=torch.float32, device="cuda")
    fa.border_smooth_device(dI.data_ptr(), dO.data_ptr(), out.data_ptr(), nx, ny, nz, tw, bw, True, stream)
    _identical(out.cpu().numpy(), want, "border_smooth 1024x1024x17 out of place")
    assert np.array_equal(dI.cpu().numpy().view(np.uint32), I.view(np.uint32)) and np.array_equal(dO.cpu().numpy().view(np.uint32), O.view(np.uint32))
    fa.border_smooth_device(dI.data_ptr(), dO.data_ptr(), dI.data_ptr(), nx, ny, nz, tw, bw, True, stream)
    _identical(dI.cpu().numpy(), want, "border_smooth 1024x1024x17 in place on the inner")
    del dI, dO, out
    torch.cuda.empty_cache()
