"""ctypes front-end of oracle/_ref/libmifi_ref.so: the reference's own src/interpolation.c and
src/vertical_coordinate_transformations.c, compiled unmodified with oracle/ref_shim (recipe in oracle/Makefile).

TEST INFRASTRUCTURE ONLY.  Signatures are those of the reference's include/fimex/interpolation.h and
include/fimex/vertical_coordinate_transformations.h: the point functions and the rotations take int sizes, the two
*_by_matrix_f functions a leading int method, the fills and blends size_t.  The methods mirror the oracle's front-end
(oracle/__init__.py) so that a test calls both sides with the same arguments; they add the return code where the oracle's
front-end drops it.  Inputs on which the reference reads out of bounds (divergences D1, D2, D5 of oracle/fimex_oracle.c)
must never reach these functions: that is the caller's duty (tests/test_oracle_vs_reference.py computes the masks).
"""
import ctypes

import numpy as np

_F = ctypes.POINTER(ctypes.c_float)
_D = ctypes.POINTER(ctypes.c_double)
_Z = ctypes.c_size_t
_I = ctypes.c_int
_S = ctypes.c_char_p
_TRANSFORM = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_long, _D, _D)

MIFI_VECTOR_KEEP_SIZE = 0  # include/fimex/mifi_constants.h
BLENDS = ("mifi_get_values_nearest_f", "mifi_get_values_linear_f", "mifi_get_values_linear_weak_extrapol_f",
          "mifi_get_values_linear_no_extrapol_f", "mifi_get_values_linear_const_extrapol_f", "mifi_get_values_log_f",
          "mifi_get_values_log_log_f")  # in the order of the oracle's BLEND_* codes


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _f(a):
    return a.ctypes.data_as(_F)


def _d(a):
    return a.ctypes.data_as(_D)


class Reference:
    def __init__(self, path):
        self.path = path
        L = self.lib = ctypes.CDLL(path)
        self._hook = None
        L.ref_shim_set_transform.argtypes = [_TRANSFORM]
        L.ref_shim_set_transform.restype = None
        L.ref_shim_get_values_batch.argtypes = [_I, _F, _F, _D, _D, ctypes.POINTER(ctypes.c_ubyte), ctypes.c_long, _I, _I, _I]
        L.ref_shim_get_values_batch.restype = _I
        for name in ("mifi_get_values_f", "mifi_get_values_bilinear_f", "mifi_get_values_bicubic_f"):
            getattr(L, name).argtypes = [_F, _F, ctypes.c_double, ctypes.c_double, _I, _I, _I]
            getattr(L, name).restype = _I
        L.mifi_vector_reproject_values_by_matrix_f.argtypes = [_I, _D, _F, _F, _I, _I, _I]
        L.mifi_vector_reproject_direction_by_matrix_f.argtypes = [_I, _D, _F, _I, _I, _I]
        L.mifi_get_vector_reproject_matrix.argtypes = [_S, _S, _D, _D, _I, _I, _I, _I, _D]
        L.mifi_get_vector_reproject_matrix_field.argtypes = [_S, _S, _D, _D, _I, _I, _D]
        L.mifi_get_vector_reproject_matrix_points.argtypes = [_S, _S, _I, _D, _D, _I, _D]
        L.mifi_project_values.argtypes = [_S, _S, _D, _D, _I]
        L.mifi_project_axes.argtypes = [_S, _S, _D, _D, _I, _I, _D, _D]
        L.mifi_points2position.argtypes = [_D, _I, _D, _I, _I]
        L.mifi_fill2d_f.argtypes = [_Z, _Z, _F, ctypes.c_float, ctypes.c_float, _Z, ctypes.POINTER(_Z)]
        L.mifi_creepfill2d_f.argtypes = [_Z, _Z, _F, ctypes.c_ushort, ctypes.c_char, ctypes.POINTER(_Z)]
        L.mifi_creepfillval2d_f.argtypes = [_Z, _Z, _F, ctypes.c_float, ctypes.c_ushort, ctypes.c_char, ctypes.POINTER(_Z)]
        for name in BLENDS:
            getattr(L, name).argtypes = [_F, _F, _F, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        L.mifi_get_values_linear_d.argtypes = [_D, _D, _D, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        for name in ("mifi_bad2nanf", "mifi_nanf2bad"):
            getattr(L, name).argtypes = [_F, _F, ctypes.c_float]
            getattr(L, name).restype = _Z
        # include/fimex/vertical_coordinate_transformations.h
        L.mifi_atmosphere_sigma_pressure.argtypes = [_Z, ctypes.c_double, ctypes.c_double, _D, _D]
        L.mifi_atmosphere_hybrid_sigma_pressure.argtypes = [_Z, ctypes.c_double, ctypes.c_double, _D, _D, _D]
        L.mifi_atmosphere_hybrid_sigma_ap_pressure.argtypes = [_Z, ctypes.c_double, _D, _D, _D]
        L.mifi_barometric_standard_pressure.argtypes = [_Z, _D, _D]
        L.mifi_barometric_standard_altitude.argtypes = [_Z, _D, _D]
        for name in ("mifi_ocean_s_g1_z", "mifi_ocean_s_g2_z"):
            getattr(L, name).argtypes = [_Z, ctypes.c_double, ctypes.c_double, ctypes.c_double, _D, _D, _D]
        L.mifi_virtual_temperature.argtypes = [ctypes.c_float, ctypes.c_float]
        L.mifi_virtual_temperature.restype = ctypes.c_float
        L.mifi_barometric_layer_thickness.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
        L.mifi_barometric_layer_thickness.restype = ctypes.c_float

    # ---- regrid
    def interpolate_values(self, method, px, py, infield, inX, inY, skip=None):
        """mifi_get_values{,_bilinear,_bicubic}_f at every point with skip == 0 -> ([nz][n], return code); cells of skipped
        points stay NaN."""
        a = _c32(infield).ravel()
        nz = a.size // (inX * inY)
        px, py = _c64(px).ravel(), _c64(py).ravel()
        assert px.size == py.size and a.size == nz * inX * inY
        out = np.full((nz, px.size), np.nan, np.float32)
        sk = np.zeros(px.size, np.uint8) if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).ravel()
        assert sk.size == px.size
        rc = self.lib.ref_shim_get_values_batch(method, _f(a), _f(out.reshape(-1)), _d(px), _d(py),
                                                sk.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), px.size, inX, inY, nz)
        return out, rc

    def get_values(self, method, infield, x, y, ix, iy, iz=1):
        name = ("mifi_get_values_f", "mifi_get_values_bilinear_f", "mifi_get_values_bicubic_f")[method]
        a = _c32(infield).ravel()
        assert a.size == ix * iy * iz
        out = np.empty(iz, np.float32)
        rc = getattr(self.lib, name)(_f(a), _f(out), float(x), float(y), ix, iy, iz)
        return out, rc

    # ---- rotation
    def vector_reproject_values(self, matrix, u, v, ox, oy):
        m = _c64(matrix).ravel()
        u, v = _c32(u).copy().ravel(), _c32(v).copy().ravel()
        oz = u.size // (ox * oy)
        rc = self.lib.mifi_vector_reproject_values_by_matrix_f(MIFI_VECTOR_KEEP_SIZE, _d(m), _f(u), _f(v), ox, oy, oz)
        return u.reshape(oz, oy, ox), v.reshape(oz, oy, ox), rc

    def vector_reproject_direction(self, matrix, angles, ox, oy):
        m = _c64(matrix).ravel()
        a = _c32(angles).copy().ravel()
        oz = a.size // (ox * oy)
        rc = self.lib.mifi_vector_reproject_direction_by_matrix_f(MIFI_VECTOR_KEEP_SIZE, _d(m), _f(a), ox, oy, oz)
        return a.reshape(oz, oy, ox), rc

    # ---- the five PROJ.4 calls go to this hook
    def set_transform(self, fn):
        """fn(src, dst, x, y) -> (x', y') on float64 arrays (oracle.proj_oracle.transform); None removes the hook."""
        if fn is None:
            self._hook = _TRANSFORM(0)
        else:
            def cb(src, dst, n, x, y):
                try:
                    xs, ys = np.ctypeslib.as_array(x, (n,)), np.ctypeslib.as_array(y, (n,))
                    nx, ny = fn(src.decode(), dst.decode(), xs.copy(), ys.copy())
                    xs[:], ys[:] = nx, ny
                    return 0
                except Exception:  # an exception cannot cross the C frames
                    return -1
            self._hook = _TRANSFORM(cb)
        self.lib.ref_shim_set_transform(self._hook)

    def get_vector_reproject_matrix(self, proj_in, proj_out, out_x_axis, out_y_axis, x_type, y_type):
        xa, ya = _c64(out_x_axis), _c64(out_y_axis)
        m = np.full(4 * xa.size * ya.size, np.nan)
        rc = self.lib.mifi_get_vector_reproject_matrix(proj_in.encode(), proj_out.encode(), _d(xa), _d(ya), x_type, y_type,
                                                       xa.size, ya.size, _d(m))
        return m, rc

    def get_vector_reproject_matrix_field(self, proj_in, proj_out, in_x_field, in_y_field, ox, oy):
        xf, yf = _c64(in_x_field).ravel(), _c64(in_y_field).ravel()
        assert xf.size == ox * oy and yf.size == ox * oy
        m = np.full(4 * ox * oy, np.nan)
        rc = self.lib.mifi_get_vector_reproject_matrix_field(proj_in.encode(), proj_out.encode(), _d(xf), _d(yf), ox, oy, _d(m))
        return m, rc

    def get_vector_reproject_matrix_points(self, proj_in, proj_out, input_is_metric, out_x, out_y):
        xs, ys = _c64(out_x).ravel(), _c64(out_y).ravel()
        m = np.full(4 * xs.size, np.nan)
        rc = self.lib.mifi_get_vector_reproject_matrix_points(proj_in.encode(), proj_out.encode(), int(input_is_metric), _d(xs), _d(ys),
                                                              xs.size, _d(m))
        return m, rc

    def project_values(self, proj_in, proj_out, x, y):
        xs, ys = _c64(x).copy().ravel(), _c64(y).copy().ravel()
        rc = self.lib.mifi_project_values(proj_in.encode(), proj_out.encode(), _d(xs), _d(ys), xs.size)
        return xs, ys, rc

    def project_axes(self, proj_in, proj_out, x_axis, y_axis):
        xa, ya = _c64(x_axis), _c64(y_axis)
        ox, oy = np.full(xa.size * ya.size, np.nan), np.full(xa.size * ya.size, np.nan)
        rc = self.lib.mifi_project_axes(proj_in.encode(), proj_out.encode(), _d(xa), _d(ya), xa.size, ya.size, _d(ox), _d(oy))
        return ox, oy, rc

    # ---- axis positions, fills, blends, fill values
    def points2position(self, points, axis, axis_type):
        p = _c64(points).copy().ravel()
        ax = _c64(axis).ravel()
        rc = self.lib.mifi_points2position(_d(p), p.size, _d(ax), ax.size, axis_type)
        return p.reshape(np.shape(points)), rc

    def _fill(self, name, field, *args):
        a = _c32(field).copy()
        ny, nx = a.shape
        n = _Z(0)
        rc = getattr(self.lib, name)(nx, ny, _f(a), *args, ctypes.byref(n))
        return a, n.value, rc

    def fill2d(self, field, relaxCrit, corrEff, maxLoop):
        return self._fill("mifi_fill2d_f", field, relaxCrit, corrEff, maxLoop)

    def creepfill2d(self, field, repeat, setWeight):
        return self._fill("mifi_creepfill2d_f", field, repeat, bytes([setWeight & 0xFF]))

    def creepfillval2d(self, field, defaultVal, repeat, setWeight):
        return self._fill("mifi_creepfillval2d_f", field, defaultVal, repeat, bytes([setWeight & 0xFF]))

    def get_values_1d(self, kind, fieldA, fieldB, a, b, x):
        A, B = _c32(fieldA), _c32(fieldB)
        out = np.full(A.shape, -12345.0, np.float32)
        rc = getattr(self.lib, BLENDS[kind])(_f(A.reshape(-1)), _f(B.reshape(-1)), _f(out.reshape(-1)), A.size, a, b, x)
        return out, rc

    def get_values_linear_d(self, fieldA, fieldB, a, b, x):
        A, B = _c64(fieldA), _c64(fieldB)
        out = np.full(A.shape, -12345.0)
        rc = self.lib.mifi_get_values_linear_d(_d(A.reshape(-1)), _d(B.reshape(-1)), _d(out.reshape(-1)), A.size, a, b, x)
        return out, rc

    def _bad(self, name, a, bad):
        a = _c32(a).copy()
        flat = a.reshape(-1)
        ret = getattr(self.lib, name)(_f(flat), ctypes.cast(flat.ctypes.data + flat.nbytes, _F), bad)
        return a, ret

    def bad2nan(self, a, bad):
        return self._bad("mifi_bad2nanf", a, bad)

    def nan2bad(self, a, bad):
        return self._bad("mifi_nanf2bad", a, bad)

    # ---- vertical_coordinate_transformations.c
    def level_pressure(self, name, *args):
        """One of the (n, scalars..., arrays..., out) functions: scalars and float64 arrays in header order -> (out, rc)."""
        arrays = [_c64(a).ravel() for a in args if np.ndim(a) == 1]
        scalars = [float(a) for a in args if np.ndim(a) == 0]
        n = arrays[0].size
        assert all(a.size == n for a in arrays)
        out = np.full(n, np.nan)
        rc = getattr(self.lib, name)(n, *scalars, *[_d(a) for a in arrays], _d(out))
        return out, rc
