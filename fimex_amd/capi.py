"""ctypes binding of the C ABI in include/fimex_amd.h (libfimex_amd.so).

Harness glue for tests/ and bench.py: numpy arrays in and out for the *_host entry points,
raw device pointers (e.g. torch tensors' data_ptr()) for the *_device ones.  No compute
happens here and there is no fallback: a missing library or a missing GPU raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfimex_amd.so")
# the same sources built with -DFIMEX_AMD_TUNING: the only build that reads the FIMEX_AMD_<NAME> experiment switches
TUNING_LIB_PATH = os.path.join(_HERE, "libfimex_amd_tuning.so")

OK, ERROR = 1, -1

# include/fimex_amd.h (values of mifi_interpol_method)
NEAREST_NEIGHBOR, BILINEAR, BICUBIC, COORD_NN, COORD_NN_KD = 0, 1, 2, 3, 4
FORWARD_SUM, FORWARD_MEAN, FORWARD_MEDIAN, FORWARD_MAX, FORWARD_MIN = 5, 6, 7, 8, 9
FORWARD_UNDEF_SUM, FORWARD_UNDEF_MEAN, FORWARD_UNDEF_MEDIAN, FORWARD_UNDEF_MAX, FORWARD_UNDEF_MIN = 10, 11, 12, 13, 14
PROJ_AXIS, LONGITUDE, LATITUDE = 0, 1, 2
BICUBIC_REFERENCE, BICUBIC_FAST = 0, 1


class FimexAmdError(RuntimeError):
    """FIMEX_AMD_ERROR from the library; the message is fimex_amd_last_error()."""


class PlanInfo(ctypes.Structure):
    _fields_ = [("funcType", ctypes.c_int), ("device", ctypes.c_int),
                ("inX", ctypes.c_size_t), ("inY", ctypes.c_size_t), ("outX", ctypes.c_size_t), ("outY", ctypes.c_size_t),
                ("planBytes", ctypes.c_size_t), ("undefinedCells", ctypes.c_size_t), ("borderCells", ctypes.c_size_t),
                ("maxBucket", ctypes.c_size_t), ("mappedSourceCells", ctypes.c_size_t),
                ("stagedCells", ctypes.c_size_t), ("tileW", ctypes.c_size_t), ("tileH", ctypes.c_size_t),
                ("launchOrder", ctypes.c_size_t)]


BATCH_MAX_POSITIONS = 16


class BatchInfo(ctypes.Structure):
    _fields_ = [("d_data", ctypes.c_void_p), ("bytes", ctypes.c_size_t), ("bytesProbed", ctypes.c_size_t), ("bytesHeld", ctypes.c_size_t),
                ("stepBytes", ctypes.c_size_t), ("positions", ctypes.c_int), ("chosen", ctypes.c_int), ("trimmed", ctypes.c_int),
                ("msAtPosition", ctypes.c_float * BATCH_MAX_POSITIONS), ("probeSeconds", ctypes.c_double)]


class Process2d(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("relaxCrit", ctypes.c_float), ("corrEff", ctypes.c_float),
                ("maxLoop", ctypes.c_size_t), ("repeat", ctypes.c_ushort), ("setWeight", ctypes.c_char),
                ("defaultVal", ctypes.c_float)]


PROCESS_FILL2D, PROCESS_CREEPFILL2D, PROCESS_CREEPFILLVAL2D = 1, 2, 3

# mifi_vertical_interpol_method (include/fimex/mifi_constants.h) and the level kinds of fimex_amd_vertical_levels
VINT_METHOD_LIN, VINT_METHOD_LOG, VINT_METHOD_LOGLOG, VINT_METHOD_NN = 0, 1, 2, 3
VINT_METHOD_LIN_WEAK_EXTRA, VINT_METHOD_LIN_NO_EXTRA, VINT_METHOD_LIN_CONST_EXTRA = 4, 5, 6
VLEVEL_FIELD, VLEVEL_AXIS, VLEVEL_SIGMA, VLEVEL_HYBRID_SIGMA, VLEVEL_HYBRID_SIGMA_AP = 0, 1, 2, 3, 4
# surfaceFirst of fimex_amd_vertical_altitude_integrate_*
VORDER_AUTO, VORDER_SURFACE_LAST, VORDER_SURFACE_FIRST = -1, 0, 1


class VerticalLevelsStruct(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("nz", ctypes.c_size_t),
                ("axis", ctypes.c_void_p), ("sigma", ctypes.c_void_p), ("a", ctypes.c_void_p), ("ap", ctypes.c_void_p),
                ("b", ctypes.c_void_p), ("p0", ctypes.c_double), ("ptop", ctypes.c_double),
                ("ps", ctypes.c_void_p), ("field", ctypes.c_void_p)]


EXTRACT_MAX_DIMS = 8


class ExtractDim(ctypes.Structure):
    _fields_ = [("length", ctypes.c_size_t), ("reduced", ctypes.c_int), ("positions", ctypes.POINTER(ctypes.c_size_t)),
                ("nPositions", ctypes.c_size_t), ("start", ctypes.c_size_t), ("size", ctypes.c_size_t)]


class ExtractInfo(ctypes.Structure):
    _fields_ = [("inElements", ctypes.c_size_t), ("outElements", ctypes.c_size_t), ("kernelDims", ctypes.c_size_t),
                ("fastestRuns", ctypes.c_size_t), ("referenceOrderDiffers", ctypes.c_int)]


class Packing(ctypes.Structure):
    """fimex_amd_packing: how a variable is stored -- its CDM_* type code, _FillValue, scale_factor and add_offset."""
    _fields_ = [("type", ctypes.c_int), ("fill", ctypes.c_double), ("scale", ctypes.c_double), ("offset", ctypes.c_double)]

    def __init__(self, type, fill, scale=1.0, offset=0.0):
        super().__init__(int(type), float(fill), float(scale), float(offset))


class VerticalInfo(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_size_t), ("ny", ctypes.c_size_t), ("nt", ctypes.c_size_t), ("nzi", ctypes.c_size_t), ("nzo", ctypes.c_size_t),
                ("method", ctypes.c_int), ("entryBytes", ctypes.c_size_t)]


_F = ctypes.POINTER(ctypes.c_float)
_D = ctypes.POINTER(ctypes.c_double)
_Z = ctypes.c_size_t
_ZP = ctypes.POINTER(ctypes.c_size_t)
_V = ctypes.c_void_p
_PK = ctypes.POINTER(Packing)

# name -> (restype, argtypes); every symbol include/fimex_amd.h declares
SYMBOLS = {
    "fimex_amd_last_error": (ctypes.c_char_p, []),
    "fimex_amd_abi_version": (ctypes.c_int, []),
    "fimex_amd_device_count": (ctypes.c_int, []),
    "fimex_amd_set_device": (ctypes.c_int, [ctypes.c_int]),
    "fimex_amd_release_caches": (ctypes.c_int, []),
    "fimex_amd_regrid_plan_create": (ctypes.c_int, [ctypes.c_int, _D, _D, _Z, _Z, _Z, _Z, _Z, ctypes.POINTER(_V)]),
    "fimex_amd_regrid_plan_create_device": (ctypes.c_int, [ctypes.c_int, _V, _V, _Z, _Z, _Z, _Z, _Z, _V, ctypes.POINTER(_V)]),
    "fimex_amd_regrid_plan_create_opt": (ctypes.c_int, [ctypes.c_int, _D, _D, _Z, _Z, _Z, _Z, _Z, ctypes.c_int, ctypes.POINTER(_V)]),
    "fimex_amd_regrid_plan_create_device_opt": (ctypes.c_int, [ctypes.c_int, _V, _V, _Z, _Z, _Z, _Z, _Z, ctypes.c_int, _V, ctypes.POINTER(_V)]),
    "fimex_amd_regrid_plan_destroy": (ctypes.c_int, [_V]),
    "fimex_amd_regrid_plan_info": (ctypes.c_int, [_V, ctypes.POINTER(PlanInfo)]),
    "fimex_amd_regrid_apply_host": (ctypes.c_int, [_V, _F, _Z, _F, _Z, _ZP]),
    "fimex_amd_regrid_apply_device": (ctypes.c_int, [_V, _V, _Z, _V, _V]),
    "fimex_amd_regrid_plan_tune_device": (ctypes.c_int, [_V, _V, _Z, _V, _V, ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_regrid_plan_launch_order": (ctypes.c_int, [_V, _Z, ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_regrid_apply_gather_device": (ctypes.c_int, [_V, _V, _Z, _V, _V]),
    "fimex_amd_regrid_batch_alloc_device": (ctypes.c_int, [_V, _V, _Z, ctypes.c_int, _V, ctypes.POINTER(_V)]),
    "fimex_amd_regrid_source_batch_alloc_device": (ctypes.c_int, [_V, _Z, ctypes.c_int, _V, ctypes.POINTER(_V)]),
    "fimex_amd_batch_get_info": (ctypes.c_int, [_V, ctypes.POINTER(BatchInfo)]),
    "fimex_amd_batch_free": (ctypes.c_int, [_V]),
    "fimex_amd_regrid_slice_host": (ctypes.c_int, [_V, _F, _Z, ctypes.c_float, ctypes.POINTER(Process2d), _Z, _F, ctypes.c_float,
                                                   _V, ctypes.c_int, ctypes.POINTER(Process2d), _Z, _F, _Z, _ZP]),
    "fimex_amd_vector_plan_create": (ctypes.c_int, [_D, _Z, _Z, ctypes.POINTER(_V)]),
    "fimex_amd_vector_plan_destroy": (ctypes.c_int, [_V]),
    "fimex_amd_vector_reproject_values_host": (ctypes.c_int, [_V, _F, _F, _Z]),
    "fimex_amd_vector_reproject_values_device": (ctypes.c_int, [_V, _V, _V, _Z, _V]),
    "fimex_amd_regrid_apply_vector_device": (ctypes.c_int, [_V, _V, _V, _V, _Z, _V, _V, _V, ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_vector_reproject_direction_host": (ctypes.c_int, [_V, _F, _Z]),
    "fimex_amd_vector_reproject_direction_device": (ctypes.c_int, [_V, _V, _Z, _V]),
    "fimex_amd_fill2d_host": (ctypes.c_int, [_Z, _Z, _Z, _F, ctypes.c_float, ctypes.c_float, _Z, _ZP]),
    "fimex_amd_fill2d_device": (ctypes.c_int, [_Z, _Z, _Z, _V, ctypes.c_float, ctypes.c_float, _Z, _ZP, _V]),
    "fimex_amd_creepfill2d_host": (ctypes.c_int, [_Z, _Z, _Z, _F, ctypes.c_ushort, ctypes.c_char, _ZP]),
    "fimex_amd_creepfill2d_device": (ctypes.c_int, [_Z, _Z, _Z, _V, ctypes.c_ushort, ctypes.c_char, _ZP, _V]),
    "fimex_amd_creepfillval2d_host": (ctypes.c_int, [_Z, _Z, _Z, _F, ctypes.c_float, ctypes.c_ushort, ctypes.c_char, _ZP]),
    "fimex_amd_creepfillval2d_device": (ctypes.c_int, [_Z, _Z, _Z, _V, ctypes.c_float, ctypes.c_ushort, ctypes.c_char, _ZP, _V]),
    "fimex_amd_bad2nan_device": (ctypes.c_int, [_V, _Z, ctypes.c_float, _V]),
    "fimex_amd_nan2bad_device": (ctypes.c_int, [_V, _Z, ctypes.c_float, _V]),
    "fimex_amd_points2position_device": (ctypes.c_int, [_V, _Z, _D, ctypes.c_int, ctypes.c_int, _V]),
    "fimex_amd_points2position_host": (ctypes.c_int, [_D, _Z, _D, ctypes.c_int, ctypes.c_int]),
    "fimex_amd_data2interpolation_device": (ctypes.c_int, [_V, ctypes.c_int, _Z, ctypes.c_double, _V, _V]),
    "fimex_amd_interpolation2data_device": (ctypes.c_int, [_V, _Z, ctypes.c_int, ctypes.c_double, _V, _V]),
    "fimex_amd_regrid_apply_typed_device": (ctypes.c_int, [_V, _V, ctypes.c_int, _Z, ctypes.c_double, _V, _V]),
    "fimex_amd_regrid_apply_multi_device": (ctypes.c_int, [_V, _Z, ctypes.POINTER(_V), _ZP, ctypes.POINTER(_V), _V, ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_regrid_apply_multi_typed_device": (ctypes.c_int, [_V, _Z, ctypes.POINTER(_V), ctypes.c_int, _ZP, _D, ctypes.POINTER(_V), _V,
                                                                 ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_regrid_apply_vector_typed_device": (ctypes.c_int, [_V, _V, _V, ctypes.c_int, ctypes.c_double, _V, ctypes.c_int, ctypes.c_double, _Z,
                                                                  _V, _V, _V, ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_data2interpolation_host": (ctypes.c_int, [_V, ctypes.c_int, _Z, ctypes.c_double, _F]),
    "fimex_amd_interpolation2data_host": (ctypes.c_int, [_F, _Z, ctypes.c_int, ctypes.c_double, _V]),
    "fimex_amd_regrid_slice_typed_host": (ctypes.c_int, [_V, _V, ctypes.c_int, _Z, ctypes.c_double, ctypes.POINTER(Process2d), _Z,
                                                         _V, ctypes.c_int, ctypes.c_double, _V, ctypes.c_int,
                                                         ctypes.POINTER(Process2d), _Z, _V, _Z, _ZP]),
    "fimex_amd_get_values_1d_f_device": (ctypes.c_int, [ctypes.c_int, _V, _V, _V, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double, _V]),
    "fimex_amd_get_values_1d_f_host": (ctypes.c_int, [ctypes.c_int, _F, _F, _F, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "fimex_amd_get_values_linear_d_device": (ctypes.c_int, [_V, _V, _V, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double, _V]),
    "fimex_amd_vertical_interpolate_device": (ctypes.c_int, [ctypes.c_int, _Z, _Z, _Z, _V, ctypes.POINTER(VerticalLevelsStruct),
                                                             ctypes.POINTER(VerticalLevelsStruct), _D, _Z, _V, _V, ctypes.c_float, ctypes.c_float,
                                                             _V, _V]),
    "fimex_amd_vertical_interpolate_host": (ctypes.c_int, [ctypes.c_int, _Z, _Z, _Z, _F, ctypes.POINTER(VerticalLevelsStruct),
                                                           ctypes.POINTER(VerticalLevelsStruct), _D, _Z, _D, _D, ctypes.c_float, ctypes.c_float, _F]),
    "fimex_amd_vertical_plan_create_device": (ctypes.c_int, [ctypes.c_int, _Z, _Z, _Z, ctypes.POINTER(VerticalLevelsStruct),
                                                             ctypes.POINTER(VerticalLevelsStruct), _D, _Z, _V, _V, _V, ctypes.POINTER(_V)]),
    "fimex_amd_vertical_plan_destroy": (ctypes.c_int, [_V]),
    "fimex_amd_vertical_plan_info": (ctypes.c_int, [_V, ctypes.POINTER(VerticalInfo)]),
    "fimex_amd_vertical_plan_apply_device": (ctypes.c_int, [_V, _Z, ctypes.POINTER(_V), ctypes.c_int, _D, _F, _F, ctypes.POINTER(_V), _V]),
    "fimex_amd_vertical_levels_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, _V]),
    "fimex_amd_vertical_levels_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _F]),
    "fimex_amd_vertical_altitude_integrate_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, _V, _V, _V, ctypes.c_int,
                                                                    _V, ctypes.c_double, _V, _V]),
    "fimex_amd_vertical_altitude_integrate_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _F, _F, _F, _F, ctypes.c_int,
                                                                  _D, ctypes.c_double, _F]),
    "fimex_amd_vertical_standard_altitude_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, ctypes.c_double, _V, _V]),
    "fimex_amd_vertical_standard_altitude_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _D, ctypes.c_double, _F]),
    "fimex_amd_vertical_standard_pressure_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, ctypes.c_double, _V, _V]),
    "fimex_amd_vertical_standard_pressure_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _D, ctypes.c_double, _F]),
    "fimex_amd_vertical_ocean_depth_device": (ctypes.c_int, [ctypes.c_int, _Z, _Z, _Z, _Z, _D, _D, ctypes.c_double, _V, _V, _V, _V]),
    "fimex_amd_vertical_ocean_depth_host": (ctypes.c_int, [ctypes.c_int, _Z, _Z, _Z, _Z, _D, _D, ctypes.c_double, _D, _D, _F]),
    "fimex_amd_griddistance_device": (ctypes.c_int, [_Z, _Z, _V, _V, _V, _V, _V]),
    "fimex_amd_griddistance_host": (ctypes.c_int, [_Z, _Z, _D, _D, _F, _F]),
    "fimex_amd_vertical_velocity_device": (ctypes.c_int, [_Z, _Z, _Z, _Z, ctypes.c_double, ctypes.c_double, _V, _V, _D, _D, _V, _V, _V, _V, _V,
                                                          _V, _V]),
    "fimex_amd_vertical_velocity_host": (ctypes.c_int, [_Z, _Z, _Z, _Z, ctypes.c_double, ctypes.c_double, _F, _F, _D, _D, _F, _F, _F, _F, _F, _F]),
    "fimex_amd_omega_to_vertical_wind_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, _V, _V, _V]),
    "fimex_amd_omega_to_vertical_wind_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _F, _F, _F]),
    "fimex_amd_convert_scaled_device": (ctypes.c_int, [_V, ctypes.c_int, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                       ctypes.c_double, ctypes.c_double, ctypes.c_double, _V, _V]),
    "fimex_amd_theta_to_temperature_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, ctypes.c_float, _V, _V]),
    "fimex_amd_specific_to_relative_humidity_device": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _V, _V, _V, _V]),
    "fimex_amd_accumulate_device": (ctypes.c_int, [_V, ctypes.c_int, _Z, _Z, _Z, _V, _V, _V]),
    "fimex_amd_deaccumulate_device": (ctypes.c_int, [_V, ctypes.c_int, _Z, _Z, _Z, _V, _V, _V]),
    "fimex_amd_time_mapping": (ctypes.c_int, [_D, _Z, _D, _Z, _ZP, _ZP]),
    "fimex_amd_time_interpolate_device": (ctypes.c_int, [_V, ctypes.c_int, _Z, _D, _Z, _D, _Z, _V, _V]),
    "fimex_amd_quality_mask_device": (ctypes.c_int, [_V, ctypes.c_int, _Z, _V, ctypes.c_int, _Z, ctypes.c_int, _D, _Z, ctypes.c_double,
                                                     ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _V]),
    "fimex_amd_extract_describe": (ctypes.c_int, [ctypes.POINTER(ExtractDim), _Z, ctypes.POINTER(ExtractInfo)]),
    "fimex_amd_extract_plan_create": (ctypes.c_int, [ctypes.POINTER(ExtractDim), _Z, ctypes.POINTER(_V)]),
    "fimex_amd_extract_plan_destroy": (ctypes.c_int, [_V]),
    "fimex_amd_extract_plan_info": (ctypes.c_int, [_V, ctypes.POINTER(ExtractInfo)]),
    "fimex_amd_extract_apply_device": (ctypes.c_int, [_V, _V, ctypes.c_int, _V, _V]),
    "fimex_amd_extract_axis_range": (ctypes.c_int, [_D, _Z, ctypes.c_double, ctypes.c_double, _ZP, _ZP]),
    "fimex_amd_border_smooth_device": (ctypes.c_int, [_V, _V, _V, _Z, _Z, _Z, _Z, _Z, ctypes.c_int, _V]),
    "fimex_amd_border_smooth_host": (ctypes.c_int, [_F, _F, _F, _Z, _Z, _Z, _Z, _Z, ctypes.c_int]),
    "fimex_amd_overlay_device": (ctypes.c_int, [_V, _V, _V, _Z, _V]),
    "fimex_amd_overlay_host": (ctypes.c_int, [_F, _F, _F, _Z]),
    "fimex_amd_merge_plan_create": (ctypes.c_int, [_V, _V, _V, _Z, _Z, ctypes.c_int, ctypes.POINTER(_V)]),
    "fimex_amd_merge_plan_destroy": (ctypes.c_int, [_V]),
    "fimex_amd_merge_apply_device": (ctypes.c_int, [_V, _V, _V, _Z, _V, _V]),
    "fimex_amd_merge_apply_host": (ctypes.c_int, [_V, _F, _F, _Z, _F]),
    "fimex_amd_merge_apply_chain_device": (ctypes.c_int, [_V, _V, _V, _Z, _V, _V]),
    "fimex_amd_border_smooth_typed_device": (ctypes.c_int, [_V, _PK, _V, _PK, _V, _Z, _Z, _Z, _Z, _Z, ctypes.c_int, _V]),
    "fimex_amd_overlay_typed_device": (ctypes.c_int, [_V, _PK, _V, _PK, _V, _Z, _V]),
    "fimex_amd_merge_apply_typed_device": (ctypes.c_int, [_V, _V, _PK, _V, _PK, _Z, _V, _V, ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_merge_apply_typed_chain_device": (ctypes.c_int, [_V, _V, _PK, _V, _PK, _Z, _V, _V]),
    "fimex_amd_merge_apply_vector_device": (ctypes.c_int, [_V, _V, _V, _V, _V, _V, _V, _V, _Z, _V, _V, _V]),
    "fimex_amd_merge_apply_vector_chain_device": (ctypes.c_int, [_V, _V, _V, _V, _V, _V, _V, _V, _Z, _V, _V, _V]),
    "fimex_amd_merge_apply_vector_typed_device": (ctypes.c_int, [_V, _V, _V, _V, _V, _PK, _V, _PK, _V, _PK, _V, _PK, _Z, _V, _V, _V,
                                                                 ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_merge_apply_vector_typed_chain_device": (ctypes.c_int, [_V, _V, _V, _V, _V, _PK, _V, _PK, _V, _PK, _V, _PK, _Z, _V, _V, _V]),
    "fimex_amd_project_values_host": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _D, _Z]),
    "fimex_amd_project_values_device": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _V, _V, _Z, _V]),
    "fimex_amd_project_axes_host": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _D, _Z, _Z, _D, _D]),
    "fimex_amd_project_axes_device": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _D, _Z, _Z, _V, _V, _V]),
    "fimex_amd_get_vector_reproject_matrix_host": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _D, ctypes.c_int, ctypes.c_int, _Z, _Z, _D]),
    "fimex_amd_get_vector_reproject_matrix_device": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _D, ctypes.c_int, ctypes.c_int, _Z, _Z, _V, _V]),
    "fimex_amd_get_vector_reproject_matrix_field_host": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _D, _Z, _Z, _D]),
    "fimex_amd_get_vector_reproject_matrix_points_host": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, _D, _D, _Z, _D]),
    "fimex_amd_vector_reproject_direction_scaled_host": (ctypes.c_int, [_V, _F, _Z, ctypes.c_double, ctypes.c_double]),
    "fimex_amd_vector_reproject_direction_scaled_device": (ctypes.c_int, [_V, _V, _Z, ctypes.c_double, ctypes.c_double, _V]),
    "fimex_amd_rotate_vector_typed_host": (ctypes.c_int, [_V, _V, ctypes.c_int, ctypes.c_double, _V, ctypes.c_int, ctypes.c_double, _Z, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_double, _V]),
    "fimex_amd_projection_is_degree": (ctypes.c_int, [ctypes.c_char_p]),
    "fimex_amd_coord_nearest_host": (ctypes.c_int, [_D, _D, _Z, _D, _D, _Z, _Z]),
    "fimex_amd_coord_nearest_device": (ctypes.c_int, [_V, _V, _Z, _V, _V, _Z, _Z, _V]),
    "fimex_amd_coord_kdtree_host": (ctypes.c_int, [ctypes.c_double, _D, _D, _Z, _D, _D, _Z, _Z]),
    "fimex_amd_coord_kdtree_device": (ctypes.c_int, [ctypes.c_double, _V, _V, _Z, _V, _V, _Z, _Z, _V]),
    "fimex_amd_grid_distance_host": (ctypes.c_int, [_D, _D, _Z, _Z, _D]),
    "fimex_amd_scan_sum_device": (ctypes.c_int, [_V, _Z, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_double), _ZP, _V]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_derived_host.h declares: the *_host forms of the (8f n9) entries
DERIVED_HOST_SYMBOLS = {
    "fimex_amd_convert_scaled_host": (ctypes.c_int, [_V, ctypes.c_int, _Z, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                     ctypes.c_double, ctypes.c_double, ctypes.c_double, _V]),
    "fimex_amd_theta_to_temperature_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _F, ctypes.c_float, _F]),
    "fimex_amd_specific_to_relative_humidity_host": (ctypes.c_int, [ctypes.POINTER(VerticalLevelsStruct), _Z, _Z, _Z, _F, _F, _V]),
    "fimex_amd_accumulate_host": (ctypes.c_int, [_V, ctypes.c_int, _Z, _Z, _Z, _D, _D]),
    "fimex_amd_deaccumulate_host": (ctypes.c_int, [_V, ctypes.c_int, _Z, _Z, _Z, _V, _D]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_time_quality_host.h declares: the *_host forms of the (8f n10) entries
TIME_QUALITY_HOST_SYMBOLS = {
    "fimex_amd_time_interpolate_host": (ctypes.c_int, [_V, ctypes.c_int, _Z, _D, _Z, _D, _Z, _F]),
    "fimex_amd_quality_mask_host": (ctypes.c_int, [_V, ctypes.c_int, _Z, _V, ctypes.c_int, _Z, ctypes.c_int, _D, _Z, ctypes.c_double,
                                                   ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_extract_host.h declares: the entries of (8f n11) on host buffers
EXTRACT_HOST_SYMBOLS = {
    "fimex_amd_extract_apply_host": (ctypes.c_int, [_V, _V, ctypes.c_int, _V]),
    "fimex_amd_extract_bounding_box_host": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _D, _Z, _D, _Z, ctypes.c_int, ctypes.c_double,
                                                           ctypes.c_double, ctypes.c_double, ctypes.c_double, _ZP, _ZP, _ZP, _ZP]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_vector_regrid_host.h declares: a vector pair regridded and rotated on host buffers
VECTOR_REGRID_HOST_SYMBOLS = {
    "fimex_amd_regrid_apply_vector_host": (ctypes.c_int, [_V, _V, _F, _F, _Z, _F, _F, _Z, _ZP]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_vector_regrid_typed_host.h declares: a vector pair in its stored types on host buffers
VECTOR_REGRID_TYPED_HOST_SYMBOLS = {
    "fimex_amd_regrid_apply_vector_typed_host": (ctypes.c_int, [_V, _V, _V, ctypes.c_int, ctypes.c_double, _V, ctypes.c_int, ctypes.c_double, _Z,
                                                                _V, _V, _Z, _ZP]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_merge_typed_host.h declares: grid merging on stored types, on host buffers
MERGE_TYPED_HOST_SYMBOLS = {
    "fimex_amd_border_smooth_typed_host": (ctypes.c_int, [_V, _PK, _V, _PK, _V, _Z, _Z, _Z, _Z, _Z, ctypes.c_int]),
    "fimex_amd_overlay_typed_host": (ctypes.c_int, [_V, _PK, _V, _PK, _V, _Z]),
    "fimex_amd_merge_apply_typed_host": (ctypes.c_int, [_V, _V, _PK, _V, _PK, _Z, _V]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_merge_vector_host.h declares: the merge of an x/y vector pair on host buffers
MERGE_VECTOR_HOST_SYMBOLS = {
    "fimex_amd_merge_apply_vector_host": (ctypes.c_int, [_V, _V, _V, _V, _F, _F, _F, _F, _Z, _F, _F]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_merge_vector_typed_host.h declares: the merge of an x/y vector pair in
# its stored types on host buffers
MERGE_VECTOR_TYPED_HOST_SYMBOLS = {
    "fimex_amd_merge_apply_vector_typed_host": (ctypes.c_int, [_V, _V, _V, _V, _V, _PK, _V, _PK, _V, _PK, _V, _PK, _Z, _V, _V]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_vertical_plan_host.h declares: the entries of (8f n5b) on host buffers
VERTICAL_PLAN_HOST_SYMBOLS = {
    "fimex_amd_vertical_plan_create_host": (ctypes.c_int, [ctypes.c_int, _Z, _Z, _Z, ctypes.POINTER(VerticalLevelsStruct),
                                                           ctypes.POINTER(VerticalLevelsStruct), _D, _Z, _D, _D, ctypes.POINTER(_V)]),
    "fimex_amd_vertical_plan_apply_host": (ctypes.c_int, [_V, _Z, ctypes.POINTER(_V), ctypes.c_int, _D, _F, _F, ctypes.POINTER(_V)]),
    "fimex_amd_vertical_plan_read_host": (ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), _F]),
}

# name -> (restype, argtypes); every symbol include/fimex_amd_regrid_multi_host.h declares: a list of variables regridded in one call, on host buffers
REGRID_MULTI_HOST_SYMBOLS = {
    "fimex_amd_regrid_apply_multi_host": (ctypes.c_int, [_V, _Z, ctypes.POINTER(_V), _ZP, ctypes.POINTER(_V), ctypes.POINTER(ctypes.c_int)]),
    "fimex_amd_regrid_apply_multi_typed_host": (ctypes.c_int, [_V, _Z, ctypes.POINTER(_V), ctypes.c_int, _ZP, _D, ctypes.POINTER(_V),
                                                               ctypes.POINTER(ctypes.c_int)]),
}
REGRID_MULTI_MAX_VARS = 64  # FIMEX_AMD_REGRID_MULTI_MAX_VARS

_lib = None
_libs = {}


def _open(path):
    if not os.path.exists(path):
        raise FimexAmdError("%s is missing: build it with `python -m fimex_amd.build` (needs hipcc); "
                            "there is no CPU fallback" % path)
    try:
        # share the HIP runtime torch has already mapped (same SONAME) when torch is in the process
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(path)
    for name, (res, args) in list(SYMBOLS.items()) + list(DERIVED_HOST_SYMBOLS.items()) + list(TIME_QUALITY_HOST_SYMBOLS.items()) + list(
            EXTRACT_HOST_SYMBOLS.items()) + list(VERTICAL_PLAN_HOST_SYMBOLS.items()) + list(VECTOR_REGRID_HOST_SYMBOLS.items()) + list(
            VECTOR_REGRID_TYPED_HOST_SYMBOLS.items()) + list(MERGE_TYPED_HOST_SYMBOLS.items()) + list(MERGE_VECTOR_HOST_SYMBOLS.items()) + list(
            MERGE_VECTOR_TYPED_HOST_SYMBOLS.items()) + list(REGRID_MULTI_HOST_SYMBOLS.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libfimex_amd.so; raises when it has not been built (python -m fimex_amd.build)."""
    global _lib
    if _lib is None:
        use_tuning_build(False)
    return _lib


def use_tuning_build(on=True):
    """Switch this module to libfimex_amd_tuning.so (scripts/ sweeps, tests that force a fallback kernel through a
    FIMEX_AMD_<NAME> switch) or back to the product library.  Plans belong to the library that made them: switch before
    creating them.  Returns the previous setting."""
    global _lib
    path = TUNING_LIB_PATH if on else LIB_PATH
    was = _lib is not None and _lib is _libs.get(TUNING_LIB_PATH)
    if path not in _libs:
        _libs[path] = _open(path)
    _lib = _libs[path]
    return was


def _check(rc):
    if rc != OK:
        raise FimexAmdError(load().fimex_amd_last_error().decode() or "fimex_amd call failed")


def release_caches():
    _check(load().fimex_amd_release_caches())


def device_count():
    return load().fimex_amd_device_count()


def set_device(ordinal):
    _check(load().fimex_amd_set_device(ordinal))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _fp(a):
    return a.ctypes.data_as(_F)


def _dp(a):
    return a.ctypes.data_as(_D)


class RegridPlan:
    """fimex_amd_regrid_plan: backward (per output cell) or forward (per input cell) positions."""

    def __init__(self, funcType, pointsOnXAxis, pointsOnYAxis, inX, inY, outX, outY, bicubic=None):
        px, py = _f64(pointsOnXAxis).ravel(), _f64(pointsOnYAxis).ravel()
        if px.size != py.size:
            raise ValueError("position arrays differ in size")
        self._h = _V()
        self.inX, self.inY, self.outX, self.outY = inX, inY, outX, outY
        if bicubic is None:
            _check(load().fimex_amd_regrid_plan_create(funcType, _dp(px), _dp(py), px.size, inX, inY, outX, outY,
                                                       ctypes.byref(self._h)))
        else:  # BICUBIC_REFERENCE / BICUBIC_FAST
            _check(load().fimex_amd_regrid_plan_create_opt(funcType, _dp(px), _dp(py), px.size, inX, inY, outX, outY, bicubic,
                                                           ctypes.byref(self._h)))

    @classmethod
    def from_device(cls, funcType, d_px, d_py, nPoints, inX, inY, outX, outY, stream=0, bicubic=None):
        self = cls.__new__(cls)
        self._h = _V()
        self.inX, self.inY, self.outX, self.outY = inX, inY, outX, outY
        if bicubic is None:
            _check(load().fimex_amd_regrid_plan_create_device(funcType, d_px, d_py, nPoints, inX, inY, outX, outY,
                                                              stream, ctypes.byref(self._h)))
        else:
            _check(load().fimex_amd_regrid_plan_create_device_opt(funcType, d_px, d_py, nPoints, inX, inY, outX, outY, bicubic,
                                                                  stream, ctypes.byref(self._h)))
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().fimex_amd_regrid_plan_destroy(self._h)
            self._h = _V()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may be gone already
            pass

    def info(self):
        i = PlanInfo()
        _check(load().fimex_amd_regrid_plan_info(self._h, ctypes.byref(i)))
        return {k: getattr(i, k) for k, _ in PlanInfo._fields_}

    def apply_host(self, inData):
        """interpolateValues: [nz][inY][inX] float32 host array -> [nz][outY][outX]."""
        a = _f32(inData).ravel()
        n = _Z(0)
        _check(load().fimex_amd_regrid_apply_host(self._h, _fp(a), a.size, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        _check(load().fimex_amd_regrid_apply_host(self._h, _fp(a), a.size, _fp(out), out.size, ctypes.byref(n)))
        return out.reshape(-1, self.outY, self.outX)

    def apply_device(self, d_in, nz, d_out, stream=0):
        _check(load().fimex_amd_regrid_apply_device(self._h, d_in, nz, d_out, stream))

    def apply_multi_device(self, d_in, nz, d_out, stream=0, cdmType=None, badValue=None):
        """A list of variables in one call: d_in / d_out sequences of device pointers, nz the slices of each.  cdmType None: float
        slices; else the variables' stored type, badValue one fill value for all or one per variable.  Only enqueues on `stream`.
        Returns the path: 1 the list kernels, 0 the per-variable calls."""
        n = len(nz)
        if len(d_in) != n or len(d_out) != n:
            raise ValueError("as many inputs and outputs as slice counts")
        ins, outs = (_V * max(n, 1))(*d_in), (_V * max(n, 1))(*d_out)
        nzs = (_Z * max(n, 1))(*nz)
        path = ctypes.c_int(-1)
        if cdmType is None:
            _check(load().fimex_amd_regrid_apply_multi_device(self._h, n, ins, nzs, outs, stream, ctypes.byref(path)))
        else:
            bad = np.ascontiguousarray(np.broadcast_to(np.asarray(float("nan") if badValue is None else badValue, dtype=np.float64), (n,)))
            _check(load().fimex_amd_regrid_apply_multi_typed_device(self._h, n, ins, cdmType, nzs, _dp(bad), outs, stream, ctypes.byref(path)))
        return path.value

    def apply_multi_host(self, arrays, badValue=None):
        """The same on host arrays [nz[i]][inY][inX] of one element type (float32, or a stored type with badValue as above); returns
        (the regridded arrays [nz[i]][outY][outX], path)."""
        arrs = [np.ascontiguousarray(a) for a in arrays]
        n = len(arrs)
        layer = self.inX * self.inY
        nz = [a.size // layer for a in arrs]
        dtype = arrs[0].dtype if n else np.dtype(np.float32)
        if any(a.dtype != dtype or a.size != z * layer for a, z in zip(arrs, nz)):
            raise ValueError("arrays of one element type, each a whole number of source slices")
        outs = [np.empty((z, self.outY, self.outX), dtype=dtype) for z in nz]
        ins_p, outs_p = (_V * max(n, 1))(*[a.ctypes.data for a in arrs]), (_V * max(n, 1))(*[o.ctypes.data for o in outs])
        nzs = (_Z * max(n, 1))(*nz)
        path = ctypes.c_int(-1)
        if dtype == np.float32 and badValue is None:
            _check(load().fimex_amd_regrid_apply_multi_host(self._h, n, ins_p, nzs, outs_p, ctypes.byref(path)))
        else:
            bad = np.ascontiguousarray(np.broadcast_to(np.asarray(float("nan") if badValue is None else badValue, dtype=np.float64), (n,)))
            _check(load().fimex_amd_regrid_apply_multi_typed_host(self._h, n, ins_p, cdm_type_of(dtype), nzs, _dp(bad), outs_p, ctypes.byref(path)))
        return outs, path.value

    def apply_vector_device(self, vec, d_u, d_v, nz, d_uOut, d_vOut, stream=0):
        """getDataSlice's vector branch on device buffers: both components regridded and rotated by `vec` (a VectorPlan on the
        output grid).  Returns the path: 1 the fused kernel, 0 regrid, regrid, rotate."""
        path = ctypes.c_int(-1)
        _check(load().fimex_amd_regrid_apply_vector_device(self._h, vec._h, d_u, d_v, nz, d_uOut, d_vOut, stream, ctypes.byref(path)))
        return path.value

    def apply_vector_host(self, vec, u, v):
        """The same on [nz][inY][inX] float32 host arrays; returns (uOut, vOut), each [nz][outY][outX]."""
        a, b = _f32(u).ravel(), _f32(v).ravel()
        if a.size != b.size:
            raise ValueError("the components differ in size")
        nz = a.size // (self.inX * self.inY) if self.inX * self.inY else 0
        uOut, vOut = (np.empty(nz * self.outX * self.outY, dtype=np.float32) for _ in range(2))
        n = _Z(0)
        _check(load().fimex_amd_regrid_apply_vector_host(self._h, vec._h, _fp(a), _fp(b), a.size, _fp(uOut), _fp(vOut), uOut.size, ctypes.byref(n)))
        return uOut.reshape(-1, self.outY, self.outX), vOut.reshape(-1, self.outY, self.outX)

    def apply_vector_typed_device(self, vec, d_u, uType, uBad, d_v, vType, vBad, nz, d_uOut, d_vOut, stream=0):
        """The same on a pair in its stored types (CDM_* codes; each component with its own type and fill value, results in the
        same types).  Returns the path: 2 one kernel on the stored type, 1 or 0 the chain around apply_vector_device."""
        path = ctypes.c_int(-1)
        _check(load().fimex_amd_regrid_apply_vector_typed_device(self._h, vec._h, d_u, uType, uBad, d_v, vType, vBad, nz, d_uOut, d_vOut, stream,
                                                                 ctypes.byref(path)))
        return path.value

    def apply_vector_typed_host(self, vec, u, uBad, v, vBad):
        """The same on [nz][inY][inX] host arrays of any numeric CDM type; returns (uOut, vOut), each [nz][outY][outX] in the dtype
        of its component."""
        a, b = np.ascontiguousarray(u).ravel(), np.ascontiguousarray(v).ravel()
        if a.size != b.size:
            raise ValueError("the components differ in size")
        nz = a.size // (self.inX * self.inY) if self.inX * self.inY else 0
        uOut, vOut = np.empty(nz * self.outX * self.outY, dtype=a.dtype), np.empty(nz * self.outX * self.outY, dtype=b.dtype)
        n = _Z(0)
        _check(load().fimex_amd_regrid_apply_vector_typed_host(self._h, vec._h, a.ctypes.data, cdm_type_of(a.dtype), uBad, b.ctypes.data,
                                                               cdm_type_of(b.dtype), vBad, a.size, uOut.ctypes.data, vOut.ctypes.data, uOut.size,
                                                               ctypes.byref(n)))
        return uOut.reshape(-1, self.outY, self.outX), vOut.reshape(-1, self.outY, self.outX)

    def apply_gather_device(self, d_in, nz, d_out, stream=0):
        """The same regrid through the per-lane gather kernels (cross-check of the staged kernels on whole batches)."""
        _check(load().fimex_amd_regrid_apply_gather_device(self._h, d_in, nz, d_out, stream))

    def alloc_source_batch(self, nz, candidates=4, stream=0):
        """Source batch [nz][inY][inX] placed by the library (fimex_amd_regrid_source_batch_alloc_device), zero-filled."""
        return Batch(self, 0, nz, candidates, stream, source=True)

    def alloc_batch(self, d_in, nz, positions=8, stream=0):
        """Output batch [nz][outY][outX] placed by the library (fimex_amd_regrid_batch_alloc_device)."""
        return Batch(self, d_in, nz, positions, stream)

    def tune_device(self, d_in, nz, d_out, stream=0):
        """Times the plan's workgroup shapes on these device buffers and keeps the faster (0: default shape, 1: the other)."""
        chosen = ctypes.c_int(0)
        _check(load().fimex_amd_regrid_plan_tune_device(self._h, d_in, nz, d_out, stream, ctypes.byref(chosen)))
        return chosen.value

    def launch_order(self, nz):
        """The launch order apply_device runs nz float slices in: 1 an XCD runs whole tiles, 2 an XCD runs one z chunk of every tile
        (info()["launchOrder"] == 1 and a batch long enough), 0 chunk-major (tuning build), -1 not the second staged form."""
        order = ctypes.c_int(-1)
        _check(load().fimex_amd_regrid_plan_launch_order(self._h, nz, ctypes.byref(order)))
        return order.value


class Batch:
    """fimex_amd_batch: device memory of one output batch, placed where the plan's apply launch runs fastest."""

    def __init__(self, plan, d_in, nz, positions=8, stream=0, source=False):
        self._h = _V()
        if source:  # the SOURCE batch [nz][inY][inX]: `positions` whole allocations tried (d_in is not used)
            _check(load().fimex_amd_regrid_source_batch_alloc_device(plan._h, nz, positions, stream, ctypes.byref(self._h)))
        else:
            _check(load().fimex_amd_regrid_batch_alloc_device(plan._h, d_in, nz, positions, stream, ctypes.byref(self._h)))
        i = BatchInfo()
        _check(load().fimex_amd_batch_get_info(self._h, ctypes.byref(i)))
        self.info = {k: getattr(i, k) for k, _ in BatchInfo._fields_ if k != "msAtPosition"}
        self.info["msAtPosition"] = [float(i.msAtPosition[k]) for k in range(i.positions)] if i.positions > 1 else []
        self.data_ptr = i.d_data
        self.nz, self.outY, self.outX = (nz, plan.inY, plan.inX) if source else (nz, plan.outY, plan.outX)

    def as_tensor(self):
        """The batch as a torch tensor [nz][outY][outX] (no copy; keep this object alive as long as the tensor)."""
        import torch

        class _Cai:  # __cuda_array_interface__ of library-owned device memory
            pass
        c = _Cai()
        c.__cuda_array_interface__ = {"shape": (self.nz, self.outY, self.outX), "typestr": "<f4", "data": (int(self.data_ptr), False),
                                      "version": 2, "strides": None}
        t = torch.as_tensor(c, device="cuda")
        t._fimex_amd_batch = self
        return t

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().fimex_amd_batch_free(self._h)
            self._h = _V()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VectorPlan:
    """fimex_amd_vector_plan from the reference's double[4*ox*oy] rotation matrix."""

    def __init__(self, matrix, ox, oy):
        m = _f64(matrix).ravel()
        if m.size != 4 * ox * oy:
            raise ValueError("matrix must hold 4*ox*oy doubles")
        self._h = _V()
        self.ox, self.oy = ox, oy
        _check(load().fimex_amd_vector_plan_create(_dp(m), ox, oy, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().fimex_amd_vector_plan_destroy(self._h)
            self._h = _V()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def reproject_values_host(self, u, v):
        u, v = _f32(u).copy(), _f32(v).copy()
        _check(load().fimex_amd_vector_reproject_values_host(self._h, _fp(u.reshape(-1)), _fp(v.reshape(-1)), u.size))
        return u, v

    def reproject_values_device(self, d_u, d_v, oz, stream=0):
        _check(load().fimex_amd_vector_reproject_values_device(self._h, d_u, d_v, oz, stream))

    def reproject_direction_host(self, angles):
        a = _f32(angles).copy()
        _check(load().fimex_amd_vector_reproject_direction_host(self._h, _fp(a.reshape(-1)), a.size))
        return a

    def reproject_direction_device(self, d_angles, oz, stream=0):
        _check(load().fimex_amd_vector_reproject_direction_device(self._h, d_angles, oz, stream))

    def reproject_direction_scaled_host(self, angles, scale, offset):
        """packed angles: scale * a + offset, rotate, (a - offset) / scale (src/CDMProcessor.cc:621-636)."""
        a = _f32(angles).copy()
        _check(load().fimex_amd_vector_reproject_direction_scaled_host(self._h, _fp(a.reshape(-1)), a.size, scale, offset))
        return a

    def reproject_direction_scaled_device(self, d_angles, oz, scale, offset, stream=0):
        _check(load().fimex_amd_vector_reproject_direction_scaled_device(self._h, d_angles, oz, scale, offset, stream))


def fill2d_process(relaxCrit, corrEff, maxLoop):
    return Process2d(PROCESS_FILL2D, relaxCrit, corrEff, maxLoop, 0, b"\0", 0.0)


def creepfill2d_process(repeat, setWeight):
    return Process2d(PROCESS_CREEPFILL2D, 0.0, 0.0, 0, repeat, bytes([setWeight & 0xFF]), 0.0)


def creepfillval2d_process(repeat, setWeight, defaultVal):
    return Process2d(PROCESS_CREEPFILLVAL2D, 0.0, 0.0, 0, repeat, bytes([setWeight & 0xFF]), defaultVal)


def regrid_slice_host(plan, inData, badValue=float("nan"), pre=(), post=(), counterpart=None,
                      badValueCounterpart=float("nan"), vec=None, isXComponent=True):
    """The whole CDMInterpolator::getDataSlice body on the GPU (fimex_amd_regrid_slice_host)."""
    a = _f32(inData).ravel()
    c = _f32(counterpart).ravel() if counterpart is not None else None
    pre_a = (Process2d * len(pre))(*pre) if pre else None
    post_a = (Process2d * len(post))(*post) if post else None
    n = _Z(0)
    args = (plan._h, _fp(a), a.size, badValue, pre_a, len(pre), _fp(c) if c is not None else None, badValueCounterpart,
            vec._h if vec is not None else None, 1 if isXComponent else 0, post_a, len(post))
    _check(load().fimex_amd_regrid_slice_host(*args, None, 0, ctypes.byref(n)))
    out = np.empty(n.value, dtype=np.float32)
    _check(load().fimex_amd_regrid_slice_host(*args, _fp(out), out.size, ctypes.byref(n)))
    return out.reshape(-1, plan.outY, plan.outX)


# CDMDataType codes (include/fimex/CDMDataType.h:35-49) and their numpy element types
CDM_CHAR, CDM_SHORT, CDM_INT, CDM_FLOAT, CDM_DOUBLE, CDM_UCHAR, CDM_USHORT, CDM_UINT, CDM_INT64, CDM_UINT64 = 1, 2, 3, 4, 5, 7, 8, 9, 10, 11
CDM_DTYPES = {CDM_CHAR: np.int8, CDM_SHORT: np.int16, CDM_INT: np.int32, CDM_FLOAT: np.float32, CDM_DOUBLE: np.float64,
              CDM_UCHAR: np.uint8, CDM_USHORT: np.uint16, CDM_UINT: np.uint32, CDM_INT64: np.int64, CDM_UINT64: np.uint64}


def cdm_type_of(dtype):
    for code, dt in CDM_DTYPES.items():
        if np.dtype(dt) == np.dtype(dtype):
            return code
    raise TypeError("no CDMDataType for %s" % dtype)


def regrid_apply_typed_device(plan, d_in, cdmType, nz, badValue, d_out, stream=0):
    _check(load().fimex_amd_regrid_apply_typed_device(plan._h, d_in, cdmType, nz, badValue, d_out, stream))


def data2interpolation_device(d_in, cdmType, n, badValue, d_out, stream=0):
    _check(load().fimex_amd_data2interpolation_device(d_in, cdmType, n, badValue, d_out, stream))


def interpolation2data_device(d_in, n, cdmType, badValue, d_out, stream=0):
    _check(load().fimex_amd_interpolation2data_device(d_in, n, cdmType, badValue, d_out, stream))


def regrid_slice_typed_host(plan, inData, badValue, pre=(), post=(), counterpart=None, badValueCounterpart=float("nan"),
                            vec=None, isXComponent=True):
    """fimex_amd_regrid_slice_typed_host: the slice in the variable's stored type in, the same type out."""
    a = np.ascontiguousarray(inData).ravel()
    t = cdm_type_of(a.dtype)
    c = np.ascontiguousarray(counterpart).ravel() if counterpart is not None else None
    pre_a = (Process2d * len(pre))(*pre) if pre else None
    post_a = (Process2d * len(post))(*post) if post else None
    n = _Z(0)
    args = (plan._h, a.ctypes.data, t, a.size, badValue, pre_a, len(pre), c.ctypes.data if c is not None else None,
            cdm_type_of(c.dtype) if c is not None else 0, badValueCounterpart, vec._h if vec is not None else None,
            1 if isXComponent else 0, post_a, len(post))
    _check(load().fimex_amd_regrid_slice_typed_host(*args, None, 0, ctypes.byref(n)))
    out = np.empty(n.value, dtype=a.dtype)
    _check(load().fimex_amd_regrid_slice_typed_host(*args, out.ctypes.data, out.size, ctypes.byref(n)))
    return out.reshape(-1, plan.outY, plan.outX)


def _slices(field):
    a = _f32(field).copy()
    if a.ndim == 2:
        a = a[None]
    nz, ny, nx = a.shape
    return a, nx, ny, nz


def fill2d_host(field, relaxCrit, corrEff, maxLoop):
    a, nx, ny, nz = _slices(field)
    n = (ctypes.c_size_t * nz)()
    _check(load().fimex_amd_fill2d_host(nx, ny, nz, _fp(a.reshape(-1)), relaxCrit, corrEff, maxLoop, n))
    return a.reshape(np.shape(field)), list(n)


def creepfill2d_host(field, repeat, setWeight):
    a, nx, ny, nz = _slices(field)
    n = (ctypes.c_size_t * nz)()
    _check(load().fimex_amd_creepfill2d_host(nx, ny, nz, _fp(a.reshape(-1)), repeat, bytes([setWeight & 0xFF]), n))
    return a.reshape(np.shape(field)), list(n)


def creepfillval2d_host(field, defaultVal, repeat, setWeight):
    a, nx, ny, nz = _slices(field)
    n = (ctypes.c_size_t * nz)()
    _check(load().fimex_amd_creepfillval2d_host(nx, ny, nz, _fp(a.reshape(-1)), defaultVal, repeat,
                                                bytes([setWeight & 0xFF]), n))
    return a.reshape(np.shape(field)), list(n)


def fill2d_device(d_field, nx, ny, nz, relaxCrit, corrEff, maxLoop, stream=0):
    n = (ctypes.c_size_t * nz)()
    _check(load().fimex_amd_fill2d_device(nx, ny, nz, d_field, relaxCrit, corrEff, maxLoop, n, stream))
    return list(n)


def creepfill2d_device(d_field, nx, ny, nz, repeat, setWeight, stream=0):
    n = (ctypes.c_size_t * nz)()
    _check(load().fimex_amd_creepfill2d_device(nx, ny, nz, d_field, repeat, bytes([setWeight & 0xFF]), n, stream))
    return list(n)


def bad2nan_device(d_data, n, bad, stream=0):
    _check(load().fimex_amd_bad2nan_device(d_data, n, bad, stream))


def nan2bad_device(d_data, n, bad, stream=0):
    _check(load().fimex_amd_nan2bad_device(d_data, n, bad, stream))


BLEND_NEAREST, BLEND_LINEAR, BLEND_LINEAR_WEAK_EXTRAPOL, BLEND_LINEAR_NO_EXTRAPOL, BLEND_LINEAR_CONST_EXTRAPOL, BLEND_LOG, BLEND_LOG_LOG = range(7)


def get_values_1d_host(kind, fieldA, fieldB, a, b, x):
    """mifi_get_values_*_f between two fields; raises where the reference returns MIFI_ERROR."""
    A, B = _f32(fieldA), _f32(fieldB)
    out = np.empty(A.shape, np.float32)
    _check(load().fimex_amd_get_values_1d_f_host(kind, _fp(A.reshape(-1)), _fp(B.reshape(-1)), _fp(out.reshape(-1)), A.size, a, b, x))
    return out


def get_values_1d_device(kind, d_A, d_B, d_out, n, a, b, x, stream=0):
    _check(load().fimex_amd_get_values_1d_f_device(kind, d_A, d_B, d_out, n, a, b, x, stream))


def get_values_linear_d_device(d_A, d_B, d_out, n, a, b, x, stream=0):
    _check(load().fimex_amd_get_values_linear_d_device(d_A, d_B, d_out, n, a, b, x, stream))


class VerticalLevels:
    """fimex_amd_vertical_levels.  The coefficient arrays (axis, sigma, a, ap, b) are host arrays of nz doubles; ps ([nt][ny][nx]) and
    field ([nt][nz][ny][nx]) are numpy float32 arrays for the *_host calls and device pointers (ints, e.g. tensor.data_ptr()) for
    the *_device calls.  This object keeps the numpy arrays alive."""

    def __init__(self, kind, nz, axis=None, sigma=None, a=None, ap=None, b=None, p0=0.0, ptop=0.0, ps=None, field=None):
        self._keep = []
        self.kind, self.nz = kind, nz
        s = VerticalLevelsStruct()
        s.kind, s.nz, s.p0, s.ptop = kind, nz, p0, ptop
        for name, v in (("axis", axis), ("sigma", sigma), ("a", a), ("ap", ap), ("b", b)):
            if v is not None:
                arr = _f64(v).ravel()
                if arr.size != nz:
                    raise ValueError("%s must hold nz doubles" % name)
                self._keep.append(arr)
                setattr(s, name, arr.ctypes.data)
        for name, v in (("ps", ps), ("field", field)):
            if v is None:
                continue
            if isinstance(v, int):
                setattr(s, name, v)
            else:
                arr = _f32(v)
                self._keep.append(arr)
                setattr(s, name, arr.ctypes.data)
        self.struct = s

    @classmethod
    def from_field(cls, field, nz):
        return cls(VLEVEL_FIELD, nz, field=field)

    @classmethod
    def from_axis(cls, axis):
        return cls(VLEVEL_AXIS, len(axis), axis=axis)

    @classmethod
    def sigma(cls, sigma, ptop, ps):
        return cls(VLEVEL_SIGMA, len(sigma), sigma=sigma, ptop=ptop, ps=ps)

    @classmethod
    def hybrid_sigma(cls, a, b, p0, ps):
        return cls(VLEVEL_HYBRID_SIGMA, len(a), a=a, b=b, p0=p0, ps=ps)

    @classmethod
    def hybrid_sigma_ap(cls, ap, b, ps):
        return cls(VLEVEL_HYBRID_SIGMA_AP, len(ap), ap=ap, b=b, ps=ps)


def _levels_ref(levels):
    return ctypes.byref(levels.struct) if levels is not None else None


def vertical_interpolate_host(method, data, inLevels, outLevels=None, level1=None, validMin=None, validMax=None,
                              clampMin=float("nan"), clampMax=float("nan")):
    """CDMVerticalInterpolator::getLevelDataSlice on host arrays: data [nt][nzi][ny][nx] -> [nt][nzo][ny][nx], to the fixed levels
    level1 or to the levels of the template description outLevels."""
    d = _f32(data)
    nt, nzi, ny, nx = d.shape
    l1 = _f64(level1).ravel() if level1 is not None else None
    nzo = outLevels.nz if outLevels is not None else (l1.size if l1 is not None else 0)
    vmin = _f64(validMin) if validMin is not None else None
    vmax = _f64(validMax) if validMax is not None else None
    out = np.empty((nt, nzo, ny, nx), np.float32)
    _check(load().fimex_amd_vertical_interpolate_host(method, nx, ny, nt, _fp(d.reshape(-1)), _levels_ref(inLevels), _levels_ref(outLevels),
                                                      _dp(l1) if l1 is not None else None, nzo,
                                                      _dp(vmin.reshape(-1)) if vmin is not None else None,
                                                      _dp(vmax.reshape(-1)) if vmax is not None else None, clampMin, clampMax,
                                                      _fp(out.reshape(-1))))
    return out


def vertical_interpolate_device(method, nx, ny, nt, d_in, inLevels, d_out, outLevels=None, level1=None, d_validMin=None, d_validMax=None,
                                clampMin=float("nan"), clampMax=float("nan"), stream=0):
    """The same on device pointers; only enqueues on `stream`.  level1 stays a host array."""
    l1 = _f64(level1).ravel() if level1 is not None else None
    nzo = outLevels.nz if outLevels is not None else (l1.size if l1 is not None else 0)
    _check(load().fimex_amd_vertical_interpolate_device(method, nx, ny, nt, d_in, _levels_ref(inLevels), _levels_ref(outLevels),
                                                        _dp(l1) if l1 is not None else None, nzo, d_validMin, d_validMax,
                                                        clampMin, clampMax, d_out, stream))


class VerticalPlan:
    """fimex_amd_vertical_plan: the search of vertical_interpolate_* for one set of levels, kept on the device and applied to every
    variable that shares it.  Arguments as for vertical_interpolate_device (device=True: ps / field of the level descriptions,
    validMin and validMax are device pointers and the build is only enqueued on `stream`) or vertical_interpolate_host."""

    def __init__(self, method, nx, ny, nt, inLevels, outLevels=None, level1=None, validMin=None, validMax=None, device=False, stream=0):
        l1 = _f64(level1).ravel() if level1 is not None else None
        nzo = outLevels.nz if outLevels is not None else (l1.size if l1 is not None else 0)
        self._lib = load()
        self._h = _V()
        head = (method, nx, ny, nt, _levels_ref(inLevels), _levels_ref(outLevels), _dp(l1) if l1 is not None else None, nzo)
        if device:
            _check(self._lib.fimex_amd_vertical_plan_create_device(*head, validMin, validMax, stream, ctypes.byref(self._h)))
        else:
            vmin = _f64(validMin).reshape(-1) if validMin is not None else None
            vmax = _f64(validMax).reshape(-1) if validMax is not None else None
            _check(self._lib.fimex_amd_vertical_plan_create_host(*head, _dp(vmin) if vmin is not None else None,
                                                                 _dp(vmax) if vmax is not None else None, ctypes.byref(self._h)))
        self.info = VerticalInfo()
        _check(self._lib.fimex_amd_vertical_plan_info(self._h, ctypes.byref(self.info)))
        self.in_shape = (self.info.nt, self.info.nzi, self.info.ny, self.info.nx)
        self.out_shape = (self.info.nt, self.info.nzo, self.info.ny, self.info.nx)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.fimex_amd_vertical_plan_destroy(self._h)
            self._h = _V()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may be gone already
            pass

    @staticmethod
    def _per_variable(nvar, badValue, clampMin, clampMax):
        spread = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (nvar,)))
        return spread(badValue, np.float64), spread(clampMin, np.float32), spread(clampMax, np.float32)

    def apply_device(self, d_in, cdmType, d_out, badValue=float("nan"), clampMin=float("nan"), clampMax=float("nan"), stream=0):
        """d_in / d_out: one device pointer or a sequence of them, variables of cdmType [nt][nzi][ny][nx] -> [nt][nzo][ny][nx];
        badValue, clampMin, clampMax: one value for all or one per variable.  Only enqueues on `stream`."""
        ins = [d_in] if isinstance(d_in, int) else list(d_in)
        outs = [d_out] if isinstance(d_out, int) else list(d_out)
        if len(ins) != len(outs):
            raise ValueError("as many outputs as inputs")
        n = len(ins)
        bad, cmin, cmax = self._per_variable(n, badValue, clampMin, clampMax)
        _check(self._lib.fimex_amd_vertical_plan_apply_device(self._h, n, (_V * max(n, 1))(*ins), cdmType, _dp(bad), _fp(cmin), _fp(cmax),
                                                              (_V * max(n, 1))(*outs), stream))

    def apply_host(self, data, badValue=float("nan"), clampMin=float("nan"), clampMax=float("nan")):
        """One host array [nt][nzi][ny][nx] of a stored type, or a sequence of them of one type: the interpolated array(s)."""
        single = isinstance(data, np.ndarray)
        arrs = [np.ascontiguousarray(a) for a in ([data] if single else data)]
        n = len(arrs)
        for a in arrs:
            if a.dtype != arrs[0].dtype or a.size != int(np.prod(self.in_shape)):
                raise ValueError("every variable holds %r elements of one type" % (self.in_shape,))
        outs = [np.empty(self.out_shape, arrs[0].dtype) for _ in arrs]
        bad, cmin, cmax = self._per_variable(n, badValue, clampMin, clampMax)
        _check(self._lib.fimex_amd_vertical_plan_apply_host(self._h, n, (_V * n)(*[a.ctypes.data for a in arrs]), cdm_type_of(arrs[0].dtype),
                                                            _dp(bad), _fp(cmin), _fp(cmax), (_V * n)(*[o.ctypes.data for o in outs])))
        return outs[0] if single else outs

    def entries(self):
        """(first, second, factor), each [nt][nzo][ny][nx]; an undefined entry has first == second."""
        first, second = np.empty(self.out_shape, np.uint32), np.empty(self.out_shape, np.uint32)
        factor = np.empty(self.out_shape, np.float32)
        u = ctypes.POINTER(ctypes.c_uint)
        _check(self._lib.fimex_amd_vertical_plan_read_host(self._h, first.ctypes.data_as(u), second.ctypes.data_as(u), _fp(factor)))
        return first, second, factor


def vertical_levels_host(levels, nx, ny, nt):
    """verticalData4D of a level description: float32 [nt][nz][ny][nx]."""
    out = np.empty((nt, levels.nz, ny, nx), np.float32)
    _check(load().fimex_amd_vertical_levels_host(_levels_ref(levels), nx, ny, nt, _fp(out.reshape(-1))))
    return out


def vertical_levels_device(levels, nx, ny, nt, d_out, stream=0):
    _check(load().fimex_amd_vertical_levels_device(_levels_ref(levels), nx, ny, nt, d_out, stream))


def _opt(conv, ptr, v):
    """A host array as a pointer (None stays NULL); returns (array kept alive, pointer)."""
    if v is None:
        return None, None
    arr = conv(v)
    return arr, ptr(arr.reshape(-1))


def vertical_altitude_integrate_host(pressure, nx, ny, nt, airTemperature, surfacePressure, surfaceGeopotential, specificHumidity=None,
                                     surfaceFirst=VORDER_AUTO, topo=None, topoFactor=-1.0):
    """PressureIntegrationToAltitudeConverter (then AltitudeHeightConverter when topo is given) on host arrays:
    float32 [nt][nz][ny][nx]."""
    T, Tp = _opt(_f32, _fp, airTemperature)
    q, qp = _opt(_f32, _fp, specificHumidity)
    sap, sapp = _opt(_f32, _fp, surfacePressure)
    sgp, sgpp = _opt(_f32, _fp, surfaceGeopotential)
    tp, tpp = _opt(_f64, _dp, topo)
    out = np.empty((nt, pressure.nz, ny, nx), np.float32)
    _check(load().fimex_amd_vertical_altitude_integrate_host(_levels_ref(pressure), nx, ny, nt, Tp, qp, sapp, sgpp, surfaceFirst, tpp, topoFactor,
                                                             _fp(out.reshape(-1))))
    return out


def vertical_altitude_integrate_device(pressure, nx, ny, nt, d_airTemperature, d_surfacePressure, d_surfaceGeopotential, d_out,
                                       d_specificHumidity=None, surfaceFirst=VORDER_AUTO, d_topo=None, topoFactor=-1.0, stream=0):
    """The same on device pointers; only enqueues on `stream`."""
    _check(load().fimex_amd_vertical_altitude_integrate_device(_levels_ref(pressure), nx, ny, nt, d_airTemperature, d_specificHumidity,
                                                               d_surfacePressure, d_surfaceGeopotential, surfaceFirst, d_topo, topoFactor,
                                                               d_out, stream))


def _standard_host(fn, levels, nx, ny, nt, topo, topoFactor):
    tp, tpp = _opt(_f64, _dp, topo)
    out = np.empty((nt, levels.nz, ny, nx), np.float32)
    _check(fn(_levels_ref(levels), nx, ny, nt, tpp, topoFactor, _fp(out.reshape(-1))))
    return out


def vertical_standard_altitude_host(pressure, nx, ny, nt, topo=None, topoFactor=-1.0):
    """PressureToStandardAltitudeConverter (+ AltitudeHeightConverter with topo): float32 [nt][nz][ny][nx]."""
    return _standard_host(load().fimex_amd_vertical_standard_altitude_host, pressure, nx, ny, nt, topo, topoFactor)


def vertical_standard_altitude_device(pressure, nx, ny, nt, d_out, d_topo=None, topoFactor=-1.0, stream=0):
    _check(load().fimex_amd_vertical_standard_altitude_device(_levels_ref(pressure), nx, ny, nt, d_topo, topoFactor, d_out, stream))


def vertical_standard_pressure_host(altitude, nx, ny, nt, topo=None, topoFactor=1.0):
    """AltitudeStandardToPressureConverter (behind an AltitudeHeightConverter with topo): float32 [nt][nz][ny][nx]."""
    return _standard_host(load().fimex_amd_vertical_standard_pressure_host, altitude, nx, ny, nt, topo, topoFactor)


def vertical_standard_pressure_device(altitude, nx, ny, nt, d_out, d_topo=None, topoFactor=1.0, stream=0):
    _check(load().fimex_amd_vertical_standard_pressure_device(_levels_ref(altitude), nx, ny, nt, d_topo, topoFactor, d_out, stream))


def vertical_ocean_depth_host(generation, nx, ny, nt, s, C, depth_c, depth, eta=None):
    """OceanSCoordinateGToDepthConverter: float32 [nt][nz][ny][nx], positive down."""
    sa, sp = _opt(_f64, _dp, s)
    ca, cp = _opt(_f64, _dp, C)
    da, dpp = _opt(_f64, _dp, depth)
    ea, ep = _opt(_f64, _dp, eta)
    nz = sa.size if sa is not None else 0
    out = np.empty((nt, nz, ny, nx), np.float32)
    _check(load().fimex_amd_vertical_ocean_depth_host(generation, nx, ny, nz, nt, sp, cp, depth_c, dpp, ep, _fp(out.reshape(-1))))
    return out


def vertical_ocean_depth_device(generation, nx, ny, nt, s, C, depth_c, d_depth, d_out, d_eta=None, stream=0):
    """s and C stay host arrays."""
    sa, sp = _opt(_f64, _dp, s)
    ca, cp = _opt(_f64, _dp, C)
    nz = sa.size if sa is not None else 0
    _check(load().fimex_amd_vertical_ocean_depth_device(generation, nx, ny, nz, nt, sp, cp, depth_c, d_depth, d_eta, d_out, stream))


def griddistance_host(lonVals, latVals):
    """mifi_griddistance: lon / lat [ny][nx] in degrees -> (gridDistX, gridDistY) float32 [ny][nx] in m.  A grid of one point raises,
    as the reference returns MIFI_ERROR for it."""
    lo, la = _f64(lonVals), _f64(latVals)
    ny, nx = lo.shape
    gx, gy = np.empty((ny, nx), np.float32), np.empty((ny, nx), np.float32)
    _check(load().fimex_amd_griddistance_host(nx, ny, _dp(lo.reshape(-1)), _dp(la.reshape(-1)), _fp(gx.reshape(-1)), _fp(gy.reshape(-1))))
    return gx, gy


def griddistance_device(nx, ny, d_lon, d_lat, d_gridDistX, d_gridDistY, stream=0):
    """The same on device pointers; only enqueues on `stream`."""
    _check(load().fimex_amd_griddistance_device(nx, ny, d_lon, d_lat, d_gridDistX, d_gridDistY, stream))


def vertical_velocity_host(nx, ny, nt, dx, dy, gridDistX, gridDistY, ap, b, zs, ps, u, v, t):
    """mifi_compute_vertical_velocity for nt time steps on host arrays: float32 [nt][nz][ny][nx].  ap (Pa) and b hold nz doubles; zs
    [ny][nx]; ps (Pa) [nt][ny][nx]; u, v, t [nt][nz][ny][nx]."""
    apa, app = _opt(_f64, _dp, ap)
    ba, bp = _opt(_f64, _dp, b)
    nz = apa.size if apa is not None else 0
    arrays = [_opt(_f32, _fp, a) for a in (gridDistX, gridDistY, zs, ps, u, v, t)]
    out = np.empty((nt, nz, ny, nx), np.float32)
    _check(load().fimex_amd_vertical_velocity_host(nx, ny, nz, nt, dx, dy, arrays[0][1], arrays[1][1], app, bp, *[a[1] for a in arrays[2:]],
                                                   _fp(out.reshape(-1))))
    return out


def vertical_velocity_device(nx, ny, nt, dx, dy, d_gridDistX, d_gridDistY, ap, b, d_zs, d_ps, d_u, d_v, d_t, d_w, stream=0):
    """The same on device pointers; only enqueues on `stream`.  ap and b stay host arrays."""
    apa, app = _opt(_f64, _dp, ap)
    ba, bp = _opt(_f64, _dp, b)
    nz = apa.size if apa is not None else 0
    _check(load().fimex_amd_vertical_velocity_device(nx, ny, nz, nt, dx, dy, d_gridDistX, d_gridDistY, app, bp, d_zs, d_ps, d_u, d_v, d_t, d_w,
                                                     stream))


def omega_to_vertical_wind_host(pressure, nx, ny, nt, omega, t):
    """OmegaVerticalConverter (omega2vwind) on host arrays: float32 [nt][nz][ny][nx]; the pressure unit of omega is that of the level
    description."""
    oa, op = _opt(_f32, _fp, omega)
    ta, tp = _opt(_f32, _fp, t)
    out = np.empty((nt, pressure.nz, ny, nx), np.float32)
    _check(load().fimex_amd_omega_to_vertical_wind_host(_levels_ref(pressure), nx, ny, nt, op, tp, _fp(out.reshape(-1))))
    return out


def omega_to_vertical_wind_device(pressure, nx, ny, nt, d_omega, d_t, d_w, stream=0):
    """The same on device pointers; d_w may be d_omega (in place).  Only enqueues on `stream`."""
    _check(load().fimex_amd_omega_to_vertical_wind_device(_levels_ref(pressure), nx, ny, nt, d_omega, d_t, d_w, stream))


def convert_scaled_host(data, oldFill, oldScale, oldOffset, outType, newFill, newScale=1.0, newOffset=0.0):
    """DataImpl::convertDataType on a host array of a stored type: the array of outType, same shape."""
    a = np.ascontiguousarray(data)
    out = np.empty(a.shape, CDM_DTYPES[outType])
    _check(load().fimex_amd_convert_scaled_host(a.ctypes.data, cdm_type_of(a.dtype), a.size, oldFill, oldScale, oldOffset, outType, newFill,
                                                newScale, newOffset, out.ctypes.data))
    return out


def convert_scaled_device(d_in, inType, n, oldFill, oldScale, oldOffset, outType, newFill, newScale, newOffset, d_out, stream=0):
    """The same on device pointers; d_out may be d_in when both types have one size.  Only enqueues on `stream`."""
    _check(load().fimex_amd_convert_scaled_device(d_in, inType, n, oldFill, oldScale, oldOffset, outType, newFill, newScale, newOffset, d_out,
                                                  stream))


def theta_to_temperature_host(pressure, nx, ny, nt, theta, addOffset=0.0):
    """ThetaTemperatureConverter (theta2T) on host arrays: float32 [nt][nz][ny][nx], pressure levels in hPa."""
    ta, tp = _opt(_f32, _fp, theta)
    out = np.empty((nt, pressure.nz, ny, nx), np.float32)
    _check(load().fimex_amd_theta_to_temperature_host(_levels_ref(pressure), nx, ny, nt, tp, addOffset, _fp(out.reshape(-1))))
    return out


def theta_to_temperature_device(pressure, nx, ny, nt, d_theta, addOffset, d_T, stream=0):
    """The same on device pointers; d_T may be d_theta (in place).  Only enqueues on `stream`."""
    _check(load().fimex_amd_theta_to_temperature_device(_levels_ref(pressure), nx, ny, nt, d_theta, addOffset, d_T, stream))


def specific_to_relative_humidity_host(pressure, nx, ny, nt, q, T):
    """HumidityConverter (specific2relative) on host arrays: q and T float32 [nt][nz][ny][nx] -> int16 with scale factor 1 / 25000."""
    qa, qp = _opt(_f32, _fp, q)
    ta, tp = _opt(_f32, _fp, T)
    out = np.empty((nt, pressure.nz, ny, nx), np.int16)
    _check(load().fimex_amd_specific_to_relative_humidity_host(_levels_ref(pressure), nx, ny, nt, qp, tp, out.ctypes.data))
    return out


def specific_to_relative_humidity_device(pressure, nx, ny, nt, d_q, d_T, d_rh, stream=0):
    _check(load().fimex_amd_specific_to_relative_humidity_device(_levels_ref(pressure), nx, ny, nt, d_q, d_T, d_rh, stream))


def accumulate_host(data, firstPos=0, prev=None):
    """CDMProcessor's accumulate over the positions data[0 .. nt-1] = firstPos ..: float64, same shape.  prev: acc[firstPos - 1]."""
    a = np.ascontiguousarray(data)
    nt = a.shape[0]
    p = _f64(prev).reshape(-1) if prev is not None else None
    out = np.empty(a.shape, np.float64)
    _check(load().fimex_amd_accumulate_host(a.ctypes.data, cdm_type_of(a.dtype), a.size // nt if nt else 0, nt, firstPos,
                                            _dp(p) if p is not None else None, _dp(out.reshape(-1))))
    return out


def accumulate_device(d_in, cdmType, n, nt, firstPos, d_prev, d_out, stream=0):
    _check(load().fimex_amd_accumulate_device(d_in, cdmType, n, nt, firstPos, d_prev, d_out, stream))


def deaccumulate_host(data, firstPos=0, prev=None):
    """CDMProcessor's deaccumulate: float64, same shape.  prev: the position in front of the batch, in the type of data."""
    a = np.ascontiguousarray(data)
    nt = a.shape[0]
    p = np.ascontiguousarray(prev, a.dtype).reshape(-1) if prev is not None else None
    out = np.empty(a.shape, np.float64)
    _check(load().fimex_amd_deaccumulate_host(a.ctypes.data, cdm_type_of(a.dtype), a.size // nt if nt else 0, nt, firstPos,
                                              p.ctypes.data if p is not None else None, _dp(out.reshape(-1))))
    return out


def deaccumulate_device(d_in, cdmType, n, nt, firstPos, d_prev, d_out, stream=0):
    _check(load().fimex_amd_deaccumulate_device(d_in, cdmType, n, nt, firstPos, d_prev, d_out, stream))


# fimex_amd_time_interpolate_device: output steps per launch, and per chunk where a launch is split over gridDim.y (include/fimex_amd.h)
TIME_LAUNCH_STEPS, TIME_CHUNK_STEPS = 128, 32


def time_mapping(oldTimes, newTimes):
    """The slice mapping of CDMTimeInterpolator::changeTimeAxis: (t1, t2), two index arrays of len(newTimes).  Runs on the CPU."""
    o, x = _f64(oldTimes).reshape(-1), _f64(newTimes).reshape(-1)
    t1, t2 = np.zeros(x.size, np.uintp), np.zeros(x.size, np.uintp)
    _check(load().fimex_amd_time_mapping(_dp(o), o.size, _dp(x), x.size, t1.ctypes.data_as(_ZP), t2.ctypes.data_as(_ZP)))
    return t1, t2


def time_interpolate_host(data, oldTimes, newTimes):
    """CDMTimeInterpolator on a host array of a stored type, data[nOld, ...]: float32 [nNew, ...]."""
    a = np.ascontiguousarray(data)
    o, x = _f64(oldTimes).reshape(-1), _f64(newTimes).reshape(-1)
    if a.shape[0] != o.size:
        raise ValueError("data holds %d slices for %d old times" % (a.shape[0], o.size))
    out = np.empty((x.size,) + a.shape[1:], np.float32)
    _check(load().fimex_amd_time_interpolate_host(a.ctypes.data, cdm_type_of(a.dtype), a.size // o.size if o.size else 0, _dp(o), o.size, _dp(x),
                                                  x.size, _fp(out.reshape(-1))))
    return out


def time_interpolate_device(d_in, cdmType, n, oldTimes, newTimes, d_out, stream=0):
    """The same on device pointers: d_in [nOld][n] of cdmType, d_out float32 [nNew][n].  Only enqueues on `stream`."""
    o, x = _f64(oldTimes).reshape(-1), _f64(newTimes).reshape(-1)
    _check(load().fimex_amd_time_interpolate_device(d_in, cdmType, n, _dp(o), o.size, _dp(x), x.size, d_out, stream))


# fimex_amd_quality_mode
QUALITY_VALUES, QUALITY_ALL, QUALITY_MAX, QUALITY_MIN, QUALITY_HIGHEST, QUALITY_LOWEST = 0, 1, 2, 3, 4, 5
_NAN = float("nan")


def quality_mask_host(data, status, mode, fillValue, values=(), limit=_NAN, validMin=_NAN, validMax=_NAN, statusFill=_NAN):
    """CDMQualityExtractor on host arrays of stored types: a masked copy of data.  status=None: the data is its own status.
    Sizes the library refuses raise; the reference's warn-and-pass-on is the caller's part."""
    out = np.array(data, order="C", copy=True)
    s = out if status is None else np.ascontiguousarray(status)
    v = _f64(values).reshape(-1)
    _check(load().fimex_amd_quality_mask_host(out.ctypes.data, cdm_type_of(out.dtype), out.size, s.ctypes.data, cdm_type_of(s.dtype), s.size, mode,
                                              _dp(v) if v.size else None, v.size, limit, validMin, validMax, statusFill, fillValue))
    return out


def quality_mask_device(d_data, dataType, nData, d_status, statusType, nStatus, mode, fillValue, values=(), limit=_NAN, validMin=_NAN,
                        validMax=_NAN, statusFill=_NAN, stream=0):
    """The same in place on device pointers; d_status may be d_data (one type, one size).  Only enqueues on `stream`."""
    v = _f64(values).reshape(-1)
    _check(load().fimex_amd_quality_mask_device(d_data, dataType, nData, d_status, statusType, nStatus, mode, _dp(v) if v.size else None, v.size,
                                                limit, validMin, validMax, statusFill, fillValue, stream))


def _extract_dims(dims):
    """dims, fastest first: (length, positions) or (length, positions, start, size); positions None for a dimension that is not
    reduced; without a window the whole reduced dimension is taken.  Returns the ctypes array and what it points into."""
    arr = (ExtractDim * max(len(dims), 1))()
    keep = []
    for d, spec in zip(arr, dims):
        length, positions = spec[0], spec[1]
        d.length = length
        d.reduced = int(positions is not None)
        if positions is not None:
            p = np.ascontiguousarray(positions, dtype=np.uintp).reshape(-1)
            keep.append(p)
            d.positions = p.ctypes.data_as(_ZP) if p.size else None
            d.nPositions = p.size
        d.start, d.size = (spec[2], spec[3]) if len(spec) > 2 else (0, length if positions is None else d.nPositions)
    return arr, keep


def extract_describe(dims):
    """Checks a reduction (see _extract_dims) and returns the ExtractInfo of the plan it gives.  Runs on the CPU."""
    arr, keep = _extract_dims(dims)
    info = ExtractInfo()
    _check(load().fimex_amd_extract_describe(arr, len(dims), ctypes.byref(info)))
    return info


class ExtractPlan:
    """fimex_amd_extract_plan: CDMExtractor's data path for one variable, dims as for _extract_dims."""

    def __init__(self, dims):
        arr, keep = _extract_dims(dims)
        self._lib = load()
        self._h = _V()
        _check(self._lib.fimex_amd_extract_plan_create(arr, len(dims), ctypes.byref(self._h)))
        self.info = ExtractInfo()
        _check(self._lib.fimex_amd_extract_plan_info(self._h, ctypes.byref(self.info)))
        self.shape = tuple(int(d.size) for d in arr[:len(dims)])[::-1]  # slowest first, as numpy

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.fimex_amd_extract_plan_destroy(self._h)
            self._h = _V()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may be gone already
            pass

    def apply_device(self, d_in, cdmType, d_out, stream=0):
        """d_in: info.inElements elements of cdmType, d_out: info.outElements.  Only enqueues on `stream`."""
        _check(self._lib.fimex_amd_extract_apply_device(self._h, d_in, cdmType, d_out, stream))

    def apply_host(self, data):
        """A host array of a stored type with info.inElements elements: the reduced array, slowest dimension first."""
        a = np.ascontiguousarray(data)
        if a.size != self.info.inElements:
            raise ValueError("data holds %d elements, the plan reads %d" % (a.size, self.info.inElements))
        out = np.empty(self.shape, a.dtype)
        _check(self._lib.fimex_amd_extract_apply_host(self._h, a.ctypes.data, cdm_type_of(a.dtype), out.ctypes.data))
        return out


def extract_axis_range(axis, startVal, endVal):
    """The index arithmetic of CDMExtractor::reduceAxes on a 1-D axis in the unit of the bounds: (start, size).  Runs on the CPU."""
    a = _f64(axis).reshape(-1)
    start, size = ctypes.c_size_t(), ctypes.c_size_t()
    _check(load().fimex_amd_extract_axis_range(_dp(a) if a.size else None, a.size, startVal, endVal, ctypes.byref(start), ctypes.byref(size)))
    return start.value, size.value


def extract_bounding_box_host(proj_input, proj_lonlat, xAxis, yAxis, south, north, west, east, axesInDegree=False):
    """CDMExtractor::reduceLatLonBoundingBox on two 1-D axes: the ascending x and y positions with a mesh point inside the box."""
    x, y = _f64(xAxis).reshape(-1), _f64(yAxis).reshape(-1)
    xp, yp = np.zeros(x.size, np.uintp), np.zeros(y.size, np.uintp)
    nX, nY = ctypes.c_size_t(), ctypes.c_size_t()
    _check(load().fimex_amd_extract_bounding_box_host(proj_input.encode(), proj_lonlat.encode(), _dp(x) if x.size else None, x.size,
                                                      _dp(y) if y.size else None, y.size, int(bool(axesInDegree)), south, north, west, east,
                                                      xp.ctypes.data_as(_ZP), ctypes.byref(nX), yp.ctypes.data_as(_ZP), ctypes.byref(nY)))
    return xp[:nX.value].copy(), yp[:nY.value].copy()


def border_smooth_host(inner, outerOnInner, transitionWidth=5, borderWidth=2, useOuterIfInnerUndefined=True):
    """CDMBorderSmoothing::getDataSlice with the linear smoothing: two [nz][ny][nx] (or [ny][nx]) float32 host arrays -> the smoothed one."""
    i, o = _f32(inner), _f32(outerOnInner)
    if i.shape != o.shape or i.ndim < 2:
        raise ValueError("inner and outer differ in shape")
    ny, nx = i.shape[-2:]
    out = np.empty_like(i)
    _check(load().fimex_amd_border_smooth_host(_fp(i), _fp(o), _fp(out), nx, ny, i.size // max(nx * ny, 1), transitionWidth, borderWidth,
                                               int(bool(useOuterIfInnerUndefined))))
    return out


def border_smooth_device(d_inner, d_outerOnInner, d_out, nx, ny, nz, transitionWidth=5, borderWidth=2, useOuterIfInnerUndefined=True, stream=0):
    _check(load().fimex_amd_border_smooth_device(d_inner, d_outerOnInner, d_out, nx, ny, nz, transitionWidth, borderWidth,
                                                 int(bool(useOuterIfInnerUndefined)), stream))


def overlay_host(top, base):
    """CDMOverlay::getDataSlice: top where it is defined, else base."""
    t, b = _f32(top), _f32(base)
    if t.shape != b.shape:
        raise ValueError("top and base differ in shape")
    out = np.empty_like(t)
    _check(load().fimex_amd_overlay_host(_fp(t), _fp(b), _fp(out), t.size))
    return out


def overlay_device(d_top, d_base, d_out, n, stream=0):
    _check(load().fimex_amd_overlay_device(d_top, d_base, d_out, n, stream))


def _typed(a, packing):
    a = np.ascontiguousarray(a)
    if cdm_type_of(a.dtype) != packing.type:
        raise TypeError("the array's dtype %s is not the packing's type %d" % (a.dtype, packing.type))
    return a


def border_smooth_typed_host(inner, innerPacking, outerOnInner, outerPacking, transitionWidth=5, borderWidth=2, useOuterIfInnerUndefined=True):
    """CDMBorderSmoothing::getDataSlice on two [nz][ny][nx] (or [ny][nx]) host arrays in their stored types, each with its Packing
    -> the smoothed field in the inner's type and packing."""
    i, o = _typed(inner, innerPacking), _typed(outerOnInner, outerPacking)
    if i.shape != o.shape or i.ndim < 2:
        raise ValueError("inner and outer differ in shape")
    ny, nx = i.shape[-2:]
    out = np.empty_like(i)
    _check(load().fimex_amd_border_smooth_typed_host(i.ctypes.data, ctypes.byref(innerPacking), o.ctypes.data, ctypes.byref(outerPacking),
                                                     out.ctypes.data, nx, ny, i.size // max(nx * ny, 1), transitionWidth, borderWidth,
                                                     int(bool(useOuterIfInnerUndefined))))
    return out


def border_smooth_typed_device(d_inner, innerPacking, d_outerOnInner, outerPacking, d_out, nx, ny, nz, transitionWidth=5, borderWidth=2,
                               useOuterIfInnerUndefined=True, stream=0):
    """The same on device pointers; d_out may be d_inner, and d_outerOnInner where both types have one size."""
    _check(load().fimex_amd_border_smooth_typed_device(d_inner, ctypes.byref(innerPacking), d_outerOnInner, ctypes.byref(outerPacking), d_out, nx,
                                                       ny, nz, transitionWidth, borderWidth, int(bool(useOuterIfInnerUndefined)), stream))


def overlay_typed_host(top, topPacking, base, basePacking):
    """CDMOverlay::getDataSlice on two host arrays in their stored types -> the top's type and packing."""
    t, b = _typed(top, topPacking), _typed(base, basePacking)
    if t.shape != b.shape:
        raise ValueError("top and base differ in shape")
    out = np.empty_like(t)
    _check(load().fimex_amd_overlay_typed_host(t.ctypes.data, ctypes.byref(topPacking), b.ctypes.data, ctypes.byref(basePacking), out.ctypes.data,
                                               t.size))
    return out


def overlay_typed_device(d_top, topPacking, d_base, basePacking, d_out, n, stream=0):
    _check(load().fimex_amd_overlay_typed_device(d_top, ctypes.byref(topPacking), d_base, ctypes.byref(basePacking), d_out, n, stream))


class MergePlan:
    """fimex_amd_merge_plan: CDMMerger's data path on three backward RegridPlans (outer -> inner grid, inner -> target,
    outer -> target), which it keeps alive."""

    def __init__(self, outerToInner, innerToTarget, outerToTarget, transitionWidth=5, borderWidth=2, useOuterIfInnerUndefined=True):
        self._plans = (outerToInner, innerToTarget, outerToTarget)
        self._h = _V()
        self.outX, self.outY = innerToTarget.outX, innerToTarget.outY
        _check(load().fimex_amd_merge_plan_create(outerToInner._h, innerToTarget._h, outerToTarget._h, transitionWidth, borderWidth,
                                                  int(bool(useOuterIfInnerUndefined)), ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().fimex_amd_merge_plan_destroy(self._h)
            self._h = _V()
        self._plans = ()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may be gone already
            pass

    def apply_host(self, inner, outer):
        """CDMMerger::getDataSlice: inner [nz][iy][ix], outer [nz][oy][ox] float32 host arrays -> [nz][ty][tx]."""
        oi = self._plans[0]
        i, o = _f32(inner).ravel(), _f32(outer).ravel()
        nz = i.size // (oi.outX * oi.outY)
        if i.size != nz * oi.outX * oi.outY or o.size != nz * oi.inX * oi.inY:
            raise ValueError("inner and outer do not hold the same number of whole slices")
        out = np.empty((nz, self.outY, self.outX), dtype=np.float32)
        _check(load().fimex_amd_merge_apply_host(self._h, _fp(i), _fp(o), nz, _fp(out)))
        return out

    def apply_device(self, d_inner, d_outer, nz, d_out, stream=0):
        _check(load().fimex_amd_merge_apply_device(self._h, d_inner, d_outer, nz, d_out, stream))

    def apply_chain_device(self, d_inner, d_outer, nz, d_out, stream=0):
        """The same merge by the plain applies and the two elementwise kernels (cross-check and yardstick of the fused kernels)."""
        _check(load().fimex_amd_merge_apply_chain_device(self._h, d_inner, d_outer, nz, d_out, stream))

    def apply_typed_device(self, d_inner, innerPacking, d_outer, outerPacking, nz, d_out, stream=0):
        """The merge on variables in their stored types, each with its Packing; d_out holds the inner's type in the inner's packing.
        Returns the path: 1 the two fused kernels, 0 the chain of apply_typed_chain_device."""
        path = ctypes.c_int(-1)
        _check(load().fimex_amd_merge_apply_typed_device(self._h, d_inner, ctypes.byref(innerPacking), d_outer, ctypes.byref(outerPacking), nz,
                                                         d_out, stream, ctypes.byref(path)))
        return path.value

    def apply_typed_chain_device(self, d_inner, innerPacking, d_outer, outerPacking, nz, d_out, stream=0):
        """The same by regrid_apply_typed_device three times and the two typed elementwise kernels (cross-check and yardstick)."""
        _check(load().fimex_amd_merge_apply_typed_chain_device(self._h, d_inner, ctypes.byref(innerPacking), d_outer, ctypes.byref(outerPacking),
                                                               nz, d_out, stream))

    def apply_typed_host(self, inner, innerPacking, outer, outerPacking):
        """The same on host arrays inner [nz][iy][ix] and outer [nz][oy][ox] in their stored types -> [nz][ty][tx] in the inner's."""
        oi = self._plans[0]
        i, o = _typed(inner, innerPacking).ravel(), _typed(outer, outerPacking).ravel()
        nz = i.size // (oi.outX * oi.outY)
        if i.size != nz * oi.outX * oi.outY or o.size != nz * oi.inX * oi.inY:
            raise ValueError("inner and outer do not hold the same number of whole slices")
        out = np.empty((nz, self.outY, self.outX), dtype=i.dtype)
        _check(load().fimex_amd_merge_apply_typed_host(self._h, i.ctypes.data, ctypes.byref(innerPacking), o.ctypes.data, ctypes.byref(outerPacking),
                                                       nz, out.ctypes.data))
        return out

    def apply_vector_device(self, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, d_innerV, d_outerU, d_outerV, nz, d_outU, d_outV,
                            stream=0):
        """The merge of an x/y vector pair of float arrays: each of the three regrids is followed by the rotation of its VectorPlan
        (outerToInnerVec on the inner grid, the other two on the target).  Two fused kernels."""
        _check(load().fimex_amd_merge_apply_vector_device(self._h, outerToInnerVec._h, innerToTargetVec._h, outerToTargetVec._h, d_innerU, d_innerV,
                                                          d_outerU, d_outerV, nz, d_outU, d_outV, stream))

    def apply_vector_chain_device(self, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, d_innerV, d_outerU, d_outerV, nz, d_outU,
                                  d_outV, stream=0):
        """The same step by step: the pair regridded and rotated three times, the smoothing and the overlay once per component
        (cross-check and yardstick of the fused kernels)."""
        _check(load().fimex_amd_merge_apply_vector_chain_device(self._h, outerToInnerVec._h, innerToTargetVec._h, outerToTargetVec._h, d_innerU,
                                                                d_innerV, d_outerU, d_outerV, nz, d_outU, d_outV, stream))

    def apply_vector_host(self, outerToInnerVec, innerToTargetVec, outerToTargetVec, innerU, innerV, outerU, outerV):
        """The same on float32 host arrays: inner [nz][iy][ix] and outer [nz][oy][ox] components -> (outU, outV), each [nz][ty][tx]."""
        oi = self._plans[0]
        iu, iv, ou, ov = (_f32(a).ravel() for a in (innerU, innerV, outerU, outerV))
        nz = iu.size // (oi.outX * oi.outY)
        if iu.size != nz * oi.outX * oi.outY or iv.size != iu.size or ou.size != nz * oi.inX * oi.inY or ov.size != ou.size:
            raise ValueError("the four components do not hold the same number of whole slices")
        outU, outV = (np.empty((nz, self.outY, self.outX), dtype=np.float32) for _ in range(2))
        _check(load().fimex_amd_merge_apply_vector_host(self._h, outerToInnerVec._h, innerToTargetVec._h, outerToTargetVec._h, _fp(iu), _fp(iv),
                                                        _fp(ou), _fp(ov), nz, _fp(outU), _fp(outV)))
        return outU, outV

    def _vector_typed_args(self, vecs, fields, nz, outs):
        """(plan, three vector plans, pointer and packing of inner u, inner v, outer u, outer v, nz, outU, outV) of the C entries"""
        pairs = [x for ptr, packing in fields for x in (ptr, ctypes.byref(packing))]
        return [self._h] + [v._h for v in vecs] + pairs + [nz] + list(outs)

    def apply_vector_typed_device(self, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, innerUPacking, d_innerV, innerVPacking,
                                  d_outerU, outerUPacking, d_outerV, outerVPacking, nz, d_outU, d_outV, stream=0):
        """The merge of an x/y vector pair whose four fields are in their stored types, each with its Packing; the rotations act on
        the raw counts.  d_outU holds inner u's type in inner u's packing, d_outV inner v's.  Returns the path: 1 the two fused
        kernels, 0 the chain of apply_vector_typed_chain_device."""
        path = ctypes.c_int(-1)
        args = self._vector_typed_args((outerToInnerVec, innerToTargetVec, outerToTargetVec),
                                       ((d_innerU, innerUPacking), (d_innerV, innerVPacking), (d_outerU, outerUPacking), (d_outerV, outerVPacking)),
                                       nz, (d_outU, d_outV))
        _check(load().fimex_amd_merge_apply_vector_typed_device(*args, stream, ctypes.byref(path)))
        return path.value

    def apply_vector_typed_chain_device(self, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, innerUPacking, d_innerV, innerVPacking,
                                        d_outerU, outerUPacking, d_outerV, outerVPacking, nz, d_outU, d_outV, stream=0):
        """The same step by step: the pair regridded and rotated three times on its stored types, the typed smoothing and the typed
        overlay once per component (cross-check and yardstick of the fused kernels; every numeric type, components of different types)."""
        args = self._vector_typed_args((outerToInnerVec, innerToTargetVec, outerToTargetVec),
                                       ((d_innerU, innerUPacking), (d_innerV, innerVPacking), (d_outerU, outerUPacking), (d_outerV, outerVPacking)),
                                       nz, (d_outU, d_outV))
        _check(load().fimex_amd_merge_apply_vector_typed_chain_device(*args, stream))

    def apply_vector_typed_host(self, outerToInnerVec, innerToTargetVec, outerToTargetVec, innerU, innerUPacking, innerV, innerVPacking, outerU,
                                outerUPacking, outerV, outerVPacking):
        """The same on host arrays in their stored types: inner [nz][iy][ix] and outer [nz][oy][ox] components -> (outU, outV), each
        [nz][ty][tx] in its inner component's type."""
        oi = self._plans[0]
        iu, iv, ou, ov = (_typed(a, p).ravel() for a, p in ((innerU, innerUPacking), (innerV, innerVPacking), (outerU, outerUPacking),
                                                            (outerV, outerVPacking)))
        nz = iu.size // (oi.outX * oi.outY)
        if iu.size != nz * oi.outX * oi.outY or iv.size != iu.size or ou.size != nz * oi.inX * oi.inY or ov.size != ou.size:
            raise ValueError("the four components do not hold the same number of whole slices")
        outU, outV = (np.empty((nz, self.outY, self.outX), dtype=a.dtype) for a in (iu, iv))
        args = self._vector_typed_args((outerToInnerVec, innerToTargetVec, outerToTargetVec),
                                       ((iu.ctypes.data, innerUPacking), (iv.ctypes.data, innerVPacking), (ou.ctypes.data, outerUPacking),
                                        (ov.ctypes.data, outerVPacking)), nz, (outU.ctypes.data, outV.ctypes.data))
        _check(load().fimex_amd_merge_apply_vector_typed_host(*args))
        return outU, outV


def project_values_host(proj_input, proj_output, x, y):
    """mifi_project_values: returns the transformed copies of x and y."""
    xs, ys = _f64(x).copy(), _f64(y).copy()
    fx, fy = xs.reshape(-1), ys.reshape(-1)
    _check(load().fimex_amd_project_values_host(proj_input.encode(), proj_output.encode(), _dp(fx), _dp(fy), fx.size))
    return xs, ys


def project_axes_host(proj_input, proj_output, xAxis, yAxis):
    """mifi_project_axes: two [iy][ix] fields."""
    ax, ay = _f64(xAxis).ravel(), _f64(yAxis).ravel()
    ox, oy = np.empty(ax.size * ay.size), np.empty(ax.size * ay.size)
    _check(load().fimex_amd_project_axes_host(proj_input.encode(), proj_output.encode(), _dp(ax), _dp(ay), ax.size, ay.size, _dp(ox), _dp(oy)))
    return ox.reshape(ay.size, ax.size), oy.reshape(ay.size, ax.size)


def project_axes_device(proj_input, proj_output, xAxis, yAxis, d_outX, d_outY, stream=0):
    ax, ay = _f64(xAxis).ravel(), _f64(yAxis).ravel()
    _check(load().fimex_amd_project_axes_device(proj_input.encode(), proj_output.encode(), _dp(ax), _dp(ay), ax.size, ay.size, d_outX, d_outY, stream))


def get_vector_reproject_matrix_host(proj_input, proj_output, outXAxis, outYAxis, xAxisType=PROJ_AXIS, yAxisType=PROJ_AXIS):
    """mifi_get_vector_reproject_matrix: float64 [oy*ox*4]."""
    ax, ay = _f64(outXAxis).ravel(), _f64(outYAxis).ravel()
    m = np.empty(4 * ax.size * ay.size)
    _check(load().fimex_amd_get_vector_reproject_matrix_host(proj_input.encode(), proj_output.encode(), _dp(ax), _dp(ay), xAxisType, yAxisType,
                                                             ax.size, ay.size, _dp(m)))
    return m


def get_vector_reproject_matrix_device(proj_input, proj_output, outXAxis, outYAxis, xAxisType, yAxisType, d_matrix, stream=0):
    ax, ay = _f64(outXAxis).ravel(), _f64(outYAxis).ravel()
    _check(load().fimex_amd_get_vector_reproject_matrix_device(proj_input.encode(), proj_output.encode(), _dp(ax), _dp(ay), xAxisType, yAxisType,
                                                               ax.size, ay.size, d_matrix, stream))


def get_vector_reproject_matrix_field_host(proj_input, proj_output, inXField, inYField):
    fx, fy = _f64(inXField), _f64(inYField)
    oy, ox = fx.shape
    m = np.empty(4 * fx.size)
    _check(load().fimex_amd_get_vector_reproject_matrix_field_host(proj_input.encode(), proj_output.encode(), _dp(fx.reshape(-1)), _dp(fy.reshape(-1)), ox, oy, _dp(m)))
    return m


def get_vector_reproject_matrix_points_host(proj_input, proj_output, inputIsMetric, outX, outY):
    px, py = _f64(outX).ravel(), _f64(outY).ravel()
    m = np.empty(4 * px.size)
    _check(load().fimex_amd_get_vector_reproject_matrix_points_host(proj_input.encode(), proj_output.encode(), 1 if inputIsMetric else 0, _dp(px), _dp(py), px.size, _dp(m)))
    return m


def rotate_vector_typed_host(vec, xData, xFill, yData, yFill, returnX=True, outFill=None):
    """CDMProcessor's vector rotation on stored types; returns the requested component in its own type."""
    x, y = np.ascontiguousarray(xData), np.ascontiguousarray(yData)
    keep = x if returnX else y
    out = np.empty(keep.shape, keep.dtype)
    _check(load().fimex_amd_rotate_vector_typed_host(vec._h, x.ctypes.data, cdm_type_of(x.dtype), xFill, y.ctypes.data, cdm_type_of(y.dtype), yFill,
                                                     x.size, 1 if returnX else 0, cdm_type_of(keep.dtype),
                                                     (xFill if returnX else yFill) if outFill is None else outFill, out.ctypes.data))
    return out


def projection_is_degree(proj):
    r = load().fimex_amd_projection_is_degree(proj.encode())
    if r < 0:
        raise FimexAmdError(load().fimex_amd_last_error().decode() or "fimex_amd call failed")
    return bool(r)


def coord_nearest_host(lonPoints, latPoints, lonVals, latVals):
    """MIFI_INTERPOL_COORD_NN plan: (x index, y index) of the closest source cell per target point, -1 where none."""
    px, py = _f64(lonPoints).copy().ravel(), _f64(latPoints).copy().ravel()
    lo, la = _f64(lonVals), _f64(latVals)
    orgY, orgX = lo.shape
    _check(load().fimex_amd_coord_nearest_host(_dp(px), _dp(py), px.size, _dp(lo.reshape(-1)), _dp(la.reshape(-1)), orgX, orgY))
    return px, py


def coord_kdtree_host(maxDist, lonPoints, latPoints, lonVals, latVals):
    """MIFI_INTERPOL_COORD_NN_KD plan: closest source cell within maxDist metres, -1000 where none."""
    px, py = _f64(lonPoints).copy().ravel(), _f64(latPoints).copy().ravel()
    lo, la = _f64(lonVals), _f64(latVals)
    orgY, orgX = lo.shape
    _check(load().fimex_amd_coord_kdtree_host(maxDist, _dp(px), _dp(py), px.size, _dp(lo.reshape(-1)), _dp(la.reshape(-1)), orgX, orgY))
    return px, py


def grid_distance_host(lonVals, latVals):
    lo, la = _f64(lonVals), _f64(latVals)
    orgY, orgX = lo.shape
    out = ctypes.c_double(0)
    _check(load().fimex_amd_grid_distance_host(_dp(lo.reshape(-1)), _dp(la.reshape(-1)), orgX, orgY, ctypes.byref(out)))
    return out.value


def scan_sum_device(d_values, n, mode=0, average=0.0, algo=1, stream=0):
    """(sum, nUndefined) of the fills' scan-order double accumulation over n device floats."""
    out = ctypes.c_double(0.0)
    und = ctypes.c_size_t(0)
    _check(load().fimex_amd_scan_sum_device(d_values, n, mode, average, algo, ctypes.byref(out), ctypes.byref(und), stream))
    return out.value, und.value


def points2position_host(points, axis, axis_type=PROJ_AXIS):
    p = _f64(points).copy()
    ax = _f64(axis).ravel()
    flat = p.reshape(-1)
    _check(load().fimex_amd_points2position_host(_dp(flat), flat.size, _dp(ax), ax.size, axis_type))
    return p


def points2position_device(d_points, n, axis, axis_type=PROJ_AXIS, stream=0):
    ax = _f64(axis).ravel()
    _check(load().fimex_amd_points2position_device(d_points, n, _dp(ax), ax.size, axis_type, stream))
