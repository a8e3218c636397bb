"""ctypes binding of the C ABI declared in include/volxel_hip.h and include/volxel_brick.h.

The struct layouts are parsed from the headers so that the header stays the single source
of truth for the boundary.  Loading fails loudly when libvolxel_hip.so is missing: there is
no CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE_DIR = os.path.join(_ROOT, "include")
# VOLXEL_HIP_LIB: another build of the same library (variant probes of tools/); default: the in-tree build
LIB_PATH = os.environ.get("VOLXEL_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvolxel_hip.so")

_CTYPES = {
    "float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
    "uint64_t": C.c_uint64, "int64_t": C.c_int64,
}


def struct_from_header(header: str, name: str):
    """Build a ctypes.Structure from `typedef struct <name> { ... } <name>;` in a C header."""
    text = open(os.path.join(INCLUDE_DIR, header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    if not m:
        raise RuntimeError(f"struct {name} not found in {header}")
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        mm = re.match(r"(\w+)\s+(.*)$", decl, flags=re.S)
        ctype = _CTYPES[mm.group(1)]
        for item in mm.group(2).split(","):
            item = item.strip()
            am = re.match(r"(\w+)\s*\[(\d+)\]$", item)
            if am:
                fields.append((am.group(1), ctype * int(am.group(2))))
            else:
                fields.append((item, ctype))
    cls = type(name, (C.Structure,), {"_fields_": fields})
    _CTYPES[name] = cls   # a later struct may hold this one by value (VxIslandsResult::seg)
    return cls


VxParams = struct_from_header("volxel_hip.h", "VxParams")
VxCounters = struct_from_header("volxel_hip.h", "VxCounters")
VxSliceParams = struct_from_header("volxel_hip.h", "VxSliceParams")
VxIsoParams = struct_from_header("volxel_hip.h", "VxIsoParams")
VxSegmentParams = struct_from_header("volxel_hip.h", "VxSegmentParams")
VxSegmentResult = struct_from_header("volxel_hip.h", "VxSegmentResult")
VxSegmentEditParams = struct_from_header("volxel_hip.h", "VxSegmentEditParams")
VxIslandsParams = struct_from_header("volxel_hip.h", "VxIslandsParams")
VxIslandsResult = struct_from_header("volxel_hip.h", "VxIslandsResult")
VxIsland = struct_from_header("volxel_hip.h", "VxIsland")
VxDistanceParams = struct_from_header("volxel_hip.h", "VxDistanceParams")
VxDistanceResult = struct_from_header("volxel_hip.h", "VxDistanceResult")
VxMarginParams = struct_from_header("volxel_hip.h", "VxMarginParams")
VxCombineParams = struct_from_header("volxel_hip.h", "VxCombineParams")
VxCompareParams = struct_from_header("volxel_hip.h", "VxCompareParams")
VxCompareResult = struct_from_header("volxel_hip.h", "VxCompareResult")
VxHistogramParams = struct_from_header("volxel_hip.h", "VxHistogramParams")
VxHistogramResult = struct_from_header("volxel_hip.h", "VxHistogramResult")
VxMeshParams = struct_from_header("volxel_hip.h", "VxMeshParams")
VxMeshResult = struct_from_header("volxel_hip.h", "VxMeshResult")

MODE_DEFAULT, MODE_NO_DDA, MODE_RAYMARCH, MODE_DVR, MODE_DVR_PHONG, MODE_MIP, MODE_MINIP = range(7)
LAYOUT_REFERENCE, LAYOUT_CELLQUAD, LAYOUT_BRICKF32, LAYOUT_AUTO = 0, 1, 2, 3
RENDER_MODES = {"default": MODE_DEFAULT, "no_dda": MODE_NO_DDA, "raymarch": MODE_RAYMARCH,
                "dvr": MODE_DVR, "dvr_phong": MODE_DVR_PHONG, "mip": MODE_MIP, "minip": MODE_MINIP}
SHARD_TILE = 64
SLICE_MEAN, SLICE_MAX, SLICE_MIN = range(3)            # enum VxSliceReduce
SLICE_NONE, SLICE_GREY, SLICE_TF = range(3)            # enum VxSliceDisplay
SLICE_REDUCE = {"mean": SLICE_MEAN, "max": SLICE_MAX, "min": SLICE_MIN}
SLICE_DISPLAY = {None: SLICE_NONE, "grey": SLICE_GREY, "tf": SLICE_TF}
SLICE_MAX_SIZE, SLICE_MAX_SAMPLES = 16384, 4096
ISO_MAX_REFINE = 16
SEGEDIT_OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3, "fill_holes": 4}   # enum VxSegmentEditOp
SEGEDIT_MAX_STEPS = 1024
ISLANDS_OPS = {"label": 0, "keep_largest": 1, "remove_small": 2, "keep_at": 3}   # enum VxIslandsOp
DISTANCE_SIDES = {"outside": 0, "inside": 1}            # enum VxDistanceSide
MARGIN_OPS = {"grow": 0, "shrink": 1, "open": 2, "close": 3}   # enum VxMarginOp
SEGMENT_SLOTS = 32                                     # VX_SEGMENT_SLOTS
COMBINE_OPS = {"union": 0, "intersect": 1, "subtract": 2, "xor": 3, "invert": 4}   # enum VxCombineOp
HIST_SOURCES = {"volume": 0, "segment": 1, "slot": 2}   # enum VxHistSource
HIST_LINEAR, HIST_KEY = range(2)                       # enum VxHistRule
HIST_MAX_BINS, HIST_MAX_KEY_BITS = 4096, 12            # VX_HIST_MAX_BINS, VX_HIST_MAX_KEY_BITS
MESH_DENSITY, MESH_SEGMENT = range(2)                  # enum VxMeshSource


def declared_symbols(header: str):
    """Names of all functions a header declares (used by the symbol-export test)."""
    text = open(os.path.join(INCLUDE_DIR, header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vxb?_\w+)\s*\(", text)))


_lib = None


class VolxelLibraryMissing(RuntimeError):
    pass


def load_library():
    """Load libvolxel_hip.so (built by __graft_entry__.build() / volxel_amd/csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VolxelLibraryMissing(
            f"{LIB_PATH} is missing: build it with `make -C volxel_amd/csrc` "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so.7 /
    # libhsa-runtime64.so.1.  If torch is going to be used in this process (RCCL gather,
    # zero-copy slabs) its runtime has to be loaded FIRST so that our NEEDED libamdhip64.so.7
    # binds to the same instance; loading the system runtime first and torch's second gives
    # two HSA runtimes and torch reports "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except Exception:  # torch absent (e.g. Node host): the system ROCm runtime is used
        pass
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    P = C.POINTER
    sig = {
        "vx_create": ([i32, P(vp)], i32),
        "vx_create_group": ([P(i32), i32, P(vp)], i32),
        "vx_destroy": ([vp], None),
        "vx_last_error": ([vp], C.c_char_p),
        "vx_set_stream": ([vp, vp], i32),
        "vx_upload_volume": ([vp, vp, P(u32), vp, P(u32), vp, P(u32), i32, P(vp), vp, P(u32)], i32),
        "vx_set_layout": ([vp, i32], i32),
        "vx_upload_transfer": ([vp, vp, u32], i32),
        "vx_upload_brick_grid": ([vp, vp], i32),
        "vx_upload_environment": ([vp, vp, u32, u32], i32),
        "vx_debug_read_importance": ([vp, vp], i32),
        "vx_set_params": ([vp, P(VxParams)], i32),
        "vx_resize": ([vp, u32, u32], i32),
        "vx_render_frame": ([vp, u32, C.c_float], i32),
        "vx_render_frames": ([vp, u32, u32, P(C.c_float), i32], i32),
        "vx_finish": ([vp], i32),
        "vx_read_accum": ([vp, vp], i32),
        "vx_read_display": ([vp, vp, C.c_float, C.c_float], i32),
        "vx_read_display_scaled": ([vp, vp, u32, u32, C.c_float, C.c_float], i32),
        "vx_slab_info": ([vp, P(u64), P(u32)], i32),
        "vx_probe_tile_costs": ([vp, vp, u32], i32),
        "vx_set_tile_order": ([vp, vp, u32], i32),
        "vx_render_size": ([vp, P(u32), P(u32)], i32),
        "vx_slab_device_ptr": ([vp, P(vp)], i32),
        "vx_detile": ([vp, vp, vp], i32),
        "vx_get_counters": ([vp, P(VxCounters)], i32),
        "vx_reset_counters": ([vp], i32),
        "vx_device_info": ([vp, C.c_char_p, u32, P(u32), P(u64)], i32),
        "vx_version": ([], C.c_char_p),
        "vx_debug_unorm_table": ([vp, vp], i32),
        "vx_debug_rng": ([vp, i32, vp, vp, u32, vp], i32),
        "vx_probe_gather_rate": ([vp, u32, u32, P(C.c_double), P(u32)], i32),
        "vx_probe_gather_spread": ([vp, u32, P(u64)], i32),
        "vx_probe_valu_rate": ([vp, P(C.c_double), P(u32)], i32),
        "vx_upload_stats": ([vp, P(C.c_double), P(u64), P(i32)], i32),
        "vx_debug_build_skip_mask": ([vp, P(u32), vp, u32, P(VxParams), vp, P(u32), P(u32)], i32),
        "vx_debug_build_projection_bounds": ([vp, P(u32), P(VxParams), vp, P(u32), P(u32)], i32),
        "vx_debug_classify_miss_blocks": ([P(VxParams), u32, u32, vp, P(u32)], i32),
        "vx_debug_last_launch_blocks": ([vp, P(u32), P(u32)], i32),
        "vx_shadow_stats": ([vp, P(u64), P(u64), P(C.c_double)], i32),
        "vx_debug_read_shadow_grid": ([vp, vp, P(u32)], i32),
        "vx_slice": ([vp, P(VxSliceParams), vp, vp], i32),
        "vx_slice_stats": ([vp, P(u64), P(C.c_double)], i32),
        "vx_isosurface": ([vp, P(VxIsoParams), vp, vp], i32),
        "vx_iso_stats": ([vp, P(u64), P(u64), P(u64), P(u64), P(u64), P(C.c_double)], i32),
        "vx_segment": ([vp, P(VxSegmentParams), P(VxSegmentResult)], i32),
        "vx_segment_read_mask": ([vp, vp, u64], i32),
        "vx_slice_segment_mask": ([vp, P(VxSliceParams), vp], i32),
        "vx_segment_stats": ([vp, P(u32), P(u64), P(C.c_double)], i32),
        "vx_set_segment_view": ([vp, i32], i32),
        "vx_get_segment_view": ([vp, P(i32)], i32),
        "vx_segment_edit": ([vp, P(VxSegmentEditParams), P(VxSegmentResult)], i32),
        "vx_segment_write_mask": ([vp, vp, u64, P(VxSegmentResult)], i32),
        "vx_segment_edit_stats": ([vp, P(u32), P(C.c_double)], i32),
        "vx_segment_threshold": ([vp, P(VxSegmentParams), P(VxSegmentResult)], i32),
        "vx_segment_islands": ([vp, P(VxIslandsParams), P(VxIslandsResult)], i32),
        "vx_islands_read": ([vp, u64, u64, P(VxIsland)], i32),
        "vx_islands_read_labels": ([vp, vp, u64], i32),
        "vx_islands_stats": ([vp, P(u32), P(C.c_double)], i32),
        "vx_segment_distance": ([vp, P(VxDistanceParams), P(VxDistanceResult)], i32),
        "vx_distance_read": ([vp, vp, u64], i32),
        "vx_segment_margin": ([vp, P(VxMarginParams), P(VxSegmentResult)], i32),
        "vx_distance_stats": ([vp, P(u32), P(C.c_double)], i32),
        "vx_segment_store": ([vp, u32], i32),
        "vx_segment_load": ([vp, u32, P(VxSegmentResult)], i32),
        "vx_segment_drop": ([vp, u32], i32),
        "vx_segment_slots": ([vp, P(u32)], i32),
        "vx_segment_combine": ([vp, P(VxCombineParams), P(VxSegmentResult)], i32),
        "vx_segment_compare": ([vp, P(VxCompareParams), P(VxCompareResult)], i32),
        "vx_segments_labelmap": ([vp, P(u32), u32, vp, u64, P(u64)], i32),
        "vx_histogram": ([vp, P(VxHistogramParams), vp, u32, P(VxHistogramResult)], i32),
        "vx_histogram_stats": ([vp, P(u32), P(C.c_double)], i32),
        "vx_mesh_extract": ([vp, P(VxMeshParams), P(VxMeshResult)], i32),
        "vx_mesh_read": ([vp, vp, vp, vp], i32),
        "vx_mesh_stats": ([vp, P(u32), P(C.c_double)], i32),
        # preprocessor
        "vxb_build_from_u16": ([vp, P(u32), P(C.c_float), C.c_uint16, i32, P(vp)], i32),
        "vxb_read_dicoms_to_grid": ([P(vp), P(u64), u32, i32, P(vp)], i32),
        "vxb_free": ([vp], None),
        "vxb_last_error": ([], C.c_char_p),
        "vxb_indirection_size": ([vp, P(u32)], None),
        "vxb_range_size": ([vp, P(u32)], None),
        "vxb_atlas_size": ([vp, P(u32)], None),
        "vxb_indirection_data": ([vp], vp),
        "vxb_range_data": ([vp], vp),
        "vxb_atlas_data": ([vp], vp),
        "vxb_range_mipmaps": ([vp], u32),
        "vxb_range_mipmap": ([vp, u32], vp),
        "vxb_range_mipmap_stride": ([vp, u32, P(u32)], None),
        "vxb_transform": ([vp, P(C.c_float)], None),
        "vxb_minorant": ([vp], C.c_float),
        "vxb_majorant": ([vp], C.c_float),
        "vxb_index_extent": ([vp, P(u32)], None),
        "vxb_histogram_len": ([vp], u32),
        "vxb_histogram": ([vp], vp),
        "vxb_histogram_gradient": ([vp], vp),
        "vxb_histogram_gradient_min": ([vp], u32),
        "vxb_histogram_gradient_max": ([vp], u32),
        "vxb_brick_counter": ([vp], u32),
        "vxb_lookup": ([vp, u32, u32, u32], C.c_float),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib
