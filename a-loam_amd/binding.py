"""ctypes binding of libaloam_mi355x.so (include/aloam_mi355x.h) for tests and bench.

This is NOT a second implementation: every method is one C-ABI call.  The library itself refuses to work
without a HIP device (ALOAM_E_HIP); loading it and listing its symbols is possible on a CPU-only box.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

from .records import *  # noqa: F401,F403  the records, their dtypes and the enumerators of the header: declared there, used under these names
from .joint_records import AloamGraphJointGroup, AloamGraphLink, GRAPH_JOINT_GROUP_DTYPE, GRAPH_LINK_DTYPE  # noqa: F401  the records of the joined graphs
from .link_records import AloamGraphLinkRequest, GRAPH_LINK_REQUEST_DTYPE  # noqa: F401  the record of the links measured on the device
from .map_joint_records import AloamGraphMapGroup, AloamGraphMapPart, GRAPH_MAP_GROUP_DTYPE, GRAPH_MAP_PART_DTYPE  # noqa: F401  the records of the map of joined sequences

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "lib", "libaloam_mi355x.so")
HEADER_PATH = os.path.join(_ROOT, "include", "aloam_mi355x.h")

MAP_INFO_KEYS = ("cenW", "cenH", "cenD", "frame_count", "from_map_corner", "from_map_surf", "corner_stack", "surf_stack",
                 "corner_num0", "corner_num1", "surf_num0", "surf_num1", "lm_iterations0", "lm_iterations1", "termination0", "compactions")


class AloamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"aloam error {code}: {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 with csrc/Makefile (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir)] + [HEADER_PATH]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        r = subprocess.run(["make", "-j4", "-C", src_dir], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc build failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


def declared_symbols() -> list[str]:
    """Every function include/aloam_mi355x.h declares."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(aloam_[a-z_0-9]+)\s*\(", txt)))


_lib = None


def lib():
    """Load the shared library; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc) first; there is no CPU fallback")
        # PyTorch-ROCm wheels bundle their own libamdhip64; if this process loads the system HIP runtime first (through
        # libaloam_mi355x.so) and torch afterwards, torch's copy finds no device.  Loading torch first makes both use one runtime.
        # The C library itself has no torch dependency; this only concerns Python processes that use both.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(os.environ.get("ALOAM_MI355X_LIB", LIB_PATH))   # override: A/B runs of two builds of the same library
        vp, ip = C.c_void_p, C.POINTER(C.c_int)
        L.aloam_default_config.argtypes = [C.POINTER(AloamConfig)]; L.aloam_default_config.restype = None
        L.aloam_create.argtypes = [C.POINTER(AloamConfig), C.POINTER(vp)]
        L.aloam_create_stages.argtypes = [C.POINTER(AloamConfig), C.c_int, C.POINTER(vp)]
        L.aloam_destroy.argtypes = [vp]; L.aloam_destroy.restype = None
        L.aloam_last_error.argtypes = [vp]; L.aloam_last_error.restype = C.c_char_p
        L.aloam_stream.argtypes = [vp]; L.aloam_stream.restype = vp
        L.aloam_synchronize.argtypes = [vp]
        L.aloam_set_voxel_sum_order.argtypes = [vp, C.c_int]
        L.aloam_scan_register.argtypes = [vp, C.POINTER(vp), ip, C.c_int]
        L.aloam_scan_register_device.argtypes = [vp, vp, C.c_longlong, ip, C.c_int]
        L.aloam_scan_register_host.argtypes = [vp, vp, C.c_longlong, ip, C.c_int]
        L.aloam_process_host.argtypes = [vp, vp, C.c_longlong, ip, C.c_int]
        L.aloam_input_consumed.argtypes = [vp]
        L.aloam_odometry_step.argtypes = [vp]
        L.aloam_process_device.argtypes = [vp, vp, C.c_longlong, ip, C.c_int]
        L.aloam_set_range_decoder.argtypes = [vp, C.POINTER(AloamRangeDecoder)]
        L.aloam_scan_register_range_device.argtypes = [vp, vp, C.c_longlong, ip]
        L.aloam_scan_register_range_host.argtypes = [vp, vp, C.c_longlong, ip]
        L.aloam_process_range_device.argtypes = [vp, vp, C.c_longlong, ip]
        L.aloam_process_range_host.argtypes = [vp, vp, C.c_longlong, ip]
        L.aloam_cloud_size.argtypes = [vp, C.c_int, C.c_int]
        L.aloam_get_cloud.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
        L.aloam_get_pose.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.aloam_get_odom_stats.argtypes = [vp, C.c_int, C.POINTER(AloamOdomStats)]
        L.aloam_set_features.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int]
        L.aloam_set_last.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int]
        L.aloam_set_state.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.aloam_set_system_inited.argtypes = [vp, C.c_int]
        L.aloam_set_active.argtypes = [vp, vp]
        L.aloam_reset_sequences.argtypes = [vp, vp, C.c_int]
        L.aloam_set_map_frozen.argtypes = [vp, vp]
        L.aloam_score_map_corrections.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp]
        L.aloam_apply_map_corrections.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
        L.aloam_map_spill_enable.argtypes = [vp, C.c_int, C.c_int]
        L.aloam_export_map_spill.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, vp, C.c_longlong, vp, C.c_int]
        L.aloam_get_map_spill_info.argtypes = [vp, C.c_int, vp]
        L.aloam_atlas_load.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong]
        L.aloam_atlas_attach.argtypes = [vp, vp]
        L.aloam_atlas_info.argtypes = [vp, vp]
        L.aloam_places_enable.argtypes = [vp, C.c_int, C.c_float, C.c_float]
        L.aloam_places_add.argtypes = [vp, vp, C.c_int]
        L.aloam_places_match.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
        L.aloam_places_export.argtypes = [vp, C.c_int, C.c_int, vp]
        L.aloam_places_load.argtypes = [vp, vp, C.c_int]
        L.aloam_places_clear.argtypes = [vp]
        L.aloam_places_info.argtypes = [vp, vp]
        L.aloam_save_sequences.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, vp]
        L.aloam_load_sequences.argtypes = [vp, vp, C.c_int, vp, vp]
        L.aloam_get_ring_ranges.argtypes = [vp, C.c_int, vp, vp]
        L.aloam_get_curvature.argtypes = [vp, C.c_int, vp, C.c_int]
        L.aloam_get_labels.argtypes = [vp, C.c_int, vp, C.c_int]
        L.aloam_get_last_cloud_order.argtypes = [vp, C.c_int, vp]
        if hasattr(L, "aloam_get_solve_lds"):              # absent from an A/B variant built from an older tree (ALOAM_MI355X_LIB)
            L.aloam_get_solve_lds.argtypes = [vp, vp]
        L.aloam_get_correspondences.argtypes = [vp, C.c_int, vp, C.c_int, ip, vp, vp, C.c_int, ip, vp]
        L.aloam_mapping_enable.argtypes = [vp, C.c_float, C.c_float, C.c_int]
        L.aloam_mapping_step.argtypes = [vp]
        L.aloam_mapping_set_pool_limit.argtypes = [vp, C.c_int]
        L.aloam_get_map_pool_info.argtypes = [vp, vp]
        L.aloam_set_map.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]
        L.aloam_set_map_frame.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int]
        L.aloam_set_full_cloud.argtypes = [vp, C.c_int, vp, C.c_int]
        L.aloam_get_map_pose.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.aloam_get_map_info.argtypes = [vp, C.c_int, vp]
        L.aloam_map_cube_counts.argtypes = [vp, C.c_int, C.c_int, vp]
        L.aloam_get_map_cube.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int]
        L.aloam_get_map_cloud.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
        L.aloam_export_poses.argtypes = [vp, vp]
        L.aloam_export_clouds.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, vp]
        L.aloam_export_pose_information.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        L.aloam_get_map_factors.argtypes = [vp, C.c_int, vp, C.c_int, ip, vp, C.c_int, ip]
        L.aloam_graph_default_options.argtypes = [C.POINTER(AloamGraphOptions)]; L.aloam_graph_default_options.restype = None
        L.aloam_graph_enable.argtypes = [vp, C.c_int, C.c_int]
        L.aloam_graph_add_nodes.argtypes = [vp, vp, C.c_int, vp]
        L.aloam_graph_add_edges.argtypes = [vp, vp, C.c_int]
        L.aloam_graph_export.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        L.aloam_graph_export_edges.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        L.aloam_graph_clear.argtypes = [vp, vp, C.c_int]
        L.aloam_graph_info.argtypes = [vp, C.c_int, vp]
        L.aloam_graph_optimize.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphOptions), vp]
        L.aloam_graph_keyframes_enable.argtypes = [vp, C.c_int, C.c_int]
        L.aloam_graph_export_keyframes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_longlong, vp]
        L.aloam_graph_keyframe_info.argtypes = [vp, C.c_int, vp]
        L.aloam_graph_export_map.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, vp, C.c_longlong, vp, vp]
        L.aloam_graph_apply.argtypes = [vp, vp, C.c_int, vp]
        L.aloam_graph_loop_default_options.argtypes = [C.POINTER(AloamGraphLoopOptions)]; L.aloam_graph_loop_default_options.restype = None
        L.aloam_graph_loops_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.aloam_graph_register_loops.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphLoopOptions), vp]
        L.aloam_graph_loop_export_target.argtypes = [vp, C.c_int, C.c_int, vp, C.c_longlong, vp]
        L.aloam_graph_loop_default_search.argtypes = [C.POINTER(AloamGraphLoopSearch)]; L.aloam_graph_loop_default_search.restype = None
        L.aloam_graph_search_loops.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphLoopSearch), C.POINTER(AloamGraphLoopOptions), vp, vp, vp]
        L.aloam_graph_marginal_default_options.argtypes = [C.POINTER(AloamGraphMarginalOptions)]; L.aloam_graph_marginal_default_options.restype = None
        L.aloam_graph_marginals.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphMarginalOptions), vp]
        L.aloam_graph_robust_default_options.argtypes = [C.POINTER(AloamGraphRobustOptions)]; L.aloam_graph_robust_default_options.restype = None
        L.aloam_graph_optimize_robust.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphOptions), C.POINTER(AloamGraphRobustOptions), vp, vp, C.c_longlong]
        if hasattr(L, "aloam_graph_propose_loops"):        # absent from an A/B variant built from an older tree (ALOAM_MI355X_LIB)
            L.aloam_graph_propose_loops.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        if hasattr(L, "aloam_graph_trim"):                 # likewise
            L.aloam_graph_trim.argtypes = [vp, vp, vp, C.c_int, vp]
        if hasattr(L, "aloam_graph_optimize_joint"):       # likewise
            L.aloam_graph_optimize_joint.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(AloamGraphOptions), vp]
            L.aloam_graph_optimize_joint_robust.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(AloamGraphOptions),
                                                            C.POINTER(AloamGraphRobustOptions), vp, vp, C.c_longlong]
            L.aloam_graph_joint_export.argtypes = [vp, C.c_int, vp, C.c_longlong, vp, C.c_longlong, vp]
        if hasattr(L, "aloam_graph_register_links"):       # likewise
            L.aloam_graph_register_links.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphLoopOptions), vp]
            L.aloam_graph_search_links.argtypes = [vp, vp, C.c_int, C.POINTER(AloamGraphLoopSearch), C.POINTER(AloamGraphLoopOptions), vp, vp, vp]
            L.aloam_graph_propose_links.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        if hasattr(L, "aloam_graph_export_map_joint"):     # likewise
            L.aloam_graph_export_map_joint.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_longlong, vp, C.c_longlong, vp, vp]
        L.aloam_graph_save.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, vp]
        L.aloam_graph_load.argtypes = [vp, vp, C.c_int, vp, vp]
        L.aloam_profile_enable.argtypes = [vp, C.c_int]
        L.aloam_profile_kernel_count.argtypes = []
        L.aloam_profile_kernel_name.argtypes = [C.c_int]; L.aloam_profile_kernel_name.restype = C.c_char_p
        L.aloam_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _vp(x):
    """An address as a pointer argument; 0 is NULL."""
    return C.c_void_p(x) if x else None


def _ids(seqs):
    return np.ascontiguousarray([int(v) for v in seqs], dtype=np.int32)


def _ids_arg(ids):
    return _p(ids) if len(ids) else None


def _where(pinned):
    """Where a destination is allocated (torch's keywords): pinned host memory, or this process's device."""
    return {"pin_memory": True} if pinned else {"device": "cuda"}


def _out_bytes(n, dtype, pinned):
    """Zeroed room for n records (for one where n is 0): a uint8 tensor in pinned host memory, or on the device."""
    import torch
    return torch.zeros(max(1, n) * dtype.itemsize, dtype=torch.uint8, **_where(pinned))


def _records(buf, n, dtype):
    """The first n records of such a buffer as a structured array of the host's own."""
    return buf.cpu().numpy()[:n * dtype.itemsize].view(dtype).copy()


def _options(cls, default_fn, kw):
    """The library's defaults of an options record with the fields of kw replaced."""
    o = cls()
    default_fn(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


class Aloam:
    """`batch` independent sequences on one MI355X.  Method names mirror the oracle binding so parity tests read
    `gpu.scan_register(x)` next to `oracle.scan_register(x)`."""

    def __init__(self, n_scans=64, min_range=5.0, ring_from_field=False, batch=1, max_points=140000, max_ring_points=4107,
                 device=0, lm_max_iterations=4, outer_iterations=2, distortion=False, stages=STAGE_ALL):
        L = lib()
        cfg = AloamConfig()
        L.aloam_default_config(C.byref(cfg))
        cfg.n_scans, cfg.min_range, cfg.ring_from_field, cfg.batch = n_scans, min_range, int(ring_from_field), batch
        cfg.max_points, cfg.max_ring_points, cfg.device = max_points, max_ring_points, device
        cfg.lm_max_iterations, cfg.outer_iterations = lm_max_iterations, outer_iterations
        cfg.distortion = int(distortion)
        self.cfg, self.batch, self.n_scans, self.max_points = cfg, batch, n_scans, max_points
        h = C.c_void_p()
        rc = L.aloam_create_stages(C.byref(cfg), int(stages), C.byref(h))
        self.h = h
        if rc != 0:
            msg = L.aloam_last_error(h).decode() if h else "allocation failed"
            if h:
                L.aloam_destroy(h)
            self.h = None
            raise AloamError(rc, msg)

    def set_voxel_sum_order(self, reference_order=True):
        """True: pcl::VoxelGrid's own summation order (libstdc++ std::sort replayed; validation mode); False: input order (default)."""
        self._check(lib().aloam_set_voxel_sum_order(self.h, 1 if reference_order else 0))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.aloam_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise AloamError(rc, lib().aloam_last_error(self.h).decode())
        return rc

    # ---- stage 1 -------------------------------------------------------------------------------------------
    def scan_register(self, scans, check=True):
        """scans: one float32 [N,>=3] array per sequence (or a single array when batch == 1)."""
        if isinstance(scans, np.ndarray) and scans.ndim == 2:
            scans = [scans]
        assert len(scans) == self.batch
        arrs = [_f32(s) for s in scans]
        stride = arrs[0].strides[0] if arrs[0].shape[0] else 4 * arrs[0].shape[1]
        assert all(a.ndim == 2 and a.shape[1] >= 3 and (a.shape[0] == 0 or a.strides[0] == stride) for a in arrs)   # 3 columns = the 12-byte x y z wire format
        ptrs = (C.c_void_p * self.batch)(*[a.ctypes.data for a in arrs])
        nin = (C.c_int * self.batch)(*[a.shape[0] for a in arrs])
        self._check(lib().aloam_scan_register(self.h, ptrs, nin, stride))
        if check:
            self.synchronize()

    def scan_register_device(self, d_ptr, seq_stride_bytes, n_in, stride_bytes=16):
        nin = (C.c_int * self.batch)(*[int(v) for v in n_in])
        self._check(lib().aloam_scan_register_device(self.h, C.c_void_p(d_ptr), seq_stride_bytes, nin, stride_bytes))

    def process_device(self, d_ptr, seq_stride_bytes, n_in, stride_bytes=16):
        nin = n_in if isinstance(n_in, C.Array) else (C.c_int * self.batch)(*[int(v) for v in n_in])
        self._check(lib().aloam_process_device(self.h, C.c_void_p(d_ptr), seq_stride_bytes, nin, stride_bytes))

    def process_host(self, h_ptr, seq_stride_bytes, n_in, stride_bytes=16):
        """One host-resident batch (pinned for true asynchrony): batched H2D copy on the copy stream + stage 1 + stage 2."""
        nin = n_in if isinstance(n_in, C.Array) else (C.c_int * self.batch)(*[int(v) for v in n_in])
        self._check(lib().aloam_process_host(self.h, C.c_void_p(h_ptr), seq_stride_bytes, nin, stride_bytes))

    def scan_register_host(self, h_ptr, seq_stride_bytes, n_in, stride_bytes=16):
        nin = n_in if isinstance(n_in, C.Array) else (C.c_int * self.batch)(*[int(v) for v in n_in])
        self._check(lib().aloam_scan_register_host(self.h, C.c_void_p(h_ptr), seq_stride_bytes, nin, stride_bytes))

    # ---- stage 1 from 16-bit range images (a-loam_amd/range_input.py) ---------------------------------------------------------------
    def set_range_decoder(self, dec):
        """dec: a range_input.RangeDecoder, or an AloamRangeDecoder struct as it is (the error tests hand in broken ones)."""
        d = dec if isinstance(dec, AloamRangeDecoder) else range_decoder_struct(dec)[0]
        self._check(lib().aloam_set_range_decoder(self.h, C.byref(d)))

    def _ncols(self, n_cols):
        return n_cols if isinstance(n_cols, C.Array) else (C.c_int * self.batch)(*[int(v) for v in n_cols])

    def scan_register_range(self, blobs, n_cols, check=True):
        """blobs: one uint16 array per sequence (range_input.pack_sweep), from pageable memory; waits for the input to be consumed."""
        arrs = [np.ascontiguousarray(b, dtype=np.uint16).reshape(-1) for b in blobs]
        assert len(arrs) == self.batch
        stride = max(16, max(a.nbytes for a in arrs))
        buf = np.zeros(self.batch * stride, np.uint8)
        for b, a in enumerate(arrs):
            buf[b * stride:b * stride + a.nbytes] = a.view(np.uint8)
        self.scan_register_range_host(buf.ctypes.data, stride, n_cols)
        self.input_consumed()
        if check:
            self.synchronize()

    def scan_register_range_device(self, d_ptr, seq_stride_bytes, n_cols):
        self._check(lib().aloam_scan_register_range_device(self.h, C.c_void_p(d_ptr), seq_stride_bytes, self._ncols(n_cols)))

    def scan_register_range_host(self, h_ptr, seq_stride_bytes, n_cols):
        self._check(lib().aloam_scan_register_range_host(self.h, C.c_void_p(h_ptr), seq_stride_bytes, self._ncols(n_cols)))

    def process_range_device(self, d_ptr, seq_stride_bytes, n_cols):
        self._check(lib().aloam_process_range_device(self.h, C.c_void_p(d_ptr), seq_stride_bytes, self._ncols(n_cols)))

    def process_range_host(self, h_ptr, seq_stride_bytes, n_cols):
        """One host-resident batch of range images (pinned for true asynchrony): batched H2D copy on the copy stream + stage 1 + stage 2."""
        self._check(lib().aloam_process_range_host(self.h, C.c_void_p(h_ptr), seq_stride_bytes, self._ncols(n_cols)))

    def input_consumed(self):
        self._check(lib().aloam_input_consumed(self.h))

    def synchronize(self):
        rc = lib().aloam_synchronize(self.h)
        self._apply_keep = []                                 # (the stream has drained: the device has read every choice buffer)
        self._check(rc)

    def cloud(self, which, seq=0):
        n = self._check(lib().aloam_cloud_size(self.h, seq, which))
        out = np.zeros((n, 4), np.float32)
        self._check(lib().aloam_get_cloud(self.h, seq, which, _p(out), n))
        return out

    def features(self, seq=0):
        return {"cloud": self.cloud(CLOUD_FULL, seq), "sharp": self.cloud(CLOUD_SHARP, seq), "less_sharp": self.cloud(CLOUD_LESS_SHARP, seq),
                "flat": self.cloud(CLOUD_FLAT, seq), "less_flat": self.cloud(CLOUD_LESS_FLAT, seq)}

    def ring_ranges(self, seq=0):
        s = np.zeros(self.n_scans, np.int32); c = np.zeros(self.n_scans, np.int32)
        self._check(lib().aloam_get_ring_ranges(self.h, seq, _p(s), _p(c)))
        return s, c

    def per_point(self, seq=0):
        n = self._check(lib().aloam_cloud_size(self.h, seq, CLOUD_FULL))
        curv = np.zeros(n, np.float32); lab = np.zeros(n, np.int32)
        self._check(lib().aloam_get_curvature(self.h, seq, _p(curv), n))
        self._check(lib().aloam_get_labels(self.h, seq, _p(lab), n))
        return curv, lab

    # ---- stage 2 -------------------------------------------------------------------------------------------
    def set_features(self, f, seq=0):
        a = [_f32(f[k]) for k in ("sharp", "less_sharp", "flat", "less_flat")]
        self._check(lib().aloam_set_features(self.h, seq, _p(a[0]), len(a[0]), _p(a[1]), len(a[1]), _p(a[2]), len(a[2]), _p(a[3]), len(a[3])))

    def set_last(self, corner_last, surf_last, seq=0):
        a, b = _f32(corner_last), _f32(surf_last)
        self._check(lib().aloam_set_last(self.h, seq, _p(a), len(a), _p(b), len(b)))

    def set_state(self, para_q, para_t, q_w=(0, 0, 0, 1), t_w=(0, 0, 0), seq=0, inited=True):
        a, b, c, d = _f64(para_q), _f64(para_t), _f64(q_w), _f64(t_w)
        self._check(lib().aloam_set_state(self.h, seq, _p(a), _p(b), _p(c), _p(d)))
        self._check(lib().aloam_set_system_inited(self.h, int(inited)))

    # ---- per-sequence lifecycle ---------------------------------------------------------------------------------
    def set_active(self, mask=None):
        """Which sequences take part in the calls that follow (one truthy value per sequence); None = all of them."""
        if mask is None:
            self._check(lib().aloam_set_active(self.h, None))
            return
        m = np.ascontiguousarray([1 if v else 0 for v in mask], dtype=np.int32)
        assert m.shape == (self.batch,)
        self._check(lib().aloam_set_active(self.h, _p(m)))

    def reset_sequences(self, seqs):
        """Put the listed sequences back to the state of a fresh context, in stream order (no synchronisation)."""
        ids = _ids(seqs)
        self._check(lib().aloam_reset_sequences(self.h, _ids_arg(ids), len(ids)))

    def set_map_frozen(self, mask=None):
        """Which sequences localize against their map instead of extending it in the mapping steps that follow (one truthy value per
        sequence); None = none of them."""
        if mask is None:
            self._check(lib().aloam_set_map_frozen(self.h, None))
            return
        m = np.ascontiguousarray([1 if v else 0 for v in mask], dtype=np.int32)
        assert m.shape == (self.batch,)
        self._check(lib().aloam_set_map_frozen(self.h, _p(m)))

    # ---- map-pose hypotheses (stream-ordered; wait with synchronize()) --------------------------------------------------------------
    def score_map_corrections_into(self, seqs, cand_ptr, K, scores_ptr, best_ptr=0):
        """Queue the scoring of the K candidates at cand_ptr (device, pinned or pageable host memory) for `seqs`; scores_ptr receives
        len(seqs) * K aloam_map_score records, best_ptr (0 = not wanted) len(seqs) int32 - both device memory or pinned host memory."""
        ids = _ids(seqs)
        self._check(lib().aloam_score_map_corrections(self.h, _ids_arg(ids), len(ids), _vp(cand_ptr), int(K), _vp(scores_ptr), _vp(best_ptr)))

    def score_map_corrections(self, seqs, cand, pinned=True):
        """Scores of the candidates `cand` (structured array of MAP_CORRECTION_DTYPE, see map_corrections) for `seqs`, after a synchronise.
        Returns (scores, best): a structured array [len(seqs), K] of MAP_SCORE_DTYPE and int32 [len(seqs)]; with pinned=False the
        destinations are device memory, copied back afterwards."""
        import torch
        cand = np.ascontiguousarray(cand, dtype=MAP_CORRECTION_DTYPE)
        n, K = len(seqs), len(cand)
        sc = _out_bytes(n * K, MAP_SCORE_DTYPE, pinned)
        best = torch.zeros(max(1, n), dtype=torch.int32, **_where(pinned))
        self.score_map_corrections_into(seqs, cand.ctypes.data, K, sc.data_ptr(), best.data_ptr())
        self.synchronize()
        return _records(sc, n * K, MAP_SCORE_DTYPE).reshape(n, K), best.cpu().numpy()[:n].copy()

    def apply_map_corrections_from(self, seqs, cand_ptr, K, choice_ptr):
        """Queue q_wmap_wodom, t_wmap_wodom := cand[choice[i]] for seqs[i]; choice_ptr: int32 in device memory or pinned host memory, read
        on the device in stream order (the `best` of a scoring call queued before this one may be passed straight in)."""
        ids = _ids(seqs)
        self._check(lib().aloam_apply_map_corrections(self.h, _ids_arg(ids), len(ids), _vp(cand_ptr), int(K), _vp(choice_ptr)))

    def apply_map_corrections(self, seqs, cand, choice):
        """Install cand[choice[i]] as the correction of seqs[i] (choice: one int per listed sequence), in stream order."""
        import torch
        cand = np.ascontiguousarray(cand, dtype=MAP_CORRECTION_DTYPE)
        ch = torch.tensor([int(v) for v in choice], dtype=torch.int32).pin_memory() if len(seqs) else torch.zeros(1, dtype=torch.int32).pin_memory()
        self._apply_keep = getattr(self, "_apply_keep", []) + [ch]   # read by the device later: kept until the next synchronize()
        self.apply_map_corrections_from(seqs, cand.ctypes.data, len(cand), ch.data_ptr())

    # ---- map spill: the cubes that leave the window (stream-ordered; wait with synchronize()) -------------------------------------
    def map_spill_enable(self, max_tiles, max_points):
        """Keep what the window shifts of the mapping steps empty: per sequence and class up to max_tiles tiles / max_points points."""
        self._check(lib().aloam_map_spill_enable(self.h, int(max_tiles), int(max_points)))

    def export_map_spill_into(self, seqs, tiles_ptr, cap_tiles, points_ptr, cap_points, offsets_ptr, clear=True):
        """Queue the drain of the spills of `seqs`: tiles_ptr receives up to cap_tiles aloam_map_tile records, points_ptr up to cap_points
        float4 points, offsets_ptr 2 * (len(seqs) + 1) int64 (tile offsets, then point offsets) - device memory or pinned host memory; 0
        pointers with caps of 0 = the size query.  clear: empty the sequences that were written."""
        ids = _ids(seqs)
        self._check(lib().aloam_export_map_spill(self.h, _ids_arg(ids), len(ids), _vp(tiles_ptr), int(cap_tiles), _vp(points_ptr), int(cap_points),
                                                 _vp(offsets_ptr), 1 if clear else 0))

    def export_map_spill(self, seqs, clear=True, pinned=True):
        """The spills of `seqs`: a size query, one allocation (pinned host memory, or device memory with pinned=False), the drain and a
        synchronise.  Returns (tiles, points, offsets): a structured array of MAP_TILE_DTYPE, float32 [n, 4] and int64 [2, len(seqs) + 1]."""
        import torch
        n = len(seqs)
        off = torch.zeros(2 * (n + 1), dtype=torch.int64, pin_memory=True)
        self.export_map_spill_into(seqs, 0, 0, 0, 0, off.data_ptr(), clear=False)
        self.synchronize()
        nt, npts = int(off[n]), int(off[2 * n + 1])
        tiles = _out_bytes(nt, MAP_TILE_DTYPE, pinned)
        pts = torch.zeros((max(1, npts), 4), dtype=torch.float32, **_where(pinned))
        self.export_map_spill_into(seqs, tiles.data_ptr(), nt, pts.data_ptr(), npts, off.data_ptr(), clear=clear)
        self.synchronize()
        return (_records(tiles, nt, MAP_TILE_DTYPE), pts.cpu().numpy()[:npts].copy(), off.numpy().reshape(2, n + 1).copy())

    def map_spill_info(self, seq=0):
        v = np.zeros(8, np.int32)
        self._check(lib().aloam_get_map_spill_info(self.h, seq, _p(v)))
        return {"tiles": v[0:2].tolist(), "points": v[2:4].tolist(), "dropped_tiles": int(v[4]), "dropped_points": int(v[5]),
                "max_tiles": int(v[6]), "max_points": int(v[7])}

    # ---- the atlas: one tile store per context, shared by the attached (frozen) sequences ---------------------------------------------
    def atlas_load(self, tiles, points):
        """tiles: structured array of MAP_TILE_DTYPE, points: (n, 4) float32 - numpy arrays, or torch tensors on this device (tiles as
        uint8).  Synchronous.  No tiles = unload."""
        if hasattr(tiles, "data_ptr"):
            nt, npts, tp, pp = tiles.numel() // 32, points.shape[0], tiles.data_ptr(), points.data_ptr()
        else:
            tiles, points = np.ascontiguousarray(tiles, dtype=MAP_TILE_DTYPE), _f32(np.asarray(points).reshape(-1, 4))
            nt, npts, tp, pp = len(tiles), len(points), tiles.ctypes.data, points.ctypes.data
        self._check(lib().aloam_atlas_load(self.h, C.c_void_p(tp) if nt else None, nt, C.c_void_p(pp) if npts else None, npts))

    def atlas_attach(self, mask=None):
        """Which sequences take their window from the atlas (one truthy value per sequence); None = none."""
        if mask is None:
            self._check(lib().aloam_atlas_attach(self.h, None))
            return
        m = np.ascontiguousarray([1 if v else 0 for v in mask], dtype=np.int32)
        assert m.shape == (self.batch,)
        self._check(lib().aloam_atlas_attach(self.h, _p(m)))

    def atlas_info(self):
        v = np.zeros(12, np.int64)
        self._check(lib().aloam_atlas_info(self.h, _p(v)))
        return {"tiles": int(v[0]), "cubes": v[1:3].tolist(), "points": v[3:5].tolist(), "extent": v[5:8].tolist(), "largest_window": v[8:10].tolist(),
                "exact": bool(v[10]), "device_bytes": int(v[11])}

    # ---- place recognition (stream-ordered; wait with synchronize()) -------------------------------------------------------------------
    def places_enable(self, capacity, max_range=80.0, sensor_height=2.0):
        """One place store of `capacity` entries for this context, and one scan-context descriptor per sequence (made on first use)."""
        self._check(lib().aloam_places_enable(self.h, int(capacity), float(max_range), float(sensor_height)))

    def places_add(self, seqs):
        """Append the place of each listed sequence (descriptor of the sweep it holds + its pose at this point of the stream).  Returns the
        store index of the first one; the others follow in listed order."""
        ids = _ids(seqs)
        first = self.places_info()["count"]
        self._check(lib().aloam_places_add(self.h, _ids_arg(ids), len(ids)))
        return first

    def places_match_into(self, seqs, ranges, T, dst_ptr):
        """Queue the match of the listed sequences' descriptors, each against the store entries [ranges[i][0], ranges[i][1]); dst_ptr
        receives len(seqs) * T aloam_place_match records (device memory or pinned host memory)."""
        ids = _ids(seqs)
        rg = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
        assert len(rg) == len(ids)
        self._check(lib().aloam_places_match(self.h, _ids_arg(ids), len(ids), _p(rg) if len(ids) else None, int(T), _vp(dst_ptr)))

    def places_match(self, seqs, ranges=None, T=1, pinned=True):
        """The T best stored places for each listed sequence, after a synchronise: a structured array [len(seqs), T] of PLACE_MATCH_DTYPE.
        ranges: one (lo, hi) per sequence, or None = the whole store."""
        n = len(seqs)
        if ranges is None:
            ranges = [(0, self.places_info()["count"])] * n
        dst = _out_bytes(n * T, PLACE_MATCH_DTYPE, pinned)
        self.places_match_into(seqs, ranges, T, dst.data_ptr())
        self.synchronize()
        return _records(dst, n * T, PLACE_MATCH_DTYPE).reshape(n, T)

    def places_export_into(self, first, count, dst_ptr):
        self._check(lib().aloam_places_export(self.h, int(first), int(count), _vp(dst_ptr)))

    def places_export(self, first=0, count=None, pinned=True):
        """Store entries [first, first + count) (default: all that follow first) as a structured array of PLACE_DTYPE, after a synchronise."""
        if count is None:
            count = self.places_info()["count"] - first
        dst = _out_bytes(count, PLACE_DTYPE, pinned)
        self.places_export_into(first, count, dst.data_ptr())
        self.synchronize()
        return _records(dst, count, PLACE_DTYPE)

    def places_load(self, places):
        """Append stored places: a structured array of PLACE_DTYPE (pageable host memory), or a torch uint8 tensor on this device or pinned.
        Returns the store index of the first one.  The source is kept referenced until the next load (the copy is stream-ordered)."""
        first = self.places_info()["count"]
        if hasattr(places, "data_ptr"):
            n, ptr = places.numel() // PLACE_DTYPE.itemsize, places.data_ptr()
        else:
            places = np.ascontiguousarray(places, dtype=PLACE_DTYPE)
            n, ptr = len(places), places.ctypes.data
        self._places_keep = places
        self._check(lib().aloam_places_load(self.h, C.c_void_p(ptr) if n else None, n))
        return first

    def places_clear(self):
        self._check(lib().aloam_places_clear(self.h))

    def places_info(self):
        v = np.zeros(4, np.int32)
        self._check(lib().aloam_places_info(self.h, _p(v)))
        return {"count": int(v[0]), "capacity": int(v[1]), "max_range": float(v[2:3].view(np.float32)[0]), "sensor_height": float(v[3:4].view(np.float32)[0])}

    # ---- pose graphs (stream-ordered; a-loam_amd/posegraph.py holds the definitions) -------------------------------------------------------
    def graph_enable(self, max_nodes, max_edges):
        """One pose graph per sequence: rows of max_nodes nodes and max_edges edges (odometry edges included)."""
        self._check(lib().aloam_graph_enable(self.h, int(max_nodes), int(max_edges)))

    def graph_add_nodes(self, seqs, odom_info):
        """Enter the pose each listed sequence holds at this point of the stream as its next node; odom_info: one 6 x 6 information (or its
        21-element upper triangle) for all, or one per sequence, for the odometry edge to the node before.  Returns the new nodes' indices."""
        ids = _ids(seqs)
        info = np.asarray(odom_info, dtype=np.float64)
        if info.shape[-2:] == (6, 6):
            info = info[..., np.triu_indices(6)[0], np.triu_indices(6)[1]]
        info = np.ascontiguousarray(np.broadcast_to(info, (len(ids), 21)))
        index = [self.graph_info(int(b))["nodes"] for b in ids]
        self._check(lib().aloam_graph_add_nodes(self.h, _ids_arg(ids), len(ids), _p(info) if len(ids) else None))
        return index

    def graph_add_edges(self, edges):
        """edges: a structured array of GRAPH_EDGE_DTYPE (posegraph.make_edges builds one)."""
        e = np.ascontiguousarray(edges, dtype=GRAPH_EDGE_DTYPE)
        self._check(lib().aloam_graph_add_edges(self.h, _p(e) if len(e) else None, len(e)))

    def graph_options(self, **kw):
        return _options(AloamGraphOptions, lib().aloam_graph_default_options, kw)

    def graph_optimize_into(self, seqs, dst_ptr, options=None):
        """Queue the solve of the listed sequences' graphs; dst_ptr receives one aloam_graph_result each (device or pinned memory)."""
        ids = _ids(seqs)
        self._check(lib().aloam_graph_optimize(self.h, _ids_arg(ids), len(ids), C.byref(options) if options is not None else None, _vp(dst_ptr)))

    def graph_optimize(self, seqs, pinned=True, **options):
        """Solve and wait: a structured array [len(seqs)] of GRAPH_RESULT_DTYPE.  Keyword arguments are fields of aloam_graph_options."""
        buf = _out_bytes(len(seqs), GRAPH_RESULT_DTYPE, pinned)
        self.graph_optimize_into(seqs, buf.data_ptr(), self.graph_options(**options))
        self.synchronize()
        return _records(buf, len(seqs), GRAPH_RESULT_DTYPE)

    def graph_export_into(self, seq, first, count, dst_ptr, edges=False):
        f = lib().aloam_graph_export_edges if edges else lib().aloam_graph_export
        self._check(f(self.h, int(seq), int(first), int(count), _vp(dst_ptr)))

    def graph_export(self, seq=0, first=0, count=None, edges=False, pinned=True):
        """Nodes (or edges) [first, first + count) of one sequence after a synchronise, as a structured array."""
        dt = GRAPH_EDGE_DTYPE if edges else GRAPH_NODE_DTYPE
        if count is None:
            count = self.graph_info(seq)["edges" if edges else "nodes"] - first
        buf = _out_bytes(count, dt, pinned)
        self.graph_export_into(seq, first, count, buf.data_ptr(), edges)
        self.synchronize()
        return _records(buf, count, dt)

    def graph_clear(self, seqs):
        ids = _ids(seqs)
        self._check(lib().aloam_graph_clear(self.h, _ids_arg(ids), len(ids)))

    def graph_info(self, seq=0):
        v = np.zeros(4, np.int32)
        self._check(lib().aloam_graph_info(self.h, int(seq), _p(v)))
        return {"nodes": int(v[0]), "edges": int(v[1]), "max_nodes": int(v[2]), "max_edges": int(v[3])}

    # ---- keyframe clouds and the map at the graph's poses (atlas.tiles_from_keyframes holds the definition) --------------------------------
    def graph_keyframes_enable(self, max_corner_points, max_surf_points):
        """Keep every new node's stacks (sensor frame) on the device: per sequence a row of that many corner / surf points."""
        self._check(lib().aloam_graph_keyframes_enable(self.h, int(max_corner_points), int(max_surf_points)))

    def graph_export_keyframes_into(self, seq, first, count, feature_class, points_ptr, cap_points, offsets_ptr):
        self._check(lib().aloam_graph_export_keyframes(self.h, int(seq), int(first), int(count), int(feature_class), _vp(points_ptr),
                                                       int(cap_points), _vp(offsets_ptr)))

    def graph_export_keyframes(self, seq=0, first=0, count=None, feature_class=0, pinned=True):
        """The clouds of nodes [first, first + count) of one class: a size query, one allocation, the export and a synchronise.  Returns
        (points float32 [n, 4], offsets int64 [count + 1])."""
        import torch
        if count is None:
            count = self.graph_info(seq)["nodes"] - first
        off = torch.zeros(count + 1, dtype=torch.int64, pin_memory=True)
        self.graph_export_keyframes_into(seq, first, count, feature_class, 0, 0, off.data_ptr())
        self.synchronize()
        n = int(off[count])
        pts = torch.zeros((max(1, n), 4), dtype=torch.float32, **_where(pinned))
        self.graph_export_keyframes_into(seq, first, count, feature_class, pts.data_ptr(), n, off.data_ptr())
        self.synchronize()
        return pts.cpu().numpy()[:n].copy(), off.numpy().copy()

    def graph_keyframe_info(self, seq=0):
        v = np.zeros(8, np.int64)
        self._check(lib().aloam_graph_keyframe_info(self.h, int(seq), _p(v)))
        return {"points": v[0:2].tolist(), "capacity": v[2:4].tolist(), "dropped_nodes": int(v[4]), "dropped_points": int(v[5])}

    @staticmethod
    def graph_map_requests(requests):
        """[(seq, first, count, pose), ...] -> structured array of GRAPH_MAP_REQUEST_DTYPE."""
        r = np.zeros(len(requests), GRAPH_MAP_REQUEST_DTYPE)
        for i, q in enumerate(requests):
            r[i] = tuple(int(v) for v in q)
        return r

    def graph_export_map_into(self, requests, tiles_ptr, cap_tiles, points_ptr, cap_points, offsets_ptr, stats_ptr=0):
        """Queue the map of each request (synchronises the stream once on the way): tiles_ptr receives up to cap_tiles aloam_map_tile
        records, points_ptr up to cap_points float4 points, offsets_ptr 2 * (len(requests) + 1) int64, stats_ptr (0 = not wanted) one
        aloam_graph_map_stats per request - device memory or pinned host memory; 0 pointers with caps of 0 = the size query."""
        r = requests if isinstance(requests, np.ndarray) else self.graph_map_requests(requests)
        r = np.ascontiguousarray(r, dtype=GRAPH_MAP_REQUEST_DTYPE)
        self._check(lib().aloam_graph_export_map(self.h, _p(r) if len(r) else None, len(r), _vp(tiles_ptr), int(cap_tiles),
                                                 _vp(points_ptr), int(cap_points), _vp(offsets_ptr), _vp(stats_ptr)))

    def graph_export_map(self, requests, pinned=True):
        """The maps of `requests` ((seq, first, count, pose) each): a size query, pinned destinations (device memory with pinned=False), then
        the call and a synchronise.  Returns (tiles, points, offsets, stats): MAP_TILE_DTYPE [t], float32 [p, 4], int64 [2, n + 1] and
        GRAPH_MAP_STATS_DTYPE [n]."""
        import torch
        n = len(requests)
        off = torch.zeros(2 * (n + 1), dtype=torch.int64, pin_memory=True)
        self.graph_export_map_into(requests, 0, 0, 0, 0, off.data_ptr())
        self.synchronize()
        nt, npts = int(off[n]), int(off[2 * n + 1])
        tiles = _out_bytes(nt, MAP_TILE_DTYPE, pinned)
        pts = torch.zeros((max(1, npts), 4), dtype=torch.float32, **_where(pinned))
        stats = _out_bytes(n, GRAPH_MAP_STATS_DTYPE, True)
        self.graph_export_map_into(requests, tiles.data_ptr(), nt, pts.data_ptr(), npts, off.data_ptr(), stats.data_ptr())
        self.synchronize()
        return (_records(tiles, nt, MAP_TILE_DTYPE), pts.cpu().numpy()[:npts].copy(), off.numpy().reshape(2, n + 1).copy(),
                _records(stats, n, GRAPH_MAP_STATS_DTYPE))

    # ---- the map of joined sequences (atlas.tiles_from_parts holds the definition) ---------------------------------------------------------
    @staticmethod
    def graph_map_groups(groups):
        """[(parts, pose), ...] with parts = [(seq, first, count, frame), ...] -> (parts of GRAPH_MAP_PART_DTYPE, groups of
        GRAPH_MAP_GROUP_DTYPE): the parts of all groups laid end to end, every group indexing its run."""
        parts = [tuple(int(v) for v in p) for g in groups for p in g[0]]
        pr = np.zeros(len(parts), GRAPH_MAP_PART_DTYPE)
        for i, p in enumerate(parts):
            pr[i] = p
        gr = np.zeros(len(groups), GRAPH_MAP_GROUP_DTYPE)
        at = 0
        for i, (ps, pose) in enumerate(groups):
            gr[i] = (at, len(ps), int(pose), 0)
            at += len(ps)
        return pr, gr

    def graph_export_map_joint_into(self, groups, tiles_ptr, cap_tiles, points_ptr, cap_points, offsets_ptr, stats_ptr=0, frames=None):
        """Queue the map of each group of parts (synchronises the stream once on the way).  groups: [(parts, pose), ...] or a pair of
        record arrays (parts, groups); frames: [n_frames, 7] = (q_A xyzw, t_A) or None.  The destinations are those of
        graph_export_map_into, with one offset pair and one aloam_graph_map_stats per group."""
        if isinstance(groups, tuple) and len(groups) == 2 and isinstance(groups[0], np.ndarray) and isinstance(groups[1], np.ndarray):
            pr, gr = groups
        else:
            pr, gr = self.graph_map_groups(groups)
        pr, gr = np.ascontiguousarray(pr, dtype=GRAPH_MAP_PART_DTYPE), np.ascontiguousarray(gr, dtype=GRAPH_MAP_GROUP_DTYPE)
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.float64).reshape(-1, 7)
        self._check(lib().aloam_graph_export_map_joint(self.h, _p(pr) if len(pr) else None, len(pr), _p(fr) if fr is not None and len(fr) else None,
                                                       0 if fr is None else len(fr), _p(gr) if len(gr) else None, len(gr), _vp(tiles_ptr), int(cap_tiles),
                                                       _vp(points_ptr), int(cap_points), _vp(offsets_ptr), _vp(stats_ptr)))

    def graph_export_map_joint(self, groups, frames=None, pinned=True):
        """The maps of `groups` ([(parts, pose), ...], parts = [(seq, first, count, frame), ...]): a size query, pinned destinations (device
        memory with pinned=False), then the call and a synchronise.  Returns (tiles, points, offsets, stats) as graph_export_map does, with
        one row of offsets and stats per group."""
        import torch
        n = len(groups)
        off = torch.zeros(2 * (n + 1), dtype=torch.int64, pin_memory=True)
        self.graph_export_map_joint_into(groups, 0, 0, 0, 0, off.data_ptr(), frames=frames)
        self.synchronize()
        nt, npts = int(off[n]), int(off[2 * n + 1])
        tiles = _out_bytes(nt, MAP_TILE_DTYPE, pinned)
        pts = torch.zeros((max(1, npts), 4), dtype=torch.float32, **_where(pinned))
        stats = _out_bytes(n, GRAPH_MAP_STATS_DTYPE, True)
        self.graph_export_map_joint_into(groups, tiles.data_ptr(), nt, pts.data_ptr(), npts, off.data_ptr(), stats.data_ptr(), frames=frames)
        self.synchronize()
        return (_records(tiles, nt, MAP_TILE_DTYPE), pts.cpu().numpy()[:npts].copy(), off.numpy().reshape(2, n + 1).copy(),
                _records(stats, n, GRAPH_MAP_STATS_DTYPE))

    # ---- a solved graph carried into the live state (posegraph.apply_correction, atlas.window_from_keyframes hold the definition) ------------
    @staticmethod
    def graph_apply_requests(requests):
        """[(seq, first, count, flags), ...] -> structured array of GRAPH_APPLY_REQUEST_DTYPE."""
        r = np.zeros(len(requests), GRAPH_APPLY_REQUEST_DTYPE)
        for i, q in enumerate(requests):
            r[i] = tuple(int(v) for v in q)
        return r

    def graph_apply_into(self, requests, dst_ptr):
        """Queue the correction of each request's sequence (with GRAPH_APPLY_MAP the stream is synchronised on the way): dst_ptr receives one
        aloam_graph_apply_result per request, device memory or pinned host memory."""
        r = requests if isinstance(requests, np.ndarray) else self.graph_apply_requests(requests)
        r = np.ascontiguousarray(r, dtype=GRAPH_APPLY_REQUEST_DTYPE)
        self._check(lib().aloam_graph_apply(self.h, _p(r) if len(r) else None, len(r), _vp(dst_ptr)))

    def graph_apply(self, requests, pinned=True):
        """Apply and wait: a structured array [len(requests)] of GRAPH_APPLY_RESULT_DTYPE."""
        buf = _out_bytes(len(requests), GRAPH_APPLY_RESULT_DTYPE, pinned)
        self.graph_apply_into(requests, buf.data_ptr())
        self.synchronize()
        return _records(buf, len(requests), GRAPH_APPLY_RESULT_DTYPE)

    # ---- loop edges measured on the device (a-loam_amd/loopreg.py holds the definition) -----------------------------------------------------
    def graph_loops_enable(self, max_requests, max_target_corner_points, max_target_surf_points):
        """The scratch of max_requests registrations whose raw targets hold up to that many corner / surf points."""
        self._check(lib().aloam_graph_loops_enable(self.h, int(max_requests), int(max_target_corner_points), int(max_target_surf_points)))

    @staticmethod
    def graph_loop_requests(requests):
        """[(seq, i, j, first, count, pose, q_guess, t_guess), ...] -> structured array of GRAPH_LOOP_REQUEST_DTYPE."""
        r = np.zeros(len(requests), GRAPH_LOOP_REQUEST_DTYPE)
        for k, (seq, i, j, first, count, pose, q, t) in enumerate(requests):
            r[k]["seq"], r[k]["i"], r[k]["j"], r[k]["first"], r[k]["count"], r[k]["pose"] = int(seq), int(i), int(j), int(first), int(count), int(pose)
            r[k]["q"], r[k]["t"] = np.asarray(q, np.float64), np.asarray(t, np.float64)
        return r

    def graph_loop_options(self, **kw):
        return _options(AloamGraphLoopOptions, lib().aloam_graph_loop_default_options, kw)

    def graph_register_loops_into(self, requests, dst_ptr, options=None):
        """Queue the registration of each request (no host synchronisation): dst_ptr receives one aloam_graph_loop_result per request, device
        memory or pinned host memory."""
        r = requests if isinstance(requests, np.ndarray) else self.graph_loop_requests(requests)
        r = np.ascontiguousarray(r, dtype=GRAPH_LOOP_REQUEST_DTYPE)
        self._check(lib().aloam_graph_register_loops(self.h, _p(r) if len(r) else None, len(r), C.byref(options) if options is not None else None,
                                                     _vp(dst_ptr)))

    def graph_register_loops(self, requests, pinned=True, **options):
        """Register and wait: a structured array [len(requests)] of GRAPH_LOOP_RESULT_DTYPE.  Keyword arguments are fields of
        aloam_graph_loop_options."""
        buf = _out_bytes(len(requests), GRAPH_LOOP_RESULT_DTYPE, pinned)
        self.graph_register_loops_into(requests, buf.data_ptr(), self.graph_loop_options(**options))
        self.synchronize()
        return _records(buf, len(requests), GRAPH_LOOP_RESULT_DTYPE)

    def graph_loop_search(self, **kw):
        """The default grid of aloam_graph_search_loops (3 m in 0.5 m steps, 12.5 degrees in 2.5 degree steps) with the given fields replaced."""
        return _options(AloamGraphLoopSearch, lib().aloam_graph_loop_default_search, kw)

    def graph_search_loops_into(self, requests, dst_ptr, search_dst_ptr, scores_ptr=0, search=None, options=None):
        """Queue the searched registration of each request (no host synchronisation): dst_ptr receives one aloam_graph_loop_result and
        search_dst_ptr one aloam_graph_loop_search_result per request, scores_ptr (or 0) the aloam_map_score of every (request, node);
        device memory or pinned host memory."""
        r = requests if isinstance(requests, np.ndarray) else self.graph_loop_requests(requests)
        r = np.ascontiguousarray(r, dtype=GRAPH_LOOP_REQUEST_DTYPE)
        self._check(lib().aloam_graph_search_loops(self.h, _p(r) if len(r) else None, len(r), C.byref(search) if search is not None else None,
                                                   C.byref(options) if options is not None else None, _vp(dst_ptr), _vp(search_dst_ptr), _vp(scores_ptr)))

    def graph_search_loops(self, requests, search=None, scores=False, pinned=True, **options):
        """Search, register and wait: (results [n] of GRAPH_LOOP_RESULT_DTYPE, search results [n] of GRAPH_LOOP_SEARCH_RESULT_DTYPE[, scores
        [n, K] of MAP_SCORE_DTYPE]).  search: an AloamGraphLoopSearch (graph_loop_search(...)), a dict of its fields, or None for the
        defaults; keyword arguments are fields of aloam_graph_loop_options."""
        import torch
        from .relocalize import grid_axes
        g = self.graph_loop_search(**search) if isinstance(search, dict) else search if search is not None else self.graph_loop_search()
        lin, yaw = grid_axes(g.radius_m, g.step_m, g.yaw_deg, g.yaw_step_deg)
        n, K = len(requests), len(yaw) * len(lin) * len(lin)
        res, found = _out_bytes(n, GRAPH_LOOP_RESULT_DTYPE, pinned), _out_bytes(n, GRAPH_LOOP_SEARCH_RESULT_DTYPE, pinned)
        sc = torch.zeros(max(1, n) * (K * MAP_SCORE_DTYPE.itemsize if scores else 8), dtype=torch.uint8, **_where(pinned))
        self.graph_search_loops_into(requests, res.data_ptr(), found.data_ptr(), sc.data_ptr() if scores else 0, g, self.graph_loop_options(**options))
        self.synchronize()
        out = (_records(res, n, GRAPH_LOOP_RESULT_DTYPE), _records(found, n, GRAPH_LOOP_SEARCH_RESULT_DTYPE))
        if scores:
            out += (_records(sc, n * K, MAP_SCORE_DTYPE).reshape(n, K),)
        return out

    def graph_loop_target(self, slot=0, feature_class=0):
        """The filtered target of a scratch slot as the last graph_register_loops left it (parity tests): float32 [n, 4]."""
        import torch
        cnt = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self._check(lib().aloam_graph_loop_export_target(self.h, int(slot), int(feature_class), None, 0, C.c_void_p(cnt.data_ptr())))
        self.synchronize()
        n = int(cnt[0])
        pts = torch.zeros((max(1, n), 4), dtype=torch.float32, pin_memory=True)
        self._check(lib().aloam_graph_loop_export_target(self.h, int(slot), int(feature_class), C.c_void_p(pts.data_ptr()), n, C.c_void_p(cnt.data_ptr())))
        self.synchronize()
        return pts.numpy()[:n].copy()

    # ---- pose-graph marginals (posegraph.marginals holds the definition) -------------------------------------------------------------------
    def graph_marginal_options(self, **kw):
        return _options(AloamGraphMarginalOptions, lib().aloam_graph_marginal_default_options, kw)

    def graph_marginals_into(self, requests, dst_ptr, options=None):
        """Queue the marginals of each request (a structured array of GRAPH_MARGINAL_REQUEST_DTYPE, posegraph.marginal_request builds one; no
        host synchronisation): dst_ptr receives one aloam_graph_marginal_result per request, device memory or pinned host memory."""
        r = np.ascontiguousarray(requests, dtype=GRAPH_MARGINAL_REQUEST_DTYPE)
        self._check(lib().aloam_graph_marginals(self.h, _p(r) if len(r) else None, len(r), C.byref(options) if options is not None else None,
                                                _vp(dst_ptr)))

    def graph_marginals(self, requests, options=None, pinned=True):
        """Compute and wait: a structured array [len(requests)] of GRAPH_MARGINAL_RESULT_DTYPE.  options: None (the defaults), an
        AloamGraphMarginalOptions, or a dict of its fields."""
        if isinstance(options, dict):
            options = self.graph_marginal_options(**options)
        buf = _out_bytes(len(requests), GRAPH_MARGINAL_RESULT_DTYPE, pinned)
        self.graph_marginals_into(requests, buf.data_ptr(), options)
        self.synchronize()
        return _records(buf, len(requests), GRAPH_MARGINAL_RESULT_DTYPE)

    # ---- the robust solve (posegraph.optimize_robust holds the definition) ----------------------------------------------------------------
    def graph_robust_options(self, **kw):
        return _options(AloamGraphRobustOptions, lib().aloam_graph_robust_default_options, kw)

    def graph_optimize_robust_into(self, seqs, dst_ptr, options=None, robust=None, weights_ptr=0, weights_stride=0):
        """Queue the robust solve of the listed sequences' graphs (no host synchronisation): dst_ptr receives one aloam_graph_robust_result
        each, weights_ptr (or 0) one row of weights_stride doubles each; device memory or pinned host memory."""
        ids = _ids(seqs)
        self._check(lib().aloam_graph_optimize_robust(self.h, _ids_arg(ids), len(ids), C.byref(options) if options is not None else None,
                                                      C.byref(robust) if robust is not None else None, _vp(dst_ptr), _vp(weights_ptr), int(weights_stride)))

    def graph_optimize_robust(self, seqs, robust=None, pinned=True, weights_stride=None, sentinel=np.nan, **options):
        """Solve and wait: (a structured array [len(seqs)] of GRAPH_ROBUST_RESULT_DTYPE, the weights [len(seqs), weights_stride]: a row holds
        one weight per edge of its sequence and `sentinel` behind them).  robust: None (the defaults), an AloamGraphRobustOptions, or a dict of
        its fields; keyword arguments are fields of aloam_graph_options."""
        import torch
        if isinstance(robust, dict):
            robust = self.graph_robust_options(**robust)
        n = len(seqs)
        if weights_stride is None:
            weights_stride = max([self.graph_info(int(b))["edges"] for b in seqs] + [1])
        buf = _out_bytes(n, GRAPH_ROBUST_RESULT_DTYPE, pinned)
        wts = torch.full((max(1, n), int(weights_stride)), float(sentinel), dtype=torch.float64, **_where(pinned))
        self.graph_optimize_robust_into(seqs, buf.data_ptr(), self.graph_options(**options), robust, wts.data_ptr(), weights_stride)
        self.synchronize()
        return _records(buf, n, GRAPH_ROBUST_RESULT_DTYPE), wts.cpu().numpy()[:n].copy()

    # ---- loop candidates by pose proximity (posegraph.propose_loops holds the definition) ----------------------------------------------------
    def graph_propose_loops_into(self, queries, dst_ptr, counts_ptr, dist2_ptr=0, *, radius_m, growth_m_per_node=0.0, min_gap, half_window=0,
                                 separation=0, K=1, pose=GRAPH_POSE_OPTIMIZED):
        """Queue the radius search of each query ((seq, j) pairs; no host synchronisation): dst_ptr receives K aloam_graph_loop_request per
        query, counts_ptr one int, dist2_ptr (or 0) K doubles; device memory or pinned host memory."""
        qs = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 2)
        self._check(lib().aloam_graph_propose_loops(self.h, _p(qs) if len(qs) else None, len(qs), int(pose), float(radius_m), float(growth_m_per_node),
                                                    int(min_gap), int(half_window), int(separation), int(K), _vp(dst_ptr), _vp(counts_ptr), _vp(dist2_ptr)))

    def graph_propose_loops(self, queries, pinned=True, **parameters):
        """Propose and wait: (requests [n, K] of GRAPH_LOOP_REQUEST_DTYPE, counts int32 [n], dist2 float64 [n, K]).  Keyword arguments are
        the parameters of aloam_graph_propose_loops (radius_m, growth_m_per_node, min_gap, half_window, separation, K, pose)."""
        import torch
        n, K = len(np.asarray(queries).reshape(-1, 2)), int(parameters.get("K", 1))
        dst = _out_bytes(n * K, GRAPH_LOOP_REQUEST_DTYPE, pinned)
        cnt = torch.zeros(max(1, n), dtype=torch.int32, **_where(pinned))
        d2 = torch.zeros(max(1, n * K), dtype=torch.float64, **_where(pinned))
        self.graph_propose_loops_into(queries, dst.data_ptr(), cnt.data_ptr(), d2.data_ptr(), **parameters)
        self.synchronize()
        return _records(dst, n * K, GRAPH_LOOP_REQUEST_DTYPE).reshape(n, K), cnt.cpu().numpy()[:n].copy(), d2.cpu().numpy()[:n * K].reshape(n, K).copy()

    # ---- trimming a graph in place (posegraph.trim and graph_records.trim_keyframes hold the definition) -----------------------------------
    def graph_trim(self, seqs, first):
        """Drop nodes [0, first[k]) of every listed sequence's graph on the device; edges from a dropped node to a kept one become anchors.
        Synchronises the stream once.  Returns int32 [n, 8]: nodes, edges, anchored, removed_fixed, removed_reverse, corner / surf points
        freed, 0."""
        ids = _ids(seqs)
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(first, dtype=np.int32), (len(ids),)))
        out = np.zeros((len(ids), 8), np.int32)
        self._check(lib().aloam_graph_trim(self.h, _ids_arg(ids), _p(f) if len(ids) else None, len(ids), _p(out) if len(ids) else None))
        return out

    # ---- joined graphs: links between sequences and a joint solve (posegraph.join / optimize_joint hold the definition) ---------------------
    @staticmethod
    def joint_lists(groups):
        """The four host lists of a joint call from groups = [(members, links) or (members, links, align), ...]: members int32, align int32,
        links (GRAPH_LINK_DTYPE), groups (GRAPH_JOINT_GROUP_DTYPE)."""
        members, align, links, n_links, recs = [], [], [], 0, np.zeros(len(groups), GRAPH_JOINT_GROUP_DTYPE)
        for g, group in enumerate(groups):
            m, l = group[0], np.ascontiguousarray(group[1] if group[1] is not None else [], dtype=GRAPH_LINK_DTYPE).reshape(-1)
            a = group[2] if len(group) > 2 and group[2] is not None else [0] * len(m)
            recs[g] = (len(members), len(m), n_links, len(l))
            members += [int(v) for v in m]; align += [int(v) for v in a]; links.append(l)
            n_links += len(l)
        links = np.concatenate(links) if links else np.zeros(0, GRAPH_LINK_DTYPE)
        return np.array(members, np.int32), np.array(align, np.int32), np.ascontiguousarray(links), recs

    def graph_optimize_joint_into(self, groups, dst_ptr, options=None, robust=None, weights_ptr=0, weights_stride=0, robust_call=False):
        """Queue the joint solve of every group (no host synchronisation; groups as for graph_optimize_joint, or the tuple joint_lists
        made of them, for a caller that repeats a call): dst_ptr receives one aloam_graph_result per group - with
        robust_call one aloam_graph_robust_result, and weights_ptr (or 0) one row of weights_stride doubles; device or pinned memory."""
        m, a, l, g = groups if isinstance(groups, tuple) else self.joint_lists(groups)      # (a tuple: the four lists, built once by joint_lists)
        lists = (_p(m) if len(m) else None, _p(a) if len(a) else None, len(m), _p(l) if len(l) else None, len(l), _p(g) if len(g) else None, len(g))
        opt = C.byref(options) if options is not None else None
        if robust_call:
            self._check(lib().aloam_graph_optimize_joint_robust(self.h, *lists, opt, C.byref(robust) if robust is not None else None, _vp(dst_ptr),
                                                                _vp(weights_ptr), int(weights_stride)))
        else:
            self._check(lib().aloam_graph_optimize_joint(self.h, *lists, opt, _vp(dst_ptr)))

    def graph_optimize_joint(self, groups, pinned=True, **options):
        """Join, solve, write back and wait: a structured array [len(groups)] of GRAPH_RESULT_DTYPE.  groups = [(members, links) or
        (members, links, align), ...]; keyword arguments are fields of aloam_graph_options."""
        buf = _out_bytes(len(groups), GRAPH_RESULT_DTYPE, pinned)
        self.graph_optimize_joint_into(groups, buf.data_ptr(), self.graph_options(**options))
        self.synchronize()
        return _records(buf, len(groups), GRAPH_RESULT_DTYPE)

    def graph_optimize_joint_robust(self, groups, robust=None, pinned=True, weights_stride=None, sentinel=np.nan, **options):
        """The same with the robust solve: (a structured array [len(groups)] of GRAPH_ROBUST_RESULT_DTYPE, the weights
        [len(groups), weights_stride]: one per joined edge - the members' edges in member order, then the links - and `sentinel` behind them)."""
        import torch
        if isinstance(robust, dict):
            robust = self.graph_robust_options(**robust)
        n = len(groups)
        if weights_stride is None:
            weights_stride = max([sum(self.graph_info(int(b))["edges"] for b in g[0]) + (len(g[1]) if g[1] is not None else 0) for g in groups] + [1])
        buf = _out_bytes(n, GRAPH_ROBUST_RESULT_DTYPE, pinned)
        wts = torch.full((max(1, n), int(weights_stride)), float(sentinel), dtype=torch.float64, **_where(pinned))
        self.graph_optimize_joint_into(groups, buf.data_ptr(), self.graph_options(**options), robust, wts.data_ptr(), weights_stride, robust_call=True)
        self.synchronize()
        return _records(buf, n, GRAPH_ROBUST_RESULT_DTYPE), wts.cpu().numpy()[:n].copy()

    def graph_joint_export(self, group):
        """The joined rows of one group of the last joint call (synchronises): (nodes, edges, counts = [nodes, edges, member edges, links])."""
        counts = np.zeros(4, np.int32)
        self._check(lib().aloam_graph_joint_export(self.h, int(group), None, 0, None, 0, _p(counts)))
        nodes, edges = np.zeros(max(1, counts[0]), GRAPH_NODE_DTYPE), np.zeros(max(1, counts[1]), GRAPH_EDGE_DTYPE)
        self._check(lib().aloam_graph_joint_export(self.h, int(group), _p(nodes), len(nodes), _p(edges), len(edges), _p(counts)))
        return nodes[:counts[0]], edges[:counts[1]], counts

    # ---- links measured on the device (loopreg.link_request / posegraph.propose_links hold the definitions) ----------------------------------
    @staticmethod
    def graph_link_requests(requests):
        """[(seq_i, i, first, count, seq_j, j, pose, q_guess, t_guess), ...] -> structured array of GRAPH_LINK_REQUEST_DTYPE."""
        r = np.zeros(len(requests), GRAPH_LINK_REQUEST_DTYPE)
        for k, (seq_i, i, first, count, seq_j, j, pose, q, t) in enumerate(requests):
            r[k]["seq_i"], r[k]["i"], r[k]["first"], r[k]["count"] = int(seq_i), int(i), int(first), int(count)
            r[k]["seq_j"], r[k]["j"], r[k]["pose"] = int(seq_j), int(j), int(pose)
            r[k]["q"], r[k]["t"] = np.asarray(q, np.float64), np.asarray(t, np.float64)
        return r

    def graph_register_links_into(self, requests, dst_ptr, options=None):
        """Queue the registration of each link request (no host synchronisation): dst_ptr receives one aloam_graph_loop_result per request,
        device memory or pinned host memory."""
        r = requests if isinstance(requests, np.ndarray) else self.graph_link_requests(requests)
        r = np.ascontiguousarray(r, dtype=GRAPH_LINK_REQUEST_DTYPE)
        self._check(lib().aloam_graph_register_links(self.h, _p(r) if len(r) else None, len(r), C.byref(options) if options is not None else None,
                                                     _vp(dst_ptr)))

    def graph_register_links(self, requests, pinned=True, **options):
        """Register and wait: a structured array [len(requests)] of GRAPH_LOOP_RESULT_DTYPE.  Keyword arguments are fields of
        aloam_graph_loop_options."""
        buf = _out_bytes(len(requests), GRAPH_LOOP_RESULT_DTYPE, pinned)
        self.graph_register_links_into(requests, buf.data_ptr(), self.graph_loop_options(**options))
        self.synchronize()
        return _records(buf, len(requests), GRAPH_LOOP_RESULT_DTYPE)

    def graph_search_links_into(self, requests, dst_ptr, search_dst_ptr, scores_ptr=0, search=None, options=None):
        """Queue the searched registration of each link request (no host synchronisation); the outputs are those of graph_search_loops_into."""
        r = requests if isinstance(requests, np.ndarray) else self.graph_link_requests(requests)
        r = np.ascontiguousarray(r, dtype=GRAPH_LINK_REQUEST_DTYPE)
        self._check(lib().aloam_graph_search_links(self.h, _p(r) if len(r) else None, len(r), C.byref(search) if search is not None else None,
                                                   C.byref(options) if options is not None else None, _vp(dst_ptr), _vp(search_dst_ptr), _vp(scores_ptr)))

    def graph_search_links(self, requests, search=None, scores=False, pinned=True, **options):
        """Search, register and wait: what graph_search_loops returns, for link requests."""
        import torch
        from .relocalize import grid_axes
        g = self.graph_loop_search(**search) if isinstance(search, dict) else search if search is not None else self.graph_loop_search()
        lin, yaw = grid_axes(g.radius_m, g.step_m, g.yaw_deg, g.yaw_step_deg)
        n, K = len(requests), len(yaw) * len(lin) * len(lin)
        res, found = _out_bytes(n, GRAPH_LOOP_RESULT_DTYPE, pinned), _out_bytes(n, GRAPH_LOOP_SEARCH_RESULT_DTYPE, pinned)
        sc = torch.zeros(max(1, n) * (K * MAP_SCORE_DTYPE.itemsize if scores else 8), dtype=torch.uint8, **_where(pinned))
        self.graph_search_links_into(requests, res.data_ptr(), found.data_ptr(), sc.data_ptr() if scores else 0, g, self.graph_loop_options(**options))
        self.synchronize()
        out = (_records(res, n, GRAPH_LOOP_RESULT_DTYPE), _records(found, n, GRAPH_LOOP_SEARCH_RESULT_DTYPE))
        if scores:
            out += (_records(sc, n * K, MAP_SCORE_DTYPE).reshape(n, K),)
        return out

    def graph_propose_links_into(self, queries, dst_ptr, counts_ptr, dist2_ptr=0, *, frames=None, radius_m, half_window=0, separation=0, K=1,
                                 pose=GRAPH_POSE_OPTIMIZED):
        """Queue the radius search of each query ((seq_j, j, seq_i) triples; frames: [n, 7] = q_A, t_A per query, or None; no host
        synchronisation): dst_ptr receives K aloam_graph_link_request per query, counts_ptr one int, dist2_ptr (or 0) K doubles; device
        memory or pinned host memory."""
        qs = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 3)
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.float64).reshape(len(qs), 7)
        self._check(lib().aloam_graph_propose_links(self.h, _p(qs) if len(qs) else None, _p(fr) if fr is not None and len(qs) else None, len(qs), int(pose),
                                                    float(radius_m), int(half_window), int(separation), int(K), _vp(dst_ptr), _vp(counts_ptr), _vp(dist2_ptr)))

    def graph_propose_links(self, queries, pinned=True, **parameters):
        """Propose and wait: (requests [n, K] of GRAPH_LINK_REQUEST_DTYPE, counts int32 [n], dist2 float64 [n, K]).  Keyword arguments are
        the parameters of aloam_graph_propose_links (frames, radius_m, half_window, separation, K, pose)."""
        import torch
        n, K = len(np.asarray(queries).reshape(-1, 3)), int(parameters.get("K", 1))
        dst = _out_bytes(n * K, GRAPH_LINK_REQUEST_DTYPE, pinned)
        cnt = torch.zeros(max(1, n), dtype=torch.int32, **_where(pinned))
        d2 = torch.zeros(max(1, n * K), dtype=torch.float64, **_where(pinned))
        self.graph_propose_links_into(queries, dst.data_ptr(), cnt.data_ptr(), d2.data_ptr(), **parameters)
        self.synchronize()
        return _records(dst, n * K, GRAPH_LINK_REQUEST_DTYPE).reshape(n, K), cnt.cpu().numpy()[:n].copy(), d2.cpu().numpy()[:n * K].reshape(n, K).copy()

    # ---- graph records (a-loam_amd/graph_records.py holds the format) ------------------------------------------------------------------
    def graph_save_into(self, seqs, dst_ptr, cap_bytes, offsets_ptr):
        """Queue the graph records of `seqs` into dst_ptr (device memory or pinned host memory; 0 with cap_bytes 0 = the size query);
        offsets_ptr receives len(seqs) + 1 int64 byte offsets.  Stream-ordered: wait with synchronize()."""
        ids = _ids(seqs)
        self._check(lib().aloam_graph_save(self.h, _ids_arg(ids), len(ids), _vp(dst_ptr), int(cap_bytes), _vp(offsets_ptr)))

    def graph_save(self, seqs, pinned=True):
        """Graph records of `seqs`: a size query, one allocation (pinned host memory, or device memory with pinned=False), the save and a
        synchronise.  Returns (blob, offsets) shaped like save_sequences'."""
        import torch
        off = torch.zeros(len(seqs) + 1, dtype=torch.int64, pin_memory=True)
        self.graph_save_into(seqs, 0, 0, off.data_ptr())
        self.synchronize()
        total = int(off[-1])
        blob = torch.empty(max(total, 16), dtype=torch.uint8, **_where(pinned))
        self.graph_save_into(seqs, blob.data_ptr(), total, off.data_ptr())
        self.synchronize()
        return (blob[:total].numpy() if pinned else blob[:total]), off.numpy().copy()

    def graph_load(self, slots, blob, offsets):
        """Graph record i of blob (numpy array - pageable or a pinned view - or torch tensor on this device or pinned), at
        [offsets[i], offsets[i + 1]), into the empty graph of slots[i].  The blob is kept referenced until the next load (the copy is
        stream-ordered)."""
        ids = _ids(slots)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        ptr = blob.data_ptr() if hasattr(blob, "data_ptr") else blob.ctypes.data
        self._graph_load_keep = (blob, off)
        self._check(lib().aloam_graph_load(self.h, _ids_arg(ids), len(ids), _vp(ptr), _p(off)))

    # ---- sequence records ------------------------------------------------------------------------------------------------------------
    def save_sequences_into(self, seqs, dst_ptr, cap_bytes, offsets_ptr):
        """Queue the records of `seqs` into dst_ptr (device memory or pinned host memory; 0 with cap_bytes 0 = the size query); offsets_ptr
        receives len(seqs) + 1 int64 byte offsets.  Stream-ordered: wait with synchronize()."""
        ids = _ids(seqs)
        self._check(lib().aloam_save_sequences(self.h, _ids_arg(ids), len(ids), _vp(dst_ptr), int(cap_bytes), _vp(offsets_ptr)))

    def save_sequences(self, seqs, pinned=True):
        """Records of `seqs`: a size query, one allocation (pinned host memory, or device memory with pinned=False), the save and a
        synchronise.  Returns (blob, offsets): blob a uint8 numpy array (pinned) or torch tensor (device), offsets int64 numpy [len(seqs) + 1]."""
        import torch
        off = torch.zeros(len(seqs) + 1, dtype=torch.int64, pin_memory=True)
        self.save_sequences_into(seqs, 0, 0, off.data_ptr())
        self.synchronize()
        total = int(off[-1])
        blob = torch.empty(max(total, 16), dtype=torch.uint8, **_where(pinned))
        self.save_sequences_into(seqs, blob.data_ptr(), total, off.data_ptr())
        self.synchronize()
        return (blob[:total].numpy() if pinned else blob[:total]), off.numpy().copy()

    def load_sequences(self, slots, blob, offsets):
        """Record i of blob (numpy array - pageable or a pinned view - or torch tensor on this device or pinned), at
        [offsets[i], offsets[i + 1]), into slots[i].  The blob is kept referenced until the next load (the copy is stream-ordered)."""
        ids = _ids(slots)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        ptr = blob.data_ptr() if hasattr(blob, "data_ptr") else blob.ctypes.data
        self._load_keep = (blob, off)
        self._check(lib().aloam_load_sequences(self.h, _ids_arg(ids), len(ids), _vp(ptr), _p(off)))

    def odometry_step(self):
        self._check(lib().aloam_odometry_step(self.h))

    def pose(self, seq=0):
        qw, tw, ql, tl = np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(3)
        self._check(lib().aloam_get_pose(self.h, seq, _p(qw), _p(tw), _p(ql), _p(tl)))
        return {"q_w": qw, "t_w": tw, "q_lc": ql, "t_lc": tl}

    def odom_stats(self, seq=0):
        st = AloamOdomStats()
        self._check(lib().aloam_get_odom_stats(self.h, seq, C.byref(st)))
        return {k: list(getattr(st, k)) for k, _ in AloamOdomStats._fields_}

    def last_cloud_order(self, seq=0):
        v = np.zeros(2, np.int32)
        self._check(lib().aloam_get_last_cloud_order(self.h, seq, _p(v)))
        return int(v[0]), int(v[1])

    def solve_lds(self):
        """(plane slots per thread, edge slots per thread, bytes of dynamic LDS) the odometry solve keeps; zeros with ALOAM_SOLVE_STAGE=0."""
        v = np.zeros(3, np.int32)
        self._check(lib().aloam_get_solve_lds(self.h, _p(v)))
        return int(v[0]), int(v[1]), int(v[2])

    def correspondences(self, seq=0):
        cap_e, cap_p = self.n_scans * 12, self.n_scans * 24
        e = np.zeros((cap_e, 9), np.float32); p = np.zeros((cap_p, 12), np.float32)
        eq = np.zeros(cap_e, np.int32); pq = np.zeros(cap_p, np.int32)
        ne, npl = C.c_int(0), C.c_int(0)
        self._check(lib().aloam_get_correspondences(self.h, seq, _p(e), cap_e, C.byref(ne), _p(eq), _p(p), cap_p, C.byref(npl), _p(pq)))
        return e[:ne.value].copy(), p[:npl.value].copy(), eq[:ne.value].copy(), pq[:npl.value].copy()

    # ---- stage 3 -------------------------------------------------------------------------------------------
    def mapping_enable(self, line_res=0.4, plane_res=0.8, pool_points=262144, pool_limit=None):
        """pool_points: where the map pools start (they double as the map grows); pool_limit: the ceiling (None = the library's default)."""
        if pool_limit is not None:
            self._check(lib().aloam_mapping_set_pool_limit(self.h, int(pool_limit)))
        self._check(lib().aloam_mapping_enable(self.h, float(line_res), float(plane_res), int(pool_points)))

    def map_pool_info(self):
        v = np.zeros(4, np.int32)
        self._check(lib().aloam_get_map_pool_info(self.h, _p(v)))
        return {"pool_points": int(v[0]), "growths": int(v[1]), "limit": int(v[2]), "live_max": int(v[3])}

    def set_map(self, cubes, cls, seq=0):
        """cubes: {cube index: (n, 4) points} -> laserCloudCornerArray (cls 0) / laserCloudSurfArray (cls 1) of the sequence."""
        ids = np.array(sorted(cubes), np.int32)
        cnt = np.array([len(cubes[int(i)]) for i in ids], np.int32)
        pts = _f32(np.concatenate([cubes[int(i)] for i in ids])) if len(ids) else np.zeros((0, 4), np.float32)
        self._check(lib().aloam_set_map(self.h, seq, cls, _p(ids), _p(cnt), len(ids), _p(pts)))

    def set_map_frame(self, cen, q_wmap_wodom, t_wmap_wodom, frame_count, seq=0):
        a, q, t = np.ascontiguousarray(cen, dtype=np.int32), _f64(q_wmap_wodom), _f64(t_wmap_wodom)
        self._check(lib().aloam_set_map_frame(self.h, seq, _p(a), _p(q), _p(t), int(frame_count)))

    def mapping_step(self):
        self._check(lib().aloam_mapping_step(self.h))

    def set_full_cloud(self, cloud, seq=0):
        a = _f32(cloud)
        self._check(lib().aloam_set_full_cloud(self.h, seq, _p(a), len(a)))

    def mapping_step_inputs(self, q_wodom, t_wodom, corner_last, surf_last, full_res, seq=0):
        """Teacher-forced frame: inject what the mapping node receives (reference src/laserMapping.cpp:175-228), then step."""
        self.set_last(corner_last, surf_last, seq)
        self.set_full_cloud(full_res, seq)
        p = self.pose(seq)
        self.set_state(p["q_lc"], p["t_lc"], q_wodom, t_wodom, seq)
        self.mapping_step()
        return self.map_pose(seq)

    def map_pose(self, seq=0):
        qw, tw, qm, tm = np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(3)
        self._check(lib().aloam_get_map_pose(self.h, seq, _p(qw), _p(tw), _p(qm), _p(tm)))
        return {"q_w": qw, "t_w": tw, "q_wmap_wodom": qm, "t_wmap_wodom": tm}

    def map_info(self, seq=0):
        v = np.zeros(16, np.int32)
        self._check(lib().aloam_get_map_info(self.h, seq, _p(v)))
        return dict(zip(MAP_INFO_KEYS, (int(x) for x in v)))

    def map_cubes(self, cls, seq=0):
        cnt = np.zeros(21 * 21 * 11, np.int32)
        self._check(lib().aloam_map_cube_counts(self.h, seq, cls, _p(cnt)))
        out = {}
        for i in np.nonzero(cnt)[0]:
            pts = np.zeros((int(cnt[i]), 4), np.float32)
            self._check(lib().aloam_get_map_cube(self.h, seq, cls, int(i), _p(pts), len(pts)))
            out[int(i)] = pts
        return out

    def map_cloud(self, which, seq=0):
        n = self._check(lib().aloam_get_map_cloud(self.h, seq, which, None, 0))
        out = np.zeros((n, 4), np.float32)
        if n:
            self._check(lib().aloam_get_map_cloud(self.h, seq, which, _p(out), n))
        return out

    # ---- batched export (stream-ordered; wait with synchronize()) ------------------------------------------------------------
    def export_poses(self, dst_ptr):
        """One AloamPoseRecord per sequence into dst_ptr (device memory of this context's device, or pinned host memory)."""
        self._check(lib().aloam_export_poses(self.h, C.c_void_p(dst_ptr)))

    def export_clouds(self, ids, dst_ptr, cap_points, offsets_ptr):
        """Clouds `ids` (CLOUD_* or EXPORT_MAP + MAP_*) of every sequence packed into dst_ptr (16-byte points, at most cap_points of
        them), segment (i, b) at [offsets[i * batch + b], offsets[i * batch + b + 1]); offsets_ptr receives len(ids) * batch + 1 int64."""
        a = (C.c_int * max(1, len(ids)))(*[int(v) for v in ids])
        self._check(lib().aloam_export_clouds(self.h, a, len(ids), _vp(dst_ptr), int(cap_points), C.c_void_p(offsets_ptr)))

    def export_pose_information_into(self, which, seqs, dst_ptr):
        """Queue one aloam_pose_information per listed sequence (INFO_ODOMETRY / INFO_MAPPING) into dst_ptr: device memory of this
        context's device, or pinned host memory."""
        ids = _ids(seqs)
        self._check(lib().aloam_export_pose_information(self.h, int(which), _ids_arg(ids), len(ids), _vp(dst_ptr)))

    def export_pose_information(self, which, seqs, pinned=True):
        """The records of `seqs` after a synchronise: a structured array [len(seqs)] of POSE_INFORMATION_DTYPE (information.py says what a
        caller does with one); with pinned=False the destination is device memory, copied back afterwards."""
        buf = _out_bytes(len(seqs), POSE_INFORMATION_DTYPE, pinned)
        self.export_pose_information_into(which, seqs, buf.data_ptr())
        self.synchronize()
        return _records(buf, len(seqs), POSE_INFORMATION_DTYPE)

    def map_factors(self, seq=0):
        """The factor records the last mapping solve of `seq` read: (lines [n, 9] cp, a, b; planes [m, 7] cp, n, d), float64, in the solver's order."""
        nl, npl = C.c_int(0), C.c_int(0)
        self._check(lib().aloam_get_map_factors(self.h, seq, None, 0, C.byref(nl), None, 0, C.byref(npl)))
        lines, planes = np.zeros((nl.value, 9)), np.zeros((npl.value, 7))
        self._check(lib().aloam_get_map_factors(self.h, seq, _p(lines) if nl.value else None, nl.value, C.byref(nl),
                                                _p(planes) if npl.value else None, npl.value, C.byref(npl)))
        return lines, planes

    def export_segment(self, points, offsets, ids, which, seq):
        """The points of cloud `which` of sequence `seq` in an export's destination (a torch tensor or numpy array of float32, viewed as
        (n, 4)) given its offsets (after the export has finished)."""
        i = list(ids).index(which)
        lo, hi = int(offsets[i * self.batch + seq]), int(offsets[i * self.batch + seq + 1])
        return points.reshape(-1, 4)[lo:hi]

    # ---- profiling -----------------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(lib().aloam_profile_enable(self.h, int(on)))

    def profile(self):
        out = {}
        for k in range(lib().aloam_profile_kernel_count()):
            ms, n, by = C.c_double(0), C.c_longlong(0), C.c_double(0)
            self._check(lib().aloam_profile_get(self.h, k, C.byref(ms), C.byref(n), C.byref(by)))
            out[lib().aloam_profile_kernel_name(k).decode()] = {"total_ms": ms.value, "launches": n.value, "bytes_per_launch": by.value}
        return out

    def stream(self):
        return lib().aloam_stream(self.h)
