"""ctypes binding of the orbhip C ABI (include/orbhip.h) for tests and bench.py.

Plumbing only: every call goes straight to liborbhip.so (HIP kernels).  There is no
Python or CPU implementation behind these wrappers; if the shared library is missing the
import fails loudly.

torch is imported BEFORE the library is loaded so that one HIP runtime (torch's bundled
libamdhip64.so.7) serves both torch tensors and our kernels in the same process.
"""
import ctypes as C
import os
import numpy as np

try:  # one HIP runtime per process: let torch load its copy first when torch is present
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(os.path.dirname(_HERE), "lib")
LIB_PATH = os.path.join(LIB_DIR, "liborbhip.so")
SYNTH_PATH = os.path.join(LIB_DIR, "libsynth.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "liborbhip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(there is no CPU fallback for the HIP path)")

lib = C.CDLL(LIB_PATH)

OK, E_BADARG, E_NODEVICE, E_HIP, E_CAPACITY, E_ABORTED, E_NOTSPD, E_EMPTY = 0, -1, -2, -3, -4, -5, -6, -7
STAGES = ["pyramid", "fast_cells", "blur", "octree", "desc", "assemble"]

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

vp, ci, cf, cd, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
lib.orbhip_version.restype = C.c_char_p
lib.orbhip_last_error.restype = C.c_char_p
lib.orbhip_ctx_create.argtypes = [ci, vp, C.POINTER(vp)]
lib.orbhip_ctx_destroy.argtypes = [vp]
lib.orbhip_ctx_synchronize.argtypes = [vp]
lib.orbhip_ctx_stream.argtypes = [vp]
lib.orbhip_ctx_stream.restype = vp
lib.orbhip_extractor_create.argtypes = [vp, ci, cf, ci, ci, ci, C.POINTER(vp)]
lib.orbhip_extractor_destroy.argtypes = [vp]
lib.orbhip_extractor_levels.argtypes = [vp]
lib.orbhip_extractor_table.argtypes = [vp, ci, vp]
lib.orbhip_extractor_features_per_level.argtypes = [vp, vp]
lib.orbhip_extractor_umax.argtypes = [vp, vp]
lib.orbhip_blur_half_widths.argtypes = [vp]
lib.orbhip_fast_cell_table.argtypes = [C.c_int, vp, vp, vp, C.c_int]
lib.orbhip_extractor_reserve.argtypes = [vp, ci, ci, ci]
lib.orbhip_extractor_max_keypoints.argtypes = [vp]
lib.orbhip_extract_batch_device.argtypes = [vp, vp, ci, ci, sz, sz, ci, ci, ci]
lib.orbhip_extractor_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
lib.orbhip_extract_batch_host.argtypes = [vp, vp, ci, ci, sz, sz, ci, ci, ci, vp, vp, ci, vp, vp]
lib.orbhip_extractor_level_dims.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci)]
lib.orbhip_extractor_get_pyramid_level.argtypes = [vp, ci, ci, ci, vp, sz]
lib.orbhip_extractor_get_blurred_level.argtypes = [vp, ci, ci, vp, sz]
lib.orbhip_extractor_get_pyramid_padded.argtypes = [vp, ci, vp, vp]
lib.orbhip_extractor_get_fast_candidates.argtypes = [vp, ci, ci, vp, vp, vp, ci, C.POINTER(C.c_int32)]
lib.orbhip_extractor_get_level_keypoints.argtypes = [vp, ci, ci, vp, ci, C.POINTER(C.c_int32)]
lib.orbhip_extractor_set_profiling.argtypes = [vp, ci]
lib.orbhip_extractor_set_graph_mode.argtypes = [vp, ci]
lib.orbhip_extractor_stage_ms.argtypes = [vp, vp]
lib.orbhip_descriptor_distance.argtypes = [vp, vp]
lib.orbhip_match_bf2nn_device.argtypes = [vp, vp, vp, sz, vp, vp, sz, ci, ci, cd, vp, vp, vp]
lib.orbhip_search_for_initialization_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, sz, cf, cf, cf, cf, ci, cf, ci,
                                                        vp, vp, vp]
lib.orbhip_ctx_check_status.argtypes = [vp]
lib.orbhip_ctx_wait_for.argtypes = [vp, vp]
lib.orbhip_extractor_blur_kernel.argtypes = [vp, ci]
lib.orbhip_extractor_blur_kernel.restype = ci
if hasattr(lib, "orbhip_extractor_fast_kernel"):     # (tools/ab_so.sh swaps older builds of the library in)
    lib.orbhip_extractor_fast_kernel.argtypes = [vp]
    lib.orbhip_extractor_fast_kernel.restype = ci
lib.orbhip_extractor_blur_tiled.argtypes = [vp, ci]
lib.orbhip_extractor_blur_tiled.restype = ci
lib.orbhip_extractor_resize_band_rows.argtypes = [vp, ci]
lib.orbhip_extractor_resize_band_rows.restype = ci
if hasattr(lib, "orbhip_extractor_desc_plan"):       # (tools/ab_so.sh swaps older builds of the library in)
    lib.orbhip_extractor_desc_plan.argtypes = [vp, ci, vp, vp, C.POINTER(ci)]
if hasattr(lib, "orbhip_debug_octree"):              # (tools/ab_so.sh swaps older builds of the library in)
    lib.orbhip_debug_octree.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, ci, vp, vp]
lib.orbhip_prev_matched_init_device.argtypes = [vp, vp, sz, ci, ci, vp]
lib.orbhip_search_by_projection_device.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, sz, ci, cf, cf, cf, cf, ci, ci, vp, vp]
lib.orbhip_search_local_map_device.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, sz, ci, cf, cf, cf, cf, ci, cf, vp, vp]


class OrbHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed: %d (%s)" % (where, code, lib.orbhip_last_error().decode()))


def _chk(rc, where):
    if rc != OK:
        raise OrbHipError(rc, where)


class Context:
    def __init__(self, device=0, stream=None):
        h = vp()
        _chk(lib.orbhip_ctx_create(device, stream, C.byref(h)), "orbhip_ctx_create")
        self.h = h

    def synchronize(self):
        _chk(lib.orbhip_ctx_synchronize(self.h), "orbhip_ctx_synchronize")

    def check_status(self):
        _chk(lib.orbhip_ctx_check_status(self.h), "orbhip_ctx_check_status")

    def wait_for(self, other):
        """work submitted to this context from now on starts after everything submitted to `other` so far (no host synchronisation)"""
        _chk(lib.orbhip_ctx_wait_for(self.h, other.h), "orbhip_ctx_wait_for")

    @property
    def stream(self):
        return lib.orbhip_ctx_stream(self.h)

    def close(self):
        if self.h:
            lib.orbhip_ctx_destroy(self.h)
            self.h = None


def blur_half_widths():
    """per patch row |dy| = 0 .. 18: the half-width of the columns the rBRIEF pattern can sample (no device needed)"""
    out = np.zeros(19, np.int32)
    _chk(lib.orbhip_blur_half_widths(out.ctypes.data), "orbhip_blur_half_widths")
    return out


def fast_cell_table(widths, heights):
    """the FAST stage's cell table for the given per-level image sizes, decoded: int32 [cells][12] = level, x0, y0, dw, dh, key_x0, key_y0,
    list offset, tpr, rpt, magic, cell_cap (no device needed)"""
    w = np.ascontiguousarray(widths, np.int32)
    h = np.ascontiguousarray(heights, np.int32)
    n = lib.orbhip_fast_cell_table(len(w), w.ctypes.data, h.ctypes.data, None, 0)
    _chk(min(n, 0), "orbhip_fast_cell_table")
    out = np.zeros((n, 12), np.int32)
    _chk(min(lib.orbhip_fast_cell_table(len(w), w.ctypes.data, h.ctypes.data, out.ctypes.data, n), 0), "orbhip_fast_cell_table")
    return out


class Extractor:
    """Mirror of ORB_SLAM3::ORBextractor (reference include/ORBextractor.h:49-81)."""

    def __init__(self, ctx, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
        h = vp()
        _chk(lib.orbhip_extractor_create(ctx.h, nfeatures, scale_factor, nlevels, ini_th, min_th, C.byref(h)),
             "orbhip_extractor_create")
        self.h, self.ctx, self.nlevels = h, ctx, nlevels

    def close(self):
        if self.h:
            lib.orbhip_extractor_destroy(self.h)
            self.h = None

    # -- tables (GetScaleFactors etc.)
    def table(self, which):
        out = np.zeros(self.nlevels, np.float32)
        _chk(lib.orbhip_extractor_table(self.h, which, out.ctypes.data), "orbhip_extractor_table")
        return out

    def features_per_level(self):
        out = np.zeros(self.nlevels, np.int32)
        _chk(lib.orbhip_extractor_features_per_level(self.h, out.ctypes.data), "features_per_level")
        return out

    def umax(self):
        out = np.zeros(16, np.int32)
        _chk(lib.orbhip_extractor_umax(self.h, out.ctypes.data), "umax")
        return out

    def reserve(self, w, h, batch):
        _chk(lib.orbhip_extractor_reserve(self.h, w, h, batch), "orbhip_extractor_reserve")

    @property
    def max_keypoints(self):
        return lib.orbhip_extractor_max_keypoints(self.h)

    def blur_kernel(self, batch):
        """the kernel that blurs a batch of that many frames: 'k_blur' (LDS tiles), 'k_blur_rows' or 'k_blur_mfma'"""
        return ("k_blur", "k_blur_rows", "k_blur_mfma")[lib.orbhip_extractor_blur_kernel(self.h, int(batch))]

    def fast_kernel(self):
        """the instance of the per-cell FAST stage after reserve: 0 large cells, 1 small cells, 2 k_fast_runs<4>, 3 k_fast_runs<6>"""
        return lib.orbhip_extractor_fast_kernel(self.h)

    def blur_tiled(self, batch):
        """True when a batch of that many frames keeps the blurred pyramid in 16 x 8-pixel tiles (blurred_level de-tiles)"""
        return lib.orbhip_extractor_blur_tiled(self.h, int(batch)) == 1

    def desc_plan(self, batch):
        """(kp_base[nlevels], kp_cap[nlevels], waves per XCD) of the descriptor kernel for a call of that many frames (orbhip.h)"""
        base, cap, waves = np.zeros(self.nlevels, np.int32), np.zeros(self.nlevels, np.int32), ci()
        _chk(lib.orbhip_extractor_desc_plan(self.h, int(batch), base.ctypes.data, cap.ctypes.data, C.byref(waves)), "desc_plan")
        return base, cap, waves.value

    def resize_band_rows(self, level):
        """output rows per band of the row-streaming pyramid kernel at that level (0: the level takes the tile kernel)"""
        return lib.orbhip_extractor_resize_band_rows(self.h, int(level))

    def debug_octree(self, level, lists, form):
        """Test entry: the octree stage alone on caller-supplied candidate lists of one level.  lists = [(xs, ys, scores), ...], one per frame,
        coordinates relative to the detection area; form 'iterative' or 'table'.  Returns ([kept (n, 3) int32 rows x, y, score in list order per
        frame], [1 where the table form handed the list to the iterative form])."""
        offs = np.zeros(len(lists) + 1, np.int32)
        offs[1:] = np.cumsum([len(l[0]) for l in lists])
        xs, ys, ss = (np.ascontiguousarray(np.concatenate([np.asarray(l[k], np.int32) for l in lists] + [np.zeros(1, np.int32)])) for k in range(3))
        cap = int(max(len(l[0]) for l in lists)) + 16
        keys = np.zeros((len(lists), cap), np.uint32)
        counts, redo = np.zeros(len(lists), np.int32), np.zeros(len(lists), np.int32)
        _chk(lib.orbhip_debug_octree(self.h, int(level), len(lists), offs.ctypes.data, xs.ctypes.data, ys.ctypes.data, ss.ctypes.data,
                                     {"iterative": 0, "table": 1}[form], keys.ctypes.data, cap, counts.ctypes.data, redo.ctypes.data),
             "orbhip_debug_octree")
        kept = [np.stack([k & 0xFFF, (k >> 12) & 0xFFF, k >> 24], 1).astype(np.int32) for k in (keys[f, :counts[f]] for f in range(len(lists)))]
        return kept, redo.tolist()

    def set_graph_mode(self, on):
        _chk(lib.orbhip_extractor_set_graph_mode(self.h, 1 if on else 0), "orbhip_extractor_set_graph_mode")

    def set_profiling(self, on):
        _chk(lib.orbhip_extractor_set_profiling(self.h, 1 if on else 0), "set_profiling")

    def stage_ms(self):
        out = np.zeros(len(STAGES), np.float32)
        _chk(lib.orbhip_extractor_stage_ms(self.h, out.ctypes.data), "stage_ms")
        return dict(zip(STAGES, out.tolist()))

    # -- operator()
    def extract_host(self, images, lap=(0, 1000)):
        """images: uint8 [B,H,W] (or [H,W]).  Returns list of (kp structured array, desc [n,32], mono_index)."""
        img = np.ascontiguousarray(images, np.uint8)
        if img.ndim == 2:
            img = img[None]
        B, H, W = img.shape
        self.reserve(W, H, B)
        cap = self.max_keypoints
        kp = np.zeros((B, cap), KP_DTYPE)
        desc = np.zeros((B, cap, 32), np.uint8)
        cnt = np.zeros(B, np.int32)
        mono = np.zeros(B, np.int32)
        _chk(lib.orbhip_extract_batch_host(self.h, img.ctypes.data, W, H, W, W * H, B, lap[0], lap[1],
                                           kp.ctypes.data, desc.ctypes.data, cap, cnt.ctypes.data, mono.ctypes.data),
             "orbhip_extract_batch_host")
        return [(kp[f, :cnt[f]].copy(), desc[f, :cnt[f]].copy(), int(mono[f])) for f in range(B)]

    def extract_device(self, d_ptr, w, h, row_stride, frame_stride, batch, lap=(0, 1000)):
        _chk(lib.orbhip_extract_batch_device(self.h, d_ptr, w, h, row_stride, frame_stride, batch, lap[0], lap[1]),
             "orbhip_extract_batch_device")

    def results_device(self):
        a, b, c, d = vp(), vp(), vp(), vp()
        _chk(lib.orbhip_extractor_results(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "results")
        return a.value, b.value, c.value, d.value

    # -- taps
    def level_dims(self, level):
        w, h = ci(), ci()
        _chk(lib.orbhip_extractor_level_dims(self.h, level, C.byref(w), C.byref(h)), "level_dims")
        return w.value, h.value

    def pyramid_level(self, frame, level, padded=False):
        w, h = self.level_dims(level)
        if padded:
            w, h = w + 38, h + 38
        out = np.zeros((h, w), np.uint8)
        _chk(lib.orbhip_extractor_get_pyramid_level(self.h, frame, level, 1 if padded else 0, out.ctypes.data, w),
             "get_pyramid_level")
        return out

    def pyramid_padded(self, frame):
        """All levels as (w+38) x (h+38) reflect-101 padded parents (what mvImagePyramid's ROI views live in)."""
        outs = [np.zeros((h + 38, w + 38), np.uint8) for w, h in (self.level_dims(l) for l in range(self.nlevels))]
        ptrs = (vp * self.nlevels)(*[o.ctypes.data for o in outs])
        strides = (C.c_size_t * self.nlevels)(*[o.shape[1] for o in outs])
        _chk(lib.orbhip_extractor_get_pyramid_padded(self.h, frame, ptrs, strides), "get_pyramid_padded")
        return outs

    def blurred_level(self, frame, level):
        w, h = self.level_dims(level)
        out = np.zeros((h, w), np.uint8)
        _chk(lib.orbhip_extractor_get_blurred_level(self.h, frame, level, out.ctypes.data, w), "get_blurred_level")
        return out

    def fast_candidates(self, frame, level, cap=1 << 17):
        xs, ys, ss = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int32()
        _chk(lib.orbhip_extractor_get_fast_candidates(self.h, frame, level, xs.ctypes.data, ys.ctypes.data,
                                                      ss.ctypes.data, cap, C.byref(n)), "get_fast_candidates")
        return xs[:n.value].copy(), ys[:n.value].copy(), ss[:n.value].copy()

    def level_keypoints(self, frame, level, cap=8192):
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_int32()
        _chk(lib.orbhip_extractor_get_level_keypoints(self.h, frame, level, out.ctypes.data, cap, C.byref(n)),
             "get_level_keypoints")
        return out[:n.value].copy()


def match_bf2nn_device(ctx, d_descA, d_nA, strideA, d_descB, d_nB, strideB, pairs, max_n, ratio, d_idx2, d_dist2,
                       d_accept):
    """Frame.cc:1146-1153 semantics, batched; all pointers are device addresses (ints)."""
    _chk(lib.orbhip_match_bf2nn_device(ctx.h, d_descA, d_nA, strideA, d_descB, d_nB, strideB, pairs, max_n, ratio,
                                       d_idx2, d_dist2, d_accept), "orbhip_match_bf2nn_device")


def search_for_initialization_device(ctx, d_kpA, d_descA, d_nA, d_kpB, d_descB, d_nB, pairs, max_n, kp_stride, bounds,
                                     window, nn_ratio, check_ori, d_prev, d_m12, d_nmatches):
    """ORBmatcher::SearchForInitialization, batched; all pointers are device addresses (ints)."""
    _chk(lib.orbhip_search_for_initialization_device(ctx.h, d_kpA, d_descA, d_nA, d_kpB, d_descB, d_nB, pairs, max_n,
                                                     kp_stride, bounds[0], bounds[1], bounds[2], bounds[3], window,
                                                     nn_ratio, 1 if check_ori else 0, d_prev, d_m12, d_nmatches),
         "orbhip_search_for_initialization_device")


# one projected map point of ORBmatcher::SearchByProjection (include/orbhip.h: orbhip_proj_query)
PROJ_QUERY_DTYPE = np.dtype([("u", np.float32), ("v", np.float32), ("radius", np.float32), ("ur", np.float32),
                             ("angle", np.float32), ("min_level", np.int32), ("max_level", np.int32), ("has_obs", np.int32)])


def search_by_projection_device(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n, kp_stride, pairs,
                                bounds, th_high, check_ori, d_train_match, d_nmatches):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), batched; device addresses (ints)."""
    _chk(lib.orbhip_search_by_projection_device(ctx.h, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n,
                                                kp_stride, pairs, bounds[0], bounds[1], bounds[2], bounds[3], th_high,
                                                1 if check_ori else 0, d_train_match, d_nmatches),
         "orbhip_search_by_projection_device")


def search_local_map_device(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n, kp_stride, pairs,
                            bounds, th_high, nn_ratio, d_train_match, d_nmatches):
    """ORBmatcher::SearchByProjection(F, vpMapPoints, th) (TrackLocalMap), batched; device addresses (ints)."""
    _chk(lib.orbhip_search_local_map_device(ctx.h, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n,
                                            kp_stride, pairs, bounds[0], bounds[1], bounds[2], bounds[3], th_high,
                                            nn_ratio, d_train_match, d_nmatches), "orbhip_search_local_map_device")


lib.orbhip_debug_sbp_handed_back.argtypes = [vp, vp, ci, vp]


def debug_sbp_handed_back(ctx, cap=1 << 16):
    """Diagnostic: per pair of the context's last SearchByProjection launch, 1 where the replay form handed the pair to the sequential
    kernel; an empty array when that launch ran the sequential kernel alone.  Waits for the context's stream."""
    flags = np.zeros(max(cap, 1), np.int32); pairs = C.c_int(0)
    _chk(lib.orbhip_debug_sbp_handed_back(ctx.h, flags.ctypes.data, cap, C.byref(pairs)), "orbhip_debug_sbp_handed_back")
    return flags[:min(pairs.value, cap)].copy()


def prev_matched_init_device(ctx, d_kp, kp_stride, frames, max_n, d_prev):
    _chk(lib.orbhip_prev_matched_init_device(ctx.h, d_kp, kp_stride, frames, max_n, d_prev), "orbhip_prev_matched_init_device")


def descriptor_distance(a, b):
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    return lib.orbhip_descriptor_distance(a.ctypes.data, b.ctypes.data)


# ---------------------------------------------------------------- synthetic inputs (host C)
_synth = None


def synth_lib():
    global _synth
    if _synth is None:
        _synth = C.CDLL(SYNTH_PATH)
        _synth.synth_frame.argtypes = [vp, ci, ci, ci, C.c_uint64, ci]
        _synth.synth_batch.argtypes = [vp, ci, ci, ci, C.c_uint64, ci]
        _synth.synth_frame_transform.argtypes = [C.c_uint64, ci, C.POINTER(cf), C.POINTER(cf), C.POINTER(cf)]
    return _synth


def synth_frames(w, h, n, seed=20241004, first=0):
    out = np.zeros((n, h, w), np.uint8)
    synth_lib().synth_batch(out.ctypes.data, w, h, n, seed, first)
    return out


# ---------------------------------------------------------------- local BA (Optimizer::LocalBundleAdjustment core)
def rig2_fields(g):
    """Trl, fx2, fy2, cx2, cy2, camera2_model, kb2 of a graph dict (g.get('rig2') = dict(Trl, cam=(fx,fy,cx,cy), kb or None))."""
    r = g.get("rig2")
    if r is None:
        return ((cd * 7)(0, 0, 0, 0, 0, 0, 0), 0.0, 0.0, 0.0, 0.0, 0, (cd * 4)(0, 0, 0, 0))
    kb2 = r.get("kb")
    return ((cd * 7)(*r["Trl"]), *[float(c) for c in r["cam"]], 1 if kb2 is not None else 0, (cd * 4)(*(kb2 if kb2 is not None else (0, 0, 0, 0))))


class BaCamera(C.Structure):
    _fields_ = [("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("bf", cd), ("camera_model", C.c_int32), ("kb", cd * 4),
                ("Trl", cd * 7), ("fx2", cd), ("fy2", cd), ("cx2", cd), ("cy2", cd), ("camera2_model", C.c_int32), ("kb2", cd * 4)]


class BaGraph(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("pose_fixed", vp), ("edge_pose", vp), ("edge_point", vp), ("edge_obs", vp),
                ("edge_inv_sigma2", vp), ("edge_stereo", vp),
                ("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("bf", cd),
                ("camera_model", C.c_int32), ("kb", cd * 4),
                ("Trl", cd * 7), ("fx2", cd), ("fy2", cd), ("cx2", cd), ("cy2", cd), ("camera2_model", C.c_int32), ("kb2", cd * 4),
                ("n_cameras", C.c_int32), ("cameras", vp), ("pose_camera", vp)]


def camera_table(g, cls=None):
    """(n_cameras, array of camera structs or None, pose_camera array or None) of a graph dict (per-keyframe calibration, synth_ba.make_graph(cameras=...))."""
    cls = cls or BaCamera
    cams = g.get("cameras")
    if not cams:
        return 0, None, None
    arr = (cls * len(cams))()
    for i, c in enumerate(cams):
        kb = c.get("kb")
        arr[i] = cls(c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], 1 if kb is not None else 0, (cd * 4)(*(kb if kb is not None else (0, 0, 0, 0))),
                     *rig2_fields(dict(rig2=c.get("rig2"))))
    return len(cams), arr, np.ascontiguousarray(g["pose_camera"], np.int32)


class BaParams(C.Structure):
    _fields_ = [("iters1", C.c_int32), ("iters2", C.c_int32), ("huber_mono2", cd), ("huber_stereo2", cd),
                ("user_lambda_init", cd), ("tau", cd), ("max_trials", C.c_int32),
                ("stage2_exclude_outliers", C.c_int32), ("stage2_drop_robust", C.c_int32), ("no_discard", C.c_int32),
                ("gate_mono2", cd), ("gate_stereo2", cd)]


class BaStats(C.Structure):
    _fields_ = [("iterations_run", C.c_int32 * 2), ("lm_trials", C.c_int32), ("n_outliers", C.c_int32),
                ("discarded", C.c_int32), ("chi2_initial", cd), ("chi2_final", cd)]

    def as_dict(self):
        return dict(iterations_run=list(self.iterations_run), lm_trials=self.lm_trials, n_outliers=self.n_outliers,
                    discarded=self.discarded, chi2_initial=self.chi2_initial, chi2_final=self.chi2_final)


lib.orbhip_ba_default_params.argtypes = [C.POINTER(BaParams)]
lib.orbhip_ba_merge_params.argtypes = [C.POINTER(BaParams)]
lib.orbhip_ba_batch_create.argtypes = [vp, vp, ci, vp, vp, C.POINTER(vp)]
lib.orbhip_ba_batch_solve.argtypes = [vp, C.POINTER(BaParams), vp]
lib.orbhip_ba_batch_download.argtypes = [vp, vp, vp, vp, vp]
lib.orbhip_ba_batch_ticks.argtypes = [vp]
lib.orbhip_ba_batch_destroy.argtypes = [vp]
lib.orbhip_ba_solve_batch.argtypes = [vp, vp, ci, C.POINTER(BaParams), vp, vp, vp, vp, vp]
lib.orbhip_ba_batch_set_profiling.argtypes = [vp, ci]
lib.orbhip_ba_batch_gemm_profile.argtypes = [vp, C.POINTER(cf), C.POINTER(ci), C.POINTER(cd)]
lib.orbhip_mfma_f64_peak_tflops.argtypes = [vp, C.POINTER(cd)]
lib.orbhip_ba_batch_gemm_dense_flops.argtypes = [vp]
lib.orbhip_ba_batch_gemm_issued_flops.argtypes = [vp]
lib.orbhip_ba_batch_gemm_issued_flops.restype = cd
lib.orbhip_ba_batch_gemm_dense_flops.restype = cd


def mfma_f64_peak_tflops(ctx):
    v = cd()
    _chk(lib.orbhip_mfma_f64_peak_tflops(ctx.h, C.byref(v)), "orbhip_mfma_f64_peak_tflops")
    return v.value


lib.orbhip_ctx_set_ba_schur_mode.argtypes = [vp, ci]


def ba_set_schur_mode(ctx, mode):
    """0 / 1 = pair lists (default), 2 = FP64-MFMA panel GEMM; a property of the context, read when a batch is created on it."""
    _chk(lib.orbhip_ctx_set_ba_schur_mode(ctx.h, mode), "orbhip_ctx_set_ba_schur_mode")


def ba_merge_params():
    """Parameters of the map-merge local BA (Optimizer.cc:6255)."""
    p = BaParams()
    lib.orbhip_ba_merge_params(C.byref(p))
    return p


def ba_global_params(iterations, robust=True):
    """Optimizer::BundleAdjustment / GlobalBundleAdjustemnt parameters (one optimize(iterations) pass)."""
    p = BaParams()
    lib.orbhip_ba_global_params(C.byref(p), iterations, 1 if robust else 0)
    return p


def ba_default_params():
    p = BaParams()
    lib.orbhip_ba_default_params(C.byref(p))
    return p


BA_EXCHANGE_FN = C.CFUNCTYPE(ci, vp, ci, C.c_size_t)
lib.orbhip_ba_batch_exchange_doubles.restype = C.c_size_t
lib.orbhip_ba_batch_exchange_doubles.argtypes = [vp]
lib.orbhip_ba_batch_set_exchange_buffer.argtypes = [vp, vp, C.c_size_t]
lib.orbhip_ba_batch_solve_sharded.argtypes = [vp, vp, vp, BA_EXCHANGE_FN, vp]
lib.orbhip_ba_batch_create_sharded.argtypes = [vp, vp, ci, vp, vp, ci, ci, vp]


class BaBatch:
    """Device-resident batch of keyframe-window graphs (dicts as produced by synth_ba.make_graph:
    n_poses, n_points, n_edges, pose_fixed, edge_pose, edge_point, edge_obs, edge_inv_sigma2,
    edge_stereo, fx, fy, cx, cy, bf, poses0, points0)."""

    def __init__(self, ctx, graphs, rank=0, world=1):
        """world > 1: landmark-sharded batch (orbhip_ba_batch_create_sharded): every rank passes the same graphs."""
        self.ctx, self.n = ctx, len(graphs)
        self.rank, self.world = rank, world
        self._keep = []
        arr = (BaGraph * self.n)()
        self.sizes = []
        for i, g in enumerate(graphs):
            k = [np.ascontiguousarray(g["pose_fixed"], np.uint8), np.ascontiguousarray(g["edge_pose"], np.int32),
                 np.ascontiguousarray(g["edge_point"], np.int32), np.ascontiguousarray(g["edge_obs"], np.float64),
                 np.ascontiguousarray(g["edge_inv_sigma2"], np.float64), np.ascontiguousarray(g["edge_stereo"], np.uint8)]
            self._keep.append(k)
            kb = g.get("kb")                      # KannalaBrandt8 k1..k4 for the monocular edges, None = Pinhole
            ncam, cam_arr, pcam = camera_table(g)
            self._keep_cam = getattr(self, "_keep_cam", []) + [(cam_arr, pcam)]
            arr[i] = BaGraph(g["n_poses"], g["n_points"], g["n_edges"], *[a.ctypes.data for a in k],
                             g["fx"], g["fy"], g["cx"], g["cy"], g["bf"], 1 if kb is not None else 0,
                             (cd * 4)(*(kb if kb is not None else (0, 0, 0, 0))), *rig2_fields(g),
                             ncam, C.cast(cam_arr, vp) if ncam else None, pcam.ctypes.data if ncam else None)
            self.sizes.append((g["n_poses"], g["n_points"], g["n_edges"]))
        self.poses = [np.ascontiguousarray(g["poses0"], np.float64).copy() for g in graphs]
        self.points = [np.ascontiguousarray(g["points0"], np.float64).copy() for g in graphs]
        pp = (vp * self.n)(*[a.ctypes.data for a in self.poses])
        pq = (vp * self.n)(*[a.ctypes.data for a in self.points])
        h = vp()
        if world == 1:
            _chk(lib.orbhip_ba_batch_create(ctx.h, C.cast(arr, vp), self.n, C.cast(pp, vp), C.cast(pq, vp), C.byref(h)),
                 "orbhip_ba_batch_create")
        else:
            _chk(lib.orbhip_ba_batch_create_sharded(ctx.h, C.cast(arr, vp), self.n, C.cast(pp, vp), C.cast(pq, vp), rank, world,
                                                    C.byref(h)), "orbhip_ba_batch_create_sharded")
        self.h = h

    @property
    def exchange_doubles(self):
        """Doubles per rank slot of the exchange buffer (sharded batches)."""
        return lib.orbhip_ba_batch_exchange_doubles(self.h)

    def set_exchange_buffer(self, d_ptr, capacity_doubles):
        _chk(lib.orbhip_ba_batch_set_exchange_buffer(self.h, d_ptr, capacity_doubles), "orbhip_ba_batch_set_exchange_buffer")

    def solve_sharded(self, exchange, params=None, abort=None):
        """exchange(stage, count) -> None: all-gather `count` doubles per rank inside the exchange buffer (slot r = rank r)."""
        p = params or ba_default_params()
        err = []

        def _cb(user, stage, count):
            try:
                exchange(int(stage), int(count))
                return 0
            except BaseException as e:          # never let an exception cross the C boundary
                err.append(e)
                return 1
        cb = BA_EXCHANGE_FN(_cb)
        rc = lib.orbhip_ba_batch_solve_sharded(self.h, C.byref(p), abort.ctypes.data if abort is not None else None, cb, None)
        if err:
            raise err[0]
        if rc not in (OK, E_ABORTED):
            raise OrbHipError(rc, "orbhip_ba_batch_solve_sharded")
        return rc

    def solve(self, params=None, abort=None):
        p = params or ba_default_params()
        rc = lib.orbhip_ba_batch_solve(self.h, C.byref(p), abort.ctypes.data if abort is not None else None)
        if rc not in (OK, E_ABORTED):
            raise OrbHipError(rc, "orbhip_ba_batch_solve")
        return rc

    @property
    def ticks(self):
        return lib.orbhip_ba_batch_ticks(self.h)

    def set_graph_mode(self, on):
        _chk(lib.orbhip_extractor_set_graph_mode(self.h, 1 if on else 0), "orbhip_extractor_set_graph_mode")

    def set_profiling(self, on):
        _chk(lib.orbhip_ba_batch_set_profiling(self.h, 1 if on else 0), "ba set_profiling")

    def gemm_profile(self):
        ms, n, fl = cf(), ci(), cd()
        _chk(lib.orbhip_ba_batch_gemm_profile(self.h, C.byref(ms), C.byref(n), C.byref(fl)), "ba gemm_profile")
        return ms.value, n.value, fl.value

    def gemm_dense_flops(self):
        return lib.orbhip_ba_batch_gemm_dense_flops(self.h)

    def gemm_issued_flops(self):
        return lib.orbhip_ba_batch_gemm_issued_flops(self.h)

    def download(self):
        poses = [a.copy() for a in self.poses]
        points = [a.copy() for a in self.points]
        outl = [np.zeros(max(s[2], 1), np.uint8) for s in self.sizes]
        stats = (BaStats * self.n)()
        pp = (vp * self.n)(*[a.ctypes.data for a in poses])
        pq = (vp * self.n)(*[a.ctypes.data for a in points])
        po = (vp * self.n)(*[a.ctypes.data for a in outl])
        _chk(lib.orbhip_ba_batch_download(self.h, C.cast(pp, vp), C.cast(pq, vp), C.cast(po, vp), C.cast(stats, vp)),
             "orbhip_ba_batch_download")
        return poses, points, [o[:s[2]] for o, s in zip(outl, self.sizes)], [st.as_dict() for st in stats]

    def close(self):
        if self.h:
            lib.orbhip_ba_batch_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------------------------------------- inertial local BA
class IbaWindow(C.Structure):
    """orbhip_iba_window (include/orbhip.h): the flat description of one Optimizer::LocalInertialBA window."""
    _fields_ = [("n_kf", C.c_int32), ("kf_fixed", vp), ("kf_imu", vp), ("Rcb", cd * 9), ("tcb", cd * 3),
                ("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("bf", cd),
                ("camera_model", C.c_int32), ("kb", cd * 4), ("has_cam2", C.c_int32), ("Trl", cd * 12),
                ("fx2", cd), ("fy2", cd), ("cx2", cd), ("cy2", cd), ("camera2_model", C.c_int32), ("kb2", cd * 4),
                ("n_points", C.c_int32), ("n_edges", C.c_int32), ("edge_kf", vp), ("edge_point", vp), ("edge_obs", vp),
                ("edge_stereo", vp), ("edge_inv_sigma2", vp), ("edge_close", vp),
                ("n_inertial", C.c_int32), ("in_kf1", vp), ("in_kf2", vp), ("in_preint", vp), ("in_info", vp),
                ("in_info_g", vp), ("in_info_a", vp), ("in_robust", vp)]


class IbaParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("lambda_init", cd), ("large", C.c_int32), ("max_trials", C.c_int32)]


class IbaStats(C.Structure):
    _fields_ = [("iterations_run", C.c_int32), ("lm_trials", C.c_int32), ("n_outliers", C.c_int32), ("failed", C.c_int32),
                ("err", cd), ("err_end", cd)]

    def as_dict(self):
        return dict(iterations_run=self.iterations_run, lm_trials=self.lm_trials, n_outliers=self.n_outliers, failed=self.failed,
                    err=self.err, err_end=self.err_end)


IBA_KF, IBA_PREINT = 21, 67
lib.orbhip_iba_default_params.argtypes = [C.POINTER(IbaParams), ci]
lib.orbhip_inertial_ba_solve_batch.argtypes = [vp, vp, ci, C.POINTER(IbaParams), vp, vp, vp, vp]


def iba_default_params(large=False):
    p = IbaParams()
    lib.orbhip_iba_default_params(C.byref(p), 1 if large else 0)
    return p


def inertial_ba_solve_batch(ctx, windows, kf_states, points, params=None):
    """windows: list of IbaWindow (their arrays kept alive by the caller); kf_states[w] float64 [n_kf, 21], points[w] float64
    [n_points, 3] -> (kf_states, points, edge_outlier, stats) as new arrays (inputs untouched)."""
    n = len(windows)
    p = params or iba_default_params()
    arr = (IbaWindow * n)(*windows)
    kfs = [np.ascontiguousarray(a, np.float64).copy() for a in kf_states]
    pts = [np.ascontiguousarray(a, np.float64).copy() for a in points]
    outl = [np.zeros(max(w.n_edges, 1), np.uint8) for w in windows]
    stats = (IbaStats * n)()
    pk = (vp * n)(*[a.ctypes.data for a in kfs])
    pq = (vp * n)(*[a.ctypes.data for a in pts])
    po = (vp * n)(*[a.ctypes.data for a in outl])
    _chk(lib.orbhip_inertial_ba_solve_batch(ctx.h, C.cast(arr, vp), n, C.byref(p), C.cast(pk, vp), C.cast(pq, vp), C.cast(po, vp),
                                            C.cast(stats, vp)), "orbhip_inertial_ba_solve_batch")
    return kfs, pts, [o[:w.n_edges] for o, w in zip(outl, windows)], [st.as_dict() for st in stats]


class FibaParams(C.Structure):
    """orbhip_fiba_params: Optimizer::FullInertialBA's schedule."""
    _fields_ = [("iterations", C.c_int32), ("lambda_init", cd), ("max_trials", C.c_int32), ("shared_bias", C.c_int32),
                ("prior_g", cd), ("prior_a", cd)]


class FibaStats(C.Structure):
    _fields_ = [("iterations_run", C.c_int32), ("lm_trials", C.c_int32), ("end_reason", C.c_int32), ("n_unknowns", C.c_int32),
                ("chi2_first", cd), ("chi2_last", cd), ("lam", cd)]

    def as_dict(self):
        return dict(iterations_run=self.iterations_run, lm_trials=self.lm_trials, end_reason=self.end_reason,
                    n_unknowns=self.n_unknowns, chi2_first=self.chi2_first, chi2_last=self.chi2_last, lam=self.lam)


FIBA_END_ITERATIONS, FIBA_END_TRIALS, FIBA_END_NBAD = 0, 1, 2
lib.orbhip_fiba_default_params.argtypes = [C.POINTER(FibaParams), ci, ci, cd, cd]
lib.orbhip_full_inertial_ba_solve_batch.argtypes = [vp, vp, ci, C.POINTER(FibaParams), vp, vp, vp, vp, vp]


def fiba_default_params(its=200, b_init=False, prior_g=1e2, prior_a=1e6):
    """The reference passes the priors as floats (Optimizer.h:55)."""
    p = FibaParams()
    lib.orbhip_fiba_default_params(C.byref(p), int(its), 1 if b_init else 0, float(np.float32(prior_g)), float(np.float32(prior_a)))
    return p


def full_inertial_ba_solve_batch(ctx, maps, kf_states, points, shared_bias=None, params=None, stop=None):
    """maps: list of IbaWindow (arrays kept alive by the caller); kf_states[m] float64 [n_kf, 21], points[m] float64 [n_points, 3],
    shared_bias float64 [n_maps, 6] (shared mode), stop: None or a uint8 array of one element read once before the launch
    -> (kf_states, points, shared_bias, stats) as new arrays (inputs untouched)."""
    n = len(maps)
    p = params or fiba_default_params()
    arr = (IbaWindow * max(n, 1))(*maps)
    kfs = [np.ascontiguousarray(a, np.float64).reshape(-1, IBA_KF).copy() for a in kf_states]
    pts = [np.ascontiguousarray(a, np.float64).reshape(-1, 3).copy() for a in points]
    sb = np.zeros((n, 6)) if shared_bias is None else np.ascontiguousarray(shared_bias, np.float64).reshape(n, 6).copy()
    stats = (FibaStats * max(n, 1))()
    pk = (vp * max(n, 1))(*[a.ctypes.data for a in kfs])
    pq = (vp * max(n, 1))(*[a.ctypes.data for a in pts])
    _chk(lib.orbhip_full_inertial_ba_solve_batch(ctx.h, C.cast(arr, vp), n, C.byref(p), stop.ctypes.data if stop is not None else None,
                                                 C.cast(pk, vp), C.cast(pq, vp), sb.ctypes.data, C.cast(stats, vp)),
         "orbhip_full_inertial_ba_solve_batch")
    return kfs, pts, sb, [stats[i].as_dict() for i in range(n)]


class PoseGraph(C.Structure):
    """orbhip_pose_graph: the Sim3 pose graph of Optimizer::OptimizeEssentialGraph (pointers to host arrays the caller keeps alive)."""
    _fields_ = [("n_vertices", C.c_int32), ("fixed", vp), ("n_edges", C.c_int32), ("edge_v0", vp), ("edge_v1", vp), ("edge_meas", vp)]


class PoseGraphParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("lambda_init", cd), ("fix_scale", C.c_int32), ("max_trials", C.c_int32)]


class PoseGraphStats(C.Structure):
    _fields_ = [("chi2_initial", cd), ("chi2_final", cd), ("lam", cd), ("iterations", C.c_int32), ("trials", C.c_int32),
                ("end_reason", C.c_int32), ("n_free", C.c_int32), ("n_unknowns", C.c_int32)]

    def as_dict(self):
        return dict(chi2_initial=self.chi2_initial, chi2_final=self.chi2_final, lam=self.lam, iterations=self.iterations, trials=self.trials,
                    end_reason=self.end_reason, n_free=self.n_free, n_unknowns=self.n_unknowns)


PG_END_ITERATIONS, PG_END_TERMINATE, PG_END_NBAD, PG_END_SOLVE_FAILED = 0, 1, 2, 3
PG_TRACE = 4
lib.orbhip_pose_graph_default_params.argtypes = [C.POINTER(PoseGraphParams)]
lib.orbhip_pose_graph_default_params.restype = None
lib.orbhip_optimize_essential_graph_host.argtypes = [vp, vp, ci, C.POINTER(PoseGraphParams), vp, vp, vp]
lib.orbhip_pose_graph_correct_points_device.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]
lib.orbhip_debug_pose_graph_last_path.argtypes = []
lib.orbhip_pose_graph_correct_points_host.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]


def pose_graph_default_params(iterations=None, fix_scale=None):
    p = PoseGraphParams()
    lib.orbhip_pose_graph_default_params(C.byref(p))
    if iterations is not None:
        p.iterations = int(iterations)
    if fix_scale is not None:
        p.fix_scale = 1 if fix_scale else 0
    return p


def optimize_essential_graph(ctx, graphs, sim3, params=None, trace=True):
    """graphs: list of dicts with fixed [V] uint8, edge_v0 / edge_v1 [E] int32, edge_meas [E, 8] float64 (Sji as qx qy qz qw tx ty tz s);
    sim3[g] float64 [V, 8] -> (optimised sim3 as new arrays, stats dicts, traces [trials, 4] = chi2, rho, lambda, accepted)."""
    n = len(graphs)
    p = params or pose_graph_default_params()
    keep, arr = [], (PoseGraph * max(n, 1))()
    for i, g in enumerate(graphs):
        fx = np.ascontiguousarray(g["fixed"], np.uint8)
        v0, v1 = np.ascontiguousarray(g["edge_v0"], np.int32), np.ascontiguousarray(g["edge_v1"], np.int32)
        ms = np.ascontiguousarray(g["edge_meas"], np.float64).reshape(-1, 8)
        keep.append((fx, v0, v1, ms))
        arr[i] = PoseGraph(len(fx), fx.ctypes.data, len(v0), v0.ctypes.data, v1.ctypes.data, ms.ctypes.data)
    est = [np.ascontiguousarray(a, np.float64).reshape(-1, 8).copy() for a in sim3]
    pe = (vp * max(n, 1))(*[a.ctypes.data for a in est])
    stats = (PoseGraphStats * max(n, 1))()
    cap = p.iterations * p.max_trials
    tr = np.zeros((n, cap, PG_TRACE)) if trace and cap > 0 else None
    _chk(lib.orbhip_optimize_essential_graph_host(ctx.h if ctx is not None else None, C.cast(arr, vp), n, C.byref(p), C.cast(pe, vp), C.cast(stats, vp),
                                                  tr.ctypes.data if tr is not None else None), "orbhip_optimize_essential_graph_host")
    st = [stats[i].as_dict() for i in range(n)]
    return est, st, [tr[i, :st[i]["trials"]].copy() for i in range(n)] if tr is not None else None


lib.orbhip_debug_pose_graph_dense_solve_host.argtypes = [vp, vp, ci, vp, vp, ci, C.POINTER(ci)]


def debug_pose_graph_dense_solve(ctx, S, rhs, x_out, force_big=False):
    """The pose graphs' dense solve chain alone on S x = rhs (S [n, n] float64, its lower triangle read): writes x_out [n] in place
    when every pivot was good, leaves it untouched otherwise -> ok (bool)."""
    S = np.ascontiguousarray(S, np.float64)
    rhs = np.ascontiguousarray(rhs, np.float64)
    n = int(rhs.shape[0])
    assert S.shape == (n, n) and x_out.dtype == np.float64 and x_out.shape == (n,) and x_out.flags.c_contiguous
    ok = ci(-1)
    _chk(lib.orbhip_debug_pose_graph_dense_solve_host(ctx.h, S.ctypes.data, n, rhs.ctypes.data, x_out.ctypes.data, 1 if force_big else 0, C.byref(ok)),
         "orbhip_debug_pose_graph_dense_solve_host")
    return ok.value != 0


lib.orbhip_debug_geom_probe_host.argtypes = [vp, ci, vp, ci, ci, vp, ci]
# name -> (id, in_width, out_width): the ORBHIP_GEOM_* ops of orbhip_debug_geom_probe_host, in the header's order
GEOM_OPS = {name: (i, w_in, w_out) for i, (name, w_in, w_out) in enumerate([
    ("quat_to_R", 4, 9), ("R_to_quat", 9, 4), ("quat_rot", 7, 3), ("quat_mul", 8, 4), ("quat_norm_rot", 4, 4), ("huber", 3, 2),
    ("se3_oplus", 13, 7), ("se3_mul", 14, 7), ("so3_exp", 3, 9), ("so3_exp_imu", 3, 9), ("so3_log", 9, 3), ("so3_right_jac", 3, 9),
    ("so3_inv_right_jac", 3, 9), ("so3_normalize", 9, 9), ("s3_exp", 7, 8), ("s3_log", 8, 7), ("s3_mul", 16, 8), ("s3_inverse", 8, 8),
    ("s3_map", 11, 3), ("cam_project", 12, 2), ("cam_project_jac", 12, 6), ("tri_project_pinhole", 11, 2), ("tri_project_kb8", 11, 2),
    ("tri_unproject_pinhole", 10, 3), ("tri_unproject_kb8", 10, 3), ("tri_svd4_null", 16, 4)])}


def debug_geom_probe(ctx, name, inputs, out=None, n=None):
    """One shared geometry primitive alone on the device: inputs [n, in_width] float64 -> [n, out_width] float64.  out: an array to
    write into (its rows past n stay as they are); n: fewer items than inputs has rows."""
    op, w_in, w_out = GEOM_OPS[name]
    x = np.ascontiguousarray(inputs, np.float64).reshape(-1, w_in)
    n = len(x) if n is None else int(n)
    assert n <= len(x)
    if out is None:
        out = np.empty((max(n, 0), w_out), np.float64)
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.size >= max(n, 0) * w_out
    _chk(lib.orbhip_debug_geom_probe_host(ctx.h, op, x.ctypes.data, n, w_in, out.ctypes.data, w_out), "orbhip_debug_geom_probe_host")
    return out


def pose_graph_correct_points_device(ctx, d_Xw, d_ref, n_points, d_Scw, d_corrected_Swc, n_vertices, d_Xw_out):
    _chk(lib.orbhip_pose_graph_correct_points_device(ctx.h, d_Xw, d_ref, n_points, d_Scw, d_corrected_Swc, n_vertices, d_Xw_out),
         "orbhip_pose_graph_correct_points_device")


class PoseGraph4DoF(C.Structure):
    """orbhip_pose_graph4dof: the yaw + translation pose graph of Optimizer::OptimizeEssentialGraph4DoF."""
    _fields_ = [("n_vertices", C.c_int32), ("fixed", vp), ("n_edges", C.c_int32), ("edge_v0", vp), ("edge_v1", vp), ("edge_meas", vp)]


class PoseGraph4DoFParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("lambda_init", cd), ("tau", cd), ("info_diag", cd * 6), ("max_trials", C.c_int32)]


PG4_STATE = 36
lib.orbhip_pose_graph4dof_default_params.argtypes = [C.POINTER(PoseGraph4DoFParams)]
lib.orbhip_pose_graph4dof_default_params.restype = None
lib.orbhip_optimize_essential_graph4dof_host.argtypes = [vp, vp, ci, C.POINTER(PoseGraph4DoFParams), vp, vp, vp]
lib.orbhip_debug_pose_graph4dof_last_path.argtypes = []


def pose_graph4dof_default_params(iterations=None, info_diag=None, lambda_init=None):
    p = PoseGraph4DoFParams()
    lib.orbhip_pose_graph4dof_default_params(C.byref(p))
    if iterations is not None:
        p.iterations = int(iterations)
    if info_diag is not None:
        for k in range(6):
            p.info_diag[k] = float(info_diag[k])
    if lambda_init is not None:
        p.lambda_init = float(lambda_init)
    return p


def optimize_essential_graph4dof(ctx, graphs, state, params=None, trace=True):
    """graphs: list of dicts with fixed [V] uint8, edge_v0 / edge_v1 [E] int32, edge_meas [E, 12] float64 (dRij row-major, dtij);
    state[g] float64 [V, 36] = Rwb, twb, Rcw, tcw, Rcb, tcb -> (optimised state as new arrays, stats dicts, traces [trials, 4])."""
    n = len(graphs)
    p = params or pose_graph4dof_default_params()
    keep, arr = [], (PoseGraph4DoF * max(n, 1))()
    for i, g in enumerate(graphs):
        fx = np.ascontiguousarray(g["fixed"], np.uint8)
        v0, v1 = np.ascontiguousarray(g["edge_v0"], np.int32), np.ascontiguousarray(g["edge_v1"], np.int32)
        ms = np.ascontiguousarray(g["edge_meas"], np.float64).reshape(-1, 12)
        keep.append((fx, v0, v1, ms))
        arr[i] = PoseGraph4DoF(len(fx), fx.ctypes.data, len(v0), v0.ctypes.data, v1.ctypes.data, ms.ctypes.data)
    est = [np.ascontiguousarray(a, np.float64).reshape(-1, PG4_STATE).copy() for a in state]
    pe = (vp * max(n, 1))(*[a.ctypes.data for a in est])
    stats = (PoseGraphStats * max(n, 1))()
    cap = p.iterations * p.max_trials
    tr = np.zeros((n, cap, PG_TRACE)) if trace and cap > 0 else None
    _chk(lib.orbhip_optimize_essential_graph4dof_host(ctx.h if ctx is not None else None, C.cast(arr, vp), n, C.byref(p), C.cast(pe, vp), C.cast(stats, vp),
                                                      tr.ctypes.data if tr is not None else None), "orbhip_optimize_essential_graph4dof_host")
    st = [stats[i].as_dict() for i in range(n)]
    return est, st, [tr[i, :st[i]["trials"]].copy() for i in range(n)] if tr is not None else None


lib.orbhip_iba_batch_create.argtypes = [vp, vp, ci, vp, vp, C.POINTER(vp)]
lib.orbhip_iba_batch_set_states.argtypes = [vp, vp, vp]
lib.orbhip_iba_batch_solve.argtypes = [vp, C.POINTER(IbaParams)]
lib.orbhip_iba_batch_download.argtypes = [vp, vp, vp, vp, vp]
lib.orbhip_iba_batch_destroy.argtypes = [vp]
lib.orbhip_iba_batch_destroy.restype = None


class IbaBatch:
    """orbhip_iba_batch: windows resident on the device; solve() re-solves them from the states last set."""

    def __init__(self, ctx, windows, kf_states, points):
        self.n = len(windows)
        self.shapes = [(w.n_kf, w.n_points, w.n_edges) for w in windows]
        arr = (IbaWindow * self.n)(*windows)
        kfs = [np.ascontiguousarray(a, np.float64) for a in kf_states]
        pts = [np.ascontiguousarray(a, np.float64) for a in points]
        pk = (vp * self.n)(*[a.ctypes.data for a in kfs])
        pq = (vp * self.n)(*[a.ctypes.data for a in pts])
        self.h = vp()
        _chk(lib.orbhip_iba_batch_create(ctx.h, C.cast(arr, vp), self.n, C.cast(pk, vp), C.cast(pq, vp), C.byref(self.h)),
             "orbhip_iba_batch_create")

    def set_states(self, kf_states, points):
        kfs = [np.ascontiguousarray(a, np.float64) for a in kf_states]
        pts = [np.ascontiguousarray(a, np.float64) for a in points]
        pk = (vp * self.n)(*[a.ctypes.data for a in kfs])
        pq = (vp * self.n)(*[a.ctypes.data for a in pts])
        _chk(lib.orbhip_iba_batch_set_states(self.h, C.cast(pk, vp), C.cast(pq, vp)), "orbhip_iba_batch_set_states")

    def solve(self, params=None):
        p = params or iba_default_params()
        _chk(lib.orbhip_iba_batch_solve(self.h, C.byref(p)), "orbhip_iba_batch_solve")

    def download(self):
        """-> (kf_states, points, edge_outlier, stats); a failed window's states come back as zeros (not written, as the one-shot call
        leaves its inputs alone)."""
        kfs = [np.zeros((s[0], IBA_KF)) for s in self.shapes]
        pts = [np.zeros((max(s[1], 1), 3)) for s in self.shapes]
        outl = [np.zeros(max(s[2], 1), np.uint8) for s in self.shapes]
        stats = (IbaStats * self.n)()
        pk = (vp * self.n)(*[a.ctypes.data for a in kfs])
        pq = (vp * self.n)(*[a.ctypes.data for a in pts])
        po = (vp * self.n)(*[a.ctypes.data for a in outl])
        _chk(lib.orbhip_iba_batch_download(self.h, C.cast(pk, vp), C.cast(pq, vp), C.cast(po, vp), C.cast(stats, vp)),
             "orbhip_iba_batch_download")
        return (kfs, [p[:s[1]] for p, s in zip(pts, self.shapes)], [o[:s[2]] for o, s in zip(outl, self.shapes)],
                [st.as_dict() for st in stats])

    def close(self):
        if self.h:
            lib.orbhip_iba_batch_destroy(self.h)
            self.h = None


def inertial_ba_last_team_size():
    """Workgroups per window of this thread's latest inertial solve (1 = no device-wide barrier)."""
    return int(lib.orbhip_inertial_ba_last_team_size())


class Camera2(C.Structure):
    _fields_ = [("Trl", cd * 7), ("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("camera_model", C.c_int32), ("kb", cd * 4)]


lib.orbhip_pose_optimization_device.argtypes = [vp, vp, vp, vp, vp, ci, ci, cd, cd, cd, cd, cd, vp, vp, vp, vp, vp, vp, vp]


def pose_optimization_device(ctx, d_Xw, d_obs, d_inv_sigma2, d_n_edges, frames, max_edges, cam, d_pose, d_outlier,
                             d_n_inliers, d_stats=None, kb8=None, rig2=None, d_right=None):
    """Optimizer::PoseOptimization, batched over frames; device addresses (ints); cam = (fx, fy, cx, cy, bf);
    kb8 = (k1..k4) for a KannalaBrandt8 camera (host values), None = Pinhole; rig2 = dict(Trl, cam, kb) + d_right
    (device address of per-edge flags) when some observations were made in a second, rigidly attached camera."""
    kb = (cd * 4)(*kb8) if kb8 is not None else None
    c2 = None
    if rig2 is not None:
        k2 = rig2.get("kb")
        c2 = C.byref(Camera2((cd * 7)(*rig2["Trl"]), *[float(c) for c in rig2["cam"]], 1 if k2 is not None else 0,
                             (cd * 4)(*(k2 if k2 is not None else (0, 0, 0, 0)))))
    _chk(lib.orbhip_pose_optimization_device(ctx.h, d_Xw, d_obs, d_inv_sigma2, d_n_edges, frames, max_edges,
                                             float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), float(cam[4]),
                                             kb, c2, d_right, d_pose, d_outlier, d_n_inliers, d_stats), "orbhip_pose_optimization_device")


lib.orbhip_compute_stereo_matches_device.argtypes = [vp, vp, cf, cf, vp, vp, vp]


def compute_stereo_matches_device(ext_left, ext_right, mb, mbf, d_u_right, d_depth, d_n_matches=None):
    """Frame::ComputeStereoMatches on the latest results of two extractors; device addresses (ints)."""
    _chk(lib.orbhip_compute_stereo_matches_device(ext_left.h, ext_right.h, mb, mbf, d_u_right, d_depth, d_n_matches),
         "orbhip_compute_stereo_matches_device")


lib.orbhip_compute_stereo_fisheye_matches_device.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, ci, ci, ci, vp, ci, vp, vp, vp, vp, ci,
                                                           vp, vp, vp, vp, vp]
lib.orbhip_compute_stereo_fisheye_matches_host.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, ci, vp]


def _f32(a, n):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    assert a.size >= n, (a.size, n)
    return a


def compute_stereo_fisheye_matches_device(ctx, left, right, batch, max_n, rig, level_sigma2, d_l2r, d_r2l, d_depth, d_x3d, d_n_matches):
    """Frame::ComputeStereoFishEyeMatches, batched.  left / right = (d_kp, d_desc, d_n, d_mono, stride) device addresses (ints);
    rig = dict(types=(t1, t2), cam1=[8], cam2=[8], Rlr=[3x3], tlr=[3]).  Outputs [batch][max_n] (x3d [batch][max_n][3])."""
    c1, c2, R, t, s2 = _f32(rig["cam1"], 8), _f32(rig["cam2"], 8), _f32(rig["Rlr"], 9), _f32(rig["tlr"], 3), _f32(level_sigma2, 1)
    _chk(lib.orbhip_compute_stereo_fisheye_matches_device(ctx.h, left[0], left[1], left[2], left[3], left[4], right[0], right[1], right[2],
                                                          right[3], right[4], batch, max_n, int(rig["types"][0]), c1.ctypes.data,
                                                          int(rig["types"][1]), c2.ctypes.data, R.ctypes.data, t.ctypes.data, s2.ctypes.data,
                                                          len(s2), d_l2r, d_r2l, d_depth, d_x3d, d_n_matches),
         "orbhip_compute_stereo_fisheye_matches_device")


def compute_stereo_fisheye_matches_host(ext_left, ext_right, n_left, n_right, rig, level_sigma2):
    """One frame on the two extractors' latest host extractions: (l2r [n_left], r2l [n_right], depth [n_left], x3d [n_left][3], n_matches)."""
    c1, c2, R, t, s2 = _f32(rig["cam1"], 8), _f32(rig["cam2"], 8), _f32(rig["Rlr"], 9), _f32(rig["tlr"], 3), _f32(level_sigma2, 1)
    l2r = np.zeros(max(n_left, 1), np.int32); r2l = np.zeros(max(n_right, 1), np.int32)
    depth = np.zeros(max(n_left, 1), np.float32); x3d = np.zeros((max(n_left, 1), 3), np.float32); nm = np.zeros(1, np.int32)
    _chk(lib.orbhip_compute_stereo_fisheye_matches_host(ext_left.h, ext_right.h, int(rig["types"][0]), c1.ctypes.data, int(rig["types"][1]),
                                                        c2.ctypes.data, R.ctypes.data, t.ctypes.data, s2.ctypes.data, len(s2), l2r.ctypes.data,
                                                        depth.ctypes.data, x3d.ctypes.data, n_left, r2l.ctypes.data, n_right, nm.ctypes.data),
         "orbhip_compute_stereo_fisheye_matches_host")
    return l2r[:n_left], r2l[:n_right], depth[:n_left], x3d[:n_left], int(nm[0])


lib.orbhip_distinctive_descriptors_device.argtypes = [vp, vp, vp, ci, ci, vp, vp]


def distinctive_descriptors_device(ctx, d_desc, d_n, points, max_n, d_best_idx, d_best_desc=None):
    """MapPoint::ComputeDistinctiveDescriptors, batched over map points; device addresses (ints)."""
    _chk(lib.orbhip_distinctive_descriptors_device(ctx.h, d_desc, d_n, points, max_n, d_best_idx, d_best_desc),
         "orbhip_distinctive_descriptors_device")


lib.orbhip_bow_transform_device.argtypes = [vp, vp, vp, ci, ci, sz, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]


def bow_transform_device(ctx, d_desc, d_n, frames, max_n, frame_stride, voc, L, levelsup, d_word_id, d_weight, d_nid):
    """DBoW2 per-feature tree descent; voc = (d_node_desc, d_child_start, d_child_ids, d_node_word, d_node_weight)."""
    _chk(lib.orbhip_bow_transform_device(ctx.h, d_desc, d_n, frames, max_n, frame_stride, voc[0], voc[1], voc[2], voc[3], voc[4],
                                         L, levelsup, d_word_id, d_weight, d_nid), "orbhip_bow_transform_device")


lib.orbhip_fuse_search_device.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, sz, ci, vp, ci, cf, cf, cf, cf, vp, vp]


def fuse_search_device(ctx, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n, kp_stride, pairs, inv_level_sigma2,
                       bounds, d_best_idx, d_best_dist):
    """Search part of ORBmatcher::Fuse, batched; device addresses (ints); inv_level_sigma2 = host float array."""
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    _chk(lib.orbhip_fuse_search_device(ctx.h, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_u_right, d_n, max_n, kp_stride, pairs,
                                       sig.ctypes.data, len(sig), bounds[0], bounds[1], bounds[2], bounds[3], d_best_idx, d_best_dist),
         "orbhip_fuse_search_device")


lib.orbhip_search_by_bow_kf_device.argtypes = [vp] * 17 + [ci, ci, ci, sz, cf, ci, vp, vp]


def search_by_bow_kf_device(ctx, kf1, kf2, pairs, max_nodes, max_n, kp_stride, nn_ratio, check_ori, d_matches12, d_nmatches):
    """ORBmatcher::SearchByBoW(KeyFrame, KeyFrame), batched.  kf1 / kf2 = (d_node_ids, d_node_start, d_feat, d_nnodes, d_valid, d_kp,
    d_desc, d_n): device addresses (ints)."""
    _chk(lib.orbhip_search_by_bow_kf_device(ctx.h, *kf1, *kf2, pairs, max_nodes, max_n, kp_stride, nn_ratio, 1 if check_ori else 0,
                                            d_matches12, d_nmatches), "orbhip_search_by_bow_kf_device")


lib.orbhip_undistort_keypoints_device.argtypes = [vp, vp, vp, ci, ci, sz, cf, cf, cf, cf, vp, ci, vp]
lib.orbhip_assign_features_to_grid_device.argtypes = [vp, vp, vp, ci, ci, sz, cf, cf, cf, cf, vp, vp]


def undistort_keypoints_device(ctx, d_kp, d_n, frames, max_n, kp_stride, K, dist, d_kp_un):
    """Frame::UndistortKeyPoints, batched.  K = (fx, fy, cx, cy); dist: 4 or 5 host floats."""
    dc = np.ascontiguousarray(dist, np.float32)
    _chk(lib.orbhip_undistort_keypoints_device(ctx.h, d_kp, d_n, frames, max_n, kp_stride, K[0], K[1], K[2], K[3], dc.ctypes.data, len(dc),
                                               d_kp_un), "orbhip_undistort_keypoints_device")


def assign_features_to_grid_device(ctx, d_kp, d_n, frames, max_n, kp_stride, bounds, d_cell_start, d_items):
    """Frame::AssignFeaturesToGrid as a CSR per frame (cell ix*48+iy)."""
    _chk(lib.orbhip_assign_features_to_grid_device(ctx.h, d_kp, d_n, frames, max_n, kp_stride, bounds[0], bounds[1], bounds[2], bounds[3],
                                                   d_cell_start, d_items), "orbhip_assign_features_to_grid_device")


lib.orbhip_bow_vectors_device.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]


def bow_vectors_device(ctx, d_wid, d_w, d_nid, d_n, frames, max_n, max_nodes, d_node_ids, d_node_start, d_feat, d_nnodes, d_bow_word,
                       d_bow_value, d_nwords):
    """mFeatVec (CSR) and mBowVec (sorted, L1-normalised) from bow_transform_device's per-feature output."""
    _chk(lib.orbhip_bow_vectors_device(ctx.h, d_wid, d_w, d_nid, d_n, frames, max_n, max_nodes, d_node_ids, d_node_start, d_feat, d_nnodes,
                                       d_bow_word, d_bow_value, d_nwords), "orbhip_bow_vectors_device")


TRI_PAIR_DTYPE = np.dtype([("F12", "<f4", (9,)), ("ep_x", "<f4"), ("ep_y", "<f4"), ("only_stereo", "<i4"), ("coarse", "<i4")])
lib.orbhip_search_for_triangulation_device.argtypes = [vp] * 17 + [ci, ci, ci, sz, vp, vp, ci, ci, vp, vp]


def search_for_triangulation_device(ctx, kf1, kf2, d_pair, pairs, max_nodes, max_n, kp_stride, scale_factors, level_sigma2,
                                    check_ori, d_matches12, d_nmatches):
    """ORBmatcher::SearchForTriangulation, batched.  kf1 = (d_nid, d_has_mp, d_kp, d_desc, d_u_right|0, d_n),
    kf2 = (d_node_ids, d_node_start, d_feat, d_nnodes, d_has_mp, d_kp, d_desc, d_u_right|0, d_n): device addresses (ints);
    d_pair: [pairs] TRI_PAIR_DTYPE records; scale_factors / level_sigma2: host float32 arrays."""
    sf = np.ascontiguousarray(scale_factors, np.float32); ls = np.ascontiguousarray(level_sigma2, np.float32)
    assert len(sf) == len(ls)
    _chk(lib.orbhip_search_for_triangulation_device(ctx.h, *[a or None for a in kf1], *[a or None for a in kf2], d_pair, pairs, max_nodes,
                                                    max_n, kp_stride, sf.ctypes.data, ls.ctypes.data, len(sf), 1 if check_ori else 0,
                                                    d_matches12, d_nmatches), "orbhip_search_for_triangulation_device")


TRI_GENERAL_DTYPE = np.dtype([("R12", "<f4", (4, 9)), ("t12", "<f4", (4, 3)), ("F12", "<f4", (4, 9)), ("cam1", "<f4", (2, 8)), ("cam2", "<f4", (2, 8)),
                              ("cam1_type", "<i4", (2,)), ("cam2_type", "<i4", (2,)), ("ep_x", "<f4"), ("ep_y", "<f4"), ("nleft1", "<i4"), ("nleft2", "<i4"),
                              ("only_stereo", "<i4"), ("coarse", "<i4")])
lib.orbhip_search_for_triangulation_general_device.argtypes = [vp] * 17 + [ci, ci, ci, sz, vp, vp, vp, ci, ci, vp, vp]


def search_for_triangulation_general_device(ctx, kf1, kf2, d_pair, pairs, max_nodes, max_n, kp_stride, level_sigma2_1, scale_factors2,
                                            level_sigma2_2, check_ori, d_matches12, d_nmatches):
    """ORBmatcher::SearchForTriangulation for every camera combination (Pinhole / KannalaBrandt8 / two-camera rigs), batched.  kf1 / kf2 as
    in search_for_triangulation_device; d_pair: [pairs] TRI_GENERAL_DTYPE records."""
    a = [np.ascontiguousarray(x, np.float32) for x in (level_sigma2_1, scale_factors2, level_sigma2_2)]
    assert len(a[0]) == len(a[1]) == len(a[2])
    _chk(lib.orbhip_search_for_triangulation_general_device(ctx.h, *[x or None for x in kf1], *[x or None for x in kf2], d_pair, pairs, max_nodes,
                                                            max_n, kp_stride, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, len(a[0]),
                                                            1 if check_ori else 0, d_matches12, d_nmatches),
         "orbhip_search_for_triangulation_general_device")


TRI_POSES_DTYPE = np.dtype([("Tcw1", "<f4", (2, 12)), ("Tcw2", "<f4", (2, 12))])
lib.orbhip_match_and_triangulate_device.argtypes = [vp] * 16 + [ci, ci, ci, sz, vp, vp, ci, ci, vp, vp, vp]


def match_and_triangulate_device(ctx, kf1, kf2, d_pair, d_poses, pairs, max_nodes, max_n, kp_stride, level_sigma2_1, level_sigma2_2, check_ori,
                                 d_matches12, d_points12, d_nmatches):
    """ORBmatcher::SearchForTriangulation(..., vMatchedPoints) (ORBmatcher.cc:1212-1402), batched.  kf1 = [nid1, has_mp1, kp1, desc1, n1],
    kf2 = [node_ids2, node_start2, feat2, nnodes2, has_mp2, kp2, desc2, n2] device pointers; d_poses: [pairs] TRI_POSES_DTYPE records."""
    a = [np.ascontiguousarray(x, np.float32) for x in (level_sigma2_1, level_sigma2_2)]
    assert len(a[0]) == len(a[1]) and len(kf1) == 5 and len(kf2) == 8
    _chk(lib.orbhip_match_and_triangulate_device(ctx.h, *kf1, *kf2, d_pair, d_poses, pairs, max_nodes, max_n, kp_stride, a[0].ctypes.data,
                                                 a[1].ctypes.data, len(a[0]), 1 if check_ori else 0, d_matches12, d_points12, d_nmatches),
         "orbhip_match_and_triangulate_device")


class NewPointsPair(C.Structure):
    """orbhip_newpoints_pair: one (current keyframe, neighbour) pair of LocalMapping::CreateNewMapPoints"""
    _fields_ = [("cam1", cf * 8 * 2), ("cam2", cf * 8 * 2), ("cam1_type", C.c_int32 * 2), ("cam2_type", C.c_int32 * 2),
                ("nleft1", C.c_int32), ("nleft2", C.c_int32), ("Tcw1", cf * 12 * 2), ("Tcw2", cf * 12 * 2), ("Twc1", cf * 12), ("Twc2", cf * 12),
                ("Ow1", cf * 3 * 2), ("Ow2", cf * 3 * 2), ("mb1", cf), ("mb2", cf), ("mbf", cf), ("ratio_factor", cf),
                ("far_points", C.c_int32), ("th_far_points", cf)]


NEWPOINTS_PAIR_DTYPE = np.dtype([("cam1", "<f4", (2, 8)), ("cam2", "<f4", (2, 8)), ("cam1_type", "<i4", (2,)), ("cam2_type", "<i4", (2,)),
                                 ("nleft1", "<i4"), ("nleft2", "<i4"), ("Tcw1", "<f4", (2, 12)), ("Tcw2", "<f4", (2, 12)), ("Twc1", "<f4", (12,)),
                                 ("Twc2", "<f4", (12,)), ("Ow1", "<f4", (2, 3)), ("Ow2", "<f4", (2, 3)), ("mb1", "<f4"), ("mb2", "<f4"),
                                 ("mbf", "<f4"), ("ratio_factor", "<f4"), ("far_points", "<i4"), ("th_far_points", "<f4")])
assert NEWPOINTS_PAIR_DTYPE.itemsize == C.sizeof(NewPointsPair)
lib.orbhip_create_new_map_points_device.argtypes = [vp] * 13 + [ci, ci, sz, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]


def _newpoints_pairs(pair):
    """[pairs] NEWPOINTS_PAIR_DTYPE records from a record array or a list of NewPointsPair structures"""
    if isinstance(pair, np.ndarray):
        assert pair.dtype == NEWPOINTS_PAIR_DTYPE
        return np.ascontiguousarray(pair).reshape(-1)
    return np.frombuffer(b"".join(bytes(p) for p in pair), NEWPOINTS_PAIR_DTYPE).copy()


def create_new_map_points_device(ctx, kf1, kf2, d_matches12, pair, max_n, kp_stride, level_sigma2_1, scale_factors1, level_sigma2_2,
                                 scale_factors2, d_x3D, d_outcome, d_n_created, d_has_mp1=None, d_has_mp2=None):
    """The per-match loop of LocalMapping::CreateNewMapPoints on the matches SearchForTriangulation left on the device, batched over
    keyframe pairs; asynchronous on the context's stream.  kf1 / kf2 = (d_kp, d_kp_raw|0, d_u_right|0, d_depth|0, d_n): device addresses;
    pair: HOST records (NEWPOINTS_PAIR_DTYPE array or NewPointsPair list), one per pair; d_has_mp1 / d_has_mp2: writable flag rows
    or None."""
    pr = _newpoints_pairs(pair)
    a = [np.ascontiguousarray(x, np.float32) for x in (level_sigma2_1, scale_factors1, level_sigma2_2, scale_factors2)]
    assert len(a[0]) == len(a[1]) == len(a[2]) == len(a[3]) and len(kf1) == 5 and len(kf2) == 5
    _chk(lib.orbhip_create_new_map_points_device(ctx.h, *[x or None for x in kf1], *[x or None for x in kf2], d_matches12, pr.ctypes.data, len(pr),
                                                 max_n, kp_stride, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                                 len(a[0]), d_has_mp1, d_has_mp2, d_x3D, d_outcome, d_n_created),
         "orbhip_create_new_map_points_device")


class NewPointsKeyframe(C.Structure):
    """orbhip_newpoints_keyframe: HOST pointers of one keyframe of create_new_map_points_host"""
    _fields_ = [("kp", vp), ("kp_raw", vp), ("desc", vp), ("u_right", vp), ("depth", vp), ("has_mp", vp), ("n", C.c_int32), ("nid", vp),
                ("node_ids", vp), ("node_start", vp), ("feat", vp), ("nnodes", C.c_int32), ("level_sigma2", vp), ("scale_factors", vp)]


lib.orbhip_create_new_map_points_host.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]


def _newpoints_keyframe(kf, keep):
    """kf: dict(kp, desc, has_mp, level_sigma2, scale_factors [, kp_raw, u_right, depth] + nid (current) or node_ids / node_start / feat)"""
    s = NewPointsKeyframe()
    n = len(kf["kp"])
    for name, dt in (("kp", KP_DTYPE), ("kp_raw", KP_DTYPE), ("desc", np.uint8), ("u_right", np.float32), ("depth", np.float32), ("has_mp", np.uint8),
                     ("nid", np.int32), ("node_ids", np.int32), ("node_start", np.int32), ("feat", np.int32), ("level_sigma2", np.float32),
                     ("scale_factors", np.float32)):
        if kf.get(name) is not None:
            a = np.ascontiguousarray(kf[name], dt)
            keep.append(a)
            setattr(s, name, a.ctypes.data if a.size else None)
    s.n = n
    s.nnodes = len(kf["node_ids"]) if kf.get("node_ids") is not None else 0
    return s


def create_new_map_points_host(ctx, cur, neigh, geom, pair, check_ori=True):
    """LocalMapping::CreateNewMapPoints' neighbour loop for one current keyframe on the device: SearchForTriangulation then the per-match
    loop with the flag update, per neighbour in order.  cur / neigh[k]: dicts of host arrays (see _newpoints_keyframe); geom: [n_neigh]
    TRI_GENERAL_DTYPE records; pair: [n_neigh] NEWPOINTS_PAIR_DTYPE records or NewPointsPair list.
    Returns (matches12 [n_neigh][n1], x3D [n_neigh][n1][3], outcome [n_neigh][n1], n_created [n_neigh], has_mp1 [n1])."""
    keep = []
    c = _newpoints_keyframe(cur, keep)
    nb = (NewPointsKeyframe * max(len(neigh), 1))(*[_newpoints_keyframe(f, keep) for f in neigh])
    pr = _newpoints_pairs(pair) if len(neigh) else np.zeros(0, NEWPOINTS_PAIR_DTYPE)
    g = np.ascontiguousarray(np.asarray(geom, TRI_GENERAL_DTYPE)).reshape(-1)
    assert len(pr) == len(neigh) == len(g)
    n1, K = c.n, len(neigh)
    m = np.full((K, n1), -9, np.int32); x = np.full((K, n1, 3), 7, np.float32); o = np.full((K, n1), 99, np.uint8)
    nc = np.full(K, -9, np.int32); mp1 = np.zeros(n1, np.uint8)
    nlevels = len(np.asarray(cur["level_sigma2"]))
    _chk(lib.orbhip_create_new_map_points_host(ctx.h, C.addressof(c), C.addressof(nb), g.ctypes.data if K else None, pr.ctypes.data if K else None, K,
                                               nlevels, 1 if check_ori else 0, m.ctypes.data, x.ctypes.data, o.ctypes.data, nc.ctypes.data,
                                               mp1.ctypes.data), "orbhip_create_new_map_points_host")
    return m, x, o, nc, mp1


lib.orbhip_search_by_bow_device.argtypes = [vp] * 15 + [ci, ci, ci, sz, cf, ci, vp, vp]


def search_by_bow_device(ctx, kf, f, d_nF, pairs, max_nodes, max_n, kp_stride, nn_ratio, check_ori, d_match_f, d_nmatches):
    """ORBmatcher::SearchByBoW(KeyFrame, Frame), batched.  kf = (d_node_ids, d_node_start, d_feat, d_nnodes, d_valid, d_kp, d_desc),
    f = (d_node_ids, d_node_start, d_feat, d_nnodes, d_kp, d_desc): device addresses (ints)."""
    _chk(lib.orbhip_search_by_bow_device(ctx.h, kf[0], kf[1], kf[2], kf[3], kf[4], kf[5], kf[6], f[0], f[1], f[2], f[3], f[4], f[5], d_nF,
                                         pairs, max_nodes, max_n, kp_stride, nn_ratio, 1 if check_ori else 0, d_match_f, d_nmatches),
         "orbhip_search_by_bow_device")


lib.orbhip_search_by_projection_rig_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, sz, ci, cf, cf, cf, cf, ci, cf, ci, vp, vp]
lib.orbhip_search_by_bow_rig_device.argtypes = [vp] * 16 + [ci, ci, ci, sz, cf, ci, vp, vp]
lib.orbhip_assign_features_to_grid_rig_device.argtypes = [vp, vp, vp, vp, ci, ci, sz, cf, cf, cf, cf, vp, vp]


def search_by_projection_rig_device(ctx, mode, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_n, d_nleft, d_mirror, max_n, kp_stride, pairs, bounds,
                                    th_high, nn_ratio, check_ori, d_train_match, d_nmatches):
    """ORBmatcher::SearchByProjection on frames of a two-camera rig (Nleft != -1); mode 0: from the last frame, 1: local map points."""
    _chk(lib.orbhip_search_by_projection_rig_device(ctx.h, mode, d_q, d_desc_q, d_nq, max_q, d_kp, d_desc, d_n, d_nleft, d_mirror, max_n, kp_stride,
                                                    pairs, bounds[0], bounds[1], bounds[2], bounds[3], th_high, nn_ratio, 1 if check_ori else 0,
                                                    d_train_match, d_nmatches), "orbhip_search_by_projection_rig_device")


def search_by_bow_rig_device(ctx, kf, f, d_nF, d_nleft, pairs, max_nodes, max_n, kp_stride, nn_ratio, check_ori, d_match_f, d_nmatches):
    """ORBmatcher::SearchByBoW(KeyFrame, Frame) on rig frames; kf / f as in search_by_bow_device."""
    _chk(lib.orbhip_search_by_bow_rig_device(ctx.h, kf[0], kf[1], kf[2], kf[3], kf[4], kf[5], kf[6], f[0], f[1], f[2], f[3], f[4], f[5], d_nF, d_nleft,
                                             pairs, max_nodes, max_n, kp_stride, nn_ratio, 1 if check_ori else 0, d_match_f, d_nmatches),
         "orbhip_search_by_bow_rig_device")


def assign_features_to_grid_rig_device(ctx, d_kp, d_n, d_nleft, frames, max_n, kp_stride, bounds, d_cell_start, d_items):
    """Frame::AssignFeaturesToGrid on rig frames: mGrid | mGridRight as one CSR (2*3072+1 cell starts per frame)."""
    _chk(lib.orbhip_assign_features_to_grid_rig_device(ctx.h, d_kp, d_n, d_nleft, frames, max_n, kp_stride, bounds[0], bounds[1], bounds[2],
                                                       bounds[3], d_cell_start, d_items), "orbhip_assign_features_to_grid_rig_device")


class PimRig(C.Structure):
    _fields_ = [("Rcb", cd * 9), ("tcb", cd * 3), ("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("bf", cd), ("camera_model", C.c_int32),
                ("kb", cd * 4), ("has_cam2", C.c_int32), ("Trl", cd * 12), ("fx2", cd), ("fy2", cd), ("cx2", cd), ("cy2", cd),
                ("camera2_model", C.c_int32), ("kb2", cd * 4)]


def pim_rig(cam, Rcb, tcb, camera_model=0, kb=(0, 0, 0, 0), Trl=None, cam2=None, camera2_model=0, kb2=(0, 0, 0, 0)):
    """orbhip_pim_rig of a frame: cam = (fx, fy, cx, cy, bf), Tcb, optional second camera (Trl 3x4, cam2 = (fx, fy, cx, cy))."""
    r = PimRig()
    r.Rcb[:] = [float(v) for v in np.asarray(Rcb, np.float64).reshape(-1)]
    r.tcb[:] = [float(v) for v in np.asarray(tcb, np.float64).reshape(-1)]
    r.fx, r.fy, r.cx, r.cy, r.bf = [float(c) for c in cam]
    r.camera_model = int(camera_model)
    r.kb[:] = [float(v) for v in kb]
    if Trl is not None:
        r.has_cam2 = 1
        r.Trl[:] = [float(v) for v in np.asarray(Trl, np.float64).reshape(-1)]
        r.fx2, r.fy2, r.cx2, r.cy2 = [float(c) for c in cam2]
        r.camera2_model = int(camera2_model)
        r.kb2[:] = [float(v) for v in kb2]
    return r


lib.orbhip_pose_inertial_optimization_device.argtypes = [vp, ci, ci, vp, ci, ci] + [vp] * 17
lib.orbhip_pose_inertial_optimization_host.argtypes = [vp, ci, ci, vp, ci] + [vp] * 16


def pose_inertial_optimization_device(ctx, mode, rec_init, rig, frames, max_edges, d_Xw, d_obs, d_inv_sigma2, d_kind, d_close, d_n_edges,
                                      d_prev, d_preint, d_info, d_info_g, d_info_a, d_prior, d_state, d_outlier, d_ret, d_H_out,
                                      d_stats=None):
    """Optimizer::PoseInertialOptimizationLastKeyFrame (mode 0) / ...LastFrame (mode 1), batched over frames; device addresses (ints,
    d_close / d_prior / d_stats may be None); rig = PimRig (pim_rig())."""
    _chk(lib.orbhip_pose_inertial_optimization_device(ctx.h, int(mode), int(bool(rec_init)), C.byref(rig), frames, max_edges, d_Xw, d_obs,
                                                      d_inv_sigma2, d_kind, d_close, d_n_edges, d_prev, d_preint, d_info, d_info_g,
                                                      d_info_a, d_prior, d_state, d_outlier, d_ret, d_H_out, d_stats),
         "orbhip_pose_inertial_optimization_device")


def pose_inertial_optimization_host(ctx, mode, rec_init, rig, fr):
    """One frame from host arrays (fr: the dict layout of tests/synth_pose_inertial.py: Xw, obs, inv_sigma2, kind, close, state, prev,
    preint, info, info_g, info_a, and prior + prior_H in mode 1) -> (state [21], outlier [n] uint8, ret, H [15][15], stats [4])."""
    n = len(fr["Xw"])
    a = {k: np.ascontiguousarray(fr[k], t) for k, t in (("Xw", np.float64), ("obs", np.float64), ("inv_sigma2", np.float64),
                                                         ("kind", np.uint8), ("close", np.uint8), ("prev", np.float64),
                                                         ("preint", np.float64), ("info", np.float64), ("info_g", np.float64),
                                                         ("info_a", np.float64))}
    prior = np.ascontiguousarray(np.concatenate([fr["prior"], np.asarray(fr["prior_H"]).reshape(-1)]), np.float64) if mode == 1 else None
    state = np.ascontiguousarray(fr["state"], np.float64).copy()
    out = np.zeros(max(n, 1), np.uint8); ret = np.zeros(1, np.int32); H = np.zeros(225); st = np.zeros(4, np.int32)
    _chk(lib.orbhip_pose_inertial_optimization_host(ctx.h, int(mode), int(bool(rec_init)), C.byref(rig), n, a["Xw"].ctypes.data,
                                                    a["obs"].ctypes.data, a["inv_sigma2"].ctypes.data, a["kind"].ctypes.data,
                                                    a["close"].ctypes.data, a["prev"].ctypes.data, a["preint"].ctypes.data,
                                                    a["info"].ctypes.data, a["info_g"].ctypes.data, a["info_a"].ctypes.data,
                                                    None if prior is None else prior.ctypes.data, state.ctypes.data, out.ctypes.data,
                                                    ret.ctypes.data, H.ctypes.data, st.ctypes.data),
         "orbhip_pose_inertial_optimization_host")
    return state, out[:n], int(ret[0]), H.reshape(15, 15), st


class InertialOptParams(C.Structure):
    _fields_ = [("free_vel_bias", C.c_int32), ("free_gdir", C.c_int32), ("free_scale", C.c_int32), ("gauss_newton", C.c_int32),
                ("iterations", C.c_int32), ("max_trials", C.c_int32), ("lambda_init", cd), ("prior_g", cd), ("prior_a", cd)]


IO_GLOBAL = 16
lib.orbhip_inertial_opt_default_params.argtypes = [vp, ci, ci, ci, cf, cf]
lib.orbhip_inertial_opt_default_params.restype = None
lib.orbhip_inertial_opt_lds_keyframes.argtypes = []
lib.orbhip_inertial_optimization_device.argtypes = [vp, vp, ci] + [vp] * 8
lib.orbhip_inertial_optimization_host.argtypes = [vp, vp, ci] + [vp] * 7


def inertial_opt_params(overload, mono=False, fixed_vel=False, priorG=1e2, priorA=1e6):
    """orbhip_inertial_opt_params of Optimizer::InertialOptimization's overload 0..3 = (a)..(d) with the reference's arguments."""
    p = InertialOptParams()
    lib.orbhip_inertial_opt_default_params(C.byref(p), int(overload), int(bool(mono)), int(bool(fixed_vel)), float(priorG), float(priorA))
    return p


def inertial_opt_lds_keyframes():
    """The chain length up to which a map's chain state lives in LDS (longer maps use the context's work arena)."""
    return lib.orbhip_inertial_opt_lds_keyframes()


def inertial_optimization_device(ctx, params, maps, d_kf_off, d_kf, d_link, d_preint, d_info, d_global, d_stats=None, d_trace=None):
    """Optimizer::InertialOptimization batched over maps; device addresses (ints, d_stats / d_trace may be None); params =
    InertialOptParams (inertial_opt_params())."""
    _chk(lib.orbhip_inertial_optimization_device(ctx.h, C.byref(params), maps, d_kf_off, d_kf, d_link, d_preint, d_info, d_global,
                                                 d_stats, d_trace), "orbhip_inertial_optimization_device")


def inertial_optimization_host(ctx, params, mp, trace=False):
    """One map from host arrays (mp: the dict layout of tests/synth_inertial_opt.py: kf [n][21], link [n], preint [n][67], info [n][81],
    glob [16]) -> (kf [n][21], glob [16], stats [8], trace [iterations][2] or None; rows of iterations not run are NaN)."""
    kf = np.ascontiguousarray(mp["kf"], np.float64).copy()
    n = len(kf)
    link = np.ascontiguousarray(mp["link"], np.uint8)
    preint = np.ascontiguousarray(mp["preint"], np.float64)
    info = np.ascontiguousarray(mp["info"], np.float64)
    glob = np.ascontiguousarray(mp["glob"], np.float64).copy()
    st = np.zeros(8)
    tr = np.full((max(params.iterations, 1), 2), np.nan) if trace else None
    _chk(lib.orbhip_inertial_optimization_host(ctx.h, C.byref(params), n, kf.ctypes.data, link.ctypes.data, preint.ctypes.data,
                                               info.ctypes.data, glob.ctypes.data, st.ctypes.data, None if tr is None else tr.ctypes.data),
         "orbhip_inertial_optimization_host")
    return kf, glob, st, (None if tr is None else tr[:params.iterations])


class PreintParams(C.Structure):
    _fields_ = [("nga", cf * 36), ("nga_walk", cf * 36), ("force_form", C.c_int32), ("want_info", C.c_int32)]


PREINT_FORM_AUTO, PREINT_FORM_LANE, PREINT_FORM_WAVE = 0, 1, 2
lib.orbhip_preint_default_params.argtypes = [vp, cf, cf, cf, cf]
lib.orbhip_preint_default_params.restype = None
lib.orbhip_preint_wave_max_chains.argtypes = []
lib.orbhip_preintegrate_device.argtypes = [vp, vp, ci] + [vp] * 9
lib.orbhip_preintegrate_host.argtypes = [vp, vp, ci] + [vp] * 9


def preint_params(ng=1.7e-4, na=2.0e-3, ngw=1.9393e-5, naw=3.0e-3, nga=None, nga_walk=None, force_form=PREINT_FORM_AUTO, want_info=True):
    """orbhip_preint_params: the diagonal Nga / NgaWalk of IMU::Calib::Set(ng, na, ngw, naw), or full 6 x 6 matrices (nga, nga_walk)."""
    p = PreintParams()
    lib.orbhip_preint_default_params(C.byref(p), float(ng), float(na), float(ngw), float(naw))
    if nga is not None:
        p.nga[:] = [float(v) for v in np.asarray(nga, np.float32).reshape(36)]
    if nga_walk is not None:
        p.nga_walk[:] = [float(v) for v in np.asarray(nga_walk, np.float32).reshape(36)]
    p.force_form = int(force_form)
    p.want_info = int(bool(want_info))
    return p


def preint_wave_max_chains():
    """The number of chains from which the lane form takes over from the wave form."""
    return lib.orbhip_preint_wave_max_chains()


def preintegrate_device(ctx, params, chains, d_meas_off, d_meas, d_continue, d_record, d_cov, d_avg, d_info=None, d_info_g=None,
                        d_info_a=None):
    """IMU preintegration batched over chains; device addresses (ints; d_continue may be None, the info arrays without want_info);
    params = PreintParams (preint_params())."""
    _chk(lib.orbhip_preintegrate_device(ctx.h, C.byref(params), chains, d_meas_off, d_meas, d_continue, d_record, d_cov, d_avg, d_info,
                                        d_info_g, d_info_a), "orbhip_preintegrate_device")


def preintegrate_host(ctx, params, bias, meas, start=None):
    """Chains from host arrays.  bias [n][6] (bg, ba), meas: a list of n arrays [len][7] (ax, ay, az, wx, wy, wz, dt), start: None
    (every chain fresh) or a list with None / (record [67], cov [225], avg [6]) per chain to continue from ->
    (record [n][67], cov [n][15][15] float32, avg [n][6] float32, info [n][9][9], info_g [n][3][3], info_a [n][3][3]; the last three None
    without want_info)."""
    n = len(meas)
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(m) for m in meas])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1, 7) for m in meas]) if n else np.zeros((0, 7)), np.float32)
    rec = np.zeros((n, IBA_PREINT)); cov = np.zeros((n, 225), np.float32); avg = np.zeros((n, 6), np.float32)
    cont = np.zeros(max(n, 1), np.uint8)
    for c in range(n):
        if start is not None and start[c] is not None:
            rec[c] = start[c][0]; cov[c] = np.asarray(start[c][1], np.float32).reshape(225); avg[c] = start[c][2]; cont[c] = 1
        rec[c, 61:67] = np.asarray(bias[c], np.float32)
    wi = bool(params.want_info)
    info = np.zeros((n, 81)); ig = np.zeros((n, 9)); ia = np.zeros((n, 9))
    _chk(lib.orbhip_preintegrate_host(ctx.h, C.byref(params), n, off.ctypes.data, flat.ctypes.data if len(flat) else None, cont.ctypes.data,
                                      rec.ctypes.data, cov.ctypes.data, avg.ctypes.data, info.ctypes.data if wi else None,
                                      ig.ctypes.data if wi else None, ia.ctypes.data if wi else None), "orbhip_preintegrate_host")
    if not wi:
        return rec, cov.reshape(n, 15, 15), avg, None, None, None
    return rec, cov.reshape(n, 15, 15), avg, info.reshape(n, 9, 9), ig.reshape(n, 3, 3), ia.reshape(n, 3, 3)


class TvrParams(C.Structure):
    _fields_ = [("sigma", cf), ("iterations", C.c_int32), ("rh_threshold", cf), ("min_parallax", cf), ("min_triangulated", C.c_int32),
                ("draw_sets", C.c_int32), ("seed", C.c_uint64)]


class TvrStats(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("score_h", cf), ("score_f", cf), ("iter_h", C.c_int32), ("iter_f", C.c_int32),
                ("model", C.c_int32), ("n_inliers", C.c_int32), ("n_hyp", C.c_int32), ("n_good", C.c_int32 * 8),
                ("hyp_index", C.c_int32), ("parallax", cf)]


TVR_STATS_DTYPE = np.dtype([("n_matches", "<i4"), ("score_h", "<f4"), ("score_f", "<f4"), ("iter_h", "<i4"), ("iter_f", "<i4"),
                            ("model", "<i4"), ("n_inliers", "<i4"), ("n_hyp", "<i4"), ("n_good", "<i4", (8,)), ("hyp_index", "<i4"),
                            ("parallax", "<f4")])
assert TVR_STATS_DTYPE.itemsize == C.sizeof(TvrStats) == 72

lib.orbhip_tvr_default_params.argtypes = [vp]
lib.orbhip_two_view_reconstruct_device.argtypes = [vp, vp, vp, vp, vp, sz, vp, ci, ci, cf, cf, cf, cf, vp] + [vp] * 9
lib.orbhip_two_view_reconstruct_host.argtypes = [vp, vp, ci, vp, ci, vp, cf, cf, cf, cf, vp] + [vp] * 7


def tvr_params(iterations=200, sigma=1.0, rh_threshold=None, draw_sets=True, seed=0):
    """orbhip_tvr_params with the reference's defaults (TwoViewReconstruction.h:36, TwoViewReconstruction.cc:114-120)."""
    p = TvrParams()
    lib.orbhip_tvr_default_params(C.byref(p))
    p.iterations, p.sigma, p.draw_sets, p.seed = int(iterations), float(sigma), int(bool(draw_sets)), int(seed)
    if rh_threshold is not None:
        p.rh_threshold = float(rh_threshold)
    return p


def two_view_reconstruct_device(ctx, d_kp1, d_n1, d_kp2, d_n2, kp_stride, d_matches12, pairs, max_n, K, params, d_sets, d_ok, d_R21, d_t21,
                                d_P3D, d_triangulated, d_stats=None, d_hyp_scores=None, d_hyp_mats=None):
    """TwoViewReconstruction::Reconstruct, batched over frame pairs; device addresses (ints; the last three may be None);
    K = (fx, fy, cx, cy), params = TvrParams (tvr_params())."""
    _chk(lib.orbhip_two_view_reconstruct_device(ctx.h, d_kp1, d_n1, d_kp2, d_n2, kp_stride, d_matches12, pairs, max_n, K[0], K[1], K[2], K[3],
                                                C.byref(params), d_sets, d_ok, d_R21, d_t21, d_P3D, d_triangulated, d_stats, d_hyp_scores,
                                                d_hyp_mats), "orbhip_two_view_reconstruct_device")


def two_view_reconstruct_host(ctx, kp1, kp2, matches12, K, params, sets=None):
    """One pair from host arrays (kp1 / kp2: KP_DTYPE, matches12 [n1] int32; sets [iterations][8] int32 when params.draw_sets == 0)
    -> (ok, R21 [3][3], t21 [3], P3D [n1][3], triangulated [n1] bool, stats (TVR_STATS_DTYPE scalar), sets)."""
    kp1 = np.ascontiguousarray(kp1, KP_DTYPE); kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
    m = np.ascontiguousarray(matches12, np.int32)
    n1, n2 = len(kp1), len(kp2)
    assert len(m) == n1
    s = np.zeros((params.iterations, 8), np.int32) if sets is None else np.ascontiguousarray(sets, np.int32).copy()
    assert s.shape == (params.iterations, 8)
    ok = np.zeros(1, np.uint8); R = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
    P = np.zeros((max(n1, 1), 3), np.float32); tr = np.zeros(max(n1, 1), np.uint8); st = np.zeros(1, TVR_STATS_DTYPE)
    _chk(lib.orbhip_two_view_reconstruct_host(ctx.h, kp1.ctypes.data, n1, kp2.ctypes.data, n2, m.ctypes.data, K[0], K[1], K[2], K[3],
                                              C.byref(params), s.ctypes.data, ok.ctypes.data, R.ctypes.data, t.ctypes.data, P.ctypes.data,
                                              tr.ctypes.data, st.ctypes.data), "orbhip_two_view_reconstruct_host")
    return bool(ok[0]), R.reshape(3, 3), t, P[:n1], tr[:n1].astype(bool), st[0], s


class Sim3Camera(C.Structure):
    _fields_ = [("fx", cd), ("fy", cd), ("cx", cd), ("cy", cd), ("camera_model", C.c_int32), ("kb", cd * 4)]


lib.orbhip_optimize_sim3_device.argtypes = [vp] * 8 + [ci, ci, vp, vp, cd, ci, vp, vp, vp, vp]
lib.orbhip_optimize_sim3_host.argtypes = [vp] * 7 + [ci, vp, vp, cd, ci, vp, vp, vp, vp]


def sim3_camera(cam, kb8=None):
    """orbhip_sim3_camera from cam = (fx, fy, cx, cy) and kb8 = (k1..k4) for a KannalaBrandt8 camera, None = Pinhole."""
    return Sim3Camera(float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), 1 if kb8 is not None else 0,
                      (cd * 4)(*(kb8 if kb8 is not None else (0, 0, 0, 0))))


def optimize_sim3_device(ctx, d_P1c, d_P2c, d_obs1, d_obs2, d_inv_sigma2_1, d_inv_sigma2_2, d_n, pairs, max_edges, cam1, cam2, th2,
                         fix_scale, d_sim3, d_flag, d_n_in, d_stats=None):
    """Optimizer::OptimizeSim3, batched over keyframe pairs; device addresses (ints; d_stats may be None); cam1 / cam2 = Sim3Camera
    (sim3_camera()); th2 is the reference's float."""
    _chk(lib.orbhip_optimize_sim3_device(ctx.h, d_P1c, d_P2c, d_obs1, d_obs2, d_inv_sigma2_1, d_inv_sigma2_2, d_n, pairs, max_edges,
                                         C.byref(cam1), C.byref(cam2), float(np.float32(th2)), int(bool(fix_scale)), d_sim3, d_flag,
                                         d_n_in, d_stats), "orbhip_optimize_sim3_device")


def optimize_sim3_host(ctx, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, th2, fix_scale, sim3):
    """One pair from host arrays (P1c / P2c [n][3], obs1 / obs2 [n][2], inv_sigma2_1 / _2 [n], sim3 [8] = qx qy qz qw tx ty tz s)
    -> (sim3 [8], flag [n] uint8, n_in, stats [4])."""
    a = [np.ascontiguousarray(v, np.float64) for v in (P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2)]
    n = len(a[0])
    s = np.ascontiguousarray(sim3, np.float64).copy()
    flag = np.zeros(max(n, 1), np.uint8); nin = np.zeros(1, np.int32); st = np.zeros(4, np.int32)
    _chk(lib.orbhip_optimize_sim3_host(ctx.h, *[v.ctypes.data for v in a], n, C.byref(cam1), C.byref(cam2), float(np.float32(th2)),
                                       int(bool(fix_scale)), s.ctypes.data, flag.ctypes.data, nin.ctypes.data, st.ctypes.data),
         "orbhip_optimize_sim3_host")
    return s, flag[:n], int(nin[0]), st


class Sim3SolverParams(C.Structure):
    _fields_ = [("probability", cd), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("fix_scale", C.c_int32),
                ("draw_sets", C.c_int32), ("seed", C.c_uint64)]


lib.orbhip_sim3solver_default_params.argtypes = [vp]
lib.orbhip_sim3_solver_device.argtypes = [vp] * 6 + [ci, ci] + [vp] * 12
lib.orbhip_sim3_solver_host.argtypes = [vp] * 5 + [ci] + [vp] * 12


def sim3_solver_params(probability=None, min_inliers=None, max_iterations=None, fix_scale=False, draw_sets=True, seed=0):
    """orbhip_sim3solver_params with the reference's defaults (Sim3Solver.h:40: 0.99, 6, 300)."""
    p = Sim3SolverParams()
    lib.orbhip_sim3solver_default_params(C.byref(p))
    if probability is not None:
        p.probability = float(probability)
    if min_inliers is not None:
        p.min_inliers = int(min_inliers)
    if max_iterations is not None:
        p.max_iterations = int(max_iterations)
    p.fix_scale, p.draw_sets, p.seed = int(bool(fix_scale)), int(bool(draw_sets)), int(seed)
    return p


def sim3_solver_device(ctx, d_X1c, d_X2c, d_max_err1, d_max_err2, d_n, pairs, max_n, cam1, cam2, params, d_sets, d_converged, d_R12, d_t12,
                       d_s12, d_n_inliers, d_inlier, d_stats=None, d_counts=None):
    """Sim3Solver, batched over candidates; device addresses (ints; the last two may be None); cam1 / cam2 = Sim3Camera (sim3_camera()),
    params = Sim3SolverParams (sim3_solver_params())."""
    _chk(lib.orbhip_sim3_solver_device(ctx.h, d_X1c, d_X2c, d_max_err1, d_max_err2, d_n, pairs, max_n, C.byref(cam1), C.byref(cam2),
                                       C.byref(params), d_sets, d_converged, d_R12, d_t12, d_s12, d_n_inliers, d_inlier, d_stats, d_counts),
         "orbhip_sim3_solver_device")


def sim3_solver_host(ctx, X1c, X2c, max_err1, max_err2, cam1, cam2, params, sets=None, R12=None, t12=None, s12=None):
    """One candidate from host arrays (X1c / X2c [n][3] float32, max_err1 / _2 [n] truncated thresholds; sets [max_iterations][3] int32
    when params.draw_sets == 0; R12 / t12 / s12: what the outputs hold before the call) -> dict(converged, R12 [3][3], t12 [3], s12,
    n_inliers, inlier [n] uint8, stats [3], counts [max_iterations], sets)."""
    a = [np.ascontiguousarray(v, np.float32) for v in (X1c, X2c, max_err1, max_err2)]
    n = len(a[0])
    it = max(int(params.max_iterations), 1)
    s = np.zeros((it, 3), np.int32) if sets is None else np.ascontiguousarray(sets, np.int32).copy()
    assert s.shape == (it, 3)
    cv = np.zeros(1, np.uint8); R = np.zeros(9, np.float32) if R12 is None else np.ascontiguousarray(R12, np.float32).reshape(9).copy()
    t = np.zeros(3, np.float32) if t12 is None else np.ascontiguousarray(t12, np.float32).copy()
    sc = np.zeros(1, np.float32) if s12 is None else np.array([s12], np.float32)
    nin = np.zeros(1, np.int32); inl = np.zeros(max(n, 1), np.uint8); st = np.zeros(3, np.int32); cnt = np.zeros(it, np.int32)
    _chk(lib.orbhip_sim3_solver_host(ctx.h, *[v.ctypes.data for v in a], n, C.byref(cam1), C.byref(cam2), C.byref(params), s.ctypes.data,
                                     cv.ctypes.data, R.ctypes.data, t.ctypes.data, sc.ctypes.data, nin.ctypes.data, inl.ctypes.data,
                                     st.ctypes.data, cnt.ctypes.data), "orbhip_sim3_solver_host")
    return dict(converged=bool(cv[0]), R12=R.reshape(3, 3), t12=t, s12=float(sc[0]), n_inliers=int(nin[0]), inlier=inl[:n], stats=st,
                counts=cnt, sets=s)


# ---------------------------------------------------------------- MLPnPsolver (relocalisation candidates)
class MlpnpParams(C.Structure):
    _fields_ = [("probability", cd), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float),
                ("th2", C.c_float), ("first_call_iterations", C.c_int32), ("resume_at", C.c_int32), ("draw_sets", C.c_int32), ("seed", C.c_uint64)]


lib.orbhip_mlpnp_default_params.argtypes = [vp]
lib.orbhip_mlpnp_solver_device.argtypes = [vp] * 5 + [ci, ci] + [vp] * 9
lib.orbhip_mlpnp_solver_host.argtypes = [vp] * 4 + [ci] + [vp] * 9


def mlpnp_params(probability=None, min_inliers=None, max_iterations=None, min_set=None, epsilon=None, th2=None, first_call_iterations=0,
                 resume_at=0, draw_sets=True, seed=0):
    """orbhip_mlpnp_params with the reference's defaults (MLPnPsolver.h:65: 0.99, 8, 300, 6, 0.4, 5.991)."""
    p = MlpnpParams()
    lib.orbhip_mlpnp_default_params(C.byref(p))
    for name, v, conv in (("probability", probability, float), ("min_inliers", min_inliers, int), ("max_iterations", max_iterations, int),
                          ("min_set", min_set, int), ("epsilon", epsilon, float), ("th2", th2, float)):
        if v is not None:
            setattr(p, name, conv(v))
    p.first_call_iterations, p.resume_at, p.draw_sets, p.seed = int(first_call_iterations), int(resume_at), int(bool(draw_sets)), int(seed)
    return p


def mlpnp_solver_device(ctx, d_Xw, d_p2d, d_sigma2, d_n, candidates, max_n, cam, params, d_sets, d_outcome, d_Tcw, d_n_inliers, d_inlier,
                        d_stats=None, d_counts=None):
    """MLPnPsolver, batched over candidates; device addresses (ints; the last two may be None); cam = Sim3Camera (sim3_camera()),
    params = MlpnpParams (mlpnp_params())."""
    _chk(lib.orbhip_mlpnp_solver_device(ctx.h, d_Xw, d_p2d, d_sigma2, d_n, candidates, max_n, C.byref(cam), C.byref(params), d_sets, d_outcome,
                                        d_Tcw, d_n_inliers, d_inlier, d_stats, d_counts), "orbhip_mlpnp_solver_device")


def mlpnp_solver_host(ctx, Xw, p2d, sigma2, cam, params, sets=None, Tcw=None):
    """One candidate from host arrays (Xw [n][3], p2d [n][2], sigma2 [n] float32; sets [max_iterations][6] int32 when params.draw_sets == 0;
    Tcw: what the output holds before the call) -> dict(outcome, Tcw [12], n_inliers, inlier [n] uint8, stats [4],
    counts [max_iterations], sets)."""
    a = [np.ascontiguousarray(v, np.float32) for v in (Xw, p2d, sigma2)]
    n = len(a[0])
    it = max(int(params.max_iterations), 1)
    s = np.zeros((it, 6), np.int32) if sets is None else np.ascontiguousarray(sets, np.int32).copy()
    assert s.shape == (it, 6)
    oc = np.zeros(1, np.uint8); T = np.zeros(12, np.float32) if Tcw is None else np.ascontiguousarray(Tcw, np.float32).reshape(12).copy()
    nin = np.zeros(1, np.int32); inl = np.zeros(max(n, 1), np.uint8); st = np.zeros(4, np.int32); cnt = np.zeros(it, np.int32)
    _chk(lib.orbhip_mlpnp_solver_host(ctx.h, *[v.ctypes.data for v in a], n, C.byref(cam), C.byref(params), s.ctypes.data, oc.ctypes.data,
                                      T.ctypes.data, nin.ctypes.data, inl.ctypes.data, st.ctypes.data, cnt.ctypes.data),
         "orbhip_mlpnp_solver_host")
    return dict(outcome=int(oc[0]), Tcw=T, n_inliers=int(nin[0]), inlier=inl[:n], stats=st, counts=cnt, sets=s)


# ---------------------------------------------------------------- Tracking::SearchLocalPoints (Frame::isInFrustum + the local-map matcher)
FRUSTUM_MAX_LEVELS = 32
FRUSTUM_FRAME_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("Rrw", "<f4", (9,)), ("trw", "<f4", (3,)),
                                ("Orw", "<f4", (3,)), ("cam", "<f4", (2, 8)), ("cam_type", "<i4", (2,)), ("rig", "<i4"), ("mbf", "<f4"),
                                ("nlevels", "<i4"), ("scale_factors", "<f4", (FRUSTUM_MAX_LEVELS,)), ("level_thresholds", "<f4", (FRUSTUM_MAX_LEVELS,)),
                                ("th", "<f4"), ("far_points", "<i4"), ("th_far_points", "<f4"), ("viewing_cos_limit", "<f4"), ("n_points", "<i4")])
TRACK_RECORD_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("proj_yr", "<f4"), ("depth", "<f4"), ("depth_r", "<f4"),
                               ("view_cos", "<f4"), ("view_cos_r", "<f4"), ("level", "<i4"), ("level_r", "<i4"), ("in_view", "u1"),
                               ("in_view_r", "u1"), ("code", "u1"), ("code_r", "u1")])
assert FRUSTUM_FRAME_DTYPE.itemsize == 480 and TRACK_RECORD_DTYPE.itemsize == 44
lib.orbhip_frustum_chunk.argtypes = []
lib.orbhip_frustum_chunk.restype = ci
FRUSTUM_CHUNK = lib.orbhip_frustum_chunk()           # points a workgroup of k_frustum_queries takes per trip
lib.orbhip_predict_scale_thresholds.argtypes = [cf, ci, vp]
lib.orbhip_frustum_queries_device.argtypes = [vp, vp, ci, ci] + [vp] * 7 + [cf, cf, cf, cf, ci] + [vp] * 6
lib.orbhip_search_local_points_device.argtypes = [vp, vp, ci, ci] + [vp] * 7 + [ci] + [vp] * 6 + [ci, sz, cf, cf, cf, cf, ci, cf] + [vp] * 8


class LocalPoints(C.Structure):
    """orbhip_local_points: HOST pointers of the points of one frame of search_local_points_host"""
    _fields_ = [("Xw", vp), ("normal", vp), ("min_dist", vp), ("max_dist", vp), ("flags", vp), ("desc", vp), ("track_depth", vp), ("n", C.c_int32)]


lib.orbhip_search_local_points_host.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, cf, cf, cf, cf, ci, cf] + [vp] * 6
lib.orbhip_search_local_points_host_resident.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, cf, cf, cf, cf, ci, cf] + [vp] * 6


def predict_scale_thresholds(log_scale_factor, nlevels):
    """The level thresholds of MapPoint::PredictScale, found with the platform's logf (host only, no device): [nlevels - 1] float32."""
    out = np.zeros(FRUSTUM_MAX_LEVELS, np.float32)
    _chk(lib.orbhip_predict_scale_thresholds(float(np.float32(log_scale_factor)), int(nlevels), out.ctypes.data), "orbhip_predict_scale_thresholds")
    return out[:max(int(nlevels) - 1, 0)].copy()


def _frustum_frames(frame):
    f = np.ascontiguousarray(frame).reshape(-1)
    assert f.dtype == FRUSTUM_FRAME_DTYPE
    return f


def frustum_queries_device(ctx, frame, max_points, d_Xw, d_normal, d_min_dist, d_max_dist, d_flags, d_desc, d_track_depth, bounds, max_q,
                           d_track, d_n_to_match, d_q, d_desc_q, d_owner, d_nq):
    """Frame::isInFrustum over [frames][max_points] points and the matcher's query list, on the device; frame: HOST records
    (FRUSTUM_FRAME_DTYPE), everything else device addresses (ints; d_track_depth may be None); asynchronous."""
    f = _frustum_frames(frame)
    _chk(lib.orbhip_frustum_queries_device(ctx.h, f.ctypes.data, len(f), max_points, d_Xw, d_normal, d_min_dist, d_max_dist,
                                           d_flags, d_desc, d_track_depth, bounds[0], bounds[1], bounds[2], bounds[3], max_q, d_track,
                                           d_n_to_match, d_q, d_desc_q, d_owner, d_nq), "orbhip_frustum_queries_device")


def search_local_points_device(ctx, frame, max_points, d_Xw, d_normal, d_min_dist, d_max_dist, d_flags, d_desc, d_track_depth, max_q, d_kp,
                               d_desc_kp, d_u_right, d_n, d_nleft, d_mirror, max_n, kp_stride, bounds, th_high, nn_ratio, d_track, d_n_to_match,
                               d_q, d_desc_q, d_owner, d_nq, d_train_match, d_nmatches):
    """Tracking::SearchLocalPoints for len(frame) frames: the frustum kernel and the local-map matcher (the rig form when d_nleft is
    given) back to back on the context's stream; arguments as frustum_queries_device + the matcher's train side."""
    f = _frustum_frames(frame)
    _chk(lib.orbhip_search_local_points_device(ctx.h, f.ctypes.data, len(f), max_points, d_Xw, d_normal, d_min_dist, d_max_dist,
                                               d_flags, d_desc, d_track_depth, max_q, d_kp, d_desc_kp, d_u_right, d_n, d_nleft, d_mirror, max_n,
                                               kp_stride, bounds[0], bounds[1], bounds[2], bounds[3], th_high, nn_ratio, d_track, d_n_to_match,
                                               d_q, d_desc_q, d_owner, d_nq, d_train_match, d_nmatches), "orbhip_search_local_points_device")


def search_local_points_host(ctx, frame, points, kp, desc, u_right, bounds, train_match, nleft=-1, mirror=None, th_high=100, nn_ratio=0.8,
                             d_kp=None, d_desc=None):
    """One frame from host arrays.  frame: one FRUSTUM_FRAME_DTYPE record; points: dict(Xw [n][3], normal [n][3], min_dist, max_dist
    [n], flags [n] uint8, desc [n][32] [, track_depth [n]]); train side as search_by_projection_host (d_desc [+ d_kp]: device addresses
    of a resident frame) -> (track [n] TRACK_RECORD_DTYPE, n_to_match, owner [nq], train_match [len(kp)], nmatches)."""
    f = _frustum_frames(frame)
    assert len(f) == 1
    keep = {}
    for name, dt in (("Xw", np.float32), ("normal", np.float32), ("min_dist", np.float32), ("max_dist", np.float32), ("flags", np.uint8),
                     ("desc", np.uint8), ("track_depth", np.float32)):
        if points.get(name) is not None:
            keep[name] = np.ascontiguousarray(points[name], dt)
    P = LocalPoints()
    for name, a in keep.items():
        setattr(P, name, a.ctypes.data if a.size else None)
    P.n = len(keep["flags"]) if "flags" in keep else int(points.get("n", 0))
    npts = max(P.n, 1)
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    n = len(kp)
    tm = np.ascontiguousarray(train_match, np.int32).copy()
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    mi = None if mirror is None else np.ascontiguousarray(mirror, np.int32)
    track = np.zeros(npts, TRACK_RECORD_DTYPE); owner = np.full(2 * npts, -1, np.int32)
    ntm = np.zeros(1, np.int32); nq = np.zeros(1, np.int32); nm = np.zeros(1, np.int32)
    tail = (bounds[0], bounds[1], bounds[2], bounds[3], th_high, nn_ratio, track.ctypes.data, ntm.ctypes.data, owner.ctypes.data, nq.ctypes.data,
            tm.ctypes.data if n else None, nm.ctypes.data)
    if d_desc is not None:
        _chk(lib.orbhip_search_local_points_host_resident(ctx.h, f.ctypes.data, C.addressof(P), kp.ctypes.data if n else None, d_kp, d_desc,
                                                          None if ur is None else ur.ctypes.data, n, *tail), "orbhip_search_local_points_host_resident")
    else:
        d = np.ascontiguousarray(desc, np.uint8)
        _chk(lib.orbhip_search_local_points_host(ctx.h, f.ctypes.data, C.addressof(P), kp.ctypes.data if n else None, d.ctypes.data if n else None,
                                                 None if ur is None else ur.ctypes.data, n, nleft, None if mi is None else mi.ctypes.data, *tail),
             "orbhip_search_local_points_host")
    return track[:P.n], int(ntm[0]), owner[:int(nq[0])].copy(), tm, int(nm[0])


# ---------------------------------------------------------------- KeyFrameDatabase: batched BoW place recognition
KFDB_PLACE, KFDB_RELOC, KFDB_NEIGHBOURS, KFDB_MAX_WORDS, KFDB_MAX_LIST = 0, 1, 10, 4096, 4096
KFDB_QUERY_DTYPE = np.dtype([("id", "<u8"), ("map_id", "<i4"), ("mode", "<i4")])
KFDB_ENTRY_DTYPE = np.dtype([("slot", "<i4"), ("words", "<i4"), ("scored", "<i4"), ("score", "<f4")])
KFDB_CANDIDATE_DTYPE = np.dtype([("slot", "<i4"), ("score", "<f4"), ("acc_score", "<f4"), ("best_slot", "<i4")])
KFDB_STATE_DTYPE = np.dtype([("query", "<u8", (2,)), ("words", "<i4", (2,)), ("score", "<f4", (2,)), ("n_words", "<i4"), ("alive", "<i4"),
                             ("map_id", "<i4"), ("sequence", "<u4")])
assert KFDB_QUERY_DTYPE.itemsize == 16 and KFDB_ENTRY_DTYPE.itemsize == 16 and KFDB_CANDIDATE_DTYPE.itemsize == 16 and KFDB_STATE_DTYPE.itemsize == 48
lib.orbhip_kfdb_create.argtypes = [vp, ci, ci, C.POINTER(vp)]
lib.orbhip_kfdb_destroy.argtypes = [vp]
lib.orbhip_kfdb_destroy.restype = None
lib.orbhip_kfdb_add_device.argtypes = [vp, ci, ci, vp, vp, vp]
lib.orbhip_kfdb_add_host.argtypes = [vp, ci, ci, vp, vp, ci]
lib.orbhip_kfdb_erase.argtypes = [vp, ci]
lib.orbhip_kfdb_clear_map.argtypes = [vp, ci]
lib.orbhip_kfdb_clear.argtypes = [vp]
lib.orbhip_kfdb_reset_slot.argtypes = [vp, ci]
lib.orbhip_kfdb_get_state_host.argtypes = [vp, ci, ci, vp]
lib.orbhip_kfdb_score_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, ci, vp, vp]
lib.orbhip_kfdb_detect_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, vp, ci, vp, ci, ci] + [vp] * 8
lib.orbhip_kfdb_score_host.argtypes = [vp, vp, vp, vp, ci, vp, ci, ci, vp, vp]


class KeyFrameDB:
    """orbhip_kfdb: the device-resident database handle (kfdb_create); close() destroys it"""
    def __init__(self, h, capacity, max_words):
        self.h, self.capacity, self.max_words = h, capacity, max_words

    def close(self):
        if self.h:
            lib.orbhip_kfdb_destroy(self.h)
            self.h = None


def kfdb_create(ctx, capacity, max_words):
    h = vp()
    _chk(lib.orbhip_kfdb_create(ctx.h if ctx is not None else None, int(capacity), int(max_words), C.byref(h)), "orbhip_kfdb_create")
    return KeyFrameDB(h, int(capacity), int(max_words))


def kfdb_add_device(db, slot, map_id, d_word, d_value, d_nwords):
    """KeyFrameDatabase::add from one row of bow_vectors_device's outputs: device addresses (ints) of the row's words, values and count"""
    _chk(lib.orbhip_kfdb_add_device(db.h, int(slot), int(map_id), d_word, d_value, d_nwords), "orbhip_kfdb_add_device")


def kfdb_add_host(db, slot, map_id, word, value):
    w = np.ascontiguousarray(word, np.int32); v = np.ascontiguousarray(value, np.float64)
    assert len(w) == len(v)
    _chk(lib.orbhip_kfdb_add_host(db.h, int(slot), int(map_id), w.ctypes.data if len(w) else None, v.ctypes.data if len(w) else None, len(w)),
         "orbhip_kfdb_add_host")


def kfdb_erase(db, slot):
    _chk(lib.orbhip_kfdb_erase(db.h, int(slot)), "orbhip_kfdb_erase")


def kfdb_clear_map(db, map_id):
    _chk(lib.orbhip_kfdb_clear_map(db.h, int(map_id)), "orbhip_kfdb_clear_map")


def kfdb_clear(db):
    _chk(lib.orbhip_kfdb_clear(db.h), "orbhip_kfdb_clear")


def kfdb_reset_slot(db, slot):
    _chk(lib.orbhip_kfdb_reset_slot(db.h, int(slot)), "orbhip_kfdb_reset_slot")


def kfdb_get_state(db, first=0, n=None):
    """the slots' stored state and bookkeeping after everything submitted so far -> [n] KFDB_STATE_DTYPE (synchronous)"""
    n = db.capacity - first if n is None else n
    out = np.zeros(max(n, 1), KFDB_STATE_DTYPE)
    _chk(lib.orbhip_kfdb_get_state_host(db.h, int(first), int(n), out.ctypes.data), "orbhip_kfdb_get_state_host")
    return out[:max(n, 0)]


def _kfdb_queries(query):
    q = np.ascontiguousarray(query).reshape(-1)
    assert q.dtype == KFDB_QUERY_DTYPE
    return q


def kfdb_score_device(db, query, d_qword, d_qvalue, d_qn, q_stride, d_connected, d_nconnected, max_connected, max_list, d_counts, d_list):
    """The sharing lists and scores of len(query) queries; query: HOST records (KFDB_QUERY_DTYPE), everything else device addresses
    (ints; d_connected / d_nconnected may be None with max_connected 0); asynchronous."""
    q = _kfdb_queries(query)
    _chk(lib.orbhip_kfdb_score_device(db.h if db is not None else None, q.ctypes.data, len(q), d_qword, d_qvalue, d_qn, int(q_stride), d_connected,
                                      d_nconnected, int(max_connected), int(max_list), d_counts, d_list), "orbhip_kfdb_score_device")


def kfdb_detect_device(db, query, d_qword, d_qvalue, d_qn, q_stride, d_connected, d_nconnected, max_connected, d_neighbours, n_candidates,
                       bad_maps, max_list, d_counts, d_list, d_scored, d_loop, d_merge, d_ncand, d_reloc, d_nreloc):
    """DetectNBestCandidates / DetectRelocalizationCandidates for len(query) queries in index order; bad_maps: host list of map ids."""
    q = _kfdb_queries(query)
    bad = np.ascontiguousarray(bad_maps if bad_maps is not None else [], np.int32)
    _chk(lib.orbhip_kfdb_detect_device(db.h if db is not None else None, q.ctypes.data, len(q), d_qword, d_qvalue, d_qn, int(q_stride), d_connected,
                                       d_nconnected, int(max_connected), d_neighbours, int(n_candidates), bad.ctypes.data if len(bad) else None,
                                       len(bad), int(max_list), d_counts, d_list, d_scored, d_loop, d_merge, d_ncand, d_reloc, d_nreloc),
         "orbhip_kfdb_detect_device")


def kfdb_score_host(db, qid, map_id, mode, word, value, connected=(), max_list=KFDB_MAX_LIST):
    """One query from host arrays -> (counts [4] = n_sharing, max_common, n_scored, n_touched; list [n_sharing] KFDB_ENTRY_DTYPE;
    touched [n_touched] KFDB_ENTRY_DTYPE: slots whose words changed without being listed)."""
    q = np.zeros(1, KFDB_QUERY_DTYPE); q["id"], q["map_id"], q["mode"] = qid, map_id, mode
    w = np.ascontiguousarray(word, np.int32); v = np.ascontiguousarray(value, np.float64); c = np.ascontiguousarray(connected, np.int32)
    assert len(w) == len(v)
    counts = np.zeros(4, np.int32); lst = np.zeros(max(int(max_list), 1), KFDB_ENTRY_DTYPE)
    _chk(lib.orbhip_kfdb_score_host(db.h if db is not None else None, q.ctypes.data, w.ctypes.data if len(w) else None,
                                    v.ctypes.data if len(w) else None, len(w), c.ctypes.data if len(c) else None, len(c), int(max_list),
                                    counts.ctypes.data, lst.ctypes.data), "orbhip_kfdb_score_host")
    return counts, lst[:counts[0]].copy(), lst[counts[0]:counts[0] + counts[3]].copy()
