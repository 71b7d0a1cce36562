"""ctypes binding of libreze_deform.so (include/reze_deform.h) for bench.py and the GPU tests.

This is plumbing only: every method is a 1:1 call of a C-ABI entry point, so the parity tests
exercise exactly what the N-API addon binds. There is deliberately no CPU fallback — if the HIP
library is missing or no MI355X is visible, construction raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libreze_deform.so")

# every symbol include/reze_deform.h declares (tests check the library exports all of them)
SYMBOLS = [
    "rz_last_error", "rz_abi_version", "rz_device_count", "rz_device_numa_node", "rz_create", "rz_destroy", "rz_shard_range", "rz_gather_chunk",
    "rz_upload_mesh", "rz_upload_mesh_soa", "rz_upload_skeleton", "rz_upload_morphs_dense",
    "rz_upload_morphs_sparse", "rz_set_instances", "rz_set_pose", "rz_upload_skeleton_topology", "rz_set_pose_local", "rz_upload_bone_morphs", "rz_upload_animation", "rz_set_pose_sampled", "rz_override_world", "rz_read_world", "rz_deform", "rz_deform_n", "rz_fork", "rz_deform_pair", "rz_sync", "rz_read",
    "rz_read_palette", "rz_time_frames", "rz_set_tuning", "rz_get_tuning", "rz_autotune", "rz_autotune_measure", "rz_autotune_pick",
    "rz_autotune_apply", "rz_output_ptrs",
    "rz_comm_unique_id", "rz_rccl_info", "rz_comm_info", "rz_comm_init", "rz_allgather", "rz_read_gathered", "rz_comm_init_all", "rz_allgather_all", "rz_gather_direct", "rz_gather_fence", "rz_upload_edge_scale", "rz_read_hull", "rz_enable_aabb", "rz_read_aabb",
    "rz_instance_range", "rz_map_pose", "rz_commit_pose", "rz_time_span", "rz_upload_sdef", "rz_upload_ik",
    "rz_upload_qdef", "rz_upload_motions", "rz_set_pose_blended", "rz_upload_motion_masks", "rz_set_pose_layered",
    "rz_upload_physics", "rz_physics_step", "rz_physics_reset", "rz_read_physics", "rz_physics_contacts", "rz_physics_springs",
    "rz_override_follow", "rz_set_ik_enabled", "rz_upload_ik_keys", "rz_read_ik_enabled", "rz_upload_after_physics", "rz_physics_aligned",
    "rz_upload_morphs_dense_ex", "rz_read_morph_dense", "rz_morph_encode24",
]
# symbols a library older than the current ABI lacks (ABI 5: rz_gather_chunk; 6: rz_device_numa_node; 7: rz_instance_range ..
# rz_time_span; 8: rz_upload_sdef, later rz_upload_ik, rz_upload_qdef, rz_upload_motions, rz_set_pose_blended, the four physics entry
# points, rz_physics_contacts, rz_physics_springs, rz_upload_motion_masks, rz_set_pose_layered, rz_override_follow and the three chain-switch entry
# points (rz_set_ik_enabled ..), then rz_upload_after_physics and rz_physics_aligned — detected by the symbol, the version stayed 8)
OPTIONAL_SYMBOLS = {"rz_gather_chunk", "rz_device_numa_node", "rz_instance_range", "rz_map_pose", "rz_commit_pose", "rz_time_span", "rz_upload_sdef",
                    "rz_upload_ik", "rz_upload_qdef", "rz_upload_motions", "rz_set_pose_blended", "rz_upload_motion_masks", "rz_set_pose_layered",
                    "rz_upload_physics", "rz_physics_step", "rz_physics_reset", "rz_read_physics", "rz_physics_contacts", "rz_physics_springs", "rz_override_follow",
                    "rz_set_ik_enabled", "rz_upload_ik_keys", "rz_read_ik_enabled", "rz_upload_after_physics", "rz_physics_aligned",
                    "rz_upload_morphs_dense_ex", "rz_read_morph_dense", "rz_morph_encode24"}       # (24-bit dense morph storage)
POSE_WORLD16, POSE_ROWS12 = 0, 1
MORPH_F32 = 1       # upload_morphs_dense(storage=): fp32 planes instead of the default 24-bit storage


def morph_encode24(deltas):
    """The library's 24-bit dense morph encoder on the host (no device): (storage, scales[M], packed[M, 3, ceil(V / 4) * 12] uint8 or None)."""
    d = _f32(deltas)
    assert d.ndim == 3 and d.shape[2] == 3, d.shape
    M, V = d.shape[0], d.shape[1]
    L = load()
    packed = np.zeros((M, 3, (V + 3) // 4 * 12), dtype=np.uint8)
    scales = np.zeros(M, dtype=np.float32)
    storage = ctypes.c_int(0)
    rc = L.rz_morph_encode24(_fptr(d), M, V, packed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _fptr(scales), ctypes.byref(storage))
    if rc != 0:
        raise RzError(rc, (L.rz_last_error() or b"").decode())
    return storage.value, (scales if storage.value == 24 else None), (packed if storage.value == 24 else None)
NO_CLIP = 0xffffffff
NO_MASK = 0xffffffff
MAX_MOTION_LAYERS = 4
LAYER_OVERRIDE, LAYER_ADDITIVE = 0, 1


class RzAnimation(ctypes.Structure):
    _fields_ = [("n_bone_tracks", ctypes.c_uint32), ("track_bone", ctypes.POINTER(ctypes.c_int32)),
                ("key_off", ctypes.POINTER(ctypes.c_uint32)), ("key_frame", ctypes.POINTER(ctypes.c_float)),
                ("key_rot4", ctypes.POINTER(ctypes.c_float)), ("key_pos3", ctypes.POINTER(ctypes.c_float)),
                ("key_interp16", ctypes.POINTER(ctypes.c_uint8)), ("n_morph_tracks", ctypes.c_uint32),
                ("mkey_off", ctypes.POINTER(ctypes.c_uint32)), ("mkey_frame", ctypes.POINTER(ctypes.c_float)),
                ("mkey_weight", ctypes.POINTER(ctypes.c_float)), ("feed_off", ctypes.POINTER(ctypes.c_uint32)),
                ("feed_track", ctypes.POINTER(ctypes.c_int32)), ("feed_ratio", ctypes.POINTER(ctypes.c_float))]


class RzMotionState(ctypes.Structure):
    _fields_ = [("clip_a", ctypes.c_uint32), ("frame_a", ctypes.c_float), ("clip_b", ctypes.c_uint32), ("frame_b", ctypes.c_float),
                ("blend", ctypes.c_float)]


class RzMotionLayer(ctypes.Structure):
    _fields_ = [("clip", ctypes.c_uint32), ("frame", ctypes.c_float), ("weight", ctypes.c_float), ("mask", ctypes.c_uint32),
                ("mode", ctypes.c_uint32)]


class RzIkKeys(ctypes.Structure):
    _fields_ = [("n_keys", ctypes.c_uint32), ("key_frame", ctypes.POINTER(ctypes.c_float)), ("key_enabled", ctypes.POINTER(ctypes.c_uint8))]


class RzPhysics(ctypes.Structure):
    _f, _u8, _u32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    _fields_ = [("n_bodies", ctypes.c_uint32), ("bone", ctypes.POINTER(ctypes.c_int32)), ("type", _u8), ("shape", _u8),
                ("size3", _f), ("offset_pos3", _f), ("offset_rot4", _f), ("mass", _f), ("linear_damping", _f), ("angular_damping", _f),
                ("restitution", _f), ("friction", _f), ("group", _u8), ("mask", ctypes.POINTER(ctypes.c_uint16)),
                ("n_joints", ctypes.c_uint32), ("body_a", _u32), ("body_b", _u32), ("position3", _f), ("rotation3", _f),
                ("position_min3", _f), ("position_max3", _f), ("rotation_min3", _f), ("rotation_max3", _f),
                ("spring_position3", _f), ("spring_rotation3", _f), ("gravity3", _f), ("h", ctypes.c_float), ("iterations", ctypes.c_uint32)]


# the same 20 bytes as a numpy record (set_pose_blended packs a crowd's states with it)
MOTION_STATE_DTYPE = np.dtype([("clip_a", "<u4"), ("frame_a", "<f4"), ("clip_b", "<u4"), ("frame_b", "<f4"), ("blend", "<f4")])

# the 20-byte rz_motion_layer as a numpy record (set_pose_layered packs [I, n_layers] of them)
MOTION_LAYER_DTYPE = np.dtype([("clip", "<u4"), ("frame", "<f4"), ("weight", "<f4"), ("mask", "<u4"), ("mode", "<u4")])


def _animation_struct(a, keep, track_bone, key_off, key_frame, key_rot, key_pos, key_interp=None,
                      mkey_off=None, mkey_frame=None, mkey_weight=None, feed_off=None, feed_track=None, feed_ratio=None):
    """Fill the rz_animation `a` from a flattened motion; the arrays it points at are appended to `keep`."""
    def arr(x, dt, ct):
        if x is None:
            return None
        v = np.ascontiguousarray(x, dtype=dt).reshape(-1)
        keep.append(v)
        return v.ctypes.data_as(ctypes.POINTER(ct))
    a.n_bone_tracks = len(track_bone)
    a.track_bone = arr(track_bone, np.int32, ctypes.c_int32)
    a.key_off = arr(key_off, np.uint32, ctypes.c_uint32)
    a.key_frame = arr(key_frame, np.float32, ctypes.c_float)
    a.key_rot4 = arr(key_rot, np.float32, ctypes.c_float)
    a.key_pos3 = arr(key_pos, np.float32, ctypes.c_float)
    a.key_interp16 = arr(key_interp, np.uint8, ctypes.c_uint8)
    a.n_morph_tracks = 0 if mkey_off is None else len(mkey_off) - 1
    a.mkey_off = arr(mkey_off, np.uint32, ctypes.c_uint32)
    a.mkey_frame = arr(mkey_frame, np.float32, ctypes.c_float)
    a.mkey_weight = arr(mkey_weight, np.float32, ctypes.c_float)
    a.feed_off = arr(feed_off, np.uint32, ctypes.c_uint32)
    a.feed_track = arr(feed_track, np.int32, ctypes.c_int32)
    a.feed_ratio = arr(feed_ratio, np.float32, ctypes.c_float)


class RzTiming(ctypes.Structure):
    _fields_ = [("frame_ms", ctypes.c_double), ("deform_kernel_ms", ctypes.c_double),
                ("prep_kernel_ms", ctypes.c_double), ("verts_per_frame", ctypes.c_uint64),
                ("algorithmic_bytes_per_frame", ctypes.c_uint64), ("frames", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class RzTuneEntry(ctypes.Structure):
    _fields_ = [("morph_split", ctypes.c_int), ("grid_cap", ctypes.c_int), ("inst_loop", ctypes.c_int),
                ("eff_split", ctypes.c_int), ("eff_grid", ctypes.c_int), ("eff_inst_group", ctypes.c_int),
                ("same_as", ctypes.c_int), ("ms", ctypes.c_float), ("ms_min", ctypes.c_float), ("ms_max", ctypes.c_float)]


class RzError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("reze_deform error %d: %s" % (code, message))
        self.code = code


_lib = None
_libs = {}
# the tools-only build that carries EVERY kernel variant (make -C reze-engine_amd/csrc variants): the parity tests reach the
# variants the product does not ship through it; nothing in the product, bench.py or host/ loads it
VARIANTS_LIB_PATH = os.path.join(os.path.dirname(_HERE), "tools", "variants", "libreze_deform_variants.so")


def load(path=None):
    """dlopen the in-tree HIP library (or, for tests / tools, another build of it given by `path`); raises (never falls
    back) when it is missing. Each build is bound once; their exported names are the same, so they are loaded RTLD_LOCAL
    and linked -Bsymbolic-functions: a call inside one build never lands in another."""
    global _lib
    if path is None:
        if _lib is not None:
            return _lib
        path = LIB_PATH
    path = os.path.abspath(path)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError("%s not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    L = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    vp = ctypes.c_void_p
    fp = ctypes.POINTER(ctypes.c_float)
    u32 = ctypes.c_uint32
    L.rz_last_error.restype = ctypes.c_char_p
    L.rz_last_error.argtypes = []
    L.rz_abi_version.argtypes = []
    L.rz_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "rz_device_numa_node"):      # (absent from libraries older than ABI 6)
        L.rz_device_numa_node.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.rz_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.rz_destroy.argtypes = [vp]
    L.rz_shard_range.argtypes = [u32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    if hasattr(L, "rz_gather_chunk"):          # (absent from libraries older than ABI 5, which tools/ab_inproc.py loads for A/B runs)
        L.rz_gather_chunk.argtypes = [u32, ctypes.c_int, ctypes.POINTER(u32)]
    L.rz_upload_mesh.argtypes = [vp, u32, fp, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint8)]
    L.rz_upload_mesh_soa.argtypes = [vp, u32, fp, fp, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint8)]
    L.rz_upload_skeleton.argtypes = [vp, u32, fp]
    L.rz_upload_morphs_dense.argtypes = [vp, u32, fp]
    L.rz_upload_morphs_sparse.argtypes = [vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), fp]
    L.rz_set_instances.argtypes = [vp, u32]
    L.rz_set_pose.argtypes = [vp, fp, fp]
    i32p = ctypes.POINTER(ctypes.c_int32)
    L.rz_upload_skeleton_topology.argtypes = [vp, u32, i32p, fp, i32p, fp, ctypes.POINTER(ctypes.c_uint8)]
    L.rz_set_pose_local.argtypes = [vp, fp, fp, fp]
    L.rz_upload_animation.argtypes = [vp, ctypes.POINTER(RzAnimation)]
    L.rz_set_pose_sampled.argtypes = [vp, fp]
    L.rz_override_world.argtypes = [vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), fp]
    L.rz_upload_bone_morphs.argtypes = [vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), fp, fp]
    L.rz_read_world.argtypes = [vp, u32, fp]
    L.rz_deform.argtypes = [vp]
    L.rz_deform_n.argtypes = [vp, u32]
    L.rz_fork.argtypes = [vp, ctypes.POINTER(vp)]
    L.rz_deform_pair.argtypes = [vp, vp, u32]
    L.rz_sync.argtypes = [vp]
    L.rz_read.argtypes = [vp, u32, u32, u32, fp, fp]
    L.rz_read_palette.argtypes = [vp, u32, fp]
    L.rz_time_frames.argtypes = [vp, u32, ctypes.POINTER(RzTiming)]
    L.rz_autotune.argtypes = [vp, u32]
    L.rz_autotune_measure.argtypes = [vp, u32, ctypes.POINTER(RzTuneEntry), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.rz_autotune_pick.argtypes = [ctypes.POINTER(RzTuneEntry), ctypes.c_int]
    L.rz_autotune_apply.argtypes = [vp, ctypes.POINTER(RzTuneEntry)]
    L.rz_comm_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.rz_set_tuning.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    L.rz_get_tuning.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    L.rz_output_ptrs.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(u32)]
    L.rz_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.rz_rccl_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.rz_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, u32]
    L.rz_allgather.argtypes = [vp, ctypes.c_int]
    L.rz_read_gathered.argtypes = [vp, u32, u32, fp, fp]
    L.rz_upload_edge_scale.argtypes = [vp, u32, fp]
    L.rz_read_hull.argtypes = [vp, u32, u32, u32, fp]
    L.rz_enable_aabb.argtypes = [vp, ctypes.c_int]
    L.rz_read_aabb.argtypes = [vp, u32, fp]
    L.rz_comm_init_all.argtypes = [ctypes.POINTER(vp), ctypes.c_int, u32]
    L.rz_allgather_all.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int]
    L.rz_gather_direct.argtypes = [ctypes.POINTER(vp), ctypes.c_int, u32, ctypes.c_int]
    L.rz_gather_fence.argtypes = [vp]
    if hasattr(L, "rz_map_pose"):              # (ABI 7)
        L.rz_instance_range.argtypes = [u32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.rz_map_pose.argtypes = [vp, ctypes.c_int, ctypes.POINTER(fp), ctypes.POINTER(fp)]
        L.rz_commit_pose.argtypes = [vp]
        L.rz_time_span.argtypes = [vp, vp, u32, u32, ctypes.POINTER(ctypes.c_double)]
    if hasattr(L, "rz_upload_sdef"):           # (ABI 8)
        L.rz_upload_sdef.argtypes = [vp, u32, ctypes.POINTER(u32), fp, fp, fp]
    if hasattr(L, "rz_upload_qdef"):           # (ABI 8 still: the feature is detected by the symbol)
        L.rz_upload_qdef.argtypes = [vp, u32, ctypes.POINTER(u32)]
    if hasattr(L, "rz_upload_motions"):        # (ABI 8 still: the feature is detected by the symbols)
        L.rz_upload_motions.argtypes = [vp, u32, ctypes.POINTER(RzAnimation)]
        L.rz_set_pose_blended.argtypes = [vp, ctypes.POINTER(RzMotionState)]
    if hasattr(L, "rz_set_pose_layered"):      # (ABI 8 still: the feature is detected by the symbols)
        L.rz_upload_motion_masks.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)]
        L.rz_set_pose_layered.argtypes = [vp, ctypes.POINTER(RzMotionState), u32, ctypes.POINTER(RzMotionLayer)]
    if hasattr(L, "rz_upload_ik"):             # (ABI 8 still: the feature is detected by the symbol)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        L.rz_upload_ik.argtypes = [vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32), fp, ctypes.POINTER(u32), ctypes.POINTER(u32), u8p, fp, fp]
    if hasattr(L, "rz_upload_physics"):        # (ABI 8 still: the feature is detected by the symbols)
        L.rz_upload_physics.argtypes = [vp, ctypes.POINTER(RzPhysics)]
        L.rz_physics_step.argtypes = [vp, u32]
        L.rz_physics_reset.argtypes = [vp]
        L.rz_read_physics.argtypes = [vp, u32, fp]
    if hasattr(L, "rz_physics_contacts"):
        L.rz_physics_contacts.argtypes = [vp, u32]
    if hasattr(L, "rz_physics_springs"):
        L.rz_physics_springs.argtypes = [vp, u32]
    if hasattr(L, "rz_physics_aligned"):
        L.rz_physics_aligned.argtypes = [vp, u32]
    if hasattr(L, "rz_override_follow"):
        L.rz_override_follow.argtypes = [vp, u32]
    if hasattr(L, "rz_upload_morphs_dense_ex"):
        L.rz_upload_morphs_dense_ex.argtypes = [vp, u32, fp, u32]
        L.rz_read_morph_dense.argtypes = [vp, u32, fp]
        L.rz_morph_encode24.argtypes = [fp, u32, u32, ctypes.POINTER(ctypes.c_uint8), fp, ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "rz_upload_after_physics"):
        L.rz_upload_after_physics.argtypes = [vp, u32, ctypes.POINTER(u32)]
    if hasattr(L, "rz_upload_ik_keys"):
        L.rz_set_ik_enabled.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8)]
        L.rz_upload_ik_keys.argtypes = [vp, u32, ctypes.POINTER(RzIkKeys)]
        L.rz_read_ik_enabled.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8)]
    for name in SYMBOLS:
        # (libraries older than the current ABI — tools/ab_inproc.py loads them side by side — lack the newer symbols: OPTIONAL_SYMBOLS)
        if name != "rz_last_error" and (name not in OPTIONAL_SYMBOLS or hasattr(L, name)):
            getattr(L, name).restype = ctypes.c_int
    _libs[path] = L
    if path == os.path.abspath(LIB_PATH):
        _lib = L
    return L


def _chk(code, L=None):
    if code != 0:
        raise RzError(code, (L or load()).rz_last_error().decode("utf-8", "replace"))


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count():
    n = ctypes.c_int(0)
    rc = load().rz_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def shard_range(v_total, nranks, rank):
    """Pure host helper (works without a GPU): (begin, count) of `rank`'s vertex shard."""
    b = ctypes.c_uint32(0)
    n = ctypes.c_uint32(0)
    _chk(load().rz_shard_range(int(v_total), int(nranks), int(rank), ctypes.byref(b), ctypes.byref(n)))
    return b.value, n.value


def instance_range(instances, nranks, rank):
    """Pure host helper: (begin, count) of the instances `rank` poses when a crowd is sharded along the instance axis."""
    b = ctypes.c_uint32(0)
    n = ctypes.c_uint32(0)
    _chk(load().rz_instance_range(int(instances), int(nranks), int(rank), ctypes.byref(b), ctypes.byref(n)))
    return b.value, n.value


def gather_chunk(v_total, nranks):
    """Pure host helper: the stride, in vertices, between two ranks' blocks of the gathered buffers."""
    c = ctypes.c_uint32(0)
    _chk(load().rz_gather_chunk(int(v_total), int(nranks), ctypes.byref(c)))
    return c.value


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    _chk(load().rz_comm_unique_id(buf))
    return buf.raw


def rccl_info():
    """{path, version, reused}: the RCCL the library bound (reused = a copy the process had already loaded, e.g. PyTorch's)."""
    buf = ctypes.create_string_buffer(512)
    ver, reused = ctypes.c_int(0), ctypes.c_int(0)
    _chk(load().rz_rccl_info(buf, 512, ctypes.byref(ver), ctypes.byref(reused)))
    return {"path": buf.value.decode("utf-8", "replace"), "version": ver.value, "reused": bool(reused.value)}


def comm_init_all(contexts, v_total):
    """Single-process multi-GPU: contexts[r] is rank r (ncclCommInitAll)."""
    arr = (ctypes.c_void_p * len(contexts))(*[c._h for c in contexts])
    _chk(load().rz_comm_init_all(arr, len(contexts), int(v_total)))
    for c in contexts:
        c.v_total = int(v_total)


def device_numa_node(device=0, lib=None):
    """NUMA node of the host the device hangs off (rz_device_numa_node), -1 when the system does not say."""
    L = lib if lib is not None else load()
    n = ctypes.c_int(-1)
    _chk(L.rz_device_numa_node(int(device), ctypes.byref(n)), L)
    return n.value


def bind_to_device_node(device=0, lib=None):
    """Restrict the calling process to the cores of the device's NUMA node (what numactl --cpunodebind does): per-frame inputs cross the
    host link, and feeding a GPU from the other socket costs host time per HIP call and link bandwidth per pulled byte
    (include/reze_deform.h: rz_device_numa_node). Call it before contexts are created — pinned rings are first touched by the thread that
    creates them. Returns {"gpu_node": n, "cpus": "64-127,192-255"} or None when there is nothing to do (unknown node, one node,
    the node's cores are outside the affinity mask the process was given)."""
    node = device_numa_node(device, lib)
    if node < 0 or not hasattr(os, "sched_setaffinity"):
        return None
    try:
        with open("/sys/devices/system/node/node%d/cpulist" % node) as f:
            text = f.read().strip()
        if len([d for d in os.listdir("/sys/devices/system/node") if d.startswith("node") and d[4:].isdigit()]) < 2:
            return None
    except OSError:
        return None
    cpus = set()
    for part in text.split(","):
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    cpus &= os.sched_getaffinity(0)
    if not cpus:
        return None
    os.sched_setaffinity(0, cpus)
    return {"gpu_node": node, "cpus": text}


def allgather_all(contexts, with_normals=False):
    arr = (ctypes.c_void_p * len(contexts))(*[c._h for c in contexts])
    _chk(load().rz_allgather_all(arr, len(contexts), 1 if with_normals else 0))


def gather_direct(contexts, v_total, root=0):
    """Peer-direct gather: every context's kernels store their shard straight into contexts[root]'s gathered
    buffer (no collective). contexts[r] holds shard r; read the whole mesh with contexts[root].read_gathered()."""
    arr = (ctypes.c_void_p * len(contexts))(*[c._h for c in contexts])
    _chk(load().rz_gather_direct(arr, len(contexts), int(v_total), int(root)))
    for c in contexts:
        c.v_total = int(v_total)


KERNEL_NAME_KEYS = ("morph_mode", "effective_split", "effective_unroll", "effective_nt", "effective_nt_store", "effective_geo", "effective_fast", "effective_variant",
                    "effective_inst_group", "effective_inst_block", "effective_subsets", "effective_fuse_fk", "effective_inst_morphs", "effective_poses_per_wg")


def kernel_name_of(keys):
    """The frame kernel's name from the values of KERNEL_NAME_KEYS (rz_get_tuning; the library reads them off its one kernel record,
    csrc/frame_kernel.h), spelled like the demangled symbol — except that the dense kernel's eighth template argument (Q24: 24-bit morph
    planes) is OMITTED. It stays omitted: stored profiles (profiles/pmc_traffic.json) and bench lines are keyed on this string as it is."""
    tf = lambda k: "true" if keys[k] else "false"  # noqa: E731
    if keys["effective_poses_per_wg"] > 0:
        return "rz_skin_instances_reg_kernel<8, %s>" % tf("effective_nt_store")
    if keys["effective_inst_group"] > 0:
        morph = "_morph" if keys["effective_inst_morphs"] else ""     # sparse targets walked in the crowd kernels (kernels/crowd_morph.hip)
        if keys["effective_fuse_fk"]:                                 # the hierarchy solved in the crowd kernel's front
            return "rz_skin_instances_fk%s_kernel<%d, %s>" % (morph, keys["effective_inst_block"], tf("effective_nt_store"))
        return "rz_skin_instances%s_kernel<%d, %s, %s>" % (morph, keys["effective_inst_block"], tf("effective_nt_store"), tf("effective_subsets"))
    mode, s_ = keys["morph_mode"], keys["effective_split"]
    if mode == 1:
        return "rz_deform_dense_kernel<%d, %d, %s, %s, %s, %s, %d>" % (s_, 8 if keys["effective_unroll"] >= 8 else 4, tf("effective_nt"), tf("effective_nt_store"),
                                                                       tf("effective_geo"), tf("effective_fast"), keys["effective_variant"])
    return "rz_deform_small_kernel<%d, %d, %s, %s, %s, %d>" % (4 if s_ >= 4 else 1, mode, tf("effective_nt_store"), tf("effective_geo"), tf("effective_fast"), keys["effective_variant"])


class DeformContext:
    """One GPU's deformation context (rz_ctx)."""

    def __init__(self, device=0, lib=None):
        """lib: a library returned by load(path) (tests: the all-variants build); default = the product library."""
        self._L = lib if lib is not None else load()
        h = ctypes.c_void_p()
        _chk(self._L.rz_create(int(device), ctypes.byref(h)), self._L)
        self._h = h
        self.V = 0
        self.B = 0
        self.M = 0
        self.I = 1

    def _chk(self, code):
        _chk(code, self._L)

    def close(self):
        if getattr(self, "_h", None):
            for f in list(getattr(self, "_forks", [])):       # forks borrow this context's static buffers: they go first
                f.close()
            self._L.rz_destroy(self._h)
            self._h = None
            lender = getattr(self, "_lender", None)
            if lender is not None and self in lender._forks:
                lender._forks.remove(self)

    def fork(self):
        """A second context on the same GPU that borrows this one's static data (no copy) and owns its own streams, pose
        slots and outputs: alternate frames between the two to keep two frames in flight (rz_fork)."""
        h = ctypes.c_void_p()
        self._chk(self._L.rz_fork(self._h, ctypes.byref(h)))
        f = DeformContext.__new__(DeformContext)
        f._L, f._h, f.V, f.B, f.M, f.I = self._L, h, self.V, self.B, self.M, self.I
        f._lender = self
        if not hasattr(self, "_forks"):
            self._forks = []
        self._forks.append(f)
        return f

    def deform_pair(self, other, frames):
        """`frames` frames alternating between this context and `other` (each on its own stream, into its own outputs)."""
        self._chk(self._L.rz_deform_pair(self._h, other._h, int(frames)))

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- static uploads ----
    def upload_mesh_interleaved(self, vertices8, joints4, weights4):
        v = _f32(vertices8).reshape(-1, 8)
        j = np.ascontiguousarray(joints4, dtype=np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(weights4, dtype=np.uint8).reshape(-1, 4)
        assert len(v) == len(j) == len(w)
        self._chk(self._L.rz_upload_mesh(self._h, len(v), _fptr(v), j.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                    w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        self.V = len(v)
        self.M = 0

    def upload_mesh(self, pos, nrm, joints4, weights4):
        p = _f32(pos).reshape(-1, 3)
        n = _f32(nrm).reshape(-1, 3)
        j = np.ascontiguousarray(joints4, dtype=np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(weights4, dtype=np.uint8).reshape(-1, 4)
        assert len(p) == len(n) == len(j) == len(w)
        self._chk(self._L.rz_upload_mesh_soa(self._h, len(p), _fptr(p), _fptr(n),
                                        j.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                        w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        self.V = len(p)
        self.M = 0

    def upload_skeleton(self, inverse_bind):
        ib = _f32(inverse_bind).reshape(-1, 16)
        self._chk(self._L.rz_upload_skeleton(self._h, len(ib), _fptr(ib)))
        self.B = len(ib)

    def upload_morphs_dense(self, deltas, storage=None):
        """storage: None = the library's default (24-bit integers with one scale per morph), MORPH_F32 = fp32 planes."""
        if deltas is None or len(deltas) == 0:
            self._chk(self._L.rz_upload_morphs_dense(self._h, 0, None))
            self.M = 0
            return
        d = _f32(deltas)
        assert d.ndim == 3 and d.shape[1] == self.V and d.shape[2] == 3, d.shape
        if storage is None:
            self._chk(self._L.rz_upload_morphs_dense(self._h, d.shape[0], _fptr(d)))
        else:
            if not hasattr(self._L, "rz_upload_morphs_dense_ex"):
                raise RzError(-6, "this build of the library has no rz_upload_morphs_dense_ex")
            self._chk(self._L.rz_upload_morphs_dense_ex(self._h, d.shape[0], _fptr(d), int(storage)))
        self.M = d.shape[0]

    def read_morph_dense(self, m):
        """The resident (decoded) deltas of dense morph m, [3, V] planes."""
        out = np.empty((3, self.V), dtype=np.float32)
        self._chk(self._L.rz_read_morph_dense(self._h, int(m), _fptr(out)))
        return out

    def upload_morphs_sparse(self, morph_off, vert_idx, delta3):
        mo = np.ascontiguousarray(morph_off, dtype=np.uint32)
        vi = np.ascontiguousarray(vert_idx, dtype=np.uint32)
        d = _f32(delta3).reshape(-1, 3)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._chk(self._L.rz_upload_morphs_sparse(self._h, len(mo) - 1, mo.ctypes.data_as(u32p),
                                             vi.ctypes.data_as(u32p), _fptr(d)))
        self.M = len(mo) - 1

    def set_instances(self, n):
        self._chk(self._L.rz_set_instances(self._h, int(n)))
        self.I = int(n)

    # ---- per frame ----
    def set_pose(self, world, morph_weights=None):
        w = _f32(world).reshape(-1)
        assert w.size == self.I * self.B * 16, (w.size, self.I, self.B)
        if morph_weights is not None and self.M > 0:
            mw = _f32(morph_weights).reshape(-1)
            assert mw.size == self.I * self.M
            self._chk(self._L.rz_set_pose(self._h, _fptr(w), _fptr(mw)))
        else:
            self._chk(self._L.rz_set_pose(self._h, _fptr(w), None))

    def upload_skeleton_topology(self, parents, bind_translation, append_parent=None, append_ratio=None, append_move=None):
        par = np.ascontiguousarray(parents, dtype=np.int32)
        bind = _f32(bind_translation).reshape(-1, 3)
        i32p = ctypes.POINTER(ctypes.c_int32)
        ap = None if append_parent is None else np.ascontiguousarray(append_parent, dtype=np.int32)
        ar = None if append_ratio is None else _f32(append_ratio)
        am = None if append_move is None else np.ascontiguousarray(append_move, dtype=np.uint8)
        self._chk(self._L.rz_upload_skeleton_topology(
            self._h, len(par), par.ctypes.data_as(i32p), _fptr(bind),
            None if ap is None else ap.ctypes.data_as(i32p), None if ar is None else _fptr(ar),
            None if am is None else am.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def set_pose_local(self, local_rotations, morph_weights=None, local_translations=None):
        q = _f32(local_rotations).reshape(-1)
        assert q.size == self.I * self.B * 4, (q.size, self.I, self.B)
        t = None
        if local_translations is not None:
            t = _f32(local_translations).reshape(-1)
            assert t.size == self.I * self.B * 3
        mw = None
        if morph_weights is not None and self.M > 0:
            mw = _f32(morph_weights).reshape(-1)
            assert mw.size == self.I * self.M
        self._chk(self._L.rz_set_pose_local(self._h, _fptr(q), None if t is None else _fptr(t), None if mw is None else _fptr(mw)))

    def upload_animation(self, track_bone, key_off, key_frame, key_rot, key_pos, key_interp=None,
                         mkey_off=None, mkey_frame=None, mkey_weight=None, feed_off=None, feed_track=None, feed_ratio=None):
        """Flattened motion (rz_animation): bone tracks + optional morph tracks with their per-vertex-morph feeds."""
        keep = []
        a = RzAnimation()
        _animation_struct(a, keep, track_bone, key_off, key_frame, key_rot, key_pos, key_interp, mkey_off, mkey_frame, mkey_weight,
                          feed_off, feed_track, feed_ratio)
        self._chk(self._L.rz_upload_animation(self._h, ctypes.byref(a)))

    def upload_motions(self, clips):
        """The motion library (rz_upload_motions): `clips` = a list of flattened motions, each a dict with the keyword names of
        upload_animation (track_bone, key_off, key_frame, key_rot, key_pos and optionally key_interp, mkey_off, mkey_frame, mkey_weight,
        feed_off, feed_track, feed_ratio; synth.make_motion builds such dicts). An empty list removes the library."""
        if not hasattr(self._L, "rz_upload_motions"):
            raise RzError(-6, "this build of the library has no rz_upload_motions")
        clips = list(clips)
        if not clips:
            self._chk(self._L.rz_upload_motions(self._h, 0, None))
            return
        keep = []
        arr = (RzAnimation * len(clips))()
        for k, clip in enumerate(clips):
            _animation_struct(arr[k], keep, **clip)
        self._chk(self._L.rz_upload_motions(self._h, len(clips), arr))

    @staticmethod
    def pack_motion_states(n, clip_a, frame_a, clip_b=None, frame_b=None, blend=None):
        """[n] records of MOTION_STATE_DTYPE (the 20-byte rz_motion_state); scalars are broadcast, clip_b None or negative = NO_CLIP."""
        st = np.zeros(n, dtype=MOTION_STATE_DTYPE)
        st["clip_a"] = np.asarray(clip_a, dtype=np.int64).astype(np.uint32)
        st["frame_a"] = np.asarray(frame_a, dtype=np.float32)
        if clip_b is None:
            st["clip_b"] = NO_CLIP
        else:
            cb = np.broadcast_to(np.asarray(clip_b, dtype=np.int64), (n,))
            st["clip_b"] = np.where(cb < 0, NO_CLIP, cb).astype(np.uint32)
        st["frame_b"] = 0.0 if frame_b is None else np.asarray(frame_b, dtype=np.float32)
        st["blend"] = 0.0 if blend is None else np.asarray(blend, dtype=np.float32)
        return st

    def set_pose_blended(self, clip_a, frame_a, clip_b=None, frame_b=None, blend=None):
        """One state per instance (scalars are broadcast): instance i is posed from clip_a[i] at frame_a[i], cross-faded by blend[i] into
        clip_b[i] at frame_b[i] (clip_b None / negative / NO_CLIP or blend 0: clip_a alone). Sampled and blended on the GPU
        (rz_set_pose_blended); needs upload_motions and upload_skeleton_topology."""
        if not hasattr(self._L, "rz_set_pose_blended"):
            raise RzError(-6, "this build of the library has no rz_set_pose_blended")
        st = self.pack_motion_states(self.I, clip_a, frame_a, clip_b, frame_b, blend)
        self._chk(self._L.rz_set_pose_blended(self._h, st.ctypes.data_as(ctypes.POINTER(RzMotionState))))

    def upload_motion_masks(self, bone_masks, morph_masks=None):
        """The masks of layered poses (rz_upload_motion_masks): bone_masks [n_masks, B], non-zero = the mask includes the bone; optionally
        morph_masks [n_masks, M] for the vertex morphs (None: every mask includes every morph). No masks removes them."""
        if not hasattr(self._L, "rz_upload_motion_masks"):
            raise RzError(-6, "this build of the library has no rz_upload_motion_masks")
        bm = np.ascontiguousarray(np.asarray(bone_masks) != 0, dtype=np.uint8)
        if bm.size == 0:
            self._chk(self._L.rz_upload_motion_masks(self._h, 0, None, None))
            return
        bm = np.atleast_2d(bm)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        mm = None
        if morph_masks is not None:
            mm = np.ascontiguousarray(np.atleast_2d(np.asarray(morph_masks) != 0), dtype=np.uint8)
            assert mm.shape[0] == bm.shape[0], "one morph mask per bone mask"
        self._chk(self._L.rz_upload_motion_masks(self._h, bm.shape[0], bm.ctypes.data_as(u8p), None if mm is None or mm.size == 0 else mm.ctypes.data_as(u8p)))

    @staticmethod
    def pack_motion_layers(n, layers):
        """[n, n_layers] records of MOTION_LAYER_DTYPE from a record array of that shape, or from a list of n per-instance lists of dicts
        (clip, frame, weight = 1, mask = None, mode = 0 or additive = False; shorter lists are padded with skipped layers)."""
        if isinstance(layers, np.ndarray) and layers.dtype == MOTION_LAYER_DTYPE:
            out = np.ascontiguousarray(layers)
            return out.reshape(n, -1) if out.size else out.reshape(n, 0)
        rows = [list(r) for r in layers]
        assert len(rows) == n, "%d layer lists for %d instances" % (len(rows), n)
        out = np.zeros((n, max([len(r) for r in rows] + [0])), dtype=MOTION_LAYER_DTYPE)
        out["clip"] = NO_CLIP
        for i, r in enumerate(rows):
            for l, d in enumerate(r):
                clip, mask = d.get("clip"), d.get("mask")
                mode = d.get("mode", LAYER_ADDITIVE if d.get("additive") else LAYER_OVERRIDE)
                out[i, l] = (NO_CLIP if clip is None or clip < 0 else clip, d.get("frame", 0.0), d.get("weight", 1.0),
                             NO_MASK if mask is None or mask < 0 else mask, mode)
        return out

    def set_pose_layered(self, base, layers):
        """base: [I] records of MOTION_STATE_DTYPE (pack_motion_states); layers: [I, n_layers] records of MOTION_LAYER_DTYPE or a list of
        per-instance lists of dicts (pack_motion_layers). Instance i is posed from base[i] as set_pose_blended poses it, then its layers
        are applied in order on the GPU (rz_set_pose_layered)."""
        if not hasattr(self._L, "rz_set_pose_layered"):
            raise RzError(-6, "this build of the library has no rz_set_pose_layered")
        st = np.ascontiguousarray(base, dtype=MOTION_STATE_DTYPE).reshape(-1)
        assert st.size == self.I, "%d states for %d instances" % (st.size, self.I)
        ly = self.pack_motion_layers(self.I, layers)
        n = ly.shape[1]
        self._chk(self._L.rz_set_pose_layered(self._h, st.ctypes.data_as(ctypes.POINTER(RzMotionState)), n,
                                              ly.ctypes.data_as(ctypes.POINTER(RzMotionLayer)) if n else None))

    def set_pose_sampled(self, frames):
        """One (fractional, 30 fps) frame per instance; bones, morph weights and the hierarchy are evaluated on the GPU."""
        f = _f32(np.atleast_1d(frames)).reshape(-1)
        assert f.size == self.I
        self._chk(self._L.rz_set_pose_sampled(self._h, _fptr(f)))

    def upload_bone_morphs(self, morph, bone, translation3, rotation4):
        """PMX bone morphs (type 2) for device-solved poses: entry k moves `bone[k]` by weight(morph[k]) * translation and
        right-multiplies its local rotation by slerp(identity, rotation, weight). Empty arrays clear."""
        m = np.ascontiguousarray(morph, dtype=np.uint32).reshape(-1)
        if m.size == 0:
            self._chk(self._L.rz_upload_bone_morphs(self._h, 0, None, None, None, None))
            return
        b = np.ascontiguousarray(bone, dtype=np.uint32).reshape(-1)
        t = _f32(translation3).reshape(-1)
        q = _f32(rotation4).reshape(-1)
        assert b.size == m.size and t.size == m.size * 3 and q.size == m.size * 4
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._chk(self._L.rz_upload_bone_morphs(self._h, int(m.size), m.ctypes.data_as(u32p), b.ctypes.data_as(u32p), _fptr(t), _fptr(q)))

    def override_world(self, bones, world16, instances=None):
        """Physics hand-off for device-solved poses (engine.ts:2379-2381): world matrices that replace the solved ones of
        (instance, bone) after the hierarchy solve, until the next call; empty `bones` clears."""
        b = np.ascontiguousarray(bones, dtype=np.uint32).reshape(-1)
        if b.size == 0:
            self._chk(self._L.rz_override_world(self._h, 0, None, None, None))
            return
        w = _f32(world16).reshape(-1)
        assert w.size == b.size * 16
        u32p = ctypes.POINTER(ctypes.c_uint32)
        ip = None
        if instances is not None:
            i = np.ascontiguousarray(instances, dtype=np.uint32).reshape(-1)
            assert i.size == b.size
            ip = i.ctypes.data_as(u32p)
        self._chk(self._L.rz_override_world(self._h, int(b.size), ip, b.ctypes.data_as(u32p), _fptr(w)))

    def override_follow(self, on=True):
        """Bones below an overridden bone follow it (off by default; include/reze_deform.h and tests/follow_ref.py state the stage):
        W_b = O_a (S_a^-1 S_b) with a the nearest overridden ancestor of b, for hand-fed overrides and for those rz_physics_step writes.
        Needs the topology; a new skeleton or topology clears it. `on` is passed as given: values other than 0 / 1 are refused."""
        if not hasattr(self._L, "rz_override_follow"):
            raise RzError(-6, "this build of the library has no rz_override_follow")
        self._chk(self._L.rz_override_follow(self._h, int(on)))

    def upload_after_physics(self, bones):
        """PMX after-physics bones (flag 0x1000), in evaluation order — ascending transform level, then index: the listed bones are solved
        again behind the overrides, from the final pose of the bones they read (include/reze_deform.h and tests/after_ref.py state the
        stage). An empty list removes it. Needs the topology; a new skeleton or topology clears it."""
        if not hasattr(self._L, "rz_upload_after_physics"):
            raise RzError(-6, "this build of the library has no rz_upload_after_physics")
        b = np.ascontiguousarray(bones, dtype=np.uint32).reshape(-1)
        self._chk(self._L.rz_upload_after_physics(self._h, int(b.size), b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if b.size else None))

    def read_world(self, instance=0):
        out = np.empty((self.B, 16), dtype=np.float32)
        self._chk(self._L.rz_read_world(self._h, int(instance), _fptr(out)))
        return out

    def upload_edge_scale(self, edge):
        if edge is None:
            self._chk(self._L.rz_upload_edge_scale(self._h, 0, None))
            return
        e = _f32(edge).reshape(-1)
        self._chk(self._L.rz_upload_edge_scale(self._h, len(e), _fptr(e)))

    def upload_sdef(self, idx, c, r0, r1):
        """SDEF (PMX weight type 3) for the listed vertices of this shard: idx [n] shard-relative and strictly ascending, c / r0 / r1
        [n][3] in model space. An empty `idx` removes the table."""
        i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        if i.size == 0:
            self._chk(self._L.rz_upload_sdef(self._h, 0, None, None, None, None))
            return
        cc, a, b = (_f32(x).reshape(-1) for x in (c, r0, r1))
        assert cc.size == a.size == b.size == i.size * 3, (i.size, cc.size, a.size, b.size)
        self._chk(self._L.rz_upload_sdef(self._h, int(i.size), i.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _fptr(cc), _fptr(a), _fptr(b)))

    def upload_qdef(self, idx):
        """QDEF (PMX 2.1 weight type 4, dual-quaternion blending) for the listed vertices of this shard: idx [n] shard-relative and strictly
        ascending, disjoint from the SDEF table. An empty `idx` removes the table."""
        if not hasattr(self._L, "rz_upload_qdef"):
            raise RzError(-6, "this build of the library has no rz_upload_qdef")
        i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        if i.size == 0:
            self._chk(self._L.rz_upload_qdef(self._h, 0, None))
            return
        self._chk(self._L.rz_upload_qdef(self._h, int(i.size), i.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))

    def upload_ik(self, chains):
        """PMX inverse kinematics for device-solved poses: `chains` = [dict(goal, effector, loops, limit_angle, links=[dict(bone,
        min=None | [3], max=None | [3])])], links ordered from the effector outwards, limits in radians (synth.make_ik /
        synth.make_leg_rig build such lists; the loader's bone.ik has the same fields with `goal` = the bone's own index). An empty
        list removes the table. Needs upload_skeleton_topology first."""
        chains = list(chains)
        if not hasattr(self._L, "rz_upload_ik"):
            raise RzError(-6, "this build of the library has no rz_upload_ik")
        if not chains:
            self._chk(self._L.rz_upload_ik(self._h, 0, None, None, None, None, None, None, None, None, None))
            return
        u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        goal = np.array([int(ch["goal"]) for ch in chains], dtype=np.uint32)
        eff = np.array([int(ch["effector"]) for ch in chains], dtype=np.uint32)
        loops = np.array([int(ch["loops"]) for ch in chains], dtype=np.uint32)
        theta = _f32([float(ch["limit_angle"]) for ch in chains])
        off = np.zeros(len(chains) + 1, dtype=np.uint32)
        bone, limited, lo, hi = [], [], [], []
        for k, ch in enumerate(chains):
            for ln in ch["links"]:
                has = ln.get("min") is not None and ln.get("max") is not None
                bone.append(int(ln["bone"])); limited.append(1 if has else 0)
                lo.append([float(x) for x in ln["min"]] if has else [0.0, 0.0, 0.0])
                hi.append([float(x) for x in ln["max"]] if has else [0.0, 0.0, 0.0])
            off[k + 1] = len(bone)
        n = max(len(bone), 1)
        bone_a = np.zeros(n, dtype=np.uint32); bone_a[:len(bone)] = bone
        lim_a = np.zeros(n, dtype=np.uint8); lim_a[:len(limited)] = limited
        lo_a = np.zeros((n, 3), dtype=np.float32); lo_a[:len(lo)] = np.asarray(lo, dtype=np.float32).reshape(-1, 3)
        hi_a = np.zeros((n, 3), dtype=np.float32); hi_a[:len(hi)] = np.asarray(hi, dtype=np.float32).reshape(-1, 3)
        self._chk(self._L.rz_upload_ik(self._h, len(chains), goal.ctypes.data_as(u32p), eff.ctypes.data_as(u32p), loops.ctypes.data_as(u32p),
                                       _fptr(theta), off.ctypes.data_as(u32p), bone_a.ctypes.data_as(u32p), lim_a.ctypes.data_as(u8p),
                                       _fptr(lo_a), _fptr(hi_a)))

    def _ik_chains(self):
        if not hasattr(self._L, "rz_upload_ik_keys"):
            raise RzError(-6, "this build of the library has no rz_upload_ik_keys")
        return self.get_tuning("ik_chains")

    def upload_ik_keys(self, keys, clip=None):
        """VMD IK on / off keys of a motion: `keys` = (key_frame [n], key_enabled [n][n_chains]) in upload_ik's chain order, frames
        non-descending (tests/ik_switch_ref.py: flatten makes them from a loader's ikFrames), or None to remove the set. clip = None: the
        motion of upload_animation; else a clip of the library. While a set is resident the sampling pose calls write the chain switches."""
        n_chains = self._ik_chains()
        c = NO_CLIP if clip is None else int(clip)
        if keys is None:
            self._chk(self._L.rz_upload_ik_keys(self._h, c, None))
            return
        kf = np.ascontiguousarray(keys[0], dtype=np.float32).reshape(-1)
        en = np.ascontiguousarray(np.asarray(keys[1]) != 0, dtype=np.uint8).reshape(-1)
        assert en.size == kf.size * n_chains, "%d switch bytes for %d keys of %d chains" % (en.size, kf.size, n_chains)
        k = RzIkKeys(kf.size, _fptr(kf) if kf.size else None, en.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if en.size else None)
        self._chk(self._L.rz_upload_ik_keys(self._h, c, ctypes.byref(k)))

    def set_ik_enabled(self, mask=None):
        """The chain switches of the IK stage, [I][n_chains] in upload_ik's order (non-zero = on; one row is given to every instance), or
        None = all on. The last writer wins: a sampling pose call with keys resident for its source writes them too."""
        n_chains = self._ik_chains()
        if mask is None:
            self._chk(self._L.rz_set_ik_enabled(self._h, None))
            return
        m = np.asarray(mask) != 0
        if m.size == n_chains and self.I > 1:
            m = np.broadcast_to(m.reshape(1, n_chains), (self.I, n_chains))
        m = np.ascontiguousarray(m, dtype=np.uint8).reshape(-1)
        assert m.size == self.I * n_chains, "%d switches for %d instances of %d chains" % (m.size, self.I, n_chains)
        self._chk(self._L.rz_set_ik_enabled(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def read_ik_enabled(self):
        """[I][n_chains] uint8: the chain switches the next frame's solve uses (the host's mirror; nothing is synchronised)."""
        n_chains = self._ik_chains()
        out = np.empty((self.I, max(n_chains, 1)), dtype=np.uint8)
        self._chk(self._L.rz_read_ik_enabled(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out[:, :n_chains]

    def upload_physics(self, table):
        """Rigid-body physics for device-solved poses: `table` = dict(n_bodies, bone, type, shape, size [n,3], offset_pos [n,3], offset_rot
        [n,4], mass, linear_damping, angular_damping, restitution, friction, group, mask; n_joints, body_a, body_b, position, rotation,
        position_min / _max, rotation_min / _max, spring_position, spring_rotation [m,3]; gravity [3] or None, h, iterations (0 = defaults))
        — the arrays Model.physicsTables() produces on the Node side. None or n_bodies = 0 removes the table. Needs
        upload_skeleton_topology first."""
        if not hasattr(self._L, "rz_upload_physics"):
            raise RzError(-6, "this build of the library has no rz_upload_physics")
        if table is None or int(table["n_bodies"]) == 0:
            self._chk(self._L.rz_upload_physics(self._h, None))
            return
        t, keep = RzPhysics(), []

        def arr(key, dt, ct, count):
            if key in ("group", "mask", "restitution", "friction", "spring_position") and table.get(key) is None:
                return None             # (the arrays the solver itself does not read may be NULL; physics_contacts needs group, mask, friction)
            v = np.ascontiguousarray(table[key], dtype=dt).reshape(-1)
            assert v.size == count, (key, v.size, count)
            keep.append(v)
            return v.ctypes.data_as(ctypes.POINTER(ct)) if v.size else None
        nb, nj = int(table["n_bodies"]), int(table["n_joints"])
        t.n_bodies, t.n_joints = nb, nj
        t.bone = arr("bone", np.int32, ctypes.c_int32, nb)
        t.type, t.shape, t.group = (arr(k, np.uint8, ctypes.c_uint8, nb) for k in ("type", "shape", "group"))
        t.mask = arr("mask", np.uint16, ctypes.c_uint16, nb)
        t.size3, t.offset_pos3, t.offset_rot4 = arr("size", np.float32, ctypes.c_float, nb * 3), arr("offset_pos", np.float32, ctypes.c_float, nb * 3), arr("offset_rot", np.float32, ctypes.c_float, nb * 4)
        for k in ("mass", "linear_damping", "angular_damping", "restitution", "friction"):
            setattr(t, k, arr(k, np.float32, ctypes.c_float, nb))
        t.body_a, t.body_b = arr("body_a", np.uint32, ctypes.c_uint32, nj), arr("body_b", np.uint32, ctypes.c_uint32, nj)
        for k in ("position", "rotation", "position_min", "position_max", "rotation_min", "rotation_max", "spring_position", "spring_rotation"):
            setattr(t, k + "3", arr(k, np.float32, ctypes.c_float, nj * 3))
        t.gravity3 = None if table.get("gravity") is None else arr("gravity", np.float32, ctypes.c_float, 3)
        t.h, t.iterations = float(table.get("h", 0.0)), int(table.get("iterations", 0))
        self._chk(self._L.rz_upload_physics(self._h, ctypes.byref(t)))

    def physics_step(self, substeps):
        """Advance the resident physics table by `substeps` fixed steps against the resident device-solved pose (0 = only re-place the
        following bodies and re-emit the overrides). Enqueued on the frame's stream."""
        self._chk(self._L.rz_physics_step(self._h, int(substeps)))

    def physics_reset(self):
        self._chk(self._L.rz_physics_reset(self._h))

    def physics_contacts(self, on=True, boxes=False, box_pairs=False):
        """Contacts between the spheres and capsules of the resident physics table (off by default; include/reze_deform.h states the stage).
        boxes=True: the table's boxes take part against them as well (a pair of two boxes is left out and counted in the tuning key
        physics_contact_box_pairs). box_pairs=True (implies boxes): pairs of two boxes are candidates too, counted in the tuning key
        physics_contact_box_box. A new table, skeleton or topology turns contacts off again. Does not reset the simulation."""
        if not hasattr(self._L, "rz_physics_contacts"):
            raise RzError(-6, "this build of the library has no rz_physics_contacts")
        if on and box_pairs:
            self.get_tuning("physics_contact_box_box")          # (a library without box - box contacts does not know the key: its error says so)
        elif on and boxes:
            self.get_tuning("physics_contact_box_pairs")        # (a library without box contacts does not know the key: its error says so)
        self._chk(self._L.rz_physics_contacts(self._h, (3 if box_pairs else 2 if boxes else 1) if on else 0))

    def physics_springs(self, on=True):
        """The linear springs of the resident physics table's joints (PMX spring_position; off by default; include/reze_deform.h states the
        stage): a joint with play along an axis and a spring on it swings about its rest point. The table must have been uploaded with
        spring_position. A new table, skeleton or topology turns the springs off again. Does not reset the simulation."""
        if not hasattr(self._L, "rz_physics_springs"):
            raise RzError(-6, "this build of the library has no rz_physics_springs")
        self._chk(self._L.rz_physics_springs(self._h, 1 if on else 0))

    def physics_aligned(self, on=True):
        """PMX type-2 bodies ("physics + bone position alignment") of the resident table are simulated (off by default: they follow their
        bones; include/reze_deform.h states the rules): such a body with a mass and a bone swings like a dynamic one, is put back onto its
        bone at the start of every physics_step call, and its bone takes the body's rotation and keeps its own animated position. Rebuilds
        what the upload derived, so like a new upload it turns contacts and linear springs off and resets the simulation: call it right
        behind upload_physics, ahead of physics_springs and physics_contacts. A new table, skeleton or topology turns it off."""
        if not hasattr(self._L, "rz_physics_aligned"):
            raise RzError(-6, "this build of the library has no rz_physics_aligned")
        self._chk(self._L.rz_physics_aligned(self._h, 1 if on else 0))

    def read_physics(self, instance=0):
        """[n_bodies, 13] x3 q4 v3 w3 of one instance (blocking)."""
        out = np.empty((self.get_tuning("physics_bodies"), 13), dtype=np.float32)
        self._chk(self._L.rz_read_physics(self._h, int(instance), _fptr(out)))
        return out

    def read_hull(self, instance=0, v0=0, n=None):
        n = self.V - v0 if n is None else n
        out = np.empty((n, 3), dtype=np.float32)
        self._chk(self._L.rz_read_hull(self._h, int(instance), int(v0), int(n), _fptr(out)))
        return out

    def enable_aabb(self, on=True):
        self._chk(self._L.rz_enable_aabb(self._h, 1 if on else 0))

    def read_aabb(self, instance=0):
        out = np.empty(6, dtype=np.float32)
        self._chk(self._L.rz_read_aabb(self._h, int(instance), _fptr(out)))
        return out

    def frame_call(self, kind, primary, morph_weights=None, translations=None):
        """A zero-argument callable that does ONE per-frame upload + rz_deform through the raw C ABI with every array
        converted and every pointer built up front — for timing per-frame loops without numpy conversions in them
        (bench.py, tools/live_loop.py). kind: 'world' (rz_set_pose), 'local' (rz_set_pose_local), 'sampled'
        (rz_set_pose_sampled; `primary` = a [T, I] table of frame numbers that is cycled through), 'blended' (rz_set_pose_blended; a [T, I]
        table of motion states), 'layered' (rz_set_pose_layered; a pair of tables, states [T, I] and layers [T, I, n_layers]). Returns
        (call, check)."""
        L, h = self._L, self._h
        keep = []

        def ptr(a):
            if a is None:
                return None
            a = _f32(a).reshape(-1)
            keep.append(a)
            return _fptr(a)
        bad = []
        if kind == "world":
            wp, mp = ptr(primary), ptr(morph_weights if self.M > 0 else None)

            def call():
                if L.rz_set_pose(h, wp, mp) or L.rz_deform(h):
                    bad.append(1)
        elif kind == "local":
            qp, tp, mp = ptr(primary), ptr(translations), ptr(morph_weights if self.M > 0 else None)

            def call():
                if L.rz_set_pose_local(h, qp, tp, mp) or L.rz_deform(h):
                    bad.append(1)
        elif kind == "blended":
            # `primary` = a [T, I] table of MOTION_STATE_DTYPE records (pack_motion_states) that is cycled through
            rows = [np.ascontiguousarray(row, dtype=MOTION_STATE_DTYPE).reshape(-1) for row in np.atleast_2d(primary)]
            keep.extend(rows)
            table = [row.ctypes.data_as(ctypes.POINTER(RzMotionState)) for row in rows]
            tick = [0]

            def call():
                tick[0] += 1
                if L.rz_set_pose_blended(h, table[tick[0] % len(table)]) or L.rz_deform(h):
                    bad.append(1)
        elif kind == "layered":
            # `primary` = (a [T, I] table of MOTION_STATE_DTYPE records, a [T, I, n_layers] table of MOTION_LAYER_DTYPE records), cycled through
            srows = [np.ascontiguousarray(row, dtype=MOTION_STATE_DTYPE).reshape(-1) for row in np.atleast_2d(primary[0])]
            lrows = [np.ascontiguousarray(row, dtype=MOTION_LAYER_DTYPE).reshape(self.I, -1) for row in primary[1]]
            keep.extend(srows + lrows)
            n_layers = lrows[0].shape[1]
            table = [(s.ctypes.data_as(ctypes.POINTER(RzMotionState)), l.ctypes.data_as(ctypes.POINTER(RzMotionLayer)) if n_layers else None)
                     for s, l in zip(srows, lrows)]
            tick = [0]

            def call():
                tick[0] += 1
                sp, lp = table[tick[0] % len(table)]
                if L.rz_set_pose_layered(h, sp, n_layers, lp) or L.rz_deform(h):
                    bad.append(1)
        else:
            table = [ptr(row) for row in np.atleast_2d(primary)]
            tick = [0]

            def call():
                tick[0] += 1
                if L.rz_set_pose_sampled(h, table[tick[0] % len(table)]) or L.rz_deform(h):
                    bad.append(1)

        def check():
            if bad:
                raise RzError(-1, "a frame call failed: " + L.rz_last_error().decode("utf-8", "replace"))
        call.keep = keep
        return call, check

    def map_pose(self, layout=POSE_WORLD16):
        """rz_map_pose: (matrices, morph_weights) as numpy views OVER the pinned ring slot the next pose upload would have copied into —
        [I, B, 16] or (POSE_ROWS12) [I, B, 12] floats, and [I, M] floats or None. Write them in place, then commit_pose(). The views
        die with the commit (or the next pose call)."""
        mp, wp = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_float)()
        self._chk(self._L.rz_map_pose(self._h, int(layout), ctypes.byref(mp), ctypes.byref(wp)))
        per = 12 if layout == POSE_ROWS12 else 16
        mats = np.ctypeslib.as_array(mp, shape=(self.I, self.B, per))
        mw = np.ctypeslib.as_array(wp, shape=(self.I, self.M)) if (self.M > 0 and wp) else None
        return mats, mw

    def commit_pose(self):
        self._chk(self._L.rz_commit_pose(self._h))

    def mapped_frame_call(self, layout, fill=None):
        """Like frame_call, for caller-written poses: ONE rz_map_pose + fill(matrix pointer as int, bytes) + rz_commit_pose + rz_deform
        through the raw C ABI. `fill` stands in for the caller's pose solve writing its matrices in place (None: nothing is written — the
        protocol's own cost). Returns (call, check)."""
        L, h = self._L, self._h
        mp, wp = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_float)()
        mref, wref = ctypes.byref(mp), ctypes.byref(wp)
        nbytes = self.I * self.B * (48 if layout == POSE_ROWS12 else 64)
        bad = []

        def call():
            if L.rz_map_pose(h, layout, mref, wref):
                bad.append(1)
                return
            if fill is not None:
                fill(ctypes.cast(mp, ctypes.c_void_p).value, nbytes)
            if L.rz_commit_pose(h) or L.rz_deform(h):
                bad.append(1)

        def check():
            if bad:
                raise RzError(-1, "a mapped frame call failed: " + L.rz_last_error().decode("utf-8", "replace"))
        return call, check

    def time_span(self, frames, other=None, lead=0):
        """rz_time_span: ms between two events on the stream around `frames` back-to-back frames (with `other`, a fork: alternating),
        `lead` untimed frames in front of the opening event."""
        ms = ctypes.c_double(0.0)
        self._chk(self._L.rz_time_span(self._h, other._h if other is not None else None, int(lead), int(frames), ctypes.byref(ms)))
        return ms.value

    def deform(self):
        self._chk(self._L.rz_deform(self._h))

    def deform_n(self, frames):
        self._chk(self._L.rz_deform_n(self._h, int(frames)))

    def sync(self):
        self._chk(self._L.rz_sync(self._h))

    def read(self, instance=0, v0=0, n=None):
        n = self.V - v0 if n is None else n
        pos = np.empty((n, 3), dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32)
        self._chk(self._L.rz_read(self._h, int(instance), int(v0), int(n), _fptr(pos), _fptr(nrm)))
        return pos, nrm

    def read_palette(self, instance=0):
        out = np.empty((self.B, 12), dtype=np.float32)
        self._chk(self._L.rz_read_palette(self._h, int(instance), _fptr(out)))
        return out

    def autotune(self, frames=0):
        """Setup-time search over launch shapes with the current mesh / morphs / pose (rz_autotune)."""
        self._chk(self._L.rz_autotune(self._h, int(frames)))
        return {k: self.get_tuning(k) for k in ("effective_split", "effective_grid", "effective_inst_group")}

    _TUNE_FIELDS = ("morph_split", "grid_cap", "inst_loop", "eff_split", "eff_grid", "eff_inst_group", "same_as", "ms", "ms_min", "ms_max")

    def autotune_measure(self, frames=0):
        """rz_autotune_measure: the candidate table (list of dicts; entry 0 = the heuristic plan), nothing adopted."""
        tab = (RzTuneEntry * 32)()
        n = ctypes.c_int(0)
        self._chk(self._L.rz_autotune_measure(self._h, int(frames), tab, 32, ctypes.byref(n)))
        return [{k: getattr(tab[i], k) for k in self._TUNE_FIELDS} for i in range(n.value)]

    def autotune_pick(self, table):
        """rz_autotune_pick on a (possibly rank-reduced) table: entry 0 unless something beats it by >= 2 % with its slowest round under entry 0's fastest."""
        tab = (RzTuneEntry * len(table))()
        for i, e in enumerate(table):
            for k in self._TUNE_FIELDS:
                setattr(tab[i], k, e[k])
        return int(self._L.rz_autotune_pick(tab, len(table)))

    def autotune_apply(self, entry):
        e = RzTuneEntry()
        for k in self._TUNE_FIELDS:
            setattr(e, k, entry[k])
        self._chk(self._L.rz_autotune_apply(self._h, ctypes.byref(e)))

    def comm_info(self):
        """{count, user_rank} as the RCCL communicator reports them (ncclCommCount / ncclCommUserRank)."""
        n, u = ctypes.c_int(0), ctypes.c_int(-1)
        self._chk(self._L.rz_comm_info(self._h, ctypes.byref(n), ctypes.byref(u)))
        return {"comm_count": n.value, "comm_user_rank": u.value}

    def kernel_name(self):
        """The dominant kernel the CURRENT plan launches: kernel_name_of() over the tuning keys it reads."""
        return kernel_name_of({k: self.get_tuning(k) for k in KERNEL_NAME_KEYS})

    def time_frames(self, frames):
        t = RzTiming()
        self._chk(self._L.rz_time_frames(self._h, int(frames), ctypes.byref(t)))
        return {k: getattr(t, k) for k, _ in RzTiming._fields_ if k != "reserved"}

    def set_tuning(self, **kw):
        for k, v in kw.items():
            self._chk(self._L.rz_set_tuning(self._h, k.encode(), int(v)))

    def get_tuning(self, key):
        v = ctypes.c_int(0)
        self._chk(self._L.rz_get_tuning(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def output_ptrs(self):
        p = ctypes.c_void_p()
        n = ctypes.c_void_p()
        vp = ctypes.c_uint32(0)
        self._chk(self._L.rz_output_ptrs(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(vp)))
        return p.value, n.value, vp.value

    # ---- multi-GPU ----
    def comm_init(self, nranks, rank, unique_id, v_total):
        assert len(unique_id) == 128
        self._chk(self._L.rz_comm_init(self._h, int(nranks), int(rank), unique_id, int(v_total)))
        self.v_total = int(v_total)

    def allgather(self, with_normals=False):
        self._chk(self._L.rz_allgather(self._h, 1 if with_normals else 0))

    def gather_fence(self):
        """Make this (root) context's stream wait for the frames the other contributors have enqueued."""
        self._chk(self._L.rz_gather_fence(self._h))

    def read_gathered(self, v0=0, n=None):
        n = self.v_total - v0 if n is None else n
        pos = np.empty((n, 3), dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32)
        self._chk(self._L.rz_read_gathered(self._h, int(v0), int(n), _fptr(pos), _fptr(nrm)))
        return pos, nrm
