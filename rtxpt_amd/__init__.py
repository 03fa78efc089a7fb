"""rtxpt_amd — host-side mirror of the reference's render-pass seam over the C-ABI of libmi355pt.so.

The product is the shared library (hand-written HIP for gfx950, built in-tree by `rtxpt_amd/csrc/Makefile`); this
package is the thin Python host binding used by the tests and bench.py: same call order as `Sample::Render`
(/root/reference/Rtxpt/Sample.cpp:1891-2313): load/set scene -> set camera/settings -> render(sample range) -> map radiance.

There is no CPU fallback: importing works anywhere, but creating a `PathTracer` without the built library or without
a HIP device raises.
"""
import ctypes
import os
import subprocess

import numpy as np

from . import scenes  # noqa: F401  (scene generators + data-contract dtypes)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355PT_LIB", os.path.join(_HERE, "libmi355pt.so"))   # MI355PT_LIB: developer A/B builds only
HOOKS_LIB_PATH = os.path.join(_HERE, "libmi355pt_testhooks.so")                  # the tests' build: + include/mi355pt_testhooks.h
_libs = {}

PT_OK = 0
PT_ERROR_INVALID_ARGUMENT, PT_ERROR_NO_DEVICE, PT_ERROR_HIP, PT_ERROR_IO, PT_ERROR_UNSUPPORTED, PT_ERROR_NOT_READY = 1, 2, 3, 4, 5, 6
PT_TEX_RGBA8_UNORM, PT_TEX_RGBA8_SRGB, PT_TEX_RGBA32F = 0, 1, 2
STATUS = {0: "PT_OK", 1: "PT_ERROR_INVALID_ARGUMENT", 2: "PT_ERROR_NO_DEVICE", 3: "PT_ERROR_HIP", 4: "PT_ERROR_IO", 5: "PT_ERROR_UNSUPPORTED", 6: "PT_ERROR_NOT_READY"}

# every symbol include/mi355pt.h declares
EXPORTS = [
    "pt_create", "pt_destroy", "pt_get_last_error", "pt_load_scene_gltf", "pt_gltf_animation_load", "pt_gltf_animation_instances", "pt_gltf_animation_positions", "pt_gltf_animation_normals", "pt_gltf_animation_skinning", "pt_gltf_animation_palette", "pt_set_skinning", "pt_animate_skinned", "pt_get_skinning_time", "pt_get_vertex_streams", "pt_animate_normals", "pt_gltf_animation_free", "pt_set_geometry", "pt_set_instances", "pt_set_materials",
    "pt_set_environment", "pt_set_environment_cube", "pt_image_read_dds_cube", "pt_set_environment_bake", "pt_set_environment_compression", "pt_set_procedural_sky", "pt_procedural_sky_default_params", "pt_procedural_sky_update", "pt_env_bake_lights", "pt_set_lights", "pt_set_light_importance_boost", "pt_set_local_light_sampling", "pt_get_light_feedback", "pt_set_neeat", "pt_texture_filtering_default_params", "pt_set_texture_filtering", "pt_set_view_projection", "pt_neeat_reset", "pt_get_neeat_tables", "pt_neeat_pack_feedback", "pt_neeat_unpack_feedback", "pt_bridge_camera", "pt_set_camera", "pt_default_settings", "pt_set_settings", "pt_animate",
    "pt_resize", "pt_render", "pt_reset_accumulation", "pt_map_radiance", "pt_unmap_radiance", "pt_shard_info", "pt_pack_shard",
    "pt_unpack_shard", "pt_device_radiance", "pt_trace_closest", "pt_trace_visibility", "pt_get_lights", "pt_get_env_cube", "pt_get_subinstances",
    "pt_get_scene_info", "pt_get_build_stats", "pt_get_bvh_info", "pt_set_counters",
    "pt_update_texture", "pt_get_texture_level", "pt_get_alpha_plane", "pt_get_texture_ingest_stats",
    "pt_default_tonemap", "pt_tonemap", "pt_image_read_float", "pt_image_free", "pt_image_read_dds", "pt_image_read_dds_memory", "pt_image_read_jpeg", "pt_scene_import_texture", "pt_write_png", "pt_write_bmp", "pt_set_fused_traversal", "pt_set_serial_kernels", "pt_set_tail_paths", "pt_animate_ranges", "pt_set_motion_history", "pt_set_previous_pose", "pt_realtime_frame", "pt_exchange_planes_host", "pt_neeat_update_begin", "pt_neeat_update_end", "pt_pack_stable_plane_guides", "pt_unpack_stable_plane_guides", "pt_stable_planes_shard_bytes", "pt_pack_stable_planes", "pt_unpack_stable_planes", "pt_gather_stable_planes", "pt_material_from_json", "pt_convert_light",
    "pt_tonemap_color_transform", "pt_scene_json_import", "pt_scene_import_free", "pt_scene_import_cameras", "pt_scene_import_lights",
    "pt_scene_import_directional_lights", "pt_scene_import_instances", "pt_scene_import_geometries", "pt_scene_import_materials", "pt_scene_import_vertices", "pt_set_scene_directional_lights", "pt_scene_import_apply", "pt_scene_import_settings", "pt_average_luminance",
    "pt_default_tone_mapping_parameters", "pt_tonemap_from_parameters", "pt_scene_import_tone_mapping",
    "pt_stable_planes_plane_stride", "pt_build_stable_planes", "pt_fill_stable_planes", "pt_denoise_spec_hit_t", "pt_stable_planes_merge", "pt_get_stable_planes",
    "pt_denoiser_default_params", "pt_denoiser_prepare_dlss_rr", "pt_denoiser_prepare_nrd", "pt_denoiser_merge_nrd", "pt_get_denoiser_inputs", "pt_denoiser_device_buffers",
    "pt_denoise_default_settings", "pt_denoise_plane", "pt_denoised_device_buffers", "pt_get_denoised", "pt_denoise_frame", "pt_denoise_pass_times",
    "pt_taa_default_params", "pt_taa_resolve", "pt_resolved_device_buffer", "pt_get_resolved", "pt_tonemap_resolved", "pt_taa_jitter",
    "pt_bloom_default_params", "pt_bloom_kernel", "pt_bloom", "pt_bloomed_device_buffer", "pt_get_bloomed", "pt_tonemap_bloomed", "pt_average_luminance_bloomed",
    "pt_taa_upscale_default_params", "pt_taa_upscale", "pt_upscaled_size", "pt_upscaled_device_buffer", "pt_get_upscaled", "pt_bloom_upscaled", "pt_get_upscaled_bloomed",
    "pt_tonemap_upscaled", "pt_average_luminance_upscaled", "pt_upscale_tex_lod_bias",
    "pt_adaptive_default_params", "pt_render_adaptive", "pt_get_adaptive_state", "pt_get_adaptive_active",
    "pt_accum_denoise_default_params", "pt_accum_denoise", "pt_accum_denoise_host_inputs", "pt_accum_denoised_device_buffer", "pt_get_accum_denoised",
    "pt_get_accum_denoise_state", "pt_tonemap_accum_denoised", "pt_average_luminance_accum_denoised", "pt_bloom_accum_denoised",
    "pt_comm_unique_id", "pt_comm_init", "pt_comm_destroy", "pt_gather", "pt_shard_layout", "pt_gather_host", "pt_neeat_exchange_host",
]
TEST_HOOK_EXPORTS = ["pt_probe", "pt_get_inert_terminal", "pt_get_bvh8", "pt_trace_route"]      # include/mi355pt_testhooks.h: libmi355pt_testhooks.so only


class PtError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s (%d): %s" % (STATUS.get(code, "?"), code, msg))
        self.code = code


class PtGeometryBuffers(ctypes.Structure):
    _fields_ = [("indices", ctypes.c_void_p), ("numIndices", ctypes.c_uint32), ("positions", ctypes.c_void_p), ("uvs", ctypes.c_void_p),
                ("normals", ctypes.c_void_p), ("tangents", ctypes.c_void_p), ("numVertices", ctypes.c_uint32)]


class PtTextureDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("format", ctypes.c_uint32), ("pixels", ctypes.c_void_p)]


class PtEnvMapSceneParams(ctypes.Structure):
    _fields_ = [("Transform", ctypes.c_float * 12), ("ColorMultiplier", ctypes.c_float * 3), ("Enabled", ctypes.c_float)]


class PtProceduralSkyConstants(ctypes.Structure):      # SampleProceduralSky.hlsli:18-46 (40 floats; as_array() gives them as numpy)
    _fields_ = [("StarIrradiance", ctypes.c_float * 3), ("StarAngularDiameter", ctypes.c_float), ("RayleightScatteringRGB", ctypes.c_float * 3), ("PlanetSurfaceRadius", ctypes.c_float),
                ("MieScatteringRGB", ctypes.c_float * 3), ("PlanetAtmosphereRadius", ctypes.c_float), ("MieHenyeyGreensteinG", ctypes.c_float), ("SqDistanceToHorizontalBoundary", ctypes.c_float),
                ("AtmosphereHeight", ctypes.c_float), ("reserved", ctypes.c_float),
                ("FinalRadianceMultiplier", ctypes.c_float * 3), ("_padding3", ctypes.c_float), ("SunDir", ctypes.c_float * 3), ("CloudsTime", ctypes.c_float),
                ("GroundAlbedo", ctypes.c_float * 3), ("SunAngularDiameter", ctypes.c_float), ("_padding0", ctypes.c_float), ("_padding1", ctypes.c_float), ("sun_solid_angle", ctypes.c_float),
                ("_padding2", ctypes.c_float), ("physical_sky_ground_radiance", ctypes.c_float * 3), ("cloud_density_offset", ctypes.c_float),
                ("sky_transmittance", ctypes.c_float), ("sky_phase_g", ctypes.c_float), ("sky_amb_phase_g", ctypes.c_float), ("sky_scattering", ctypes.c_float)]

    def as_array(self): return np.frombuffer(bytes(self), np.float32).copy()


class PtSkyTexture(ctypes.Structure):
    _fields_ = [("rgba", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("_pad", ctypes.c_uint32)]


class PtProceduralSkyTextures(ctypes.Structure):
    _fields_ = [("transmittance", PtSkyTexture), ("scattering", PtSkyTexture), ("irradiance", PtSkyTexture), ("clouds", PtSkyTexture)]


class PtProceduralSkyParams(ctypes.Structure):         # SampleProceduralSky.h:70-82
    _fields_ = [("colorTint", ctypes.c_float * 3), ("brightness", ctypes.c_float), ("sunBrightness", ctypes.c_float), ("cloudsMovementSpeed", ctypes.c_float), ("timeOfDayMovementSpeed", ctypes.c_float),
                ("sunTimeOfDayOffset", ctypes.c_float), ("sunEastWestRotation", ctypes.c_float), ("sunAngularDiameterDeg", ctypes.c_float), ("cloudDensityOffset", ctypes.c_float),
                ("cloudTransmittance", ctypes.c_float), ("cloudScattering", ctypes.c_float)]


class PtProceduralSkyState(ctypes.Structure):
    _fields_ = [("lastSceneTime", ctypes.c_double), ("timeOfDayL1", ctypes.c_float), ("timeOfDayL2", ctypes.c_float), ("lastConstants", PtProceduralSkyConstants)]


def _sky_textures(textures):
    """four float32 arrays, (h, w, 4) or (d, h, w, 4): transmittance, scattering, irradiance, clouds -> (PtProceduralSkyTextures, the arrays kept alive)"""
    keep, t = [], PtProceduralSkyTextures()
    for name, a in zip(("transmittance", "scattering", "irradiance", "clouds"), textures):
        a = np.ascontiguousarray(a, np.float32); assert a.shape[-1] == 4 and a.ndim in (3, 4)
        d = a.shape[0] if a.ndim == 4 else 1
        setattr(t, name, PtSkyTexture(a.ctypes.data, a.shape[-2], a.shape[-3], d, 0)); keep.append(a)
    return t, keep


def procedural_sky_default_params(lib=None):
    L = lib or load_library(); p = PtProceduralSkyParams(); L.pt_procedural_sky_default_params(ctypes.byref(p)); return p


def procedural_sky_update(state, scene_time, preset="==PROCEDURAL_SKY==", params=None, force_instant=False, lib=None):
    """SampleProceduralSky::Update: -> (PtProceduralSkyConstants, changed). `state`: a PtProceduralSkyState kept between calls (PtProceduralSkyState() to start)."""
    L = lib or load_library(); out = PtProceduralSkyConstants()
    L.pt_procedural_sky_update.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_char_p, ctypes.c_int32, ctypes.c_void_p]; L.pt_procedural_sky_update.restype = ctypes.c_int32
    r = L.pt_procedural_sky_update(ctypes.byref(state), ctypes.byref(params) if params is not None else None, float(scene_time), preset.encode() if preset is not None else None, 1 if force_instant else 0, ctypes.byref(out))
    if r < 0: raise RuntimeError("pt_procedural_sky_update failed: %s" % STATUS.get(-r, r))
    return out, bool(r)


class PtDeviceDesc(ctypes.Structure):
    _fields_ = [("deviceOrdinal", ctypes.c_int32), ("shardRank", ctypes.c_uint32), ("shardCount", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


PT_STF_FILTER_POINT, PT_STF_FILTER_LINEAR, PT_STF_FILTER_CUBIC, PT_STF_FILTER_GAUSSIAN = 0, 1, 2, 3


class PtTextureFiltering(ctypes.Structure):      # include/mi355pt.h
    _fields_ = [("enable", ctypes.c_uint32), ("filter", ctypes.c_uint32), ("magnification", ctypes.c_uint32), ("gaussianSigma", ctypes.c_float)]


def texture_filtering_default_params():
    """pt_texture_filtering_default_params: (enable, filter, magnification, gaussianSigma) = (0, LINEAR, 0, 0.3)."""
    p = PtTextureFiltering(); L = load_library()
    f = L.pt_texture_filtering_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(ctypes.byref(p))
    if r != PT_OK: raise PtError(r, "pt_texture_filtering_default_params")
    return p.enable, p.filter, p.magnification, p.gaussianSigma


class PtTextureIngestStats(ctypes.Structure):      # pt_get_texture_ingest_stats
    _fields_ = [("onDevice", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("stagingChunks", ctypes.c_uint32), ("_pad", ctypes.c_uint32),
                ("sourceBytes", ctypes.c_uint64), ("level0Texels", ctypes.c_uint64), ("poolTexels", ctypes.c_uint64), ("hostBytesHeld", ctypes.c_uint64),
                ("uploadMs", ctypes.c_double), ("level0Ms", ctypes.c_double), ("mipMs", ctypes.c_double), ("alphaMs", ctypes.c_double), ("totalMs", ctypes.c_double)]


class PtFrameStats(ctypes.Structure):
    _fields_ = [("extendRays", ctypes.c_uint64), ("shadowRays", ctypes.c_uint64), ("hits", ctypes.c_uint64),
                ("nodeVisitsExtend", ctypes.c_uint64), ("triTestsExtend", ctypes.c_uint64), ("nodeVisitsShadow", ctypes.c_uint64), ("triTestsShadow", ctypes.c_uint64),
                ("leafVisitsExtend", ctypes.c_uint64), ("waveItersExtend", ctypes.c_uint64), ("leafVisitsShadow", ctypes.c_uint64), ("waveItersShadow", ctypes.c_uint64),
                ("extendPhaseCycles", ctypes.c_uint64 * 4), ("leafBlocksExtend", ctypes.c_uint64), ("waveItersMaxExtend", ctypes.c_uint64), ("extendRayIterHist", ctypes.c_uint64 * 16), ("longRayCount", ctypes.c_uint32), ("_padLong", ctypes.c_uint32), ("longRays", (ctypes.c_float * 8) * 32), ("extendEvents", ctypes.c_uint64 * 8),
                ("gpuMilliseconds", ctypes.c_double), ("extendKernelMs", ctypes.c_double), ("shadeKernelMs", ctypes.c_double), ("shadowKernelMs", ctypes.c_double),
                ("extendLaunches", ctypes.c_uint32), ("iterations", ctypes.c_uint32), ("pathsTraced", ctypes.c_uint32), ("tailLaunches", ctypes.c_uint32)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if isinstance(getattr(self, n), ctypes.Array) else getattr(self, n)) for n, _ in self._fields_ if n != "_pad"}


def build_library(verbose=False):
    """Compile libmi355pt.so for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("libmi355pt.so build failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH




def _share_hip_runtime_with_torch():
    """One HIP runtime per process. PyTorch-ROCm ships its own libamdhip64.so; were libmi355pt.so loaded first it would bind /opt/rocm's copy, a later
    `import torch` would bring a second runtime into the process, and whichever of the two initialises second no longer finds the device (seen on the
    MI355X box: load_library(); import torch; torch.cuda.is_available(); pt_create -> PT_ERROR_NO_DEVICE). Loading torch's copy first — without importing
    torch — makes both resolve to it by SONAME, in either import order. Without torch installed, /opt/rocm's copy is used as linked."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def _share_rccl_with_torch():
    """One RCCL per process, for the same reason as the HIP runtime: libmi355pt.so binds RCCL at run time (dlopen, RTLD_NOLOAD first), so loading torch's
    copy before pt_comm_unique_id / pt_comm_init makes the library and torch.distributed use the same one whatever the import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


COMM_ID_BYTES = 128


def comm_unique_id():
    """pt_comm_unique_id: 128 bytes created on rank 0; hand them to the other ranks (torch.distributed broadcast, MPI, a file) and call PathTracer.comm_init everywhere."""
    _share_rccl_with_torch()
    L = load_library()
    buf = (ctypes.c_ubyte * COMM_ID_BYTES)()
    r = L.pt_comm_unique_id(buf)
    if r != 0:
        raise PtError(r, "pt_comm_unique_id")
    return bytes(buf)


def shard_layout(width, height, rank, world):
    """pt_shard_layout: packed pixel ids (x<<16|y) owned by `rank`, in pack order (host only)."""
    L = load_library()
    n = ctypes.c_uint32()
    r = L.pt_shard_layout(width, height, rank, world, None, 0, ctypes.byref(n))
    if r != 0:
        raise PtError(r, "pt_shard_layout")
    out = np.zeros(n.value, np.uint32)
    r = L.pt_shard_layout(width, height, rank, world, _p(out), n.value, None)
    if r != 0:
        raise PtError(r, "pt_shard_layout")
    return out


class PtTransport(ctypes.Structure):
    SEND = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32)
    RECV = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32)
    GROUP = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p)
    _fields_ = [("user", ctypes.c_void_p), ("send", SEND), ("recv", RECV), ("group_begin", GROUP), ("group_end", GROUP)]


def _transport(send, recv, group_begin=None, group_end=None):
    """A PtTransport over Python callables: send(ptr, nbytes, peer) / recv(ptr, nbytes, peer) take raw addresses; group_begin() / group_end() are optional (NULL when not
    given). Returns (the structure, what must stay alive for as long as it is used)."""
    def guarded(fn):
        def cb(user, *args):
            try:
                fn(*args); return 0
            except Exception:      # an exception must not unwind through the C frames
                import traceback; traceback.print_exc(); return 1
        return cb
    fns = (PtTransport.SEND(guarded(send)), PtTransport.RECV(guarded(recv)),
           PtTransport.GROUP(guarded(group_begin)) if group_begin else PtTransport.GROUP(), PtTransport.GROUP(guarded(group_end)) if group_end else PtTransport.GROUP())
    return PtTransport(None, *fns), fns


def gather_host(width, height, rank, world, rgba, send, recv, group_begin=None, group_end=None):
    """pt_gather_host: the library's gather protocol over host memory and the caller's point-to-point transport (_transport); rgba: (h, w, 4) float32, modified in place on rank 0."""
    L = load_library()
    assert rgba.dtype == np.float32 and rgba.flags["C_CONTIGUOUS"] and rgba.shape == (height, width, 4)
    t, _keep = _transport(send, recv, group_begin, group_end)
    r = L.pt_gather_host(width, height, rank, world, _p(rgba), ctypes.byref(t))
    if r != 0:
        raise PtError(r, "pt_gather_host")
    return rgba


def neeat_exchange_host(width, height, rank, world, total_weight, candidates, depth, send, recv, group_begin=None, group_end=None):
    """pt_neeat_exchange_host: all ranks end up with all ranks' feedback reservoirs and exported depth; (h, w) float32 / uint32 / float32 planes, modified in place; send / recv as in gather_host"""
    L = load_library()
    assert total_weight.dtype == np.float32 and candidates.dtype == np.uint32 and depth.dtype == np.float32 and total_weight.shape == candidates.shape == depth.shape == (height, width)
    t, _keep = _transport(send, recv, group_begin, group_end)
    r = L.pt_neeat_exchange_host(width, height, rank, world, _p(total_weight), _p(candidates), _p(depth), ctypes.byref(t))
    if r != 0:
        raise PtError(r, "pt_neeat_exchange_host")


def exchange_planes_host(width, height, rank, world, planes, send, recv, to_root=False, group_begin=None, group_end=None):
    """pt_exchange_planes_host: `planes` = C-contiguous arrays of shape (height, width[, ...]) — any bytes per pixel; all-to-all (every rank ends up with every rank's pixels) or,
    with to_root, towards rank 0 only; modified in place; send / recv as in gather_host"""
    L = load_library()
    for a in planes: assert a.flags["C_CONTIGUOUS"] and a.shape[0] == height and a.shape[1] == width
    bpp = np.array([a.nbytes // (width * height) for a in planes], np.uint32)
    ptrs = (ctypes.c_void_p * len(planes))(*[a.ctypes.data for a in planes])
    t, _keep = _transport(send, recv, group_begin, group_end)
    f = L.pt_exchange_planes_host; f.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(width, height, rank, world, ptrs, _p(bpp), len(planes), 1 if to_root else 0, ctypes.byref(t))
    if r != 0:
        raise PtError(r, "pt_exchange_planes_host")


def kernel_source_digest():
    """SHA-256 over the sources of the library (rtxpt_amd/csrc/*.h, *.hip and *.cpp, names and contents, in name order): what ties a rocprofv3 counter summary under
    profiles/ to the code a bench.py run executes (tools/profile_round.sh writes it, bench.py compares it before quoting `bound` / `traffic`). The binary itself is tied by
    library_digest()."""
    import glob, hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.cpp"))):
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()


def library_digest(test_hooks=False):
    """SHA-256 of the shared library file load_library() opens — the binary the numbers of a run come from (bench.py prints it, tools/profile_round.sh records it)."""
    import hashlib
    h = hashlib.sha256()
    with open(HOOKS_LIB_PATH if test_hooks else LIB_PATH, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""): h.update(blk)
    return h.hexdigest()


def load_library(test_hooks=False):
    """dlopen libmi355pt.so (test_hooks: libmi355pt_testhooks.so, the tests' build with include/mi355pt_testhooks.h's evaluation hooks). Raises if it has not been built:
    the product path never falls back to anything else."""
    if _libs.get(test_hooks) is None:
        path = HOOKS_LIB_PATH if test_hooks else LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError("%s is missing (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C rtxpt_amd/csrc`." % (os.path.basename(path), path))
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(path)
        L.pt_get_last_error.restype = ctypes.c_char_p
        L.pt_get_last_error.argtypes = [ctypes.c_void_p]
        _libs[test_hooks] = L
    return _libs[test_hooks]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


TONEMAP_DTYPE = np.dtype([("whiteScale", "<f4"), ("whiteMaxLuminance", "<f4"), ("toneMapOperator", "<u4"), ("clamped", "<u4"),
                          ("autoExposure", "<u4"), ("avgLuminance", "<f4"), ("autoExposureLumValueMin", "<f4"), ("autoExposureLumValueMax", "<f4"),
                          ("colorTransform", "<f4", (9,)), ("enabled", "<u4"), ("_pad0", "<u4"), ("_pad1", "<u4")])
assert TONEMAP_DTYPE.itemsize == 80
TONEMAP_OPERATORS = {"linear": 0, "reinhard": 1, "reinhard_modified": 2, "heji_hable_alu": 3, "hable_uc2": 4, "aces": 5}


def default_tonemap(exposure_compensation=0.0, film_speed=100.0, shutter=1.0, f_number=1.0, **kw):
    """pt_default_tonemap: ToneMappingParameters defaults + manual-exposure colour transform (ToneMappingPasses.h:36-53, .cpp:428-441). No device needed."""
    L = load_library()
    t = np.zeros((), dtype=TONEMAP_DTYPE)
    L.pt_default_tonemap.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    r = L.pt_default_tonemap(_p(t), exposure_compensation, film_speed, shutter, f_number)
    if r != 0:
        raise PtError(r, "pt_default_tonemap")
    for k, v in kw.items():
        t[k] = TONEMAP_OPERATORS[v] if (k == "toneMapOperator" and isinstance(v, str)) else v
    return t


TONE_MAPPING_PARAMETERS_DTYPE = np.dtype([("exposureMode", "<u4"), ("toneMapOperator", "<u4"), ("autoExposure", "<u4"), ("exposureCompensation", "<f4"), ("exposureValue", "<f4"),
                                          ("filmSpeed", "<f4"), ("fNumber", "<f4"), ("shutter", "<f4"), ("whiteBalance", "<u4"), ("whitePoint", "<f4"), ("whiteMaxLuminance", "<f4"),
                                          ("whiteScale", "<f4"), ("clamped", "<u4"), ("exposureValueMin", "<f4"), ("exposureValueMax", "<f4")])
assert TONE_MAPPING_PARAMETERS_DTYPE.itemsize == 60


def default_tone_mapping_parameters(**kw):
    """pt_default_tone_mapping_parameters: ToneMappingParameters{} (ToneMappingPasses.h:36-53) as a TONE_MAPPING_PARAMETERS_DTYPE record. No device needed."""
    L = load_library()
    u = np.zeros((), dtype=TONE_MAPPING_PARAMETERS_DTYPE)
    L.pt_default_tone_mapping_parameters.argtypes = [ctypes.c_void_p]
    r = L.pt_default_tone_mapping_parameters(_p(u))
    if r != 0:
        raise PtError(r, "pt_default_tone_mapping_parameters")
    for k, v in kw.items():
        u[k] = TONEMAP_OPERATORS[v] if (k == "toneMapOperator" and isinstance(v, str)) else v
    return u


def tonemap_from_parameters(ui, avg_luminance=1.0, enabled=True):
    """pt_tonemap_from_parameters: ToneMappingPass::PreRender + the constant fill of ::Render on a ToneMappingParameters block -> TONEMAP_DTYPE record."""
    L = load_library()
    t = np.zeros((), dtype=TONEMAP_DTYPE)
    L.pt_tonemap_from_parameters.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32, ctypes.c_void_p]
    r = L.pt_tonemap_from_parameters(_p(ui), avg_luminance, 1 if enabled else 0, _p(t))
    if r != 0:
        raise PtError(r, "pt_tonemap_from_parameters")
    return t


def tonemap_color_transform(params, white_balance=False, white_point=6500.0, exposure_compensation=0.0, film_speed=100.0, shutter=1.0, f_number=1.0):
    """pt_tonemap_color_transform: UpdateWhiteBalanceTransform + UpdateColorTransform (ToneMappingPasses.cpp:392-441, ColorUtils.h:128-197) written into
    params["colorTransform"] (a TONEMAP_DTYPE record, modified in place and returned). No device needed."""
    L = load_library()
    L.pt_tonemap_color_transform.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_float] * 5
    r = L.pt_tonemap_color_transform(_p(params), 1 if white_balance else 0, white_point, exposure_compensation, film_speed, shutter, f_number)
    if r != 0:
        raise PtError(r, "pt_tonemap_color_transform")
    return params


class PtMaterialJsonInfo(ctypes.Structure):
    _fields_ = [("texturePath", (ctypes.c_char * 256) * 5), ("textureSRGB", ctypes.c_uint32 * 5), ("textureNormalMap", ctypes.c_uint32 * 5),
                ("enableAlphaTesting", ctypes.c_uint32), ("excludeFromNEE", ctypes.c_uint32), ("skipRender", ctypes.c_uint32), ("useDonutEmissiveIntensity", ctypes.c_uint32)]


def material_from_json(text, texture_words=(0xFFFFFFFF,) * 5):
    """pt_material_from_json: an RTXPT `.material.json` document -> (PTMaterialData record as numpy scalar, info dict). No device needed.
    texture_words: packed texture words of the Base / ORM / Normal / Emissive / Transmission textures (0xFFFFFFFF = not loaded)."""
    from . import scenes
    L = load_library()
    out = np.zeros((), dtype=scenes.MATERIAL_DTYPE)
    info = PtMaterialJsonInfo()
    words = (ctypes.c_uint32 * 5)(*[int(w) & 0xFFFFFFFF for w in texture_words])
    L.pt_material_from_json.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    r = L.pt_material_from_json(text.encode() if isinstance(text, str) else text, words, _p(out), ctypes.byref(info))
    if r != 0:
        raise PtError(r, "pt_material_from_json")
    return out, {"texturePath": [bytes(info.texturePath[i]).split(b"\0")[0].decode() for i in range(5)], "textureSRGB": list(info.textureSRGB),
                 "textureNormalMap": list(info.textureNormalMap), "enableAlphaTesting": bool(info.enableAlphaTesting), "excludeFromNEE": bool(info.excludeFromNEE),
                 "skipRender": bool(info.skipRender), "useDonutEmissiveIntensity": bool(info.useDonutEmissiveIntensity)}


class PtAnalyticLightDesc(ctypes.Structure):
    _fields_ = [("type", ctypes.c_uint32), ("position", ctypes.c_float * 3), ("direction", ctypes.c_float * 3), ("color", ctypes.c_float * 3), ("intensity", ctypes.c_float),
                ("radius", ctypes.c_float), ("innerAngle", ctypes.c_float), ("outerAngle", ctypes.c_float)]


class PtSkinRange(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("firstVertex", "numVertices", "firstMatrix", "numMatrices", "firstMorphDelta", "numTargets", "firstWeight", "geometryFlags")]


class PtSkinningDesc(ctypes.Structure):
    _fields_ = [("numVertices", ctypes.c_uint32), ("numRanges", ctypes.c_uint32), ("numMatrices", ctypes.c_uint32), ("numMorphWeights", ctypes.c_uint32),
                ("joints", ctypes.c_void_p), ("weights", ctypes.c_void_p), ("normals", ctypes.c_void_p), ("tangents", ctypes.c_void_p),
                ("morphPositionDeltas", ctypes.c_void_p), ("morphNormalDeltas", ctypes.c_void_p), ("morphTangentDeltas", ctypes.c_void_p), ("numMorphDeltaFloats", ctypes.c_uint64),
                ("ranges", ctypes.c_void_p)]


SKIN_RANGE_DTYPE = np.dtype([(k, np.uint32) for k in ("firstVertex", "numVertices", "firstMatrix", "numMatrices", "firstMorphDelta", "numTargets", "firstWeight", "geometryFlags")])


class SkinningDesc:
    """PtSkinningDesc as numpy arrays (PathTracer.set_skinning's argument): joints uint16 [V, 4], weights float32 [V, 4], normals float32 [V, 3], tangents float32 [V, 4]
    (bind pose, per vertex of the whole stream), morph_position / _normal / _tangent_deltas float32 [D], ranges SKIN_RANGE_DTYPE [R], num_matrices, num_morph_weights."""
    def __init__(self, joints, weights, normals, tangents, ranges, num_matrices, num_morph_weights=0, morph_position_deltas=None, morph_normal_deltas=None, morph_tangent_deltas=None):
        z = np.zeros(0, np.float32)
        self.joints = np.ascontiguousarray(joints, np.uint16).reshape(-1, 4); self.weights = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3); self.tangents = np.ascontiguousarray(tangents, np.float32).reshape(-1, 4)
        self.morph_position_deltas = np.ascontiguousarray(z if morph_position_deltas is None else morph_position_deltas, np.float32).reshape(-1)
        self.morph_normal_deltas = np.ascontiguousarray(np.zeros_like(self.morph_position_deltas) if morph_normal_deltas is None else morph_normal_deltas, np.float32).reshape(-1)
        self.morph_tangent_deltas = np.ascontiguousarray(np.zeros_like(self.morph_position_deltas) if morph_tangent_deltas is None else morph_tangent_deltas, np.float32).reshape(-1)
        self.ranges = np.ascontiguousarray(ranges, SKIN_RANGE_DTYPE).reshape(-1); self.num_matrices = int(num_matrices); self.num_morph_weights = int(num_morph_weights)

    def struct(self):
        """the ctypes PtSkinningDesc over these arrays (which must outlive it)"""
        assert len(self.weights) == len(self.joints) == len(self.normals) == len(self.tangents) and len(self.morph_normal_deltas) == len(self.morph_tangent_deltas) == len(self.morph_position_deltas)
        d = PtSkinningDesc(len(self.joints), len(self.ranges), self.num_matrices, self.num_morph_weights)
        d.joints, d.weights, d.normals, d.tangents = (a.ctypes.data for a in (self.joints, self.weights, self.normals, self.tangents))
        d.morphPositionDeltas, d.morphNormalDeltas, d.morphTangentDeltas = (a.ctypes.data for a in (self.morph_position_deltas, self.morph_normal_deltas, self.morph_tangent_deltas))
        d.numMorphDeltaFloats = len(self.morph_position_deltas); d.ranges = self.ranges.ctypes.data
        return d


class GltfAnimation:
    """pt_gltf_animation_*: the animations of a .gltf / .glb file, evaluated on the host into the instance transforms pt_animate takes."""
    def __init__(self, path):
        self.L = load_library(); self.h = ctypes.c_void_p(); n = ctypes.c_uint32(); d = ctypes.c_float()
        self.L.pt_gltf_animation_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)]
        self.L.pt_gltf_animation_instances.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32]
        self.L.pt_gltf_animation_free.argtypes = [ctypes.c_void_p]; self.L.pt_gltf_animation_free.restype = None
        r = self.L.pt_gltf_animation_load(str(path).encode(), ctypes.byref(self.h), ctypes.byref(n), ctypes.byref(d))
        if r != PT_OK: raise PtError(r, "pt_gltf_animation_load(%s)" % path)
        self.count, self.duration = n.value, d.value

    def instances(self, t, animation=0):
        """INSTANCE_DTYPE array of the scene's instances at time t [s]"""
        from . import scenes
        n = self.L.pt_gltf_animation_instances(self.h, animation, float(t), None, 0)
        if n < 0: raise PtError(-n, "pt_gltf_animation_instances")
        out = np.zeros(n, scenes.INSTANCE_DTYPE)
        if n: assert self.L.pt_gltf_animation_instances(self.h, animation, float(t), _p(out), n) == n
        return out

    def positions(self, t, animation=0):
        """pt_gltf_animation_positions: float32 [vertices, 3], the file's vertex stream with every skinned primitive posed at time t [s] (pt_animate's `positions`)."""
        self.L.pt_gltf_animation_positions.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32]
        n = self.L.pt_gltf_animation_positions(self.h, animation, float(t), None, 0)
        if n < 0: raise PtError(-n, "pt_gltf_animation_positions")
        out = np.zeros((n, 3), np.float32)
        if n: assert self.L.pt_gltf_animation_positions(self.h, animation, float(t), _p(out), n) == n
        return out

    def normals(self, t, animation=0):
        """pt_gltf_animation_normals: (normals, tangents) uint32 [vertices], the posed NORMAL / TANGENT streams in pt_set_geometry's SNORM8 packing (pt_animate_normals' arguments)."""
        f = self.L.pt_gltf_animation_normals; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        n = f(self.h, animation, float(t), None, None, 0)
        if n < 0: raise PtError(-n, "pt_gltf_animation_normals")
        nrm, tan = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        if n: assert f(self.h, animation, float(t), _p(nrm), _p(tan), n) == n
        return nrm, tan

    def skinning(self):
        """pt_gltf_animation_skinning: the file's static skinning data as a SkinningDesc (copies; PathTracer.set_skinning's argument)"""
        f = self.L.pt_gltf_animation_skinning; f.argtypes = [ctypes.c_void_p, ctypes.POINTER(PtSkinningDesc)]; f.restype = ctypes.c_int32
        d = PtSkinningDesc(); r = f(self.h, ctypes.byref(d))
        if r != PT_OK: raise PtError(r, "pt_gltf_animation_skinning")
        def arr(ptr, dtype, count): return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (count,)).copy() if ptr and count else np.zeros(0, dtype)
        nv, nd = d.numVertices, d.numMorphDeltaFloats
        ranges = np.frombuffer(ctypes.string_at(d.ranges, d.numRanges * SKIN_RANGE_DTYPE.itemsize), SKIN_RANGE_DTYPE).copy() if d.numRanges else np.zeros(0, SKIN_RANGE_DTYPE)
        return SkinningDesc(arr(d.joints, np.uint16, 4 * nv), arr(d.weights, np.float32, 4 * nv), arr(d.normals, np.float32, 3 * nv), arr(d.tangents, np.float32, 4 * nv), ranges, d.numMatrices, d.numMorphWeights,
                            arr(d.morphPositionDeltas, np.float32, nd), arr(d.morphNormalDeltas, np.float32, nd), arr(d.morphTangentDeltas, np.float32, nd))

    def palette(self, t, animation=0):
        """pt_gltf_animation_palette: (matrices float64 [M, 16] column major, morph weights float64 [W]) at time t [s] — pt_animate_skinned's per-frame arguments"""
        f = self.L.pt_gltf_animation_palette; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]; f.restype = ctypes.c_int32
        n = f(self.h, animation, float(t), None, 0, None, 0)
        if n < 0: raise PtError(-n, "pt_gltf_animation_palette")
        if not hasattr(self, "_numMorphWeights"): self._numMorphWeights = self.skinning().num_morph_weights
        m = np.zeros((n, 16), np.float64); w = np.zeros(self._numMorphWeights, np.float64)
        if n or len(w):
            r = f(self.h, animation, float(t), _p(m), n, _p(w), len(w))
            if r < 0: raise PtError(-r, "pt_gltf_animation_palette")
        return m, w

    def close(self):
        if self.h: self.L.pt_gltf_animation_free(self.h); self.h = ctypes.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def read_dds(path):
    """pt_image_read_dds: the top mip level of a 2D .dds file. Returns (pixels, format): uint8 [h, w, 4] with PT_TEX_RGBA8_UNORM / PT_TEX_RGBA8_SRGB, or
    float32 [h, w, 4] with PT_TEX_RGBA32F. No device needed."""
    L = load_library()
    w, h, fmt = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(); p = ctypes.c_void_p()
    L.pt_image_read_dds.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_void_p)]
    L.pt_image_free.argtypes = [ctypes.c_void_p]; L.pt_image_free.restype = None
    r = L.pt_image_read_dds(str(path).encode(), ctypes.byref(w), ctypes.byref(h), ctypes.byref(fmt), ctypes.byref(p))
    if r != PT_OK: raise PtError(r, "pt_image_read_dds(%s)" % path)
    try:
        ct, dt = (ctypes.c_float, np.float32) if fmt.value == 2 else (ctypes.c_uint8, np.uint8)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape=(h.value, w.value, 4)).astype(dt, copy=True), int(fmt.value)
    finally:
        L.pt_image_free(p)


def read_dds_cube(path):
    """pt_image_read_dds_cube: the six faces (top level) of a float / BC6H cube-map .dds as float32 [6, dim, dim, 4] in D3D's face order — an environment source for
    the scene key "env_cube_source" (pt_set_environment_cube). No device needed."""
    L = load_library()
    dim = ctypes.c_uint32(); p = ctypes.c_void_p()
    L.pt_image_read_dds_cube.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_void_p)]
    L.pt_image_free.argtypes = [ctypes.c_void_p]; L.pt_image_free.restype = None
    r = L.pt_image_read_dds_cube(str(path).encode(), ctypes.byref(dim), ctypes.byref(p))
    if r != PT_OK: raise PtError(r, "pt_image_read_dds_cube(%s)" % path)
    try:
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(6, dim.value, dim.value, 4)).astype(np.float32, copy=True)
    finally:
        L.pt_image_free(p)


def read_jpeg(data):
    """pt_image_read_jpeg: a JPEG stream (bytes, or a path) as uint8 [h, w, 4]. No device needed."""
    if not isinstance(data, (bytes, bytearray)): data = open(data, "rb").read()
    L = load_library(); w, h = ctypes.c_uint32(), ctypes.c_uint32(); p = ctypes.c_void_p()
    L.pt_image_read_jpeg.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_void_p)]
    L.pt_image_free.argtypes = [ctypes.c_void_p]; L.pt_image_free.restype = None
    r = L.pt_image_read_jpeg(bytes(data), len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(p))
    if r != PT_OK: raise PtError(r, "pt_image_read_jpeg")
    try:
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(h.value, w.value, 4)).copy()
    finally:
        L.pt_image_free(p)


def read_float_image(path):
    """pt_image_read_float: an OpenEXR (scan-line; none / RLE / ZIPS / ZIP) or Radiance .hdr file as float32 [h, w, 3], top row first. No device needed."""
    L = load_library()
    w, h = ctypes.c_uint32(), ctypes.c_uint32(); p = ctypes.POINTER(ctypes.c_float)()
    L.pt_image_read_float.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    L.pt_image_free.argtypes = [ctypes.c_void_p]; L.pt_image_free.restype = None
    r = L.pt_image_read_float(str(path).encode(), ctypes.byref(w), ctypes.byref(h), ctypes.byref(p))
    if r != PT_OK: raise PtError(r, "pt_image_read_float(%s)" % path)
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        L.pt_image_free(p)


def env_bake_lights(world_lights, cube_dim, transform=None):
    """pt_env_bake_lights (Sample::UpdateLighting): world-space rows of EMB_DirectionalLight -> the rows pt_set_environment_bake takes (angular size raised to
    what the cube resolves, direction in the environment's local frame). transform: the 12 floats of EnvMapSceneParams.Transform or None. No device needed."""
    L = load_library()
    a = np.ascontiguousarray(world_lights, np.float32).reshape(-1, 8); out = np.zeros_like(a)
    p = None
    if transform is not None:
        p = PtEnvMapSceneParams((ctypes.c_float * 12)(*np.asarray(transform, np.float32).tolist()), (ctypes.c_float * 3)(1.0, 1.0, 1.0), 1.0)
    r = L.pt_env_bake_lights(_p(a) if len(a) else None, len(a), ctypes.byref(p) if p is not None else None, int(cube_dim), _p(out) if len(a) else None)
    if r != PT_OK: raise PtError(r, "pt_env_bake_lights")
    return out


def convert_light(kind, position, color, intensity, radius, direction=(0.0, -1.0, 0.0), inner_angle=0.0, outer_angle=0.0):
    """pt_convert_light (LightsBaker::ConvertLight): kind "point" / "spot" -> (8 words PolymorphicLightInfo, 4 words PolymorphicLightInfoEx) as uint32 arrays. No device needed."""
    L = load_library()
    d = PtAnalyticLightDesc(); d.type = {"point": 0, "spot": 1}[kind]
    d.position[:] = [float(x) for x in position]; d.direction[:] = [float(x) for x in direction]; d.color[:] = [float(x) for x in color]
    d.intensity, d.radius, d.innerAngle, d.outerAngle = float(intensity), float(radius), float(inner_angle), float(outer_angle)
    base = np.zeros(8, np.uint32); ex = np.zeros(4, np.uint32)
    L.pt_convert_light.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    r = L.pt_convert_light(ctypes.byref(d), _p(base), _p(ex))
    if r != 0:
        raise PtError(r, "pt_convert_light")
    return base, ex


SCENE_CAMERA_DTYPE = np.dtype([("position", "<f4", 3), ("direction", "<f4", 3), ("up", "<f4", 3), ("verticalFov", "<f4"), ("zNear", "<f4"), ("exposureMask", "<u4"),
                               ("enableAutoExposure", "<u4"), ("exposureCompensation", "<f4"), ("exposureValue", "<f4"), ("exposureValueMin", "<f4"),
                               ("exposureValueMax", "<f4"), ("name", "S64")])
SCENE_JSON_INFO_DTYPE = np.dtype([("numModels", "<u4"), ("numGeometries", "<u4"), ("numMeshes", "<u4"), ("numInstances", "<u4"), ("numMaterials", "<u4"), ("numTextures", "<u4"),
                                  ("numLights", "<u4"), ("numCameras", "<u4"), ("materialOverrides", "<u4"), ("texturesNotLoaded", "<u4"), ("lightsDropped", "<u4"),
                                  ("lightProxies", "<u4"), ("skippedGeometries", "<u4"), ("directionalLights", "<u4"), ("hasEnvironment", "<u4"),
                                  ("envRadianceScale", "<f4", 3), ("envRotation", "<f4"), ("envTextureIndex", "<i4"), ("envPath", "S260"), ("settingsMask", "<u4"),
                                  ("realtimeMode", "<u4"), ("enableAnimations", "<u4"), ("startingCamera", "<i4"), ("realtimeFireflyFilter", "<f4"), ("maxBounces", "<i4"),
                                  ("maxDiffuseBounces", "<i4"), ("textureMIPBias", "<f4"), ("selectedCamera", "<i4"), ("lightProxiesResolved", "<u4")])
assert SCENE_CAMERA_DTYPE.itemsize == 132 and SCENE_JSON_INFO_DTYPE.itemsize == 380


class SceneImport:
    """pt_scene_json_import: an RTXPT `.scene.json` asset folder read on the host (ExtendedScene + Sample::SceneLoaded + MaterialsBaker::Load). No device
    needed; PathTracer.apply_scene_import hands it to a context."""

    def __init__(self, scene_path, media_path=None):
        from . import scenes
        self.L = load_library()
        self.h = ctypes.c_void_p()
        self.info = np.zeros((), dtype=SCENE_JSON_INFO_DTYPE)
        self.L.pt_scene_json_import.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
        r = self.L.pt_scene_json_import(str(scene_path).encode(), None if media_path is None else str(media_path).encode(), ctypes.byref(self.h), _p(self.info))
        if r != 0:
            raise PtError(r, "pt_scene_json_import")
        self.L.pt_scene_import_free.argtypes = [ctypes.c_void_p]; self.L.pt_scene_import_free.restype = None

        def fetch(fn, dtype, n):
            a = np.zeros(max(int(n), 1), dtype=dtype)
            f = getattr(self.L, fn); f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
            got = f(self.h, _p(a), int(n))
            assert got == n, (fn, got, n)
            return a[:n]
        I = self.info
        self.cameras = fetch("pt_scene_import_cameras", SCENE_CAMERA_DTYPE, I["numCameras"])
        self.instances = fetch("pt_scene_import_instances", scenes.INSTANCE_DTYPE, I["numInstances"])
        self.geometries = fetch("pt_scene_import_geometries", scenes.GEOMETRY_DTYPE, I["numGeometries"])
        self.materials = fetch("pt_scene_import_materials", scenes.MATERIAL_DTYPE, I["numMaterials"])
        self.L.pt_scene_import_vertices.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        nv = self.L.pt_scene_import_vertices(self.h, None, 0); self.positions = np.zeros((max(nv, 1), 3), np.float32)
        assert self.L.pt_scene_import_vertices(self.h, _p(self.positions), nv) == nv
        self.positions = self.positions[:nv]
        n = int(I["numLights"]); self.lights = np.zeros((max(n, 1), 8), np.uint32); self.lights_ex = np.zeros((max(n, 1), 4), np.uint32)
        self.L.pt_scene_import_lights.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        assert self.L.pt_scene_import_lights(self.h, _p(self.lights), _p(self.lights_ex), n) == n
        self.lights, self.lights_ex = self.lights[:n], self.lights_ex[:n]
        self.L.pt_scene_import_directional_lights.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        nd = self.L.pt_scene_import_directional_lights(self.h, None, 0)
        self.directional_lights = np.zeros((max(nd, 1), 8), np.float32)      # rows of EMB_DirectionalLight in world space: colour rgb, irradiance, direction xyz, angular size [rad]
        assert self.L.pt_scene_import_directional_lights(self.h, _p(self.directional_lights), nd) == nd
        self.directional_lights = self.directional_lights[:nd]

    def texture(self, index):
        """pt_scene_import_texture: the decoded top level of imported texture `index` as (uint8 [h, w, 4], format)."""
        d = PtTextureDesc()
        self.L.pt_scene_import_texture.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        r = self.L.pt_scene_import_texture(self.h, int(index), ctypes.byref(d))
        if r != 0: raise PtError(r, "pt_scene_import_texture(%d)" % index)
        return np.ctypeslib.as_array(ctypes.cast(d.pixels, ctypes.POINTER(ctypes.c_uint8)), shape=(d.height, d.width, 4)).copy(), int(d.format)

    def tone_mapping(self, ui=None, camera=-1):
        """pt_scene_import_tone_mapping: Sample::SceneLoaded's exposure defaults + Sample::UpdateCameraFromScene on a ToneMappingParameters record."""
        ui = default_tone_mapping_parameters() if ui is None else ui
        self.L.pt_scene_import_tone_mapping.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        r = self.L.pt_scene_import_tone_mapping(self.h, int(camera), _p(ui))
        if r != 0:
            raise PtError(r, "pt_scene_import_tone_mapping")
        return ui

    def apply_settings(self, settings):
        """pt_scene_import_settings: the scene's SampleSettings keys written over a SETTINGS_DTYPE record (in place)."""
        self.L.pt_scene_import_settings.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        r = self.L.pt_scene_import_settings(self.h, _p(settings))
        if r != 0:
            raise PtError(r, "pt_scene_import_settings")
        return settings

    def close(self):
        if self.h:
            self.L.pt_scene_import_free(self.h); self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_image(path, rgba8):
    """pt_write_png / pt_write_bmp by extension (the reference's screenshot formats). rgba8: (H, W, 4) uint8."""
    L = load_library()
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    fn = L.pt_write_bmp if path.lower().endswith(".bmp") else L.pt_write_png
    fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    r = fn(path.encode(), _p(a), a.shape[1], a.shape[0])
    if r != 0:
        raise PtError(r, "write_image " + path)


def bridge_camera(width, height, pos, direction, up, fov_y, near_z=0.01, far_z=1e5, focal_distance=10.0, aperture_radius=0.0, jitter=(0.0, 0.0)):
    """pt_bridge_camera: the library's BridgeCamera (PathTracerShared.h:109-141). Does not need a device."""
    L = load_library()
    cam = np.zeros((), dtype=scenes.CAMERA_DTYPE)
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    j = (ctypes.c_float * 2)(float(jitter[0]), float(jitter[1]))
    r = L.pt_bridge_camera(ctypes.c_uint32(width), ctypes.c_uint32(height), f3(pos), f3(direction), f3(up), ctypes.c_float(fov_y), ctypes.c_float(near_z),
                           ctypes.c_float(far_z), ctypes.c_float(focal_distance), ctypes.c_float(aperture_radius), j, _p(cam))
    if r != PT_OK:
        raise PtError(r, "pt_bridge_camera")
    return cam


# PtDenoiserParams (include/mi355pt.h): what the denoiser passes read of the frame's constants besides PtStablePlanesParams
DENOISER_PARAMS_DTYPE = np.dtype([("matWorldToView", "<f4", 16), ("preExposedGrayLuminance", "<f4"), ("denoiserRadianceClampK", "<f4"), ("DLSSRRBrightnessClampK", "<f4"),
                                  ("stablePlanesSuppressPrimaryIndirectSpecularK", "<f4")])
# PtDenoiserBuffers' members in order: (key, numpy dtype, values per pixel)
DENOISER_BUFFERS = (("rr_diffuse_albedo", np.uint32, 1), ("rr_specular_albedo", np.uint32, 1), ("rr_normal_roughness", np.uint16, 4), ("rr_specular_motion_vectors", np.uint16, 2),
                    ("nrd_view_z", np.float32, 1), ("nrd_motion_vectors", np.uint16, 4), ("nrd_normal_roughness", np.float32, 4), ("nrd_diff_radiance_hit_dist", np.float32, 4),
                    ("nrd_spec_radiance_hit_dist", np.float32, 4), ("nrd_roughness", np.float32, 1), ("nrd_disocclusion_threshold_mix", np.uint8, 1),
                    ("nrd_combined_history_clamp_relax", np.uint8, 1))


class PtDenoiserBuffers(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k, _, _ in DENOISER_BUFFERS] + [("pitch", ctypes.c_size_t * 12)]


def denoiser_default_params(lib=None):
    """pt_denoiser_default_params: identity view matrix, grey luminance 1, radiance clamp 8, DLSS-RR brightness clamp 4096, suppression 0.6"""
    L = lib or load_library()
    out = np.zeros((), DENOISER_PARAMS_DTYPE)
    f = L.pt_denoiser_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_denoiser_default_params")
    return out


# PtDenoiseSettings (include/mi355pt.h): the device denoiser's settings (pt_denoise_plane / pt_denoise_frame)
DENOISE_SETTINGS_DTYPE = np.dtype([("atrousIterationNum", "<u4"), ("depthThreshold", "<f4"), ("lobeAngleFraction", "<f4"), ("diffuseMaxAccumulatedFrameNum", "<u4"),
                                   ("specularMaxAccumulatedFrameNum", "<u4"), ("diffuseMaxFastAccumulatedFrameNum", "<u4"), ("specularMaxFastAccumulatedFrameNum", "<u4"),
                                   ("enableAntiFirefly", "<u4"), ("disocclusionThreshold", "<f4"), ("disocclusionThresholdAlternate", "<f4"), ("useDisocclusionThresholdMix", "<u4"),
                                   ("luminanceSigmaScale", "<f4")])


def denoise_default_settings(lib=None, **overrides):
    """pt_denoise_default_settings: the reference's RELAX defaults (NrdConfig.cpp:15-47, SampleUI.h:294-296), luminanceSigmaScale 4; keywords override fields"""
    L = lib or load_library()
    out = np.zeros((), DENOISE_SETTINGS_DTYPE)
    f = L.pt_denoise_default_settings; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_denoise_default_settings")
    for k, v in overrides.items(): out[k] = v
    return out


# PtTaaParams (include/mi355pt.h): the temporal anti-aliasing resolve's parameters (pt_taa_resolve)
TAA_PARAMS_DTYPE = np.dtype([("newFrameWeight", "<f4"), ("clampingFactor", "<f4"), ("maxRadiance", "<f4"), ("enableHistoryClamping", "<u4"), ("useHistoryClampRelax", "<u4"),
                             ("useCatmullRomFilter", "<u4"), ("luminanceWeighted", "<u4")])
TAA_JITTER_HALTON, TAA_JITTER_R2 = 1, 2      # the UI combo "MSAA\0Halton\0R2\0White Noise" (SampleUI.cpp:1126); 0 and 3 are refused


def taa_default_params(lib=None, **overrides):
    """pt_taa_default_params: new frame weight 0.1, clamping on (factor 1, relaxed by nrdCombinedHistoryClampRelax), Catmull-Rom history, luminance-weighted blend; keywords override"""
    L = lib or load_library()
    out = np.zeros((), TAA_PARAMS_DTYPE)
    f = L.pt_taa_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_taa_default_params")
    for k, v in overrides.items(): out[k] = v
    return out


def taa_jitter(sequence, frame_index, lib=None):
    """pt_taa_jitter: the sub-pixel camera offset (x, y) of a frame, in pixels in [-0.5, 0.5): sequence 1 Halton (2, 3), 2 R2. Does not need a device."""
    L = lib or load_library()
    out = (ctypes.c_float * 2)()
    f = L.pt_taa_jitter; f.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(int(sequence), int(frame_index), out)
    if r != PT_OK: raise PtError(r, "pt_taa_jitter")
    return np.float32(out[0]), np.float32(out[1])


# PtTaaUpscaleParams (include/mi355pt.h): the temporal upscaling resolve's parameters (pt_taa_upscale) — PtTaaParams, then the two fields of the resampling
TAA_UPSCALE_PARAMS_DTYPE = np.dtype(TAA_PARAMS_DTYPE.descr + [("kernelRadius", "<f4"), ("confidenceWeighted", "<u4")])


def taa_upscale_default_params(lib=None, **overrides):
    """pt_taa_upscale_default_params: taa_default_params()'s fields, kernelRadius 1, confidenceWeighted 1; keywords override"""
    L = lib or load_library()
    out = np.zeros((), TAA_UPSCALE_PARAMS_DTYPE)
    f = L.pt_taa_upscale_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_taa_upscale_default_params")
    for k, v in overrides.items(): out[k] = v
    return out


def upscale_tex_lod_bias(render_w, render_h, display_w, display_h, lib=None):
    """pt_upscale_tex_lod_bias: what a frame traced at the render size for a display of the display size adds to PtSettings.texLODBias (Sample.cpp:1504). Does not need a device."""
    L = lib or load_library()
    v = ctypes.c_float(0.0)
    f = L.pt_upscale_tex_lod_bias; f.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(int(render_w), int(render_h), int(display_w), int(display_h), ctypes.byref(v))
    if r != PT_OK: raise PtError(r, "pt_upscale_tex_lod_bias")
    return np.float32(v.value)


# PtBloomParams (include/mi355pt.h): the bloom pass's parameters (pt_bloom)
BLOOM_PARAMS_DTYPE = np.dtype([("radius", "<f4"), ("intensity", "<f4"), ("maxRadiance", "<f4"), ("enable", "<u4")])
BLOOM_SOURCE_RADIANCE, BLOOM_SOURCE_RESOLVED = 0, 1
BLOOM_MAX_TAPS = 48


def bloom_default_params(lib=None, **overrides):
    """pt_bloom_default_params: on, width 8 pixels, intensity 0.004 (SampleUI.h:305-307), maxRadiance 10000; keywords override"""
    L = lib or load_library()
    out = np.zeros((), BLOOM_PARAMS_DTYPE)
    f = L.pt_bloom_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_bloom_default_params")
    for k, v in overrides.items(): out[k] = v
    return out


def bloom_kernel(radius, lib=None, capacity=BLOOM_MAX_TAPS + 1):
    """pt_bloom_kernel: (the blur's taps g[0 .. R] as float32, their float sum G) for a radius in (0, 64]. Does not need a device."""
    L = lib or load_library()
    g = np.zeros(max(int(capacity), 1), np.float32); n, G = ctypes.c_uint32(), ctypes.c_float()
    f = L.pt_bloom_kernel; f.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(float(radius), _p(g), int(capacity), ctypes.byref(n), ctypes.byref(G))
    if r != PT_OK: raise PtError(r, "pt_bloom_kernel")
    return g[:n.value + 1].copy(), np.float32(G.value)


# PtAdaptiveParams / PtAdaptiveStats (include/mi355pt.h): adaptive sampling in reference mode (pt_render_adaptive)
ADAPTIVE_PARAMS_DTYPE = np.dtype([("minSamples", "<u4"), ("maxSamples", "<u4"), ("step", "<u4"), ("threshold", "<f4"), ("darkFloor", "<f4")])
ADAPTIVE_STATS_DTYPE = np.dtype([("rounds", "<u4"), ("evaluations", "<u4"), ("samplesTraced", "<u8"), ("unconvergedPixels", "<u4"), ("minCount", "<u4"), ("maxCount", "<u4"),
                                 ("errorPassMs", "<f4")])
assert ADAPTIVE_PARAMS_DTYPE.itemsize == 20 and ADAPTIVE_STATS_DTYPE.itemsize == 32


def adaptive_default_params(lib=None, **overrides):
    """pt_adaptive_default_params: minSamples 16, step 8, maxSamples 1024, threshold 0.02, darkFloor 0.01 (starting values, unmeasured); keywords override"""
    L = lib or load_library()
    out = np.zeros((), ADAPTIVE_PARAMS_DTYPE)
    f = L.pt_adaptive_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_adaptive_default_params")
    for k, v in overrides.items(): out[k] = v
    return out


# PtAccumDenoiseParams (include/mi355pt.h): the reference-mode denoiser's parameters (pt_accum_denoise)
ACCUM_DENOISE_PARAMS_DTYPE = np.dtype([("searchRadius", "<u4"), ("patchRadius", "<u4"), ("k", "<f4"), ("alpha", "<f4"), ("epsilon", "<f4"), ("maxRadiance", "<f4")])
assert ACCUM_DENOISE_PARAMS_DTYPE.itemsize == 24


def accum_denoise_default_params(lib=None, **overrides):
    """pt_accum_denoise_default_params: searchRadius 5, patchRadius 2, k 0.45, alpha 1, epsilon 1e-10, maxRadiance 65504 (starting values, unmeasured); keywords override"""
    L = lib or load_library()
    out = np.zeros((), ACCUM_DENOISE_PARAMS_DTYPE)
    f = L.pt_accum_denoise_default_params; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
    r = f(_p(out))
    if r != PT_OK: raise PtError(r, "pt_accum_denoise_default_params")
    for k, v in overrides.items(): out[k] = v
    return out


class PathTracer:
    """One pt_context (one GPU). Method names follow the C-ABI; the call order follows Sample::Render."""

    def __init__(self, device=0, shard_rank=0, shard_count=1, serial_kernels=False, prefer_fast_build=False, host_sah_builder=False, test_hooks=False, device_textures=False):
        """serial_kernels: PT_DEVICE_SERIAL_KERNELS — pt_render runs one batch on one stream (clean per-kernel timings) instead of two pipelined half-frame batches.
        prefer_fast_build: PT_DEVICE_PREFER_FAST_BUILD — scene builds use the plain device-side PLOC builder instead of the default fast-trace tree (PLOC + parallel
        re-insertion + cost-driven wide nodes, on the device); host_sah_builder: PT_DEVICE_HOST_SAH_BUILDER — round 2's binned SAH + re-insertion on the host's cores.
        device_textures: PT_DEVICE_TEXTURES_ON_DEVICE — textures are converted, mip-mapped and given their alpha planes on the device (the same bits as the host path's).
        test_hooks: run on libmi355pt_testhooks.so, the tests' build of the same sources that also exports pt_probe (include/mi355pt_testhooks.h)."""
        self.L = load_library(test_hooks)
        self.test_hooks = test_hooks
        self.h = ctypes.c_void_p()
        desc = PtDeviceDesc(device, shard_rank, shard_count, (1 if serial_kernels else 0) | (2 if prefer_fast_build else 0) | (4 if host_sah_builder else 0) | (8 if device_textures else 0))
        r = self.L.pt_create(ctypes.byref(desc), ctypes.byref(self.h))
        if r != PT_OK:
            raise PtError(r, "pt_create failed (no HIP device? this library has no CPU path)")
        self.width = self.height = 0
        self.shard_rank, self.shard_count = shard_rank, shard_count
        self._keep = []

    def _chk(self, r, what):
        if r != PT_OK:
            raise PtError(r, what + ": " + (self.L.pt_get_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            self.L.pt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- scene
    def load_scene_gltf(self, path):
        self._chk(self.L.pt_load_scene_gltf(self.h, path.encode()), "pt_load_scene_gltf")

    def apply_scene_import(self, imp):
        """pt_scene_import_apply: materials, geometry, instances and analytic lights of a SceneImport (camera / environment / settings stay with the caller)."""
        self.L.pt_scene_import_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.pt_scene_import_apply(self.h, imp.h), "pt_scene_import_apply")

    def set_scene(self, sc):
        """sc: dict from rtxpt_amd.scenes (same arrays the oracle receives)."""
        self._keep = [sc]
        tex = (PtTextureDesc * max(1, len(sc["textures"])))()
        for i, (w, h, fmt, px) in enumerate(sc["textures"]):
            tex[i] = PtTextureDesc(w, h, fmt, px.ctypes.data)
        self._chk(self.L.pt_set_materials(self.h, _p(sc["materials"]), len(sc["materials"]), tex, len(sc["textures"])), "pt_set_materials")
        gb = PtGeometryBuffers(sc["indices"].ctypes.data, sc["indices"].size, sc["positions"].ctypes.data, sc["uvs"].ctypes.data,
                               sc["normals"].ctypes.data, sc["tangents"].ctypes.data, sc["positions"].shape[0])
        self._chk(self.L.pt_set_geometry(self.h, ctypes.byref(gb), _p(sc["geometries"]), len(sc["geometries"]), _p(sc["meshes"]), len(sc["meshes"])), "pt_set_geometry")
        self._chk(self.L.pt_set_instances(self.h, _p(sc["instances"]), len(sc["instances"])), "pt_set_instances")
        if sc.get("env") is not None or sc.get("env_cube_source") is not None:
            rgb, tw, cm = sc["env"] if sc.get("env") is not None else sc["env_cube_source"]      # "env_cube_source": (faces float32 [6, d, d, 4], transform, colour multiplier) — a cube map as the image
            # EnvMapSceneParams::ColorMultiplier as Sample.cpp:1936-1948 fills it: tint * intensity / c_envMapRadianceScale (the cube holds radiance * 1/4)
            cm4 = (np.asarray(cm, np.float32) * np.float32(4.0)).astype(np.float32)
            p = PtEnvMapSceneParams((ctypes.c_float * 12)(*tw.tolist()), (ctypes.c_float * 3)(*cm4.tolist()), 1.0)
            if sc.get("env") is not None:
                self._chk(self.L.pt_set_environment(self.h, _p(rgb), rgb.shape[1], rgb.shape[0], ctypes.byref(p)), "pt_set_environment")
            else:
                faces = np.ascontiguousarray(rgb, np.float32); assert faces.ndim == 4 and faces.shape[0] == 6 and faces.shape[1] == faces.shape[2] and faces.shape[3] == 4
                self._chk(self.L.pt_set_environment_cube(self.h, _p(faces), faces.shape[1], ctypes.byref(p)), "pt_set_environment_cube")
            dl = sc.get("env_directional_lights")       # rows of EMB_DirectionalLight: colour rgb, intensity, direction xyz, angular size
            dl = np.ascontiguousarray(dl, np.float32).reshape(-1, 8) if dl is not None else np.zeros((0, 8), np.float32)
            self._chk(self.L.pt_set_environment_bake(self.h, int(sc.get("env_cube_dim", 256)), _p(dl) if len(dl) else None, len(dl)), "pt_set_environment_bake")
            self._chk(self.L.pt_set_environment_compression(self.h, int(sc.get("env_compression", 0))), "pt_set_environment_compression")
        else:
            self._chk(self.L.pt_set_environment(self.h, None, 0, 0, None), "pt_set_environment")
        if sc.get("sky") is not None:                   # {"consts": PtProceduralSkyConstants or 40 floats, "textures": four arrays}: the procedural sky as the cube's source
            self.set_procedural_sky(sc["sky"]["consts"], sc["sky"].get("textures"))
            if sc.get("env") is None and sc.get("env_cube_source") is None: self._chk(self.L.pt_set_environment_bake(self.h, int(sc.get("env_cube_dim", 256)), None, 0), "pt_set_environment_bake")
        if sc.get("lights") is not None:
            base, ex = sc["lights"]
            self._chk(self.L.pt_set_lights(self.h, _p(base), _p(ex), len(base)), "pt_set_lights")

    def set_environment(self, env):
        """pt_set_environment alone: env = (lat-long float32 [h, w, 3], transform [12], colour multiplier [3]) as a scene's "env" entry, or None (off). The bake settings stay."""
        if env is None: self._chk(self.L.pt_set_environment(self.h, None, 0, 0, None), "pt_set_environment"); return
        rgb, tw, cm = env; rgb = np.ascontiguousarray(rgb, np.float32)
        cm4 = (np.asarray(cm, np.float32) * np.float32(4.0)).astype(np.float32)
        p = PtEnvMapSceneParams((ctypes.c_float * 12)(*np.asarray(tw, np.float32).tolist()), (ctypes.c_float * 3)(*cm4.tolist()), 1.0)
        self._chk(self.L.pt_set_environment(self.h, _p(rgb), rgb.shape[1], rgb.shape[0], ctypes.byref(p)), "pt_set_environment")

    def set_procedural_sky(self, consts, textures=None):
        """consts: PtProceduralSkyConstants / 40 float32 values / None (off); textures: four float32 arrays (transmittance, scattering, irradiance, clouds) or None (keep)"""
        if consts is None: self._chk(self.L.pt_set_procedural_sky(self.h, None, None), "pt_set_procedural_sky"); return
        cbuf = np.frombuffer(bytes(consts), np.float32).copy() if isinstance(consts, ctypes.Structure) else np.ascontiguousarray(consts, np.float32).reshape(40)
        t = keep = None
        if textures is not None: t, keep = _sky_textures(textures)
        self._chk(self.L.pt_set_procedural_sky(self.h, _p(cbuf), ctypes.byref(t) if t is not None else None), "pt_set_procedural_sky")

    def set_local_light_sampling(self, table=None, jitter=(0, 0), ratio=0.65, ssc_threshold=0.3, feedback=False):
        """NEE-AT inputs (pt_set_local_light_sampling). table: uint32 [tilesY, tilesX, 128] packed entries (light << 9 | count - 1, sorted per tile) or None (no local layer)"""
        f = self.L.pt_set_local_light_sampling
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_float, ctypes.c_float, ctypes.c_int32]; f.restype = ctypes.c_int32
        if table is None: self._chk(f(self.h, None, 0, 0, 0, 0, float(ratio), float(ssc_threshold), 1 if feedback else 0), "pt_set_local_light_sampling"); return
        t = np.ascontiguousarray(table, np.uint32)
        if t.ndim != 3 or t.shape[2] != 128: raise ValueError("local sampling table: uint32 [tilesY, tilesX, 128]")
        self._chk(f(self.h, _p(t), t.shape[1], t.shape[0], int(jitter[0]), int(jitter[1]), float(ratio), float(ssc_threshold), 1 if feedback else 0), "pt_set_local_light_sampling")

    def set_light_importance_boost(self, view_proj=None, mul=8.0, fade_distance=5.0):
        """pt_set_light_importance_boost: the frustum term of LightsBaker's ImportanceBooster; view_proj: the host's 4 x 4 view-projection matrix (row vectors: clip = p @ M) or None (off)"""
        f = self.L.pt_set_light_importance_boost; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float]; f.restype = ctypes.c_int32
        m = None if view_proj is None else np.ascontiguousarray(view_proj, np.float32).reshape(16)
        self._chk(f(self.h, _p(m), float(mul), float(fade_distance)), "pt_set_light_importance_boost")

    def set_view_projection(self, world_to_clip=None):
        """pt_set_view_projection: the host's world-to-clip matrix (row vectors), for the depth the reference-mode path tracer exports and NEE-AT's disocclusion test reads"""
        f = self.L.pt_set_view_projection; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        m = None if world_to_clip is None else np.ascontiguousarray(world_to_clip, np.float32).reshape(16)
        self._chk(f(self.h, _p(m)), "pt_set_view_projection")

    def build_stable_planes(self, sample_index, params):
        """pt_build_stable_planes + pt_get_stable_planes: the realtime mode's pre-pass over the frame. params: a record of scenes.STABLE_PLANES_PARAMS_DTYPE. Returns a dict of
        header [4, h, w] u32, planes [3 * plane stride, 20] u32 (records of scenes.STABLE_PLANE_DTYPE, tiled-swizzled order), stable_radiance / motion_vectors [h, w, 4] binary16 bit
        patterns, depth / spec_hit_t [h, w] f32, throughput [h, w] R11G11B10, plane_stride, stats."""
        w, h = self.width, self.height
        f = self.L.pt_stable_planes_plane_stride; f.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        stride = ctypes.c_uint32(0); self._chk(f(w, h, ctypes.byref(stride)), "pt_stable_planes_plane_stride"); stride = int(stride.value)
        prm = np.ascontiguousarray(params); assert prm.dtype.itemsize == 224
        st = PtFrameStats()
        f = self.L.pt_build_stable_planes; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, int(sample_index), _p(prm), ctypes.byref(st)), "pt_build_stable_planes")
        out = dict(header=np.zeros((4, h, w), np.uint32), planes=np.zeros((3 * stride, 20), np.uint32), stable_radiance=np.zeros((h, w, 4), np.uint16), depth=np.zeros((h, w), np.float32),
                   spec_hit_t=np.zeros((h, w), np.float32), motion_vectors=np.zeros((h, w, 4), np.uint16), throughput=np.zeros((h, w), np.uint32))
        f = self.L.pt_get_stable_planes; f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 5; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(out["header"]), _p(out["planes"]), 3 * stride, _p(out["stable_radiance"]), _p(out["depth"]), _p(out["spec_hit_t"]), _p(out["motion_vectors"]), _p(out["throughput"])), "pt_get_stable_planes")
        out["plane_stride"] = stride
        out["stats"] = st.as_dict()
        return out

    def fill_stable_planes(self, sample_index, params, sub_samples=1):
        """pt_fill_stable_planes for sub_samples consecutive sample indices + pt_get_stable_planes: the realtime mode's noisy passes over the frame build_stable_planes left.
        Returns the same dict as build_stable_planes (planes with their noisy radiance, spec_hit_t filled), stats summed over the sub-samples."""
        prm = np.ascontiguousarray(params); assert prm.dtype.itemsize == 224
        f = self.L.pt_fill_stable_planes; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        total = {}
        for s in range(sub_samples):
            st = PtFrameStats()
            self._chk(f(self.h, int(sample_index) + s, _p(prm), ctypes.byref(st)), "pt_fill_stable_planes")
            for k, v in st.as_dict().items():
                if np.isscalar(v): total[k] = total.get(k, 0) + v
        w, h = self.width, self.height
        g = self.L.pt_stable_planes_plane_stride; g.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]; g.restype = ctypes.c_int32
        stride = ctypes.c_uint32(0); self._chk(g(w, h, ctypes.byref(stride)), "pt_stable_planes_plane_stride"); stride = int(stride.value)
        out = dict(header=np.zeros((4, h, w), np.uint32), planes=np.zeros((3 * stride, 20), np.uint32), stable_radiance=np.zeros((h, w, 4), np.uint16), depth=np.zeros((h, w), np.float32),
                   spec_hit_t=np.zeros((h, w), np.float32), motion_vectors=np.zeros((h, w, 4), np.uint16), throughput=np.zeros((h, w), np.uint32))
        g = self.L.pt_get_stable_planes; g.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 5; g.restype = ctypes.c_int32
        self._chk(g(self.h, _p(out["header"]), _p(out["planes"]), 3 * stride, _p(out["stable_radiance"]), _p(out["depth"]), _p(out["spec_hit_t"]), _p(out["motion_vectors"]), _p(out["throughput"])), "pt_get_stable_planes")
        out["plane_stride"] = stride; out["stats"] = total
        return out

    def get_stable_planes(self):
        """pt_get_stable_planes: the buffers of the last build / fill / realtime pass (the dict build_stable_planes returns, without stats)"""
        w, h = self.width, self.height
        g = self.L.pt_stable_planes_plane_stride; g.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]; g.restype = ctypes.c_int32
        stride = ctypes.c_uint32(0); self._chk(g(w, h, ctypes.byref(stride)), "pt_stable_planes_plane_stride"); stride = int(stride.value)
        out = dict(header=np.zeros((4, h, w), np.uint32), planes=np.zeros((3 * stride, 20), np.uint32), stable_radiance=np.zeros((h, w, 4), np.uint16), depth=np.zeros((h, w), np.float32),
                   spec_hit_t=np.zeros((h, w), np.float32), motion_vectors=np.zeros((h, w, 4), np.uint16), throughput=np.zeros((h, w), np.uint32))
        g = self.L.pt_get_stable_planes; g.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 5; g.restype = ctypes.c_int32
        self._chk(g(self.h, _p(out["header"]), _p(out["planes"]), 3 * stride, _p(out["stable_radiance"]), _p(out["depth"]), _p(out["spec_hit_t"]), _p(out["motion_vectors"]), _p(out["throughput"])), "pt_get_stable_planes")
        out["plane_stride"] = stride
        return out

    def stable_planes_shard_bytes(self, rank):
        f = self.L.pt_stable_planes_shard_bytes; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        n = ctypes.c_size_t(0); self._chk(f(self.h, int(rank), ctypes.byref(n)), "pt_stable_planes_shard_bytes"); return int(n.value)

    # ---- the records of a tile-sharded frame as flat device buffers (device pointers come from torch tensors): the owned pixels' records in shard_layout order / rank `rank`'s into place
    def _pack(self, name, device_ptr, nbytes):
        f = getattr(self.L, name); f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.c_void_p(device_ptr), nbytes), name)

    def _unpack(self, name, device_ptr, nbytes, rank):
        f = getattr(self.L, name); f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.c_void_p(device_ptr), nbytes, int(rank)), name)

    def pack_shard(self, device_ptr, nbytes): self._pack("pt_pack_shard", device_ptr, nbytes)      # the radiance, 16 bytes per pixel
    def unpack_shard(self, device_ptr, nbytes, rank): self._unpack("pt_unpack_shard", device_ptr, nbytes, rank)
    def neeat_pack_feedback(self, device_ptr, nbytes): self._pack("pt_neeat_pack_feedback", device_ptr, nbytes)      # reservoir weight | candidate | exported depth, 12 bytes
    def neeat_unpack_feedback(self, device_ptr, nbytes, rank): self._unpack("pt_neeat_unpack_feedback", device_ptr, nbytes, rank)
    def pack_stable_plane_guides(self, device_ptr, nbytes): self._pack("pt_pack_stable_plane_guides", device_ptr, nbytes)      # depth | specular hit distance | motion vectors, 16 bytes: what the other ranks' bakers need of the build pass
    def unpack_stable_plane_guides(self, device_ptr, nbytes, rank): self._unpack("pt_unpack_stable_plane_guides", device_ptr, nbytes, rank)
    def pack_stable_planes(self, device_ptr, nbytes): self._pack("pt_pack_stable_planes", device_ptr, nbytes)      # the whole record, stable_planes_shard_bytes
    def unpack_stable_planes(self, device_ptr, nbytes, rank): self._unpack("pt_unpack_stable_planes", device_ptr, nbytes, rank)

    def neeat_update_begin(self):
        """pt_neeat_update_begin: LightsBaker::UpdateBegin on its own (the realtime frame in parts)"""
        f = self.L.pt_neeat_update_begin; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32; self._chk(f(self.h), "pt_neeat_update_begin")

    def neeat_update_end(self):
        """pt_neeat_update_end: LightsBaker::UpdateEnd on the depth and motion vectors the last build_stable_planes left"""
        f = self.L.pt_neeat_update_end; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32; self._chk(f(self.h), "pt_neeat_update_end")

    def gather_stable_planes(self):
        f = self.L.pt_gather_stable_planes; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h), "pt_gather_stable_planes")

    def realtime_frame(self, sample_index, params):
        """pt_realtime_frame: UpdateBegin -> build pass -> UpdateEnd on this frame's depth and motion vectors -> params.subSampleCount fill passes (with pt_set_neeat: the baker in the loop).
        Returns (buffers as get_stable_planes, build stats, fill stats)."""
        prm = np.ascontiguousarray(params); assert prm.dtype.itemsize == 224
        f = self.L.pt_realtime_frame; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        b, fl = PtFrameStats(), PtFrameStats()
        self._chk(f(self.h, int(sample_index), _p(prm), ctypes.byref(b), ctypes.byref(fl)), "pt_realtime_frame")
        return self.get_stable_planes(), b.as_dict(), fl.as_dict()

    def stable_planes_merge(self):
        """pt_stable_planes_merge: the realtime frame without a denoiser (stable + noisy radiance) into the radiance buffer; returns radiance()"""
        f = self.L.pt_stable_planes_merge; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h), "pt_stable_planes_merge")
        return self.radiance()

    def denoise_spec_hit_t(self):
        """pt_denoise_spec_hit_t: the fill-in of the specular hit distance that ends a realtime frame's noisy passes; returns spec_hit_t [h, w] f32"""
        f = self.L.pt_denoise_spec_hit_t; f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h), "pt_denoise_spec_hit_t")
        out = np.zeros((self.height, self.width), np.float32)
        g = self.L.pt_get_stable_planes; g.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 5; g.restype = ctypes.c_int32
        self._chk(g(self.h, None, None, 0, None, None, _p(out), None, None), "pt_get_stable_planes")
        return out

    def denoiser_prepare_dlss_rr(self, sp_params, params):
        """pt_denoiser_prepare_dlss_rr: PostProcess.hlsl DENOISER_PREPARE_INPUTS with DENOISER_DLSS_RR over the context's planes. sp_params: scenes.STABLE_PLANES_PARAMS_DTYPE,
        params: DENOISER_PARAMS_DTYPE. The main input colour goes to the radiance buffer (radiance()); the guides: get_denoiser_inputs()."""
        prm = np.ascontiguousarray(sp_params); dn = np.ascontiguousarray(params); assert prm.dtype.itemsize == 224 and dn.dtype == DENOISER_PARAMS_DTYPE
        f = self.L.pt_denoiser_prepare_dlss_rr; f.argtypes = [ctypes.c_void_p] * 3; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(prm), _p(dn)), "pt_denoiser_prepare_dlss_rr")

    def denoiser_prepare_nrd(self, sp_params, params, plane_index, init_with_stable_radiance):
        """pt_denoiser_prepare_nrd: PostProcess.hlsl DENOISER_PREPARE_INPUTS for NRD, one plane (Sample::Denoise calls planes active - 1 .. 0, init on the first call only)"""
        prm = np.ascontiguousarray(sp_params); dn = np.ascontiguousarray(params); assert prm.dtype.itemsize == 224 and dn.dtype == DENOISER_PARAMS_DTYPE
        f = self.L.pt_denoiser_prepare_nrd; f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint32]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(prm), _p(dn), int(plane_index), 1 if init_with_stable_radiance else 0), "pt_denoiser_prepare_nrd")

    def denoiser_merge_nrd(self, plane_index, diff_device_ptr, spec_device_ptr):
        """pt_denoiser_merge_nrd: DENOISER_FINAL_MERGE of one plane; the two arguments are device pointers (ints) to the host's unpacked denoised radiance, RGBA32F, h x w"""
        f = self.L.pt_denoiser_merge_nrd; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, int(plane_index), ctypes.c_void_p(diff_device_ptr), ctypes.c_void_p(spec_device_ptr)), "pt_denoiser_merge_nrd")

    def get_denoiser_inputs(self, keys=None):
        """pt_get_denoiser_inputs: {key: array} for the keys of DENOISER_BUFFERS (all of them by default); [h, w] or [h, w, n]"""
        h, w = self.height, self.width
        out, b = {}, PtDenoiserBuffers()
        for k, dt, n in DENOISER_BUFFERS:
            if keys is not None and k not in keys: continue
            out[k] = np.zeros((h, w) if n == 1 else (h, w, n), dt); setattr(b, k, out[k].ctypes.data)
        f = self.L.pt_get_denoiser_inputs; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.byref(b)), "pt_get_denoiser_inputs")
        return out

    def denoiser_device_buffers(self):
        """pt_denoiser_device_buffers: {key: (device pointer, row pitch in bytes)}"""
        b = PtDenoiserBuffers()
        f = self.L.pt_denoiser_device_buffers; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.byref(b)), "pt_denoiser_device_buffers")
        return {k: (getattr(b, k), int(b.pitch[i])) for i, (k, _, _) in enumerate(DENOISER_BUFFERS)}

    def denoise_plane(self, sp_params, settings, plane_index, reset_history=False):
        """pt_denoise_plane: the device denoiser over the NRD buffers denoiser_prepare_nrd(plane_index) just left; settings: DENOISE_SETTINGS_DTYPE. Result: get_denoised()"""
        prm = np.ascontiguousarray(sp_params); ds = np.ascontiguousarray(settings); assert prm.dtype.itemsize == 224 and ds.dtype == DENOISE_SETTINGS_DTYPE
        f = self.L.pt_denoise_plane; f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint32]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(prm), _p(ds), int(plane_index), 1 if reset_history else 0), "pt_denoise_plane")

    def denoised_device_buffers(self, plane_index):
        """pt_denoised_device_buffers: (diffuse device pointer, specular device pointer, row pitch in bytes) of a plane's denoised radiance: what denoiser_merge_nrd takes"""
        d, s, pitch = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        f = self.L.pt_denoised_device_buffers; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 3; f.restype = ctypes.c_int32
        self._chk(f(self.h, int(plane_index), ctypes.byref(d), ctypes.byref(s), ctypes.byref(pitch)), "pt_denoised_device_buffers")
        return d.value, s.value, int(pitch.value)

    def get_denoised(self, plane_index):
        """pt_get_denoised: (diffuse [h, w, 4] f32, specular [h, w, 4] f32, history lengths [h, w, 2] f32: diffuse, specular) of a plane after denoise_plane"""
        h, w = self.height, self.width
        d, s, n = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w, 2), np.float32)
        f = self.L.pt_get_denoised; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 3; f.restype = ctypes.c_int32
        self._chk(f(self.h, int(plane_index), _p(d), _p(s), _p(n)), "pt_get_denoised")
        return d, s, n

    def denoise_frame(self, sp_params, params, settings, reset_history=False):
        """pt_denoise_frame: Sample::Denoise's loop — planes active - 1 .. 0: prepare (init on the first), denoise, merge; returns radiance()"""
        prm = np.ascontiguousarray(sp_params); dn = np.ascontiguousarray(params); ds = np.ascontiguousarray(settings)
        assert prm.dtype.itemsize == 224 and dn.dtype == DENOISER_PARAMS_DTYPE and ds.dtype == DENOISE_SETTINGS_DTYPE
        f = self.L.pt_denoise_frame; f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(prm), _p(dn), _p(ds), 1 if reset_history else 0), "pt_denoise_frame")
        return self.radiance()

    # ---- the display tail (pt_display.hip): one mirror per kind of entry point; `size` is (W, H) of the picture, `selector` the uint32 arguments that pick it
    def _tonemap(self, name, params, size, *selector):
        """a tone map entry point (TONEMAP_DTYPE; default_tonemap() if None) -> (H, W, 4) uint8"""
        t = default_tonemap() if params is None else params
        out = np.empty((size[1], size[0], 4), dtype=np.uint8)
        f = getattr(self.L, name); f.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * len(selector) + [ctypes.c_void_p, ctypes.c_size_t]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(t), *selector, _p(out), out.nbytes), name)
        return out

    def _average_luminance(self, name, *selector):
        """an average luminance entry point -> float"""
        v = ctypes.c_float(0.0)
        f = getattr(self.L, name); f.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] * len(selector) + [ctypes.POINTER(ctypes.c_float)]; f.restype = ctypes.c_int32
        self._chk(f(self.h, *selector, ctypes.byref(v)), name)
        return float(v.value)

    def _device_buffer(self, name):
        """a device buffer entry point -> (device pointer, row pitch in bytes)"""
        d, pitch = ctypes.c_void_p(), ctypes.c_size_t()
        f = getattr(self.L, name); f.argtypes = [ctypes.c_void_p] * 3; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.byref(d), ctypes.byref(pitch)), name)
        return d.value, int(pitch.value)

    def _read_back(self, name, size, capacity=False):
        """a read-back entry point -> [H, W, 4] f32; capacity: it takes the buffer's size in floats"""
        out = np.empty((size[1], size[0], 4), np.float32)
        f = getattr(self.L, name); f.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_size_t] * capacity; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(out), *([out.size] * capacity)), name)
        return out

    def taa_resolve(self, params=None, reset_history=False, timed=False):
        """pt_taa_resolve: the radiance buffer resolved against the previous call's result (TAA_PARAMS_DTYPE; defaults if None). Returns get_resolved(), or with timed
        (resolved, the kernel's event-timed milliseconds)"""
        tp = np.ascontiguousarray(taa_default_params(self.L) if params is None else params); assert tp.dtype == TAA_PARAMS_DTYPE
        ms = ctypes.c_float(0.0)
        f = self.L.pt_taa_resolve; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(tp), 1 if reset_history else 0, ctypes.byref(ms) if timed else None), "pt_taa_resolve")
        return (self.get_resolved(), float(ms.value)) if timed else self.get_resolved()

    def get_resolved(self):
        """pt_get_resolved: the resolved picture of the last taa_resolve, [h, w, 4] f32, alpha 1"""
        return self._read_back("pt_get_resolved", (self.width, self.height))

    def resolved_device_buffer(self):
        """pt_resolved_device_buffer: (device pointer, row pitch in bytes) of the resolved picture"""
        return self._device_buffer("pt_resolved_device_buffer")

    def tonemap_resolved(self, params=None):
        """pt_tonemap_resolved: tonemap() over the resolved picture instead of the radiance buffer -> (H, W, 4) uint8"""
        return self._tonemap("pt_tonemap_resolved", params, (self.width, self.height))

    def bloom(self, params=None, source=0, timed=False):
        """pt_bloom: source 0 (the radiance buffer) or 1 (the resolved picture of taa_resolve) bloomed into a third buffer (BLOOM_PARAMS_DTYPE; defaults if None). Returns
        bloomed(), or with timed (bloomed, the pass's event-timed milliseconds)"""
        bp = np.ascontiguousarray(bloom_default_params(self.L) if params is None else params); assert bp.dtype == BLOOM_PARAMS_DTYPE
        ms = ctypes.c_float(0.0)
        f = self.L.pt_bloom; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(bp), int(source), ctypes.byref(ms) if timed else None), "pt_bloom")
        return (self.bloomed(), float(ms.value)) if timed else self.bloomed()

    def bloomed(self):
        """pt_get_bloomed: the bloomed picture of the last bloom, [h, w, 4] f32"""
        return self._read_back("pt_get_bloomed", (self.width, self.height))

    def bloomed_device_buffer(self):
        """pt_bloomed_device_buffer: (device pointer, row pitch in bytes) of the bloomed picture"""
        return self._device_buffer("pt_bloomed_device_buffer")

    def tonemap_bloomed(self, params=None):
        """pt_tonemap_bloomed: tonemap() over the bloomed picture instead of the radiance buffer -> (H, W, 4) uint8"""
        return self._tonemap("pt_tonemap_bloomed", params, (self.width, self.height))

    def average_luminance_bloomed(self):
        """pt_average_luminance_bloomed: average_luminance() of the bloomed picture — the picture the reference's auto exposure measures"""
        return self._average_luminance("pt_average_luminance_bloomed")

    def taa_upscale(self, params=None, display=None, jitter=(0.0, 0.0), reset_history=False, timed=False):
        """pt_taa_upscale: the radiance buffer (the frame size is the render size) resolved into the display-size history (TAA_UPSCALE_PARAMS_DTYPE; defaults if None).
        display: (W, H), within [w, 4 w] x [h, 4 h]; jitter: the frame's camera offset in render pixels (None: the library's NULL). Returns upscaled(), or with timed
        (upscaled, the kernel's event-timed milliseconds)"""
        up = np.ascontiguousarray(taa_upscale_default_params(self.L) if params is None else params); assert up.dtype == TAA_UPSCALE_PARAMS_DTYPE
        W, H = (self.width, self.height) if display is None else display
        j = None if jitter is None else (ctypes.c_float * 2)(float(jitter[0]), float(jitter[1]))
        ms = ctypes.c_float(0.0)
        f = self.L.pt_taa_upscale; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(up), int(W), int(H), j, 1 if reset_history else 0, ctypes.byref(ms) if timed else None), "pt_taa_upscale")
        return (self.upscaled(), float(ms.value)) if timed else self.upscaled()

    def upscaled_size(self):
        """pt_upscaled_size: (W, H) of the upscaled picture"""
        W, H = ctypes.c_uint32(), ctypes.c_uint32()
        f = self.L.pt_upscaled_size; f.argtypes = [ctypes.c_void_p] * 3; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.byref(W), ctypes.byref(H)), "pt_upscaled_size")
        return int(W.value), int(H.value)

    def upscaled(self):
        """pt_get_upscaled: the upscaled picture of the last taa_upscale, [H, W, 4] f32, alpha 1"""
        return self._read_back("pt_get_upscaled", self.upscaled_size(), capacity=True)

    def upscaled_device_buffer(self):
        """pt_upscaled_device_buffer: (device pointer, row pitch in bytes) of the upscaled picture"""
        return self._device_buffer("pt_upscaled_device_buffer")

    def bloom_upscaled(self, params=None, timed=False):
        """pt_bloom_upscaled: bloom()'s pass over the upscaled picture at the display size, into a bloomed picture of its own. Returns upscaled_bloomed(), or with timed
        (upscaled_bloomed, the pass's event-timed milliseconds)"""
        bp = np.ascontiguousarray(bloom_default_params(self.L) if params is None else params); assert bp.dtype == BLOOM_PARAMS_DTYPE
        ms = ctypes.c_float(0.0)
        f = self.L.pt_bloom_upscaled; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(bp), ctypes.byref(ms) if timed else None), "pt_bloom_upscaled")
        return (self.upscaled_bloomed(), float(ms.value)) if timed else self.upscaled_bloomed()

    def upscaled_bloomed(self):
        """pt_get_upscaled_bloomed: the bloomed picture of the last bloom_upscaled, [H, W, 4] f32"""
        return self._read_back("pt_get_upscaled_bloomed", self.upscaled_size(), capacity=True)

    def tonemap_upscaled(self, params=None, bloomed=False):
        """pt_tonemap_upscaled: tonemap() over the upscaled picture, or with bloomed over its bloom -> (H, W, 4) uint8 at the display size"""
        return self._tonemap("pt_tonemap_upscaled", params, self.upscaled_size(), int(bloomed))

    def average_luminance_upscaled(self, bloomed=False):
        """pt_average_luminance_upscaled: average_luminance() of the upscaled picture, or with bloomed of its bloom"""
        return self._average_luminance("pt_average_luminance_upscaled", int(bloomed))

    def denoise_pass_times(self, enable=True):
        """pt_denoise_pass_times: switches the event timing of denoise_plane's passes on / off and returns the last timed call's milliseconds [temporal, clamp, a-trous 0, 1, ...]"""
        ms = np.zeros(16, np.float32); n = ctypes.c_uint32()
        f = self.L.pt_denoise_pass_times; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, 1 if enable else 0, _p(ms), 16, ctypes.byref(n)), "pt_denoise_pass_times")
        return ms[:n.value].copy()

    def set_texture_filtering(self, enable, filter=1, magnification=0, gaussian_sigma=0.3):
        """pt_set_texture_filtering: stochastic texture filtering — one texel per material lookup (filter: PT_STF_FILTER_POINT / LINEAR / CUBIC). Off by default."""
        p = PtTextureFiltering(1 if enable is True else int(enable), int(filter), int(magnification), float(gaussian_sigma))
        f = self.L.pt_set_texture_filtering; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, ctypes.byref(p)), "pt_set_texture_filtering")

    def set_neeat(self, enable=True, global_feedback_weight=0.75, ratio=0.65, ssc_threshold=0.3, prefilter=True):
        """NEE-AT with the light baker in the loop (pt_set_neeat): every sample of render() becomes a frame — feedback passes, then the path tracer"""
        f = self.L.pt_set_neeat; f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int32]; f.restype = ctypes.c_int32
        self._chk(f(self.h, 1 if enable else 0, float(global_feedback_weight), float(ratio), float(ssc_threshold), 1 if prefilter else 0), "pt_set_neeat")

    def neeat_reset(self): self._chk(self.L.pt_neeat_reset(self.h), "pt_neeat_reset")

    def neeat_tables(self):
        """(tile table uint32 [tilesY, tilesX, 128], jitter (x, y)) the last frame was traced with"""
        txy = np.zeros(2, np.uint32); jxy = np.zeros(2, np.uint32)
        self._chk(self.L.pt_get_neeat_tables(self.h, _p(txy), _p(jxy), None, 0), "pt_get_neeat_tables")
        t = np.zeros((int(txy[1]), int(txy[0]), 128), np.uint32)
        self._chk(self.L.pt_get_neeat_tables(self.h, None, None, _p(t), t.size), "pt_get_neeat_tables")
        return t, (int(jxy[0]), int(jxy[1]))

    def light_feedback(self, sample=0):
        """the feedback reservoirs sample `sample` of the last render() call filled: (total weight float32 [H, W], candidate uint32 [H, W])"""
        w = np.zeros((self.height, self.width), np.float32); c = np.zeros((self.height, self.width), np.uint32)
        self._chk(self.L.pt_get_light_feedback(self.h, int(sample), _p(w), _p(c)), "pt_get_light_feedback")
        return w, c

    def animate(self, instances=None, positions=None, rebuild=False, vertex_ranges=None):
        """pt_animate; vertex_ranges = [(first, count), ...]: pt_animate_ranges — only those vertices of `positions` moved"""
        if vertex_ranges is None:
            self._chk(self.L.pt_animate(self.h, _p(instances), 0 if instances is None else len(instances), _p(positions), 0 if positions is None else positions.shape[0],
                                        1 if rebuild else 0), "pt_animate")
            return
        f = self.L.pt_animate_ranges; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32]; f.restype = ctypes.c_int32
        r = np.ascontiguousarray(np.asarray(vertex_ranges, np.uint32).reshape(-1, 2))
        self._chk(f(self.h, _p(instances), 0 if instances is None else len(instances), _p(positions), 0 if positions is None else positions.shape[0], _p(r), len(r), 1 if rebuild else 0), "pt_animate_ranges")

    def set_motion_history(self, enable=True):
        """pt_set_motion_history: every animate() call is a scene refresh from now on (the pose it finds becomes the previous pose); the stable-plane build pass's motion vectors carry object motion"""
        f = self.L.pt_set_motion_history; f.argtypes = [ctypes.c_void_p, ctypes.c_int32]; f.restype = ctypes.c_int32
        self._chk(f(self.h, 1 if enable else 0), "pt_set_motion_history")

    def set_previous_pose(self, instances=None, positions=None):
        """pt_set_previous_pose: the previous frame's instance transforms / vertex positions handed over directly (None = that part did not move)"""
        f = self.L.pt_set_previous_pose; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]; f.restype = ctypes.c_int32
        a = None if instances is None else np.ascontiguousarray(instances); b = None if positions is None else np.ascontiguousarray(positions, np.float32)
        self._chk(f(self.h, _p(a), 0 if a is None else len(a), _p(b), 0 if b is None else b.shape[0]), "pt_set_previous_pose")

    def animate_normals(self, normals=None, tangents=None):
        """pt_animate_normals: the deformed meshes' packed vertex normals / tangents (uint32 per vertex, SNORM8) — with pt_animate(positions) a skinned frame is complete"""
        f = self.L.pt_animate_normals; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]; f.restype = ctypes.c_int32
        n = len(normals) if normals is not None else len(tangents)
        a = None if normals is None else np.ascontiguousarray(normals, np.uint32); b = None if tangents is None else np.ascontiguousarray(tangents, np.uint32)
        self._chk(f(self.h, _p(a), _p(b), n), "pt_animate_normals")

    def set_skinning(self, desc):
        """pt_set_skinning: a SkinningDesc (GltfAnimation.skinning(), or a host's own) uploaded once; the scene's current positions become the bind pose. None removes it."""
        f = self.L.pt_set_skinning; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        if desc is None: self._chk(f(self.h, None), "pt_set_skinning"); return
        d = desc.struct()
        self._chk(f(self.h, ctypes.byref(d)), "pt_set_skinning")

    def animate_skinned(self, instances=None, matrices=None, morph_weights=None, rebuild=False):
        """pt_animate_skinned: one scene refresh from a joint palette (float64 [M, 16], column major) and morph weights (float64 [W]), posed on the device"""
        f = self.L.pt_animate_skinned; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32]; f.restype = ctypes.c_int32
        i = None if instances is None else np.ascontiguousarray(instances)
        m = None if matrices is None else np.ascontiguousarray(matrices, np.float64).reshape(-1, 16); w = None if morph_weights is None else np.ascontiguousarray(morph_weights, np.float64).reshape(-1)
        self._chk(f(self.h, _p(i), 0 if i is None else len(i), _p(m), 0 if m is None else len(m), _p(w), 0 if w is None else len(w), 1 if rebuild else 0), "pt_animate_skinned")

    def animate_gltf(self, anim, t, animation=0, rebuild=False):
        """a GltfAnimation's frame at time t [s] on the device: its instances and palette through animate_skinned (set_skinning(anim.skinning()) first)"""
        m, w = anim.palette(t, animation)
        self.animate_skinned(anim.instances(t, animation), m, w, rebuild)

    def skinning_time(self):
        """pt_get_skinning_time: the skinning kernel's device time in the last animate_skinned call [ms]"""
        f = self.L.pt_get_skinning_time; f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]; f.restype = ctypes.c_int32
        ms = ctypes.c_double(); self._chk(f(self.h, ctypes.byref(ms)), "pt_get_skinning_time"); return ms.value

    def vertex_streams(self, previous=False):
        """pt_get_vertex_streams: the device's current streams, (positions float32 [V, 3], normals uint32 [V], tangents uint32 [V]); previous=True: the previous pose's
        positions as a fourth array (motion history on)"""
        f = self.L.pt_get_vertex_streams; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]; f.restype = ctypes.c_int32
        n = f(self.h, None, None, None, None, 0)
        if n < 0: self._chk(-n, "pt_get_vertex_streams")
        p = np.zeros((n, 3), np.float32); q = np.zeros((n, 3), np.float32) if previous else None; nr = np.zeros(n, np.uint32); tg = np.zeros(n, np.uint32)
        if n:
            r = f(self.h, _p(p), _p(q), _p(nr), _p(tg), n)
            if r < 0: self._chk(-r, "pt_get_vertex_streams")
        return (p, nr, tg, q) if previous else (p, nr, tg)

    # ---- per-frame state
    def set_camera(self, cam):
        cam = np.ascontiguousarray(cam)
        self._chk(self.L.pt_set_camera(self.h, _p(cam)), "pt_set_camera")

    def default_settings(self):
        s = np.zeros((), dtype=scenes.SETTINGS_DTYPE)
        self._chk(self.L.pt_default_settings(_p(s)), "pt_default_settings")
        return s

    def set_settings(self, s):
        s = np.ascontiguousarray(s)
        self._chk(self.L.pt_set_settings(self.h, _p(s)), "pt_set_settings")

    def resize(self, w, h):
        self.width, self.height = w, h
        self._chk(self.L.pt_resize(self.h, w, h), "pt_resize")

    def reset_accumulation(self):
        self._chk(self.L.pt_reset_accumulation(self.h), "pt_reset_accumulation")

    def set_counters(self, enable):
        self._chk(self.L.pt_set_counters(self.h, 1 if enable else 0), "pt_set_counters")

    def render(self, first, count):
        st = PtFrameStats()
        self._chk(self.L.pt_render(self.h, first, count, ctypes.byref(st)), "pt_render")
        return st.as_dict()

    def render_adaptive(self, params=None):
        """pt_render_adaptive: a new accumulation sampled in rounds of `step` samples, the 8 x 8 blocks whose error estimate is below the threshold leaving between rounds
        (ADAPTIVE_PARAMS_DTYPE; defaults if None). Returns (PtAdaptiveStats as a dict, PtFrameStats summed over the rounds as a dict). render() is refused afterwards
        until reset_accumulation()."""
        ap = np.ascontiguousarray(adaptive_default_params(self.L) if params is None else params); assert ap.dtype == ADAPTIVE_PARAMS_DTYPE
        st = np.zeros((), ADAPTIVE_STATS_DTYPE); fs = PtFrameStats()
        f = self.L.pt_render_adaptive; f.argtypes = [ctypes.c_void_p] * 4; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(ap), _p(st), ctypes.byref(fs)), "pt_render_adaptive")
        return {n: st[n].item() for n in ADAPTIVE_STATS_DTYPE.names}, fs.as_dict()

    def adaptive_state(self):
        """pt_get_adaptive_state: what the last render_adaptive left — counts [h, w] u32 and half [h, w, 4] f32 (the means of the even-indexed samples), full-frame maps
        with the pixels of other shards zero, and block_error [ceil(h / 8), ceil(w / 8)] f32, every block's error at its last evaluation"""
        h, w = self.height, self.width
        out = dict(counts=np.zeros((h, w), np.uint32), half=np.zeros((h, w, 4), np.float32), block_error=np.zeros(((h + 7) // 8, (w + 7) // 8), np.float32))
        f = self.L.pt_get_adaptive_state; f.argtypes = [ctypes.c_void_p] * 4; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(out["counts"]), _p(out["half"]), _p(out["block_error"])), "pt_get_adaptive_state")
        return out

    def adaptive_active(self):
        """pt_get_adaptive_active: the pixels still active after the last evaluation, packed x << 16 | y, in list order (u32)"""
        f = self.L.pt_get_adaptive_active; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]; f.restype = ctypes.c_int32
        n = f(self.h, None, 0)
        if n < 0: self._chk(-n, "pt_get_adaptive_active")
        out = np.zeros(n, np.uint32)
        if n:
            r = f(self.h, _p(out), n)
            if r < 0: self._chk(-r, "pt_get_adaptive_active")
        return out

    def _accum_denoise_params(self, params):
        dp = np.ascontiguousarray(accum_denoise_default_params(self.L) if params is None else params); assert dp.dtype == ACCUM_DENOISE_PARAMS_DTYPE
        return dp

    def accum_denoise(self, params=None, timed=False):
        """pt_accum_denoise: the dual-buffer non-local-means filter over what the last render_adaptive left (the radiance buffer and the even-sample means), into a picture
        of the context's own (ACCUM_DENOISE_PARAMS_DTYPE; defaults if None). Returns accum_denoised(), or with timed (accum_denoised, the two launches' event-timed
        milliseconds). Refused on a rank of a sharded layout."""
        dp = self._accum_denoise_params(params); ms = ctypes.c_float(0.0)
        f = self.L.pt_accum_denoise; f.argtypes = [ctypes.c_void_p] * 3; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(dp), ctypes.byref(ms) if timed else None), "pt_accum_denoise")
        return (self.accum_denoised(), float(ms.value)) if timed else self.accum_denoised()

    def accum_denoise_host_inputs(self, mean, half, params=None, timed=False):
        """pt_accum_denoise_host_inputs: accum_denoise()'s launches over two host pictures [h, w, 4] f32 (the mean of all samples, the mean of the even-indexed ones); neither
        the radiance buffer nor the adaptive state is touched, and only resize() is needed"""
        dp = self._accum_denoise_params(params); ms = ctypes.c_float(0.0)
        a = np.ascontiguousarray(mean, np.float32); hh = np.ascontiguousarray(half, np.float32)
        assert a.shape == hh.shape == (self.height, self.width, 4), (a.shape, hh.shape)
        f = self.L.pt_accum_denoise_host_inputs; f.argtypes = [ctypes.c_void_p] * 5; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(dp), _p(a), _p(hh), ctypes.byref(ms) if timed else None), "pt_accum_denoise_host_inputs")
        return (self.accum_denoised(), float(ms.value)) if timed else self.accum_denoised()

    def accum_denoised(self):
        """pt_get_accum_denoised: the denoised picture of the last accum_denoise / accum_denoise_host_inputs, [h, w, 4] f32"""
        return self._read_back("pt_get_accum_denoised", (self.width, self.height))

    def accum_denoised_device_buffer(self):
        """pt_accum_denoised_device_buffer: (device pointer, row pitch in bytes) of the denoised picture"""
        return self._device_buffer("pt_accum_denoised_device_buffer")

    def accum_denoise_state(self):
        """pt_get_accum_denoise_state: what the prepare launch of the last denoiser call left — odd [h, w, 3] f32 (the staged odd-sample means), variance [h, w, 3] f32 and
        valid [h, w] u8"""
        h, w = self.height, self.width
        out = dict(odd=np.zeros((h, w, 3), np.float32), variance=np.zeros((h, w, 3), np.float32), valid=np.zeros((h, w), np.uint8))
        f = self.L.pt_get_accum_denoise_state; f.argtypes = [ctypes.c_void_p] * 4; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(out["odd"]), _p(out["variance"]), _p(out["valid"])), "pt_get_accum_denoise_state")
        return out

    def tonemap_accum_denoised(self, params=None):
        """pt_tonemap_accum_denoised: tonemap() over the denoised picture instead of the radiance buffer -> (H, W, 4) uint8"""
        return self._tonemap("pt_tonemap_accum_denoised", params, (self.width, self.height))

    def average_luminance_accum_denoised(self):
        """pt_average_luminance_accum_denoised: average_luminance() of the denoised picture"""
        return self._average_luminance("pt_average_luminance_accum_denoised")

    def bloom_accum_denoised(self, params=None, timed=False):
        """pt_bloom_accum_denoised: bloom()'s pass with the denoised picture as the source; the result is bloomed()'s picture, which tonemap_bloomed() and
        average_luminance_bloomed() read. Returns bloomed(), or with timed (bloomed, the pass's event-timed milliseconds)"""
        bp = np.ascontiguousarray(bloom_default_params(self.L) if params is None else params); assert bp.dtype == BLOOM_PARAMS_DTYPE
        ms = ctypes.c_float(0.0)
        f = self.L.pt_bloom_accum_denoised; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int32
        self._chk(f(self.h, _p(bp), ctypes.byref(ms) if timed else None), "pt_bloom_accum_denoised")
        return (self.bloomed(), float(ms.value)) if timed else self.bloomed()

    def radiance(self):
        ptr = ctypes.POINTER(ctypes.c_float)()
        pitch = ctypes.c_size_t()
        self._chk(self.L.pt_map_radiance(self.h, ctypes.byref(ptr), ctypes.byref(pitch)), "pt_map_radiance")
        img = np.ctypeslib.as_array(ptr, shape=(self.height, self.width, 4)).copy()
        self.L.pt_unmap_radiance(self.h)
        return img

    def set_serial_kernels(self, enable):
        self._chk(self.L.pt_set_serial_kernels(self.h, 1 if enable else 0), "pt_set_serial_kernels")

    def set_tail_paths(self, max_paths):
        """pt_set_tail_paths: batches with at most this many live paths are finished by the tail kernel (0: never)."""
        self._chk(self.L.pt_set_tail_paths(self.h, int(max_paths)), "pt_set_tail_paths")

    def set_fused_traversal(self, mode):
        """pt_set_fused_traversal: 0 = visibility rays in launches of their own, 1 = in the next bounce's closest-hit launch (k_trace_pair), 2 = by the size of the call. Default 1.
        The same frames keep the live paths compacted by queue position (environment MI355PT_COMPACT_POOL=0 at pt_create: off), at five more uint4 arrays per path.
        A compacted batch starts without a generation launch: its first pass forms the vertex-0 state where it is used (environment MI355PT_FIRST_VERTEX_IN_PLACE=0 at pt_create:
        k_generate in front of every batch, as before). No image depends on either switch."""
        self._chk(self.L.pt_set_fused_traversal(self.h, int(mode)), "pt_set_fused_traversal")

    def tonemap(self, params=None):
        """pt_tonemap: the accumulation buffer through ToneMappingPass into sRGB RGBA8 -> (H, W, 4) uint8."""
        return self._tonemap("pt_tonemap", params, (self.width, self.height))

    # ---- multi-GPU shard plumbing (device pointers come from torch tensors)
    def average_luminance(self):
        """pt_average_luminance: the auto-exposure luminance capture (ToneMappingPasses.cpp:225-288) of the current accumulation buffer."""
        return self._average_luminance("pt_average_luminance")

    def shard_info(self):
        n, b = ctypes.c_uint32(), ctypes.c_size_t()
        self._chk(self.L.pt_shard_info(self.h, ctypes.byref(n), ctypes.byref(b)), "pt_shard_info")
        return n.value, b.value

    # ---- probes
    def comm_init(self, unique_id, rank, world):
        """pt_comm_init (collective): the RCCL communicator of the frame gather on this context's device."""
        _share_rccl_with_torch()
        buf = (ctypes.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.pt_comm_init(self.h, buf, rank, world), "pt_comm_init")

    def gather(self):
        """pt_gather (collective): every rank's tiles -> rank 0's accumulation buffer, on the library's stream."""
        self._chk(self.L.pt_gather(self.h), "pt_gather")

    def comm_destroy(self):
        self._chk(self.L.pt_comm_destroy(self.h), "pt_comm_destroy")

    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, np.float32)
        out = np.zeros((rays.shape[0], 4), np.float32)
        ms = ctypes.c_double()
        self._chk(self.L.pt_trace_closest(self.h, _p(rays), rays.shape[0], _p(out), ctypes.byref(ms)), "pt_trace_closest")
        return out, ms.value

    def trace_visibility(self, rays):
        rays = np.ascontiguousarray(rays, np.float32)
        out = np.zeros(rays.shape[0], np.uint32)
        ms = ctypes.c_double()
        self._chk(self.L.pt_trace_visibility(self.h, _p(rays), rays.shape[0], _p(out), ctypes.byref(ms)), "pt_trace_visibility")
        return out, ms.value

    def lights(self):
        n, npx, dim = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.L.pt_get_lights(self.h, ctypes.byref(n), ctypes.byref(npx), None, None, None, None, None, ctypes.byref(dim)), "pt_get_lights")
        lights = np.zeros((n.value, 8), np.uint32)
        ex = np.zeros((n.value, 4), np.uint32)
        pc = np.zeros(n.value, np.uint32)
        pi = np.zeros(npx.value, np.uint32)
        el = np.zeros(dim.value * dim.value, np.uint32)
        self._chk(self.L.pt_get_lights(self.h, None, None, _p(lights), _p(ex), _p(pc), _p(pi), _p(el), None), "pt_get_lights")
        return dict(lights=lights, lightsEx=ex, proxyCounters=pc, proxyIndices=pi, envLookup=el, envLookupDim=dim.value)

    def env_cube(self):
        """pt_get_env_cube: the baked RGBA16F environment cube as uint32 [texels, 2] plus (dim, mipLevels)."""
        n, dim, lv = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.L.pt_get_env_cube(self.h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(lv), None, 0), "pt_get_env_cube")
        out = np.zeros((n.value, 2), np.uint32)
        if n.value: self._chk(self.L.pt_get_env_cube(self.h, None, None, None, _p(out), n.value), "pt_get_env_cube")
        return out, dim.value, lv.value

    def update_texture(self, index, pixels):
        """pt_update_texture: new pixels for texture `index` of the scene — uint8 [h, w, 4] for the two 8-bit formats, float32 [h, w, 4] for PT_TEX_RGBA32F; the size and the
        format (sRGB or not: the texture's own) stay. With device_textures only that texture is converted again and the BVH stays."""
        sc = self._keep[0] if self._keep and isinstance(self._keep[0], dict) else {}
        if np.asarray(pixels).dtype == np.float32: fmt = PT_TEX_RGBA32F
        elif index < len(sc.get("textures", ())): fmt = sc["textures"][index][2]          # the format set_scene handed in
        else: fmt = PT_TEX_RGBA8_UNORM
        self.update_texture_desc(index, pixels, fmt)

    def update_texture_desc(self, index, pixels, fmt):
        """pt_update_texture with an explicit PtTextureDesc format."""
        px = np.ascontiguousarray(pixels); assert px.ndim == 3 and px.shape[2] == 4 and px.dtype in (np.uint8, np.float32)
        d = PtTextureDesc(px.shape[1], px.shape[0], int(fmt), px.ctypes.data)
        self.L.pt_update_texture.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; self.L.pt_update_texture.restype = ctypes.c_int32
        self._chk(self.L.pt_update_texture(self.h, int(index), ctypes.byref(d)), "pt_update_texture")

    def texture_level(self, index, mip):
        """pt_get_texture_level: the texels of one mip level as the kernels sample them, float32 [h, w, 4]."""
        f = self.L.pt_get_texture_level; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]; f.restype = ctypes.c_int32
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(f(self.h, int(index), int(mip), ctypes.byref(w), ctypes.byref(h), None, 0), "pt_get_texture_level")
        out = np.zeros((h.value, w.value, 4), np.float32)
        self._chk(f(self.h, int(index), int(mip), None, None, _p(out), w.value * h.value), "pt_get_texture_level")
        return out

    def alpha_plane(self, index):
        """pt_get_alpha_plane: (fmt, plane) — fmt 0: uint8 [texels], every opacity of level 0 is k / 255; fmt 1: float32 [texels]."""
        f = self.L.pt_get_alpha_plane; f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
        fmt, n = ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(f(self.h, int(index), ctypes.byref(fmt), None, 0, ctypes.byref(n)), "pt_get_alpha_plane")
        out = np.zeros(n.value, np.uint8)
        self._chk(f(self.h, int(index), None, _p(out), n.value, None), "pt_get_alpha_plane")
        return fmt.value, (out if fmt.value == 0 else out.view(np.float32))

    def texture_ingest_stats(self):
        """pt_get_texture_ingest_stats: what the last texture ingest or update did (PtTextureIngestStats as a dict)."""
        s = PtTextureIngestStats()
        self.L.pt_get_texture_ingest_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; self.L.pt_get_texture_ingest_stats.restype = ctypes.c_int32
        self._chk(self.L.pt_get_texture_ingest_stats(self.h, ctypes.byref(s)), "pt_get_texture_ingest_stats")
        return {n: getattr(s, n) for n, _ in PtTextureIngestStats._fields_ if not n.startswith("_")}

    def subinstances(self):
        n = ctypes.c_uint32()
        self._chk(self.L.pt_get_subinstances(self.h, ctypes.byref(n), None), "pt_get_subinstances")
        out = np.zeros((n.value, 8), np.uint32)
        self._chk(self.L.pt_get_subinstances(self.h, None, _p(out)), "pt_get_subinstances")
        return out

    def scene_info(self):
        a, b, c, d = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.L.pt_get_scene_info(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)), "pt_get_scene_info")
        return dict(triangles=a.value, bvhNodes=b.value, instances=c.value, materials=d.value)

    def build_stats(self):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._chk(self.L.pt_get_build_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "pt_get_build_stats")
        return dict(buildMs=a.value, refitMs=b.value, lightBakeMs=c.value)

    def bvh_info(self):
        """pt_get_bvh_info: which builder made the tree and where it ran."""
        class PtBvhInfo(ctypes.Structure):
            _fields_ = [("builder", ctypes.c_uint32), ("builtOnDevice", ctypes.c_uint32), ("numTriangles", ctypes.c_uint32), ("numWideNodes", ctypes.c_uint32),
                        ("collapseLevels", ctypes.c_uint32), ("optimiserPasses", ctypes.c_uint32), ("hostMs", ctypes.c_float), ("buildMs", ctypes.c_float)]
        o = PtBvhInfo()
        self._chk(self.L.pt_get_bvh_info(self.h, ctypes.byref(o)), "pt_get_bvh_info")
        names = {0: "PLOC", 1: "Karras radix tree", 2: "binned SAH + re-insertion (host)", 3: "PLOC + parallel re-insertion + cost-driven wide nodes"}
        d = {k: getattr(o, k) for k, _ in PtBvhInfo._fields_}
        d["builderName"] = names.get(o.builder, "?"); d["builtOn"] = "device" if o.builtOnDevice else "host"
        return d

    def probe(self, kind, inp, out_shape, out_dtype=np.float32):
        """pt_probe (include/mi355pt_testhooks.h): only on a PathTracer(test_hooks=True)"""
        if not self.test_hooks: raise RuntimeError("pt_probe is not part of the shipped library: PathTracer(test_hooks=True)")
        inp = np.ascontiguousarray(inp)
        out = np.zeros(out_shape, out_dtype)
        self._chk(self.L.pt_probe(self.h, kind, _p(inp), inp.nbytes, _p(out), out.nbytes, out_shape[0]), "pt_probe")
        return out

    def inert_terminal(self):
        """pt_get_inert_terminal (include/mi355pt_testhooks.h): (bits, dropped) — bits[p] = the two "inert when terminal" bits of global primitive p (1: cannot emit and is no
        light proxy, 2: thin surface) as the device built them, dropped = the terminating hits the last render() left unshaded. Only on a PathTracer(test_hooks=True)."""
        if not self.test_hooks: raise RuntimeError("pt_get_inert_terminal is not part of the shipped library: PathTracer(test_hooks=True)")
        n, dropped = ctypes.c_uint32(), ctypes.c_uint64()
        self.L.pt_get_inert_terminal.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        self._chk(self.L.pt_get_inert_terminal(self.h, ctypes.byref(n), None, 0, ctypes.byref(dropped)), "pt_get_inert_terminal")
        words = np.zeros((n.value + 15) // 16, np.uint32)
        if n.value: self._chk(self.L.pt_get_inert_terminal(self.h, None, _p(words), words.size, None), "pt_get_inert_terminal")
        prim = np.arange(n.value, dtype=np.uint32)
        return ((words[prim // 16] >> (2 * (prim % 16))) & 3).astype(np.uint32), int(dropped.value)

    ROUTES = {"extend": 0, "extend_ranged": 1, "shadow": 2, "packets": 3}

    def trace_route(self, route, rays, task_cap=0, max_blocks=0, step_cap=0, stack_bound=0):
        """pt_trace_route (include/mi355pt_testhooks.h): rays [n, 8] (origin | tmin | direction | tmax) through the traversal launches a frame runs. route: "extend",
        "extend_ranged", "packets" (-> hit records [n, 4] float32: t | primitive bits | u | v) or "shadow" (-> [n] uint32, 1 = visible), or the route's number. The options: 0
        is the product's value. Returns (out, stats): stats = dict of split (rays cut into sub-trees), tasks (sub-trees fed to each of the four task rounds), packet_rays,
        leftover_rays, overflow. An error of the call is raised as PtError with the stats of the launches, where they ran, in its .stats. Only on a PathTracer(test_hooks=True)."""
        if not self.test_hooks: raise RuntimeError("pt_trace_route is not part of the shipped library: PathTracer(test_hooks=True)")
        route = self.ROUTES.get(route, route)
        rays = np.ascontiguousarray(rays, np.float32); n = rays.shape[0]
        out = np.zeros(n, np.uint32) if route == 2 else np.zeros((n, 4), np.float32)
        opt = np.array([task_cap, max_blocks, step_cap, stack_bound], np.uint32); st = np.full(8, 0xFFFFFFFF, np.uint32)
        f = self.L.pt_trace_route; f.restype = ctypes.c_int32
        f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        r = f(self.h, int(route), _p(rays), n, _p(opt), _p(out), _p(st))
        stats = None if (st == 0xFFFFFFFF).all() else dict(split=int(st[0]), tasks=[int(x) for x in st[1:5]], packet_rays=int(st[5]), leftover_rays=int(st[6]), overflow=int(st[7]))
        try:
            self._chk(r, "pt_trace_route")
        except PtError as e:
            e.stats = stats; raise
        return out, stats

    def get_bvh8(self, short_by=0):
        """pt_get_bvh8 (include/mi355pt_testhooks.h): the wide tree as the traversal reads it — dict of nodes [numNodes8, 32] uint32 (the 128-byte Bvh8Node records), tris
        [numTris, 12] uint32 (the 48-byte leaf-order TriRecords, stored pad included), bounds [6] float32 (scene min xyz, max xyz), levels (collapseLevels) and level_start
        [min(levels, 64) + 1] uint32. short_by: hand the node buffer over with that many records less than it needs (the refusal's test). Only on a PathTracer(test_hooks=True)."""
        if not self.test_hooks: raise RuntimeError("pt_get_bvh8 is not part of the shipped library: PathTracer(test_hooks=True)")
        f = self.L.pt_get_bvh8; f.restype = ctypes.c_int32
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        nn, nt, nl = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(f(self.h, ctypes.byref(nn), None, 0, ctypes.byref(nt), None, 0, None, ctypes.byref(nl), None, 0), "pt_get_bvh8")
        nodes = np.zeros((nn.value, 32), np.uint32); tris = np.zeros((nt.value, 12), np.uint32)
        bounds = np.zeros(6, np.float32); start = np.zeros(min(nl.value, 64) + 1, np.uint32)
        self._chk(f(self.h, None, _p(nodes) if nodes.size else None, max(nn.value - short_by, 0), None, _p(tris) if tris.size else None, nt.value, _p(bounds), None, _p(start), start.size), "pt_get_bvh8")
        return dict(nodes=nodes, tris=tris, bounds=bounds, levels=int(nl.value), level_start=start)
