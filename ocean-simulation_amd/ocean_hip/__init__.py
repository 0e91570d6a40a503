"""ocean_hip -- Python host mirror of the reference's WaterBody / IFFT interface
over liboceanhip.so (the MI355X C ABI declared in include/ocean/ocean.h).

The reference's host side is C# (Unity MonoBehaviours); no C# toolchain exists
in this image, so the host layer that the tests and the bench drive is this
ctypes binding, shaped like the reference:

    WaterBody  (Assets/Scripts/Water/WaterBody.cs)  -- fields, Awake(),
               CalculateWavesTexturesAtTime(t), Update(t), GetWaterHeight(pos)
    IFFT       (Assets/Scripts/Water/IFFT.cs)       -- InverseFastFourierTransform(plane)
    WaterCascade (Assets/Scripts/Water/WaterCascade.cs)

A compile-ready C# P/Invoke facade of the same ABI lives in ../csharp/ and in
INTEGRATION.md.  There is no CPU fallback: if the HIP library cannot be loaded
(or no GPU is present) every compute call raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

# torch is only plumbing here (device count, torch.distributed in bench.py), but
# its bundled HIP runtime must be the one this library binds to: import it first
# so that libamdhip64.so.7 resolves to the already-loaded copy (one runtime per
# process).
try:  # pragma: no cover - import side effect only
    import torch as _torch  # noqa: F401
except Exception:  # torch absent: the library then binds to /opt/rocm's runtime
    _torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCEAN_HIP_LIB") or os.path.join(_HERE, "liboceanhip.so")

OK = 0
E_INVALID_ARG = -1
E_UNSUPPORTED = -2
E_STATE = -3
E_DEVICE = -4
E_OUT_OF_MEMORY = -5

F_DISPLACEMENT_ONLY = 0x1
F_NORMALS = 0x2
F_UNFUSED = 0x4
F_MIPS = 0x8
F_VELOCITY = 0x10

TEX_NOISE, TEX_H0, TEX_WAVES = 0, 1, 2
TEX_PLANE0, TEX_PLANE1, TEX_PLANE2, TEX_PLANE3 = 3, 4, 5, 6
TEX_DISP, TEX_DERIV, TEX_TURB, TEX_NORMAL = 7, 8, 9, 10
TEX_VELOCITY = 11
_TEX_CHANNELS = {TEX_NOISE: 2, TEX_H0: 4, TEX_WAVES: 4, TEX_PLANE0: 2, TEX_PLANE1: 2, TEX_PLANE2: 2,
                 TEX_PLANE3: 2, TEX_DISP: 4, TEX_DERIV: 4, TEX_TURB: 4, TEX_NORMAL: 4, TEX_VELOCITY: 4}

# symbols declared in include/ocean/ocean.h
EXPORTED_SYMBOLS = (
    "ocean_create", "ocean_destroy", "ocean_set_params", "ocean_set_noise", "ocean_generate_noise",
    "ocean_init_spectrum", "ocean_step", "ocean_evolve", "ocean_ifft2d", "ocean_fill", "ocean_read",
    "ocean_write", "ocean_get_device_ptr", "ocean_get_stream", "ocean_synchronize",
    "ocean_set_kernel_timing", "ocean_kernel_stats", "ocean_step_bytes", "ocean_read_mip", "ocean_get_mip_ptr",
    "ocean_generate_noise_device", "ocean_read_async", "ocean_readback_status", "ocean_readback_wait", "ocean_readback_release",
    "ocean_readback_copy_ms", "ocean_read_height_async", "ocean_set_readback_timing",
    "ocean_host_alloc", "ocean_host_free", "ocean_last_error", "ocean_abi_version", "ocean_set_column_band",
    "ocean_reset_foam", "ocean_sample_world", "ocean_sample_world_device", "ocean_kernel_name",
    "ocean_set_column_parity", "ocean_query_surface", "ocean_query_surface_device", "ocean_query_surface_async",
    "ocean_surface_grid", "ocean_surface_grid_device", "ocean_surface_grid_async",
    "ocean_body_buoyancy", "ocean_body_buoyancy_device", "ocean_body_buoyancy_async",
    "ocean_query_velocity", "ocean_query_velocity_device", "ocean_query_velocity_async",
    "ocean_surface_bounds", "ocean_surface_bounds_device",
    "ocean_raycast", "ocean_raycast_device", "ocean_raycast_async",
    "ocean_body_dynamics", "ocean_body_dynamics_device", "ocean_body_dynamics_async",
    "ocean_whitecaps", "ocean_whitecaps_device", "ocean_whitecaps_async",
    "ocean_camera", "ocean_camera_device", "ocean_camera_async",
    "ocean_body_step", "ocean_body_step_device", "ocean_body_step_async",
    "ocean_atmosphere", "ocean_sky_update", "ocean_atmosphere_read", "ocean_atmosphere_lut", "ocean_sun_color",
    "ocean_spray_step", "ocean_spray_step_device", "ocean_spray_step_async",
    "ocean_camera_bodies", "ocean_camera_bodies_device", "ocean_camera_bodies_async",
    "ocean_camera_scene", "ocean_camera_scene_device", "ocean_camera_scene_async",
    "ocean_body_hydrostatics", "ocean_body_hydrostatics_device", "ocean_body_hydrostatics_async",
)

# ocean_query_surface* modes and limits (ocean.h)
QUERY_REFERENCE, QUERY_SURFACE = 0, 1
QUERY_MAX_POINTS = 65536
# ocean_surface_grid* modes and limits (ocean.h)
GRID_VERTICES, GRID_SURFACE, GRID_HEIGHTFIELD = 0, 1, 2
GRID_MAX_NODES = 1 << 22
# ocean_body_buoyancy* limits (ocean.h); the modes are the queries'
BODY_MAX_BODIES = 8192
BODY_MAX_PROBES = 4096
BODY_MAX_SAMPLES = 1 << 22
# ocean_body_dynamics* drag laws (ocean.h); modes and limits are the bodies'
DRAG_LINEAR, DRAG_QUADRATIC = 0, 1
# ocean_raycast* statuses and limits (ocean.h)
RAY_MISS, RAY_HIT, RAY_SUBMERGED = 0, 1, 2
RAY_MAX_RAYS = 16384
RAY_MAX_STEPS = 1024
RAY_MAX_SAMPLES = 1 << 24
# ocean_whitecaps* limit (ocean.h): records of a list, the header not counted
WHITECAP_MAX_RECORDS = 65535
# ocean_camera* modes, array sizes and limits (ocean.h)
CAMERA_HITS, CAMERA_RANGE, CAMERA_COLOR = 0, 1, 2
CAMERA_FLOATS = 14
CAMERA_MATERIAL_FLOATS = 32
CAMERA_MAX_PIXELS = 1 << 22
CAMERA_MAX_SAMPLES = 1 << 28
# the colour image with the atmosphere's sky: valid only as CAMERA_COLOR | CAMERA_SKY_LUT (ocean.h, "The atmosphere")
CAMERA_SKY_LUT = 16
# ocean_atmosphere*: the params array, the tables' ids, default sizes and the size limit (ocean.h)
ATMOSPHERE_FLOATS = 32
ATMOSPHERE_MAX_DIM = 1024
LUT_TRANSMITTANCE, LUT_MULTISCATTER, LUT_SKYVIEW = 0, 1, 2
ATMOSPHERE_DEFAULT_DIMS = (64, 256, 64, 64, 256, 128)
# ocean_body_step* array size and limits (ocean.h); modes, laws and the body limits are the dynamics'
BODY_STEP_FLOATS = 8
BODY_MAX_SUBSTEPS = 64
BODY_STEP_MAX_SAMPLES = 1 << 24
# ocean_spray_step* array size and limits (ocean.h): the device form's particles, and those of the host and async
# forms, which stage pool and list
SPRAY_FLOATS = 16
SPRAY_MAX_PARTICLES = (1 << 20) - 1
SPRAY_MAX_STAGED = 65535
SPRAY_MAX_SUBSTEPS = 64
# ocean_camera_bodies*: the status of a body pixel, the paint's size and the limits of a record's stride (ocean.h); the
# modes and limits are the camera's, the body limit the bodies'
RAY_BODY = 3
BODY_PAINT_FLOATS = 4
BODY_STRIDE_MIN, BODY_STRIDE_MAX = 10, 64
# ocean_camera_scene*: its own mode (the record of every pixel's shadow, through-water and reflection links) and the
# size of its optics array (ocean.h)
CAMERA_LINKS = 3
SCENE_OPTICS_FLOATS = 6
# ocean_body_hydrostatics*: the mesh's limits and the record's size (ocean.h); the body limits are the bodies'
HULL_MAX_VERTICES = 2048
HULL_MAX_TRIANGLES = 4096
HULL_RECORD_FLOATS = 16


class OceanError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where} failed ({code}): {msg}")
        self.code = code


class ocean_params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in
                ("wind_speed", "wind_dir_x", "wind_dir_y", "gravity", "fetch", "depth")]


class ocean_cascade(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("wavelength", "cutoff_low", "cutoff_high", "swell", "fade")]


_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load liboceanhip.so (raises if it was not built -- there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OceanError(E_DEVICE, "load_library",
                         f"{path} not found: build it with `make -C ocean-simulation_amd` "
                         "(or __graft_entry__.build())")
    L = ctypes.CDLL(path)
    P = ctypes.c_void_p
    i, u32, u64, f, sz = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_size_t
    sig = {
        "ocean_create": ([i, i, i, i, u32, ctypes.POINTER(P)], i),
        "ocean_destroy": ([P], None),
        "ocean_set_params": ([P, ctypes.POINTER(ocean_params), ctypes.POINTER(ocean_cascade)], i),
        "ocean_set_noise": ([P, i, P], i),
        "ocean_generate_noise": ([P, u64], i),
        "ocean_init_spectrum": ([P], i),
        "ocean_reset_foam": ([P], i),
        "ocean_sample_world": ([P, i, P, i, P], i),
        "ocean_sample_world_device": ([P, i, P, i, P], i),
        "ocean_step": ([P, f], i),
        "ocean_evolve": ([P, f], i),
        "ocean_ifft2d": ([P, i], i),
        "ocean_fill": ([P], i),
        "ocean_read": ([P, i, i, i, P, sz], i),
        "ocean_write": ([P, i, i, i, P, sz], i),
        "ocean_get_device_ptr": ([P, i, ctypes.POINTER(P), ctypes.POINTER(sz)], i),
        "ocean_get_stream": ([P, ctypes.POINTER(P)], i),
        "ocean_synchronize": ([P], i),
        "ocean_set_kernel_timing": ([P, i], i),
        "ocean_kernel_stats": ([P, i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)], i),
        "ocean_kernel_name": ([P, i, ctypes.c_char_p, sz], i),
        "ocean_step_bytes": ([P, ctypes.POINTER(u64), ctypes.POINTER(u64)], i),
        "ocean_read_mip": ([P, i, i, i, i, P, sz], i),
        "ocean_generate_noise_device": ([P, u64], i),
        "ocean_get_mip_ptr": ([P, i, i, ctypes.POINTER(P), ctypes.POINTER(sz)], i),
        "ocean_read_async": ([P, i, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_readback_status": ([P], i),
        "ocean_readback_wait": ([P], i),
        "ocean_readback_release": ([P], None),
        "ocean_readback_copy_ms": ([P, ctypes.POINTER(f)], i),
        "ocean_read_height_async": ([P, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_set_readback_timing": ([P, i], i),
        "ocean_host_alloc": ([sz, ctypes.POINTER(P)], i),
        "ocean_host_free": ([P], None),
        "ocean_last_error": ([], ctypes.c_char_p),
        "ocean_abi_version": ([], i),
        "ocean_set_column_band": ([P, i, i], i),
        "ocean_set_column_parity": ([P, i], i),
        "ocean_query_surface": ([P, i, i, i, P, i, P], i),
        "ocean_query_surface_device": ([P, i, i, i, P, i, P], i),
        "ocean_query_surface_async": ([P, i, i, i, P, i, P, ctypes.POINTER(P)], i),
        "ocean_surface_grid": ([P, i, i, i, f, f, f, f, f, i, i, P, sz], i),
        "ocean_surface_grid_device": ([P, i, i, i, f, f, f, f, f, i, i, P, sz], i),
        "ocean_surface_grid_async": ([P, i, i, i, f, f, f, f, f, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_body_buoyancy": ([P, i, i, i, P, i, P, i, P], i),
        "ocean_body_buoyancy_device": ([P, i, i, i, P, i, P, i, P], i),
        "ocean_body_buoyancy_async": ([P, i, i, i, P, i, P, i, P, ctypes.POINTER(P)], i),
        "ocean_query_velocity": ([P, i, i, P, i, P], i),
        "ocean_query_velocity_device": ([P, i, i, P, i, P], i),
        "ocean_query_velocity_async": ([P, i, i, P, i, P, ctypes.POINTER(P)], i),
        "ocean_surface_bounds": ([P, i, P, sz], i),
        "ocean_surface_bounds_device": ([P, i, P, sz], i),
        "ocean_raycast": ([P, i, i, i, i, P, i, P], i),
        "ocean_raycast_device": ([P, i, i, i, i, P, i, P], i),
        "ocean_raycast_async": ([P, i, i, i, i, P, i, P, ctypes.POINTER(P)], i),
        "ocean_body_dynamics": ([P, i, i, i, i, P, i, P, P, i, P], i),
        "ocean_body_dynamics_device": ([P, i, i, i, i, P, i, P, P, i, P], i),
        "ocean_body_dynamics_async": ([P, i, i, i, i, P, i, P, P, i, P, ctypes.POINTER(P)], i),
        "ocean_whitecaps": ([P, i, f, f, f, f, f, f, i, i, i, P, sz], i),
        "ocean_whitecaps_device": ([P, i, f, f, f, f, f, f, i, i, i, P, sz], i),
        "ocean_whitecaps_async": ([P, i, f, f, f, f, f, f, i, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_camera": ([P, i, i, i, i, i, P, P, i, i, P, sz], i),
        "ocean_camera_device": ([P, i, i, i, i, i, P, P, i, i, P, sz], i),
        "ocean_camera_async": ([P, i, i, i, i, i, P, P, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_body_step": ([P, i, i, i, i, i, P, P, i, P, P, i, P], i),
        "ocean_body_step_device": ([P, i, i, i, i, i, P, P, i, P, P, i, P], i),
        "ocean_body_step_async": ([P, i, i, i, i, i, P, P, i, P, P, i, P, ctypes.POINTER(P)], i),
        "ocean_atmosphere": ([P, P, i, i, i, i, i, i], i),
        "ocean_sky_update": ([P, P], i),
        "ocean_atmosphere_read": ([P, i, P, sz], i),
        "ocean_atmosphere_lut": ([P, i, ctypes.POINTER(P), ctypes.POINTER(sz), ctypes.POINTER(sz)], i),
        "ocean_sun_color": ([P, P, P], i),
        "ocean_spray_step": ([P, i, i, i, P, P, i, P, i, P, sz], i),
        "ocean_spray_step_device": ([P, i, i, i, P, P, i, P, i, P, sz], i),
        "ocean_spray_step_async": ([P, i, i, i, P, P, i, P, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_camera_bodies": ([P, i, i, i, i, i, P, P, i, i, P, P, P, i, i, P, sz], i),
        "ocean_camera_bodies_device": ([P, i, i, i, i, i, P, P, i, i, P, P, P, i, i, P, sz], i),
        "ocean_camera_bodies_async": ([P, i, i, i, i, i, P, P, i, i, P, P, P, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_camera_scene": ([P, i, i, i, i, i, P, P, i, i, P, P, P, P, i, i, P, sz], i),
        "ocean_camera_scene_device": ([P, i, i, i, i, i, P, P, i, i, P, P, P, P, i, i, P, sz], i),
        "ocean_camera_scene_async": ([P, i, i, i, i, i, P, P, i, i, P, P, P, P, i, i, P, sz, ctypes.POINTER(P)], i),
        "ocean_body_hydrostatics": ([P, i, i, P, i, P, i, P, i, P], i),
        "ocean_body_hydrostatics_device": ([P, i, i, P, i, P, i, P, i, P], i),
        "ocean_body_hydrostatics_async": ([P, i, i, P, i, P, i, P, i, P, ctypes.POINTER(P)], i),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _check(rc: int, where: str) -> None:
    if rc != OK:
        msg = load_library().ocean_last_error().decode(errors="replace")
        raise OceanError(rc, where, msg)


def look_at_camera(eye, target, up, fov_y: float, width: int, height: int, t0: float, t1: float) -> np.ndarray:
    """The float32[14] camera of ocean_camera (ocean.h) for a pinhole at `eye` looking at `target`: pixel (i, j) looks
    through the centre of its cell of an image plane one unit ahead, `fov_y` radians tall, row 0 at the top, column
    0 at the left (right = forward x up).  Every ray searches [t0, t1].  Computed in float64 and rounded once."""
    e, t, u = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = t - e
    fwd = fwd / np.sqrt((fwd * fwd).sum())
    right = np.cross(fwd, u)
    right = right / np.sqrt((right * right).sum())
    top = np.cross(right, fwd)
    step = 2.0 * np.tan(0.5 * float(fov_y)) / int(height)  # a pixel's side on the image plane: square pixels
    du, dv = right * step, -top * step
    d00 = fwd + du * (0.5 - 0.5 * int(width)) + dv * (0.5 - 0.5 * int(height))
    return np.concatenate([e, d00, du, dv, [float(t0), float(t1)]]).astype(np.float32)


def material(color=(0.02, 0.1, 0.16), roughness: float = 0.3, ex: float = 0.25, ey: float = 0.25,
             environment_strength: float = 1.0, sun_strength: float = 1.0, subsurface_intensity: float = 0.5,
             subsurface_color=(0.0, 0.6, 0.5), foam_color=(1.0, 1.0, 1.0), foam_threshold: float = 0.5,
             foam_blending: float = 0.5, light_direction=(0.3, 0.5, 0.4), light_color=(1.0, 0.96, 0.9),
             horizon_color=(0.75, 0.82, 0.9), zenith_color=(0.2, 0.4, 0.8), lod_slope: float = 0.0) -> np.ndarray:
    """The float32[32] material of ocean_camera's colour mode (ocean.h names the fields; the arguments are
    Water.shader's properties, a light and a two-colour sky).  Computed in float64 and rounded once: R0 of air over
    water, the Fresnel exponent 5 exp(-2.69 roughness) and divisor 1 + 22.7 roughness^1.5, the subsurface colour
    times its intensity, and the direction towards the light normalised."""
    light = np.asarray(light_direction, np.float64)
    light = light / np.sqrt((light * light).sum())
    r = float(roughness)
    m = np.zeros(CAMERA_MATERIAL_FLOATS, np.float64)
    m[0:3] = color
    m[3] = ((1.0 - 1.333) / (1.0 + 1.333)) ** 2
    m[4] = 5.0 * np.exp(-2.69 * r)
    m[5] = 1.0 + 22.7 * r ** 1.5
    m[6], m[7], m[8], m[9] = r, lod_slope, ex, ey
    m[10], m[11] = environment_strength, sun_strength
    m[12:15] = np.asarray(subsurface_color, np.float64) * float(subsurface_intensity)
    m[15] = foam_threshold
    m[16:19] = foam_color
    m[19] = foam_blending
    m[20:23] = light
    m[23:26] = light_color
    m[26:29] = horizon_color
    m[29:32] = zenith_color
    return m.astype(np.float32)


_material = material  # (WaterBody.Camera has a parameter of that name)


def atmosphere_params(planet_radius: float = 6360000.0, atmosphere_radius: float = 6420000.0,
                      rayleigh_scattering=(5.802e-6, 13.558e-6, 6.5e-5), rayleigh_absorption=(0.0, 0.0, 0.0),
                      rayleigh_scale_height: float = 8000.0, mie_scattering=(3.996e-6, 3.996e-6, 3.996e-6),
                      mie_absorption=(4.4e-6, 4.4e-6, 4.4e-6), mie_scale_height: float = 1200.0, g: float = 0.85,
                      ozone_scattering=(0.0, 0.0, 0.0), ozone_absorption=(0.65e-6, 1.881e-6, 0.085e-6),
                      ground_albedo=(0.0, 0.0, 0.0), sun_size: float = 0.04) -> np.ndarray:
    """The float32[32] `params` of ocean_atmosphere (ocean.h names the fields): AtmosphereController's public fields
    with its defaults, and Atmosphere.shader's _SunSize.  Rounded once; [27..31] are reserved and zero."""
    p = np.zeros(ATMOSPHERE_FLOATS, np.float64)
    p[0], p[1] = planet_radius, atmosphere_radius
    p[2:5], p[5:8], p[8] = rayleigh_scattering, rayleigh_absorption, rayleigh_scale_height
    p[9:12], p[12:15], p[15], p[16] = mie_scattering, mie_absorption, mie_scale_height, g
    p[17:20], p[20:23], p[23:26], p[26] = ozone_scattering, ozone_absorption, ground_albedo, sun_size
    return p.astype(np.float32)


def optics(shadow_color=(0.0, 0.0, 0.0), shadow_intensity: float = 0.5, fog_density: float = 0.2,
           reach: float = 100.0) -> np.ndarray:
    """The float32[6] `optics` of ocean_camera_scene (ocean.h) = (SH.r, SH.g, SH.b, SI, WF, reach): Water.shader's
    _ShadowsColor, _ShadowsIntensity and _WaterFogDensity, and the length in metres that the shadow ray and the mirror
    ray search for a body.  Rounded once."""
    return np.array([*shadow_color, shadow_intensity, fog_density, reach], np.float32)


def step_params(h: float, g: float = 9.81, buoyancy: Optional[float] = None, drag: float = 0.0, drag_torque: float = 0.0,
                linear_damping: float = 0.0, angular_damping: float = 0.0, density: float = 1.0) -> np.ndarray:
    """The float32[8] `step` of ocean_body_step (ocean.h) = (h, g, B, kd, kt, la, aa, 0): the substep in seconds,
    gravity's magnitude, the buoyant force per unit of submerged volume (`buoyancy`, by default g * density, the
    reference's BuoyantObject), the coefficients of the drag force and torque against the water's velocity, and the
    reference's `drag` and `angularDrag` (damping against still water while a probe is wet).  Rounded once."""
    b = float(g) * float(density) if buoyancy is None else float(buoyancy)
    return np.array([h, g, b, drag, drag_torque, linear_damping, angular_damping, 0.0], np.float32)


class OceanContext:
    """Thin owner of one ocean_ctx (one device, T tiles x C cascades at N x N)."""

    def __init__(self, n: int, n_cascades: int, n_tiles: int = 1, flags: int = 0, device: int = 0):
        self.lib = load_library()
        self.n, self.C, self.T, self.flags, self.device = n, n_cascades, n_tiles, flags, device
        self.planes = 2 if flags & F_DISPLACEMENT_ONLY else 4
        h = ctypes.c_void_p()
        _check(self.lib.ocean_create(device, n, n_cascades, n_tiles, flags, ctypes.byref(h)), "ocean_create")
        self._h = h

    # -- lifetime -----------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ocean_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- configuration --------------------------------------------------------
    def set_params(self, params: dict, cascades: Sequence[dict]) -> None:
        if len(cascades) != self.C:
            raise ValueError(f"expected {self.C} cascades, got {len(cascades)}")
        p = ocean_params(params["wind_speed"], params["wind_dir_x"], params["wind_dir_y"], params["gravity"],
                         params["fetch"], params["depth"])
        cs = (ocean_cascade * self.C)(*[ocean_cascade(c["wavelength"], c["cutoff_low"], c["cutoff_high"],
                                                      c["swell"], c["fade"]) for c in cascades])
        _check(self.lib.ocean_set_params(self._h, ctypes.byref(p), cs), "ocean_set_params")

    def set_noise(self, tile: int, rg: np.ndarray) -> None:
        a = np.ascontiguousarray(rg, np.float32)
        if a.shape != (self.n, self.n, 2):
            raise ValueError(f"noise must be float32[{self.n}][{self.n}][2], got {a.shape}")
        _check(self.lib.ocean_set_noise(self._h, tile, a.ctypes.data), "ocean_set_noise")

    def generate_noise(self, seed: int) -> None:
        _check(self.lib.ocean_generate_noise(self._h, ctypes.c_uint64(seed)), "ocean_generate_noise")

    # -- compute --------------------------------------------------------------
    def generate_noise_device(self, seed: int) -> None:
        """Counter-based noise generated on the GPU for every tile (ocean.h)."""
        _check(self.lib.ocean_generate_noise_device(self._h, seed), "ocean_generate_noise_device")

    def init_spectrum(self) -> None:
        _check(self.lib.ocean_init_spectrum(self._h), "ocean_init_spectrum")

    def reset_foam(self) -> None:
        _check(self.lib.ocean_reset_foam(self._h), "ocean_reset_foam")

    def step(self, t: float) -> None:
        _check(self.lib.ocean_step(self._h, ctypes.c_float(t)), "ocean_step")

    def evolve(self, t: float) -> None:
        _check(self.lib.ocean_evolve(self._h, ctypes.c_float(t)), "ocean_evolve")

    def ifft2d(self, plane_mask: int) -> None:
        _check(self.lib.ocean_ifft2d(self._h, plane_mask), "ocean_ifft2d")

    def fill(self) -> None:
        _check(self.lib.ocean_fill(self._h), "ocean_fill")

    def synchronize(self) -> None:
        _check(self.lib.ocean_synchronize(self._h), "ocean_synchronize")

    # -- textures -------------------------------------------------------------
    def read(self, tex: int, tile: int = 0, cascade: int = 0) -> np.ndarray:
        ch = _TEX_CHANNELS[tex]
        out = np.empty((self.n, self.n, ch), np.float32)
        _check(self.lib.ocean_read(self._h, tex, tile, cascade, out.ctypes.data, out.nbytes), "ocean_read")
        return out

    def read_all(self, tex: int, tile: int = 0) -> np.ndarray:
        return np.stack([self.read(tex, tile, c) for c in range(self.C)])

    def write(self, tex: int, data: np.ndarray, tile: int = 0, cascade: int = 0) -> None:
        a = np.ascontiguousarray(data, np.float32)
        _check(self.lib.ocean_write(self._h, tex, tile, cascade, a.ctypes.data, a.nbytes), "ocean_write")

    def read_mip(self, tex: int, level: int, tile: int = 0, cascade: int = 0) -> np.ndarray:
        """Level `level` of DERIV / TURB's mip chain (OCEAN_F_MIPS); level 0 = read()."""
        m = self.n >> level
        out = np.empty((m, m, 4), np.float32)
        _check(self.lib.ocean_read_mip(self._h, tex, tile, cascade, level, out.ctypes.data, out.nbytes),
               "ocean_read_mip")
        return out

    def mip_ptr(self, tex: int, level: int):
        """(device pointer of level `level` of slice 0, bytes between slices' chains)."""
        p, st = ctypes.c_void_p(), ctypes.c_size_t()
        _check(self.lib.ocean_get_mip_ptr(self._h, tex, level, ctypes.byref(p), ctypes.byref(st)), "ocean_get_mip_ptr")
        return p.value, st.value

    def sample_world(self, points: np.ndarray, tile: int = 0) -> np.ndarray:
        """Cascade-summed world sampling (Water.shader:314-348; ocean.h ocean_sample_world):
        points float[M][3] = (world x, world z, lod) -> float32[M][3][4]: (Dx, Dy, Dz,
        turbulence), (Dyx, Dyz, Dxx, Dzz), (normal x, y, z, 0)."""
        p = np.ascontiguousarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"points must be float32[M][3], got {p.shape}")
        out = np.empty((p.shape[0], 3, 4), np.float32)
        _check(self.lib.ocean_sample_world(self._h, tile, p.ctypes.data, p.shape[0], out.ctypes.data),
               "ocean_sample_world")
        return out

    @staticmethod
    def _query_points(points) -> np.ndarray:
        p = np.ascontiguousarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"points must be float32[M][2] = (world x, world z), got {p.shape}")
        return p

    def query_surface(self, points, tile: int = 0, mode: int = QUERY_SURFACE, iterations: int = 4) -> np.ndarray:
        """Surface queries on the device (ocean.h ocean_query_surface), blocking: points float[M][2] =
        (world x, world z) -> float32[M][8].  QUERY_SURFACE: (height of the surface above the point,
        p.x, p.z, residual, normal x, y, z, foam) after `iterations` fixed-point steps of p + D_xz(p) = q;
        QUERY_REFERENCE (iterations 0): (GetWaterHeight's texel .y, px, py, 0, 0, 0, 0, 0)."""
        p = self._query_points(points)
        out = np.empty((p.shape[0], 8), np.float32)
        _check(self.lib.ocean_query_surface(self._h, tile, mode, iterations, p.ctypes.data, p.shape[0],
                                            out.ctypes.data), "ocean_query_surface")
        return out

    def query_surface_async(self, points, tile: int = 0, mode: int = QUERY_SURFACE, iterations: int = 4,
                            buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_query_surface_async): the query runs behind the queued steps and its
        float32[M][8] lands in pinned host memory like a read_async slice; `points` is consumed by the call.
        Poll .done() / .wait(), then .data; `buf`: a caller-owned pinned slot of at least M x 32 B."""
        p = self._query_points(points)
        return Readback(self, (p.shape[0], 8), p.shape[0] * 32, "ocean_query_surface_async",
                        lambda dst, req: self.lib.ocean_query_surface_async(self._h, tile, mode, iterations, p.ctypes.data,
                                                                            p.shape[0], dst, req), buf)

    def query_velocity(self, points, tile: int = 0, iterations: int = 4) -> np.ndarray:
        """Surface velocity on the device (ocean.h ocean_query_velocity; F_VELOCITY contexts), blocking: points
        float[M][2] = (world x, world z) -> float32[M][8]: (velocity x, y, z of the water particle on the
        surface above the point, residual, height, p.x, p.z, dDxz/dt) after `iterations` fixed-point steps,
        the same as query_surface's."""
        p = self._query_points(points)
        out = np.empty((p.shape[0], 8), np.float32)
        _check(self.lib.ocean_query_velocity(self._h, tile, iterations, p.ctypes.data, p.shape[0], out.ctypes.data),
               "ocean_query_velocity")
        return out

    def query_velocity_async(self, points, tile: int = 0, iterations: int = 4, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_query_velocity_async), as query_surface_async: the query runs behind the
        queued steps and its float32[M][8] lands in pinned host memory; `points` is consumed by the call."""
        p = self._query_points(points)
        return Readback(self, (p.shape[0], 8), p.shape[0] * 32, "ocean_query_velocity_async",
                        lambda dst, req: self.lib.ocean_query_velocity_async(self._h, tile, iterations, p.ctypes.data,
                                                                             p.shape[0], dst, req), buf)

    def query_velocity_device(self, points_ptr: int, count: int, out_ptr: int, tile: int = 0, iterations: int = 4) -> None:
        """The device-pointer form (ocean_query_velocity_device): points float[count][2] and out float[count][8]
        live on this context's device (points 4-B, out 16-B aligned); async on the context's stream, after
        the queued steps."""
        vp = ctypes.c_void_p
        _check(self.lib.ocean_query_velocity_device(self._h, tile, iterations, vp(points_ptr), count, vp(out_ptr)),
               "ocean_query_velocity_device")

    def surface_bounds(self, tile: int = 0) -> np.ndarray:
        """Per-cascade bounds of the displacement (ocean.h ocean_surface_bounds), blocking: float32[C][8] =
        (min x, y, z, w, max x, y, z, w) over the texels of each DISP slice of `tile`, exact.  The cascade sum of
        the records bounds sample_world's displacement, up to rounding: a displaced mesh's bounding box."""
        out = np.empty((self.C, 8), np.float32)
        _check(self.lib.ocean_surface_bounds(self._h, tile, out.ctypes.data, out.nbytes), "ocean_surface_bounds")
        return out

    def surface_bounds_device(self, out_ptr: int, tile: int = 0) -> None:
        """The device-pointer form (ocean_surface_bounds_device): out float[C][8] on this context's device, 16-B
        aligned; async on the context's stream, after the queued steps."""
        _check(self.lib.ocean_surface_bounds_device(self._h, tile, ctypes.c_void_p(out_ptr), self.C * 32),
               "ocean_surface_bounds_device")

    @staticmethod
    def _rays(rays) -> np.ndarray:
        r = np.ascontiguousarray(rays, np.float32)
        if r.ndim != 2 or r.shape[1] != 8:
            raise ValueError(f"rays must be float32[M][8] = (origin xyz, direction xyz, t0, t1), got {r.shape}")
        return r

    def raycast(self, rays, tile: int = 0, iterations: int = 4, steps: int = 64, refine: int = 8) -> np.ndarray:
        """Ray casts against the surface (ocean.h ocean_raycast), blocking: rays float[M][8] = (origin x, y, z,
        direction x, y, z, t0, t1) -> float32[M][8]: (t*, the ray point's height over the water there, the
        fixed point's residual, status RAY_MISS / RAY_HIT / RAY_SUBMERGED, normal x, y, z, foam).  A march over
        `steps` intervals of [t0, t1], then `refine` bisections of the first one that crosses; `iterations` as
        query_surface.  The point met is origin + t* direction."""
        r = self._rays(rays)
        out = np.empty((r.shape[0], 8), np.float32)
        _check(self.lib.ocean_raycast(self._h, tile, iterations, steps, refine, r.ctypes.data, r.shape[0],
                                      out.ctypes.data), "ocean_raycast")
        return out

    def raycast_async(self, rays, tile: int = 0, iterations: int = 4, steps: int = 64, refine: int = 8,
                      buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_raycast_async), as query_surface_async: the rays are cast behind the queued
        steps and their float32[M][8] lands in pinned host memory; `rays` is consumed by the call."""
        r = self._rays(rays)
        return Readback(self, (r.shape[0], 8), r.shape[0] * 32, "ocean_raycast_async",
                        lambda dst, req: self.lib.ocean_raycast_async(self._h, tile, iterations, steps, refine,
                                                                      r.ctypes.data, r.shape[0], dst, req), buf)

    def raycast_device(self, rays_ptr: int, count: int, out_ptr: int, tile: int = 0, iterations: int = 4,
                       steps: int = 64, refine: int = 8) -> None:
        """The device-pointer form (ocean_raycast_device): rays float[count][8] and out float[count][8] live on
        this context's device (rays 4-B, out 16-B aligned); async on the context's stream, after the queued
        steps; count is bounded by RAY_MAX_SAMPLES / steps alone."""
        vp = ctypes.c_void_p
        _check(self.lib.ocean_raycast_device(self._h, tile, iterations, steps, refine, vp(rays_ptr), count,
                                             vp(out_ptr)), "ocean_raycast_device")

    # -- the atmosphere (ocean.h, "The atmosphere") ---------------------------------
    def atmosphere(self, params=None, dims=None) -> None:
        """The transmittance and the multiscatter table (ocean_atmosphere), queued on the context's stream: `params`
        float32[32] (atmosphere_params(), its defaults when None), `dims` the six sizes (Tw, Th, Mw, Mh, Sw, Sh),
        AtmosphereController's when None.  The sky-view table is stale until the next sky_update."""
        p = np.ascontiguousarray(atmosphere_params() if params is None else params, np.float32).reshape(-1)
        if p.shape[0] != ATMOSPHERE_FLOATS:
            raise ValueError(f"params must be float32[{ATMOSPHERE_FLOATS}] (atmosphere_params()), got {p.shape}")
        d = [0] * 6 if dims is None else [int(v) for v in dims]
        if len(d) != 6:
            raise ValueError("dims must be the six sizes (Tw, Th, Mw, Mh, Sw, Sh)")
        _check(self.lib.ocean_atmosphere(self._h, p.ctypes.data, *d), "ocean_atmosphere")

    def sky_update(self, sun) -> None:
        """The sky-view table for the direction towards the sun, any length > 0 (ocean_sky_update): the per-frame
        call, queued on the context's stream before later camera calls."""
        s = np.ascontiguousarray(sun, np.float32).reshape(-1)
        if s.shape[0] != 3:
            raise ValueError("sun must be three floats")
        _check(self.lib.ocean_sky_update(self._h, s.ctypes.data), "ocean_sky_update")

    def atmosphere_lut_ptr(self, which: int):
        """(device pointer, width, height) of table `which` (ocean_atmosphere_lut)."""
        dev, w, h = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        _check(self.lib.ocean_atmosphere_lut(self._h, which, ctypes.byref(dev), ctypes.byref(w), ctypes.byref(h)),
               "ocean_atmosphere_lut")
        return dev.value, int(w.value), int(h.value)

    def atmosphere_lut(self, which: int) -> np.ndarray:
        """Table `which` (LUT_TRANSMITTANCE, LUT_MULTISCATTER, LUT_SKYVIEW) as float32[height][width][4]; blocking
        (ocean_atmosphere_read)."""
        _, w, h = self.atmosphere_lut_ptr(which)
        out = np.empty((h, w, 4), np.float32)
        _check(self.lib.ocean_atmosphere_read(self._h, which, out.ctypes.data, out.nbytes), "ocean_atmosphere_read")
        return out

    def sun_color(self, sun) -> np.ndarray:
        """The colour of the sun's light for the direction towards the sun, float32[3]: the reference's
        colorBySunElevation gradient over the transmittance table (ocean_sun_color); a material's light_color."""
        s = np.ascontiguousarray(sun, np.float32).reshape(-1)
        if s.shape[0] != 3:
            raise ValueError("sun must be three floats")
        rgb = np.empty(3, np.float32)
        _check(self.lib.ocean_sun_color(self._h, s.ctypes.data, rgb.ctypes.data), "ocean_sun_color")
        return rgb

    @staticmethod
    def _camera_args(camera, material, mode: int, width: int, height: int):
        """(camera float32[14], material float32[32] or None, result shape, bytes)."""
        cam = np.ascontiguousarray(camera, np.float32).reshape(-1)
        if cam.shape[0] != CAMERA_FLOATS:
            raise ValueError(f"camera must be float32[{CAMERA_FLOATS}] (look_at_camera), got {cam.shape}")
        mat = None
        if material is not None:
            mat = np.ascontiguousarray(material, np.float32).reshape(-1)
            if mat.shape[0] != CAMERA_MATERIAL_FLOATS:
                raise ValueError(f"material must be float32[{CAMERA_MATERIAL_FLOATS}] (material()), got {mat.shape}")
        w, h = max(int(width), 0), max(int(height), 0)
        if w * h > CAMERA_MAX_PIXELS:  # refused by the library as well; no host buffer of that size first
            w = h = 0
        shape = {CAMERA_HITS: (h, w, 8), CAMERA_RANGE: (h, w), CAMERA_COLOR: (h, w, 4),
                 CAMERA_COLOR | CAMERA_SKY_LUT: (h, w, 4)}.get(mode, (0,))
        return cam, mat, shape, int(np.prod(shape, dtype=np.int64)) * 4

    def camera(self, camera, width: int, height: int, mode: int = CAMERA_COLOR, material=None, tile: int = 0,
               iterations: int = 4, steps: int = 64, refine: int = 8) -> np.ndarray:
        """An image of the sea (ocean.h ocean_camera), blocking: pixel (i, j)'s ray follows from `camera`
        (look_at_camera) and meets the water where raycast says that ray does.  CAMERA_HITS: raycast's records,
        float32[height][width][8]; CAMERA_RANGE: the distance along the ray, inf after a miss,
        float32[height][width]; CAMERA_COLOR: Water.shader's fragment stage at the point met under `material`
        (material()), float32[height][width][4] = (r, g, b, status)."""
        cam, mat, shape, nbytes = self._camera_args(camera, material, mode, width, height)
        out = np.empty(shape, np.float32)
        _check(self.lib.ocean_camera(self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                                     mat.ctypes.data if mat is not None else None, width, height, out.ctypes.data,
                                     nbytes), "ocean_camera")
        return out

    def camera_async(self, camera, width: int, height: int, mode: int = CAMERA_COLOR, material=None, tile: int = 0,
                     iterations: int = 4, steps: int = 64, refine: int = 8, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_camera_async), as surface_grid_async: the image is computed behind the queued
        steps and lands in pinned host memory; it must fit a readback slot."""
        cam, mat, shape, nbytes = self._camera_args(camera, material, mode, width, height)
        return Readback(self, shape, nbytes, "ocean_camera_async",
                        lambda dst, req: self.lib.ocean_camera_async(self._h, tile, mode, iterations, steps, refine,
                                                                     cam.ctypes.data,
                                                                     mat.ctypes.data if mat is not None else None,
                                                                     width, height, dst, nbytes, req), buf)

    def camera_device(self, out_ptr: int, camera, width: int, height: int, mode: int = CAMERA_COLOR, material=None,
                      tile: int = 0, iterations: int = 4, steps: int = 64, refine: int = 8) -> None:
        """The device-pointer form (ocean_camera_device): the image is written to `out_ptr` on this context's device,
        16-B aligned; async on the context's stream, after the queued steps.  `camera` and `material` are host
        arrays, consumed by the call."""
        cam, mat, _, nbytes = self._camera_args(camera, material, mode, width, height)
        _check(self.lib.ocean_camera_device(self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                                            mat.ctypes.data if mat is not None else None, width, height,
                                            ctypes.c_void_p(out_ptr), nbytes), "ocean_camera_device")

    @staticmethod
    def _body_view_args(box, paint, bodies):
        """(box float32[6], paint float32[4] or None, records float32[count][stride] or None, stride, count)."""
        bx = np.ascontiguousarray(box, np.float32).reshape(-1)
        if bx.shape[0] != 6:
            raise ValueError(f"box must be float32[6] = (lo, hi), got {bx.shape}")
        pt = None
        if paint is not None:
            pt = np.ascontiguousarray(paint, np.float32).reshape(-1)
            if pt.shape[0] != BODY_PAINT_FLOATS:
                raise ValueError(f"paint must be float32[{BODY_PAINT_FLOATS}] = (r, g, b, ka), got {pt.shape}")
        if bodies is None or len(bodies) == 0:
            return bx, pt, None, BODY_STRIDE_MIN, 0
        rec = np.ascontiguousarray(bodies, np.float32)
        if rec.ndim != 2 or rec.shape[1] < BODY_STRIDE_MIN:
            raise ValueError(f"bodies must be float32[count][stride >= 10] = (c, q, s, ...), got {rec.shape}")
        return bx, pt, rec, rec.shape[1], rec.shape[0]

    def camera_bodies(self, camera, width: int, height: int, bodies, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5),
                      paint=(0.8, 0.8, 0.8, 1.0), mode: int = CAMERA_COLOR, material=None, tile: int = 0,
                      iterations: int = 4, steps: int = 64, refine: int = 8) -> np.ndarray:
        """camera() with the boxes of `bodies` in front of the water (ocean.h ocean_camera_bodies), blocking.  bodies:
        float32[count][stride], stride in [10, 64], a record's first ten floats (c, q, s) as body_buoyancy takes them
        (the state or the result of body_step serves as it is), or None; box: (lo, hi) of the one box all bodies share,
        in the body frame before the scale; paint: (r, g, b, ka), read in the colour modes.  A body pixel has the
        status RAY_BODY: HITS (te, 0, 0, 3, normal, index), RANGE te, COLOR the painted box under the sky and the sun."""
        cam, mat, shape, nbytes = self._camera_args(camera, material, mode, width, height)
        bx, pt, rec, stride, count = self._body_view_args(box, paint, bodies)
        out = np.empty(shape, np.float32)
        _check(self.lib.ocean_camera_bodies(self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                                            mat.ctypes.data if mat is not None else None, width, height, bx.ctypes.data,
                                            pt.ctypes.data if pt is not None else None,
                                            rec.ctypes.data if rec is not None else None, stride, count,
                                            out.ctypes.data, nbytes), "ocean_camera_bodies")
        return out

    def camera_bodies_async(self, camera, width: int, height: int, bodies, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5),
                            paint=(0.8, 0.8, 0.8, 1.0), mode: int = CAMERA_COLOR, material=None, tile: int = 0,
                            iterations: int = 4, steps: int = 64, refine: int = 8, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_camera_bodies_async), as camera_async: `bodies` is consumed by the call."""
        cam, mat, shape, nbytes = self._camera_args(camera, material, mode, width, height)
        bx, pt, rec, stride, count = self._body_view_args(box, paint, bodies)
        return Readback(self, shape, nbytes, "ocean_camera_bodies_async",
                        lambda dst, req: self.lib.ocean_camera_bodies_async(
                            self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                            mat.ctypes.data if mat is not None else None, width, height, bx.ctypes.data,
                            pt.ctypes.data if pt is not None else None, rec.ctypes.data if rec is not None else None,
                            stride, count, dst, nbytes, req), buf)

    def camera_bodies_device(self, out_ptr: int, camera, width: int, height: int, bodies_ptr: int, count: int,
                             stride: int = 32, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5), paint=(0.8, 0.8, 0.8, 1.0),
                             mode: int = CAMERA_COLOR, material=None, tile: int = 0, iterations: int = 4,
                             steps: int = 64, refine: int = 8) -> None:
        """The device-pointer form (ocean_camera_bodies_device): `bodies_ptr` holds `count` records `stride` floats
        apart on this context's device (32: where body_step_device left them), `out_ptr` is 16-B aligned; async on the
        context's stream, after the queued steps.  camera, material, box and paint are host arrays."""
        cam, mat, _, nbytes = self._camera_args(camera, material, mode, width, height)
        bx, pt, _, _, _ = self._body_view_args(box, paint, None)
        _check(self.lib.ocean_camera_bodies_device(self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                                                   mat.ctypes.data if mat is not None else None, width, height,
                                                   bx.ctypes.data, pt.ctypes.data if pt is not None else None,
                                                   ctypes.c_void_p(bodies_ptr) if bodies_ptr else None, stride, count,
                                                   ctypes.c_void_p(out_ptr), nbytes), "ocean_camera_bodies_device")

    @staticmethod
    def _scene_args(camera, material, optics, width, height):
        """(camera, material, optics float32[6], result shape, bytes): 16 B per pixel in every mode of the scene."""
        cam, mat, shape, nbytes = OceanContext._camera_args(camera, material, CAMERA_COLOR, width, height)
        op = np.ascontiguousarray(optics, np.float32).reshape(-1)
        if op.shape[0] != SCENE_OPTICS_FLOATS:
            raise ValueError(f"optics must be float32[{SCENE_OPTICS_FLOATS}] (optics()), got {op.shape}")
        return cam, mat, op, shape, nbytes

    def camera_scene(self, camera, width: int, height: int, bodies, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5),
                     paint=(0.8, 0.8, 0.8, 1.0), optics=(0.0, 0.0, 0.0, 0.5, 0.2, 100.0), mode: int = CAMERA_COLOR,
                     material=None, tile: int = 0, iterations: int = 4, steps: int = 64, refine: int = 8) -> np.ndarray:
        """camera_bodies() with the water seeing the bodies (ocean.h ocean_camera_scene), blocking: at a water pixel
        the body behind the surface shows through, fogged by its distance behind it; a body between the point met and
        the sun shadows it; a body on the mirror ray is reflected instead of the sky.  optics: optics().  mode:
        CAMERA_COLOR, CAMERA_COLOR | CAMERA_SKY_LUT, or CAMERA_LINKS: float32[height][width][4] = (sf, the body seen
        through the water or -1, the body reflected or -1, status), a body pixel (1, its body, -1, RAY_BODY).  The
        material is required in every mode, the paint in the colour modes."""
        cam, mat, op, shape, nbytes = self._scene_args(camera, material, optics, width, height)
        bx, pt, rec, stride, count = self._body_view_args(box, paint, bodies)
        out = np.empty(shape, np.float32)
        _check(self.lib.ocean_camera_scene(self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                                           mat.ctypes.data if mat is not None else None, width, height, bx.ctypes.data,
                                           pt.ctypes.data if pt is not None else None, op.ctypes.data,
                                           rec.ctypes.data if rec is not None else None, stride, count,
                                           out.ctypes.data, nbytes), "ocean_camera_scene")
        return out

    def camera_scene_async(self, camera, width: int, height: int, bodies, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5),
                           paint=(0.8, 0.8, 0.8, 1.0), optics=(0.0, 0.0, 0.0, 0.5, 0.2, 100.0), mode: int = CAMERA_COLOR,
                           material=None, tile: int = 0, iterations: int = 4, steps: int = 64, refine: int = 8,
                           buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_camera_scene_async), as camera_bodies_async: `bodies` is consumed by the call."""
        cam, mat, op, shape, nbytes = self._scene_args(camera, material, optics, width, height)
        bx, pt, rec, stride, count = self._body_view_args(box, paint, bodies)
        return Readback(self, shape, nbytes, "ocean_camera_scene_async",
                        lambda dst, req: self.lib.ocean_camera_scene_async(
                            self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                            mat.ctypes.data if mat is not None else None, width, height, bx.ctypes.data,
                            pt.ctypes.data if pt is not None else None, op.ctypes.data,
                            rec.ctypes.data if rec is not None else None, stride, count, dst, nbytes, req), buf)

    def camera_scene_device(self, out_ptr: int, camera, width: int, height: int, bodies_ptr: int, count: int,
                            stride: int = 32, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5), paint=(0.8, 0.8, 0.8, 1.0),
                            optics=(0.0, 0.0, 0.0, 0.5, 0.2, 100.0), mode: int = CAMERA_COLOR, material=None,
                            tile: int = 0, iterations: int = 4, steps: int = 64, refine: int = 8) -> None:
        """The device-pointer form (ocean_camera_scene_device), as camera_bodies_device: `bodies_ptr` holds `count`
        records `stride` floats apart on this context's device (32: where body_step_device left them), `out_ptr` is
        16-B aligned; async on the context's stream.  camera, material, box, paint and optics are host arrays."""
        cam, mat, op, _, nbytes = self._scene_args(camera, material, optics, width, height)
        bx, pt, _, _, _ = self._body_view_args(box, paint, None)
        _check(self.lib.ocean_camera_scene_device(self._h, tile, mode, iterations, steps, refine, cam.ctypes.data,
                                                  mat.ctypes.data if mat is not None else None, width, height,
                                                  bx.ctypes.data, pt.ctypes.data if pt is not None else None,
                                                  op.ctypes.data, ctypes.c_void_p(bodies_ptr) if bodies_ptr else None,
                                                  stride, count, ctypes.c_void_p(out_ptr), nbytes),
               "ocean_camera_scene_device")

    @staticmethod
    def grid_points(x0: float, z0: float, dx: float, dz: float, nx: int, ny: int) -> np.ndarray:
        """The nodes of a grid as ocean_surface_grid places them, float32[ny * nx][2] = (world x, world z):
        node (i, j) at (x0 + float32(i) * dx, z0 + float32(j) * dz), one fp32 multiply and one fp32 add
        each, at row j * nx + i."""
        f32 = np.float32
        xs = f32(x0) + np.arange(nx, dtype=f32) * f32(dx)
        zs = f32(z0) + np.arange(ny, dtype=f32) * f32(dz)
        out = np.empty((ny, nx, 2), f32)
        out[..., 0] = xs[None, :]
        out[..., 1] = zs[:, None]
        return out.reshape(ny * nx, 2)

    @staticmethod
    def _grid_args(mode: int, iterations: Optional[int], nx: int, ny: int):
        """(iterations, result shape, bytes): `iterations` defaults to 4, to 0 for GRID_VERTICES."""
        if iterations is None:
            iterations = 0 if mode == GRID_VERTICES else 4
        nx, ny = int(nx), int(ny)
        shape = (max(ny, 0), max(nx, 0)) if mode == GRID_HEIGHTFIELD else (max(ny, 0), max(nx, 0), 8)
        return iterations, shape, int(np.prod(shape, dtype=np.int64)) * 4

    def surface_grid(self, x0: float, z0: float, dx: float, dz: float, nx: int, ny: int, mode: int = GRID_SURFACE,
                     iterations: Optional[int] = None, lod: float = 0.0, tile: int = 0) -> np.ndarray:
        """The surface over a regular grid (ocean.h ocean_surface_grid), blocking: node (i, j) at
        (x0 + i dx, z0 + j dz) -> float32[ny][nx][8], or float32[ny][nx] for GRID_HEIGHTFIELD.
        GRID_VERTICES (iterations 0, `lod` as sample_world): displaced vertex x, y, z, foam, normal x, y, z, 0
        (MeshGenerator's plane through the domain stage of Water.shader); GRID_SURFACE (`iterations`
        defaults to 4): query_surface's record at every node; GRID_HEIGHTFIELD: its height alone."""
        iterations, shape, nbytes = self._grid_args(mode, iterations, nx, ny)
        if nx * ny > GRID_MAX_NODES:  # refused by the library as well; no host buffer of that size first
            shape, nbytes = (0,), 0
        out = np.empty(shape, np.float32)
        _check(self.lib.ocean_surface_grid(self._h, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny,
                                           out.ctypes.data, nbytes), "ocean_surface_grid")
        return out

    def surface_grid_async(self, x0: float, z0: float, dx: float, dz: float, nx: int, ny: int,
                           mode: int = GRID_SURFACE, iterations: Optional[int] = None, lod: float = 0.0,
                           tile: int = 0, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_surface_grid_async): the grid is computed behind the queued steps and
        lands in pinned host memory like a read_async slice.  Poll .done() / .wait(), then .data; `buf`: a
        caller-owned pinned slot of at least the result's size."""
        iterations, shape, nbytes = self._grid_args(mode, iterations, nx, ny)
        return Readback(self, shape, nbytes, "ocean_surface_grid_async",
                        lambda dst, req: self.lib.ocean_surface_grid_async(self._h, tile, mode, iterations, lod, x0, z0, dx,
                                                                           dz, nx, ny, dst, nbytes, req), buf)

    @staticmethod
    def parse_whitecaps(buf: np.ndarray):
        """(T, records float32[W][8]) of a whitecap list float32[capacity + 1][8] as ocean_whitecaps writes it: the
        header's eight uint32 (T, W, nodes, capacity, 0, 0, 0, 0), then W records in ascending node order."""
        buf = np.ascontiguousarray(buf, np.float32).reshape(-1, 8)
        head = buf[0].view(np.uint32)
        return int(head[0]), buf[1:1 + int(head[1])].copy()

    def whitecaps(self, threshold: float, x0: float, z0: float, dx: float, dz: float, nx: int, ny: int,
                  capacity: int = 4096, lod: float = 0.0, tile: int = 0):
        """Whitecap emitters (ocean.h ocean_whitecaps), blocking: the nodes (i, j) at (x0 + i dx, z0 + j dz) whose
        foam, sample_world's [0][3] at `lod`, is >= threshold, in ascending k = j nx + i -> (T, float32[W][8]): T the
        number of selected nodes, W = min(T, capacity) records (displaced x, y, z, foam, the water's velocity x, y,
        z on an F_VELOCITY context else zeros, float(k))."""
        capacity = int(capacity)
        # (a capacity outside the limits is refused by the library; no host buffer of that size first)
        buf = np.empty((capacity + 1 if 1 <= capacity <= WHITECAP_MAX_RECORDS else 1, 8), np.float32)
        _check(self.lib.ocean_whitecaps(self._h, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, buf.ctypes.data,
                                        buf.nbytes), "ocean_whitecaps")
        return self.parse_whitecaps(buf)

    def whitecaps_async(self, threshold: float, x0: float, z0: float, dx: float, dz: float, nx: int, ny: int,
                        capacity: int = 4096, lod: float = 0.0, tile: int = 0, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_whitecaps_async): the list is built behind the queued steps and its
        float32[capacity + 1][8] lands in pinned host memory like a read_async slice.  Poll .done() / .wait(), then
        .whitecaps() -> (T, records[W][8]); `buf`: a caller-owned pinned slot of at least (capacity + 1) x 32 B."""
        nbytes = (int(capacity) + 1) * 32
        return Readback(self, (int(capacity) + 1, 8), nbytes, "ocean_whitecaps_async",
                        lambda dst, req: self.lib.ocean_whitecaps_async(self._h, tile, lod, threshold, x0, z0, dx, dz, nx,
                                                                        ny, capacity, dst, nbytes, req), buf)

    def whitecaps_device(self, out_ptr: int, threshold: float, x0: float, z0: float, dx: float, dz: float, nx: int,
                         ny: int, capacity: int, lod: float = 0.0, tile: int = 0) -> None:
        """The device-pointer form (ocean_whitecaps_device): out float[capacity + 1][8] on this context's device,
        16-B aligned; async on the context's stream, after the queued steps.  parse_whitecaps reads a copy of it."""
        _check(self.lib.ocean_whitecaps_device(self._h, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity,
                                               ctypes.c_void_p(out_ptr), (int(capacity) + 1) * 32), "ocean_whitecaps_device")

    @staticmethod
    def spray_params(h: float, g: float = 9.81, kd: float = 0.0, wind=(0.0, 0.0, 0.0), life: float = 4.0,
                     jet: float = 1.0, lift: float = 0.0) -> np.ndarray:
        """The float32[16] `spray` of ocean_spray_step (ocean.h): (h, g, kd, wind xyz, life, jet, lift, zeros)."""
        sp = np.zeros(SPRAY_FLOATS, np.float32)
        sp[:9] = (h, g, kd, wind[0], wind[1], wind[2], life, jet, lift)
        return sp

    @staticmethod
    def spray_pool(records, capacity: int) -> np.ndarray:
        """A pool float32[capacity + 1][8] as ocean_spray_step reads it, holding `records` float32[W][8] = (position,
        age, velocity, tag) behind the header (W, W, W, capacity, 0, 0, 0, 0); the rest is zero."""
        rec = np.ascontiguousarray(records, np.float32).reshape(-1, 8)
        if rec.shape[0] > capacity:
            raise ValueError(f"{rec.shape[0]} records > capacity {capacity}")
        buf = np.zeros((int(capacity) + 1, 8), np.float32)
        buf[0].view(np.uint32)[:4] = (rec.shape[0], rec.shape[0], rec.shape[0], capacity)
        buf[1:1 + rec.shape[0]] = rec
        return buf

    @staticmethod
    def parse_spray(buf: np.ndarray):
        """(T, M, records float32[W][8]) of a pool float32[capacity + 1][8] as ocean_spray_step writes it: the header's
        eight uint32 (T, W, M, capacity, 0, 0, 0, 0), then the W surviving particles in candidate order (a copy)."""
        buf = np.ascontiguousarray(buf, np.float32).reshape(-1, 8)
        head = buf[0].view(np.uint32)
        return int(head[0]), int(head[2]), buf[1:1 + int(head[1])].copy()

    @staticmethod
    def _spray_args(spray, pool, emitters):
        """(spray float32[16], pool float32[capacity + 1][8], capacity, emitters or None, emit_capacity)."""
        sp = np.ascontiguousarray(spray, np.float32).reshape(-1)
        if sp.shape[0] != SPRAY_FLOATS:
            raise ValueError(f"spray must be float32[{SPRAY_FLOATS}] (spray_params), got {sp.shape}")
        pl = np.ascontiguousarray(pool, np.float32)
        if pl.ndim != 2 or pl.shape[1] != 8 or pl.shape[0] < 1:
            raise ValueError(f"pool must be float32[capacity + 1][8], got {pl.shape}")
        em = None
        if emitters is not None:
            em = np.ascontiguousarray(emitters, np.float32)
            if em.ndim != 2 or em.shape[1] != 8 or em.shape[0] < 1:
                raise ValueError(f"emitters must be float32[emit_capacity + 1][8], got {em.shape}")
        return sp, pl, pl.shape[0] - 1, em, (em.shape[0] - 1 if em is not None else 0)

    def spray_step(self, spray, pool, emitters=None, substeps: int = 1, iterations: int = 2, tile: int = 0) -> np.ndarray:
        """Spray particles (ocean.h ocean_spray_step), blocking: the candidates of `pool` float32[capacity + 1][8]
        and, behind them, one fresh particle per record of the whitecap list `emitters` float32[emit_capacity + 1][8]
        (or None) take `substeps` substeps under `spray` (spray_params) and the survivors come back compacted, in
        candidate order -> float32[capacity + 1][8], the records past W zero; parse_spray reads it."""
        sp, pl, capacity, em, emit_capacity = self._spray_args(spray, pool, emitters)
        out = np.zeros_like(pl)
        _check(self.lib.ocean_spray_step(self._h, tile, iterations, substeps, sp.ctypes.data, pl.ctypes.data, capacity,
                                         em.ctypes.data if em is not None else None, emit_capacity, out.ctypes.data,
                                         out.nbytes), "ocean_spray_step")
        out[1 + min(int(out[0].view(np.uint32)[1]), capacity):] = 0  # unspecified in the library's output
        return out

    def spray_step_async(self, spray, pool, emitters=None, substeps: int = 1, iterations: int = 2, tile: int = 0,
                         buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_spray_step_async): `pool` and `emitters` are consumed by the call, the pool is
        stepped behind the queued steps and its float32[capacity + 1][8] lands in pinned host memory.  Poll .done() /
        .wait(), then .spray() -> (T, M, records[W][8])."""
        sp, pl, capacity, em, emit_capacity = self._spray_args(spray, pool, emitters)
        nbytes = pl.nbytes
        return Readback(self, pl.shape, nbytes, "ocean_spray_step_async",
                        lambda dst, req: self.lib.ocean_spray_step_async(
                            self._h, tile, iterations, substeps, sp.ctypes.data, pl.ctypes.data, capacity,
                            em.ctypes.data if em is not None else None, emit_capacity, dst, nbytes, req), buf)

    def spray_step_device(self, out_ptr: int, spray, pool_ptr: int, capacity: int, emitters_ptr: int = 0,
                          emit_capacity: int = 0, substeps: int = 1, iterations: int = 2, tile: int = 0) -> None:
        """The device-pointer form (ocean_spray_step_device): pool and out float[capacity + 1][8], emitters
        float[emit_capacity + 1][8] or 0, on this context's device, 16-B aligned; async on the context's stream, after
        the queued steps.  `out_ptr` overlaps neither input: ping-pong two pools.  `spray` is a host array."""
        sp = np.ascontiguousarray(spray, np.float32).reshape(-1)
        if sp.shape[0] != SPRAY_FLOATS:
            raise ValueError(f"spray must be float32[{SPRAY_FLOATS}] (spray_params), got {sp.shape}")
        _check(self.lib.ocean_spray_step_device(self._h, tile, iterations, substeps, sp.ctypes.data,
                                                ctypes.c_void_p(pool_ptr), capacity,
                                                ctypes.c_void_p(emitters_ptr) if emitters_ptr else None, emit_capacity,
                                                ctypes.c_void_p(out_ptr), (int(capacity) + 1) * 32),
               "ocean_spray_step_device")

    @staticmethod
    def _body_args(hull, bodies):
        h = np.ascontiguousarray(hull, np.float32)
        b = np.ascontiguousarray(bodies, np.float32)
        if h.ndim != 2 or h.shape[1] != 5:
            raise ValueError(f"hull must be float32[P][5] = (rx, ry, rz, h, v), got {h.shape}")
        if b.ndim != 2 or b.shape[1] != 10:
            raise ValueError(f"bodies must be float32[M][10] = (c, quaternion xyzw, scale), got {b.shape}")
        return h, b

    def body_buoyancy(self, hull, bodies, iterations: int = 4, mode: int = QUERY_SURFACE, tile: int = 0) -> np.ndarray:
        """Buoyant bodies on the device (ocean.h ocean_body_buoyancy), blocking: hull float[P][5] = (cell centre
        in the body frame, vertical extent, volume), shared by the bodies float[M][10] = (origin, body -> world
        quaternion xyzw, per-axis scale) -> float32[M][8]: (submerged volume V, V * centroid relative to the
        origin xyz, V-weighted water normal xyz, worst residual).  `mode` and `iterations` as query_surface
        (QUERY_REFERENCE takes iterations 0); buoyancy_wrench turns the records into forces."""
        h, b = self._body_args(hull, bodies)
        out = np.empty((b.shape[0], 8), np.float32)
        _check(self.lib.ocean_body_buoyancy(self._h, tile, mode, iterations, h.ctypes.data, h.shape[0], b.ctypes.data,
                                            b.shape[0], out.ctypes.data), "ocean_body_buoyancy")
        return out

    def body_buoyancy_async(self, hull, bodies, iterations: int = 4, mode: int = QUERY_SURFACE, tile: int = 0,
                            buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_body_buoyancy_async): the kernel runs behind the queued steps and its
        float32[M][8] lands in pinned host memory like a read_async slice; `hull` and `bodies` are consumed by
        the call.  Poll .done() / .wait(), then .data; `buf`: a caller-owned pinned slot of at least M x 32 B."""
        h, b = self._body_args(hull, bodies)
        return Readback(self, (b.shape[0], 8), b.shape[0] * 32, "ocean_body_buoyancy_async",
                        lambda dst, req: self.lib.ocean_body_buoyancy_async(self._h, tile, mode, iterations, h.ctypes.data,
                                                                            h.shape[0], b.ctypes.data, b.shape[0], dst,
                                                                            req), buf)

    def body_buoyancy_device(self, hull_ptr: int, probes: int, bodies_ptr: int, count: int, out_ptr: int,
                             iterations: int = 4, mode: int = QUERY_SURFACE, tile: int = 0) -> None:
        """The device-pointer form (ocean_body_buoyancy_device): hull float[probes][5], bodies float[count][10]
        and out float[count][8] live on this context's device (hull and bodies 4-B, out 16-B aligned); async
        on the context's stream, after the queued steps."""
        vp = ctypes.c_void_p
        _check(self.lib.ocean_body_buoyancy_device(self._h, tile, mode, iterations, vp(hull_ptr), probes, vp(bodies_ptr),
                                                   count, vp(out_ptr)), "ocean_body_buoyancy_device")

    @staticmethod
    def _motion_arg(motion, count: int) -> np.ndarray:
        m = np.ascontiguousarray(motion, np.float32)
        if m.ndim != 2 or m.shape != (count, 6):
            raise ValueError(f"motion must be float32[M][6] = (velocity, angular velocity) for M = {count}, got {m.shape}")
        return m

    def body_dynamics(self, hull, bodies, motion, iterations: int = 4, mode: int = QUERY_SURFACE,
                      law: int = DRAG_LINEAR, tile: int = 0) -> np.ndarray:
        """Buoyancy and drag against the water's velocity on the device (ocean.h ocean_body_dynamics; F_VELOCITY
        contexts), blocking: hull and bodies as body_buoyancy, motion float[M][6] = (world linear velocity of the
        body origin, world angular velocity) -> float32[M][16]: body_buoyancy's record, then (sum F xyz, sum T xyz
        about the origin, largest relative speed over the wet probes, number of wet probes) with F = g u
        (DRAG_LINEAR) or g |u| u (DRAG_QUADRATIC) per probe, u = water - hull velocity, g the submerged volume.
        The drag force is k out[8:11] and its torque k out[11:14] for the host's coefficient k."""
        h, b = self._body_args(hull, bodies)
        m = self._motion_arg(motion, b.shape[0])
        out = np.empty((b.shape[0], 16), np.float32)
        _check(self.lib.ocean_body_dynamics(self._h, tile, mode, iterations, law, h.ctypes.data, h.shape[0], b.ctypes.data,
                                            m.ctypes.data, b.shape[0], out.ctypes.data), "ocean_body_dynamics")
        return out

    def body_dynamics_async(self, hull, bodies, motion, iterations: int = 4, mode: int = QUERY_SURFACE,
                            law: int = DRAG_LINEAR, tile: int = 0, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_body_dynamics_async), as body_buoyancy_async: float32[M][16] lands in pinned
        host memory; `hull`, `bodies` and `motion` are consumed by the call.  `buf`: a caller-owned pinned slot of
        at least M x 64 B."""
        h, b = self._body_args(hull, bodies)
        m = self._motion_arg(motion, b.shape[0])
        return Readback(self, (b.shape[0], 16), b.shape[0] * 64, "ocean_body_dynamics_async",
                        lambda dst, req: self.lib.ocean_body_dynamics_async(self._h, tile, mode, iterations, law,
                                                                            h.ctypes.data, h.shape[0], b.ctypes.data,
                                                                            m.ctypes.data, b.shape[0], dst, req), buf)

    def body_dynamics_device(self, hull_ptr: int, probes: int, bodies_ptr: int, motion_ptr: int, count: int, out_ptr: int,
                             iterations: int = 4, mode: int = QUERY_SURFACE, law: int = DRAG_LINEAR, tile: int = 0) -> None:
        """The device-pointer form (ocean_body_dynamics_device): hull float[probes][5], bodies float[count][10],
        motion float[count][6] and out float[count][16] live on this context's device (inputs 4-B, out 16-B
        aligned); async on the context's stream, after the queued steps."""
        vp = ctypes.c_void_p
        _check(self.lib.ocean_body_dynamics_device(self._h, tile, mode, iterations, law, vp(hull_ptr), probes,
                                                   vp(bodies_ptr), vp(motion_ptr), count, vp(out_ptr)),
               "ocean_body_dynamics_device")

    @staticmethod
    def _step_args(hull, state, props, step):
        h = np.ascontiguousarray(hull, np.float32)
        s = np.ascontiguousarray(state, np.float32)
        p = np.ascontiguousarray(props, np.float32)
        sp = np.ascontiguousarray(step, np.float32).reshape(-1)
        if h.ndim != 2 or h.shape[1] != 5:
            raise ValueError(f"hull must be float32[P][5] = (rx, ry, rz, h, v), got {h.shape}")
        if s.ndim != 2 or s.shape[1] != 32:
            raise ValueError(f"state must be float32[M][32] = (c, quaternion xyzw, scale, v, omega, 16 more), got {s.shape}")
        if p.shape != (s.shape[0], 4):
            raise ValueError(f"props must be float32[M][4] = (1 / mass, 1 / Ix, 1 / Iy, 1 / Iz) for M = {s.shape[0]}, got {p.shape}")
        if sp.shape[0] != BODY_STEP_FLOATS:
            raise ValueError(f"step must be float32[{BODY_STEP_FLOATS}] (step_params), got {sp.shape}")
        return h, s, p, sp

    @staticmethod
    def body_state(bodies, motion=None) -> np.ndarray:
        """float32[M][32] for body_step from bodies float[M][10] and motion float[M][6] (at rest by default); the
        sixteen floats behind them, which the entry ignores on input, are zero."""
        b = np.ascontiguousarray(bodies, np.float32)
        s = np.zeros((b.shape[0], 32), np.float32)
        s[:, :10] = b
        if motion is not None:
            s[:, 10:16] = motion
        return s

    def body_step(self, hull, state, props, step, substeps: int = 1, iterations: int = 4, mode: int = QUERY_SURFACE,
                  law: int = DRAG_LINEAR, tile: int = 0) -> np.ndarray:
        """`substeps` substeps of M rigid bodies on the device (ocean.h ocean_body_step; F_VELOCITY contexts),
        blocking: state float[M][32] = (bodies' record, motion's record, 16 ignored), props float[M][4] = (inverse
        mass, inverse principal moments), step float[8] (step_params) -> float32[M][32]: the state after the last
        substep, then body_dynamics' record of that substep.  The result is the next call's `state`."""
        h, s, p, sp = self._step_args(hull, state, props, step)
        out = np.empty((s.shape[0], 32), np.float32)
        _check(self.lib.ocean_body_step(self._h, tile, mode, iterations, law, substeps, sp.ctypes.data, h.ctypes.data,
                                        h.shape[0], p.ctypes.data, s.ctypes.data, s.shape[0], out.ctypes.data),
               "ocean_body_step")
        return out

    def body_step_async(self, hull, state, props, step, substeps: int = 1, iterations: int = 4, mode: int = QUERY_SURFACE,
                        law: int = DRAG_LINEAR, tile: int = 0, buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_body_step_async), as body_dynamics_async: float32[M][32] lands in pinned host
        memory; `hull`, `state`, `props` and `step` are consumed by the call.  `buf`: a caller-owned pinned slot of
        at least M x 128 B."""
        h, s, p, sp = self._step_args(hull, state, props, step)
        return Readback(self, (s.shape[0], 32), s.shape[0] * 128, "ocean_body_step_async",
                        lambda dst, req: self.lib.ocean_body_step_async(self._h, tile, mode, iterations, law, substeps,
                                                                        sp.ctypes.data, h.ctypes.data, h.shape[0],
                                                                        p.ctypes.data, s.ctypes.data, s.shape[0], dst, req),
                        buf)

    def body_step_device(self, hull_ptr: int, probes: int, props_ptr: int, state_ptr: int, count: int, out_ptr: int, step,
                         substeps: int = 1, iterations: int = 4, mode: int = QUERY_SURFACE, law: int = DRAG_LINEAR,
                         tile: int = 0) -> None:
        """The device-pointer form (ocean_body_step_device): hull float[probes][5], props float[count][4], state
        float[count][32] and out float[count][32] live on this context's device (inputs 4-B, out 16-B aligned), and
        out_ptr may equal state_ptr (in place); `step` is a host array (step_params).  Async on the context's
        stream, after the queued steps."""
        vp = ctypes.c_void_p
        sp = np.ascontiguousarray(step, np.float32).reshape(-1)
        if sp.shape[0] != BODY_STEP_FLOATS:
            raise ValueError(f"step must be float32[{BODY_STEP_FLOATS}] (step_params), got {sp.shape}")
        _check(self.lib.ocean_body_step_device(self._h, tile, mode, iterations, law, substeps, sp.ctypes.data, vp(hull_ptr),
                                               probes, vp(props_ptr), vp(state_ptr), count, vp(out_ptr)),
               "ocean_body_step_device")

    @staticmethod
    def _mesh_args(vertices, triangles, bodies):
        v = np.ascontiguousarray(vertices, np.float32)
        t = np.ascontiguousarray(triangles, np.int32)
        b = np.ascontiguousarray(bodies, np.float32)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f"vertices must be float32[V][3] in the body frame, got {v.shape}")
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError(f"triangles must be int32[T][3], counter-clockwise seen from outside, got {t.shape}")
        if b.ndim != 2 or b.shape[1] != 10:
            raise ValueError(f"bodies must be float32[M][10] = (c, quaternion xyzw, scale), got {b.shape}")
        return v, t, b

    def body_hydrostatics(self, vertices, triangles, bodies, iterations: int = 4, tile: int = 0) -> np.ndarray:
        """Mesh hulls on the device (ocean.h ocean_body_hydrostatics), blocking: vertices float[V][3] in the body frame
        and triangles int[T][3] (outward-wound), shared by the bodies float[M][10] as body_buoyancy takes them ->
        float32[M][16]: (sum F xyz, wetted area, sum Tq xyz about the origin, worst residual, the wetted area's first
        moment xyz, wet triangles, draught, wet vertices, sum Av.y, 0).  rho g times out[0:3] and out[4:7] are the
        hydrostatic force and torque; -out[14] is the waterplane area of a closed hull."""
        v, t, b = self._mesh_args(vertices, triangles, bodies)
        out = np.empty((b.shape[0], HULL_RECORD_FLOATS), np.float32)
        _check(self.lib.ocean_body_hydrostatics(self._h, tile, iterations, v.ctypes.data, v.shape[0], t.ctypes.data,
                                                t.shape[0], b.ctypes.data, b.shape[0], out.ctypes.data),
               "ocean_body_hydrostatics")
        return out

    def body_hydrostatics_async(self, vertices, triangles, bodies, iterations: int = 4, tile: int = 0,
                                buf: "PinnedBuffer" = None) -> "Readback":
        """The per-frame form (ocean_body_hydrostatics_async), as body_buoyancy_async: float32[M][16] lands in pinned
        host memory; the three arrays are consumed by the call.  `buf`: a caller-owned pinned slot of at least
        M x 64 B."""
        v, t, b = self._mesh_args(vertices, triangles, bodies)
        return Readback(self, (b.shape[0], HULL_RECORD_FLOATS), b.shape[0] * HULL_RECORD_FLOATS * 4,
                        "ocean_body_hydrostatics_async",
                        lambda dst, req: self.lib.ocean_body_hydrostatics_async(self._h, tile, iterations, v.ctypes.data,
                                                                                v.shape[0], t.ctypes.data, t.shape[0],
                                                                                b.ctypes.data, b.shape[0], dst, req), buf)

    def body_hydrostatics_device(self, vertices_ptr: int, nverts: int, triangles_ptr: int, ntris: int, bodies_ptr: int,
                                 count: int, out_ptr: int, iterations: int = 4, tile: int = 0) -> None:
        """The device-pointer form (ocean_body_hydrostatics_device): vertices float[nverts][3], triangles int[ntris][3],
        bodies float[count][10] and out float[count][16] live on this context's device (inputs 4-B, out 16-B aligned);
        async on the context's stream, after the queued steps.  The kernel clamps each index into [0, nverts)."""
        vp = ctypes.c_void_p
        _check(self.lib.ocean_body_hydrostatics_device(self._h, tile, iterations, vp(vertices_ptr), nverts,
                                                       vp(triangles_ptr), ntris, vp(bodies_ptr), count, vp(out_ptr)),
               "ocean_body_hydrostatics_device")

    @staticmethod
    def box_mesh(sx: float, sy: float, sz: float, nx: int = 1, ny: int = 1, nz: int = 1):
        """The box [-sx/2, sx/2] x [-sy/2, sy/2] x [-sz/2, sz/2] as a closed triangle mesh, each face cut into a
        lattice of nx, ny, nz cells along x, y, z and every cell into two triangles: (vertices float32[V][3],
        triangles int32[T][3]), wound counter-clockwise seen from outside.  The lattice points on edges and corners are
        shared: V = 2 (nx ny + ny nz + nz nx) + 2 and T = 4 (nx ny + ny nz + nz nx); (1, 1, 1) is 8 and 12."""
        if nx < 1 or ny < 1 or nz < 1:
            raise ValueError("nx, ny and nz must be at least 1")
        n = (nx, ny, nz)
        size = (float(sx), float(sy), float(sz))
        ids, verts, tris = {}, [], []

        def vertex(g):
            if g not in ids:
                ids[g] = len(verts)
                verts.append([size[a] * (g[a] / n[a] - 0.5) for a in range(3)])
            return ids[g]

        for axis in range(3):
            u, w = (axis + 1) % 3, (axis + 2) % 3  # e_u x e_w = e_axis
            for side in (0, 1):
                for j in range(n[w]):
                    for i in range(n[u]):
                        def at(di, dj):
                            g = [0, 0, 0]
                            g[axis], g[u], g[w] = side * n[axis], i + di, j + dj
                            return vertex(tuple(g))
                        q = (at(0, 0), at(1, 0), at(1, 1), at(0, 1))  # counter-clockwise seen from +axis
                        if side == 0:
                            q = q[::-1]
                        tris.append([q[0], q[1], q[2]])
                        tris.append([q[0], q[2], q[3]])
        return np.asarray(verts, np.float32), np.asarray(tris, np.int32)

    @staticmethod
    def box_hull(nx: int, nz: int, ny: int = 1) -> np.ndarray:
        """The unit box [-1/2, 1/2]^3 cut into nx x ny x nz cells, as a hull float32[nx * ny * nz][5]: each
        probe is its cell's centre ((i + 1/2) / n - 1/2 along each axis), h = 1 / ny, v = 1 / (nx ny nz); x
        fastest, then z, then y.  A body's scale makes it a box of that size."""
        if nx < 1 or nz < 1 or ny < 1:
            raise ValueError("nx, nz and ny must be at least 1")
        xs = (np.arange(nx, dtype=np.float64) + 0.5) / nx - 0.5
        zs = (np.arange(nz, dtype=np.float64) + 0.5) / nz - 0.5
        ys = (np.arange(ny, dtype=np.float64) + 0.5) / ny - 0.5
        hull = np.empty((ny, nz, nx, 5), np.float32)
        hull[..., 0] = xs[None, None, :]
        hull[..., 1] = ys[:, None, None]
        hull[..., 2] = zs[None, :, None]
        hull[..., 3] = 1.0 / ny
        hull[..., 4] = 1.0 / (nx * ny * nz)
        return hull.reshape(nx * ny * nz, 5)

    @staticmethod
    def buoyancy_wrench(out, density: float = 1000.0, gravity: float = 9.81):
        """What a rigid-body solver takes from body_buoyancy's records float[M][8], in float64: (force [M][3] =
        (0, density gravity out[0], 0); its application point relative to the body origin [M][3] = out[1..3] /
        out[0], zero for a dry body; torque about the body origin [M][3] = density gravity (-out[3], 0, out[1]))."""
        o = np.asarray(out, np.float64).reshape(-1, 8)
        k = float(density) * float(gravity)
        force = np.zeros((len(o), 3))
        force[:, 1] = k * o[:, 0]
        wet = o[:, 0] != 0.0
        point = np.zeros((len(o), 3))
        point[wet] = o[wet, 1:4] / o[wet, 0:1]
        torque = np.zeros((len(o), 3))
        torque[:, 0] = -k * o[:, 3]
        torque[:, 2] = k * o[:, 1]
        return force, point, torque

    def read_async(self, tex: int, tile: int = 0, cascade: int = 0, buf: "PinnedBuffer" = None) -> "Readback":
        """AsyncGPUReadback.Request (WaterBody.cs:288-296): copy one slice into pinned
        host memory once the queued steps finish; poll .done() / .wait(), then .data.
        `buf`: a caller-owned pinned slot to land in (else the request allocates its own)."""
        ch = _TEX_CHANNELS[tex]
        nbytes = self.n * self.n * ch * 4
        return Readback(self, (self.n, self.n, ch), nbytes, "ocean_read_async",
                        lambda dst, req: self.lib.ocean_read_async(self._h, tex, tile, cascade, dst, nbytes, req), buf)

    def read_height_async(self, tile: int = 0, cascade: int = 0, buf: "PinnedBuffer" = None) -> "Readback":
        """The height-only readback (ocean_read_height_async): DISP.y of one slice as float32[N][N], a
        quarter of read_async(TEX_DISP)'s bytes -- all GetWaterHeight reads (WaterBody.cs:195-209)."""
        nbytes = self.n * self.n * 4
        return Readback(self, (self.n, self.n), nbytes, "ocean_read_height_async",
                        lambda dst, req: self.lib.ocean_read_height_async(self._h, tile, cascade, dst, nbytes, req), buf)

    def set_readback_timing(self, enable: bool) -> None:
        """Time each new readback's device-to-host copy (Readback.copy_ms); off after create."""
        _check(self.lib.ocean_set_readback_timing(self._h, 1 if enable else 0), "ocean_set_readback_timing")

    def device_ptr(self, tex: int):
        p, b = ctypes.c_void_p(), ctypes.c_size_t()
        _check(self.lib.ocean_get_device_ptr(self._h, tex, ctypes.byref(p), ctypes.byref(b)), "ocean_get_device_ptr")
        return p.value, b.value

    def stream(self) -> int:
        s = ctypes.c_void_p()
        _check(self.lib.ocean_get_stream(self._h, ctypes.byref(s)), "ocean_get_stream")
        return s.value or 0

    def set_column_band(self, x_begin: int, x_count: int) -> None:
        """Restrict the fused step's stores, column transforms and fill to columns
        [x_begin, x_begin + x_count) (one GPU's share of a unit split over several)."""
        _check(self.lib.ocean_set_column_band(self._h, x_begin, x_count), "ocean_set_column_band")

    def set_column_parity(self, parity: int) -> None:
        """Compute only the columns x = 2m + parity (stored compact at texture column m < N/2):
        one of two GPUs sharing a unit with no duplicated row transform (ocean.h); -1 = off."""
        _check(self.lib.ocean_set_column_parity(self._h, parity), "ocean_set_column_parity")

    # -- timing ---------------------------------------------------------------
    def set_kernel_timing(self, enable: bool) -> None:
        _check(self.lib.ocean_set_kernel_timing(self._h, 1 if enable else 0), "ocean_set_kernel_timing")

    def kernel_stats(self, kind: int):
        ms, cnt = ctypes.c_double(), ctypes.c_longlong()
        _check(self.lib.ocean_kernel_stats(self._h, kind, ctypes.byref(ms), ctypes.byref(cnt)), "ocean_kernel_stats")
        return ms.value, cnt.value

    def kernel_name(self, kind: int) -> Optional[str]:
        """Demangled symbol of the kernel this context launched last in `kind` (0 pass A / rows,
        1 pass B / columns, 2 other), as rocprofv3 names it; None before any such launch."""
        buf = ctypes.create_string_buffer(1024)
        rc = self.lib.ocean_kernel_name(self._h, kind, buf, len(buf))
        if rc == E_STATE:
            return None
        _check(rc, "ocean_kernel_name")
        return buf.value.decode()

    def step_bytes(self):
        """(pass A, pass B) algorithmic HBM bytes of one step in this context's schedule."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self.lib.ocean_step_bytes(self._h, ctypes.byref(a), ctypes.byref(b)), "ocean_step_bytes")
        return a.value, b.value


class PinnedBuffer:
    """Pinned host memory from ocean_host_alloc, freed by release() (hipHostFree synchronizes the
    device, so a host that reads back every frame allocates its slots once and reuses them)."""

    def __init__(self, nbytes: int):
        self.lib = load_library()
        self.nbytes = nbytes
        self.ptr = ctypes.c_void_p()
        _check(self.lib.ocean_host_alloc(nbytes, ctypes.byref(self.ptr)), "ocean_host_alloc")

    def release(self) -> None:
        if self.ptr:
            self.lib.ocean_host_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.release()
        except Exception:
            pass


class Readback:
    """One readback request (any ocean_*_async entry) into pinned host memory: a caller's PinnedBuffer slot, or
    one of its own (freed by release()).  The OceanContext method that makes it knows the result's `shape` and
    `nbytes` and passes `call(dst, req)`, which issues its entry (named `where` in errors) with the pinned
    destination and the request handle's address and returns the entry's code."""

    def __init__(self, ctx: "OceanContext", shape: tuple, nbytes: int, where: str, call,
                 buf: Optional[PinnedBuffer] = None):
        self.lib = ctx.lib
        self.shape, self.nbytes = shape, nbytes
        self._h = ctypes.c_void_p()
        self.slot = buf
        self._own = buf is None
        if buf is None:
            # (an empty query or a grid beyond the limits still reaches the library, which refuses it)
            buf = PinnedBuffer(min(max(self.nbytes, 32), GRID_MAX_NODES * 32))
        elif buf.nbytes < self.nbytes:
            raise ValueError(f"pinned slot of {buf.nbytes} B < request {self.nbytes} B")
        self._pinned = buf
        self._buf = buf.ptr
        rc = call(self._buf, ctypes.byref(self._h))
        if rc != OK:
            if self._own:
                buf.release()
            self._pinned = None
            self._buf = ctypes.c_void_p()
            _check(rc, where)

    def done(self) -> bool:
        rc = self.lib.ocean_readback_status(self._h)
        if rc < 0:
            _check(rc, "ocean_readback_status")
        return rc == 1

    def wait(self) -> None:
        _check(self.lib.ocean_readback_wait(self._h), "ocean_readback_wait")

    def copy_ms(self) -> float:
        """The completed request's device-to-host copy duration (ocean_readback_copy_ms; the request must
        have been made with readback timing on: OceanContext.set_readback_timing)."""
        ms = ctypes.c_float()
        _check(self.lib.ocean_readback_copy_ms(self._h, ctypes.byref(ms)), "ocean_readback_copy_ms")
        return ms.value

    @property
    def data(self) -> np.ndarray:
        """A copy of the completed readback (waits if still pending)."""
        return self.view().copy()

    def view(self) -> np.ndarray:
        """The completed readback in place, read-only, without a copy (waits if still pending).  Valid
        while the pinned slot is neither released nor handed to another request."""
        self.wait()
        raw = (ctypes.c_float * (self.nbytes // 4)).from_address(self._buf.value)
        v = np.frombuffer(raw, np.float32).reshape(self.shape)
        v.flags.writeable = False
        return v

    def whitecaps(self):
        """A completed whitecaps_async request parsed: (T, records float32[W][8]) (waits if still pending)."""
        return OceanContext.parse_whitecaps(self.view())

    def spray(self):
        """A completed spray_step_async request parsed: (T, M, records float32[W][8]) (waits if still pending)."""
        return OceanContext.parse_spray(self.view())

    def release(self) -> None:
        if self._h:
            self.lib.ocean_readback_release(self._h)
            self._h = ctypes.c_void_p()
        if self._pinned is not None and self._own:
            self._pinned.release()
        self._pinned = None
        self._buf = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.release()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# Reference-shaped facade
# ---------------------------------------------------------------------------
@dataclass
class WaterCascade:
    """WaterCascade.cs:10-24 (defaults from the script)."""
    wavelength: float = 10.0
    cutoffHigh: float = 5.0
    cutoffLow: float = 0.0001
    swell: float = 0.4
    fade: float = 0.1

    def as_dict(self) -> dict:
        return dict(wavelength=self.wavelength, cutoff_low=self.cutoffLow, cutoff_high=self.cutoffHigh,
                    swell=self.swell, fade=self.fade)


@dataclass
class WaterHit:
    """What WaterBody.Raycast met (the RaycastHit of Unity's Physics.Raycast, for the water)."""
    distance: float       # along the normalised direction
    point: np.ndarray     # origin + distance * direction, float32[3]
    normal: np.ndarray    # the surface normal there, float32[3]
    foam: float
    submerged: bool       # the origin is under water: distance 0


@dataclass
class WaterBody:
    """WaterBody.cs public surface over the HIP library.

    Fields and defaults follow WaterBody.cs:10-33.  Awake() allocates and runs
    the initial spectrum (WaterBody.cs:211-256); CalculateWavesTexturesAtTime(t)
    is the per-frame path (WaterBody.cs:180-193, mip chains of DERIV and TURB
    included when `mips`); Update(t) additionally requests displacement slice 0
    asynchronously and, once a request completes, refreshes buoyancyData for
    GetWaterHeight (AsyncGPUReadback, WaterBody.cs:284-297, 195-209).
    `tiles` > 1 batches independent oceans (tile k uses seed + k).
    `readback`: "height" (default) requests only the .g channel GetWaterHeight reads
    (ocean_read_height_async, 4 B per texel: the reference's buoyancyData is private,
    WaterBody.cs:58, and that is its only reader); "rgba" requests the whole Color slice
    (16 B per texel) as the reference does.  GetWaterHeight returns the same bits in both.
    "probes" reads no slice back: SetProbes(points) names the world positions a consumer asks
    about (one per buoyant body), Update issues one ocean_query_surface_async per frame for them
    (probeMode, probeIterations) and ProbeHeights is the newest landed answer, 32 B per probe over
    the link.  In this mode GetWaterHeight keeps returning 0, as the reference does before its
    first readback, and buoyancyData stays None.
    """
    windSpeed: float = 1.0
    windDirection: tuple = (1.0, 1.0)
    gravity: float = 9.81
    fetch: float = 1.0
    depth: float = 4.0
    texturesSize: int = 256
    cascades: List[WaterCascade] = field(default_factory=lambda: [WaterCascade()])
    seed: int = 20251121
    tiles: int = 1
    displacementOnly: bool = False
    normals: bool = False
    mips: bool = True  # WaterBody.cs:228-229 creates DERIV / TURB with mip chains
    velocity: bool = False  # also keep the VELOCITY texture (F_VELOCITY): GetWaterVelocity
    device: int = 0
    noise: Optional[np.ndarray] = None  # explicit noise texture (tile 0), float32[N][N][2]
    readback: str = "height"  # "height" (DISP.y only), "rgba" (the whole displacement slice) or "probes"
    probeMode: int = QUERY_SURFACE  # readback "probes": ocean_query_surface_async's mode ...
    probeIterations: int = 4        # ... and fixed-point steps (0 with QUERY_REFERENCE)
    probeCapacity: int = 64         # probes the pinned ring is sized for at Awake (or the probes set by then, if more)

    def __post_init__(self):
        self._probes: Optional[np.ndarray] = None  # SetProbes' (world x, world z), float32[M][2]
        self._probe_cap = 0
        self._probe_view: Optional[np.ndarray] = None  # the last landed [M][8], a view of the held pinned slot
        self.ctx: Optional[OceanContext] = None
        self._buoy: Optional[np.ndarray] = None  # the last landed slice: a view of the held pinned slot
        self._readbacks: List[Readback] = []
        self._ring: List[PinnedBuffer] = []  # pinned readback slots, allocated in Awake
        self._idle: List[PinnedBuffer] = []
        self._held: Optional[PinnedBuffer] = None  # the pinned slot the last landed slice stays in
        self._buoy_copy: Optional[np.ndarray] = None  # buoyancyData's copy of the landed slice (first access)
        self.readback_copy_ms: Optional[List[float]] = None  # set to [] to log each landed copy's time
        self._timed = False  # the context's readback timing (on while readback_copy_ms is a list)

    def params(self) -> dict:
        return dict(wind_speed=self.windSpeed, wind_dir_x=self.windDirection[0], wind_dir_y=self.windDirection[1],
                    gravity=self.gravity, fetch=self.fetch, depth=self.depth)

    def Awake(self) -> "WaterBody":
        flags = (F_DISPLACEMENT_ONLY if self.displacementOnly else 0) | (F_NORMALS if self.normals else 0)
        if self.mips and not self.displacementOnly:
            flags |= F_MIPS
        if self.velocity:
            flags |= F_VELOCITY
        self.ctx = OceanContext(self.texturesSize, len(self.cascades), self.tiles, flags, self.device)
        self.ctx.set_params(self.params(), [c.as_dict() for c in self.cascades])
        if self.noise is not None:
            self.ctx.set_noise(0, self.noise)
            for t in range(1, self.tiles):
                self.ctx.set_noise(t, self.noise)
        else:
            self.ctx.generate_noise(self.seed)
        self.ctx.init_spectrum()
        if self.readback not in ("height", "rgba", "probes"):
            raise ValueError(f"readback must be 'height', 'rgba' or 'probes', got {self.readback!r}")
        self._timed = False
        if self.readback == "probes":
            self._probe_cap = max(int(self.probeCapacity), 0 if self._probes is None else len(self._probes), 1)
            if self._probe_cap > QUERY_MAX_POINTS:
                raise ValueError(f"at most {QUERY_MAX_POINTS} probes, got {self._probe_cap}")
            slice_bytes = self._probe_cap * 32
        else:
            slice_bytes = self.texturesSize * self.texturesSize * (4 if self.readback == "height" else 16)
        # one slot more than the requests in flight: the one the last landed slice stays in
        self._ring = [PinnedBuffer(slice_bytes) for _ in range(self._in_flight() + 1)]
        self._idle = list(self._ring)
        self._held = None
        return self

    def OnValidate(self) -> None:
        """Parameter change -> spectrum re-init (the commented OnValidate, WaterBody.cs:324-337);
        the foam accumulator carries over, as there."""
        self.ctx.set_params(self.params(), [c.as_dict() for c in self.cascades])
        self.ctx.init_spectrum()

    def CalculateWavesTexturesAtTime(self, time: float) -> None:
        self.ctx.step(time)

    # Bound on queued requests (the reference's queue is engine-managed); the ring holds one pinned slot
    # more, the one the last landed slice stays in.  Measured at cfg3 (tools/readback_probe.py): 2-4 in
    # flight keep the 16 MiB copies back to back beside the frames, 0.33 ms per frame; 8 in flight run
    # 0.82 ms per frame, each copy stretched to 2.5x its time alone.
    MAX_READBACKS_IN_FLIGHT = 4

    def _in_flight(self) -> int:
        """The bound in force: at least one request (water_body.h clamps the same way)."""
        return max(int(self.MAX_READBACKS_IN_FLIGHT), 1)

    def Update(self, time: float) -> None:
        """WaterBody.Update (WaterBody.cs:284-297): step, then issue a new AsyncGPUReadback
        request of displacement slice 0 EVERY frame (:288); requests complete in order and
        each completed one refreshes buoyancyData, as the reference's callback does (:292-295)."""
        self.CalculateWavesTexturesAtTime(time)
        self._poll_readbacks()
        if self.readback == "probes" and (self._probes is None or len(self._probes) == 0):
            return  # nobody asks: no request
        # at most MAX_READBACKS_IN_FLIGHT requests queued (the ring's extra slot holds the landed slice):
        # when full, wait for the oldest
        while self._readbacks and (len(self._readbacks) >= self._in_flight() or not self._idle):
            self._complete(self._readbacks.pop(0))
        if (self.readback_copy_ms is not None) != self._timed:  # copy times logged: timed requests
            self._timed = self.readback_copy_ms is not None
            self.ctx.set_readback_timing(self._timed)
        slot = self._idle.pop()
        try:
            if self.readback == "probes":
                # one query for every probe, in place of the slice request: 32 B per probe come back
                rb = self.ctx.query_surface_async(self._probes, 0, self.probeMode, self.probeIterations, slot)
            elif self.readback == "height":
                rb = self.ctx.read_height_async(0, 0, slot)
            else:
                rb = self.ctx.read_async(TEX_DISP, 0, 0, slot)
            rb.timed = self._timed
            self._readbacks.append(rb)
        except Exception:
            self._idle.append(slot)
            raise

    def _complete(self, rb: "Readback") -> None:
        # The reference copies every completed request out (request.GetData<Color>().ToArray(),
        # WaterBody.cs:295): Unity's NativeArray lives only inside the callback.  A pinned ring slot
        # outlives its request, so the landed slice stays in place instead: the slot leaves the
        # ring until the next completed readback replaces it, GetWaterHeight reads it there, and
        # buoyancyData copies it out only when a caller asks (16 MiB of host copy saved per frame
        # at 1024^2).
        view = rb.view()
        if self.readback_copy_ms is not None and rb.timed:
            self.readback_copy_ms.append(rb.copy_ms())
        slot = rb.slot
        rb.release()
        if self._held is not None:
            self._idle.append(self._held)
        self._held = slot
        if self.readback == "probes":  # buoyancyData is not filled: GetWaterHeight keeps returning 0
            self._probe_view = view
            return
        self._buoy = view
        self._buoy_copy = None

    def SetProbes(self, points) -> None:
        """The world positions Update asks about in readback "probes": [M][3] (x, y, z; x and z are
        used, as GetWaterHeight uses its worldPosition).  After Awake, at most the capacity the ring
        was sized for.  Takes effect at the next Update; answers already in flight keep their own M."""
        p = np.asarray(points, np.float32).reshape(-1, 3)
        if self.ctx is not None and self.readback == "probes" and len(p) > self._probe_cap:
            raise ValueError(f"{len(p)} probes > the capacity {self._probe_cap} the ring was sized for at Awake")
        self._probes = np.ascontiguousarray(p[:, [0, 2]])

    @property
    def ProbeResults(self) -> Optional[np.ndarray]:
        """The newest landed query, float32[M][8] as ocean_query_surface returns it (a copy), or None
        before the first lands."""
        return None if self._probe_view is None else np.array(self._probe_view)

    @property
    def ProbeHeights(self) -> Optional[np.ndarray]:
        """The newest landed heights, float32[M] in SetProbes' order, or None before the first lands."""
        return None if self._probe_view is None else np.array(self._probe_view[:, 0])

    @property
    def buoyancyData(self) -> Optional[np.ndarray]:
        """The last landed displacement slice 0 (WaterBody.cs:295's array), read-only: [y][x] heights
        (.g) with readback "height", [y][x][rgba] with "rgba".
        The slice is copied out of its pinned slot once, on the first access after it lands, and the
        same array is returned until the next readback lands: per-sample indexing costs no copy, as
        reading the reference's field does not."""
        if self._buoy is None:
            return None
        if self._buoy_copy is None:
            self._buoy_copy = np.array(self._buoy)
            self._buoy_copy.flags.writeable = False
        return self._buoy_copy

    def _poll_readbacks(self) -> None:
        while self._readbacks and self._readbacks[0].done():
            self._complete(self._readbacks.pop(0))

    def WaitForReadback(self) -> None:
        """Block until every pending readback has landed (the last one in buoyancyData)."""
        while self._readbacks:
            self._complete(self._readbacks.pop(0))

    def GetWaterHeight(self, worldPosition) -> float:
        """WaterBody.cs:195-209, including its quirk of mapping world x,z over
        [-texturesSize/2, texturesSize/2] instead of the cascade length."""
        if self._buoy is None:
            return 0.0
        n = self.texturesSize

        def inv_lerp(a, b, v):
            return 0.0 if a == b else min(max((v - a) / (b - a), 0.0), 1.0)
        u = inv_lerp(-(n // 2), n // 2, float(worldPosition[0]))
        v = inv_lerp(-(n // 2), n // 2, float(worldPosition[2]))
        x = min(max(int(u * n), 0), n - 1)
        y = min(max(int(v * n), 0), n - 1)
        return float(self._buoy[y, x] if self.readback == "height" else self._buoy[y, x, 1])

    def SampleWorld(self, points, tile: int = 0) -> np.ndarray:
        """What Water.shader reads at world positions (x, z, lod): summed displacement,
        derivatives, turbulence and the normal (Water.shader:314-348)."""
        return self.ctx.sample_world(np.asarray(points, np.float32).reshape(-1, 3), tile)

    def SurfaceGrid(self, x0: float, z0: float, dx: float, dz: float, nx: int, ny: int, mode: int = GRID_SURFACE,
                    iterations: Optional[int] = None, lod: float = 0.0, tile: int = 0) -> np.ndarray:
        """The surface over a regular grid (OceanContext.surface_grid): MeshGenerator's plane displaced as
        the domain stage of Water.shader does (GRID_VERTICES), the Eulerian surface or a height map."""
        return self.ctx.surface_grid(x0, z0, dx, dz, nx, ny, mode, iterations, lod, tile)

    def Buoyancy(self, hull, bodies, iterations: int = 4, mode: int = QUERY_SURFACE, tile: int = 0) -> np.ndarray:
        """BuoyantObject.FixedUpdate's lookup for M bodies of P probes each (OceanContext.body_buoyancy): the
        displaced volume, where it acts and the water plane under every hull, float32[M][8]."""
        return self.ctx.body_buoyancy(hull, bodies, iterations, mode, tile)

    def Hydrostatics(self, vertices, triangles, bodies, iterations: int = 4, tile: int = 0) -> np.ndarray:
        """The hydrostatic force, torque, wetted and waterplane area of M bodies that share a triangle mesh
        (OceanContext.body_hydrostatics), float32[M][16].  The reference has no counterpart: its BuoyantObject is one
        probe."""
        return self.ctx.body_hydrostatics(vertices, triangles, bodies, iterations, tile)

    def Dynamics(self, hull, bodies, motion, iterations: int = 4, mode: int = QUERY_SURFACE, law: int = DRAG_LINEAR,
                 tile: int = 0) -> np.ndarray:
        """Buoyancy's records with the drag against the water's own velocity beside them, float32[M][16]
        (OceanContext.body_dynamics; `velocity=True`).  The reference drags against still water
        (BuoyantObject.FixedUpdate: -rb.velocity * drag)."""
        return self.ctx.body_dynamics(hull, bodies, motion, iterations, mode, law, tile)

    def StepBodies(self, hull, state, props, step, substeps: int = 1, iterations: int = 4, mode: int = QUERY_SURFACE,
                   law: int = DRAG_LINEAR, tile: int = 0) -> np.ndarray:
        """BuoyantObject.FixedUpdate for M bodies of P probes each, `substeps` fixed updates against this frame's
        water in one launch (OceanContext.body_step; `velocity=True`): float32[M][32], the next call's `state`."""
        return self.ctx.body_step(hull, state, props, step, substeps, iterations, mode, law, tile)

    def GetWaterVelocity(self, worldPosition, iterations: int = 4, tile: int = 0) -> np.ndarray:
        """The velocity (x, y, z) of the water particle on the surface above worldPosition (x and z are used, as
        GetWaterHeight uses them), float32[3]: what drag relative to the water and particle advection need
        (OceanContext.query_velocity; `velocity=True`).  The reference has no counterpart: its BuoyantObject
        drags against still water.  Blocking, and exact at the last step's time."""
        q = np.float32([[worldPosition[0], worldPosition[2]]])
        return self.ctx.query_velocity(q, tile, iterations)[0, :3].copy()

    def Raycast(self, origin, direction, max_distance: float, iterations: int = 4, steps: int = 64, refine: int = 8,
                tile: int = 0) -> Optional["WaterHit"]:
        """Physics.Raycast for the water (OceanContext.raycast): the ray from `origin` along `direction`
        (normalised here, as Unity does) searched over [0, max_distance] in `steps` intervals.  Returns None when
        it stays above the water, else a WaterHit: distance, point, normal, foam, and `submerged` when the
        origin itself is under water (distance 0).  The reference has no counterpart.  Blocking."""
        o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
        norm = float(np.sqrt((d * d).sum()))
        if not norm > 0.0:
            raise ValueError("direction must be non-zero")
        d = d / norm
        ray = np.float32([[o[0], o[1], o[2], d[0], d[1], d[2], 0.0, max_distance]])
        rec = self.ctx.raycast(ray, tile, iterations, steps, refine)[0]
        if int(rec[3]) == RAY_MISS:
            return None
        point = ray[0, :3] + rec[0] * ray[0, 3:6]  # fp32: pos(t*) of ocean.h
        return WaterHit(float(rec[0]), point, rec[4:7].copy(), float(rec[7]), int(rec[3]) == RAY_SUBMERGED)

    def Camera(self, eye, target, width: int, height: int, fov_y: float = 1.0, max_distance: float = 2000.0,
               mode: int = CAMERA_COLOR, material=None, up=(0.0, 1.0, 0.0), iterations: int = 4, steps: int = 64,
               refine: int = 8, tile: int = 0) -> np.ndarray:
        """What a camera at `eye` looking at `target` sees of the water (OceanContext.camera over look_at_camera;
        colour mode shades with `material`, material()'s defaults when None): the headless stand-in for the
        reference's renderer, whose fragment stage (Water.shader:336-374) this evaluates.  Blocking."""
        if mode == CAMERA_COLOR and material is None:
            material = _material()
        cam = look_at_camera(eye, target, up, fov_y, width, height, 0.0, max_distance)
        return self.ctx.camera(cam, width, height, mode, material, tile, iterations, steps, refine)

    def camera_bodies(self, eye, target, width: int, height: int, bodies, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5),
                      paint=(0.8, 0.8, 0.8, 1.0), fov_y: float = 1.0, max_distance: float = 2000.0,
                      mode: int = CAMERA_COLOR, material=None, up=(0.0, 1.0, 0.0), iterations: int = 4, steps: int = 64,
                      refine: int = 8, tile: int = 0) -> np.ndarray:
        """Camera() with the boxes of `bodies` in the picture (OceanContext.camera_bodies over look_at_camera): what a
        vessel's camera or lidar sees of the sea and of the hulls StepBodies moves."""
        if material is None and mode in (CAMERA_COLOR, CAMERA_COLOR | CAMERA_SKY_LUT):
            material = _material()
        cam = look_at_camera(eye, target, up, fov_y, width, height, 0.0, max_distance)
        return self.ctx.camera_bodies(cam, width, height, bodies, box, paint, mode, material, tile, iterations, steps, refine)

    def camera_scene(self, eye, target, width: int, height: int, bodies, box=(-0.5, -0.5, -0.5, 0.5, 0.5, 0.5),
                     paint=(0.8, 0.8, 0.8, 1.0), optics=(0.0, 0.0, 0.0, 0.5, 0.2, 100.0), fov_y: float = 1.0,
                     max_distance: float = 2000.0, mode: int = CAMERA_COLOR, material=None, up=(0.0, 1.0, 0.0),
                     iterations: int = 4, steps: int = 64, refine: int = 8, tile: int = 0) -> np.ndarray:
        """camera_bodies() with the hulls' shadows on the water, their reflections in it and their submerged parts
        through it (OceanContext.camera_scene over look_at_camera)."""
        if material is None:
            material = _material()
        cam = look_at_camera(eye, target, up, fov_y, width, height, 0.0, max_distance)
        return self.ctx.camera_scene(cam, width, height, bodies, box, paint, optics, mode, material, tile, iterations,
                                     steps, refine)

    def Whitecaps(self, threshold: float, x0: float, z0: float, dx: float, dz: float, nx: int, ny: int,
                  capacity: int = 4096, lod: float = 0.0, tile: int = 0):
        """Where the sea is breaking (OceanContext.whitecaps): the nodes of the grid whose foam reaches `threshold`,
        as (T, float32[W][8]): spawn points for spray and foam particles with the water's velocity beside them
        (`velocity=True`).  The reference has the foam only as a shading term (Water.shader:343).  Blocking."""
        return self.ctx.whitecaps(threshold, x0, z0, dx, dz, nx, ny, capacity, lod, tile)

    def Spray(self, spray, pool, emitters=None, substeps: int = 1, iterations: int = 2, tile: int = 0):
        """Spray particles (OceanContext.spray_step): the pool float32[capacity + 1][8] and one fresh particle per
        record of the whitecap list `emitters` take `substeps` substeps against this frame's water; those that fall
        back into the sea or outlive `life` are retired -> (T, M, float32[W][8]) and the stepped pool itself, which
        is the next call's `pool`.  The reference has no particles.  Blocking."""
        out = self.ctx.spray_step(spray, pool, emitters, substeps, iterations, tile)
        return OceanContext.parse_spray(out) + (out,)

    def SurfaceBounds(self, tile: int = 0) -> np.ndarray:
        """(min xyz, max xyz) float32[2][3] of the cascade-summed displacement, from the per-cascade records
        (OceanContext.surface_bounds): what a renderer adds to a patch's corners for its bounding box."""
        rec = self.ctx.surface_bounds(tile)
        return np.stack([rec[:, 0:3].sum(axis=0, dtype=np.float32), rec[:, 4:7].sum(axis=0, dtype=np.float32)])

    # texture-out contract (material properties, WaterBody.cs:277-281)
    def DisplacementsTextures(self, tile: int = 0) -> np.ndarray:
        return self.ctx.read_all(TEX_DISP, tile)

    def DerivativesTextures(self, tile: int = 0) -> np.ndarray:
        return self.ctx.read_all(TEX_DERIV, tile)

    def TurbulenceTextures(self, tile: int = 0) -> np.ndarray:
        return self.ctx.read_all(TEX_TURB, tile)

    def OnDisable(self) -> None:
        for rb in self._readbacks:
            rb.release()
        self._readbacks = []
        if self._buoy is not None:  # the last landed slice outlives the pinned ring
            self._buoy = self.buoyancyData
        if self._probe_view is not None:
            self._probe_view = np.array(self._probe_view)
        for b in self._ring:
            b.release()
        self._ring, self._idle, self._held = [], [], None
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None


class IFFT:
    """IFFT.cs operator: InverseFastFourierTransform on a plane texture array of a context."""

    def __init__(self, ctx: OceanContext):
        self.ctx = ctx

    def InverseFastFourierTransform(self, plane: int) -> None:
        """plane in 0..3 (DxDz, DyDxz, DyxDyz, DxxDzz): in-place, all tiles and cascades."""
        self.ctx.ifft2d(1 << plane)


def scene_water_body(n: int = 512, n_cascades: int = 3, **kw) -> WaterBody:
    """The reference scene (Assets/Scenes/Waves.unity:1305-1322, cascades :1431-1435, :470-474,
    :1249-1253, 4th unreferenced cascade :1572-1576)."""
    cs = [WaterCascade(1530, 1e12, 1e-10, 0.4, 0.1), WaterCascade(1000, 1e7, 1e-7, 0.3, 0.2),
          WaterCascade(201, 1e6, 1e-5, 0.1, 0.1), WaterCascade(34, 10, 0.001, 0.4, 0.1)][:n_cascades]
    return WaterBody(windSpeed=8.0, windDirection=(1.0, -1.0), gravity=9.81, fetch=50000.0, depth=2560.0,
                     texturesSize=n, cascades=cs, **kw)
