"""libyafaray_amd — Python host mirror of libYafaRay's C API over the MI355X core (libyafaray4.so).

The shared library is the product: every call below is a thin ctypes forward to an extern "C"
symbol of include/yafaray_c_api.h (reference include/public_api/yafaray_c_api.h:53-130) or of the
MI355X extensions in include/yafaray_amd.h.  There is no Python or CPU fallback: importing works
without a GPU (so the C ABI can be inspected), but rendering / tracing raise if the HIP path
fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YAFARAY_AMD_LIB") or os.path.join(HERE, "libyafaray4.so")

# enums (yafaray_c_api.h)
LOG_MUTE, LOG_ERROR, LOG_WARNING, LOG_PARAMS, LOG_INFO, LOG_VERBOSE, LOG_DEBUG = range(7)
CONSOLE_HIDDEN, CONSOLE_NORMAL = 0, 1

PutPixelCb = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                         C.c_void_p)
FlushAreaCb = C.CFUNCTYPE(None, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
FlushCb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)
NotifyViewCb = C.CFUNCTYPE(None, C.c_char_p, C.c_void_p)
NotifyLayerCb = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p)
ProgressCb = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_char_p, C.c_void_p)
LoggerCb = C.CFUNCTYPE(None, C.c_int, C.c_long, C.c_char_p, C.c_char_p, C.c_void_p)


class Stats(C.Structure):
    _fields_ = [("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("node_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("samples", C.c_uint64), ("build_seconds", C.c_double),
                ("render_seconds", C.c_double), ("trace_kernel_ms", C.c_double), ("trace_launches", C.c_uint64),
                ("bvh_nodes", C.c_uint32), ("bvh_depth", C.c_uint32), ("scene_in_lds", C.c_uint32),
                ("bvh_width", C.c_uint32), ("trace_grid", C.c_uint32), ("shade_grid", C.c_uint32),
                ("trace_block", C.c_uint32), ("stack_depth", C.c_uint32), ("shade_kernel_ms", C.c_double),
                ("nee_kernel_ms", C.c_double), ("photons", C.c_uint64), ("photon_seconds", C.c_double),
                ("photon_shoot_seconds", C.c_double), ("photon_tree_seconds", C.c_double), ("gather_visits", C.c_uint64),
                ("caustic_photons", C.c_uint64), ("radiance_points", C.c_uint64), ("radiance_photons", C.c_uint64),
                ("fg_thin_seconds", C.c_double), ("fg_radiance_seconds", C.c_double), ("fg_thin_rounds", C.c_int64),
                ("gather_queries", C.c_uint64), ("gather_photons", C.c_uint64),
                ("photon_maps_mode", C.c_int32), ("reserved0", C.c_int32),
                ("gather_accepts", C.c_uint64), ("gather_overflows", C.c_uint64),
                ("photon_paths_traced", C.c_uint64), ("photon_slots", C.c_uint64),
                ("fg_paths", C.c_uint64), ("fg_lookups", C.c_uint64), ("fg_nearest_visits", C.c_uint64),
                ("pregather_visits", C.c_uint64), ("pregather_photons", C.c_uint64), ("pkd_split_level", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def build(quiet: bool = True) -> str:
    """Compile libyafaray4.so for gfx950 in-tree (libyafaray_amd/csrc/Makefile)."""
    import subprocess
    out = subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j8"], capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("libyafaray4.so build failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])
    if not quiet:
        print(out.stdout)
    return LIB_PATH


def lib():
    """Load libyafaray4.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run libyafaray_amd.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        vp, cp, i, d, f, b = C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_float, C.c_int
        sig = {
            "yafaray_createInterface": (vp, [i, cp, C.c_void_p, vp, i]),
            "yafaray_destroyInterface": (None, [vp]),
            "yafaray_createScene": (None, [vp]),
            "yafaray_getSceneFilmWidth": (i, [vp]),
            "yafaray_getSceneFilmHeight": (i, [vp]),
            "yafaray_startGeometry": (b, [vp]),
            "yafaray_endGeometry": (b, [vp]),
            "yafaray_endObject": (b, [vp]),
            "yafaray_addVertex": (i, [vp, d, d, d]),
            "yafaray_addVertexWithOrco": (i, [vp, d, d, d, d, d, d]),
            "yafaray_addTriangle": (b, [vp, i, i, i]),
            "yafaray_addTriangleWithUv": (b, [vp, i, i, i, i, i, i]),
            "yafaray_addUv": (i, [vp, f, f]),
            "yafaray_addNormal": (None, [vp, d, d, d]),
            "yafaray_smoothMesh": (b, [vp, cp, d]),
            "yafaray_addInstance": (b, [vp, cp] + [f] * 16),
            "yafaray_addInstanceArray": (b, [vp, cp, C.POINTER(C.c_float)]),
            "yafaray_amd_getPrimitives": (i, [vp, i, i, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
            "yafaray_clearAll": (None, [vp]),
            "yafaray_getNextFreeId": (C.c_uint, [vp]),
            "yafaray_createImage": (vp, [vp, cp]),
            "yafaray_setImageColor": (b, [vp, i, i, f, f, f, f]),
            "yafaray_getImageColor": (b, [vp, i, i, C.POINTER(f), C.POINTER(f), C.POINTER(f), C.POINTER(f)]),
            "yafaray_paramsSetMatrix": (None, [vp, cp] + [f] * 16 + [b]),
            "yafaray_paramsSetVector": (None, [vp, cp, d, d, d]),
            "yafaray_paramsSetString": (None, [vp, cp, cp]),
            "yafaray_paramsSetBool": (None, [vp, cp, b]),
            "yafaray_paramsSetInt": (None, [vp, cp, i]),
            "yafaray_paramsSetFloat": (None, [vp, cp, d]),
            "yafaray_paramsSetColor": (None, [vp, cp, f, f, f, f]),
            "yafaray_paramsClearAll": (None, [vp]),
            "yafaray_paramsPushList": (None, [vp]),
            "yafaray_paramsEndList": (None, [vp]),
            "yafaray_setCurrentMaterial": (None, [vp, cp]),
            "yafaray_createObject": (b, [vp, cp]),
            "yafaray_createLight": (b, [vp, cp]),
            "yafaray_createTexture": (b, [vp, cp]),
            "yafaray_createMaterial": (b, [vp, cp]),
            "yafaray_createCamera": (b, [vp, cp]),
            "yafaray_createBackground": (b, [vp, cp]),
            "yafaray_createIntegrator": (b, [vp, cp]),
            "yafaray_createRenderView": (b, [vp, cp]),
            "yafaray_createOutput": (b, [vp, cp]),
            "yafaray_setRenderPutPixelCallback": (None, [vp, PutPixelCb, vp]),
            "yafaray_setRenderFlushAreaCallback": (None, [vp, FlushAreaCb, vp]),
            "yafaray_setRenderHighlightAreaCallback": (None, [vp, FlushAreaCb, vp]),
            "yafaray_setRenderFlushCallback": (None, [vp, FlushCb, vp]),
            "yafaray_setRenderNotifyViewCallback": (None, [vp, NotifyViewCb, vp]),
            "yafaray_setRenderNotifyLayerCallback": (None, [vp, NotifyLayerCb, vp]),
            "yafaray_setupRender": (None, [vp]),
            "yafaray_render": (None, [vp, ProgressCb, vp, i]),
            "yafaray_defineLayer": (None, [vp]),
            "yafaray_setConsoleVerbosityLevel": (None, [vp, i]),
            "yafaray_setLogVerbosityLevel": (None, [vp, i]),
            "yafaray_cancelRendering": (None, [vp]),
            "yafaray_setInputColorSpace": (None, [vp, cp, f]),
            "yafaray_getVersionString": (vp, []),
            "yafaray_deallocateCharPointer": (None, [vp]),
            "yafaray_amd_addVertices": (i, [vp, C.POINTER(C.c_double), i]),
            "yafaray_amd_addTriangles": (b, [vp, C.POINTER(C.c_int), i]),
            "yafaray_amd_buildAccelerator": (b, [vp]),
            "yafaray_amd_traceClosest": (b, [vp, C.POINTER(C.c_float), i, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
            "yafaray_amd_traceShadow": (b, [vp, C.POINTER(C.c_float), i, C.POINTER(C.c_int)]),
            "yafaray_amd_traceQueued": (b, [vp, C.POINTER(C.c_float), i, C.POINTER(C.c_float), i, i, i, C.POINTER(C.c_float),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
            "yafaray_amd_thinRadPoints": (b, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i, f, i, C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_int), C.POINTER(C.c_int)]),
            "yafaray_amd_aaNextPass": (b, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i, i, i, i, i, f, i, i, f, i, i,
                                           C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32)]),
            "yafaray_amd_queryPhotons": (b, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             i, i, f, i, i, i, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_ulonglong)]),
            "yafaray_amd_getFilm": (b, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
            "yafaray_amd_getFilmDevice": (b, [vp, vp, i, i]),
            "yafaray_amd_getLayerCount": (i, [vp]),
            "yafaray_amd_getLayerName": (cp, [vp, i]),
            "yafaray_amd_getFilmLayer": (b, [vp, cp, C.POINTER(C.c_float)]),
            "yafaray_getLayersTable": (vp, [vp]),
            "yafaray_amd_setTileRowShard": (None, [vp, i, i]),
            "yafaray_amd_setRowBandShard": (None, [vp, i, i]),
            "yafaray_amd_setRowBandRange": (None, [vp, i, i, i]),
            "yafaray_amd_getOwnedRows": (i, [vp, C.POINTER(C.c_int), i]),
            "yafaray_amd_renderQuiet": (b, [vp]),
            "yafaray_amd_getStats": (None, [vp, C.POINTER(Stats)]),
            "yafaray_amd_buildInfo": (cp, []),
            "yafaray_amd_getGroupReport": (C.c_size_t, [vp, C.c_char_p, C.c_size_t]),
            "yafaray_amd_getStatsEx": (C.c_size_t, [vp, C.POINTER(Stats), C.c_size_t]),
            "yafaray_amd_setDeviceGroup": (b, [vp, i, C.POINTER(C.c_int)]),
            "yafaray_amd_getDeviceGroupSize": (i, [vp]),
            "yafaray_amd_packBand": (i, [C.POINTER(C.c_float), i, i, i, C.POINTER(C.c_int), i, i, C.POINTER(C.c_float)]),
            "yafaray_amd_unpackBands": (i, [C.POINTER(C.c_float), i, i, i, C.POINTER(C.c_int), i, i, C.POINTER(C.c_float)]),
            "yafaray_amd_buildPhotonTree": (b, [C.POINTER(C.c_float), i, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
            "yafaray_amd_buildPhotonTreeMember": (b, [C.POINTER(C.c_float), i, i, i, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
            "yafaray_amd_photonTreeSegments": (None, [C.c_uint, i, i, i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                      C.POINTER(C.c_uint32)]),
            "yafaray_amd_setChunkSlots": (None, [vp, i]),
            "yafaray_amd_setProfileKernels": (None, [vp, b]),
            "yafaray_amd_setTraceStats": (None, [vp, b]),
            "yafaray_amd_lastError": (cp, [vp]),
            "yafaray_amd_getRenderGroupId": (i, [vp, i]),
            "yafaray_amd_setRenderGroup": (b, [vp, i, i, vp, i]),
            "yafaray_amd_rebalanceBands": (i, [C.POINTER(C.c_int), i, C.POINTER(C.c_double), i, C.POINTER(C.c_int)]),
            "yafaray_amd_getKernelTimes": (i, [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64), i]),
        }
        # LIBYAFARAY_AMD_1.4 / 1.7 (variant builds of older sources lack them)
        # ... / 1.8: the render layers
        optional = {"yafaray_amd_buildInfo", "yafaray_amd_getGroupReport", "yafaray_amd_getPrimitives",
                    "yafaray_amd_getLayerCount", "yafaray_amd_getLayerName", "yafaray_amd_getFilmLayer"}
        for name, (res, args) in sig.items():
            if name in optional and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def build_info() -> str:
    """The library's build flags (yafaray_amd_buildInfo): device arch + extra flags, host compiler."""
    L = lib()
    return L.yafaray_amd_buildInfo().decode() if hasattr(L, "yafaray_amd_buildInfo") else "unknown (library before LIBYAFARAY_AMD_1.4)"


def lib_sha256() -> str:
    """sha256 of the loaded libyafaray4.so (bench.py prints it with build_info)."""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def version() -> str:
    L = lib()
    p = L.yafaray_getVersionString()
    s = C.cast(p, C.c_char_p).value.decode()
    L.yafaray_deallocateCharPointer(p)
    return s


def _b(s):
    return s.encode() if isinstance(s, str) else s


class Interface:
    """One yafaray_Interface_t.  Method names are the C API's without the `yafaray_` prefix."""

    def __init__(self, console=CONSOLE_HIDDEN, verbosity=LOG_WARNING):
        self.L = lib()
        self.h = self.L.yafaray_createInterface(0, None, None, None, console)
        self.L.yafaray_setConsoleVerbosityLevel(self.h, verbosity)
        self._keep = []

    def close(self):
        if self.h:
            self.L.yafaray_destroyInterface(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- generic forwarding for simple calls ---
    def __getattr__(self, name):
        fn = getattr(lib(), "yafaray_" + name, None)
        if fn is None:
            raise AttributeError(name)

        def call(*args):
            return fn(self.h, *[_b(a) for a in args])
        return call

    # --- images (the handle is the first argument, not the interface) ---
    def setImageColor(self, image, x, y, r, g, b, a):
        return self.L.yafaray_setImageColor(image, x, y, r, g, b, a)

    def getImageColor(self, image, x, y):
        c = [C.c_float() for _ in range(4)]
        ok = self.L.yafaray_getImageColor(image, x, y, *[C.byref(v) for v in c])
        return tuple(v.value for v in c) if ok else None

    # --- bulk geometry (extensions) ---
    def addVertices(self, xyz):
        a = np.ascontiguousarray(xyz, np.float64).reshape(-1)
        return self.L.yafaray_amd_addVertices(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), len(a) // 3)

    def addTriangles(self, abc):
        a = np.ascontiguousarray(abc, np.int32).reshape(-1)
        if not self.L.yafaray_amd_addTriangles(self.h, a.ctypes.data_as(C.POINTER(C.c_int)), len(a) // 3):
            raise RuntimeError(self.last_error())

    # --- object instances ---
    def addInstance(self, base_name, m):
        """yafaray_addInstance: `m` is obj_to_world, (3, 4) or (4, 4) row-major (row 3 is never read)."""
        m = np.asarray(m, np.float32)
        if m.shape == (3, 4):
            m = np.concatenate([m, np.asarray([[0, 0, 0, 1]], np.float32)])
        return bool(self.L.yafaray_addInstance(self.h, _b(base_name), *[float(x) for x in m.reshape(16)]))

    def addInstanceArray(self, base_name, m):
        """yafaray_addInstanceArray: the same through a float[4][4]."""
        m = np.ascontiguousarray(m, np.float32)
        if m.shape == (3, 4):
            m = np.ascontiguousarray(np.concatenate([m, np.asarray([[0, 0, 0, 1]], np.float32)]))
        return bool(self.L.yafaray_addInstanceArray(self.h, _b(base_name), m.ctypes.data_as(C.POINTER(C.c_float))))

    def primitives(self, first=0, count=None):
        """The built scene's primitives [first, first + count) as the device holds them (yafaray_amd_getPrimitives):
        {"verts": (n, 3, 3), "ng": (n, 3), "vnormals": (n, 3, 3), "material": (n,)}.  count None: to the end."""
        fp = C.POINTER(C.c_float)
        if count is None:
            total = self.L.yafaray_amd_getPrimitives(self.h, 0, 0, None, None, None, None)
            if total < 0:
                raise RuntimeError("getPrimitives failed: " + self.last_error())
            count = total - first
        v = np.empty((count, 3, 3), np.float32)
        ng = np.empty((count, 3), np.float32)
        vn = np.empty((count, 3, 3), np.float32)
        mat = np.empty(count, np.int32)
        if self.L.yafaray_amd_getPrimitives(self.h, int(first), int(count), v.ctypes.data_as(fp), ng.ctypes.data_as(fp),
                                            vn.ctypes.data_as(fp), mat.ctypes.data_as(C.POINTER(C.c_int))) < 0:
            raise RuntimeError("getPrimitives failed: " + self.last_error())
        return {"verts": v, "ng": ng, "vnormals": vn, "material": mat}

    def last_error(self) -> str:
        e = self.L.yafaray_amd_lastError(self.h)
        return e.decode() if e else ""

    # --- render ---
    def render(self, progress=None, put_pixel=None, flush_area=None, flush=None, highlight_area=None, put_layer_pixel=None,
               notify_layer=None):
        """put_pixel(x, y, r, g, b, a) sees the combined layer; put_layer_pixel(layer, x, y, r, g, b, a) every exported
        layer with the layer name the library reports; notify_layer(layer, exported_name, width, height, channels)."""
        # every callback is (re)registered, a missing one as NULL (an empty CFUNCTYPE instance): the library
        # keeps the pointers between renders, and the previous render's ctypes thunks are released below
        # (self._keep) — a render without a callback after one with it called a freed thunk
        cbs = []
        cb = FlushAreaCb(lambda v, aid, x0, y0, x1, y1, d: highlight_area(aid, x0, y0, x1, y1)) if highlight_area is not None else FlushAreaCb()
        self.L.yafaray_setRenderHighlightAreaCallback(self.h, cb, None)
        cbs.append(cb)
        def _put(v, l, x, y, r, g, b, a, d):
            if put_layer_pixel is not None:
                put_layer_pixel(l.decode(), x, y, r, g, b, a)
            if put_pixel is not None and l == b"combined":
                put_pixel(x, y, r, g, b, a)
        cb = PutPixelCb(_put) if (put_pixel is not None or put_layer_pixel is not None) else PutPixelCb()
        self.L.yafaray_setRenderPutPixelCallback(self.h, cb, None)
        cbs.append(cb)
        cb = FlushAreaCb(lambda v, aid, x0, y0, x1, y1, d: flush_area(aid, x0, y0, x1, y1)) if flush_area is not None else FlushAreaCb()
        self.L.yafaray_setRenderFlushAreaCallback(self.h, cb, None)
        cbs.append(cb)
        cb = (NotifyLayerCb(lambda l, e, w, h, c, d: notify_layer(l.decode(), (e or b"").decode(), w, h, c)) if notify_layer is not None
              else NotifyLayerCb())
        self.L.yafaray_setRenderNotifyLayerCallback(self.h, cb, None)
        cbs.append(cb)
        cb = FlushCb(lambda v, d: flush()) if flush is not None else FlushCb()
        self.L.yafaray_setRenderFlushCallback(self.h, cb, None)
        cbs.append(cb)
        pcb = ProgressCb(lambda t, dn, tag, d: progress(t, dn) if progress else None)
        cbs.append(pcb)
        self._keep = cbs
        before = self.last_error()
        self.L.yafaray_render(self.h, pcb, None, CONSOLE_HIDDEN)
        err = self.last_error()
        if err and err != before:
            raise RuntimeError("yafaray_render failed: " + err)

    def render_quiet(self):
        if not self.L.yafaray_amd_renderQuiet(self.h):
            raise RuntimeError("render failed: " + self.last_error())

    def film(self):
        w, h = self.L.yafaray_getSceneFilmWidth(self.h), self.L.yafaray_getSceneFilmHeight(self.h)
        rgba = np.empty((h, w, 4), np.float32)
        wt = np.empty((h, w), np.float32)
        if not self.L.yafaray_amd_getFilm(self.h, rgba.ctypes.data_as(C.POINTER(C.c_float)),
                                          wt.ctypes.data_as(C.POINTER(C.c_float))):
            raise RuntimeError("no film: " + self.last_error())
        return rgba, wt

    def layers(self):
        """The type names of the layers the next render produces, "combined" first (yafaray_amd_getLayerName)."""
        n = int(self.L.yafaray_amd_getLayerCount(self.h))
        return [self.L.yafaray_amd_getLayerName(self.h, k).decode() for k in range(n)]

    def film_layer(self, name):
        """One layer of the last render's film, (h, w, 4) float32, as put-pixel reports it (yafaray_amd_getFilmLayer)."""
        w, h = self.L.yafaray_getSceneFilmWidth(self.h), self.L.yafaray_getSceneFilmHeight(self.h)
        rgba = np.empty((h, w, 4), np.float32)
        if not self.L.yafaray_amd_getFilmLayer(self.h, _b(name), rgba.ctypes.data_as(C.POINTER(C.c_float))):
            raise RuntimeError(f"no film layer '{name}': " + self.last_error())
        return rgba

    def layers_table(self) -> str:
        """yafaray_getLayersTable: one line per exported layer."""
        p = self.L.yafaray_getLayersTable(self.h)
        s = C.cast(p, C.c_char_p).value.decode()
        self.L.yafaray_deallocateCharPointer(p)
        return s

    def stats(self) -> dict:
        s = Stats()
        self.L.yafaray_amd_getStatsEx(self.h, C.byref(s), C.sizeof(s))
        return s.as_dict()

    def set_device_group(self, members, devices=None):
        """yafaray_amd_setDeviceGroup: `members` renderers of this process share the film (row bands);
        devices[m] = member m's HIP device (None: current device + m modulo the visible devices, so
        several logical members can share one GPU).  members <= 0: back to the "gpus" parameter."""
        arr = None
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        if not self.L.yafaray_amd_setDeviceGroup(self.h, int(members), arr):
            raise RuntimeError("setDeviceGroup failed: " + self.last_error())

    def device_group_size(self) -> int:
        return int(self.L.yafaray_amd_getDeviceGroupSize(self.h))

    def group_report(self) -> dict:
        """How the last render was split across GPUs (yafaray_amd_getGroupReport): mode, devices, the
        peer-access matrix, the band copy path, band bounds and each member's render time."""
        import json
        n = int(self.L.yafaray_amd_getGroupReport(self.h, None, 0))
        if n <= 0:
            raise RuntimeError("getGroupReport failed: " + self.last_error())
        buf = C.create_string_buffer(n)
        self.L.yafaray_amd_getGroupReport(self.h, buf, n)
        return json.loads(buf.value.decode())

    def kernel_times(self) -> dict:
        """{kernel: {"ms", "launches", "items"}} of the last render with profiling on (yafaray_amd_getKernelTimes)."""
        n = 32
        names = (C.c_char_p * n)()
        ms = (C.c_double * n)()
        la = (C.c_uint64 * n)()
        it = (C.c_uint64 * n)()
        k = self.L.yafaray_amd_getKernelTimes(self.h, names, ms, la, it, n)
        return {names[j].decode(): {"ms": ms[j], "launches": la[j], "items": it[j]} for j in range(min(k, n)) if la[j]}

    def owned_rows(self):
        """[(y0, y1), ...] pixel rows this rank's last render owns (yafaray_amd_getOwnedRows)."""
        n = self.L.yafaray_amd_getOwnedRows(self.h, None, 0)
        buf = (C.c_int * max(2, 2 * n))()
        self.L.yafaray_amd_getOwnedRows(self.h, buf, n)
        return [(buf[2 * k], buf[2 * k + 1]) for k in range(n)]

    def trace_closest(self, rays):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1)
        n = len(r) // 8
        t = np.empty(n, np.float32)
        p = np.empty(n, np.int32)
        if not self.L.yafaray_amd_traceClosest(self.h, r.ctypes.data_as(C.POINTER(C.c_float)), n,
                                               t.ctypes.data_as(C.POINTER(C.c_float)),
                                               p.ctypes.data_as(C.POINTER(C.c_int))):
            raise RuntimeError("traceClosest failed: " + self.last_error())
        return t, p

    def trace_shadow(self, rays):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1)
        n = len(r) // 8
        o = np.empty(n, np.int32)
        if not self.L.yafaray_amd_traceShadow(self.h, r.ctypes.data_as(C.POINTER(C.c_float)), n,
                                              o.ctypes.data_as(C.POINTER(C.c_int))):
            raise RuntimeError("traceShadow failed: " + self.last_error())
        return o

    TRACE_PARTS = {"both": 0, "closest": 1, "shadow": 2}

    def trace_queued(self, closest_rays, shadow_rays, n_seg=None, part="both", sentinel_t=-7.0, sentinel_prim=-7,
                     sentinel_occ=-7):
        """Test infrastructure (yafaray_amd_traceQueued): the rays through the k_trace launch a render of this
        scene uses, dealt over n_seg ragged queue segments (None: the render's own segment count).  Returns
        (t, prim, occluded, closest_counted, shadow_counted); entries the kernel did not write hold the
        sentinels."""
        fp = C.POINTER(C.c_float)
        cr = np.ascontiguousarray(closest_rays, np.float32).reshape(-1)
        sr = np.ascontiguousarray(shadow_rays, np.float32).reshape(-1)
        nc, ns = len(cr) // 8, len(sr) // 8
        if n_seg is None:
            if self.L.yafaray_amd_traceQueued(self.h, None, 0, None, 0, 1, 0, None, None, None, None):   # (builds the accelerator)
                n_seg = int(self.stats()["shade_grid"])
            else:
                raise RuntimeError("traceQueued failed: " + self.last_error())
        t = np.full(max(nc, 1), sentinel_t, np.float32)
        p = np.full(max(nc, 1), sentinel_prim, np.int32)
        o = np.full(max(ns, 1), sentinel_occ, np.int32)
        counted = (C.c_ulonglong * 2)()
        if not self.L.yafaray_amd_traceQueued(self.h, cr.ctypes.data_as(fp), nc, sr.ctypes.data_as(fp), ns, int(n_seg),
                                              self.TRACE_PARTS[part], t.ctypes.data_as(fp), p.ctypes.data_as(C.POINTER(C.c_int)),
                                              o.ctypes.data_as(C.POINTER(C.c_int)), counted):
            raise RuntimeError("traceQueued failed: " + self.last_error())
        return t[:nc], p[:nc], o[:ns], int(counted[0]), int(counted[1])

    THIN_MODES = {"render": 0, "gpu": 1, "host": 2}

    def thin_rad_points(self, pos, nrm, maxrad, mode="render"):
        """Test infrastructure (yafaray_amd_thinRadPoints): final gathering's radiance-point thinning of (n, 3)
        positions and normals.  mode "render": the render's choice (GPU, host twin where the GPU refuses),
        "gpu" / "host": one of them alone.  Returns (kept indices uint32, rounds; -1 after the host twin)."""
        fp = C.POINTER(C.c_float)
        p = np.ascontiguousarray(pos, np.float32).reshape(-1)
        q = np.ascontiguousarray(nrm, np.float32).reshape(-1)
        n = len(p) // 3
        assert len(q) == len(p) == 3 * n
        kept = np.zeros(max(n, 1), np.uint32)
        nk, rounds = C.c_int(0), C.c_int(0)
        if not self.L.yafaray_amd_thinRadPoints(self.h, p.ctypes.data_as(fp), q.ctypes.data_as(fp), n, float(np.float32(maxrad)),
                                                self.THIN_MODES[mode], kept.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nk),
                                                C.byref(rounds)):
            raise RuntimeError("thinRadPoints failed: " + self.last_error())
        return kept[:nk.value].copy(), rounds.value

    def aa_next_pass(self, accum, weights, tile, threshold, detect_color_noise=False, dark_type=0, dark_factor=0.0, variance_edge=10,
                     variance_pixels=0, ry0=0, ry1=None):
        """Test infrastructure (yafaray_amd_aaNextPass): adaptive AA's nextPass on an accumulated film ((H, W, 4)
        accumulators, (H, W) weights).  Returns (flags (H, W) uint8, plist of the rows [ry0, ry1) in visiting
        order, count of the whole film, local_count)."""
        fp = C.POINTER(C.c_float)
        w = np.ascontiguousarray(weights, np.float32)
        H, W = w.shape
        a = np.ascontiguousarray(accum, np.float32).reshape(H, W, 4)
        flags = np.zeros((H, W), np.uint8)
        plist = np.zeros(max(H * W, 1), np.uint32)
        count, local = C.c_uint32(0), C.c_uint32(0)
        if not self.L.yafaray_amd_aaNextPass(self.h, a.ctypes.data_as(fp), w.ctypes.data_as(fp), W, H, int(tile), int(bool(detect_color_noise)),
                                             int(dark_type), float(dark_factor), int(variance_edge), int(variance_pixels),
                                             float(np.float32(threshold)), int(ry0), int(H if ry1 is None else ry1),
                                             flags.ctypes.data_as(C.POINTER(C.c_uint8)), plist.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             C.byref(count), C.byref(local)):
            raise RuntimeError("aaNextPass failed: " + self.last_error())
        return flags, plist[:local.value].copy(), count.value, local.value

    QUERY_COUNTERS = ("visits", "accepts", "overflows", "depth", "pm_stack", "lds_levels", "spill", "path", "max_seg", "log_cap", "grid",
                      "grid_ties", "photons", "kd_order")

    def query_photons(self, pos, queries, kind, k=1, radius2=1e30, dirs=None, normals=None, n_seg=1, log_cap=0, want_log=False):
        """Test infrastructure (yafaray_amd_queryPhotons): the photon-map queries of a render on the map of (n, 3)
        positions (and directions, nearest kinds) for (m, 3) query points (and normals).  kind 0 - 5 (k-NN gathers)
        return a dict with found (m,) int32, radius2 (m,) float32, idx (m, k) uint32 and dist (m, k) float32 in
        heap-array order, counters (name -> int) and, with want_log, log_n (m,) and log_e (m, cap, 2) uint32;
        kind 6 - 8 (nearest searches) return nearest (m,) int32, grid_raw (kind 7) and counters."""
        fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
        arr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        pos, dirs, qs, ns = arr(pos), arr(dirs), arr(queries), arr(normals)
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        n, m, k = len(pos), len(qs), int(k)
        near = kind in (6, 7, 8)
        counters = np.zeros(16, np.uint64)
        out = {}
        if near:
            out["nearest"] = np.full(max(m, 1), -3, np.int32)
            out["grid_raw"] = np.full(max(m, 1), -3, np.int32) if kind == 7 else None
        else:
            out["found"] = np.zeros(max(m, 1), np.int32)
            out["radius2"] = np.zeros(max(m, 1), np.float32)
            out["idx"] = np.zeros((max(m, 1), max(k, 1)), np.uint32)
            out["dist"] = np.zeros((max(m, 1), max(k, 1)), np.float32)
        cap = 0
        if want_log and not near:
            cap = int(log_cap) if log_cap else (max(k, int(os.environ.get("YAFARAY_AMD_GATHER_LOG", "512"))) + 1) & ~1
            out["log_n"] = np.zeros(max(m, 1), np.uint32)
            out["log_e"] = np.zeros((max(m, 1), max(cap, 1), 2), np.uint32)
        if not self.L.yafaray_amd_queryPhotons(self.h, ptr(pos, fp), ptr(dirs, fp), n, ptr(qs, fp), ptr(ns, fp), m, k, float(np.float32(radius2)),
                                               int(n_seg), int(log_cap), int(kind), ptr(out.get("found"), ip), ptr(out.get("radius2"), fp),
                                               ptr(out.get("idx"), up), ptr(out.get("dist"), fp), ptr(out.get("nearest"), ip),
                                               ptr(out.get("grid_raw"), ip), ptr(out.get("log_n"), up), ptr(out.get("log_e"), up),
                                               counters.ctypes.data_as(C.POINTER(C.c_ulonglong))):
            raise RuntimeError("queryPhotons failed: " + self.last_error())
        res = {key: (v[:m] if v is not None else None) for key, v in out.items()}
        res["counters"] = {name: int(counters[j]) for j, name in enumerate(self.QUERY_COUNTERS)}
        if want_log and not near:
            assert res["counters"]["log_cap"] in (0, cap), "the log cap the wrapper sized for differs from the library's"
        return res



def render_group_id() -> bytes:
    """A fresh render-group id (RCCL unique id) for yafaray_amd_setRenderGroup."""
    buf = C.create_string_buffer(128)
    n = lib().yafaray_amd_getRenderGroupId(buf, 128)
    if n <= 0:
        raise RuntimeError("yafaray_amd_getRenderGroupId failed")
    return buf.raw[:n]


def join_render_group(yi, rank, world, dist):
    """Make `yi` member `rank` of a `world`-GPU render group (one process per GPU): rank 0 creates
    the id, torch.distributed broadcasts it, every member joins on its current HIP device.  The
    library then splits every render into row bands and all-gathers them over RCCL itself."""
    obj = [render_group_id() if rank == 0 else None]
    if world > 1:
        dist.broadcast_object_list(obj, src=0)
    gid = obj[0]
    if not yi.L.yafaray_amd_setRenderGroup(yi.h, int(rank), int(world), gid, len(gid)):
        raise RuntimeError("setRenderGroup failed: " + yi.last_error())


def build_photon_tree(xyz):
    """The GPU point kd-tree of n positions ((n, 3) float32): ((2n - 1, 4) uint32 nodes, depth) in
    the reference's depth-first layout (yafaray_amd_buildPhotonTree)."""
    import numpy as np
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n = int(xyz.shape[0])
    nodes = np.zeros((2 * n - 1, 4), np.uint32)
    depth = C.c_int(0)
    ok = lib().yafaray_amd_buildPhotonTree(xyz.ctypes.data_as(C.POINTER(C.c_float)), n,
                                           nodes.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(depth))
    if not ok:
        raise RuntimeError("yafaray_amd_buildPhotonTree failed")
    return nodes, depth.value


def build_photon_tree_member(xyz, member, members):
    """A group member's share of the distributed point kd-tree build (yafaray_amd_buildPhotonTreeMember):
    (nodes (2n - 1, 4) uint32, kd-order positions (n, 4) float32, depth, split level, device ms)."""
    import numpy as np
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n = int(xyz.shape[0])
    nodes = np.zeros((2 * n - 1, 4), np.uint32)
    kd = np.zeros((n, 4), np.float32)
    depth, level, ms = C.c_int(0), C.c_int(0), C.c_double(0)
    ok = lib().yafaray_amd_buildPhotonTreeMember(xyz.ctypes.data_as(C.POINTER(C.c_float)), n, member, members,
                                                 nodes.ctypes.data_as(C.POINTER(C.c_uint32)), kd.ctypes.data_as(C.POINTER(C.c_float)),
                                                 C.byref(depth), C.byref(level), C.byref(ms))
    if not ok:
        raise RuntimeError("yafaray_amd_buildPhotonTreeMember failed")
    return nodes, kd, depth.value, level.value, ms.value


def photon_tree_segments(n, level, member=0, members=1):
    """The level-`level` subtrees of a tree over n photons ((2^level, 3) uint32: node, start, end) and the
    owned range [s0, s1) of member `member` (yafaray_amd_photonTreeSegments)."""
    import numpy as np
    seg = np.zeros((1 << level, 3), np.uint32)
    s0, s1 = C.c_uint32(0), C.c_uint32(0)
    lib().yafaray_amd_photonTreeSegments(n, level, member, members, seg.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(s0), C.byref(s1))
    return seg, (s0.value, s1.value)


def rebalance_bands(bounds, times, cap_rows=0):
    """The library's band balancer (yafaray_amd_rebalanceBands)."""
    world = len(bounds) - 1
    b = (C.c_int * (world + 1))(*bounds)
    t = (C.c_double * world)(*times)
    out = (C.c_int * (world + 1))()
    lib().yafaray_amd_rebalanceBands(b, world, t, int(cap_rows), out)
    return list(out)


def pack_band(film, bounds, rank):
    """The library's band plan (yafaray_amd_packBand): `rank`'s rows of a (H, W, C) float32 film in a
    zero-padded (max band rows, W, C) buffer, as the render group sends it."""
    film = np.ascontiguousarray(film, np.float32)
    H, W = film.shape[:2]
    ch = 1 if film.ndim == 2 else film.shape[2]
    world = len(bounds) - 1
    rows = max(bounds[r + 1] - bounds[r] for r in range(world))
    out = np.zeros((rows, W) + film.shape[2:], np.float32)
    b = (C.c_int * (world + 1))(*bounds)
    fp = C.POINTER(C.c_float)
    if not lib().yafaray_amd_packBand(film.ctypes.data_as(fp), W, H, ch, b, world, int(rank), out.ctypes.data_as(fp)):
        raise RuntimeError("packBand failed")
    return out


def unpack_bands(gathered, bounds, rank, film):
    """The library's band plan (yafaray_amd_unpackBands): every other member's rows of an all-gather
    result (world * max band rows, W, C) into `film` (H, W, C), in place; `rank`'s own rows stay."""
    gathered = np.ascontiguousarray(gathered, np.float32)
    assert film.dtype == np.float32 and film.flags["C_CONTIGUOUS"]
    H, W = film.shape[:2]
    ch = 1 if film.ndim == 2 else film.shape[2]
    world = len(bounds) - 1
    b = (C.c_int * (world + 1))(*bounds)
    fp = C.POINTER(C.c_float)
    if not lib().yafaray_amd_unpackBands(gathered.ctypes.data_as(fp), W, H, ch, b, world, int(rank), film.ctypes.data_as(fp)):
        raise RuntimeError("unpackBands failed")
    return film


def render_spec(spec, chunk_slots=None, profile=False, shard=None, members=None, devices=None):
    """Replay a scenes.SceneSpec through the C API and render it; returns (rgba, weights, stats).
    members: a device group of this many members (set_device_group)."""
    from . import scenes
    yi = Interface()
    scenes.apply(spec, yi)
    if members is not None:
        yi.set_device_group(members, devices)
    if chunk_slots:
        yi.L.yafaray_amd_setChunkSlots(yi.h, int(chunk_slots))
    if profile:
        yi.L.yafaray_amd_setProfileKernels(yi.h, 1)
    if shard is not None:
        # (rank, world[, mode]): mode "band" (default, contiguous row band) or "tile" (tile rows r % world)
        fn = yi.L.yafaray_amd_setTileRowShard if (len(shard) > 2 and shard[2] == "tile") else yi.L.yafaray_amd_setRowBandShard
        fn(yi.h, int(shard[0]), int(shard[1]))
    yi.render()
    rgba, w = yi.film()
    st = yi.stats()
    st["owned_rows"] = yi.owned_rows()
    if profile:
        st["kernel_times"] = yi.kernel_times()
    yi.close()
    return rgba, w, st
