"""Python host side of the MI355X ray tracer: a thin ctypes binding over the C ABI in include/mirt.h.

The functions mirror the reference's host interface for the hot path (main.cu:25-94), same names and
argument meaning:

    parseInput(path)                        -> StlConfig          parse.hpp:10
    initRawConfigFromStl(stl) +
    copyConfigDataToDevice(stl, raw)        -> RawConfig          config_utils.cuh:11-17
    build_lbvh_karas(raw, morton_bits=30)                         lbvh_builder.cuh:14
    render(d_image, w, h, aa, raw)                                draw.cuh:10
    freeRawConfigDeviceMemory(raw)                                config_utils.cuh:20

Device memory, streams and torch.distributed come from PyTorch (plumbing only); every computation runs in the
hand-written HIP kernels of libmirt.so.  There is no CPU fallback: if the library is missing or no GPU is present
the calls raise.
"""
import contextlib
import ctypes as C
import os

from .binding import (LIB_PATH, EXPORTS, MIRT_ERR_ARG, MIRT_RENDER_COUNTERS, MIRT_HIT_NONE, MIRT_HIT_SPHERE, MIRT_HIT_TRIANGLE,      # noqa: F401
                      MIRT_HIT_PLANE, MIRT_QUERY_ANY_HIT, MIRT_DENOISE_SIGMA_C, MIRT_DENOISE_SIGMA_N, MIRT_DENOISE_SIGMA_P, MirtError, Vec3, Ray,
                      Hit, Camera, Shading, SceneDesc, RenderParams, Stats, MultiStats, TreeNode, RecordInfo, SampleOrderInfo, lib, _check)

# The dtypes a tensor argument may have, by name: torch is imported when a call needs it (uint32 only where torch has it)
_F32, _U8, _INT, _HIT = ("float32",), ("uint8",), ("int32", "uint32"), ("float32", "int32", "uint32")


def _struct_with(cls, s, fields, what):
    """A `cls` copy of `s` with the keyword fields replaced (a Vec3 field takes a Vec3 or three numbers)."""
    out = cls.from_buffer_copy(bytes(s))
    names = dict(cls._fields_)
    for k, v in fields.items():
        if k not in names:
            raise ValueError(f"{k} is not a {what} field; expected one of {sorted(names)}")
        if names[k] is Vec3 and not isinstance(v, Vec3):
            v = Vec3(*(float(c) for c in v))
        setattr(out, k, v)
    return out


def _camera_with(cam, fields):
    """A copy of `cam` with the keyword fields replaced (a Vec3 field takes a Vec3 or three numbers)."""
    return _struct_with(Camera, cam, fields, "camera")


def _shading_with(sh, fields):
    """A copy of `sh` with the keyword fields replaced."""
    return _struct_with(Shading, sh, fields, "shading")


class _Handle:
    """Owner of one library handle, self._h, which the entry point named by _destroy frees: close() frees it once, and __del__
    closes without raising (the interpreter may be half gone)."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------------
# StlConfig: the parsed scene on the host (config.hpp:24-73)
# ------------------------------------------------------------------------------------------------------
class StlConfig(_Handle):
    _destroy = "mirt_host_scene_destroy"

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        self.desc = SceneDesc()
        _check(lib().mirt_host_scene_desc(self._h, C.byref(self.desc)))
        self.filename = lib().mirt_host_scene_filename(self._h).decode()
        for name in ("width", "height", "bounces", "aa", "dof_focus", "dof_lens", "expose", "fisheye", "panorama", "gi",
                     "num_spheres", "num_triangles", "num_prims", "num_planes", "num_suns", "num_bulbs"):
            setattr(self, name, getattr(self.desc, name))

    def array(self, which):
        """Host arrays as numpy structured views (spheres, triangles, prim_refs, planes, suns, bulbs)."""
        import numpy as np
        from . import layouts
        dt, cnt, ptr = {
            "spheres": (layouts.SPHERE, self.desc.num_spheres, self.desc.spheres),
            "triangles": (layouts.TRIANGLE, self.desc.num_triangles, self.desc.triangles),
            "prim_refs": (layouts.PRIMREF, self.desc.num_prims, self.desc.prim_refs),
            "planes": (layouts.PLANE, self.desc.num_planes, self.desc.planes),
            "suns": (layouts.LIGHT, self.desc.num_suns, self.desc.suns),
            "bulbs": (layouts.LIGHT, self.desc.num_bulbs, self.desc.bulbs),
        }[which]
        if cnt == 0:
            return np.zeros(0, dtype=dt)
        buf = (C.c_char * (cnt * dt.itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dt, count=cnt).copy()


def parseInput(path):
    """parseInput(argv, StlConfig&), parse.cpp:16-39.  Raises MirtError with the reference's messages
    ("Error opening file...", "One of the lines are not valid.") where the reference prints them and exits."""
    h = C.c_void_p()
    _check(lib().mirt_parse_scene_file(os.fsencode(path), C.byref(h)))
    return StlConfig(h.value)


def parseText(text):
    data = text.encode()
    h = C.c_void_p()
    _check(lib().mirt_parse_scene_text(data, len(data), C.byref(h)))
    return StlConfig(h.value)


def syntheticScene(num_spheres=1_000_000, num_triangles=1_000_000, seed=1234):
    """The synthetic stress scene of BASELINE config 5."""
    h = C.c_void_p()
    _check(lib().mirt_synthetic_scene(seed, num_spheres, num_triangles, C.byref(h)))
    return StlConfig(h.value)


# ------------------------------------------------------------------------------------------------------
# RawConfig: the device-resident scene (config.hpp:75-126)
# ------------------------------------------------------------------------------------------------------
class RawConfig(_Handle):
    _destroy = "mirt_scene_destroy"

    def __init__(self, stl_or_desc, device=0):
        desc = stl_or_desc.desc if hasattr(stl_or_desc, "desc") else stl_or_desc
        self._keep = stl_or_desc
        self.desc = desc
        self.device = device
        h = C.c_void_p()
        _check(lib().mirt_scene_create(C.byref(desc), device, C.byref(h)))
        self._h = h
        self.build_ms = None

    def stats(self):
        """MirtStats as a dict.  Raises MirtError (status 6) when a capacity overflow was recorded during a render."""
        st = Stats()
        _check(lib().mirt_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def set_option(self, name, value):
        """mirt_scene_set_option: the build option "bounds_as_shipped" takes effect at the next build_lbvh_karas, every other one at the next render."""
        _check(lib().mirt_scene_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int(0)
        _check(lib().mirt_scene_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def stack_info(self):
        """The read-only facts of mirt_scene_get_option about the traversal stack: {"tree_depth": D of the built tree,
        "lds_capacity": stack entries held without spilling, "lds_only": the last render ran the trace kernel without a spill path}."""
        return {"tree_depth": self.get_option("tree_depth"), "lds_capacity": self.get_option("stack_lds_capacity"),
                "lds_only": bool(self.get_option("stack_lds_only"))}

    def camera(self):
        """mirt_scene_get_camera: the scene's camera as a Camera."""
        cam = Camera()
        _check(lib().mirt_scene_get_camera(self._h, C.byref(cam)))
        return cam

    def set_camera(self, cam=None, **fields):
        """mirt_scene_set_camera: `cam` (default: the current camera) with the keyword fields replaced, e.g.
        set_camera(eye=(0, 1, 5), fisheye=1).  The fields are taken as given.  Applies to the calls issued afterwards; a frame
        in flight keeps its camera.  Returns the camera that was set."""
        new = _camera_with(cam if cam is not None else self.camera(), fields)
        _check(lib().mirt_scene_set_camera(self._h, C.byref(new)))
        return new

    def lights(self):
        """mirt_scene_get_lights: (suns, bulbs) as numpy layouts.LIGHT arrays -- v is a sun's direction or a bulb's position --
        as the scene was created or as set_lights left them."""
        import numpy as np
        from . import layouts
        suns = np.zeros(self.desc.num_suns, dtype=layouts.LIGHT)
        bulbs = np.zeros(self.desc.num_bulbs, dtype=layouts.LIGHT)
        _check(lib().mirt_scene_get_lights(self._h, suns.ctypes.data if len(suns) else None, bulbs.ctypes.data if len(bulbs) else None))
        return suns, bulbs

    def set_lights(self, suns=None, bulbs=None, stream=None):
        """mirt_scene_set_lights: new suns and / or bulbs (numpy layouts.LIGHT arrays of the scene's num_suns / num_bulbs
        records; None leaves that kind as it is).  The counts are fixed: a zero colour switches a light off.  The scene stays
        built; a frame in flight keeps its lights.  Asynchronous on `stream` (default: torch's current stream)."""
        ptrs = _light_ptrs(self.desc, suns, bulbs)
        _check(lib().mirt_scene_set_lights(self._h, *ptrs, _stream_ptr(stream)))

    def planes(self):
        """mirt_scene_get_planes: every plane as a numpy layouts.PLANE array."""
        import numpy as np
        from . import layouts
        out = np.zeros(self.desc.num_planes, dtype=layouts.PLANE)
        _check(lib().mirt_scene_get_planes(self._h, 0, len(out), _host_ptr(out)))
        return out

    def set_planes(self, planes, first=0, stream=None):
        """mirt_scene_set_planes: planes first .. first+n-1 take the records of `planes` (numpy layouts.PLANE [n]; make_plane
        makes one the way the parser does), taken as given.  The scene stays built; a frame in flight keeps its planes.
        Asynchronous on `stream` (default: torch's current stream)."""
        from . import layouts
        a = _records(planes, "planes", layouts.PLANE, None)
        _check(lib().mirt_scene_set_planes(self._h, _host_ptr(a), int(first), len(a), _stream_ptr(stream)))

    def shading(self):
        """mirt_scene_get_shading: the scene's bounces, gi and expose as a Shading."""
        sh = Shading()
        _check(lib().mirt_scene_get_shading(self._h, C.byref(sh)))
        return sh

    def set_shading(self, sh=None, **fields):
        """mirt_scene_set_shading: `sh` (default: the current settings) with the keyword fields replaced, e.g.
        set_shading(expose=2.0) or set_shading(bounces=2, gi=1).  Applies to the calls issued afterwards; a frame in flight keeps
        its settings.  Returns the Shading that was set."""
        new = _shading_with(sh if sh is not None else self.shading(), fields)
        _check(lib().mirt_scene_set_shading(self._h, C.byref(new)))
        return new

    def tree(self):
        """(nodes, codes, refs, bounds) in the reference's numbering -- for parity tests."""
        import numpy as np
        from . import layouts
        n = self.desc.num_prims
        nodes = np.zeros(max(2 * n - 1, 0), dtype=layouts.TREENODE)
        codes = np.zeros(n, dtype=np.uint32)
        refs = np.zeros(n, dtype=layouts.PRIMREF)
        bounds = np.zeros(6, dtype=np.float32)
        _check(lib().mirt_get_tree(self._h, nodes.ctypes.data if n else None, codes.ctypes.data if n else None,
                                   refs.ctypes.data if n else None, bounds.ctypes.data))
        return nodes, codes, refs, bounds

    def records(self):
        """mirt_get_records: what the traversal kernels read, as a dict -- "info" (a RecordInfo), "nodes" float32 [N-1, 16],
        "qnodes" uint32 [N-1, 8] or [0, 8], "wnodes" uint32 [N-1, 16] or [0, 16], "prims" float32 [units, 4], "unit_prim",
        "tris_before" uint32, "tri_boxes" float32 [Nt, 8], "qparams" float32 [9] or [0] -- for parity tests."""
        import numpy as np
        n, ns, nt = self.desc.num_prims, self.desc.num_spheres, self.desc.num_triangles
        m, units = max(n - 1, 0), ns + 3 * nt
        info = RecordInfo()
        a = {"nodes": np.zeros((m, 16), np.float32), "qnodes": np.zeros((m, 8), np.uint32), "wnodes": np.zeros((m, 16), np.uint32),
             "prims": np.zeros((units, 4), np.float32), "unit_prim": np.zeros(units, np.uint32), "tris_before": np.zeros(n + 1, np.uint32),
             "tri_boxes": np.zeros((nt, 8), np.float32), "qparams": np.zeros(9, np.float32)}
        _check(lib().mirt_get_records(self._h, C.byref(info), *(_host_ptr(v) for v in a.values())))
        counts = {"nodes": info.num_nodes, "qnodes": info.num_qnodes, "wnodes": info.num_wnodes, "prims": info.prim_units,
                  "unit_prim": info.prim_units, "tris_before": info.num_tris_before, "tri_boxes": info.num_tri_boxes, "qparams": info.num_qparams}
        out = {k: v[:counts[k]] for k, v in a.items()}
        out["info"] = info
        return out

    def sample_order(self):
        """mirt_get_sample_order: the by-sample hand-out table (sched = 2) as a dict -- "total_samples" and "last_launch_samples",
        "order" uint32 [total_samples] (every launch's segment a permutation of its own sample indices), "keys" and "sorted_keys"
        uint32 [last_launch_samples], the cost keys of the last launch measured by sample and in hand-out order -- for parity
        tests.  Waits for a measurement in flight; MirtError (MIRT_ERR_STATE) when the scene has no table."""
        import numpy as np
        info = SampleOrderInfo()
        _check(lib().mirt_get_sample_order(self._h, C.byref(info), None, None, None))
        order = np.zeros(info.total_samples, np.uint32)
        keys, sorted_keys = np.zeros(info.last_launch_samples, np.uint32), np.zeros(info.last_launch_samples, np.uint32)
        _check(lib().mirt_get_sample_order(self._h, C.byref(info), _host_ptr(order), _host_ptr(keys), _host_ptr(sorted_keys)))
        return {"total_samples": info.total_samples, "last_launch_samples": info.last_launch_samples, "order": order, "keys": keys,
                "sorted_keys": sorted_keys}


def _light_ptrs(desc, suns, bulbs):
    """The two host pointers of a set_lights call: each array None, or layouts.LIGHT records, as many as the scene has."""
    from . import layouts
    arrays = [_records(a, name, layouts.LIGHT, n) for a, name, n in ((suns, "suns", desc.num_suns), (bulbs, "bulbs", desc.num_bulbs))]
    return [_host_ptr(a) for a in arrays]


def _records(a, name, dtype, count):
    """ValueError unless `a` is None or a C-contiguous one-dimensional numpy array of `dtype` (of `count` records, if given);
    returns it (None stays None)."""
    import numpy as np
    if a is None:
        return None
    if not isinstance(a, np.ndarray):
        raise ValueError(f"{name} must be a numpy array")
    if a.dtype != dtype:
        raise ValueError(f"{name} has dtype {a.dtype}; expected {dtype}")
    if a.ndim != 1 or (count is not None and a.shape[0] != count):
        raise ValueError(f"{name} has shape {list(a.shape)}; expected [{'n' if count is None else count}]")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name} must be contiguous")
    return a


def _host_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def make_plane(abcd, mat):
    """mirt_make_plane: the record (numpy layouts.PLANE, one element) the parser makes of a `plane a b c d` line under material
    `mat` (a layouts.MAT record): nor and point by the parser's own arithmetic.  Host only."""
    import numpy as np
    from . import layouts
    c = np.ascontiguousarray(abcd, dtype=np.float32)
    if c.shape != (4,):
        raise ValueError(f"abcd has shape {list(c.shape)}; expected [4]")
    mm = np.zeros(1, dtype=layouts.MAT)
    mm[0] = mat
    out = np.zeros(1, dtype=layouts.PLANE)
    _check(lib().mirt_make_plane(c.ctypes.data, mm.ctypes.data, out.ctypes.data))
    return out


def initRawConfigFromStl(stl, device=0):
    """initRawConfigFromStl + copyConfigDataToDevice (config_utils.cu:18-199): uploads the scene."""
    return RawConfig(stl, device)


copyConfigDataToDevice = initRawConfigFromStl


def freeRawConfigDeviceMemory(raw):
    raw.close()


def part_pixel_xy(params, local):
    """mirt_part_pixel_xy: frame coordinates of local pixel `local` of a part's compact buffer (host arithmetic, no GPU)."""
    x, y = C.c_int32(0), C.c_int32(0)
    _check(lib().mirt_part_pixel_xy(C.byref(params), local, C.byref(x), C.byref(y)))
    return x.value, y.value


class MultiGpu(_Handle):
    """mirt_multi_*: one process, several GPUs, RCCL framebuffer gather (include/mirt.h)."""
    _destroy = "mirt_multi_destroy"

    def __init__(self, stl, ngpu=1, devices=None):
        self._keep = stl
        dv = (C.c_int * ngpu)(*devices) if devices is not None else None
        h = C.c_void_p()
        _check(lib().mirt_multi_create(C.byref(stl.desc), ngpu, dv, C.byref(h)))
        self._h = h

    def set_option(self, name, value):
        """mirt_multi_set_option: the option on every device's scene."""
        _check(lib().mirt_multi_set_option(self._h, name.encode(), int(value)))

    def set_camera(self, cam, **fields):
        """mirt_multi_set_camera: `cam` (with the keyword fields replaced) on every device's scene, for the frames submitted
        afterwards."""
        new = _camera_with(cam, fields)
        _check(lib().mirt_multi_set_camera(self._h, C.byref(new)))
        return new

    def set_lights(self, suns=None, bulbs=None):
        """mirt_multi_set_lights: RawConfig.set_lights on every device's scene, for the frames submitted afterwards."""
        ptrs = _light_ptrs(self._keep.desc, suns, bulbs)
        _check(lib().mirt_multi_set_lights(self._h, *ptrs))

    def set_planes(self, planes, first=0):
        """mirt_multi_set_planes: RawConfig.set_planes on every device's scene, for the frames submitted afterwards."""
        from . import layouts
        a = _records(planes, "planes", layouts.PLANE, None)
        _check(lib().mirt_multi_set_planes(self._h, _host_ptr(a), int(first), len(a)))

    def set_shading(self, sh, **fields):
        """mirt_multi_set_shading: `sh` (with the keyword fields replaced) on every device's scene, for the frames submitted
        afterwards."""
        new = _shading_with(sh, fields)
        _check(lib().mirt_multi_set_shading(self._h, C.byref(new)))
        return new

    def render_frame(self, width, height, spp, stripe_rows=4):
        import numpy as np
        out = np.zeros((height, width, 4), np.uint8)
        st = MultiStats()
        _check(lib().mirt_render_frame_multi(self._h, width, height, spp, stripe_rows, out.ctypes.data, C.byref(st)))
        return out, self._stats(st)

    @staticmethod
    def _stats(st):
        n = st.num_gpus
        return dict(num_gpus=n, build_ms=st.build_ms, render_ms=list(st.render_ms)[:n], gather_ms=st.gather_ms, frame_ms=st.frame_ms)

    def submit(self, width, height, spp, stripe_rows=4, out=None):
        """mirt_multi_submit: issues a frame, returns its ticket.  `out` (numpy uint8 [height, width, 4], kept alive by the caller
        until wait) receives the frame."""
        t = C.c_uint64(0)
        _check(lib().mirt_multi_submit(self._h, width, height, spp, stripe_rows, out.ctypes.data if out is not None else None, C.byref(t)))
        return t.value

    def wait(self, ticket):
        st = MultiStats()
        _check(lib().mirt_multi_wait(self._h, ticket, C.byref(st)))
        return self._stats(st)

    def render_frames(self, width, height, spp, nframes, in_flight=2, stripe_rows=4):
        """mirt_render_frames_multi: nframes frames back to back, `in_flight` of them in flight; (last frame, its stats, ms per frame)."""
        import numpy as np
        out = np.zeros((height, width, 4), np.uint8)
        st = MultiStats()
        ms = C.c_float(0)
        _check(lib().mirt_render_frames_multi(self._h, width, height, spp, stripe_rows, nframes, in_flight, out.ctypes.data, C.byref(st), C.byref(ms)))
        return out, self._stats(st), ms.value

    def stats(self, part):
        st = Stats()
        _check(lib().mirt_multi_get_stats(self._h, part, C.byref(st)))
        return st.as_dict()


def _stream_ptr(stream):
    if stream is None:
        try:
            import torch
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        except Exception:
            return None
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream)
    return C.c_void_p(int(stream))


def _ptr(x):
    """A tensor's device address (or an int that is one) as a void* argument; None and an empty tensor give NULL."""
    if x is None:
        return None
    if not hasattr(x, "data_ptr"):
        return C.c_void_p(int(x)) if int(x) else None
    return C.c_void_p(x.data_ptr()) if x.numel() else None


def _tensors(*specs):
    """ValueError unless every (x, name, dtypes, want) in turn is a contiguous torch tensor of one of the dtypes (names: _F32, _INT, ...)
    and, `want` a list, of that shape (None stands for any size, as in [None, 8]) or, `want` a number, of that many elements in any
    shape.  Returns the (x, name) pairs, which is what _on_device takes."""
    import torch
    for x, name, dtypes, want in specs:
        dtypes = [getattr(torch, d) for d in dtypes if hasattr(torch, d)]
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if x.dtype not in dtypes:
            raise ValueError(f"{name} has dtype {x.dtype}; expected one of {[str(d) for d in dtypes]}")
        if isinstance(want, list):
            if x.dim() != len(want) or any(k is not None and have != k for have, k in zip(x.shape, want)):
                raise ValueError(f"{name} has shape {list(x.shape)}; expected [{', '.join('n' if k is None else str(k) for k in want)}]")
        elif x.numel() != want:
            raise ValueError(f"{name} has shape {list(x.shape)}; expected {want} elements")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return [(x, name) for x, name, _, _ in specs]


def _on_device(tensors, device=None, first=None):
    """ValueError unless every (tensor, name), the one named `first` ahead of the others, is on cuda device `device` (None: on the
    device of the first).  Returns its index."""
    import torch
    for x, name in sorted(tensors, key=lambda t: t[1] != first):
        index = None
        if x.device.type == "cuda":
            index = x.device.index if x.device.index is not None else torch.cuda.current_device()
        if index is None or (device is not None and index != device):
            raise ValueError(f"{name} is on {x.device}; expected " + ("a cuda device" if device is None else f"cuda:{device}"))
        device = index
    return device


@contextlib.contextmanager
def _device_and_stream(device, stream):
    """cuda device `device` current and `stream` (None: the stream current on that device) torch's current stream: what a driver
    allocates and issues its calls under.  Gives (torch device, stream)."""
    import torch
    dev = torch.device("cuda", device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        yield dev, s


def _frame(params, width, height, spp):
    """`params`, or without them the whole width x height frame at `spp`."""
    return params if params is not None else render_params(width, height, spp)


# build_lbvh_karas, render, render_accumulate, finalize and scatter_part check nothing in Python (the library checks what it is
# given): a frame loop calls them once per frame, and they stay this thin.
def build_lbvh_karas(raw, morton_bits=30, stream=None):
    """build_lbvh_karas(RawConfig&, int morton_bits = 30), lbvh_builder.cu:401-521.  morton_bits is accepted and
    ignored exactly as in the reference (10 bits per axis are hard-coded there, lbvh_utils.cu:84)."""
    ms = C.c_float(0)
    _check(lib().mirt_build_lbvh(raw._h, _stream_ptr(stream), C.byref(ms)))
    raw.build_ms = ms.value
    return ms.value


def render_params(width, height, aa, stripe_rows=None, num_parts=1, part=0, counters=False):
    p = RenderParams()
    p.width, p.height, p.spp = width, height, aa
    p.stripe_rows = stripe_rows if stripe_rows else height
    p.num_parts, p.part = num_parts, part
    p.flags = MIRT_RENDER_COUNTERS if counters else 0
    return p


def num_pixels(params):
    n = lib().mirt_render_num_pixels(C.byref(params))
    if n < 0:
        raise MirtError(MIRT_ERR_ARG, "bad render parameters")
    return n


def render(d_image, img_width, img_height, aa, raw, d_float=None, params=None, stream=None):
    """render(pixel_t* d_image, w, h, aa, RawConfig*), draw.cu:215-239.

    d_image: a CUDA/HIP uint8 tensor (or raw device pointer) of num_pixels*4 bytes, RGBA.
    d_float: optional float32 tensor of num_pixels*4 -- the linear sample mean before sRGB/quantisation.
    params : optional RenderParams selecting one part of a striped frame (multi-GPU); default = whole frame.
    Asynchronous on `stream` (default: torch's current stream)."""
    p = _frame(params, img_width, img_height, aa)
    _check(lib().mirt_render(raw._h, C.byref(p), _ptr(d_image), _ptr(d_float), _stream_ptr(stream)))


def render_accumulate(d_accum, img_width, img_height, sample_first, sample_count, raw, params=None, stream=None):
    """render_kernel_atomic_aa, draw.cu:49-92: adds samples [sample_first, sample_first + sample_count) of every pixel to the
    float32 accumulation buffer d_accum (num_pixels * 4, zeroed by the caller before the first call)."""
    p = _frame(params, img_width, img_height, max(sample_first + sample_count, 2))
    _check(lib().mirt_render_accumulate(raw._h, C.byref(p), _ptr(d_accum), int(sample_first), int(sample_count), _stream_ptr(stream)))


def finalize(d_image, d_accum, img_width, img_height, total_samples, params=None, stream=None):
    """finalize_kernel, draw.cu:13-47: mean over total_samples, sRGB, 8-bit with rounding."""
    p = _frame(params, img_width, img_height, max(total_samples, 2))
    _check(lib().mirt_finalize(C.byref(p), _ptr(d_accum), int(total_samples), _ptr(d_image), _stream_ptr(stream)))


def scatter_part(params, d_part, d_frame, stream=None):
    _check(lib().mirt_scatter_part(C.byref(params), _ptr(d_part), _ptr(d_frame), _stream_ptr(stream)))


# ------------------------------------------------------------------------------------------------------
# Ray queries (mirt_trace_rays / mirt_camera_rays): rays are float32 [n, 8] tensors (MirtRay), hits 4-byte [n, 6] tensors (MirtHit)
# ------------------------------------------------------------------------------------------------------
def _ray_tensors(d_rays, d_hits, *features):
    """_tensors for a ray tensor, the hit tensor of as many rows and every (tensor, name) of `features`, float32 [n, 8] rows for
    the same rays.  Returns the number of rays and the (tensor, name) pairs."""
    tensors = _tensors((d_rays, "d_rays", _F32, [None, 8]))
    n = d_rays.shape[0]
    return n, tensors + _tensors((d_hits, "d_hits", _HIT, [n, 6]), *((x, name, _F32, [n, 8]) for x, name in features))


def _record_tensors(rows, d_hits, d_counts, d_features=None, max_k=8, check_k=None):
    """_tensors for a record query (trace_rays_multi, closest_points_multi, overlap_boxes), in this order: `rows` = (tensor, name,
    width), float32 [n, width]; d_hits, a 4-byte dtype [n, k, 6] with k at most max_k (None: k = 0); d_counts, int32 [n], which a
    call with k = 0 needs; check_k(k), the caller's own check; d_features, float32 [n, k, 8].  Returns the (tensor, name) pairs,
    n and k."""
    x, name, width = rows
    tensors = _tensors((x, name, _F32, [None, width]))
    n, k = x.shape[0], 0
    if d_hits is not None:
        tensors += _tensors((d_hits, "d_hits", _HIT, [n, None, 6]))
        k = d_hits.shape[1]
        if k > max_k:
            raise ValueError(f"d_hits has shape {list(d_hits.shape)}; expected [n, k, 6] with k at most {max_k}")
    if d_counts is not None:
        tensors += _tensors((d_counts, "d_counts", _INT, [n]))
    elif k == 0:
        raise ValueError("a call without hit records (d_hits None or k = 0) needs d_counts")
    if check_k is not None:
        check_k(k)
    if d_features is not None:
        tensors += _tensors((d_features, "d_features", _F32, [n, k, 8]))
    return tensors, n, k


def _count_tensor(rows, d_counts=None):
    """For the count wrappers: checks `rows` = (tensor, name, width) as _record_tensors does and returns d_counts or, without one, a
    new int32 [n] tensor on the rows' device."""
    import torch
    x, name, width = rows
    _tensors((x, name, _F32, [None, width]))
    return d_counts if d_counts is not None else torch.empty(x.shape[0], dtype=torch.int32, device=x.device)


def trace_rays(raw, d_rays, d_hits, any_hit=False, stream=None):
    """mirt_trace_rays: closest hit (hitNearest, draw.cu:292-318) or, with any_hit, occlusion of every ray of d_rays (float32
    [n, 8], MirtRay rows: pack_rays) into d_hits (a 4-byte dtype, [n, 6], MirtHit rows: unpack_hits).  Both contiguous and on
    the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    n, tensors = _ray_tensors(d_rays, d_hits)
    _on_device(tensors, raw.device)
    _check(lib().mirt_trace_rays(raw._h, _ptr(d_rays), n, _ptr(d_hits), MIRT_QUERY_ANY_HIT if any_hit else 0, _stream_ptr(stream)))


def camera_rays(raw, d_rays, img_width, img_height, aa, params=None, stream=None):
    """mirt_camera_rays: the primary ray of sample 0 of every pixel of the frame (or of the part `params` selects), in the order
    render writes pixels, into d_rays (float32 [num_pixels, 8], contiguous, on the scene's device).  trace_rays of these rays
    gives the render's primary hits."""
    p = _frame(params, img_width, img_height, aa)
    _on_device(_tensors((d_rays, "d_rays", _F32, [num_pixels(p), 8])), raw.device)
    _check(lib().mirt_camera_rays(raw._h, C.byref(p), _ptr(d_rays), _stream_ptr(stream)))


# ------------------------------------------------------------------------------------------------------
# Updates in place (mirt_scene_update_spheres / mirt_scene_update_triangles): new geometry from device tensors
# ------------------------------------------------------------------------------------------------------
def _range_call(symbol, raw, d, name, cols, first, stream):
    """The update and get calls of a range of spheres or triangles: `d` (float32 [n, cols], contiguous, on the scene's device)
    holds, or receives, the values of primitives first .. first+n-1.  An update takes (pointer, first, n), a get (first, n,
    pointer)."""
    _on_device(_tensors((d, name, _F32, [None, cols])), raw.device)
    f = getattr(lib(), symbol)
    where = (int(first), d.shape[0], _ptr(d)) if "_get_" in symbol else (_ptr(d), int(first), d.shape[0])
    _check(f(raw._h, *where, _stream_ptr(stream)))


def update_spheres(raw, d_xyzr, first=0, stream=None):
    """mirt_scene_update_spheres: spheres first .. first+n-1 (file order) take cx, cy, cz, r from d_xyzr (float32 [n, 4],
    contiguous, on the scene's device).  Asynchronous on `stream` (default: torch's current stream); the scene is not built
    until the next build_lbvh_karas (n = 0 changes nothing)."""
    _range_call("mirt_scene_update_spheres", raw, d_xyzr, "d_xyzr", 4, first, stream)


def update_triangles(raw, d_verts, first=0, stream=None):
    """mirt_scene_update_triangles: triangles first .. first+n-1 (file order) take p0, p1, p2 from d_verts (float32 [n, 9],
    contiguous, on the scene's device); nor, e1 and e2 are computed on the device as the parser computes them
    (object.cuh:177-191).  Asynchronous on `stream`; the scene is not built until the next build_lbvh_karas."""
    _range_call("mirt_scene_update_triangles", raw, d_verts, "d_verts", 9, first, stream)


def update_sphere_materials(raw, d_mats, first=0, stream=None):
    """mirt_scene_update_sphere_materials: spheres first .. first+n-1 (file order) take their material from d_mats (float32
    [n, 11]: colour rgb, shininess rgb, trans rgb, ior, roughness -- layouts.MAT's order; contiguous, on the scene's device).
    Asynchronous on `stream` (default: torch's current stream); the scene stays built (n = 0 changes nothing).  The next render
    waits once, on the host, for the update's kernels."""
    _range_call("mirt_scene_update_sphere_materials", raw, d_mats, "d_mats", 11, first, stream)


def update_triangle_materials(raw, d_mats, first=0, stream=None):
    """mirt_scene_update_triangle_materials: update_sphere_materials for triangles first .. first+n-1 (file order)."""
    _range_call("mirt_scene_update_triangle_materials", raw, d_mats, "d_mats", 11, first, stream)


def get_sphere_materials(raw, d_mats, first=0, stream=None):
    """mirt_scene_get_sphere_materials: the materials of spheres first .. first+n-1 into d_mats (float32 [n, 11], contiguous, on
    the scene's device): what update_sphere_materials was given, or the file's values.  Asynchronous on `stream`."""
    _range_call("mirt_scene_get_sphere_materials", raw, d_mats, "d_mats", 11, first, stream)


def get_triangle_materials(raw, d_mats, first=0, stream=None):
    """mirt_scene_get_triangle_materials: get_sphere_materials for triangles first .. first+n-1."""
    _range_call("mirt_scene_get_triangle_materials", raw, d_mats, "d_mats", 11, first, stream)


# ------------------------------------------------------------------------------------------------------
# Adaptive sampling (mirt_render_accumulate_pixels / mirt_select_pixels / mirt_finalize_counts): accum and accum_sq are float32
# tensors of num_pixels * 4 elements, counts 4-byte integer tensors of num_pixels, pixel lists int32 / uint32 [n]
# ------------------------------------------------------------------------------------------------------
def render_accumulate_pixels(raw, d_accum, img_width, img_height, sample_first, sample_count, pixels=None, d_accum_sq=None, d_counts=None,
                             params=None, stream=None):
    """mirt_render_accumulate_pixels: render_accumulate for the pixels of `pixels` (int32 / uint32 [n], distinct local pixel
    indices, any order; None: every pixel), adding as well the squared samples to d_accum_sq and sample_count to d_counts (both
    optional).  Unlisted pixels are neither traced nor written.  Asynchronous on `stream` (default: torch's current stream)."""
    p = _frame(params, img_width, img_height, max(sample_first + sample_count, 2))
    n = num_pixels(p)
    _on_device(_tensors((d_accum, "d_accum", _F32, 4 * n)), raw.device)
    for spec in ((d_accum_sq, "d_accum_sq", _F32, 4 * n), (d_counts, "d_counts", _INT, n), (pixels, "pixels", _INT, [None])):
        if spec[0] is not None:      # (one at a time, its device included, before the next)
            _on_device(_tensors(spec), raw.device)
    listed = pixels.shape[0] if pixels is not None else 0
    if pixels is not None and listed == 0:      # (an empty tensor has no address to pass: an empty list renders nothing)
        return
    _check(lib().mirt_render_accumulate_pixels(raw._h, C.byref(p), _ptr(pixels), listed, _ptr(d_accum), _ptr(d_accum_sq), _ptr(d_counts),
                                               int(sample_first), int(sample_count), _stream_ptr(stream)))


def select_pixels(d_accum, d_accum_sq, d_counts, img_width, img_height, min_samples, max_samples, max_variance, d_pixels_out, d_num_out,
                  params=None, stream=None):
    """mirt_select_pixels: the pixels with fewer than max_samples samples that have fewer than min_samples or whose estimated
    variance of the mean exceeds max_variance, in increasing order, into d_pixels_out (int32 / uint32 [num_pixels]); their number
    into d_num_out (one 4-byte integer).  All tensors on the device of d_accum.  Asynchronous on `stream`."""
    import torch
    p = _frame(params, img_width, img_height, 2)
    n = num_pixels(p)
    device = _on_device(_tensors((d_accum, "d_accum", _F32, 4 * n), (d_accum_sq, "d_accum_sq", _F32, 4 * n), (d_counts, "d_counts", _INT, n),
                                 (d_pixels_out, "d_pixels_out", _INT, n), (d_num_out, "d_num_out", _INT, 1)))
    with torch.cuda.device(device):
        _check(lib().mirt_select_pixels(C.byref(p), _ptr(d_accum), _ptr(d_accum_sq), _ptr(d_counts), int(min_samples), int(max_samples),
                                        float(max_variance), _ptr(d_pixels_out), _ptr(d_num_out), _stream_ptr(stream)))


def finalize_counts(d_image, d_accum, d_counts, img_width, img_height, params=None, stream=None):
    """mirt_finalize_counts: finalize with d_counts[pixel] as each pixel's number of samples (0: a zero pixel)."""
    import torch
    p = _frame(params, img_width, img_height, 2)
    n = num_pixels(p)
    device = _on_device(_tensors((d_image, "d_image", _U8, 4 * n), (d_accum, "d_accum", _F32, 4 * n), (d_counts, "d_counts", _INT, n)), first="d_accum")
    with torch.cuda.device(device):
        _check(lib().mirt_finalize_counts(C.byref(p), _ptr(d_accum), _ptr(d_counts), _ptr(d_image), _stream_ptr(stream)))


def render_adaptive(raw, width, height, min_spp, max_spp, step, max_variance, params=None, stream=None):
    """Adaptive sampling of one frame (or of the part `params` selects): samples [0, min_spp) for every pixel, then rounds of
    select_pixels -> render_accumulate_pixels adding samples [min_spp + r step, min_spp + (r + 1) step) to the pixels still
    noisier than max_variance, while the round stays within max_spp; finalize_counts at the end.  Every round uses one sample
    range for all its pixels, so no pixel sees a sample index twice.  Reads 4 bytes back per round (the number selected).
    Returns (rgba8 uint8 [num_pixels * 4], counts int32 [num_pixels], rounds)."""
    import torch
    if min_spp < 2 or max_spp < min_spp or step < 1:
        raise ValueError("render_adaptive needs 2 <= min_spp <= max_spp and step >= 1")
    p = _frame(params, width, height, max(max_spp, 2))
    n = num_pixels(p)
    with _device_and_stream(raw.device, stream) as (dev, s):
        accum = torch.zeros(4 * n, dtype=torch.float32, device=dev)
        accum_sq = torch.zeros(4 * n, dtype=torch.float32, device=dev)
        counts = torch.zeros(n, dtype=torch.int32, device=dev)
        pixels = torch.empty(n, dtype=torch.int32, device=dev)
        num = torch.zeros(1, dtype=torch.int32, device=dev)
        image = torch.empty(4 * n, dtype=torch.uint8, device=dev)
        render_accumulate_pixels(raw, accum, width, height, 0, min_spp, None, accum_sq, counts, params=p, stream=s)
        rounds = 0
        while min_spp + (rounds + 1) * step <= max_spp:
            select_pixels(accum, accum_sq, counts, width, height, min_spp, max_spp, max_variance, pixels, num, params=p, stream=s)
            k = int(num.item())
            if k == 0:
                break
            render_accumulate_pixels(raw, accum, width, height, min_spp + rounds * step, step, pixels[:k], accum_sq, counts, params=p, stream=s)
            rounds += 1
        finalize_counts(image, accum, counts, width, height, params=p, stream=s)
    return image, counts, rounds


# ------------------------------------------------------------------------------------------------------
# Denoising (mirt_hit_features / mirt_denoise): features are float32 [n, 8] tensors, (Px, Py, Pz, hit, nx, ny, nz, 0) per ray
# ------------------------------------------------------------------------------------------------------
# Defaults of the filter's three scales
DENOISE_SIGMA_C, DENOISE_SIGMA_N, DENOISE_SIGMA_P = MIRT_DENOISE_SIGMA_C, MIRT_DENOISE_SIGMA_N, MIRT_DENOISE_SIGMA_P


def hit_features(raw, d_rays, d_hits, d_features, stream=None):
    """mirt_hit_features: rays (float32 [n, 8]) and their closest-hit records (a 4-byte dtype, [n, 6]) -> d_features (float32
    [n, 8]): hit point and hit flag, normal and 0; a miss gives a zero row.  All contiguous and on the scene's device.
    Asynchronous on `stream` (default: torch's current stream)."""
    n, tensors = _ray_tensors(d_rays, d_hits, (d_features, "d_features"))
    _on_device(tensors, raw.device)
    _check(lib().mirt_hit_features(raw._h, _ptr(d_rays), _ptr(d_hits), n, _ptr(d_features), _stream_ptr(stream)))


def _sigmas(**sigmas):
    for name, s in sigmas.items():
        if not (0.0 < float(s) < float("inf")):
            raise ValueError(f"{name} is {s}; expected a finite positive number")


def denoise_work_bytes(img_width, img_height, params=None):
    """mirt_denoise_work_bytes: the bytes of workspace a denoise call of this frame needs (40 per pixel; host arithmetic)."""
    p = _frame(params, img_width, img_height, 2)
    return int(lib().mirt_denoise_work_bytes(C.byref(p)))


def denoise(d_out, d_accum, d_accum_sq, d_counts, d_features, img_width, img_height, d_work, iterations=5, sigma_c=DENOISE_SIGMA_C,
            sigma_n=DENOISE_SIGMA_N, sigma_p=DENOISE_SIGMA_P, params=None, stream=None):
    """mirt_denoise: the variance-guided a-trous filter over a whole frame.  d_accum, d_accum_sq (float32, 4 per pixel) and
    d_counts (a 4-byte integer per pixel) as render_accumulate_pixels leaves them, d_features (float32 [num_pixels, 8]) from
    hit_features of the frame's camera rays; d_out (float32, 4 per pixel) receives the filtered mean -- finalize(..., 1) makes the
    8-bit image of it; d_work is a float32 tensor of denoise_work_bytes / 4 elements that no other call in flight uses.  All
    tensors contiguous, on one device, and distinct.  Asynchronous on `stream`."""
    import torch
    p = _frame(params, img_width, img_height, 2)
    if p.num_parts != 1:
        raise ValueError("denoise works on whole frames: params.num_parts must be 1")
    n = num_pixels(p)
    tensors = _tensors((d_out, "d_out", _F32, 4 * n), (d_accum, "d_accum", _F32, 4 * n), (d_accum_sq, "d_accum_sq", _F32, 4 * n), (d_counts, "d_counts", _INT, n),
                       (d_features, "d_features", _F32, [n, 8]), (d_work, "d_work", _F32, 10 * n))
    if not 0 <= int(iterations) <= 8:
        raise ValueError(f"iterations is {iterations}; expected 0..8")
    _sigmas(sigma_c=sigma_c, sigma_n=sigma_n, sigma_p=sigma_p)
    device = _on_device(tensors, first="d_accum")
    with torch.cuda.device(device):
        _check(lib().mirt_denoise(C.byref(p), _ptr(d_accum), _ptr(d_accum_sq), _ptr(d_counts), _ptr(d_features), int(iterations), float(sigma_c),
                                  float(sigma_n), float(sigma_p), _ptr(d_work), _ptr(d_out), _stream_ptr(stream)))


def _primary_features(raw, params, rays, hits, features, stream):
    """camera_rays of the frame `params` describes -> trace_rays -> hit_features, into the caller's buffers.  params.spp decides
    which rays these are (mirt_camera_rays: un-jittered for 0, each pixel's own jitter above 1)."""
    camera_rays(raw, rays, params.width, params.height, params.spp, params=params, stream=stream)
    trace_rays(raw, rays, hits, stream=stream)
    hit_features(raw, rays, hits, features, stream=stream)


def denoise_frame(raw, accum, accum_sq, counts, width, height, spp, iterations=5, sigma_c=DENOISE_SIGMA_C, sigma_n=DENOISE_SIGMA_N,
                  sigma_p=DENOISE_SIGMA_P, stream=None):
    """Denoise the frame whose moments render_accumulate_pixels (or render_adaptive's loop) left in accum, accum_sq and counts:
    camera_rays (sample 0 of every pixel of a width x height frame at `spp`) -> trace_rays -> hit_features -> denoise ->
    finalize with total_samples = 1.  Returns (rgba8 uint8 [num_pixels * 4], float32 [num_pixels * 4]: the filtered mean)."""
    import torch
    p = render_params(width, height, max(spp, 2))      # (the seeding of render_accumulate's samples, whatever their number)
    n = num_pixels(p)
    with _device_and_stream(raw.device, stream) as (dev, s):
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        hits = torch.empty((n, 6), dtype=torch.int32, device=dev)
        features = torch.empty((n, 8), dtype=torch.float32, device=dev)
        work = torch.empty(10 * n, dtype=torch.float32, device=dev)
        out = torch.empty(4 * n, dtype=torch.float32, device=dev)
        image = torch.empty(4 * n, dtype=torch.uint8, device=dev)
        _primary_features(raw, p, rays, hits, features, s)
        denoise(out, accum, accum_sq, counts, features, width, height, work, iterations, sigma_c, sigma_n, sigma_p, params=p, stream=s)
        finalize(image, out, width, height, 1, params=p, stream=s)
    return image, out

# ------------------------------------------------------------------------------------------------------
# Temporal accumulation (mirt_scene_get_spheres / mirt_scene_get_triangles / mirt_prev_features / mirt_temporal_accumulate)
# ------------------------------------------------------------------------------------------------------
def get_spheres(raw, d_xyzr, first=0, stream=None):
    """mirt_scene_get_spheres: cx, cy, cz, r of spheres first .. first+n-1 (file order) into d_xyzr (float32 [n, 4], contiguous,
    on the scene's device): what update_spheres was given, or the file's values.  Asynchronous on `stream`; the scene stays as
    built as it was."""
    _range_call("mirt_scene_get_spheres", raw, d_xyzr, "d_xyzr", 4, first, stream)


def get_triangles(raw, d_verts, first=0, stream=None):
    """mirt_scene_get_triangles: p0, p1, p2 of triangles first .. first+n-1 (file order) into d_verts (float32 [n, 9], contiguous,
    on the scene's device).  Asynchronous on `stream`; the scene stays as built as it was."""
    _range_call("mirt_scene_get_triangles", raw, d_verts, "d_verts", 9, first, stream)


def prev_features(raw, d_rays, d_hits, d_features, d_prev_xyzr=None, d_prev_verts=None, stream=None):
    """mirt_prev_features: hit_features' rows with the hit point and normal as they were in the previous geometry: d_prev_xyzr
    (float32 [num_spheres, 4]) and d_prev_verts (float32 [num_triangles, 9]) are get_spheres / get_triangles of the whole scene
    before it moved; None: that kind did not move.  All contiguous and on the scene's device.  Asynchronous on `stream`."""
    n, tensors = _ray_tensors(d_rays, d_hits, (d_features, "d_features"))
    previous = ((d_prev_xyzr, "d_prev_xyzr", _F32, [raw.desc.num_spheres, 4]), (d_prev_verts, "d_prev_verts", _F32, [raw.desc.num_triangles, 9]))
    _on_device(tensors + _tensors(*(spec for spec in previous if spec[0] is not None)), raw.device)
    _check(lib().mirt_prev_features(raw._h, _ptr(d_rays), _ptr(d_hits), n, _ptr(d_prev_xyzr), _ptr(d_prev_verts), _ptr(d_features), _stream_ptr(stream)))


def _is_pinhole(cam):
    return cam.fisheye == 0 and cam.panorama == 0 and cam.dof_focus == 0.0


def temporal_accumulate(d_out_accum, d_out_accum_sq, d_out_counts, d_accum, d_accum_sq, d_counts, d_prev_features, d_hist_accum, d_hist_accum_sq,
                        d_hist_counts, d_hist_features, prev_camera, img_width, img_height, max_history=32, sigma_n=DENOISE_SIGMA_N,
                        sigma_p=DENOISE_SIGMA_P, params=None, stream=None):
    """mirt_temporal_accumulate: this frame's moments (d_accum, d_accum_sq: float32, 4 per pixel; d_counts: a 4-byte integer per
    pixel) plus what survives of the previous merged frame (d_hist_*, with d_hist_features = hit_features of that frame and
    prev_camera its Camera, a pinhole), looked up where d_prev_features (prev_features of this frame's rays) says each pixel's
    surface point was, into d_out_*.  An output may be its own current-frame tensor (in place); no other overlap.  All tensors
    contiguous and on one device.  Asynchronous on `stream`."""
    import torch
    p = _frame(params, img_width, img_height, 2)
    if p.num_parts != 1:
        raise ValueError("temporal_accumulate works on whole frames: params.num_parts must be 1")
    n = num_pixels(p)
    moments = ((d_out_accum, "d_out_accum"), (d_out_accum_sq, "d_out_accum_sq"), (d_accum, "d_accum"), (d_accum_sq, "d_accum_sq"),
               (d_hist_accum, "d_hist_accum"), (d_hist_accum_sq, "d_hist_accum_sq"))
    counts = ((d_out_counts, "d_out_counts"), (d_counts, "d_counts"), (d_hist_counts, "d_hist_counts"))
    feats = ((d_prev_features, "d_prev_features"), (d_hist_features, "d_hist_features"))
    tensors = _tensors(*[(x, name, _F32, 4 * n) for x, name in moments], *[(x, name, _INT, n) for x, name in counts],
                       *[(x, name, _F32, [n, 8]) for x, name in feats])
    if not isinstance(prev_camera, Camera):
        raise ValueError("prev_camera must be a Camera")
    if not _is_pinhole(prev_camera):
        raise ValueError("prev_camera must be a pinhole: fisheye, panorama and dof_focus 0")
    if int(max_history) < 1:
        raise ValueError(f"max_history is {max_history}; expected at least 1")
    _sigmas(sigma_n=sigma_n, sigma_p=sigma_p)
    device = _on_device(tensors, first="d_accum")
    with torch.cuda.device(device):
        _check(lib().mirt_temporal_accumulate(C.byref(p), C.byref(prev_camera), _ptr(d_accum), _ptr(d_accum_sq), _ptr(d_counts), _ptr(d_prev_features),
                                              _ptr(d_hist_accum), _ptr(d_hist_accum_sq), _ptr(d_hist_counts), _ptr(d_hist_features), int(max_history),
                                              float(sigma_n), float(sigma_p), _ptr(d_out_accum), _ptr(d_out_accum_sq), _ptr(d_out_counts),
                                              _stream_ptr(stream)))


class TemporalAccumulator:
    """Frames of an animated scene that reuse the previous frame's samples.  (A history gathered under other lights, planes,
    materials or shading settings is stale -- reprojection follows surface points, not what they looked like: after set_lights,
    set_planes, set_shading or a material update call reset(), or keep max_history low.)  Allocates once: this frame's moments and two history
    sets used in turn, two feature buffers, the reprojected features, rays, hits, the snapshots of the spheres and triangles as
    the previous frame saw them, the denoiser's workspace and the image.  The caller moves the camera (raw.set_camera), moves
    geometry (update_spheres / update_triangles) and rebuilds (build_lbvh_karas) between frame() calls.  The scene's camera must
    be a pinhole, at construction and at every frame."""

    def __init__(self, raw, width, height, spp, max_history=32, sigma_n=DENOISE_SIGMA_N, sigma_p=DENOISE_SIGMA_P, stream=None):
        import torch
        if not _is_pinhole(raw.camera()):
            raise ValueError("TemporalAccumulator needs a pinhole camera: fisheye, panorama and dof_focus 0")
        if not 1 <= int(spp) <= 4096:
            raise ValueError(f"spp is {spp}; expected 1..4096")
        if int(max_history) < 1:
            raise ValueError(f"max_history is {max_history}; expected at least 1")
        self.raw, self.width, self.height, self.spp = raw, int(width), int(height), int(spp)
        self.max_history, self.sigma_n, self.sigma_p = int(max_history), float(sigma_n), float(sigma_p)
        self.params = render_params(self.width, self.height, max(self.spp, 2))
        n = self.n = num_pixels(self.params)
        dev = self.device = torch.device("cuda", raw.device)
        self.stream = stream
        f = dict(dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            self.cur = (torch.zeros(4 * n, **f), torch.zeros(4 * n, **f), torch.zeros(n, dtype=torch.int32, device=dev))
            self.hist = [(torch.zeros(4 * n, **f), torch.zeros(4 * n, **f), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(2)]
            self.features = [torch.zeros((n, 8), **f) for _ in range(2)]
            self.reprojected = torch.zeros((n, 8), **f)
            self.rays = torch.zeros((n, 8), **f)
            self.hits = torch.zeros((n, 6), dtype=torch.int32, device=dev)
            self.prev_xyzr = torch.zeros((raw.desc.num_spheres, 4), **f)
            self.prev_verts = torch.zeros((raw.desc.num_triangles, 9), **f)
            self.work = torch.zeros(10 * n, **f)
            self.filtered = torch.zeros(4 * n, **f)
            self.image = torch.zeros(4 * n, dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        """Forget the history: the next frame is its own samples only.  The sample indices start again at 0."""
        self.frame_index = 0
        self.have_history = False
        self.slot = 0              # hist[slot], features[slot]: the previous merged frame
        self.prev_camera = None

    def frame(self, denoise_iterations=0):
        """One frame of the scene as it is now.  Samples [first, first + spp) of every pixel with first = (frame_index * spp) mod
        (4096 // spp * spp): consecutive frames draw different samples, and the index wraps to 0 before it would pass the
        renderer's limit of 4096 sample indices (after 4096 // spp frames a frame repeats the samples of an earlier one, long
        after max_history has scaled that one away).  Returns (rgba8 uint8 [num_pixels * 4], accum, accum_sq, counts): the image
        and the merged moments, which are the history of the next frame -- they stay valid until the frame after that."""
        raw, w, h, p = self.raw, self.width, self.height, self.params
        cam = raw.camera()
        if not _is_pinhole(cam):
            raise ValueError("TemporalAccumulator needs a pinhole camera: fisheye, panorama and dof_focus 0")
        first = (self.frame_index * self.spp) % (4096 // self.spp * self.spp)
        S, Q, k = self.cur
        old, new = self.slot, 1 - self.slot
        with _device_and_stream(raw.device, self.stream) as (_, s):
            S.zero_(); Q.zero_(); k.zero_()
            render_accumulate_pixels(raw, S, w, h, first, self.spp, None, Q, k, params=p, stream=s)
            # (the un-jittered rays through the pixel centres, not the jittered ones denoise_frame takes: reprojection inverts them)
            _primary_features(raw, render_params(w, h, 0), self.rays, self.hits, self.features[new], s)
            oS, oQ, ok = self.hist[new]
            if self.have_history:
                prev_features(raw, self.rays, self.hits, self.reprojected, self.prev_xyzr if self.prev_xyzr.shape[0] else None,
                              self.prev_verts if self.prev_verts.shape[0] else None, stream=s)
                hS, hQ, hk = self.hist[old]
                temporal_accumulate(oS, oQ, ok, S, Q, k, self.reprojected, hS, hQ, hk, self.features[old], self.prev_camera, w, h,
                                    self.max_history, self.sigma_n, self.sigma_p, params=p, stream=s)
            else:
                oS.copy_(S); oQ.copy_(Q); ok.copy_(k)
            self.prev_camera = cam
            if self.prev_xyzr.shape[0]:
                get_spheres(raw, self.prev_xyzr, stream=s)
            if self.prev_verts.shape[0]:
                get_triangles(raw, self.prev_verts, stream=s)
            self.slot, self.have_history = new, True
            self.frame_index += 1
            if denoise_iterations:
                denoise(self.filtered, oS, oQ, ok, self.features[new], w, h, self.work, int(denoise_iterations), DENOISE_SIGMA_C, self.sigma_n,
                        self.sigma_p, params=p, stream=s)
                finalize(self.image, self.filtered, w, h, 1, params=p, stream=s)
            else:
                finalize_counts(self.image, oS, ok, w, h, params=p, stream=s)
        return self.image, oS, oQ, ok


# Direct light at surface points (include/mirt_light.h): lighting.py holds the extension header's signature and calls
from .lighting import MIRT_LIGHT_RAW, direct_light, pack_features, direct_light_frame      # noqa: E402,F401
# Hemisphere visibility at surface points (include/mirt_visibility.h): visibility.py holds that header's signature and calls
from .visibility import hemisphere_visibility, cosine_directions, rotations, ambient_occlusion_frame      # noqa: E402,F401
# Indirect light at surface points (include/mirt_indirect.h): indirect.py holds that header's signature and calls
from .indirect import indirect_light, indirect_light_frame      # noqa: E402,F401
# Closest-point queries (include/mirt_closest.h): closest.py holds that header's signature and call
from .closest import closest_points, pack_points      # noqa: E402,F401

# Multi-hit ray queries (include/mirt_multihit.h): multihit.py holds that header's signature and calls
from .multihit import trace_rays_multi, count_hits      # noqa: E402,F401
# Contact queries (include_ext/mirt_contacts.h): contacts.py holds that header's signature and calls
from .contacts import closest_points_multi, count_within      # noqa: E402,F401
# Sphere casts (include_ext/mirt_spherecast.h): spherecast.py holds that header's signature and calls
from .spherecast import cast_spheres, pack_casts      # noqa: E402,F401
# Box overlaps (include_ext/mirt_overlap.h): overlap.py holds that header's signature and calls
from .overlap import overlap_boxes, count_overlaps, pack_boxes, voxel_rows, occupancy_grid      # noqa: E402,F401
# Overlap lists (include_ext/mirt_overlap_list.h): overlap_list.py holds that header's signatures and calls
from .overlap_list import list_offsets, list_offsets_work_bytes, overlap_list, overlap_lists, unpack_words, voxel_lists      # noqa: E402,F401
# Ray and ball lists (include_ext/mirt_query_lists.h): query_lists.py holds that header's signatures and calls
from .query_lists import ray_list, ball_list, ray_lists, ball_lists      # noqa: E402,F401
# Triangle overlaps (include_ext2/mirt_overlap_tris.h): overlap_tris.py holds that header's signatures and calls
from .overlap_tris import overlap_triangles, triangle_list, triangle_lists, pack_triangles, scene_triangle_rows      # noqa: E402,F401
# Cast lists (include_ext3/mirt_cast_lists.h): cast_lists.py holds that header's signatures and calls
from .cast_lists import count_casts, cast_list, cast_lists      # noqa: E402,F401


def pack_rays(origins, dirs, tmax=float("inf")):
    """float32 [n, 8] MirtRay rows from origins [n, 3] (or [3]), directions [n, 3] (any non-zero length) and tmax (a number or
    [n]), on the directions' device."""
    import torch
    dirs = torch.as_tensor(dirs, dtype=torch.float32)
    if dirs.dim() != 2 or dirs.shape[1] != 3:
        raise ValueError(f"dirs has shape {list(dirs.shape)}; expected [n, 3]")
    n = dirs.shape[0]
    out = torch.zeros((n, 8), dtype=torch.float32, device=dirs.device)
    out[:, 0:3] = torch.as_tensor(origins, dtype=torch.float32, device=dirs.device)
    out[:, 3] = torch.as_tensor(tmax, dtype=torch.float32, device=dirs.device)
    out[:, 4:7] = dirs
    return out


def unpack_hits(hits):
    """(t, kind, id, normal) views of a [n, 6] hit tensor: t float32 [n] (-1 for a miss), kind / id int32 [n] (MIRT_HIT_*; the
    index into the scene's sphere, triangle or plane array), normal float32 [n, 3]."""
    import torch
    if hits.dim() != 2 or hits.shape[1] != 6 or hits.element_size() != 4:
        raise ValueError(f"hits must be a 4-byte [n, 6] tensor, got {hits.dtype} {list(hits.shape)}")
    f = hits.view(torch.float32)
    i = hits.view(torch.int32)
    return f[:, 0], i[:, 1], i[:, 2], f[:, 3:6]


def write_png(path, rgba_u8_host, width, height):
    """Image::save, libpng.cpp:73-107."""
    import numpy as np
    a = np.ascontiguousarray(rgba_u8_host, dtype=np.uint8)
    assert a.size == width * height * 4
    _check(lib().mirt_write_png(os.fsencode(path), a.ctypes.data, width, height))


def probe_math(which, x, device=0):
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(x)
    _check(lib().mirt_probe_math(device, which, x.size, x.ctypes.data, out.ctypes.data))
    return out


def probe_xorwow(spp, num_streams, draws, device=0):
    import numpy as np
    out = np.zeros((num_streams, draws), dtype=np.uint32)
    _check(lib().mirt_probe_xorwow(device, spp, num_streams, draws, out.ctypes.data))
    return out


def probe_qbox(cases, device=0):
    """mirt_probe_qbox: `cases` is a numpy layouts.QBOX_CASE array [n]; returns a layouts.QBOX_RESULT array [n]."""
    import numpy as np
    from . import layouts
    a = _records(cases, "cases", layouts.QBOX_CASE, None)
    if a is None or a.size == 0:
        raise ValueError("cases must hold at least one case")
    out = np.zeros(a.shape[0], dtype=layouts.QBOX_RESULT)
    _check(lib().mirt_probe_qbox(device, a.shape[0], a.ctypes.data, out.ctypes.data))
    return out


def _probe_words(a, name):
    """`a` as the uint32 [n >= 1] array a probe takes."""
    import numpy as np
    a = _records(a, name, np.dtype(np.uint32), None)
    if a is None or a.size == 0:
        raise ValueError(f"{name} must hold at least one element")
    return a


def probe_sort(mode, keys, device=0):
    """mirt_probe_sort: the build's four-pass sort (mode 0) or the one-byte pass of the sample hand-out (mode 1) over `keys`
    (numpy uint32 [n]); returns (keys_out, vals_out), the sorted keys and where each stood."""
    import numpy as np
    if mode not in (0, 1):
        raise ValueError(f"mode is {mode!r}; expected 0 (the build's sort) or 1 (the low-byte pass)")
    a = _probe_words(keys, "keys")
    keys_out, vals_out = np.zeros_like(a), np.zeros_like(a)
    _check(lib().mirt_probe_sort(device, mode, a.shape[0], a.ctypes.data, keys_out.ctypes.data, vals_out.ctypes.data))
    return keys_out, vals_out


def probe_sched(which, x, device=0):
    """mirt_probe_sched: the cost key of every step count in `x` (which 0), or the chunk order of the chunk costs `x` (which 1);
    `x` is numpy uint32 [n], and so is the result."""
    import numpy as np
    if which not in (0, 1):
        raise ValueError(f"which is {which!r}; expected 0 (cost keys) or 1 (the chunk order)")
    a = _probe_words(x, "x")
    out = np.zeros_like(a)
    _check(lib().mirt_probe_sched(device, which, a.shape[0], a.ctypes.data, out.ctypes.data))
    return out
