"""The argument errors of the package's Python layer, as a list of (id, thunk): every thunk must raise.

tests/golden/make_api_errors.py records each exception's type name and str() into tests/golden/api_errors.json;
tests/test_api_errors.py replays the list against that file.  Every case fails in Python, or in host-only arithmetic of the
library (mirt_render_num_pixels, mirt_part_pixel_xy, the parser): scenes are the fake ones of the *_abi tests and tensors
live on the CPU, so the list behaves the same with and without a GPU.

What the list cannot reach: a function that checks the device argument by argument stops at its first CPU tensor, so
  - render_accumulate_pixels: every check of d_accum_sq, d_counts and pixels (d_accum's device check comes first);
  - the device check of every tensor but the first one named in a batched device check;
  - everything render_adaptive, denoise_frame and TemporalAccumulator do after their scalar checks (they allocate on the GPU).
Errors that numpy, torch or ctypes word themselves (a string where a number belongs) are left out: their text is not ours.
"""
import types

W, H = 8, 8
N = W * H


def _scene(cam=None, **desc):
    d = types.SimpleNamespace(num_suns=2, num_bulbs=1, num_planes=3, num_spheres=2, num_triangles=1)
    d.__dict__.update(desc)
    return types.SimpleNamespace(device=0, _h=None, desc=d, camera=lambda: cam)


def cases():
    import numpy as np
    import torch

    import cuda_ray_tracer_amd as m
    from cuda_ray_tracer_amd import api, layouts

    out = []

    def case(name, fn):
        assert name not in {n for n, _ in out}, name
        out.append((name, fn))

    f32, f64, i32, i64, u8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
    z = torch.zeros
    raw = _scene()
    striped = api.render_params(W, H, 8, stripe_rows=2, num_parts=2, part=0)

    def pinhole(**fields):
        cam = api.Camera()
        cam.eye, cam.forward, cam.right, cam.up = api.Vec3(0, 0, 0), api.Vec3(0, 0, -1), api.Vec3(1, 0, 0), api.Vec3(0, 1, 0)
        return api._camera_with(cam, fields)

    def tensor_cases(prefix, call, name, good, dtypes_bad, shapes_bad, strided):
        """The cases one tensor argument can show: not a tensor (None, a list, a numpy array), each wrong dtype, each wrong
        shape, not contiguous.  call(**{name: x}) makes the call with that argument replaced."""
        for tag, x in (("none", None), ("list", good.tolist()), ("numpy", good.numpy())):
            case(f"{prefix}:{name}:{tag}", lambda x=x: call(**{name: x}))
        for d in dtypes_bad:
            case(f"{prefix}:{name}:dtype_{str(d).split('.')[-1]}", lambda d=d: call(**{name: good.to(d)}))
        for k, s in enumerate(shapes_bad):
            case(f"{prefix}:{name}:shape{k}", lambda s=s: call(**{name: z(s, dtype=good.dtype)}))
        case(f"{prefix}:{name}:strided", lambda: call(**{name: strided}))

    # ---- host arithmetic ----------------------------------------------------------------------------------------------------
    case("num_pixels:zero_width", lambda: m.num_pixels(api.render_params(0, H, 1)))
    case("num_pixels:part_out_of_range", lambda: m.num_pixels(api.render_params(W, H, 1, 4, 2, 2)))
    case("part_pixel_xy:past_the_part", lambda: api.part_pixel_xy(striped, N // 2))
    case("parseText:bad_line", lambda: m.parseText("png 4 4 a.png\nsphere 0 0\n"))
    case("write_png:size", lambda: m.write_png("unused.png", np.zeros(15, np.uint8), 2, 2))

    # ---- ray queries --------------------------------------------------------------------------------------------------------
    rays, hits, feat = z((5, 8)), z((5, 6), dtype=i32), z((5, 8))
    good = dict(d_rays=rays, d_hits=hits)
    call = lambda good=good, **kw: m.trace_rays(raw, **{**good, **kw})      # noqa: E731
    tensor_cases("trace_rays", call, "d_rays", rays, (f64, i32, torch.float16), ((5, 7), (40,), (5, 8, 1)), z((8, 5)).t())
    tensor_cases("trace_rays", call, "d_hits", hits, (torch.int16, i64, f64), ((4, 6), (5, 5), (30,)), z((5, 12), dtype=i32)[:, ::2])
    case("trace_rays:cpu", lambda call=call: call())
    case("trace_rays:both_bad", lambda call=call: call(d_rays=z((5, 7)), d_hits=None))

    call = lambda **kw: m.camera_rays(raw, **{**dict(d_rays=z((N, 8)), img_width=W, img_height=H, aa=0), **kw})      # noqa: E731
    tensor_cases("camera_rays", call, "d_rays", z((N, 8)), (f64, torch.float16), ((N - 1, 8), (N, 7), (N * 8,)), z((N, 16))[:, ::2])
    case("camera_rays:cpu", lambda call=call: call())
    case("camera_rays:part_shape", lambda call=call: call(params=striped))
    case("camera_rays:part_cpu", lambda call=call: call(params=striped, d_rays=z((N // 2, 8))))
    case("camera_rays:bad_frame", lambda call=call: call(img_width=0))
    case("camera_rays:bad_frame_before_tensor", lambda call=call: call(img_height=-1, d_rays=None))

    # ---- the eight range calls ----------------------------------------------------------------------------------------------
    for fn, cols in (("update_spheres", 4), ("update_triangles", 9), ("update_sphere_materials", 11), ("update_triangle_materials", 11),
                     ("get_sphere_materials", 11), ("get_triangle_materials", 11), ("get_spheres", 4), ("get_triangles", 9)):
        f = getattr(m, fn)
        call = lambda f=f, **kw: f(raw, kw["x"])      # noqa: E731
        tensor_cases(fn, call, "x", z((4, cols)), (f64, i32), ((4, cols + 1), (4 * cols,), (4, cols, 1)), z((cols, 4)).t())
        case(f"{fn}:x:strided_columns", lambda f=f, cols=cols: f(raw, z((4, 2 * cols))[:, ::2]))
        case(f"{fn}:cpu", lambda f=f, cols=cols: f(raw, z((4, cols)), first=1))
        case(f"{fn}:empty_cpu", lambda f=f, cols=cols: f(raw, z((0, cols))))

    # ---- adaptive sampling --------------------------------------------------------------------------------------------------
    acc, cnt, lst = z(4 * N), z(N, dtype=i32), z(5, dtype=i32)
    call = lambda **kw: m.render_accumulate_pixels(raw, **{**dict(d_accum=acc, img_width=W, img_height=H, sample_first=0, sample_count=4), **kw})      # noqa: E731
    tensor_cases("render_accumulate_pixels", call, "d_accum", acc, (f64, i32), ((4 * N - 4,), (N, 3)), z(8 * N)[::2])
    case("render_accumulate_pixels:cpu", lambda call=call: call(pixels=lst, d_accum_sq=acc, d_counts=cnt))
    case("render_accumulate_pixels:part_shape", lambda call=call: call(params=striped))
    case("render_accumulate_pixels:bad_frame", lambda call=call: call(img_width=0, d_accum=None))
    case("render_accumulate_pixels:d_accum_before_the_rest", lambda call=call: call(d_accum=acc.double(), pixels=None, d_accum_sq=[1.0], d_counts=cnt.float()))

    good = dict(d_accum=acc, d_accum_sq=acc.clone(), d_counts=cnt, img_width=W, img_height=H, min_samples=2, max_samples=8, max_variance=0.1,
                d_pixels_out=z(N, dtype=i32), d_num_out=z(1, dtype=i32))
    call = lambda good=good, **kw: m.select_pixels(**{**good, **kw})      # noqa: E731
    for name in ("d_accum", "d_accum_sq"):
        tensor_cases("select_pixels", call, name, acc, (f64, i32), ((4 * N - 4,), (N, 3)), z(8 * N)[::2])
    for name in ("d_counts", "d_pixels_out"):
        tensor_cases("select_pixels", call, name, cnt, (i64, f32), ((N - 1,), (N, 2)), z(2 * N, dtype=i32)[::2])
    for tag, x in (("none", None), ("list", [0]), ("dtype_int64", z(1, dtype=i64)), ("dtype_float32", z(1)), ("two", z(2, dtype=i32)), ("empty", z(0, dtype=i32))):
        case(f"select_pixels:d_num_out:{tag}", lambda x=x, call=call: call(d_num_out=x))      # (one element is always contiguous)
    case("select_pixels:cpu", lambda call=call: call())
    case("select_pixels:order", lambda call=call: call(d_accum_sq=None, d_counts=cnt.float(), d_num_out=z(2, dtype=i32)))
    case("select_pixels:bad_frame", lambda call=call: call(img_height=0, d_accum=None))
    case("select_pixels:part_shape", lambda call=call: call(params=striped))

    good = dict(d_image=z(4 * N, dtype=u8), d_accum=acc, d_counts=cnt, img_width=W, img_height=H)
    call = lambda good=good, **kw: m.finalize_counts(**{**good, **kw})      # noqa: E731
    tensor_cases("finalize_counts", call, "d_image", z(4 * N, dtype=u8), (torch.int8, f32), ((4 * N - 1,), (N, 3)), z(8 * N, dtype=u8)[::2])
    tensor_cases("finalize_counts", call, "d_accum", acc, (f64, u8), ((4 * N - 4,),), z(8 * N)[::2])
    tensor_cases("finalize_counts", call, "d_counts", cnt, (i64, f32), ((N - 1,),), z(2 * N, dtype=i32)[::2])
    case("finalize_counts:cpu", lambda call=call: call())
    case("finalize_counts:order", lambda call=call: call(d_image=None, d_accum=None, d_counts=None))
    case("finalize_counts:bad_frame", lambda call=call: call(img_width=-3, d_image=None))

    for tag, args in (("min_spp_1", (1, 8, 4)), ("min_spp_0", (0, 8, 4)), ("max_below_min", (4, 3, 4)), ("step_0", (4, 8, 0)), ("step_negative", (4, 8, -1))):
        case(f"render_adaptive:{tag}", lambda args=args: m.render_adaptive(raw, W, H, *args, 0.1))
    case("render_adaptive:bad_frame", lambda: m.render_adaptive(raw, 0, H, 2, 8, 2, 0.1))
    case("render_adaptive:range_before_frame", lambda: m.render_adaptive(raw, 0, H, 1, 8, 2, 0.1))

    # ---- denoising ----------------------------------------------------------------------------------------------------------
    call = lambda **kw: m.hit_features(raw, **{**dict(d_rays=rays, d_hits=hits, d_features=feat), **kw})      # noqa: E731
    tensor_cases("hit_features", call, "d_rays", rays, (f64, i32), ((5, 7), (40,)), z((8, 5)).t())
    tensor_cases("hit_features", call, "d_hits", hits, (i64, torch.int16), ((4, 6), (5, 5)), z((5, 12), dtype=i32)[:, ::2])
    tensor_cases("hit_features", call, "d_features", feat, (f64, i32), ((5, 6), (4, 8), (40,)), z((10, 8))[::2])
    case("hit_features:cpu", lambda call=call: call())
    case("hit_features:order", lambda call=call: call(d_hits=hits[:4], d_features=None))

    F, work = z((N, 8)), z(10 * N)
    good = dict(d_out=acc.clone(), d_accum=acc, d_accum_sq=acc.clone(), d_counts=cnt, d_features=F, img_width=W, img_height=H, d_work=work)
    call = lambda good=good, **kw: m.denoise(**{**good, **kw})      # noqa: E731
    for name in ("d_out", "d_accum", "d_accum_sq"):
        tensor_cases("denoise", call, name, acc, (f64, i32), ((4 * N - 4,), (N, 3)), z(8 * N)[::2])
    tensor_cases("denoise", call, "d_counts", cnt, (i64, f32), ((N - 1,),), z(2 * N, dtype=i32)[::2])
    tensor_cases("denoise", call, "d_features", F, (f64, i32), ((N * 8,), (N, 7), (N - 1, 8)), z((2 * N, 8))[::2])
    tensor_cases("denoise", call, "d_work", work, (f64, u8), ((10 * N - 1,), (40 * N,)), z(20 * N)[::2])
    for it in (-1, 9, 100):
        case(f"denoise:iterations_{it}", lambda it=it, call=call: call(iterations=it))
    for name in ("sigma_c", "sigma_n", "sigma_p"):
        for tag, v in (("zero", 0.0), ("negative", -1.0), ("inf", float("inf")), ("nan", float("nan"))):
            case(f"denoise:{name}_{tag}", lambda name=name, v=v, call=call: call(**{name: v}))
    case("denoise:num_parts", lambda call=call: call(params=striped))
    case("denoise:num_parts_before_tensors", lambda call=call: call(params=striped, d_out=None))
    case("denoise:bad_frame", lambda call=call: call(img_width=0, d_out=None))
    case("denoise:tensors_before_iterations", lambda call=call: call(d_work=work[:-1], iterations=9))
    case("denoise:iterations_before_sigmas", lambda call=call: call(iterations=9, sigma_c=0.0))
    case("denoise:sigmas_in_order", lambda call=call: call(sigma_p=0.0, sigma_n=0.0))
    case("denoise:scalars_before_device", lambda call=call: call(sigma_p=float("nan")))
    case("denoise:cpu", lambda call=call: call())
    case("denoise_frame:bad_frame", lambda: m.denoise_frame(raw, acc, acc, cnt, 0, H, 8))

    # ---- temporal accumulation ----------------------------------------------------------------------------------------------
    good = dict(d_rays=rays, d_hits=hits, d_features=feat)
    call = lambda good=good, **kw: m.prev_features(raw, **{**good, **kw})      # noqa: E731
    tensor_cases("prev_features", call, "d_rays", rays, (f64,), ((5, 7), (40,)), z((8, 5)).t())
    tensor_cases("prev_features", call, "d_hits", hits, (i64,), ((4, 6), (5, 5)), z((5, 12), dtype=i32)[:, ::2])
    tensor_cases("prev_features", call, "d_features", feat, (f64,), ((5, 6), (4, 8)), z((10, 8))[::2])
    for name, shape, bad in (("d_prev_xyzr", (2, 4), ((3, 4), (2, 3), (8,))), ("d_prev_verts", (1, 9), ((2, 9), (1, 3, 3), (9,)))):
        for tag, x in (("list", z(shape).tolist()), ("numpy", z(shape).numpy())):      # (None is a value here: that kind did not move)
            case(f"prev_features:{name}:{tag}", lambda name=name, x=x, call=call: call(**{name: x}))
        case(f"prev_features:{name}:dtype_float64", lambda name=name, shape=shape, call=call: call(**{name: z(shape, dtype=f64)}))
        for k, s in enumerate(bad):
            case(f"prev_features:{name}:shape{k}", lambda name=name, s=s, call=call: call(**{name: z(s)}))
        case(f"prev_features:{name}:strided", lambda name=name, shape=shape, call=call: call(**{name: z((2 * shape[0], shape[1]))[::2]}))
    case("prev_features:cpu", lambda call=call: call())
    case("prev_features:cpu_with_previous_geometry", lambda call=call: call(d_prev_xyzr=z((2, 4)), d_prev_verts=z((1, 9))))
    case("prev_features:order", lambda call=call: call(d_features=None, d_prev_xyzr=z((3, 4))))
    case("prev_features:xyzr_before_verts", lambda call=call: call(d_prev_xyzr=z((3, 4)), d_prev_verts=z((2, 9))))

    good = dict(d_out_accum=acc.clone(), d_out_accum_sq=acc.clone(), d_out_counts=cnt.clone(), d_accum=acc, d_accum_sq=acc.clone(), d_counts=cnt,
                d_prev_features=F, d_hist_accum=acc.clone(), d_hist_accum_sq=acc.clone(), d_hist_counts=cnt.clone(), d_hist_features=F.clone(),
                prev_camera=pinhole(), img_width=W, img_height=H)
    call = lambda good=good, **kw: m.temporal_accumulate(**{**good, **kw})      # noqa: E731
    for name in ("d_out_accum", "d_out_accum_sq", "d_accum", "d_accum_sq", "d_hist_accum", "d_hist_accum_sq"):
        tensor_cases("temporal_accumulate", call, name, acc, (f64,), ((4 * N - 4,),), z(8 * N)[::2])
    for name in ("d_out_counts", "d_counts", "d_hist_counts"):
        tensor_cases("temporal_accumulate", call, name, cnt, (f32, i64), ((N - 1,),), z(2 * N, dtype=i32)[::2])
    for name in ("d_prev_features", "d_hist_features"):
        tensor_cases("temporal_accumulate", call, name, F, (f64,), ((N * 8,), (N, 7)), z((2 * N, 8))[::2])
    case("temporal_accumulate:moments_before_counts_before_features", lambda call=call: call(d_hist_features=None, d_out_counts=None, d_hist_accum_sq=None))
    case("temporal_accumulate:counts_before_features", lambda call=call: call(d_prev_features=None, d_hist_counts=None))
    for tag, cam in (("none", None), ("tuple", (0, 0, 0)), ("shading", api.Shading())):
        case(f"temporal_accumulate:prev_camera:{tag}", lambda cam=cam, call=call: call(prev_camera=cam))
    for tag, fields in (("fisheye", dict(fisheye=1)), ("panorama", dict(panorama=1)), ("dof", dict(dof_focus=2.0)), ("dof_nan", dict(dof_focus=float("nan")))):
        case(f"temporal_accumulate:prev_camera:{tag}", lambda fields=fields, call=call: call(prev_camera=pinhole(**fields)))
    for v in (0, -1):
        case(f"temporal_accumulate:max_history_{v}", lambda v=v, call=call: call(max_history=v))
    for name in ("sigma_n", "sigma_p"):
        for tag, v in (("zero", 0.0), ("negative", -1.0), ("inf", float("inf")), ("nan", float("nan"))):
            case(f"temporal_accumulate:{name}_{tag}", lambda name=name, v=v, call=call: call(**{name: v}))
    case("temporal_accumulate:num_parts", lambda call=call: call(params=striped))
    case("temporal_accumulate:num_parts_before_tensors", lambda call=call: call(params=striped, d_out_accum=None))
    case("temporal_accumulate:bad_frame", lambda call=call: call(img_height=0, d_out_accum=None))
    case("temporal_accumulate:tensors_before_camera", lambda call=call: call(d_hist_features=F[:-1], prev_camera=None))
    case("temporal_accumulate:camera_before_max_history", lambda call=call: call(prev_camera=pinhole(fisheye=1), max_history=0))
    case("temporal_accumulate:max_history_before_sigmas", lambda call=call: call(max_history=0, sigma_n=0.0))
    case("temporal_accumulate:sigmas_in_order", lambda call=call: call(sigma_p=0.0, sigma_n=0.0))
    case("temporal_accumulate:cpu", lambda call=call: call())

    for tag, fields in (("fisheye", dict(fisheye=1)), ("panorama", dict(panorama=1)), ("dof", dict(dof_focus=3.0))):
        case(f"TemporalAccumulator:{tag}", lambda fields=fields: m.TemporalAccumulator(_scene(pinhole(**fields)), 33, 17, 8))
    for spp in (0, -1, 4097):
        case(f"TemporalAccumulator:spp_{spp}", lambda spp=spp: m.TemporalAccumulator(_scene(pinhole()), 33, 17, spp))
    for mh in (0, -5):
        case(f"TemporalAccumulator:max_history_{mh}", lambda mh=mh: m.TemporalAccumulator(_scene(pinhole()), 33, 17, 8, max_history=mh))
    case("TemporalAccumulator:camera_before_spp", lambda: m.TemporalAccumulator(_scene(pinhole(fisheye=1)), 33, 17, 0, max_history=0))
    case("TemporalAccumulator:spp_before_max_history", lambda: m.TemporalAccumulator(_scene(pinhole()), 33, 17, 0, max_history=0))
    case("TemporalAccumulator:bad_frame", lambda: m.TemporalAccumulator(_scene(pinhole()), 0, 17, 8))

    def frame_of_a_fisheye():
        t = object.__new__(m.TemporalAccumulator)      # (a constructed one needs a GPU; frame() checks the camera before it touches anything)
        t.raw, t.width, t.height, t.spp, t.params, t.n = _scene(pinhole(fisheye=1)), 33, 17, 8, api.render_params(33, 17, 8), 33 * 17
        t.frame()
    case("TemporalAccumulator.frame:fisheye", frame_of_a_fisheye)

    # ---- camera and shading fields ------------------------------------------------------------------------------------------
    multi = types.SimpleNamespace(_h=None, _keep=types.SimpleNamespace(desc=raw.desc))
    cam, sh = pinhole(), api.Shading(4, 0, float("inf"))
    case("_camera_with:unknown", lambda: api._camera_with(cam, dict(expose=1.0)))
    case("_camera_with:known_then_unknown", lambda: api._camera_with(cam, dict(eye=(1, 2, 3), bounces=2)))
    case("RawConfig.set_camera:unknown", lambda: api.RawConfig.set_camera(raw, cam, gi=1))
    case("RawConfig.set_camera:unknown_on_the_current_camera", lambda: api.RawConfig.set_camera(_scene(cam), position=(0, 0, 0)))
    case("MultiGpu.set_camera:unknown", lambda: api.MultiGpu.set_camera(multi, cam, lens=1.0))
    case("_shading_with:unknown", lambda: api._shading_with(sh, dict(eye=(0, 0, 0))))
    case("_shading_with:known_then_unknown", lambda: api._shading_with(sh, dict(gi=1, exposure=2.0)))
    case("RawConfig.set_shading:unknown", lambda: api.RawConfig.set_shading(raw, sh, fisheye=1))
    case("MultiGpu.set_shading:unknown", lambda: api.MultiGpu.set_shading(multi, sh, fisheye=1))

    # ---- lights and planes --------------------------------------------------------------------------------------------------
    LIGHT, PLANE = layouts.LIGHT, layouts.PLANE
    for who, set_lights, set_planes in (("RawConfig", lambda **kw: api.RawConfig.set_lights(raw, **kw), lambda *a, **kw: api.RawConfig.set_planes(raw, *a, **kw)),
                                        ("MultiGpu", lambda **kw: api.MultiGpu.set_lights(multi, **kw), lambda *a, **kw: api.MultiGpu.set_planes(multi, *a, **kw))):
        for name, count in (("suns", 2), ("bulbs", 1)):
            p = f"{who}.set_lights:{name}"
            case(f"{p}:list", lambda f=set_lights, name=name, count=count: f(**{name: [(0, 1, 0, 1, 1, 1)] * count}))
            case(f"{p}:tensor", lambda f=set_lights, name=name, count=count: f(**{name: z((count, 6))}))
            case(f"{p}:dtype_f32", lambda f=set_lights, name=name, count=count: f(**{name: np.zeros((count, 6), np.float32)}))
            case(f"{p}:dtype_plane", lambda f=set_lights, name=name, count=count: f(**{name: np.zeros(count, PLANE)}))
            case(f"{p}:count", lambda f=set_lights, name=name, count=count: f(**{name: np.zeros(count + 1, LIGHT)}))
            case(f"{p}:empty", lambda f=set_lights, name=name: f(**{name: np.zeros(0, LIGHT)}))
            case(f"{p}:2d", lambda f=set_lights, name=name, count=count: f(**{name: np.zeros((count, 1), LIGHT)}))
            case(f"{p}:strided", lambda f=set_lights, name=name, count=count: f(**{name: np.zeros(2 * count, LIGHT)[::2]}))
        case(f"{who}.set_lights:suns_before_bulbs", lambda f=set_lights: f(suns=np.zeros(3, LIGHT), bulbs=[1]))
        p = f"{who}.set_planes"
        case(f"{p}:list", lambda f=set_planes: f([1, 2, 3]))
        case(f"{p}:tensor", lambda f=set_planes: f(z((2, 21))))
        case(f"{p}:dtype_light", lambda f=set_planes: f(np.zeros(2, LIGHT)))
        case(f"{p}:dtype_f32", lambda f=set_planes: f(np.zeros((2, 21), np.float32)))
        case(f"{p}:2d", lambda f=set_planes: f(np.zeros((2, 1), PLANE)))
        case(f"{p}:0d", lambda f=set_planes: f(np.zeros((), PLANE)))
        case(f"{p}:strided", lambda f=set_planes: f(np.zeros(4, PLANE)[::2], first=1))

    mat = np.zeros(1, layouts.MAT)[0]
    for tag, abcd in (("three", [0, 1, 0]), ("five", [0, 1, 0, 1, 2]), ("2x2", [[0, 1], [0, 1]]), ("scalar", 1.0), ("1x4", [[0, 1, 0, 1]])):
        case(f"make_plane:abcd_{tag}", lambda abcd=abcd: m.make_plane(abcd, mat))

    # ---- introspection ------------------------------------------------------------------------------------------------------
    for tag, x in (("none", None), ("list", [0.0] * 20), ("dtype_f32", np.zeros((3, 20), np.float32)), ("2d", np.zeros((3, 1), layouts.QBOX_CASE)),
                   ("strided", np.zeros(6, layouts.QBOX_CASE)[::2]), ("empty", np.zeros(0, layouts.QBOX_CASE))):
        case(f"probe_qbox:cases:{tag}", lambda x=x: api.probe_qbox(x))
    words = np.arange(6, dtype=np.uint32)
    for fn, probe, name in (("probe_sort", api.probe_sort, "keys"), ("probe_sched", api.probe_sched, "x")):
        for tag, x in (("none", None), ("list", [1, 2, 3]), ("tensor", z(6, dtype=i32)), ("dtype_i32", words.astype(np.int32)), ("dtype_u64", words.astype(np.uint64)),
                       ("dtype_f32", words.astype(np.float32)), ("2d", words.reshape(3, 2)), ("strided", words[::2]), ("empty", words[:0])):
            case(f"{fn}:{name}:{tag}", lambda probe=probe, x=x: probe(0, x))
        for sel in (2, -1, None):
            case(f"{fn}:selector_{sel}", lambda probe=probe, sel=sel: probe(sel, words))
        case(f"{fn}:selector_before_{name}", lambda probe=probe: probe(7, None))

    # ---- packing ------------------------------------------------------------------------------------------------------------
    for tag, dirs in (("flat", [0.0, 0.0, -1.0]), ("two_columns", z((4, 2))), ("four_columns", z((4, 4))), ("3d", z((4, 3, 1))), ("scalar", 1.0)):
        case(f"pack_rays:dirs_{tag}", lambda dirs=dirs: m.pack_rays(z((4, 3)), dirs))
    for tag, h in (("five_columns", z((4, 5))), ("flat", z(24)), ("3d", z((4, 6, 1))), ("int64", z((4, 6), dtype=i64)), ("float16", z((4, 6), dtype=torch.float16)),
                   ("uint8", z((4, 6), dtype=u8)), ("float64", z((4, 6), dtype=f64))):
        case(f"unpack_hits:{tag}", lambda h=h: m.unpack_hits(h))
    return out


def record(fn):
    """(type name, str()) of what fn raises; None when it returns."""
    try:
        fn()
    except Exception as e:      # noqa: BLE001  (the point is to see which)
        return type(e).__name__, str(e)
    return None
