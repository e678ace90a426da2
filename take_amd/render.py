"""Host-side mirror of the reference's `render()` (src/render.h:5, src/render.cpp:9-86).

Same argument convention — a parameter list holding a scene file and an optional `-max_depth D`
(default 50, src/render.cpp:14) — and the same result: the image in `Image3` layout (row 0 = top,
`img(x, y)` at [y, x, :]).  The scene file is a `.tkscene`, i.e. a reference `Scene` flattened by
take_amd/host/take_flatten.hpp after the reference's own XML parser ran (the parser is outside this path).
All rendering happens in libtake_hip.so on the current HIP device; without it the call raises.
"""
import numpy as np

from . import cdefs as D
from .capi import Scene, tonemap, tonemap_bloom
from .scene import SceneData, load_tkscene


def parse_params(params):
    """argument handling of src/render.cpp:14-23"""
    max_depth = 50
    filename = None
    i = 0
    while i < len(params):
        if params[i] == "-max_depth":
            i += 1
            max_depth = int(params[i])
        elif filename is None:
            filename = params[i]
        i += 1
    return filename, max_depth


def render(params, seed=0, precision=D.TAKE_PRECISION_F32, ray_epsilon=0.0):
    """render(["scene.tkscene", "-max_depth", "5"]) -> (H, W, 3) numpy image (float32, or float64 in f64 mode).
    An empty parameter list returns an empty image, as the reference does (src/render.cpp:10-12)."""
    if len(params) < 1:
        return np.zeros((0, 0, 3), np.float32)
    filename, max_depth = parse_params(list(params))
    sd = filename if isinstance(filename, SceneData) else load_tkscene(filename)
    scene = Scene(sd, precision=precision)
    try:
        return scene.render(spp=sd.spp, max_depth=max_depth, seed=seed, ray_epsilon=ray_epsilon)
    finally:
        scene.close()


def with_refined_meshes(sd, refined, levels):
    """the description with some meshes replaced by their Loop subdivision: `refined` is {mesh: (positions, indices,
    normals or None, uvs or None)} after `levels` levels.  Face f of such a mesh became the faces 4^levels f ..
    4^levels (f + 1) - 1, so every triangle shape on it becomes that many shapes in its place, and an area light on it
    one light per new shape in the light's place; everything else keeps its order."""
    import copy
    import dataclasses

    out = copy.copy(sd)
    out.meshes = list(sd.meshes)
    for m, (pos, idx, nrm, uv) in refined.items():
        out.meshes[m] = dataclasses.replace(sd.meshes[m], positions=np.ascontiguousarray(pos, np.float64), indices=np.ascontiguousarray(idx, np.int32),
                                            normals=nrm if sd.meshes[m].normals is not None else None, uvs=uv)
    k = 4 ** int(levels)
    split = (sd.shape_kind == 1) & np.isin(sd.shape_ref, list(refined))
    rep = np.where(split, k, 1)
    first = np.concatenate([[0], np.cumsum(rep)])[:-1]  # where an old shape's (first) new shape is
    within = np.arange(int(rep.sum())) - np.repeat(first, rep)
    out.shape_kind, out.shape_ref = np.repeat(sd.shape_kind, rep).astype(np.int32), np.repeat(sd.shape_ref, rep).astype(np.int32)
    out.shape_face = (np.repeat(np.where(split, sd.shape_face.astype(np.int64) * k, sd.shape_face), rep) + within).astype(np.int32)
    out.shape_area_light = np.full(int(rep.sum()), -1, np.int32)
    out.lights = []
    for light in sd.lights:
        if light.kind != 1:  # (a point light, an environment map: no shape)
            out.lights.append(light)
            continue
        for j in range(int(rep[light.shape_id])):
            out.shape_area_light[first[light.shape_id] + j] = len(out.lights)
            out.lights.append(dataclasses.replace(light, shape_id=int(first[light.shape_id] + j)))
    return out


def subdivide_scene(sd, levels, log=None):
    """every triangle mesh of the description refined `levels` levels on the device (capi.Subdiv): positions, indices and
    uvs, and vertex normals where the mesh had them.  A mesh the scheme refuses is named through `log` and left as it is."""
    from .capi import Subdiv, TakeError

    refined = {}
    for m, mesh in enumerate(sd.meshes):
        try:
            with Subdiv(mesh.indices, mesh.positions.shape[0], levels, uvs=mesh.uvs) as sub:
                idx, uv = sub.topology()
                pos, nrm = sub.refine(mesh.positions)
        except TakeError as e:
            if e.code != D.TAKE_E_INVALID:
                raise
            if log:
                log(f"-subdivide: mesh {m} is left as loaded: {e}")
            continue
        refined[m] = (pos, idx, nrm, uv)
    return with_refined_meshes(sd, refined, levels)


def displace_scene(sd, image, scale, bias=0.0, log=None):
    """every triangle mesh of the description that has uvs displaced by the height image (h, w) on the device
    (capi.Displace): positions move along the mesh's own vertex normals where it has them, otherwise along the handle's
    own, and vertex normals are replaced by the displaced surface's where the mesh had them.  A mesh without uvs is named
    through `log` and left as it is."""
    import copy
    import dataclasses

    from .capi import Displace

    out = copy.copy(sd)
    out.meshes = list(sd.meshes)
    for m, mesh in enumerate(sd.meshes):
        if mesh.uvs is None:
            if log:
                log(f"-displace: mesh {m} is left as loaded: it has no uvs")
            continue
        with Displace(mesh.indices, mesh.positions.shape[0], mesh.uvs, image) as dis:
            pos, nrm = dis.apply(mesh.positions, mesh.normals, scale, bias)
        out.meshes[m] = dataclasses.replace(mesh, positions=pos, normals=nrm if mesh.normals is not None else None)
    return out


def parse_displace(params):
    """`-displace FILE,SCALE[,BIAS]` taken out of `params` -> ((h, w) height image, scale, bias), or None without
    -displace; FILE is read as -envmap reads its file (.exr or .npy), of which the first channel is the height"""
    if "-displace" not in params:
        return None
    i = params.index("-displace")
    if i + 1 >= len(params):
        raise SystemExit("-displace needs a value")
    value = params[i + 1]
    del params[i:i + 2]
    try:
        parts = value.split(",")
        if len(parts) not in (2, 3):
            raise ValueError("a file, a scale and an optional bias")
        path, scale, bias = parts[0], float(parts[1]), float(parts[2]) if len(parts) == 3 else 0.0
        if path.endswith(".npy"):
            img = np.load(path)
        elif path.endswith(".exr"):
            from .exr import read_exr

            channels, _ = read_exr(path)
            first = next((c for c in ("R", "Y") if c in channels), None) or sorted(channels)[0]
            img = channels[first].astype(np.float32)
        else:
            raise ValueError(f"unsupported image format: {path}")
        if img.ndim == 3:
            img = img[:, :, 0]
        if img.ndim != 2 or img.dtype not in (np.float32, np.float64):
            raise ValueError(f"{path}: the image must be a float32 or float64 array of shape (h, w) or (h, w, channels)")
        return np.ascontiguousarray(img), scale, bias
    except (ValueError, OSError, IndexError) as e:
        raise SystemExit(f"-displace FILE,SCALE[,BIAS]: {e}")


def imwrite(path, img):
    """the reference's imwrite (src/image.cpp:135-177): `.exr` (half, as tinyexr writes it — take_amd/exr.py) or `.pfm`"""
    if str(path).endswith(".exr"):
        from .exr import write_exr

        write_exr(path, img)
    elif str(path).endswith(".pfm"):
        imwrite_pfm(path, img)
    else:
        raise ValueError(f"Unsupported image format: {path}")


def imwrite_pfm(path, img):
    """PFM as the reference writes it (src/image.cpp:145-153): header `PF\\nW H\\n-1\\n`, float32 RGB rows in
    Image3 order."""
    a = np.ascontiguousarray(img, np.float32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())


def parse_lens(params):
    """`-aperture R [-focus D | -focus_pixel X,Y]` taken out of `params` -> (radius, focus distance, (column, row) or None),
    or None without -aperture; the focus distance is 0 (automatic: the camera's lookat) unless -focus gives one"""
    def take(flag):
        if flag not in params:
            return None
        i = params.index(flag)
        if i + 1 >= len(params):
            raise SystemExit(f"{flag} needs a value")
        value = params[i + 1]
        del params[i:i + 2]
        return value

    aperture, focus, pixel = take("-aperture"), take("-focus"), take("-focus_pixel")
    if aperture is None:
        if focus is not None or pixel is not None:
            raise SystemExit("-focus and -focus_pixel need -aperture")
        return None
    if focus is not None and pixel is not None:
        raise SystemExit("-focus and -focus_pixel exclude each other")
    try:
        xy = None if pixel is None else tuple(int(v) for v in pixel.split(","))
        if xy is not None and len(xy) != 2:
            raise ValueError(pixel)
        return float(aperture), 0.0 if focus is None else float(focus), xy
    except ValueError as e:
        raise SystemExit(f"-aperture R [-focus D | -focus_pixel X,Y]: {e}")


def parse_shutter(params):
    """`-shutter OPEN,CLOSE [-slices K] -from_camera fx,fy,fz,ax,ay,az` taken out of `params` -> (open, close, slices,
    lookfrom, lookat) of the marked frame's camera, or None without -shutter; slices is 0 (the library's default) unless
    -slices gives one"""
    def take(flag):
        if flag not in params:
            return None
        i = params.index(flag)
        if i + 1 >= len(params):
            raise SystemExit(f"{flag} needs a value")
        value = params[i + 1]
        del params[i:i + 2]
        return value

    shutter, slices, cam = take("-shutter"), take("-slices"), take("-from_camera")
    if shutter is None:
        if slices is not None or cam is not None:
            raise SystemExit("-slices and -from_camera need -shutter")
        return None
    if cam is None:
        raise SystemExit("-shutter needs -from_camera: the marked frame's lookfrom and lookat")
    try:
        oc, six = [float(v) for v in shutter.split(",")], [float(v) for v in cam.split(",")]
        if len(oc) != 2 or len(six) != 6:
            raise ValueError("two numbers for -shutter, six for -from_camera")
        return oc[0], oc[1], 0 if slices is None else int(slices), tuple(six[:3]), tuple(six[3:])
    except ValueError as e:
        raise SystemExit(f"-shutter OPEN,CLOSE [-slices K] -from_camera fx,fy,fz,ax,ay,az: {e}")


def parse_envmap(params):
    """`-envmap FILE [-envscale R,G,B]` taken out of `params` -> ((h, w, 3) image, scale or None), or None without -envmap;
    FILE is an .exr (take_amd/exr.read_exr) or a .npy holding a float32 or float64 (h, w, 3) array"""
    def take(flag):
        if flag not in params:
            return None
        i = params.index(flag)
        if i + 1 >= len(params):
            raise SystemExit(f"{flag} needs a value")
        value = params[i + 1]
        del params[i:i + 2]
        return value

    path, scale = take("-envmap"), take("-envscale")
    if path is None:
        if scale is not None:
            raise SystemExit("-envscale needs -envmap")
        return None
    try:
        rgb = None if scale is None else tuple(float(v) for v in scale.split(","))
        if rgb is not None and len(rgb) != 3:
            raise ValueError("three numbers for -envscale")
        if path.endswith(".npy"):
            img = np.load(path)
        elif path.endswith(".exr"):
            from .exr import read_exr

            channels, _ = read_exr(path)
            if not all(c in channels for c in "RGB"):
                raise ValueError(f"{path}: the file has no R, G and B channels")
            img = np.stack([channels[c].astype(np.float32) for c in "RGB"], -1)
        else:
            raise ValueError(f"unsupported image format: {path}")
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"{path}: the image must have shape (h, w, 3)")
        return img, rgb
    except (ValueError, OSError) as e:
        raise SystemExit(f"-envmap FILE [-envscale R,G,B]: {e}")


def main(argv=None):
    """`python -m take_amd.render scene.tkscene [-max_depth D] [-features] [-denoise] [-adaptive [threshold]]
    [-png [linear|reinhard|aces] [-bloom [INTENSITY]]] [-aperture R [-focus D | -focus_pixel X,Y]]
    [-shutter OPEN,CLOSE [-slices K] -from_camera fx,fy,fz,ax,ay,az] [-envmap FILE [-envscale R,G,B]] [-subdivide L]
    [-displace FILE,SCALE[,BIAS]]` — the reference's main.cpp:9-27:
    render, then imwrite("image.exr") into the current directory.  -features (an extension): also the first-hit albedo
    and shading normal of the same camera rays (Scene.render_features), as albedo.exr and normal.exr — what a denoiser
    reads beside the image.  -denoise (an extension): also denoised.exr, the same render filtered on the device with
    the default options (Scene.render_denoised); image.exr is the same bytes with or without it.  -adaptive (an
    extension): also adaptive.exr, the scene's spp as the maximum per pixel and pixels stopped once the relative standard
    error of their mean is at or below `threshold` (default: the library's; Scene.render_adaptive), and one line with
    the samples taken against width * height * spp; image.exr is the same bytes with or without it.  Both -adaptive and
    -denoise: also adaptive_denoised.exr, the adaptive render filtered with the sampler's own variance estimate
    (Scene.render_adaptive_denoised); every other file is the same bytes as without the other flag.  -png (an extension):
    beside every .exr a .png of the same stem — exposure, the tone operator (default aces), the sRGB transfer and 8-bit
    RGBA on the device (capi.tonemap), from the float image that was rendered, not from the halves in the .exr.  All of
    them use ONE exposure, the auto-exposure of image.exr's render, so that image.png, denoised.png and
    adaptive_denoised.png can be compared; one line prints it.  Every .exr is the same bytes with or without the flag.
    -bloom (an extension, needs -png): the .png files get glare around what exceeds the display range after that one
    exposure (capi.tonemap_bloom with the library's threshold and knee, and INTENSITY if the next parameter reads as a
    number); one more line says so; without it every file is the same bytes as before.  -aperture (an extension): a thin lens of
    that radius (Scene.set_lens) set before anything is rendered, focused at -focus D along the view axis, on what pixel
    X,Y (row 0 = top) sees (-focus_pixel; Scene.focus_distance_at), or on the camera's lookat; every file is then of the
    camera with the lens, and one line prints the focus distance in effect.  -shutter (an extension): also shutter.exr,
    camera motion blur (Scene.render_shutter) — the scene file's camera is the current frame, the six numbers of
    -from_camera are lookfrom and lookat of the marked one (up and vfov stay), the exposure lasts from OPEN to CLOSE of
    the interval between them, in K slices (default: the library's); every other file is the same bytes with or without
    it.  Moving placements need the API.  -envmap (an extension): the scene's environment map is replaced by FILE (.exr or
    .npy, (h, w, 3), row 0 = zenith) right after the scene is created (Scene.set_envmap: its tables are built on the device),
    and the light's intensity by -envscale if given; the scene must have an environment-map light; every file is then
    of the scene under the new map.  -subdivide L (an extension): every triangle mesh of the scene is refined by L levels
    of Loop subdivision on the device (subdivide_scene) before the scene is created, vertex normals replaced by the
    refined surface's where the mesh had them; a mesh the scheme refuses (an edge of three faces, a bow-tie, ...) is
    named on stderr and left as loaded; every file is then of the refined scene.  -displace FILE,SCALE[,BIAS] (an
    extension): every triangle mesh with uvs is displaced by SCALE * height + BIAS along its vertex normals on the device
    (displace_scene), after -subdivide and before the scene is created; FILE is read as -envmap's (.exr or .npy), its
    first channel the height; vertex normals are replaced where the mesh had them; a mesh without uvs is named on stderr
    and left as loaded."""
    import sys

    params = list(sys.argv[1:] if argv is None else argv)
    if "-t" in params:  # main.cpp:13-15: thread count of the CPU pool; meaningless here, accepted and dropped
        i = params.index("-t")
        del params[i:i + 2]
    adaptive, threshold = "-adaptive" in params, -1.0
    if adaptive:  # the threshold is optional: the next parameter, if it reads as a number
        i = params.index("-adaptive")
        try:
            threshold = float(params[i + 1])
            del params[i + 1]
        except (IndexError, ValueError):
            pass
        del params[i]
    png_op = None
    if "-png" in params:  # the operator is optional: the next parameter, if it is one of the three words
        i = params.index("-png")
        png_op = "aces"
        if i + 1 < len(params) and params[i + 1] in D.TONEMAP_OPS:
            png_op = params[i + 1]
            del params[i + 1]
        del params[i]
    bloom = None
    if "-bloom" in params:  # the intensity is optional: the next parameter, if it reads as a number
        i = params.index("-bloom")
        bloom = {}
        try:
            bloom = {"intensity": float(params[i + 1])}
            del params[i + 1]
        except (IndexError, ValueError):
            pass
        del params[i]
        if png_op is None:
            raise SystemExit("-bloom needs -png")
    lens = parse_lens(params)
    shutter = parse_shutter(params)
    envmap = parse_envmap(params)
    displace = parse_displace(params)
    subdivide = 0
    if "-subdivide" in params:
        i = params.index("-subdivide")
        try:
            subdivide = int(params[i + 1])
        except (IndexError, ValueError):
            raise SystemExit("-subdivide L: L is the number of levels, 1..6")
        del params[i:i + 2]
        if not 1 <= subdivide <= 6:
            raise SystemExit("-subdivide L: L is the number of levels, 1..6")
    features, denoise = "-features" in params, "-denoise" in params
    params = [p for p in params if p not in ("-features", "-denoise")]
    if not params:
        return 0  # an empty image is not written (src/image.cpp:136-138)
    floats = []  # (stem, float image) of every .exr written from one: what -png transforms

    def imwrite_exr(stem, img):
        imwrite(stem + ".exr", img)
        floats.append((stem, img))

    # render + float -> half + scanline packing on the device (take_hip_render_exr_scanlines); what the host adds is
    # the byte-serial rest of imwrite: ZIP pre-filter, deflate, header (take_amd/exr.py)
    from .exr import write_exr_scanlines

    filename, max_depth = parse_params(params)
    sd = load_tkscene(filename)
    if subdivide:
        sd = subdivide_scene(sd, subdivide, log=lambda line: print(line, file=sys.stderr))
    if displace is not None:
        sd = displace_scene(sd, *displace, log=lambda line: print(line, file=sys.stderr))
    scene = Scene(sd)
    try:
        if envmap is not None:  # before everything else: all the files below are of the scene under the new map
            scene.set_envmap(envmap[0], scale=envmap[1])
        if shutter is not None:  # the marked frame: the other camera, marked; then the scene file's camera again
            scene.set_camera(shutter[3], shutter[4], sd.up, sd.vfov)
            scene.mark_frame()
            scene.set_camera(sd.lookfrom, sd.lookat, sd.up, sd.vfov)
        if lens is not None:  # before every render: all the files below are of the camera with the lens
            radius, focus, pixel = lens
            if pixel is not None:
                focus = scene.focus_distance_at(*pixel)
                if not focus > 0:
                    raise SystemExit(f"-focus_pixel {pixel[0]},{pixel[1]}: the pixel's centre ray hits nothing to focus on")
            scene.set_lens(radius, focus)
            print(f"lens: aperture radius {radius!r}, focus distance {scene.get_lens()['focus_distance']!r}")
        write_exr_scanlines("image.exr", scene.render_exr_scanlines(spp=sd.spp, max_depth=max_depth, seed=0))
        if shutter is not None:
            imwrite_exr("shutter", scene.render_shutter(spp=sd.spp, max_depth=max_depth, seed=0, open=shutter[0], close=shutter[1], slices=shutter[2]))
        if features:
            planes = scene.render_features(spp=sd.spp, seed=0, want=("albedo", "normal"))
            imwrite_exr("albedo", planes["albedo"])
            imwrite_exr("normal", planes["normal"])
        if denoise:
            imwrite_exr("denoised", scene.render_denoised(spp=sd.spp, max_depth=max_depth, seed=0))
        if adaptive:
            img, stats = scene.render_adaptive(spp=sd.spp, max_depth=max_depth, seed=0, threshold=threshold, stats=True)
            imwrite_exr("adaptive", img)
            taken, full = int(stats["count"].sum(dtype=np.int64)), sd.width * sd.height * sd.spp
            print(f"adaptive: {taken} of {full} samples ({100.0 * taken / full:.1f} %)")
        if adaptive and denoise:
            imwrite_exr("adaptive_denoised", scene.render_adaptive_denoised(spp=sd.spp, max_depth=max_depth, seed=0, threshold=threshold))
        if png_op:
            # after every .exr is written: image.exr's render as floats (the halves in the file are not read back), its
            # auto-exposure, and that one exposure for every image
            from .png import write_png

            def display(img, exposure=None):
                if bloom is None:
                    return tonemap(img, exposure=exposure, op=png_op)
                return tonemap_bloom(img, exposure=exposure, op=png_op, **bloom)

            rgba, exposure = display(scene.render(spp=sd.spp, max_depth=max_depth, seed=0))
            write_png("image.png", rgba)
            for stem, img in floats:
                write_png(stem + ".png", display(img, exposure)[0])
            print(f"png: exposure {exposure!r} ({png_op})")
            if bloom is not None:
                print(f"png: bloom intensity {bloom.get('intensity', D.BLOOM_DEFAULTS['intensity'])!r}")
    finally:
        scene.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
