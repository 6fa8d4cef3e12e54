"""Scenes whose films tests/f64_scatter.py predicts pixel by pixel, and the check of a film against that prediction.  Shared by
tests/test_scatter_f64.py (oracle, device code on the CPU) and tests/test_gpu_scatter_f64.py (HIP kernels).  One description
per case gives both the YAML the product loads and the float64 scene of S.ray_colour.  One sample per pixel, seed C.SEED, films
of 64 x 48; the environment is the tagged 64 x 32 map of f64_cases.background_scene, so an escaped path's film value is
(product of attenuations) x texel (i, j)."""
import os

import numpy as np

from tests import f64_cases as C
from tests import f64_reference as F
from tests import f64_scatter as S

W, H = 64, 48
ENV = (64, 32)
WHITE = (1.0, 1.0, 1.0)
_NAMES = {"xy_rect": ("x", "y"), "xz_rect": ("x", "z"), "yz_rect": ("y", "z")}


def lambertian(albedo=WHITE):
    return dict(kind=S.LAMBERTIAN, albedo=albedo)


def metal(roughness, albedo=WHITE):
    return dict(kind=S.METAL, albedo=albedo, roughness=roughness)


def glass(roughness, ior=1.5):
    return dict(kind=S.DIELECTRIC, ior=ior, roughness=roughness)


def light(emit, strength):
    return dict(kind=S.DIFFUSE_LIGHT, emit=emit, strength=strength)


def rect(shape, a, b, k, mat):
    return dict(shape=shape, a=a, b=b, k=k, mat=mat)


def sphere(center, radius, mat):
    return dict(shape="sphere", center=center, radius=radius, mat=mat)


# the PBR two-texel mix: texel 0 (u < 0.5) far below 0.5 in length -> Lambertian, texel 1 far above -> Metal of PBR_RHO
MIX_BYTES = np.array([[[30, 20, 10], [200, 180, 160]]], np.uint8)             # lengths 0.147 and 1.23 (ImageTexture: byte / 255)
MIX_LEN = np.sqrt(((MIX_BYTES[0].astype(np.float64) / 255.0) ** 2).sum(-1))
PBR_RHO = 0.4


def pbr_mix(ob):
    """The material of a PBR rect whose mix texture is MIX_BYTES, resolved at the hit point: u along the rect's first axis
    (aarect.h), texel int(u * 2).  -> f(rec, flip) -> (material, texel ambiguous)."""
    ax = [i for i in range(3) if i != S._RECT_AXES[ob["shape"]]][0]

    def resolve(rec, flip):
        u = (rec["p"][..., ax] - ob["a"][0]) / (ob["a"][1] - ob["a"][0])
        i, lo, hi, amb = F.band(lambda x: F.image_i(x, 2), u, F.EPS * (1.0 + np.abs(rec["p"]).max(-1)) / (ob["a"][1] - ob["a"][0]))
        if flip:
            i = np.where(amb, 1 - i, i)
        return dict(kind=S.PBR, albedo=WHITE, roughness=PBR_RHO, mix=MIX_LEN[i]), amb
    return resolve


FLOOR = dict(a=(-6.0, 6.0), b=(-7.5, -0.5), k=0.0)                    # an xz_rect seen from (0, 1.5, 0) towards (0, 0, -2.6): 60 degrees
CAM_60 = dict(look_from=(0.0, 1.5, 0.0), look_at=(0.0, 0.0, -2.6), up=(0, 1, 0), fov=40)
CAM_BELOW = dict(look_from=(0.0, -1.5, 0.0), look_at=(0.0, 0.0, -2.6), up=(0, 1, 0), fov=30)   # incidence >= 45 > asin(1 / 1.5)
CAM_FRONT = dict(look_from=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0, 1, 0), fov=60)
BALL = dict(center=(0.1, -0.05, -3.0), radius=1.1)
PANEL = dict(a=(-1.5, 1.7), b=(-0.9, 1.1), k=-3.0)                    # an xy_rect in front of CAM_PANEL, its four edges in view
CAM_PANEL = dict(look_from=(0.1, 0.05, 0.0), look_at=(0.1, 0.05, -1.0), up=(0, 1, 0), fov=75)
CAM_PANEL_BACK = dict(look_from=(0.1, 0.05, -6.0), look_at=(0.1, 0.05, -5.0), up=(0, 1, 0), fov=75)
WALL = dict(a=(-10.0, 10.0), b=(0.2, 12.0), k=-8.0)                   # an xy_rect the floor's mirror image looks at
TINT = (0.5, 0.25, 1.0)
EMIT, STRENGTH = (0.9, 0.5, 0.2), 3.5
BG = (0.2, 0.5, 0.9)
MEDIUM_DENSITY = 3.0
CAM_MEDIUM = dict(look_from=(0.1, 0.1, 4.0), look_at=(0.1, 0.1, 0.0), up=(0, 1, 0), fov=35)


def _floor(mat):
    return rect("xz_rect", mat=mat, **FLOOR)


def _pbr_floor():
    ob = _floor(None)
    ob["mat"] = pbr_mix(ob)
    ob["yaml_mat"] = "pbr"
    return ob


# name -> dict(cam, scene, max_depth, background: "sky" or a colour)
CASES = {
    # 1, 5: Lambertian sphere: the texel along n + sph on the sphere, the primary texel off it; black at depth 1
    "lambert_sphere_d2": dict(cam=CAM_FRONT, scene=[sphere(mat=lambertian(), **BALL)], max_depth=2),
    "lambert_sphere_d1": dict(cam=CAM_FRONT, scene=[sphere(mat=lambertian(), **BALL)], max_depth=1),
    # 2: rough Metal at 60 degrees: the texel, or black where absorbed
    "rough_metal_d2": dict(cam=CAM_60, scene=[_floor(metal(0.5))], max_depth=2),
    # 3: glass: a reflected or a transmitted texel by the float64 coin; from below, beyond the critical angle, all reflected
    "glass_smooth_d2": dict(cam=CAM_60, scene=[_floor(glass(0.0))], max_depth=2),
    "glass_rough_d2": dict(cam=CAM_60, scene=[_floor(glass(0.2))], max_depth=2),
    "glass_below_d2": dict(cam=CAM_BELOW, scene=[_floor(glass(0.0))], max_depth=2, all_tir=True),
    # 4: camera -> tinted mirror -> white Lambertian wall -> sky: atten *= attenuation, the bounce field of the key, so = rec.p
    "mirror_wall_d3": dict(cam=CAM_60, scene=[_floor(metal(0.0, TINT)), rect("xy_rect", mat=lambertian(), **WALL)], max_depth=3,
                           three_segments=True),
    "mirror_wall_d2": dict(cam=CAM_60, scene=[_floor(metal(0.0, TINT)), rect("xy_rect", mat=lambertian(), **WALL)], max_depth=2),
    # 6: constant background: film = attenuation x background
    "const_bg_lambert_d2": dict(cam=CAM_FRONT, scene=[sphere(mat=lambertian((0.8, 0.4, 0.3)), **BALL)], max_depth=2, background=BG),
    "const_bg_uvtest_d2": dict(cam=CAM_PANEL, scene=[rect("xy_rect", mat=dict(kind=S.UVTEST), **PANEL)], max_depth=2, background=BG),
    # ... and on the sphere, where the normal varies: every channel, negative components included, is normal x background, to
    # rtol 1e-6 plus the error the normal (p - c) / r inherits from the fp32 hit point (S.ray_colour's atten_err, ~ 1e-4)
    "const_bg_uvtest_sphere_d2": dict(cam=CAM_FRONT, scene=[sphere(mat=dict(kind=S.UVTEST), **BALL)], max_depth=2, background=BG),
    # 7: DiffuseLight: emit * strength on both faces, at depth 1 and 5; in a tinted mirror: result += atten * emitted, atten = TINT
    "light_front_d1": dict(cam=CAM_PANEL, scene=[rect("xy_rect", mat=light(EMIT, STRENGTH), **PANEL)], max_depth=1),
    "light_front_d5": dict(cam=CAM_PANEL, scene=[rect("xy_rect", mat=light(EMIT, STRENGTH), **PANEL)], max_depth=5),
    "light_back_d1": dict(cam=CAM_PANEL_BACK, scene=[rect("xy_rect", mat=light(EMIT, STRENGTH), **PANEL)], max_depth=1),
    "light_back_d5": dict(cam=CAM_PANEL_BACK, scene=[rect("xy_rect", mat=light(EMIT, STRENGTH), **PANEL)], max_depth=5),
    "light_in_mirror_d3": dict(cam=CAM_60, scene=[_floor(metal(0.0, TINT)), rect("xy_rect", mat=light(EMIT, STRENGTH), **WALL)], max_depth=3,
                               lit=True),
    # 8: Isotropic in a ConstantMedium box: free path, ballRand keyed bounce 0, a second free path keyed bounce 1
    "medium_d2": dict(cam=CAM_MEDIUM, scene=[dict(shape="medium", geom=C.MEDIUM_BOX, density=MEDIUM_DENSITY, albedo=WHITE)], max_depth=2,
                      medium=True),
    # 9: the PBR two-texel mix: the left half scatters as a Lambertian, the right half as a Metal of PBR_RHO
    "pbr_mix_d2": dict(cam=CAM_60, scene=[_pbr_floor()], max_depth=2, pbr=True),
}


def _material_yaml(name, mat):
    if mat == "pbr":
        return f"  - name: {name}\n    type: pbr\n    albedo: {C._vec(WHITE)}\n    metalness: 0.0\n    roughness: {PBR_RHO}\n"
    k = mat["kind"]
    y = f"  - name: {name}\n    type: {k}\n"
    if k in (S.LAMBERTIAN, S.METAL):
        y += f"    albedo: {C._vec(mat['albedo'])}\n"
    if k == S.METAL:
        y += f"    roughness: {mat['roughness']}\n"
    if k == S.DIELECTRIC:
        y += f"    ior: {mat['ior']}\n    roughness: {mat['roughness']}\n"
    if k == S.DIFFUSE_LIGHT:
        y += f"    albedo: {C._vec(mat['emit'])}\n    strength: {mat['strength']}\n"
    return y


def _object_yaml(ob, mat_name):
    if ob["shape"] == "sphere":
        return f"  - type: sphere\n    center: {C._vec(ob['center'])}\n    radius: {ob['radius']}\n    material: {mat_name}\n"
    if ob["shape"] == "medium":
        lo, hi = ob["geom"]
        return (f"  - type: constant_medium\n    density: {ob['density']}\n    colour: {C._vec(ob['albedo'])}\n    boundary:\n"
                f"        type: box\n        min: {C._vec(lo)}\n        max: {C._vec(hi)}\n")
    a, b = _NAMES[ob["shape"]]
    return (f"  - type: {ob['shape']}\n    {a}: {C._vec(ob['a'])}\n    {b}: {C._vec(ob['b'])}\n    k: {ob['k']}\n"
            f"    material: {mat_name}\n")


def _carrier(cs):
    """The sphere that carries the PBR case's mix image into the flat scene: above and behind the camera, where no traced path
    goes (predict() asserts it).  Its float64 stand-in is a light, so that a path reaching it would show as emitted."""
    c = np.asarray(cs["cam"]["look_from"], float) + [0.0, 60.0, 60.0]
    return sphere(tuple(c), 0.5, light(WHITE, 1.0))


def build_scene(tmp_path, name):
    """The HostScene of CASES[name].  A PBR's mix texture cannot be named in a scene file (scene.cpp builds the PBR of constants
    only), so the PBR case declares the image on a carrier material and points the flattened PBR's mix_tex at it."""
    from hobbyraytracer_amd import api
    cs = CASES[name]
    d = str(tmp_path)
    bg = cs.get("background", "sky")
    y = C._camera_yaml(W, H, cs["cam"]["look_from"], cs["cam"]["look_at"], cs["cam"]["up"], cs["cam"]["fov"], 0.0, 1.0,
                       "sky" if bg == "sky" else C._vec(bg))
    tex = ""
    if bg == "sky":
        EW, EH = ENV
        img = np.zeros((EH, EW, 3), np.uint8)
        img[..., 0] = np.arange(EW)[None, :]
        img[..., 1] = np.arange(EH)[:, None]
        img[..., 2] = C.ENV_TAG
        api.write_image(os.path.join(d, "env.png"), img)
        tex += "  - name: sky\n    type: environment\n    path: env.png\n"
    mats, objs = "", ""
    for i, ob in enumerate(cs["scene"]):
        if ob["shape"] != "medium":
            mats += _material_yaml(f"m{i}", ob.get("yaml_mat", ob["mat"]))
        objs += _object_yaml(ob, f"m{i}")
    if cs.get("pbr"):
        api.write_image(os.path.join(d, "mix.png"), MIX_BYTES)
        tex += "  - name: mix\n    type: image\n    path: mix.png\n"
        mats += "  - name: carrier\n    type: lambertian\n    albedo: mix\n"
        objs += _object_yaml(_carrier(cs), "carrier")
    if not mats:
        mats = "  - name: unused\n    type: lambertian\n    albedo: [0.5, 0.5, 0.5]\n"
    y += ("textures:\n" + tex if tex else "") + "materials:\n" + mats + "objects:\n" + objs
    p = os.path.join(d, f"{name}.yaml")
    with open(p, "w") as f:
        f.write(y)
    hs = api.HostScene(p, d)
    if cs.get("pbr"):
        point_pbr_mix_at_image(hs)
    return hs


def point_pbr_mix_at_image(hs, which=None):
    """Makes the scene's one PBR read its mix from the scene's two-texel image (or the one texture `which` accepts)."""
    from hobbyraytracer_amd import api
    fs = hs.flat_ptr.contents
    which = which or (lambda t: t.kind == api.TEX_IMAGE and t.width == 2)
    img = [t for t in range(fs.n_textures) if which(fs.textures[t])]
    pbr = [m for m in range(fs.n_materials) if fs.materials[m].kind == api.MAT_PBR]
    assert len(img) == 1 and len(pbr) == 1
    fs.materials[pbr[0]].mix_tex = img[0]


def _decode(q):
    """(bytes, valid): the PNG byte each value decodes to (stbi_loadf's (b / 255)^2.2, f64_cases._LDR) and whether it is one."""
    k = np.abs(q[..., None] - C._LDR).argmin(-1)
    return k, (np.abs(q - C._LDR[k]) <= 1e-5 * np.maximum(C._LDR[k], 1e-6)).all(-1)


def _matches(film, r, bg, loose):
    """Per pixel: does the film value equal outcome r?  Escaped: emitted + atten x (the predicted texel | the background colour);
    else emitted alone (black where nothing was emitted).  rtol 1e-6 per channel: the film tolerance DESIGN.md 2 states."""
    film = film.reshape(-1, 3).astype(np.float64)
    ended = (np.abs(film - r["emitted"]) <= 1e-6 * np.abs(r["emitted"])).all(-1)
    if bg != "sky":
        bg = np.asarray(bg, np.float32).astype(np.float64)
        want = r["emitted"] + r["atten"] * bg
        # atten_err: 0 but for a UVTest on a sphere, whose attenuation, the normal, has the hit point's fp32 error
        esc = (np.abs(film - want) <= 1e-6 * np.abs(want) + r["atten_err"][:, None] * bg).all(-1)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            k, valid = _decode(np.nan_to_num((film - r["emitted"]) / r["atten"], posinf=-1.0, neginf=-1.0))
        gi, gj, tag = k[..., 0], k[..., 1], k[..., 2]
        if loose:
            same = ((gi == r["ilo"]) | (gi == r["ihi"]) | (gi == r["i"])) & ((gj == r["jlo"]) | (gj == r["jhi"]) | (gj == r["j"]))
        else:
            same = (gi == r["i"]) & (gj == r["j"])
        esc = valid & (tag == C.ENV_TAG) & same
    return np.where(r["escaped"], esc, ended)


def predict(name):
    """(the float64 outcome of every pixel, its other outcome where a decision is ambiguous), computed once per case."""
    if name not in _PREDICTED:
        cs = CASES[name]
        cam = dict(cs["cam"], W=W, H=H)
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        o, d = F.primary_rays(C.f64_camera(cam), W, H, px, py, 0, C.SEED_LO, C.SEED_HI)
        key = dict(seed_lo=C.SEED_LO, seed_hi=C.SEED_HI, pixel=(py * W + px).ravel().astype(np.uint64), sample=0)
        env = ENV if cs.get("background", "sky") == "sky" else None
        o, d = np.broadcast_to(o, d.shape).reshape(-1, 3), d.reshape(-1, 3)
        if cs.get("pbr"):          # the carrier sphere is in the rendered scene only: no path of either outcome may reach it
            for f in (False, True):
                with_carrier = S.ray_colour(cs["scene"] + [_carrier(cs)], o, d, key, cs["max_depth"], env=env, flip=f)
                assert not with_carrier["emitted"].any(), "a path reaches the sphere that carries the mix image"
        _PREDICTED[name] = tuple(S.ray_colour(cs["scene"], o, d, key, cs["max_depth"], env=env, flip=f) for f in (False, True))
    return _PREDICTED[name]


_PREDICTED = {}


def check_film(film, name):
    """Black where the reference says black, the predicted texel (or attenuation x background) where the path is unambiguous, one
    of the two float64 outcomes and their neighbouring texels inside the band.  -> ambiguous share (asserted below 2 %)."""
    cs = CASES[name]
    bg = cs.get("background", "sky")
    assert film.shape == (H, W, 3) and np.isfinite(film).all()
    r, r2 = predict(name)
    amb = r["ambiguous"] | r2["ambiguous"]
    frac = float(amb.mean())
    assert frac < C.MAX_AMBIGUOUS, f"ambiguity band too wide: {frac:.4f}"
    strict = _matches(film, r, bg, False)
    bad = ~amb & ~strict
    assert not bad.any(), _describe(bad, film, r)
    loose = _matches(film, r, bg, True) | _matches(film, r2, bg, True)
    bad = amb & ~loose
    assert not bad.any(), "in the band: " + _describe(bad, film, r)
    # the case shows what it is there to show
    assert (r["escaped"] & (r["depth"] == 1)).mean() < 0.85, "the object must fill a good part of the view"
    if cs.get("all_tir"):
        assert (r["direction"][r["escaped"] & (r["depth"] == 2), 1] < 0).all(), "beyond the critical angle every path is reflected"
    if cs.get("three_segments"):
        assert (r["escaped"] & (r["depth"] == 3)).mean() > 0.15, "camera -> mirror -> wall -> sky must be a good part of the view"
    if cs.get("lit"):
        assert ((r["emitted"] > 0).all(-1) & (r["depth"] == 2)).mean() > 0.25, "the light must be seen in the mirror"
    if cs.get("medium"):
        inside = r["depth"] == 2
        assert (r["escaped"] & inside).sum() >= 0.25 * inside.sum() and (~r["escaped"] & inside).sum() >= 0.1 * inside.sum()
    return frac


def _describe(bad, film, r):
    a = int(np.nonzero(bad)[0][0])
    want = f"texel ({r['i'][a]}, {r['j'][a]}) x {r['atten'][a]}" if r["escaped"][a] and "i" in r else \
        ("background x " + str(r["atten"][a]) if r["escaped"][a] else "no escape")
    return (f"{int(bad.sum())} pixels differ from the float64 path, first: pixel ({a % W}, {a // W}) got {film.reshape(-1, 3)[a]}, "
            f"expected {want} + emitted {r['emitted'][a]} after {r['depth'][a]} segments")
