"""Float64 restatement of Material::scatter (material.h:73-242, material.cpp:18-28, hobbyraytracer.h:34-38) and of the rayColour
loop (main.cpp:38-79), written from those lines and from glm's published formulas (gtc/random.inl: linearRand, sphericalRand,
ballRand; detail/func_geometric.inl: reflect, refract, normalize) plus the counter layout of csrc/hrt_rng.h.  numpy only, one
vertex further down the path than tests/f64_reference.py, whose Philox, primary rays, intersections and free path it reuses.
glm itself is not on the test machines: this pins the published formulas, not glm's binary.

Every decision a scatter takes (absorbed or not, reflected / refracted / total internal reflection, the PBR mix, nearZero, a
ballRand attempt accepted or not) comes with a MARGIN: the distance of the decided quantity from its threshold divided by that
quantity's scale.  A ray whose margin is below F.EPS (64 * 2^-24) is ambiguous: fp32 may decide either way, so callers compute
the other outcome as well (`flip`) and accept both; they assert that fewer than 2 % of their rays are ambiguous."""
import numpy as np

from tests import f64_reference as F

LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT, ISOTROPIC, PBR, UVTEST = \
    "lambertian", "metal", "dielectric", "diffuse_light", "isotropic", "pbr", "uv_test"
TWO_PI_F32 = float(np.float32(6.283185307179586476925286766559))     # glm::linearRand(0.0f, 6.2831...f): the literal as a float
EPS_F32 = float(np.finfo(np.float32).eps)                            # std::numeric_limits<float>::epsilon()
T_MIN = float(np.float32(0.001))                                     # main.cpp:45
# Absolute error allowed on a component of a scattered direction built from sphericalRand: the <= 4 ulp libm restatement
# (tests/test_glm_math.py) gives 4 ulps on phi <= pi and on theta <= 2 pi, times a unit-size product, ~ 2.5e-6
# (tests/test_oracle_kats.py uses the same bound for the same quantities).
SD_ATOL = 5e-6
# A rect's hit point is fl(o + fl(t d)) with t = fl((k - o_ax) / d_ax): three roundings of values no larger than |o_ax| + |k|,
# so its coordinate on the rect's axis lies within 2 ulps of k; 8 leaves a factor of four.  (The general band, 64 ulps of the
# whole point's magnitude, would call every ray that leaves a rect at a shallow angle ambiguous.)
SELF_ULPS = 8
MIRROR_ATOL = 3e-7                                                   # a smooth metal's direction: no libm call in it


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _unit(a):
    return a / _norm(a)[..., None]


# ------------------------------------------------------------------ draws (gtc/random.inl)
def spherical_rand(u_theta, u_z):
    """glm::sphericalRand(1): theta = linearRand(0, 2 pi), phi = acos(linearRand(-1, 1)); (sin phi cos theta, sin phi sin theta,
    cos phi).  linearRand(a, b) = u * (b - a) + a with u = u01(word)."""
    theta = F.u01(u_theta) * TWO_PI_F32
    phi = np.arccos(F.u01(u_z) * 2.0 - 1.0)
    return np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], -1)


def fresnel_coin(z, w):
    """glm::linearRand(0.0, 1.0), a double: 53 bits of (z << 32 | w)."""
    v = (np.asarray(z, np.uint64) << np.uint64(32)) | np.asarray(w, np.uint64)
    return (v >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def ball_rand(key, flip=None):
    """glm::ballRand(1): linearRand(vec3(-1), vec3(1)) until length <= 1; attempt a = 0, 1, ... is the draw (RNG_BALL, aux = a),
    words x, y, z.  flip: (n,) bool, the rays whose attempt nearest the unit sphere is decided the other way.
    -> (r, number of attempts, margin: the smallest | |r| - 1 | over the attempts made, the attempt that margin belongs to)."""
    n = np.shape(key["pixel"])
    nearest = None
    if flip is not None and np.any(flip):
        nearest = ball_rand(key)[3]
    r = np.zeros(n + (3,))
    attempts = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    which = np.zeros(n, np.int64)
    todo = np.ones(n, bool)
    for a in range(64):
        if not todo.any():
            break
        w = F.draw(key["seed_lo"], key["seed_hi"], key["pixel"], key["sample"], key["bounce"], F.RNG_BALL, a)
        cand = np.stack([F.u01(w[k]) * 2.0 - 1.0 for k in range(3)], -1)
        ln = _norm(cand)
        r[todo] = cand[todo]
        attempts[todo] = a + 1
        m = np.abs(ln - 1.0)
        closer = todo & (m < margin)
        margin[closer] = m[closer]
        which[closer] = a
        reject = ln > 1.0
        if nearest is not None:
            reject = reject ^ (flip & (nearest == a))
        todo &= reject
    return r, attempts, margin, which


def reflect(i, n):
    """glm::reflect: I - N * dot(N, I) * 2."""
    return i - n * (_dot(n, i) * 2.0)[..., None]


def refract(i, n, eta):
    """glm::refract: k = 1 - eta^2 (1 - dot(N, I)^2); k < 0 ? 0 : eta I - (eta dot(N, I) + sqrt(k)) N."""
    d = _dot(n, i)
    k = 1.0 - eta * eta * (1.0 - d * d)
    out = eta[..., None] * i - (eta * d + np.sqrt(np.maximum(k, 0.0)))[..., None] * n
    return np.where((k < 0)[..., None], 0.0, out)


# ------------------------------------------------------------------ Material::scatter
def _decide(name, value, threshold, scale, margins, flip):
    """value > threshold, its margin |value - threshold| / scale recorded; flipped where flip[name] says so."""
    margins[name] = np.abs(value - threshold) / scale
    dec = value > threshold
    if flip is not None and name in flip:
        dec = dec ^ flip[name]
    return dec


def scatter(mat, rec, d_in, key, flip=None, words=("x", "y", "z", "w")):
    """Material::scatter for n rays.  mat: kind plus, as the kind needs them, albedo (3,) or (n, 3), roughness, ior, emit,
    strength, mix (the length of the mix texture's colour), each a scalar or (n,): a MatScalar read from a texture is the length
    of its rgb, which the caller passes.  rec: p, normal (n, 3), front_face (n,).  d_in: (n, 3), any length.  key: seed_lo,
    seed_hi, pixel, sample, bounce.  flip: {decision: (n,) bool} inverts these decisions for these rays (the other float64
    outcome of an ambiguous ray).  words: which words of the RNG_SCATTER draw play x, y (sphericalRand) and z, w (the coin);
    only a test's self-check passes another order.
    -> dict(scattered, sd, attenuation, emitted, margins {decision: (n,)}, attempts)."""
    kind = mat["kind"]
    nrm = np.asarray(rec["normal"], np.float64)
    n = nrm.shape[:-1]
    d_in = np.asarray(d_in, np.float64)
    margins = {}
    zero3 = np.zeros(n + (3,))
    out = dict(scattered=np.ones(n, bool), sd=zero3, attenuation=zero3, emitted=zero3, margins=margins, attempts=np.zeros(n, np.int64))

    def vec(v):
        return np.broadcast_to(np.asarray(v, np.float64), n + (3,))

    def scal(v):
        return np.broadcast_to(np.asarray(v, np.float64), n)

    if kind == DIFFUSE_LIGHT:      # material.h:96-104: no frontFace test
        out["scattered"] = np.zeros(n, bool)
        out["emitted"] = vec(mat["emit"]) * scal(mat["strength"])[..., None]
        return out
    if kind == ISOTROPIC:          # material.h:79-85
        r, attempts, m, _ = ball_rand(key, None if flip is None else flip.get("ball"))
        margins["ball"] = m
        out.update(sd=r, attenuation=vec(mat["albedo"]), attempts=attempts)
        return out
    w = dict(zip("xyzw", F.draw(key["seed_lo"], key["seed_hi"], key["pixel"], key["sample"], key["bounce"], F.RNG_SCATTER)))
    sph = spherical_rand(w[words[0]], w[words[1]])
    coin = fresnel_coin(w[words[2]], w[words[3]])

    def lambertian():              # material.h:137-153 / 116-129
        sd = nrm + sph
        nz = ~_decide("near_zero", np.abs(sd).max(-1), 1e-8, 1.0, margins, flip)
        return np.where(nz[..., None], nrm, sd)

    def metal():                   # material.h:166-177
        nn = _unit(nrm)
        refl = reflect(_unit(d_in), nn)
        rho = np.minimum(np.abs(scal(mat["roughness"])), 1.0)           # glm::length of a float, then "< 1 ? r : 1"
        sd = refl + rho[..., None] * sph + EPS_F32
        ok = _decide("absorbed", _dot(sd, nn), 0.0, _norm(sd), margins, flip)
        return sd, ok

    if kind in (LAMBERTIAN, UVTEST):
        out.update(sd=lambertian(), attenuation=nrm if kind == UVTEST else vec(mat["albedo"]))
        return out
    if kind == METAL:
        sd, ok = metal()
        out.update(sd=sd, scattered=ok, attenuation=vec(mat["albedo"]))
        return out
    if kind == PBR:                # material.cpp:18-28
        is_metal = _decide("mix", scal(mat["mix"]), 0.5, 0.5, margins, flip)
        sd_m, ok = metal()
        sd_l = lambertian()
        margins["absorbed"] = np.where(is_metal, margins["absorbed"], np.inf)
        margins["near_zero"] = np.where(is_metal, np.inf, margins["near_zero"])
        out.update(sd=np.where(is_metal[..., None], sd_m, sd_l), scattered=np.where(is_metal, ok, True), attenuation=vec(mat["albedo"]))
        return out
    assert kind == DIELECTRIC      # material.h:204-241
    ior = scal(mat["ior"])
    ratio = np.where(rec["front_face"], 1.0 / ior, ior)
    unit = _unit(d_in)
    cos_t = np.minimum(_dot(-unit, nrm), 1.0)
    sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    cannot = _decide("tir", ratio * sin_t, 1.0, 1.0, margins, flip)
    r0 = ((1.0 - ratio) / (1.0 + ratio)) ** 2
    ref = r0 + (1.0 - r0) * (1.0 - cos_t) ** 5
    by_coin = _decide("coin", ref, coin, 1.0, margins, flip)
    margins["coin"] = np.where(cannot, np.inf, margins["coin"])
    reflected = cannot | by_coin
    direction = np.where(reflected[..., None], reflect(unit, nrm), refract(unit, nrm, ratio))
    out.update(sd=direction + scal(mat.get("roughness", 0.0))[..., None] * sph, attenuation=np.ones(n + (3,)), reflected=reflected,
               schlick=ref, coin=coin, tir=cannot)
    return out


def ambiguous(margins):
    """{decision: margin below F.EPS} and their union."""
    masks = {k: m < F.EPS for k, m in margins.items()}
    any_ = np.zeros(next(iter(margins.values())).shape, bool) if margins else False
    for m in masks.values():
        any_ = any_ | m
    return masks, any_


# ------------------------------------------------------------------ hit records, float64 (aarect.h, sphere.cpp:20-46, hittable.h:21-24)
_RECT_AXES = {"yz_rect": 0, "xz_rect": 1, "xy_rect": 2}


def face_normal(d, outward):
    front = _dot(d, outward) < 0
    return front, np.where(front[..., None], outward, -outward)


def _hit_object(ob, o, d, perr, derr, on_self, self_err):
    """(t, hit, ambiguous) of one object for rays (o, d); t_min = 0.001, t_max = inf.  perr, derr: the absolute fp32 error
    already carried by the origin and the direction.  on_self: the rays that start on this very object (the previous vertex);
    self_err: how far from its plane fp32 may have put that origin (SELF_ULPS)."""
    L = _norm(d)
    scale = _norm(o) + 1.0
    if ob["shape"] in _RECT_AXES:
        ax = _RECT_AXES[ob["shape"]]
        with np.errstate(invalid="ignore"):
            t, p, inside = F.rect_hit(o, d, ax, *ob["a"], *ob["b"], ob["k"])
        with np.errstate(invalid="ignore", divide="ignore"):
            ep = perr + np.abs(t) * derr + F.EPS * (scale + _norm(np.nan_to_num(p)))         # error of the hit point
            et = ep / np.abs(d[..., ax])                                                   # ... and of t
            hit = inside & (t >= T_MIN)
            ab = [i for i in range(3) if i != ax]
            edge = np.zeros(t.shape, bool)
            for c, (lo, hi) in zip(ab, (ob["a"], ob["b"])):
                edge |= (np.abs(p[..., c] - lo) < ep) | (np.abs(p[..., c] - hi) < ep)
            near = np.isfinite(t) & (t > T_MIN - et)
            for c, (lo, hi) in zip(ab, (ob["a"], ob["b"])):
                near &= (p[..., c] > lo - ep) & (p[..., c] < hi + ep)
            amb = near & (edge | (np.abs(t - T_MIN) < et))
            # a ray leaving the rect: t = 0 here, |origin - plane| / |d_ax| in fp32; a hit only if that reaches t_min
            hit = hit & ~on_self
            amb = np.where(on_self, self_err > 0.5 * T_MIN * np.abs(d[..., ax]), amb)
        return np.where(np.isfinite(t), t, np.inf), hit, amb
    assert ob["shape"] == "sphere"
    c, r = np.asarray(ob["center"], np.float64), ob["radius"]
    t0, t1, dist = F.sphere_roots(o, d, c, r)
    et = F.sphere_root_error(o, d, c, r) + (perr + derr * np.abs(np.nan_to_num(t1))) / L
    with np.errstate(invalid="ignore"):
        use0 = t0 >= T_MIN                                             # sphere.cpp:29-35: the near root, else the far one
        t = np.where(use0, t0, t1)
        hit = np.isfinite(t) & (t >= T_MIN)
        sil = np.abs(dist - r) < F.EPS * (scale + _norm(c) + r) + perr + derr * np.abs(_dot(c - o, d)) / (L * L)
        amb = (sil & (np.nan_to_num(-_dot(o - c, d)) > 0)) | (np.abs(t0 - T_MIN) < et) | (np.abs(t1 - T_MIN) < et)
    return np.where(hit, t, np.where(sil, -_dot(o - c, d) / (L * L), np.inf)), hit, amb


def hit_record(ob, o, d, t):
    p = o + t[..., None] * d
    if ob["shape"] in _RECT_AXES:
        outward = np.zeros(p.shape)
        outward[..., _RECT_AXES[ob["shape"]]] = 1.0
    else:
        outward = (p - np.asarray(ob["center"], np.float64)) / ob["radius"]
    front, nrm = face_normal(d, outward)
    return dict(p=p, normal=nrm, front_face=front)


# ------------------------------------------------------------------ rayColour (main.cpp:38-79)
def ray_colour(scene, o, d, key, max_depth, env=None, flip=False):
    """Follows n paths for max_depth segments through `scene`: a list of objects dict(shape = xy_rect | xz_rect | yz_rect (a, b:
    the two in-plane ranges, k) | sphere (center, radius) | medium (geom = (min, max) of a box, density; its material is an
    Isotropic of `albedo`), mat = a material of scatter()); a medium must be the scene's only object.  key: seed_lo, seed_hi,
    pixel (n,), sample; the bounce field is the segment index.  env = (EW, EH): the escape texel is looked up in a map of that
    size.  flip = True: every ambiguous decision (a scatter's, hit or miss at a silhouette, an edge or t_min, the free path's)
    takes its other outcome.
    -> dict(escaped (n,) bool, i, j (and ilo, ihi, jlo, jhi, the neighbours inside the band), atten (n, 3): the product of the
    attenuations, atten_err (n,): the absolute fp32 error its components may carry (a UVTest on a sphere; else 0), emitted (n, 3):
    the sum of atten * emitted, ambiguous (n,): the union of the flags met, depth (n,): segments traced, direction (n, 3): of the escaping segment)."""
    o, d = np.array(o, np.float64), np.array(d, np.float64)
    n = o.shape[:-1]
    assert len(n) == 1
    N = n[0]
    atten, result = np.ones((N, 3)), np.zeros((N, 3))
    alive = np.ones(N, bool)
    escaped = np.zeros(N, bool)
    esc_d = np.tile([1.0, 0.0, 0.0], (N, 1))
    esc_derr = np.zeros(N)
    amb = np.zeros(N, bool)
    depth = np.zeros(N, np.int64)
    perr = F.EPS * _norm(o)
    derr = F.EPS * _norm(d)
    last = np.full(N, -1)
    self_err = np.zeros(N)
    atten_err = np.zeros(N)
    for seg in range(max_depth):
        if not alive.any():
            break
        k = dict(key, bounce=seg)
        best_t = np.full(N, np.inf)
        best = np.full(N, -1)
        seg_amb = np.zeros(N, bool)
        ts = []
        for idx, ob in enumerate(scene):
            if ob["shape"] == "medium":
                assert len(scene) == 1, "a medium is pinned alone"
                u = F.u01(F.draw(key["seed_lo"], key["seed_hi"], key["pixel"], key["sample"], seg, F.RNG_MEDIUM, idx)[0])
                with np.errstate(divide="ignore"):
                    t, _, a = F.medium_free_path("box", ob["geom"], np.float64(np.float32(ob["density"])), o, d, T_MIN, np.inf, u)
                hit = np.isfinite(t)
                if flip:
                    hit = hit ^ a
                    t = np.where(hit & ~np.isfinite(t), T_MIN, t)
                t = np.where(hit, t, np.inf)
            else:
                t, hit, a = _hit_object(ob, o, d, perr, derr, last == idx, self_err)
                if flip:
                    hit = hit ^ a
            seg_amb |= a
            ts.append(np.where(hit, t, np.inf))
            closer = hit & (t < best_t)
            best_t = np.where(closer, t, best_t)
            best = np.where(closer, idx, best)
        if len(ts) > 1:            # two surfaces at the same distance: the order is fp32's
            s = np.sort(np.stack(ts, 0), 0)
            with np.errstate(invalid="ignore"):
                seg_amb |= np.isfinite(s[1]) & (s[1] - s[0] < F.EPS * (1.0 + s[0]))
        amb |= alive & seg_amb
        depth += alive
        miss = alive & (best < 0)
        escaped |= miss
        esc_d[miss] = d[miss]
        esc_derr[miss] = derr[miss]
        alive = alive & ~miss
        new_o, new_d = o.copy(), d.copy()
        for idx, ob in enumerate(scene):
            sel = alive & (best == idx)
            if not sel.any():
                continue
            sub = {f: (v[sel] if np.ndim(v) else v) for f, v in k.items()}
            extra = False
            last[sel] = idx
            if ob["shape"] in _RECT_AXES:
                self_err[sel] = SELF_ULPS * 2.0 ** -24 * (np.abs(o[sel][:, _RECT_AXES[ob["shape"]]]) + abs(ob["k"]))
            if ob["shape"] == "medium":  # constantMedium.cpp:29-35: p on the ray, normal (1, 0, 0), frontFace true
                p = o[sel] + best_t[sel, None] * d[sel]
                rec = dict(p=p, normal=np.tile([1.0, 0.0, 0.0], (len(p), 1)), front_face=np.ones(len(p), bool))
                mat = dict(kind=ISOTROPIC, albedo=ob["albedo"])
            else:
                rec = hit_record(ob, o[sel], d[sel], best_t[sel])
                mat = ob["mat"]
                if callable(mat):  # a material whose scalars come from a texture: (rec, flip) -> (material, texel ambiguous)
                    mat, extra = mat(rec, flip)
            s = scatter(mat, rec, d[sel], sub)
            masks, any_ = ambiguous(s["margins"])
            any_ = any_ | extra
            if flip and any(m.any() for m in masks.values()):
                s = scatter(mat, rec, d[sel], sub, flip=masks)
            a = np.zeros(N, bool)
            a[sel] = any_
            amb |= a
            result[sel] += atten[sel] * s["emitted"]
            ok = s["scattered"]
            dead = np.zeros(N, bool)
            dead[sel] = ~ok
            alive = alive & ~dead
            new_o[sel] = rec["p"]
            new_d[sel] = s["sd"]
            pe = perr[sel] + best_t[sel] * derr[sel] + F.EPS * (_norm(o[sel]) + _norm(rec["p"]))
            if ob["shape"] == "sphere":                                # the root's own conditioning, worst near the silhouette
                pe = pe + F.sphere_root_error(o[sel], d[sel], ob["center"], ob["radius"]) * _norm(d[sel])
                if mat["kind"] == UVTEST:                              # attenuation = the normal (p - c) / r: it carries p's error
                    atten_err[sel] += np.abs(atten[sel]).max(-1) * pe / ob["radius"]
            perr[sel] = pe
            atten[sel] = np.where(ok[..., None], atten[sel] * s["attenuation"], atten[sel])
            # the new direction's error: the scatter's own tolerance (per component, hence sqrt 3) plus, where it is built from
            # the incoming direction (reflect; refract magnifies by at most 3 at ior 1.5), that direction's relative error
            smooth = mat["kind"] == METAL and float(np.max(np.abs(mat["roughness"]))) == 0.0
            derr[sel] = (MIRROR_ATOL if smooth else SD_ATOL) * np.sqrt(3.0) + derr[sel] / _norm(d[sel]) * (1.0 + 2.0 * (mat["kind"] == DIELECTRIC))
            if ob["shape"] == "sphere":
                derr[sel] += 2.0 * pe / ob["radius"]                   # the normal (p - c) / r carries p's error
        o, d = new_o, new_d
    out = dict(escaped=escaped, atten=atten, atten_err=atten_err, emitted=result, depth=depth, direction=esc_d)
    if env is not None:
        EW, EH = env
        u, v = F.miss_uv(esc_d)
        du, dv = F.miss_uv_delta(esc_d)
        grow = 1.0 + esc_derr / (_norm(esc_d) * F.EPS)                 # miss_uv_delta assumes F.EPS on the unit direction
        du, dv = du * grow, dv * grow
        i, ilo, ihi, ai = F.band_wrap(lambda x: F.env_index(x, EW), u, du)
        j, jlo, jhi, aj = F.band(lambda x: F.env_index(x, EH), v, dv)
        amb = amb | (escaped & (ai | aj))
        out.update(i=i, j=j, ilo=ilo, ihi=ihi, jlo=jlo, jhi=jhi)
    out["ambiguous"] = amb
    return out
