/* hrt.h — C ABI of libhrt_hip.so: the MI355X (gfx950) replacement for the
 * reference's per-pixel Monte-Carlo render loop.
 *
 * The reference (Todegal/HobbyRaytracer) has no plugin/FFI interface; its only
 * seam for this path is the free function
 *     static void render(int nThreads, const std::shared_ptr<Texture> background,
 *                        const std::shared_ptr<Hittable> world, const Camera& camera,
 *                        std::shared_ptr<Film>& film)          (main.cpp:81-82)
 * called once from main() (main.cpp:176) on objects produced by the Scene
 * getters (main.cpp:158-162, scene.h:29-33).  Everything that function does
 * between "object graph" and "Film::pixels" is what this library replaces:
 *     rayColour            main.cpp:38-79
 *     render pixel loop    main.cpp:111-135
 *     Hittable::hit tree   hittableList.cpp:4-21, bvh.cpp:69-78, triangle.cpp:57-131,
 *                          sphere.cpp:20-49, aarect.h:12-39/59-86/106-133, box.h:27-55,
 *                          translate.cpp:7-19, scale.cpp:11-27, rotateQuat.cpp:44-66,
 *                          rotateY.cpp:44-75, constantMedium.cpp:4-38
 *     Material::scatter    material.h:79-85,96-104,116-129,137-153,166-177,204-229, material.cpp:18-28
 *     Texture::colourValue texture.cpp:17-28,53-74,76-97
 *     Film::tonemap/writeColour  film.cpp:25-52
 * INTEGRATION.md shows the ~40-line binding a maintainer of the reference adds.
 *
 * Conventions: plain C structs, pointers and sizes only; the library copies
 * what it is given at hrt_scene_create (caller keeps ownership of host arrays);
 * every entry point returns hrt_status (0 = ok) and never throws;
 * hrt_last_error() returns the HIP error text of the calling thread's last
 * failure.  All arithmetic is fp32 except Dielectric's Fresnel term (fp64,
 * material.h:210-218).
 */
#ifndef HRT_H
#define HRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hrt_status {
    HRT_OK = 0,
    HRT_ERR_INVALID = 1,      /* bad argument / inconsistent flat scene */
    HRT_ERR_HIP = 2,          /* a HIP runtime call failed: see hrt_last_error() */
    HRT_ERR_NO_DEVICE = 3,    /* no gfx950 device visible */
    HRT_ERR_OOM = 4,
    HRT_ERR_IO = 5,
    HRT_ERR_PARSE = 6,
    HRT_ERR_UNSUPPORTED = 7
} hrt_status;

/* ---- flattened scene (what Hittable::flatten() emits) ------------------- */

/* Top-level object kinds, in the reference's class vocabulary. */
enum {
    HRT_PRIM_SPHERE = 0,   /* sphere.cpp      p = cx,cy,cz,r                     */
    HRT_PRIM_XY_RECT = 1,  /* aarect.h:106    p = x0,x1,y0,y1,k                  */
    HRT_PRIM_XZ_RECT = 2,  /* aarect.h:59     p = x0,x1,z0,z1,k                  */
    HRT_PRIM_YZ_RECT = 3,  /* aarect.h:12     p = y0,y1,z0,z1,k                  */
    HRT_PRIM_BOX = 4,      /* box.h           p = min.xyz, max.xyz               */
    HRT_PRIM_MESH = 5,     /* mesh.cpp        mesh = index into meshes[]         */
    HRT_PRIM_MEDIUM = 6,   /* constantMedium.cpp  boundary_kind + p, density     */
    HRT_PRIM_TRIANGLE = 7  /* triangle.cpp:4-40  Triangle (NOT the mesh's ITriangle: nothing in the reference
                              constructs one)   p = v0.xyz, v1.xyz, v2.xyz */
};

/* Instance wrappers (translate.cpp, scale.cpp, rotateQuat.cpp, rotateY.cpp).
 * The chain is stored OUTERMOST FIRST, i.e. in the order the ray meets them. */
enum {
    HRT_XF_TRANSLATE = 0,  /* v = offset.xyz                                     */
    HRT_XF_SCALE = 1,      /* v = factor.xyz                                     */
    HRT_XF_ROTATE_QUAT = 2,/* v = quat x,y,z,w                                   */
    HRT_XF_ROTATE_Y = 3    /* v = sinTheta, cosTheta                             */
};
#define HRT_MAX_XFORMS 4

typedef struct hrt_xform {
    int32_t kind;
    float v[4];
} hrt_xform;

typedef struct hrt_prim {
    int32_t kind;
    int32_t material;        /* index into materials[] (MEDIUM: the Isotropic phase function) */
    int32_t mesh;            /* HRT_PRIM_MESH only */
    int32_t boundary_kind;   /* HRT_PRIM_MEDIUM only: HRT_PRIM_SPHERE or HRT_PRIM_BOX */
    float p[9];
    float density;           /* HRT_PRIM_MEDIUM only */
    int32_t n_xforms;
    hrt_xform xf[HRT_MAX_XFORMS];
} hrt_prim;

enum {
    HRT_MAT_LAMBERTIAN = 0,    /* material.h:132-157  albedo                     */
    HRT_MAT_METAL = 1,         /* material.h:159-182  albedo, s0 = roughness     */
    HRT_MAT_DIELECTRIC = 2,    /* material.h:199-242  s0 = ir, s1 = roughness    */
    HRT_MAT_DIFFUSE_LIGHT = 3, /* material.h:91-109   albedo = emit, s0 = strength */
    HRT_MAT_ISOTROPIC = 4,     /* material.h:73-89    albedo                     */
    HRT_MAT_PBR = 5,           /* material.cpp:4-28   albedo, s0 = roughness, mix_tex */
    HRT_MAT_UVTEST = 6         /* material.h:111-130                             */
};

typedef struct hrt_matvec3 {   /* material.h:10-35 MatVec3: constant or texture */
    int32_t tex;               /* < 0 : constant c */
    float c[3];
} hrt_matvec3;

typedef struct hrt_matscalar { /* material.h:37-58 MatScalar: constant or length(texture rgb) */
    int32_t tex;
    float c;
} hrt_matscalar;

typedef struct hrt_material {
    int32_t kind;
    hrt_matvec3 albedo;
    hrt_matscalar s0;
    hrt_matscalar s1;
    int32_t mix_tex;
} hrt_material;

enum {
    HRT_TEX_SOLID = 0,    /* texture.h:18-21   c                                  */
    HRT_TEX_CHECKER = 1,  /* texture.cpp:17-28 even, odd = texture indices        */
    HRT_TEX_IMAGE = 2,    /* texture.cpp:53-74 u8 RGB, texels_u8 + offset         */
    HRT_TEX_ENV = 3       /* texture.cpp:76-97 fp32, `channels` per texel, texels_f32 + offset */
};

typedef struct hrt_texture {
    int32_t kind;
    float c[3];
    int32_t even, odd;
    int32_t width, height, channels;
    int32_t _pad;
    uint64_t offset;      /* element offset into texels_u8 / texels_f32; width==0 => "no data" (cyan) */
} hrt_texture;

/* One triangle mesh = a contiguous range of the triangle arrays plus its
 * flattened BVH (node indices are relative to node_first). */
typedef struct hrt_mesh {
    uint32_t tri_first, tri_count;
    uint32_t node_first, node_count;
} hrt_mesh;

/* 64-byte BVH node holding the boxes of BOTH children, so one fetch tests
 * two boxes (32 B per box, the unit SURVEY.md §8(d) prices a "node visit" at).
 *   child >= 0 : index of an inner node (relative to the mesh's node_first)
 *   child <  0 : leaf, ~child = (first_tri_in_mesh << 3) | (tri_count - 1)
 * An unused child slot has an inverted box (min = +inf, max = -inf). */
typedef struct hrt_bvh_node {
    float c0_min_x, c0_max_x, c0_min_y, c0_max_y;
    float c1_min_x, c1_max_x, c1_min_y, c1_max_y;
    float c0_min_z, c0_max_z, c1_min_z, c1_max_z;
    int32_t child0, child1;
    int32_t _pad0, _pad1;
} hrt_bvh_node;

typedef struct hrt_flat_scene {
    uint32_t n_prims;      const hrt_prim* prims;          /* world list order (hittableList.cpp:12) */
    uint32_t n_materials;  const hrt_material* materials;
    uint32_t n_textures;   const hrt_texture* textures;
    uint32_t n_meshes;     const hrt_mesh* meshes;
    uint64_t n_tris;
    const float* tri_pos;  /* 9 floats per triangle: v0.xyz v1.xyz v2.xyz  (triangle.h:31) */
    const float* tri_nrm;  /* 9 floats per triangle */
    const float* tri_uv;   /* 6 floats per triangle */
    const float* tri_box;  /* 6 floats per triangle (min.xyz, max.xyz): the box of the LOWEST BVHNode that
                              holds the triangle in the reference's own tree (bvh.cpp:20-36,52-60 over the
                              padded ITriangle boxes of triangle.cpp:133-151).  The reference rejects a
                              triangle hit whose leaf-level box fails AABB::hit (bvh.cpp:71), which matters
                              for the t < t_min self-hits of Q-2; the flattened BVH applies the same test to
                              accepted candidates so results do not depend on ITS topology.  NULL = derived by the
                              library from tri_pos and tri_ref_order (hrt_pack.h pack_ref_tree). */
    const uint32_t* tri_ref_order; /* per triangle: (node << 1) | side, where `node` numbers the lowest
                              BVHNodes of the reference's own tree for the mesh in depth-first order and
                              `side` is 0 for that node's `left` child, 1 for `right` (bvh.cpp:20-36).  Once
                              BVHNode::hit has accepted a hit with t < t_min every later BOX test fails
                              (bvh.cpp:71 with t_max = rec.t), so among several such self-hits the reference
                              keeps the one in the FIRST node its walk meets — except that the `right`
                              triangle of that same node is still tested (no box in between, bvh.cpp:75) and
                              wins if it is not farther.  The flattened traversal reproduces exactly that.
                              The codes also DEFINE the reference's whole tree for the library: the reference sorts and
                              splits at start + n / 2 (bvh.cpp:39-43), so a node is a contiguous range of the depth-first
                              order and its box the union of the padded triangle boxes of the range; rays whose
                              ITriangle::hit arithmetic has gone meaningless (quirk Q-4 with a vanishing direction
                              component on the shear axis) are walked through THAT tree, node by node in its order
                              (hrt_device.h ref_walk).  hrt_scene_create refuses codes that are not the depth-first
                              code of such a tree.  NULL = the triangles in the given order (a tree whose sorts
                              changed nothing). */
    uint64_t n_nodes;      const hrt_bvh_node* nodes;
    uint64_t n_texels_u8;  const uint8_t* texels_u8;
    uint64_t n_texels_f32; const float* texels_f32;
    int32_t background_tex;  /* main.cpp:58 background->colourValue(u, v, 0) */
    int32_t _pad;
} hrt_flat_scene;

/* camera.h:41-48 — the constants of Camera::getRay.  The reference hard-wires the lens offset to 0 (camera.h:34:
 * `rd = {0,0,0}; // glm::circularRand(lensRadius)`, "TODO: Add back in randomness"), so lens_u / lens_v / lens_radius are only
 * read with HRT_FLAG_THIN_LENS, which puts that commented-out call back: rd = circularRand(lensRadius) -- a point ON the circle
 * of that radius, as glm defines it --, offset = u * rd.x + v * rd.y (camera.h:35-37). */
typedef struct hrt_camera {
    float origin[3];
    float lower_left[3];
    float horizontal[3];
    float vertical[3];
    float lens_u[3];        /* camera.h:20  u = normalize(cross(up, w)) */
    float lens_v[3];        /* camera.h:21  v = cross(w, u)             */
    float lens_radius;      /* camera.h:26  aperture / 2                */
} hrt_camera;

/* Quirk switches.  A set bit = reference behaviour. */
enum {
    HRT_Q1_ROTQ_NORMALIZE = 1u << 0,  /* rotateQuat.cpp:51 normalises the direction, t units change */
    HRT_Q2_TRI_NO_TMIN = 1u << 1,     /* triangle.cpp:106-109 has no t_min test                    */
    HRT_Q3_TRI_NO_FACE = 1u << 2,     /* triangle.cpp:118-128 never calls setFaceNormal            */
    HRT_Q4_SHEAR_FROM_ORIGIN = 1u << 3/* triangle.cpp:70 picks kZ from the ray ORIGIN              */
};
#define HRT_QUIRKS_REFERENCE 0xFu
#define HRT_QUIRKS_FIXED 0x0u

typedef struct hrt_params {
    int32_t width, height;   /* film_desc.dimensions (film.h:3-7) */
    int32_t samples;         /* film_desc.samples                  */
    int32_t max_depth;       /* MAX_DEPTH = 50 (main.cpp:32)       */
    float t_min;             /* 0.001f (main.cpp:45)               */
    uint32_t quirks;
    uint32_t seed_lo, seed_hi;
    uint32_t flags;          /* HRT_FLAG_* */
} hrt_params;

/* hrt_params.flags */
enum {
    HRT_FLAG_STATS = 1u << 0,  /* also count box_tests / tri_tests / mesh_hits / env_lookups (the counting
                                  build of the kernels; rays and samples are always counted) */
    HRT_FLAG_MEGAKERNEL = 1u << 1, /* render with the single persistent-lanes kernel (k_pathtrace) instead of the
                                  default wavefront pipeline (k_wf_*); results are bit-identical */
    HRT_FLAG_TIMING = 1u << 2, /* wavefront pipeline: also time the traversal kernel's launches with HIP events
                                  (hrt_stats.traversal_ms) */
    HRT_FLAG_THIN_LENS = 1u << 3, /* sample the lens as camera.h:34's commented-out call would (see hrt_camera); off = the reference */
    HRT_FLAG_PROGRESS = 1u << 4, /* keep the host-readable progress counter of hrt_scene_progress / hrt_multi_progress up to date
                                    (the reference's reporter thread, main.cpp:97-109): one tiny launch per round */
    HRT_FLAG_NEE = 1u << 5,     /* next-event estimation (off = the reference's rayColour estimator): at every vertex whose
                                    scatter is Lambertian and whose next segment is traced, one light of the scene's light table (its
                                    unwrapped rects and spheres with a DiffuseLight material) is sampled and a shadow ray traced, and the
                                    result is combined with the BSDF bounce by multiple importance sampling (power heuristic).  The path
                                    itself, and hrt_stats::rays, are those of the default render; the shadow rays are counted in
                                    hrt_stats::shadow_rays.  Wavefront pipeline only: with HRT_FLAG_MEGAKERNEL every render call returns
                                    HRT_ERR_UNSUPPORTED.  A scene without table lights renders as without the flag. */
    HRT_FLAG_NEE_ENV = 1u << 6, /* with HRT_FLAG_NEE (alone: HRT_ERR_INVALID): also importance-sample the environment map.
                                    Every eligible vertex takes one more sample, drawn by luminance x solid angle from a table of the
                                    HRT_TEX_ENV background's texels (built at hrt_scene_create), and traces a second shadow ray that sees
                                    the sky when it hits nothing; an escaping bounce from such a vertex gets the matching MIS weight.
                                    Both shadow rays count in hrt_stats::shadow_rays.  A background without a table (not an environment
                                    map, or one of total weight 0) renders exactly as HRT_FLAG_NEE alone.  Megakernel: HRT_ERR_UNSUPPORTED. */
    HRT_FLAG_NEE_EMITTERS = 1u << 7, /* with HRT_FLAG_NEE (alone: HRT_ERR_INVALID); may be combined with HRT_FLAG_NEE_ENV: sample the emitter
                                    table instead of the light table.  It holds every DiffuseLight rect, box face and mesh
                                    triangle, under any wrapper chain, and the unwrapped spheres (built at hrt_scene_create, see
                                    hrt_emitter_table_build); the light is chosen by an alias table and a planar one sampled uniformly
                                    over its world-space area.  A bounce that hits any entry gets the matching MIS weight; wrapped spheres
                                    and free `triangle` prims (whose hit test does not accept their geometric triangle) still emit with
                                    weight 1.  A scene without entries renders exactly as without the flag.  Shadow rays
                                    count in hrt_stats::shadow_rays.  Megakernel: HRT_ERR_UNSUPPORTED. */
    HRT_FLAG_NEE_LOBES = 1u << 8, /* with HRT_FLAG_NEE (alone: HRT_ERR_INVALID); may be combined with HRT_FLAG_NEE_ENV and HRT_FLAG_NEE_EMITTERS:
                                    the vertices that sample a light are, besides the Lambertian ones, every Metal scatter (a Metal, or a
                                    PBR whose mix chose metal) of roughness >= 1/64 and every Isotropic one (a ConstantMedium hit)
                                    (DESIGN.md 4.8); a bounce from such a vertex gets the matching MIS weight.  Dielectric and UVTest
                                    scatters and smoother metals keep weight 1.  Where the other NEE flags have nothing to sample the flag
                                    changes nothing.  Megakernel: HRT_ERR_UNSUPPORTED. */
    HRT_FLAG_STRATIFIED = 1u << 9, /* the stratified sampler (off = independent Philox words per sample): the samples 0, 1, 2, ...
                                    of a pixel take, at every draw site (pixel, bounce, purpose, aux), the points of an Owen-scrambled,
                                    index-shuffled Sobol' (0,2)-sequence, padded across sites (csrc/hrt_rng.h strat_draw).  It replaces the
                                    draws of the pixel jitter, the lens, the scatter direction and Fresnel coin, and the light and
                                    environment samples of the NEE flags; ConstantMedium free paths and ballRand keep Philox.  The sequence
                                    is indexed by the sample index alone, so the film is the same bits for every tiling, device count,
                                    batch size and adaptive schedule, as without the flag.  Combines with every flag but
                                    HRT_FLAG_MEGAKERNEL (HRT_ERR_UNSUPPORTED).  The estimate stays unbiased; the samples of a pixel are no
                                    longer independent, so hrt_render_adaptive's variance estimate over-states the error of the mean. */
    HRT_FLAG_ROULETTE = 1u << 10,/* Russian roulette (off = every path is followed until it escapes, is absorbed or reaches
                                    max_depth): at every vertex that scatters, from the first_bounce-th scatter of a path on, the path
                                    survives with probability q = max(q_floor, min(1, the largest component of its attenuation)) and a
                                    survivor's attenuation is divided by q (csrc/hrt_roulette.h; the parameters: hrt_scene_set_roulette,
                                    3 and 0.05 by default).  The coin is a draw of its own keyed by (pixel, sample, bounce), so the film is
                                    the same bits for every tiling, device count, batch size and adaptive schedule.  The estimate stays
                                    unbiased; hrt_stats::rays and shadow_rays count what was traced, which is less than without the flag.
                                    Combines with the NEE flags and HRT_FLAG_STRATIFIED; with HRT_FLAG_MEGAKERNEL, and with HRT_FLAG_STATS
                                    (there are no counting variants of its kernels), every render call returns HRT_ERR_UNSUPPORTED. */
    HRT_FLAG_FILTER = 1u << 11   /* the film reconstruction filter of the scene ("reconstruction filter" below; the kind and
                                    the radius: hrt_scene_set_filter, Mitchell at radius 2 by default; off = the reference's box filter, a
                                    pixel is the mean of its own samples): a pixel is the weighted mean of the samples of its neighbourhood.
                                    The paths, hrt_stats and the workspace are those of the render without the flag.  Honoured by
                                    hrt_render_tile, by hrt_render_stripes* and the accumulate forms with n_ranks == 1 and by
                                    hrt_multi_render on a session of one device; HRT_ERR_UNSUPPORTED, output untouched, with n_ranks > 1 or a
                                    session of more devices (neighbouring rows belong to other ranks), from the adaptive entry points (a
                                    list of pixels has no neighbours) and with HRT_FLAG_MEGAKERNEL.  The feature buffers and id mattes
                                    accept the flag and stay box-filtered. */
};

typedef struct hrt_rect { int32_t x0, y0, w, h; } hrt_rect;   /* y0 = row index from the TOP (pIdx / W) */

typedef struct hrt_stats {
    uint64_t rays;       /* path segments = iterations of main.cpp:43-45 */
    uint64_t samples;    /* camera samples                                */
    uint64_t box_tests;  /* BVH child boxes tested (32 B each)            */
    uint64_t tri_tests;  /* triangles tested (36 B each)                  */
    uint64_t mesh_hits;  /* segments whose closest hit is a mesh triangle (60 B attrs) */
    uint64_t env_lookups;/* segments that escaped to an fp32 env map (12 B); HRT_FLAG_NEE_ENV's environment shadow rays read the map
                            too but are not segments: they are counted in shadow_rays only */
    double kernel_ms;    /* path-trace time (megakernel launch, or the whole wavefront pipeline of one render
                            call), summed over `launches`, from HIP events recorded on the launch stream */
    uint64_t launches;   /* render calls (megakernel launches / wavefront pipeline runs) accumulated here */
    double traversal_ms; /* wavefront pipeline with HRT_FLAG_TIMING: time of the BVH traversal kernel (k_wf_ext),
                            summed over its `traversal_launches` launches, from HIP events around each launch */
    uint64_t traversal_launches;
    uint64_t traversal_box_tests, traversal_tri_tests;   /* the part of box_tests / tri_tests counted inside those k_wf_ext
                            launches (HRT_FLAG_STATS): rounds that run inside the task-persistent tail kernel are not in it */
    uint64_t shadow_rays; /* HRT_FLAG_NEE: shadow rays traced (one per eligible vertex with a light sample); not part of `rays` */
} hrt_stats;

typedef struct hrt_hit {          /* hitRecord (hittable.h:8-25) as seen by rayColour */
    float t;
    int32_t prim;                 /* -1 = miss */
    int32_t tri;                  /* triangle index within the mesh, -1 otherwise */
    int32_t front_face;           /* hittable.h:19.  Under quirk Q-3 a mesh hit never writes it (triangle.cpp:118-128): for a mesh
                                     that stands in the world list without a wrapper it is the flag of the previous successful object
                                     of HittableList::hit's walk (hittableList.cpp:6-16), `1` when there was none */
    float p[3];
    float normal[3];
    float u, v;
} hrt_hit;

/* The culling tree of one mesh, built on `device`: a Morton-ordered LBVH (csrc/hrt_lbvh.hip).  Stands where the reference has
 * the BVHNode constructor (bvh.cpp:6-61) -- for the TOPOLOGY only, like the host's binned-SAH builder (host/bvh_build.cpp): the
 * closest hit does not depend on it.  tri_pos: 9 floats per triangle (host memory), finite; max_leaf in 1..8, n_tris > max_leaf.
 * Out (host memory, caller-allocated): nodes_out[n_tris - 1] (hrt_bvh_node, root = 0, child boxes = padded ITriangle boxes
 * (triangle.cpp:133-151) united and widened by the kernels' rounding guard), *n_nodes_out, order_out[n_tris] = the triangle at each
 * position of the leaf order the nodes' leaf codes refer to, *depth_out = inner-node levels (the traversal's stack need). */
hrt_status hrt_bvh_build_device(int device, const float* tri_pos, uint32_t n_tris, uint32_t max_leaf, hrt_bvh_node* nodes_out,
                                uint32_t* n_nodes_out, uint32_t* order_out, int32_t* depth_out);
/* The same interface, THE host builder's tree: host/bvh_build.cpp's binned-SAH algorithm run on the device with the same decisions
 * and arithmetic (csrc/hrt_sahbvh.hip) -- the same topology, up to the order of the triangles inside a leaf.  HRT_ERR_UNSUPPORTED
 * when a large node needs the host's median split (exhausted depth budget): the caller builds that mesh on the host. */
hrt_status hrt_bvh_build_sah(int device, const float* tri_pos, uint32_t n_tris, uint32_t max_leaf, hrt_bvh_node* nodes_out,
                             uint32_t* n_nodes_out, uint32_t* order_out, int32_t* depth_out);

typedef struct hrt_scene hrt_scene;   /* device-resident flattened scene */

hrt_status hrt_device_count(int* n);

/* Uploads (copies) the flat scene to `device`.  Validates every index. */
hrt_status hrt_scene_create(const hrt_flat_scene* flat, int device, hrt_scene** out);
void hrt_scene_destroy(hrt_scene* scene);
/* HRT_FLAG_ROULETTE's parameters for the renders of `scene` that follow: roulette is played from a path's first_bounce-th scatter on
 * (0 and 1: from the first) and no path survives with a probability below q_floor.  A new scene has 3 and 0.05.  HRT_ERR_INVALID for
 * first_bounce < 0 and for a q_floor outside (0, 1] or NaN; the scene then keeps what it had.  Without the flag they are not read. */
hrt_status hrt_scene_set_roulette(hrt_scene* scene, int32_t first_bounce, float q_floor);
/* HRT_FLAG_FILTER's parameters for the renders of `scene` that follow ("reconstruction filter" below): kind = HRT_FILTER_*, radius in
 * pixels, radius <= 0 = the kind's default (tent 1, bspline 2, mitchell 2).  A new scene has HRT_FILTER_MITCHELL at 2.  HRT_ERR_INVALID for
 * an unknown kind, a NaN radius and a radius outside [0.5, 2.5]; the scene then keeps what it had.  Without the flag they are not read. */
hrt_status hrt_scene_set_filter(hrt_scene* scene, int32_t kind, float radius);
/* Reads and clears the time the filter's own kernels took in the render calls on `scene` so far, in ms, from HIP events around their
 * launches (it is part of hrt_stats::kernel_ms too); synchronises the device.  0 when no call had HRT_FLAG_FILTER. */
hrt_status hrt_scene_filter_ms(hrt_scene* scene, double* ms);

/* Blocking: renders tile (x0,y0,w,h) of the W x H film and writes
 * w*h*3 fp32 LINEAR radiance means (row-major within the tile, row 0 = top)
 * to the caller-owned HOST buffer.  This is render() of main.cpp:81-140 up to
 * and including `pixelColour /= samples` (main.cpp:126). */
hrt_status hrt_render_tile(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, hrt_rect tile,
                           float* out_rgb_linear, hrt_stats* stats);

/* Asynchronous multi-GPU form: renders the interleaved row blocks owned by
 * `rank` of `n_ranks` (block b = rows [b*rows_per_block, (b+1)*rows_per_block)
 * belongs to rank b % n_ranks) into a DEVICE buffer of
 * hrt_stripe_rows(height, rows_per_block, rank, n_ranks) * W * 3 floats, rows in
 * increasing absolute row order, on HIP stream `stream` (NULL = default
 * stream).  Counters are accumulated on the device; fetch them with
 * hrt_scene_stats() after synchronising the stream. */
hrt_status hrt_render_stripes_device(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params,
                                     int32_t rows_per_block, int32_t rank, int32_t n_ranks, float* d_out_rgb_linear,
                                     void* stream);
/* Progressive / resumable form (the reference's render() takes all samples of a pixel in one go,
 * main.cpp:118-126).  Adds samples [sample_first, sample_first + sample_count) of params->samples to the
 * accumulation buffer (same layout as hrt_render_stripes_device's output): it holds the running SUM of the samples'
 * radiances, added in sample order.  sample_first == 0 starts a new accumulation (the buffer need not be
 * cleared).  The call whose range reaches params->samples divides the sums by params->samples (main.cpp:126),
 * after which the buffer is bit-identical to a one-shot render with the same params, however the samples
 * were batched.  The buffer plus the next sample index is the whole checkpoint of a render: it can be copied out,
 * stored, and continued later (the row layout depends on rows_per_block / rank / n_ranks only).  Between passes a
 * preview is accum / samples_done.  sample_count < 0 means "all that are left" (params->samples - sample_first); a range
 * outside [0, params->samples) or an empty one is HRT_ERR_INVALID.  Wavefront pipeline only: HRT_FLAG_MEGAKERNEL with a
 * partial range is HRT_ERR_UNSUPPORTED. */
hrt_status hrt_render_stripes_accumulate_device(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params,
                                                int32_t rows_per_block, int32_t rank, int32_t n_ranks, float* d_accum,
                                                int32_t sample_first, int32_t sample_count, void* stream);
/* Blocking host-buffer form: `accum` is uploaded first when sample_first > 0, and downloaded after the pass. */
hrt_status hrt_render_stripes_accumulate(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params,
                                         int32_t rows_per_block, int32_t rank, int32_t n_ranks, float* accum,
                                         int32_t sample_first, int32_t sample_count, hrt_stats* stats);
/* ---- adaptive sampling ---------------------------------------------------
 * Per-pixel sample counts driven by the noise of each pixel's mean luminance, rendered in passes over the row blocks of
 * hrt_render_stripes_device.  Buffers use that stripe layout: d_sums 3 floats (running radiance sums, added in sample
 * order, never divided), d_sq 1 float (running sum of Y*Y with Y = 0.2126f*r + 0.7152f*g + 0.0722f*b of each sample, in
 * sample order, fp32 without contraction) and d_count 1 int32 (samples taken) per pixel.  Every path is keyed by
 * (pixel, sample, bounce) as in the uniform render, so a pixel with count n holds exactly the sums of samples [0, n) of
 * hrt_render_stripes_accumulate_device.
 * Schedule: pass 0 takes samples [0, min_samples) of every pixel; pass k >= 1 adds min(pass_samples, samples - n) to every
 * pixel still active, where n = min(samples, min_samples + (k - 1) * pass_samples) is the count all of them share (a stopped
 * pixel never restarts).
 * Stopping rule, in fp32, with n = count, m = Y(sums) / n, var = max(0, (sq - n*m*m) / (n - 1)): a pixel stops when
 * n >= min_samples && var / n < (threshold * max(m, floor))^2, or when n == samples.  The comparison is strict (threshold 0
 * never stops a pixel early) and a NaN keeps the pixel active until `samples`. */
typedef struct hrt_adaptive {
    int32_t min_samples;   /* pass 0 takes these for every pixel; 2 <= min_samples <= samples */
    int32_t pass_samples;  /* each later pass adds these to every pixel still active; >= 1 */
    float threshold;       /* relative standard error of the mean luminance at which a pixel stops; 0 = never */
    float floor;           /* luminance floor of the relative error's denominator (dark pixels); >= 0 */
} hrt_adaptive;

/* One pass.  pass == 0 starts (the buffers need not be initialised); passes of one render run in order on one stream.  The
 * active pixels are selected and compacted on the device; the call reads back their number (one 4-byte copy, synchronising
 * `stream`) and enqueues the pass's render on `stream`.  *active_out = pixels rendered in this pass (0: the render is
 * finished; nothing was enqueued).  HRT_ERR_INVALID for NULLs, min_samples outside [2, samples], pass_samples < 1, a negative
 * or NaN threshold or floor, pass < 0; HRT_ERR_UNSUPPORTED with HRT_FLAG_MEGAKERNEL.  Samples and segments are counted
 * (hrt_scene_stats: samples = those actually taken); HRT_FLAG_PROGRESS counts per pass. */
hrt_status hrt_render_stripes_adaptive_device(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block,
                                              int32_t rank, int32_t n_ranks, const hrt_adaptive* adaptive, float* d_sums, float* d_sq,
                                              int32_t* d_count, int32_t pass, int64_t* active_out, void* stream);
/* Blocking host-buffer form: the three buffers are uploaded first when pass > 0 and downloaded after a pass that rendered;
 * `stats` (optional) describes this call only. */
hrt_status hrt_render_stripes_adaptive(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block,
                                       int32_t rank, int32_t n_ranks, const hrt_adaptive* adaptive, float* sums, float* sq,
                                       int32_t* count, int32_t pass, int64_t* active_out, hrt_stats* stats);
/* mean = sums / (float)count per pixel (3 floats each), on `stream`: a pixel with count == samples gets exactly the bits of
 * the uniform render (main.cpp:126). */
hrt_status hrt_adaptive_mean_device(hrt_scene* scene, const float* d_sums, const int32_t* d_count, int64_t n_pixels, float* d_mean,
                                    void* stream);
/* Blocking host-buffer form of the above (used by the CLI's one-thread-per-GPU
 * scheduler): same row layout, output copied to the caller-owned HOST buffer. */
hrt_status hrt_render_stripes(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block,
                              int32_t rank, int32_t n_ranks, float* out_rgb_linear, hrt_stats* stats);
int32_t hrt_stripe_rows(int32_t height, int32_t rows_per_block, int32_t rank, int32_t n_ranks);
/* Absolute row index of local row `local` of rank's stripes; -1 if out of range. */
int32_t hrt_stripe_row_index(int32_t height, int32_t rows_per_block, int32_t rank, int32_t n_ranks, int32_t local);

/* ---- feature buffers -------------------------------------
 * What a denoiser or a compositor takes beside the film: first-hit albedo, alpha, normal and depth.  Sample s of pixel (px, py) traces
 * the camera ray of the film's own path -- the same jitter and lens draw, keyed by (seed, pixel, sample), under HRT_FLAG_THIN_LENS,
 * HRT_FLAG_STRATIFIED and params->quirks -- once, to its first hit under that key, so a ConstantMedium is met where the film's path
 * meets it.  Every other flag is accepted and has no effect.  Eight floats per pixel, two groups of four:
 *   albedo r, g, b   hit: the material's albedo at the hit, i.e. what its scatter multiplies the path by, un-clamped (Lambertian, Metal,
 *                    Isotropic, PBR; UVTest: the normal, its attenuation); Dielectric: 1, 1, 1; DiffuseLight: emit x strength, each
 *                    channel clamped to [0, 1], NaN -> 0.            miss: the background's value for the ray, clamped the same way
 *   alpha            hit: 1                                          miss: 0
 *   normal x, y, z   hit: hitRecord::normal as the film's path sees it (not re-normalised, not flipped again); 0, 0, 0 for a
 *                    ConstantMedium.                                 miss: 0, 0, 0
 *   depth            hit: hitRecord::t x length(direction), fp32     miss: 0
 * No specular follow-through: a mirror or a glass reports itself.  A pixel holds the plain mean over its samples, misses included
 * (depth / alpha is the un-premultiplied depth), accumulated as hrt_render_stripes_accumulate_device does it: one thread walks the
 * pixel's samples in ascending order, sum = sum + value in fp32.  The pass counts nothing: hrt_stats and hrt_scene_stats do not see it.
 *
 * Blocking: tile (x0,y0,w,h) of the film, samples [0, params->samples), into the caller-owned HOST buffer of w*h*8 floats (row-major
 * within the tile, row 0 = top).  HRT_ERR_INVALID for a NULL argument and for an empty tile or one outside the film; the buffer is
 * then untouched. */
hrt_status hrt_render_aov_tile(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, hrt_rect tile, float* out);
/* Asynchronous, on HIP stream `stream`: the row blocks of `rank` (hrt_render_stripes_device's layout) into a DEVICE buffer of
 * hrt_stripe_rows(...) * W * 8 floats, 16-byte aligned.  Adds samples [sample_first, sample_first + sample_count) of params->samples to
 * the buffer: it holds the running SUM of the samples' values, added in sample order.  sample_first == 0 starts a new accumulation (the
 * buffer need not be cleared).  The call whose range reaches params->samples divides the sums by params->samples, after which the
 * buffer is bit-identical to a one-shot call with the same params, however the samples were batched.  sample_count < 0 means "all that
 * are left" (params->samples - sample_first); a range outside [0, params->samples) or an empty one is HRT_ERR_INVALID. */
hrt_status hrt_render_aov_stripes_device(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block,
                                         int32_t rank, int32_t n_ranks, float* d_out, int32_t sample_first, int32_t sample_count, void* stream);
/* Blocking host-buffer form: `out` is uploaded first when sample_first > 0, and downloaded after the pass. */
hrt_status hrt_render_aov_stripes(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block, int32_t rank,
                                  int32_t n_ranks, float* out, int32_t sample_first, int32_t sample_count);

/* ---- id mattes and position --------------------------------
 * What a compositor needs to isolate an object or a material: for every pixel, which objects and which materials its samples saw
 * first and what share of the samples each of them took, and where the surface is.  Sample s of pixel (px, py) traces exactly the ray
 * of the feature buffers above -- the film's camera ray under (seed, pixel, s), HRT_FLAG_THIN_LENS, HRT_FLAG_STRATIFIED and
 * params->quirks, to its first hit; every other flag is accepted and has no effect -- and yields
 *   object id     hit: the index of the hit primitive in hrt_flat_scene::prims      miss: -1
 *   material id   hit: the material index of the film's hitRecord there             miss: -1
 *   position      hit: hitRecord::p, fp32                                           miss: 0, 0, 0
 *
 * The matte rule.  A pixel owns, for each of the two id kinds, a table of HRT_AOV_ID_SLOTS (id, count) slots, empty when the call
 * starts.  The samples of the call are visited in ascending order.  A sample whose id is in the table adds 1 to that slot's count.
 * Otherwise it takes the first empty slot, with count 1.  Otherwise -- the table is full -- the sample is dropped: its share of the
 * pixel shows only as 1 - (the sum of the coverages reported).  After the last sample the used slots are ordered by count, largest
 * first, and among equal counts by id, smallest first (ids are signed: the miss id -1 comes before 0).  The first HRT_AOV_ID_RANKS
 * slots of that order are reported as id (int32) and coverage = (float)count / (float)sample_count, one IEEE fp32 division; a rank
 * beyond the used slots is id = INT32_MIN, coverage = +0.
 *
 * Position is the plain fp32 sum of the samples' positions in sample order, starting from +0, each component divided once by
 * (float)sample_count: like the feature buffers it is premultiplied by coverage (misses add 0, 0, 0).
 *
 * 80 bytes per pixel, five groups of 16:
 *   float position x, y, z, 0 | int32 object id of rank 0 .. 3 | float object coverage of rank 0 .. 3 |
 *   int32 material id of rank 0 .. 3 | float material coverage of rank 0 .. 3
 * in the pixel order of hrt_render_aov_*: row-major within the tile, or the rank's row blocks.
 *
 * There is no accumulate form: a bounded table cannot be continued exactly (whether a dropped sample would have been dropped depends
 * on every sample before it), so each call takes its sample range, starts from empty tables and overwrites the buffer, whatever
 * sample_first is.  The pass counts nothing: hrt_stats and hrt_scene_stats do not see it.  Not reported: triangle ids, motion
 * vectors, hashed names.
 *
 * Every entry point returns HRT_ERR_INVALID, with a message, for a NULL argument, an empty tile or one outside the film, a bad
 * partition, an empty sample range or one outside [0, params->samples), and a device pointer that is not 16-byte aligned; the buffer
 * is then untouched. */
#define HRT_AOV_ID_SLOTS 8
#define HRT_AOV_ID_RANKS 4
/* bytes of the buffer of n_pixels pixels (80 each); 0 for n_pixels < 0 */
uint64_t hrt_aov_ids_bytes(int64_t n_pixels);
/* Blocking: tile (x0,y0,w,h) of the film, samples [0, params->samples), into the caller-owned HOST buffer of hrt_aov_ids_bytes(w*h). */
hrt_status hrt_render_aov_ids_tile(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, hrt_rect tile, void* out);
/* Asynchronous, on HIP stream `stream`: samples [sample_first, sample_first + sample_count) of the row blocks of `rank`
 * (hrt_render_stripes_device's layout) into a DEVICE buffer of hrt_aov_ids_bytes(hrt_stripe_rows(...) * W), 16-byte aligned.
 * sample_count < 0 means params->samples - sample_first. */
hrt_status hrt_render_aov_ids_stripes_device(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block,
                                             int32_t rank, int32_t n_ranks, void* d_out, int32_t sample_first, int32_t sample_count, void* stream);
/* Blocking host-buffer form of the above. */
hrt_status hrt_render_aov_ids_stripes(hrt_scene* scene, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block, int32_t rank,
                                      int32_t n_ranks, void* out, int32_t sample_first, int32_t sample_count);

/* ---- guided denoiser --------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with a variance-guided luminance weight (the spatial part of SVGF,
 * Schied et al. 2017) over albedo-demodulated radiance, guided by the feature buffers above.  It needs no scene.  Everything is fp32 and
 * uses only + - * /, sqrtf, fabsf and comparisons, evaluated left to right in the order written here without fused multiply-adds, so
 * that a restatement of these words with IEEE fp32 operations gives the same bits (tests/denoise_np.py).  In this text max(a, b) means
 * (a > b ? a : b) and max(0, x) means (x > 0 ? x : 0): a NaN gives the second operand.
 *
 * Inputs, whole-film images in film order (row 0 = top), W x H pixels:
 *   rgb   3 floats per pixel: the film's linear means c
 *   aov   8 floats per pixel: the buffer of hrt_render_aov_*, A = albedo r, g, b, alpha and B = normal x, y, z, depth
 *   var   optional (NULL: estimated, see below), 1 float per pixel: the variance of the pixel's mean luminance; from the buffers of
 *         hrt_render_stripes_adaptive that is max(0, (sq - n m m) / (n - 1)) / n with m = Y(sums) / n
 * Y(r, g, b) = 0.2126f * r + 0.7152f * g + 0.0722f * b.
 *
 * Prepare, per pixel p:
 *   af_k = a_k > albedo_floor ? a_k : albedo_floor  (a NaN albedo becomes the floor)     valid = all three c_k are finite
 *   e_k = c_k / af_k                 l = Y(e)
 *   d = n.x * n.x + n.y * n.y + n.z * n.z        nh = d > 0 ? n * (1.0f / sqrtf(d)) : (0, 0, 0)
 *   z = alpha > 0 ? depth / alpha : 0
 *   var given:   v = (var > 0 ? var : 0) / (Y(af) * Y(af))
 *   var absent:  over the 7 x 7 window at spacing 1 around p, its in-film valid pixels q in row-major order (p among them):
 *                s1 += l_q, s2 += l_q * l_q, n += 1;  then m = s1 / n and v = max(0, s2 / n - m * m)
 *
 * Iteration j = 0 .. iterations - 1, with s = 1 << j, from the image (e, v) to a second one (ping-pong):
 *   an invalid centre is copied through unchanged.  Otherwise
 *   vbar = (sum of g * v_q) / (sum of g) over the in-film valid q = p + (dx, dy), dy outer and dx inner over -1 .. 1,
 *          g = b[|dx|] * b[|dy|], b = (0.5, 0.25);   sd = sqrtf(vbar)
 *   taps q = p + s * (dx, dy), dy outer and dx inner over -2 .. 2; taps outside the film and invalid taps are skipped:
 *     h = k[|dx|] * k[|dy|], k = (0.375, 0.25, 0.0625)
 *     the centre tap: w = h.   Every other tap: w = h * wn * wz * wl with
 *     wn = 1 when nh_p and nh_q are both zero (all three components == 0), 0 when exactly one is, otherwise
 *          t = max(0, nh_p.x * nh_q.x + nh_p.y * nh_q.y + nh_p.z * nh_q.z), then t = t * t done normal_squarings times
 *     wz = r(fabsf(z_p - z_q) / (sigma_z * max(z_p, z_q) + 1e-6f))
 *     wl = r(fabsf(l_p - l_q) / (sigma_l * sd + 1e-6f)), l = Y(e) of the iteration's input image
 *     r(x) = u * u with u = max(0, 1.0f - x)
 *     sum_k += w * e_q,k     sw += w     sv += (w * w) * v_q
 *   e'_k = sum_k / sw and v' = sv / (sw * sw); sw >= 0.140625 (the centre tap) always.
 *
 * Finish: out_k = valid ? e_k * af_k : c_k.  An invalid pixel keeps its bits and never contributes to another pixel.
 *
 * Temporal accumulation, specular follow-through and an exp-shaped falloff are not part of it. */
typedef struct hrt_denoise_params {
    int32_t iterations;       /* 1 .. 8; default 5: the last iteration's taps reach 2 << (iterations - 1) pixels */
    int32_t normal_squarings; /* 0 .. 10; default 7: the normal weight is the clamped cosine to the power 1 << normal_squarings */
    float sigma_l;            /* finite, > 0; default 2.5: luminance differences up to sigma_l standard deviations get a weight */
    float sigma_z;            /* finite, > 0; default 0.5: relative depth differences up to sigma_z get a weight */
    float albedo_floor;       /* finite, > 0; default 0.01: the smallest albedo the radiance is divided by */
} hrt_denoise_params;
/* Fills in the defaults. */
void hrt_denoise_defaults(hrt_denoise_params* params);
/* The bytes hrt_denoise_device needs as workspace for a W x H film (48 per pixel); 0 when W or H is below 1 or W x H above 2^30. */
uint64_t hrt_denoise_workspace_bytes(int32_t W, int32_t H);
/* Asynchronous, on HIP stream `stream` of `device`: filters the DEVICE image d_rgb into d_out (d_out == d_rgb is allowed; no other
 * overlap is).  d_var may be NULL.  d_aov and d_workspace must be 16-byte aligned.  HRT_ERR_INVALID, with a message, for a NULL
 * argument, W or H below 1, more than 2^30 pixels, a parameter outside its range or NaN, or a misaligned pointer -- decided before any
 * device is touched, and the output is left untouched. */
hrt_status hrt_denoise_device(int device, int32_t W, int32_t H, const hrt_denoise_params* params, const float* d_rgb, const float* d_aov,
                              const float* d_var, float* d_out, void* d_workspace, void* stream);
/* Blocking, HOST buffers (out == rgb is allowed); allocates its own workspace on `device`.  The same refusals. */
hrt_status hrt_denoise(int device, int32_t W, int32_t H, const hrt_denoise_params* params, const float* rgb, const float* aov,
                       const float* var, float* out);
/* hrt_resolve_u8 for a caller that holds no hrt_scene (a filtered film after its scene is gone): the same bytes.  Blocking, host buffers. */
hrt_status hrt_denoise_resolve_u8(int device, const float* rgb_linear, int64_t n_pixels, uint8_t* out_rgb8);

/* ---- measured variance ------------------------------------
 * The `var` input of hrt_denoise, measured instead of guessed: the variance of every pixel's mean luminance, from the batch means of a
 * render taken in passes (hrt_render_stripes_accumulate*, hrt_multi_render: any batching ends in the one-shot film's bits, so the batches
 * cost no sample) or from the buffers of an adaptive render.  It needs no scene.  Everything is fp32 and uses only + - * / and
 * comparisons, evaluated in the order written here without fused multiply-adds, so that a restatement of these words with IEEE fp32
 * operations gives the same bits (tests/variance_np.py).  Y is the luminance of the denoiser's text above, max(0, x) means
 * (x > 0 ? x : 0): a NaN gives 0.  Pixels are independent of each other; the buffers may have any layout (film order, stripes).
 *
 * Fold, after a batch of c = samples_batch samples that follows done = samples_before earlier ones, per pixel:
 *   rgb    3 floats: the accumulation buffer after the batch
 *   scale  1 while the buffer holds undivided sums; (float)samples for the buffer whose last pass has divided by `samples`
 *   state  2 floats: (yprev, M2), the luminance of the sums before this batch and the running sum of squared deviations
 *   y = Y(rgb) * scale
 *   done == 0:  M2 = 0, yprev = y                          (the state need not be initialised)
 *   done  > 0:  mb = (y - yprev) / (float)c                 the mean luminance of this batch
 *               mp = yprev / (float)done                    the mean of everything before it
 *               d = mb - mp
 *               w = ((float)done * (float)c) / (float)(done + c)
 *               M2 = M2 + (d * d) * w, yprev = y            (Chan et al.'s pairwise update: no sq - n m m cancellation)
 * Finish, after `batches` folds that covered `samples` samples:  var = max(0, M2 / (float)(batches - 1)) / (float)samples.
 * With batches of equal size that is the sample variance of the batch means over the number of batches, i.e. an unbiased estimate of
 * the variance of the pixel's mean with batches - 1 degrees of freedom (relative standard deviation sqrt(2 / (batches - 1)) for
 * Gaussian noise); with unequal batches the weights w keep it unbiased.  Under HRT_FLAG_STRATIFIED consecutive sample ranges are not
 * independent and the estimate is too large (conservative).
 * Adaptive, from the buffers of hrt_render_stripes_adaptive*, per pixel:  n = (float)count, m = Y(sums) / n,
 *   var = max(0, (sq - n * m * m) / (n - 1.0f)) / n, and var = 0 where count < 2.
 *
 * HRT_ERR_INVALID, with a message, for a NULL argument, n_pixels < 1 or > 2^30, samples_before < 0, samples_batch < 1, a sum of the two
 * above 2^31 - 1, batches < 2, samples < batches, a scale that is not finite and positive, or a misaligned pointer (state: 8 bytes,
 * everything else: 4) -- decided before any device is touched, and the outputs are left untouched. */
/* The bytes of the state of n_pixels pixels (8 per pixel); 0 when n_pixels is below 1 or above 2^30. */
uint64_t hrt_variance_state_bytes(int64_t n_pixels);
/* Asynchronous, on HIP stream `stream` of `device`, DEVICE buffers: one fold. */
hrt_status hrt_variance_fold_device(int device, int64_t n_pixels, const float* d_rgb, float scale, int32_t samples_before,
                                    int32_t samples_batch, float* d_state, void* stream);
/* Asynchronous: the variance (1 float per pixel) from the state. */
hrt_status hrt_variance_finish_device(int device, int64_t n_pixels, const float* d_state, int32_t samples, int32_t batches, float* d_var,
                                      void* stream);
/* Asynchronous: the variance from the buffers of an adaptive render. */
hrt_status hrt_adaptive_variance_device(int device, int64_t n_pixels, const float* d_sums, const float* d_sq, const int32_t* d_count,
                                        float* d_var, void* stream);
/* Blocking, HOST buffers: `state` is uploaded first when samples_before > 0, and downloaded after the fold.  The same refusals. */
hrt_status hrt_variance_fold(int device, int64_t n_pixels, const float* rgb, float scale, int32_t samples_before, int32_t samples_batch,
                             float* state);
hrt_status hrt_variance_finish(int device, int64_t n_pixels, const float* state, int32_t samples, int32_t batches, float* var);
hrt_status hrt_adaptive_variance(int device, int64_t n_pixels, const float* sums, const float* sq, const int32_t* count, float* var);

/* ---- despeckle --------------------------------------------
 * An energy-preserving outlier filter for the film ahead of the denoiser.  A pixel far brighter than its window (a "firefly") is brought
 * down to a yardstick taken from the window, and what it held above the yardstick is dealt out in equal shares over the window's valid
 * pixels, itself included, so that no energy leaves the film; a pixel with a non-finite channel becomes the mean of its valid
 * neighbours.  It needs no scene.  Everything is fp32 and uses only + - * /, sqrtf and comparisons, evaluated in the order written here
 * without fused multiply-adds, so that a restatement of these words with IEEE fp32 operations gives the same bits
 * (tests/despeckle_np.py).  Y is the luminance of the denoiser's text above; max(0, x) means (x > 0 ? x : 0): a NaN gives 0.
 *
 * Inputs, whole-film images in film order (row 0 = top), W x H pixels:
 *   rgb   3 floats per pixel: the film's linear means c
 *   var   optional (NULL: the gate of step 3 is off), 1 float per pixel: the variance of the pixel's mean luminance, as
 *         hrt_variance_finish or hrt_adaptive_variance give it
 * The window of a pixel p is the (2 * radius + 1) x (2 * radius + 1) square around it; only its pixels inside the film count.
 *
 * 1. Validity and luminance, per pixel:  l = Y(c).  A pixel is valid when c.r, c.g, c.b and l are all finite.
 * 2. Yardstick, per valid pixel p:  of the luminances of the valid pixels of p's window, p itself left out, ref is the rank-th largest
 *    (equal values are separate entries).  With fewer than `rank` such pixels p is not an outlier.
 * 3. Outlier test:  p is an outlier when it is valid and l > 0 and ref >= 0 and l > ratio * ref and, when var is given and gate_z > 0,
 *    gate_z * sqrtf(max(0, var_p)) >= l - ref.  (A single-sample spike of value x among n samples has an excess and a standard
 *    deviation of its mean that are both about x / n and passes the gate; a real highlight has a small variance and is left alone.)
 * 4. Kept part and shares, per outlier:  s = ref / l,  kept_k = c_k * s,  excess_k = c_k - kept_k,  share_k = excess_k / (float)n with
 *    n the number of valid pixels of its window, itself included.  For every other pixel kept = c and share = 0.
 * 5. Output:
 *    a valid p:  out_k = kept_k, then out_k = out_k + share_q,k for every valid q of p's window, p included, in row-major order
 *                (dy outer, dx inner); the zero shares of pixels that are no outliers are added like any other.
 *    an invalid p, with repair_invalid set and at least one valid pixel in its window:  the mean of those pixels' INPUT values,
 *                sum_k = +0.0f, sum_k = sum_k + c_q,k in row-major order, out_k = sum_k / (float)count.
 *    any other invalid p keeps its bits.  An invalid pixel receives no share and is never counted in an n.
 * 6. Map, an optional output of 1 float per pixel:  1.0f - s for an outlier, -1.0f for a repaired pixel, 0 for every other one.
 *
 * Every read is of the input image: one pass, no iteration, and the output must not be the input.  Iteration, a robust estimate over
 * batches and filtering per stripe inside the multi-GPU session are not part of it. */
typedef struct hrt_despeckle_params {
    int32_t radius;         /* 1 or 2; default 1: the window is (2 * radius + 1) squared */
    int32_t rank;           /* 1 .. 4; default 2: the yardstick is the rank-th largest neighbour, so clusters of up to rank - 1 ... */
    float ratio;            /* finite, > 1; default 2: ... pixels more than `ratio` times brighter than it are outliers */
    float gate_z;           /* finite, >= 0; default 2: with a variance, the excess must lie within gate_z standard deviations; 0: no gate */
    int32_t repair_invalid; /* 0 or 1; default 1: a pixel with a non-finite channel becomes the mean of its valid neighbours */
} hrt_despeckle_params;
/* Fills in the defaults. */
void hrt_despeckle_defaults(hrt_despeckle_params* params);
/* The bytes hrt_despeckle_device needs as workspace for a W x H film (20 per pixel); 0 when W or H is below 1 or W x H above 2^30. */
uint64_t hrt_despeckle_workspace_bytes(int32_t W, int32_t H);
/* Asynchronous, on HIP stream `stream` of `device`: filters the DEVICE image d_rgb into d_out; no two buffers may overlap.  d_var and
 * d_map may be NULL.  d_workspace must be 16-byte aligned.  HRT_ERR_INVALID, with a message, for a NULL required argument, W or H
 * below 1, more than 2^30 pixels, a parameter outside its range or NaN, d_out == d_rgb, or a misaligned pointer -- decided before any
 * device is touched, and the outputs are left untouched. */
hrt_status hrt_despeckle_device(int device, int32_t W, int32_t H, const hrt_despeckle_params* params, const float* d_rgb, const float* d_var,
                                float* d_out, float* d_map, void* d_workspace, void* stream);
/* Blocking, HOST buffers; var and map may be NULL; allocates its own workspace on `device`.  The same refusals. */
hrt_status hrt_despeckle(int device, int32_t W, int32_t H, const hrt_despeckle_params* params, const float* rgb, const float* var,
                         float* out, float* map);

/* ---- reconstruction filter --------------------------------
 * HRT_FLAG_FILTER: a pixel of the film is the weighted mean of the samples of its neighbourhood, each weighted by a separable
 * piecewise-polynomial kernel at the sample's distance from the pixel's centre, instead of the plain mean of its own samples (the box
 * filter of main.cpp:118-126).  It is a gather over what a render holds anyway -- every sample's radiance and its jitter, which is a pure
 * function of (seed, pixel, sample) -- so the paths, their weights and hrt_stats are those of the render without the flag.  Everything
 * is fp32 and uses only + - * /, fabsf and comparisons, evaluated in the order written here without fused multiply-adds, so that a
 * restatement of these words with IEEE fp32 operations gives the same bits (tests/filter_np.py).  Only whether a value is a NaN is
 * defined, not a NaN's sign and payload.
 *
 * Inputs: the call's rectangle of the W x H film -- a tile, or the whole film as the stripes of one rank; both are row-major, local
 * pixel lp = ly * rw + lx --, a filter `kind` and a radius R in pixels.
 *
 * Per tap.  For the output pixel p = (px, py), sample s and a neighbour pixel q = (qx, qy) inside the rectangle (p itself is one):
 *   jx = (float)(word x >> 8) * 2^-24, jy likewise from word y, of sample s of pixel q's jitter draw: the RNG_JITTER site at bounce 0
 *        under (seed, pixel = qy * W + qx, sample = s), Philox or, with HRT_FLAG_STRATIFIED, the stratified sampler (csrc/hrt_rng.h
 *        rng_draw / strat_draw, u01): what the sample's camera ray adds to x = qx and to y = H - qy
 *   dx = ((float)(qx - px) + jx) - 0.5f
 *   dy = ((float)(py - qy) + jy) - 0.5f                    (rows count downwards, the camera's y upwards)
 *   tx = fabsf(dx) / R,  ty = fabsf(dy) / R
 *   the tap counts if and only if tx < 1 && ty < 1; a tap that does not count is not added at all (0 * NaN must not poison a pixel)
 *   w = k(tx) * k(ty)
 * The kernels k, for t in [0, 1); the two cubics take x = t + t and end in one division:
 *   HRT_FILTER_TENT      k = 1.0f - t
 *   HRT_FILTER_BSPLINE   x < 1:      a = 3.0f * x - 6.0f;  a = a * x;  a = a * x;  a = a + 4.0f;  k = a / 6.0f
 *                        otherwise:  u = 2.0f - x;  a = (u * u) * u;  k = a / 6.0f
 *   HRT_FILTER_MITCHELL  x < 1:      a = 7.0f * x - 12.0f;  a = a * x;  a = a * x;  a = a + 5.3333335f;  k = a / 6.0f
 *   (Mitchell-Netravali, otherwise:  a = -2.3333333f * x + 12.0f;  a = a * x - 20.0f;  a = a * x + 10.666667f;  k = a / 6.0f
 *    B = C = 1/3)                    (the floats nearest 16/3, -7/3 and 32/3; the outer lobe is negative)
 *
 * Accumulation, per pixel p:  acc_k = acc_k + w * v_k for each channel k, and Wsum = Wsum + w, over the samples in ascending order and,
 * within a sample, over the counting taps with qy ascending, then qx ascending.  v is the sample's value, rad or rad + direct per channel
 * under HRT_FLAG_NEE.  acc starts from +0, or from what the accumulation buffer holds when sample_first > 0.  Which window of neighbours
 * is visited is not part of the definition: any window that holds every counting tap gives the same bits (half-width 0 for R = 0.5,
 * 1 for R <= 1.5, 2 for R <= 2.5).
 *
 * Finishing.  The call whose sample range reaches params->samples finishes each pixel: Wsum over ALL samples [0, samples) in the order
 * above, from +0; out_k = Wsum > 0 ? acc_k / Wsum : 0; then out_k = out_k < 0 ? 0 : out_k (Mitchell's negative lobes can leave a
 * negative sum; a NaN stays a NaN, as in the unfiltered film).  Wsum depends on the jitters only, so the accumulation buffer plus the
 * next sample index remains the whole state of a render, and any split of [0, samples) into consecutive calls gives the bits of the
 * one-shot call.  Before the last call the buffer holds the unnormalised acc.
 *
 * Edges.  Pixels outside the rectangle contribute nothing, at the film's edges and at a tile's: a sub-tile therefore differs from the
 * same pixels of the full film along its border, by definition.
 *
 * Not part of it: filtering across ranks or devices, filtered feature buffers and adaptive passes, Gaussian and
 * Lanczos kernels (expf and sinf are not among the operations pinned here). */
enum {
    HRT_FILTER_TENT = 0,      /* default radius 1 */
    HRT_FILTER_BSPLINE = 1,   /* default radius 2 */
    HRT_FILTER_MITCHELL = 2   /* default radius 2 */
};
/* The filter without a scene, on stored samples: rad = [samples][rect.h][rect.w][3] floats, the value of sample s of every pixel of
 * `rect` of the W x H film (what the film's path under (seed, pixel, s) returned); out = [rect.h][rect.w][3], the finished pixels.  The
 * jitters are those of a render with this seed and, with stratified = 1, HRT_FLAG_STRATIFIED.  radius <= 0 = the kind's default.
 * Blocking, HOST buffers, on `device`; the same kernels as a render under HRT_FLAG_FILTER.  HRT_ERR_INVALID, with a message, for an
 * unknown kind, a NaN radius or one outside [0.5, 2.5], a NULL buffer, W or H below 1 or more than 2^30 pixels, a rectangle that is
 * empty or not inside the film, samples < 1 and stratified other than 0 or 1 -- decided before any device is touched, and the output is
 * left untouched. */
hrt_status hrt_filter_samples(int device, int32_t kind, float radius, int32_t W, int32_t H, hrt_rect rect, uint32_t seed_lo, uint32_t seed_hi,
                              int32_t stratified, int32_t samples, const float* rad, float* out);

/* ---- develop ----------------------------------------------
 * The stage between the clean linear film and the resolve: an energy-conserving pyramid bloom, then an exposure -- none, a manual one
 * in stops, or one metered from the film's own luminance histogram.  It needs no scene and does not touch the tone curve.  Everything
 * is fp32 and uses only + - * / and comparisons, evaluated in the order written here without fused multiply-adds, so that a restatement
 * of these words with IEEE fp32 operations gives the same bits (tests/develop_np.py); the two float64 passages are marked.
 * Y(r, g, b) = 0.2126f * r + 0.7152f * g + 0.0722f * b, left to right.  clamp(v, a, b) = v < a ? a : v > b ? b : v.
 *
 * Input: rgb, the whole film in film order (row 0 = top), W x H pixels, 3 floats per pixel: the linear means c.
 * A pixel is VALID when its three channels are finite.  An invalid pixel keeps its bits through the whole stage and contributes
 * (0, 0, 0) to the pyramid.  Only whether an output is a NaN is defined, not a NaN's sign and payload.
 *
 * Bloom, with bloom_levels and bloom_strength s.  Level 0 is the film, W_0 x H_0 = W x H; level k + 1 is (W_k + 1) / 2 x (H_k + 1) / 2
 * pixels (integer division), and levels exist while max(W_k, H_k) > 1: a 37 x 29 film has 6, a 1 x 1 film none.  L = min(bloom_levels,
 * the levels that exist) is the effective level count.  With L = 0 or s = 0 the bloom is skipped: m = c, bit for bit.  Otherwise:
 * 1. D_0(p) = c_p for a valid p, else (0, 0, 0).
 * 2. Down, k = 0 .. L - 1, per channel:  D_{k+1}(x, y) is a sum that starts from +0.0f and adds the 16 taps in row-major order, j = 0 .. 3
 *    outer, i = 0 .. 3 inner:  sum = sum + D_k(clamp(2x - 1 + i, 0, W_k - 1), clamp(2y - 1 + j, 0, H_k - 1)) * (w_j * w_i)  with
 *    w = (0.125f, 0.375f, 0.375f, 0.125f); the weight products are exact in fp32.
 * 3. Up, from a w x h level C to a finer size, per channel:  cx = x >> 1,  nx = clamp(cx + (x odd ? 1 : -1), 0, w - 1),  cy and ny
 *    likewise from y and h,  U(C)(x, y) = C(cx, cy) * 0.5625f + C(nx, cy) * 0.1875f + C(cx, ny) * 0.1875f + C(nx, ny) * 0.0625f,
 *    left to right.
 * 4. E_L = D_L;  E_k = D_k + U(E_{k+1}) at level k's size, for k = L - 1 .. 1;  B = U(E_1) / (float)L at the film's size.
 * 5. A valid p:  m_k = c_k * (1.0f - s) + B_k * s per channel, with 1.0f - s formed once.  An invalid p:  m = c, its bits.
 * Both filters have weights that sum to 1, so B holds the film's sum, per channel, when everything lit lies at least 3 * 2^L pixels
 * from every border (measured: within 1e-8 relative; the reach is 7 pixels at L = 2 and 19 at L = 3).  At the borders the clamped
 * coordinates leak or gain a little (0.6 % on a 37 x 29 noise film): the stage does NOT preserve the film's sum there.
 *
 * Exposure, with exposure_mode:
 *   0, none:    out = m, bit for bit.
 *   1, manual:  scale = (float)exp2((double)exposure_ev), formed on the host;  out_k = m_k * scale for a valid p.
 *   2, auto:    the film after bloom, m, is metered, and out_k = m_k * scale for a valid p:
 *     A pixel is METERED when it is valid, l = Y(m) is finite and l >= meter_floor.  Its bin is b = bits(l) >> 20, 0 .. 2047: the
 *     exponent and three mantissa bits, 8 bins to the stop, integer arithmetic only (0.18 -> 995, 1.0 -> 1016, 1.5 -> 1020).
 *     n_b is the number of metered pixels of bin b, exact; N is their sum.  With N = 0:  scale = 1, mean_ev = 0.  Otherwise, in
 *     float64, with C_b the number of metered pixels of the bins below b:
 *       lo = (double)meter_low * N,  hi = (double)meter_high * N                      (the window, in pixels of the sorted film)
 *       o_b = max(0, min(C_b + n_b, hi) - max(C_b, lo))                               (what of bin b lies inside the window)
 *       ev_b = (double)((b >> 3) - 127) + c[b & 7],  c[k] = log2(1 + (k + 0.5) / 8):  (the bin's middle, in stops)
 *         c = 0.0874628412503394, 0.2479275134435855, 0.3923174227787603, 0.5235619560570128,
 *             0.6438561897747247, 0.7548875021634686, 0.8579809951275721, 0.9541963103868752
 *       mean_ev = (sum of o_b * ev_b) / (sum of o_b), both over b ascending, then clamped to [ev_min, ev_max]
 *       scale = (float)((double)key * exp2(-mean_ev))
 *     The grouping of the two float64 sums and exp2 itself are not pinned: mean_ev is defined to 1e-9 and scale to one fp32 ulp, and
 *     the film is m * (the scale the call reports), to the bit.
 * An invalid pixel is never scaled.  The histogram is built in mode 2 only; in modes 0 and 1 every n_b and `metered` are 0, mean_ev is 0.
 *
 * Not part of it: a threshold or bright-pass, per-level tints, other tone curves, developing the previews of a
 * progressive render, and the stage per stripe inside the multi-GPU session. */
typedef struct hrt_develop_params {
    int32_t bloom_levels;   /* 0 .. 8; default 0 = no bloom */
    float bloom_strength;   /* [0, 1]; default 0.05: the share of the blurred film in the mix (a convention, not a measurement) */
    int32_t exposure_mode;  /* 0 none, 1 manual, 2 auto; default 0 */
    float exposure_ev;      /* finite, |ev| <= 64; default 0: manual exposure in stops */
    float key;              /* finite, > 0; default 0.18: the luminance the metered level is brought to */
    float meter_low;        /* 0 <= meter_low < meter_high <= 1; defaults 0.10 and 0.90: the window of the sorted metered pixels that ... */
    float meter_high;       /* ... is averaged (the darkest and the brightest tenth are left out) */
    float meter_floor;      /* finite, >= 2^-126; default 2^-16: luminances below it (black, negative) are not metered */
    float ev_min;           /* finite; default -16 ... */
    float ev_max;           /* ... finite, ev_min <= ev_max; default 16: the clamp of the metered level */
} hrt_develop_params;
typedef struct hrt_develop_info {
    double mean_ev;         /* auto: the metered level in stops, after the clamp; otherwise 0 */
    float scale;            /* what every valid pixel was multiplied by (1 in mode 0) */
    uint32_t metered;       /* auto: N, the metered pixels; otherwise 0 */
    uint32_t levels;        /* L, the effective level count (0: the bloom was skipped because there are no levels; s = 0 leaves L as it is) */
    uint32_t pad;
} hrt_develop_info;
#define HRT_DEVELOP_BINS 2048
/* Fills in the defaults, with which the stage is the identity. */
void hrt_develop_defaults(hrt_develop_params* params);
/* The bytes hrt_develop_device needs as workspace for a W x H film with bloom_levels = levels: the HRT_DEVELOP_BINS counters, the info
 * record and the pyramid's levels 1 .. L (16 bytes per pixel of each); 0 when W or H is below 1, W x H above 2^30 or levels outside 0 .. 8. */
uint64_t hrt_develop_workspace_bytes(int32_t W, int32_t H, int32_t levels);
/* Asynchronous, on HIP stream `stream` of `device`: develops the DEVICE image d_rgb into d_out.  d_out == d_rgb is allowed (every launch
 * that writes d_out reads its own pixel of d_rgb only); no other overlap is.  d_info (one hrt_develop_info) and d_hist
 * (HRT_DEVELOP_BINS x uint32_t, the n_b) are optional DEVICE outputs and may be NULL.  d_workspace must be 16-byte aligned; the call clears
 * its counters itself, in stream order, and two calls in flight need two workspaces.  HRT_ERR_INVALID, with a message, for a NULL
 * required argument, W or H below 1, more than 2^30 pixels, a parameter outside its range or NaN, or a misaligned pointer -- decided
 * before any device is touched, and the outputs are left untouched. */
hrt_status hrt_develop_device(int device, int32_t W, int32_t H, const hrt_develop_params* params, const float* d_rgb, float* d_out,
                              hrt_develop_info* d_info, uint32_t* d_hist, void* d_workspace, void* stream);
/* Blocking, HOST buffers; out == rgb is allowed; info and hist may be NULL; allocates its own workspace on `device`.  The same refusals. */
hrt_status hrt_develop(int device, int32_t W, int32_t H, const hrt_develop_params* params, const float* rgb, float* out,
                       hrt_develop_info* info, uint32_t* hist);

/* ---- multi-GPU session -----------------------------------
 * The reference's render() (main.cpp:81-140) has one parallel loop over all pixels of the film (main.cpp:111-135, no state
 * shared between pixels).  Here the flattened scene is replicated on `n_devices` GPUs of THIS process (`devices` = their
 * indices, NULL = 0..n-1), the film rows are dealt to them in interleaved blocks (hrt_stripe_rows) and every device keeps
 * the running sums of its rows in its own memory.  With more than one device (or force_rccl != 0) the session owns an RCCL
 * communicator per device (ncclCommInitAll) and hrt_multi_render gathers the device-resident stripes on the first device
 * with one grouped ncclAllGather of equal, padded shares over xGMI; nothing but the finished film crosses PCIe.
 * force_rccl < 0 is LOOPBACK, a test mode for boxes with fewer devices than ranks: a device may be listed once per logical
 * rank and the gather is one device-to-device copy per rank on that rank's stream instead of ncclAllGather (RCCL refuses two
 * ranks on one device); one host thread, stream and scene per rank, the padded shares, idle ranks and the film assembly are
 * the production code.
 * If a rank fails inside hrt_multi_render the others have already added the sample range to their sums: the session then
 * refuses to continue until it is given resume_sums (a checkpoint) or started again at sample 0. */
typedef struct hrt_multi hrt_multi;
hrt_status hrt_multi_create(const hrt_flat_scene* flat, int32_t n_devices, const int32_t* devices, int32_t force_rccl, hrt_multi** out);
void hrt_multi_destroy(hrt_multi* m);
int32_t hrt_multi_devices(const hrt_multi* m);
int32_t hrt_multi_uses_rccl(const hrt_multi* m);
/* hrt_scene_set_roulette for every device of the session. */
hrt_status hrt_multi_set_roulette(hrt_multi* m, int32_t first_bounce, float q_floor);
/* hrt_scene_set_filter for every device of the session. */
hrt_status hrt_multi_set_filter(hrt_multi* m, int32_t kind, float radius);
/* hrt_scene_filter_ms of the session (the slowest device's). */
hrt_status hrt_multi_filter_ms(hrt_multi* m, double* ms);
/* Adds samples [sample_first, sample_first + sample_count) of params->samples on all devices at once (sample_count < 0: all that
 * are left; 0: none, only gather what is there), gathers, and hands out (both optional, caller-owned HOST buffers):
 *   out_sums  W*H*3 floats in film order: the running sums -- the means once the range has reached params->samples
 *             (main.cpp:126); this plus the next sample index is the checkpoint of the render;
 *   out_u8    W*H*3 bytes: Film::tonemap + writeColour (film.cpp:25-52) of sums / samples_done, resolved on the first device.
 * resume_sums != NULL (W*H*3 floats, film order): the devices' sums are set from it first (continuing from a checkpoint,
 * with any device count).  Blocking.  `stats`: summed over the devices; the two times are the slowest device's. */
hrt_status hrt_multi_render(hrt_multi* m, const hrt_camera* cam, const hrt_params* params, int32_t rows_per_block, int32_t sample_first,
                            int32_t sample_count, const float* resume_sums, float* out_sums, uint8_t* out_u8, hrt_stats* stats);

/* The reference's progress counter (main.cpp:95-109: `pixelsCompleted`, printed every 500 ms by a reporter thread) for a path
 * that finishes its pixels together: *paths_done = camera paths (pixel samples) finished so far in the render call that is
 * running -- or ran last -- on `scene` with HRT_FLAG_PROGRESS, *paths_total = all paths of that call.  The counter lives in
 * host-mapped memory the device writes after every round: these calls read it without any HIP call or lock, from any thread,
 * while the render runs.  hrt_multi_progress sums the session's ranks.  (pixels = width * height * done / total.) */
hrt_status hrt_scene_progress(const hrt_scene* scene, uint64_t* paths_done, uint64_t* paths_total);
hrt_status hrt_multi_progress(const hrt_multi* m, uint64_t* paths_done, uint64_t* paths_total);

/* Reads and clears the device-side counters of `scene` (synchronises its device). */
hrt_status hrt_scene_stats(hrt_scene* scene, hrt_stats* stats);

/* Film::tonemap + Film::writeColour (film.cpp:25-52) on the GPU.
 * Host-buffer form and device-buffer form. */
hrt_status hrt_resolve_u8(hrt_scene* scene, const float* rgb_linear, int64_t n_pixels, uint8_t* out_rgb8);
hrt_status hrt_resolve_u8_device(hrt_scene* scene, const float* d_rgb_linear, int64_t n_pixels, uint8_t* d_out_rgb8,
                                 void* stream);

/* Test entry: world->hit(r, t_min, t_max, rec) of
 * main.cpp:45 for n rays given as host arrays o[3n], d[3n].  `pixel0` keys the
 * RNG used by ConstantMedium::hit: ray i draws as (pixel0 + i, sample 0, bounce 0). */
hrt_status hrt_closest_hit(hrt_scene* scene, const hrt_params* params, int64_t n, const float* o, const float* d,
                           float t_min, float t_max, uint32_t pixel0, hrt_hit* out);

/* Test entry: evaluates the shared math kernels on the GPU so that tests can
 * check CPU == GPU bit for bit.  op: 0 sin, 1 cos, 2 acos, 3 atan2(x=in, y=in2), 4 log,
 * 5 philox (in = counter words as float bits; out 4 words per input). */
hrt_status hrt_math_probe(int device, int32_t op, int64_t n, const float* in, const float* in2, float* out);

/* Test entry: HRT_FLAG_STRATIFIED's draw (csrc/hrt_rng.h strat_draw) on the GPU for n keys; seed = hrt_params' seed_lo | seed_hi << 32,
 * keys[4 i ..] = pixel, sample, bounce, purpose | aux << 8; out[4 i ..] = the draw's words x, y, z, w. */
hrt_status hrt_sampler_probe(int device, uint64_t seed, int64_t n, const uint32_t* keys, uint32_t* out);

/* HRT_FLAG_NEE_ENV's sampling table of an environment map, built by the same kernels hrt_scene_create runs, on the current
 * device, from host memory: texels = W x H x channels fp32 (channels >= 3; rows from the top, as the HRT_TEX_ENV texture stores them).
 * marginal_out gets H + 1 floats (the CDF over rows), conditional_out H x (W + 1) floats (each row's CDF over its columns).  Every CDF
 * starts at exactly 0, ends at exactly 1 and is monotone; a row of weight 0 is all 0 but its last entry.  When the map has no table
 * (total weight 0 or not finite) every entry of both outputs is 0, so marginal_out[H] == 0 says "no table". */
hrt_status hrt_env_table_build(const float* texels, int32_t W, int32_t H, int32_t channels, float* marginal_out, float* conditional_out);

/* HRT_FLAG_NEE_EMITTERS' emitter table of a flattened scene (csrc/hrt_emitters.h), exactly as hrt_scene_create builds it;
 * host only, no device needed.  Size query: every output NULL, *n_entries gets the number of entries (0: the scene has no table).  Fill:
 * *n_entries = that number, and records_out gets 16 floats per entry (4 float4: prim bits, kind bits, P_sel, sub bits / origin or centre,
 * area or radius / edge 1, wrapped / edge 2), shade_out 4 per entry (unit normal, P_sel / area; sphere: centre, -radius), thresh_out and
 * alias_out one per alias slot, base_out one per prim (its first entry, -1: none).  P_sel is the probability the fp32 alias table
 * realises. */
hrt_status hrt_emitter_table_build(const hrt_flat_scene* flat, int64_t* n_entries, float* records_out, float* shade_out, float* thresh_out,
                                   int32_t* alias_out, int32_t* base_out);

/* Debug entry: a library built with -DHRT_DEBUG_BOUNDS checks every table index a hit record is built from (triangle of a mesh,
 * prim, material, texture, mesh, frontFace source) against its table, counts the violations per kind and carries on with index 0
 * instead of faulting.  Reads and clears the 8 counters of `device`; HRT_ERR_UNSUPPORTED from a normal build
 * (tests/tools/debug_bounds.sh runs the GPU suite on such a build). */
hrt_status hrt_debug_bounds_violations(int32_t device, int64_t* out8);

const char* hrt_status_str(hrt_status s);
const char* hrt_last_error(void);
const char* hrt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HRT_H */
