/* TEST INFRASTRUCTURE ONLY.  extern "C" entry points over the reference's HLSL text compiled for the CPU (oracle/ref_hlsl.py writes
 * the text under oracle/_ref/gen/, oracle/hlsl_cpu.hpp makes it C++).  Nothing here restates a shader: every entry point fills the
 * bindings or the inputs a reference function takes and calls that function (RefPaths: the generated raygen() itself).
 *
 * The file is compiled once per REF_UNIT: the path-tracing shaders and each of the three background kernels have their own `main`
 * and their own bindings, so each gets a translation unit and a namespace of its own.
 *   0 hrtsystem/main.hlsl (and everything it includes)   1 background/equirectangular_to_equal_area.hlsl
 *   2 background/luminance.hlsl                          3 background/fold.hlsl */
#include "hlsl_cpu.hpp"
#include "orc_scene.h"      /* RefPaths reads the oracle's scene tables (the project's own structs) to build the reference's */

#include <atomic>
#include <thread>
#include <vector>

#ifndef REF_UNIT
#define REF_UNIT 0
#endif

extern "C" {
void RefEnvEquirect(const float *src_rgba, uint32_t w, uint32_t h, uint32_t size, float *dst_rgba);
void RefEnvLuminance(const float *rgba, uint32_t size, float *lum);
void RefEnvFold(const float *src, uint32_t src_size, float *dst);
}

#if REF_UNIT == 0
/* ================================================================================================================== */
namespace hlsl {
namespace ref {

/* TraceRay: the search is the caller's (two function pointers in the acceleration structure); what happens to the payload on a
 * hit or a miss is the reference's closesthit / miss / shadowmiss, reached through on_trace() below once they are defined */
template <class Payload>
void TraceRay(const RaytracingAccelerationStructure &accel, uint flags, uint, uint, uint, uint, const RayDesc &ray, Payload &payload) {
    on_trace(accel, flags, ray, payload);
}

/* storeColor's hook (a rule of oracle/ref_hlsl.py puts the call at its top): while a thread captures, the colour raygen hands to storeColor is kept and the
 * image is left alone; otherwise storeColor runs as written */
static thread_local float3 *t_capture = nullptr;
inline bool on_store_color(const float3 &color) { if (!t_capture) return false; *t_capture = color; return true; }

#include "hrtsystem/main.hlsl.h"

inline void on_trace(const RaytracingAccelerationStructure &accel, uint, const RayDesc &ray, Intersection &payload) {
    RayHit hit = {};
    if (accel.closest && accel.closest(accel.user, ray.Origin.d, ray.Direction.d, ray.TMax, &hit)) {
        invocation().hit = hit;
        Attributes attribs; attribs.barycentrics = hit.barycentrics;
        closesthit(payload, attribs);
    } else {
        miss(payload);
    }
}
inline void on_trace(const RaytracingAccelerationStructure &accel, uint, const RayDesc &ray, ShadowIntersection &payload) {
    if (!(accel.any && accel.any(accel.user, ray.Origin.d, ray.Direction.d, ray.TMax))) shadowmiss(payload);
}

struct Env { const float *rgb; const float *const *lum; uint32_t size, levels; };

static float3 f3(const float *p) { return float3(p[0], p[1], p[2]); }
static void put(float *o, const float3 &v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
static void put(float *o, const float2 &v) { o[0] = v.x; o[1] = v.y; }
static void put(float *o, const Frame &f) { put(o, f.n); put(o + 3, f.s); put(o + 6, f.t); }
static Texture2D<float4> texel_texture(const float *rgba) { Texture2D<float4> t; t.mip[0] = rgba; t.w = t.h = 1; t.levels = 1; return t; }
static uint64_t address(const void *p) { return (uint64_t)(uintptr_t)p; }
static float3x4 matrix(const float *p) { float3x4 m; for (int r = 0; r < 3; r++) for (int k = 0; k < 4; k++) m.row[r].d[k] = p[4 * r + k]; return m; }

static EnvMap env_map(const Env *e) {
    Texture2D<float3> rgb; rgb.mip[0] = e->rgb; rgb.w = rgb.h = e->size; rgb.levels = 1; rgb.stride = 4;
    Texture2D<float> lum; lum.w = lum.h = e->size; lum.levels = e->levels;
    for (uint32_t l = 0; l < e->levels && l < 16; l++) lum.mip[l] = e->lum[l];
    SamplerState s; s.address = ADDRESS_MIRRORED_REPEAT;            /* BackgroundManager.zig:80ff */
    return EnvMap::create(rgb, s, lum);
}

/* the probe table of OrcProbeBatch (oracle/orc_core.c) / MsneShadeProbe, without 17 (the bare texture sample would test the shim) */
static const uint32_t PROBE_IN[21]  = { 15, 2, 3, 3, 2, 3, 2, 2, 2, 3, 6, 3, 12, 7, 7, 4, 9, 3, 51, 13, 18 };
static const uint32_t PROBE_OUT[21] = {  8, 7, 4, 3, 3, 2, 2, 2, 3, 1, 3, 6,  1, 3, 3, 1, 6, 4, 23,  9,  6 };

static int probe_one(int fn, const float *a, float *o, const Env *env, uint32_t record) {
    switch (fn) {
        case 0: {   /* MaterialVariant over a host-side material record and constant textures */
            const float color[4] = { a[1], a[2], a[3], 0.0f }, metalness[4] = { a[4], 0, 0, 0 }, roughness[4] = { a[5], 0, 0, 0 };
            Texture2D<float4> textures[3] = { texel_texture(color), texel_texture(metalness), texel_texture(roughness) };
            dTextures = textures;
            dTextureSampler = SamplerState();
            struct { uint color, metalness, roughness; float ior; } pbr = { 0, 1, 2, a[6] };
            struct { uint color; } lambert = { 0 };
            struct { float ior; } glass = { a[6] };
            const MaterialType type = (MaterialType)(uint)a[0];
            const void *rec = type == MaterialType::StandardPBR ? (const void *)&pbr : type == MaterialType::Lambert ? (const void *)&lambert : (const void *)&glass;
            MaterialVariant m = MaterialVariant::load(type, address(rec), float2(0.25f, 0.75f));
            const float3 wi = f3(a + 7), wo = f3(a + 10);
            o[0] = m.pdf(wi, wo);
            put(o + 1, m.eval(wi, wo));
            MaterialSample s = m.sample(wo, float2(a[13], a[14]));
            put(o + 4, s.dirFs); o[7] = s.pdf;
            dTextures = nullptr;
            return 0; }
        case 1: { if (!env) return -1;
            LightSample s = env_map(env).sample(RaytracingAccelerationStructure(), float3(0, 0, 0), float3(0, 0, 1), float2(a[0], a[1]));
            put(o, s.dirWs); put(o + 3, s.radiance); o[6] = s.pdf; return 0; }
        case 2: { if (!env) return -1; LightEval l = env_map(env).eval(f3(a)); put(o, l.radiance); o[3] = l.pdf; return 0; }
        case 3: { if (!env) return -1; put(o, env_map(env).incomingRadiance(f3(a))); return 0; }
        case 4: put(o, squareToEqualAreaSphere(float2(a[0], a[1]))); return 0;
        case 5: put(o, squareToEqualAreaSphereInverse(f3(a))); return 0;
        case 6: put(o, squareToTriangle(float2(a[0], a[1]))); return 0;
        case 7: put(o, squareToGaussian(float2(a[0], a[1]))); return 0;
        case 8: put(o, squareToCosineHemisphere(float2(a[0], a[1]))); return 0;
        case 9: o[0] = Fresnel::dielectric(a[0], a[1], a[2]); return 0;
        case 10: put(o, offsetAlongNormal(f3(a), f3(a + 3))); return 0;
        case 11: { float3 p, q; coordinateSystem(f3(a), p, q); put(o, p); put(o + 3, q); return 0; }
        case 12: o[0] = areaMeasureToSolidAngleMeasure(f3(a), f3(a + 3), f3(a + 6), f3(a + 9)); return 0;
        case 13: { GGX g = GGX::create(a[0]); o[0] = g.D(f3(a + 1)); o[1] = g.Λ(f3(a + 1)); o[2] = g.G(f3(a + 1), f3(a + 4)); return 0; }
        case 14: put(o, refractDir(f3(a), f3(a + 3), a[6])); return 0;
        case 15: o[0] = powerHeuristic((uint)a[0], a[1], (uint)a[2], a[3]); return 0;
        case 16: { Frame f; f.n = f3(a); f.s = f3(a + 3); f.t = float3(0, 0, 0); f.reorthogonalize();
                   put(o, f.worldToFrame(f3(a + 6))); put(o + 3, f.frameToWorld(f3(a + 6))); return 0; }
        case 18: {  /* a real World over host buffers: one instance, one geometry, a mesh whose triangle 1 is the record's (triangle 0 is a
                     * decoy).  Even records use indexed attributes, odd records per-corner ones (attribute 3 * primitive + corner). */
            const uint flags = (uint)a[26];
            const bool indexed = (record & 1u) == 0;
            float positions[9]; std::memcpy(positions, a, sizeof positions);
            const uint indices[6] = { 0, 0, 0, 0, 1, 2 };
            float texcoords[12] = { 9, 9, 9, 9, 9, 9 }, normals[18] = { 9, 9, 9, 9, 9, 9, 9, 9, 9 };
            std::memcpy(texcoords + (indexed ? 0 : 6), a + 9, 6 * sizeof(float));
            std::memcpy(normals + (indexed ? 0 : 9), a + 15, 9 * sizeof(float));
            Mesh mesh = {}; mesh.positionAddress = address(positions); mesh.indexAddress = address(indices);
            mesh.texcoordAddress = (flags & 1u) ? address(texcoords) : 0; mesh.normalAddress = (flags & 2u) ? address(normals) : 0;
            Instance inst = {}; inst.transform = matrix(a + 27); inst.instanceCustomIndexAndMask = 0xFF000000u;
            float3x4 to_mesh = matrix(a + 39);
            Geometry geo = {}; geo.meshIdx = 0; geo.materialIdx = 0; geo.sampled = false;
            World w;
            w.instances.data = &inst; w.instances.count = 1; w.worldToInstance.data = &to_mesh; w.worldToInstance.count = 1;
            w.meshes.data = &mesh; w.meshes.count = 1; w.geometries.data = &geo; w.geometries.count = 1;
            w.indexed_attributes = indexed; w.two_component_normal_texture = true;
            MeshAttributes at = MeshAttributes::lookupAndInterpolate(w, 0, 0, 1, float2(a[24], a[25])).inWorld(w, 0);
            put(o, at.position); put(o + 3, at.texcoord); put(o + 5, at.triangleFrame); put(o + 14, at.frame);
            return 0; }
        case 19: {
            const float texel[4] = { a[0], a[1], a[2], 1.0f };
            Texture2D<float4> textures[1] = { texel_texture(texel) };
            dTextures = textures;
            dTextureSampler = SamplerState();
            MaterialVariantData data = {}; data.normal = 0;
            World w; w.materials.data = &data; w.materials.count = 1; w.indexed_attributes = true; w.two_component_normal_texture = a[12] != 0.0f;
            put(o, getTextureFrame(w, 0, float2(0.5f, 0.5f), Frame::create(f3(a + 3), f3(a + 6), f3(a + 9))));
            dTextures = nullptr;
            return 0; }
        case 20: {
            if (!(a[12] >= 1.0f && a[13] >= 1.0f)) return -1;
            Camera cam; cam.origin = f3(a); cam.forward = f3(a + 3); cam.up = f3(a + 6); cam.vfov = a[9]; cam.aperture = a[10]; cam.focus_distance = a[11];
            RWTexture2D<float4> film; film.w = (uint)a[12]; film.h = (uint)a[13];
            RayDesc r = cam.generateRay(film, float2(a[14], a[15]), float2(a[16], a[17]));
            put(o, r.Origin); put(o + 3, r.Direction); return 0; }
    }
    return -1;
}

}  // namespace ref
}  // namespace hlsl

using namespace hlsl;

extern "C" int RefProbeBatch(int fn, const float *in, uint32_t n, float *out, const ref::Env *env) {
    if (fn < 0 || fn > 20 || fn == 17) return -1;
    for (uint32_t i = 0; i < n; i++)
        if (ref::probe_one(fn, in + (size_t)i * ref::PROBE_IN[fn], out + (size_t)i * ref::PROBE_OUT[fn], env, i) != 0) return -1;
    return 0;
}

/* Rng::fromSeed(uint3(s, x, y)) then n getFloat() (random.hlsl:25-47) */
extern "C" void RefRngFloats(uint32_t s, uint32_t x, uint32_t y, float *out, uint32_t n, uint32_t *state0) {
    ref::Rng rng = ref::Rng::fromSeed(uint3(s, x, y));
    *state0 = rng.state;
    for (uint32_t i = 0; i < n; i++) out[i] = rng.getFloat();
}

/* the three background kernels over their dispatches: equal-area rgb (size x size x 4) and every luminance level */
extern "C" int RefEnvBuild(const float *src_rgba, uint32_t w, uint32_t h, uint32_t size, float *rgb, float *const *lum) {
    if (!src_rgba || w == 0 || h == 0 || size == 0) return -1;
    RefEnvEquirect(src_rgba, w, h, size, rgb);
    RefEnvLuminance(rgb, size, lum[0]);
    for (uint32_t l = 1; (size >> l) >= 1; l++) RefEnvFold(lum[l - 1], size >> (l - 1), lum[l]);
    return 0;
}

/* storeColor (main.hlsl:43-51) for every pixel of one launch: film (h, w, 4) updated in place from the launch's summed colours (h, w, 3) */
extern "C" void RefStoreColor(float *film, uint32_t w, uint32_t h, uint32_t sample_count, uint32_t samples_per_run_, const float *colors) {
    ref::dOutputImage.data = reinterpret_cast<float4 *>(film); ref::dOutputImage.w = w; ref::dOutputImage.h = h;
    ref::pushConsts.sampleCount = sample_count;
    ref::samples_per_run = samples_per_run_;
    invocation().dimensions = uint3(w, h, 1u);
    for (uint32_t y = 0; y < h; y++) for (uint32_t x = 0; x < w; x++) {
        invocation().index = uint3(x, y, 0u);
        ref::storeColor(ref::f3(colors + 3 * ((size_t)y * w + x)));
    }
    ref::dOutputImage.data = nullptr;
}

/* ---- RefPaths ----------------------------------------------------------------------------------------------------- */
typedef int (*OrcClosestFn)(OrcContext *, const float o[3], const float d[3], float tmax, uint32_t ids[3], float tuv[3]);
typedef int (*OrcShadowFn)(OrcContext *, const float o[3], const float d[3], float tmax);

namespace {
struct Tracer { OrcContext *ctx; OrcClosestFn closest; OrcShadowFn shadow; };
thread_local std::vector<uint32_t> *t_hits = nullptr;      /* (instance, geometry, primitive) of every closest hit of the path being traced */

int trace_closest(void *user, const float o[3], const float d[3], float tmax, RayHit *hit) {
    const Tracer *t = static_cast<const Tracer *>(user);
    uint32_t ids[3]; float tuv[3];
    if (!t->closest(t->ctx, o, d, tmax, ids, tuv)) return 0;
    hit->instanceIndex = ids[0]; hit->geometryIndex = ids[1]; hit->primitiveIndex = ids[2]; hit->barycentrics = float2(tuv[1], tuv[2]);
    if (t_hits) { t_hits->push_back(ids[0]); t_hits->push_back(ids[1]); t_hits->push_back(ids[2]); }
    return 1;
}
int trace_any(void *user, const float o[3], const float d[3], float tmax) {
    const Tracer *t = static_cast<const Tracer *>(user);
    return t->shadow(t->ctx, o, d, tmax);
}
}

/* For each job (x, y, sample index k): the reference's own raygen() (main.hlsl:61-95), launched with samples_per_run = 1 and the push constant
 * sampleCount = k, its rays served by the oracle's search through the two function pointers, the colour it hands to storeColor captured.  The driver only
 * fills the bindings, the push constants and the specialization constants: the scene tables are the oracle's (`ctx`, acceleration structure already
 * built), laid out as the reference's host code lays them out.
 * out_rgb: 3 floats per job.  out_hits: `cap` triples (instance, geometry, primitive) per job, out_nhits: how many the path had. */
extern "C" int RefPaths(OrcContext *ctx, OrcClosestFn closest, OrcShadowFn shadow, uint32_t sensor, uint32_t lens, const uint32_t *jobs, uint32_t njobs,
                        float *out_rgb, uint32_t *out_hits, uint32_t *out_nhits, uint32_t cap, int threads) {
    if (!ctx || ctx->accel_dirty || sensor >= ctx->sensor_count || lens >= ctx->lens_count) return -1;
    /* textures, material records, meshes, geometries, instances */
    std::vector<Texture2D<float4> > textures(ctx->texture_count);
    for (uint32_t i = 0; i < ctx->texture_count; i++) { textures[i].mip[0] = ctx->textures[i].rgba; textures[i].w = ctx->textures[i].w; textures[i].h = ctx->textures[i].h; textures[i].levels = 1; }
    struct Record { uint32_t w[4]; };
    std::vector<Record> records(ctx->material_count);
    std::vector<ref::MaterialVariantData> materials(ctx->material_count);
    for (uint32_t i = 0; i < ctx->material_count; i++) {
        const orc_material &m = ctx->materials[i];
        Record &r = records[i]; std::memset(&r, 0, sizeof r);
        if (m.type == (uint32_t)ref::MaterialType::StandardPBR) { r.w[0] = m.color; r.w[1] = m.metalness; r.w[2] = m.roughness; std::memcpy(&r.w[3], &m.ior, 4); }
        else if (m.type == (uint32_t)ref::MaterialType::Lambert) r.w[0] = m.color;
        else if (m.type == (uint32_t)ref::MaterialType::Glass) std::memcpy(&r.w[0], &m.ior, 4);
        materials[i].normal = m.normal; materials[i].emissive = m.emissive; materials[i].type = (ref::MaterialType)m.type; materials[i].materialAddress = ref::address(&r);
    }
    std::vector<ref::Mesh> meshes(ctx->mesh_count);
    for (uint32_t i = 0; i < ctx->mesh_count; i++) {
        const orc_mesh &m = ctx->meshes[i];
        meshes[i].positionAddress = ref::address(m.positions); meshes[i].texcoordAddress = m.texcoords ? ref::address(m.texcoords) : 0;
        meshes[i].normalAddress = m.normals ? ref::address(m.normals) : 0; meshes[i].indexAddress = ref::address(m.indices);
    }
    std::vector<ref::Geometry> geometries(ctx->geometry_count);
    for (uint32_t i = 0; i < ctx->geometry_count; i++) { geometries[i].meshIdx = ctx->geometries[i].mesh; geometries[i].materialIdx = ctx->geometries[i].material; geometries[i].sampled = ctx->geometries[i].sampled != 0; }
    std::vector<ref::Instance> instances(ctx->instance_count);
    std::vector<float3x4> to_instance(ctx->instance_count);
    for (uint32_t i = 0; i < ctx->instance_count; i++) {
        std::memset(static_cast<void *>(&instances[i]), 0, sizeof instances[i]);
        instances[i].transform = ref::matrix(&ctx->instances[i].transform.m[0][0]);
        instances[i].instanceCustomIndexAndMask = (ctx->instances[i].geo_offset & 0x00FFFFFFu) | (ctx->instances[i].visible ? 0xFF000000u : 0u);   /* Accel.zig:394-412 */
        to_instance[i] = ref::matrix(&ctx->instances[i].world_to_instance.m[0][0]);
    }
    static_assert(sizeof(ref::AliasEntry<ref::LightAliasData>) == sizeof(orc_alias_entry), "alias entries are laid out alike");
    const orc_sensor &film = ctx->sensors[sensor];
    Tracer tracer = { ctx, closest, shadow };

    /* the bindings and constants of main.hlsl:10-40 */
    ref::dTextures = textures.data();
    ref::dTextureSampler = SamplerState();                                     /* MaterialManager.zig:428-436: linear, repeat */
    ref::dTLAS.user = &tracer; ref::dTLAS.closest = trace_closest; ref::dTLAS.any = trace_any;
    ref::dInstances.data = instances.data(); ref::dInstances.count = ctx->instance_count;
    ref::dWorldToInstance.data = to_instance.data(); ref::dWorldToInstance.count = ctx->instance_count;
    ref::dEmitterAliasTable.data = reinterpret_cast<const ref::AliasEntry<ref::LightAliasData> *>(ctx->alias); ref::dEmitterAliasTable.count = ctx->alias[0].alias + 1;
    ref::dMeshes.data = meshes.data(); ref::dMeshes.count = ctx->mesh_count;
    ref::dGeometries.data = geometries.data(); ref::dGeometries.count = ctx->geometry_count;
    ref::dMaterials.data = materials.data(); ref::dMaterials.count = ctx->material_count;
    ref::Env env = { ctx->env.rgb, ctx->env.lum, ctx->env.size, ctx->env.mip_count };
    const ref::EnvMap em = ref::env_map(&env);
    ref::dBackgroundRgbTexture = em.rgbTexture; ref::dBackgroundSampler = em.sampler; ref::dBackgroundLuminanceTexture = em.luminanceTexture;
    ref::dOutputImage.data = nullptr; ref::dOutputImage.w = film.w; ref::dOutputImage.h = film.h;
    static_assert(sizeof(ref::Camera) == sizeof(Lens), "Camera is laid out like Lens");
    ref::samples_per_run = 1; ref::max_bounces = ctx->opts.max_bounces; ref::env_samples_per_bounce = ctx->opts.env_samples_per_bounce; ref::mesh_samples_per_bounce = ctx->opts.mesh_samples_per_bounce;
    ref::flip_image = ctx->opts.flip_image != 0; ref::indexed_attributes = ctx->opts.indexed_attributes != 0; ref::two_component_normal_texture = ctx->opts.two_component_normal_texture != 0;

    std::atomic<uint32_t> next(0);
    auto work = [&]() {
        std::vector<uint32_t> hits;
        t_hits = &hits;
        invocation().dimensions = uint3(film.w, film.h, 1u);
        std::memcpy(static_cast<void *>(&ref::pushConsts.camera), &ctx->lenses[lens], sizeof(Lens));      /* push constants are per thread */
        for (;;) {
            const uint32_t j = next.fetch_add(1);
            if (j >= njobs) break;
            const uint32_t x = jobs[3 * j], y = jobs[3 * j + 1], k = jobs[3 * j + 2];
            invocation().index = uint3(x, y, 0u);
            hits.clear();
            ref::pushConsts.sampleCount = k;
            float3 color(0.0f, 0.0f, 0.0f);
            ref::t_capture = &color;
            ref::raygen();
            ref::t_capture = nullptr;
            ref::put(out_rgb + 3 * (size_t)j, color);
            const uint32_t n = (uint32_t)(hits.size() / 3);
            out_nhits[j] = n;
            for (uint32_t h = 0; h < n && h < cap; h++) for (int q = 0; q < 3; q++) out_hits[((size_t)j * cap + h) * 3 + q] = hits[3 * h + q];
        }
        t_hits = nullptr;
    };
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    ref::dTextures = nullptr; ref::dTLAS = RaytracingAccelerationStructure();
    return 0;
}

#else
/* ================================================================================================================== */
/* one background kernel: its bindings are the namespace's globals, its main() runs once per thread of the dispatch */
#if REF_UNIT == 1
#define REF_KERNEL_NS equirect
#elif REF_UNIT == 2
#define REF_KERNEL_NS luminance_kernel
#else
#define REF_KERNEL_NS fold
#endif
namespace hlsl {
namespace REF_KERNEL_NS {
#if REF_UNIT == 1
#include "background/equirectangular_to_equal_area.hlsl.h"
#elif REF_UNIT == 2
#include "background/luminance.hlsl.h"
#else
#include "background/fold.hlsl.h"
#endif
static void dispatch(uint32_t w, uint32_t h) {
    /* whole 8x8 groups, as vkCmdDispatch launches them: the kernels' own bounds checks drop the surplus threads */
    for (uint32_t y = 0; y < (h + 7) / 8 * 8; y++) for (uint32_t x = 0; x < (w + 7) / 8 * 8; x++) main(uint3(x, y, 0u));
}
}
}
using namespace hlsl;
namespace k = hlsl::REF_KERNEL_NS;

#if REF_UNIT == 1
extern "C" void RefEnvEquirect(const float *src_rgba, uint32_t w, uint32_t h, uint32_t size, float *dst_rgba) {
    k::srcTexture.mip[0] = src_rgba; k::srcTexture.w = w; k::srcTexture.h = h; k::srcTexture.levels = 1; k::srcTexture.stride = 4;
    k::srcTextureSampler.address = ADDRESS_MIRRORED_REPEAT;        /* BackgroundManager.zig:80ff: the one sampler of the background */
    k::dstImage.data = reinterpret_cast<float4 *>(dst_rgba); k::dstImage.w = k::dstImage.h = size;
    k::dispatch(size, size);
}
#elif REF_UNIT == 2
extern "C" void RefEnvLuminance(const float *rgba, uint32_t size, float *lum) {
    k::srcColorImage.mip[0] = rgba; k::srcColorImage.w = k::srcColorImage.h = size; k::srcColorImage.levels = 1; k::srcColorImage.stride = 4;
    k::dstLuminanceImage.data = lum; k::dstLuminanceImage.w = k::dstLuminanceImage.h = size;
    k::dispatch(size, size);
}
#else
extern "C" void RefEnvFold(const float *src, uint32_t src_size, float *dst) {
    k::srcMip.mip[0] = src; k::srcMip.w = k::srcMip.h = src_size; k::srcMip.levels = 1;
    k::dstMip.data = dst; k::dstMip.w = k::dstMip.h = src_size / 2;
    k::dispatch(src_size / 2, src_size / 2);
}
#endif
#endif
