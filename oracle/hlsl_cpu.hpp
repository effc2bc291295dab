/* TEST INFRASTRUCTURE ONLY.  A C++17 compatibility header under which the reference's HLSL text (rewritten at the syntax level by
 * oracle/ref_hlsl.py, never committed) compiles and runs on the CPU: vector and matrix types with lvalue swizzles, the intrinsics
 * the shaders call, and host-memory stand-ins for the resource types.  Everything lives in namespace hlsl; the generated files are
 * included inside a namespace nested in it (oracle/ref_hlsl_driver.cpp), so an unqualified sqrt / pow / max in shader text finds
 * the functions below and not libm's double versions.
 *
 * Arithmetic follows the operand types the way HLSL does with one exception that is the point of the second build: a `double`
 * operand (an unsuffixed literal when the text is compiled WITHOUT -fsingle-precision-constant) keeps scalar expressions and scalar
 * intrinsics in double.  Vectors are always float/int/uint/bool.
 *
 * The one thing this header implements itself rather than takes from the reference is Texture2D::SampleLevel: Vulkan's linear
 * filter at level 0 with unnormalised-to-texel coordinate u * size - 1/2, weights frac(), and the address mode of the sampler
 * that is passed: repeat for material textures (MaterialManager.zig:428-436), mirrored repeat for the background
 * (BackgroundManager.zig:80ff).  A 1x1 texture returns its texel.  Reads outside an image return zero. */
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include "orc_math.h"
#undef INFINITY

namespace hlsl {

typedef uint32_t uint;
template <class T, int N> struct vec;

/* scalar promotion: double if any operand is double, float otherwise (ints promote to float in the intrinsics) */
template <class... A> struct promote { typedef typename std::conditional<(std::is_same<A, double>::value || ...), double, float>::type type; };
template <class T> using if_arith = typename std::enable_if<std::is_arithmetic<T>::value, int>::type;

/* ---- swizzles: a view of components I... of an N-vector, sharing its storage.  V is the vector type the view converts to; it is a
 * template TYPE argument so that argument-dependent lookup finds V's friend functions for a bare swizzle argument ---- */
template <class V, class T, int N, int... I> struct swz {
    T d[N];
    operator V() const { return V(d[I]...); }
    swz &operator=(const V &v) { int k = 0; ((d[I] = v.d[k++]), ...); return *this; }
};

/* ---- operators and intrinsics shared by all vector widths, as hidden friends (non-template functions: implicit conversions of
 * scalars, swizzles and other vector types apply to their arguments) ---- */
template <class T, int N> struct vec_ops {
    typedef vec<T, N> V;
    typedef vec<bool, N> B;
#define HLSL_BIN(op) \
    friend V operator op(const V &a, const V &b) { V r; for (int i = 0; i < N; i++) r.d[i] = (T)(a.d[i] op b.d[i]); return r; } \
    friend V &operator op##=(V &a, const V &b) { for (int i = 0; i < N; i++) a.d[i] = (T)(a.d[i] op b.d[i]); return a; }
    HLSL_BIN(+) HLSL_BIN(-) HLSL_BIN(*) HLSL_BIN(/)
#undef HLSL_BIN
#define HLSL_CMP(op) friend B operator op(const V &a, const V &b) { B r; for (int i = 0; i < N; i++) r.d[i] = a.d[i] op b.d[i]; return r; }
    HLSL_CMP(<) HLSL_CMP(>) HLSL_CMP(<=) HLSL_CMP(>=) HLSL_CMP(==) HLSL_CMP(!=)
#undef HLSL_CMP
    friend V operator-(const V &a) { V r; for (int i = 0; i < N; i++) r.d[i] = (T)(-a.d[i]); return r; }
    friend V operator+(const V &a) { return a; }
    friend V abs(const V &a) { V r; for (int i = 0; i < N; i++) r.d[i] = a.d[i] < T(0) ? (T)(-a.d[i]) : a.d[i]; return r; }
    friend V sign(const V &a) { V r; for (int i = 0; i < N; i++) r.d[i] = (T)((a.d[i] > T(0)) - (a.d[i] < T(0))); return r; }
    friend V min(const V &a, const V &b) { V r; for (int i = 0; i < N; i++) r.d[i] = b.d[i] < a.d[i] ? b.d[i] : a.d[i]; return r; }
    friend V max(const V &a, const V &b) { V r; for (int i = 0; i < N; i++) r.d[i] = a.d[i] < b.d[i] ? b.d[i] : a.d[i]; return r; }
    friend V clamp(const V &x, const V &lo, const V &hi) { return min(max(x, lo), hi); }
    friend V select(const B &c, const V &a, const V &b) { V r; for (int i = 0; i < N; i++) r.d[i] = c.d[i] ? a.d[i] : b.d[i]; return r; }
    friend T dot(const V &a, const V &b) { T s = a.d[0] * b.d[0]; for (int i = 1; i < N; i++) s = s + a.d[i] * b.d[i]; return s; }
    friend T length(const V &a) { return std::sqrt(dot(a, a)); }
    friend T distance(const V &a, const V &b) { return length(a - b); }
    friend V normalize(const V &a) { return a * V(T(1) / length(a)); }
    friend V sqrt(const V &a) { V r; for (int i = 0; i < N; i++) r.d[i] = std::sqrt(a.d[i]); return r; }
    friend V lerp(const V &a, const V &b, const V &t) { return a * (V(T(1)) - t) + b * t; }
    friend V saturate(const V &a) { return clamp(a, V(T(0)), V(T(1))); }
    friend V reflect(const V &i, const V &n) { return i - V(T(2) * dot(n, i)) * n; }
    friend bool all(const V &a) { for (int i = 0; i < N; i++) if (!a.d[i]) return false; return true; }
    friend bool any(const V &a) { for (int i = 0; i < N; i++) if (a.d[i]) return true; return false; }
    friend vec<int, N> asint(const V &a) { static_assert(sizeof(T) == 4, "32-bit components"); vec<int, N> r; std::memcpy(r.d, a.d, sizeof r.d); return r; }
    friend vec<float, N> asfloat(const V &a) { static_assert(sizeof(T) == 4, "32-bit components"); vec<float, N> r; std::memcpy(r.d, a.d, sizeof r.d); return r; }
};

#define HLSL_VEC_COMMON(N) \
    vec() {} \
    template <class S, if_arith<S> = 0> vec(S s) { for (int i = 0; i < N; i++) d[i] = (T)s; } \
    template <class U> vec(const vec<U, N> &o) { for (int i = 0; i < N; i++) d[i] = (T)o.d[i]; } \
    template <class U, int M, int... I> vec(const swz<vec<U, N>, U, M, I...> &s) { const vec<U, N> o = s; for (int i = 0; i < N; i++) d[i] = (T)o.d[i]; } \
    T &operator[](int i) { return d[i]; } \
    const T &operator[](int i) const { return d[i]; }

template <class T> struct vec<T, 2> : vec_ops<T, 2> {
    union {
        T d[2];
        struct { T x, y; };
        struct { T r, g; };
        swz<vec<T, 2>, T, 2, 0, 1> xy, rg;
        swz<vec<T, 2>, T, 2, 1, 0> yx;
    };
    HLSL_VEC_COMMON(2)
    template <class A, class B, if_arith<A> = 0, if_arith<B> = 0> vec(A a, B b) { d[0] = (T)a; d[1] = (T)b; }
};
template <class T> struct vec<T, 3> : vec_ops<T, 3> {
    union {
        T d[3];
        struct { T x, y, z; };
        struct { T r, g, b; };
        swz<vec<T, 2>, T, 3, 0, 1> xy, rg;
        swz<vec<T, 3>, T, 3, 0, 1, 2> xyz, rgb;
    };
    HLSL_VEC_COMMON(3)
    template <class A, class B, class C, if_arith<A> = 0, if_arith<B> = 0, if_arith<C> = 0> vec(A a, B b, C c) { d[0] = (T)a; d[1] = (T)b; d[2] = (T)c; }
    template <class U, class C, if_arith<C> = 0> vec(const vec<U, 2> &a, C c) { d[0] = (T)a.d[0]; d[1] = (T)a.d[1]; d[2] = (T)c; }
};
template <class T> struct vec<T, 4> : vec_ops<T, 4> {
    union {
        T d[4];
        struct { T x, y, z, w; };
        struct { T r, g, b, a; };
        swz<vec<T, 2>, T, 4, 0, 1> xy, rg;
        swz<vec<T, 3>, T, 4, 0, 1, 2> xyz, rgb;
    };
    HLSL_VEC_COMMON(4)
    template <class A, class B, class C, class D, if_arith<A> = 0, if_arith<B> = 0, if_arith<C> = 0, if_arith<D> = 0> vec(A a_, B b_, C c, D e) { d[0] = (T)a_; d[1] = (T)b_; d[2] = (T)c; d[3] = (T)e; }
    template <class U, class D, if_arith<D> = 0> vec(const vec<U, 3> &v, D e) { d[0] = (T)v.d[0]; d[1] = (T)v.d[1]; d[2] = (T)v.d[2]; d[3] = (T)e; }
};
#undef HLSL_VEC_COMMON

typedef vec<float, 2> float2; typedef vec<float, 3> float3; typedef vec<float, 4> float4;
typedef vec<int, 2> int2;     typedef vec<int, 3> int3;     typedef vec<int, 4> int4;
typedef vec<uint, 2> uint2;   typedef vec<uint, 3> uint3;   typedef vec<uint, 4> uint4;
typedef vec<bool, 2> bool2;   typedef vec<bool, 3> bool3;   typedef vec<bool, 4> bool4;
static_assert(sizeof(float2) == 8 && sizeof(float3) == 12 && sizeof(float4) == 16 && sizeof(uint3) == 12, "vectors are packed like HLSL's in buffers");

inline float3 cross(const float3 &a, const float3 &b) { return float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

/* ---- scalar intrinsics ---- */
/* sin, cos, tan, acos, log and atan2 of float operands are the project's own deterministic functions (oracle/orc_math.h, pinned by
 * tests/golden/math.npz); HLSL leaves their rounding to the driver, and with the same ones on both sides a difference between
 * this build and the oracle is a difference of TEXT.  The same holds for normalize (x * (1 / length)) and lerp (x (1 - s) + y s). */
inline float sin(float a) { return det_sinf(a); }     inline double sin(double a) { return std::sin(a); }
inline float cos(float a) { return det_cosf(a); }     inline double cos(double a) { return std::cos(a); }
inline float tan(float a) { return det_tanf(a); }     inline double tan(double a) { return std::tan(a); }
inline float acos(float a) { return det_acosf(a); }   inline double acos(double a) { return std::acos(a); }
inline float log(float a) { return det_logf(a); }     inline double log(double a) { return std::log(a); }
inline float atan2(float a, float b) { return det_atan2f(a, b); }
inline double atan2(double a, double b) { return std::atan2(a, b); }
inline double atan2(double a, float b) { return std::atan2(a, (double)b); }
inline double atan2(float a, double b) { return std::atan2((double)a, b); }
#define HLSL_F1(name, fn) template <class A, if_arith<A> = 0> inline typename promote<A>::type name(A a) { typedef typename promote<A>::type P; return std::fn((P)a); }
HLSL_F1(sqrt, sqrt) HLSL_F1(log2, log2) HLSL_F1(floor, floor)
#undef HLSL_F1
template <class A, if_arith<A> = 0> inline A abs(A a) { return a < A(0) ? (A)(-a) : a; }
template <class A, if_arith<A> = 0> inline A sign(A a) { return (A)((a > A(0)) - (a < A(0))); }
template <class A, if_arith<A> = 0> inline bool isinf(A a) { return std::isinf((typename promote<A>::type)a); }
template <class A, if_arith<A> = 0> inline typename promote<A>::type frac(A a) { typedef typename promote<A>::type P; return (P)a - std::floor((P)a); }
template <class A, if_arith<A> = 0> inline typename promote<A>::type saturate(A a) { typedef typename promote<A>::type P; return (P)a < P(0) ? P(0) : ((P)a > P(1) ? P(1) : (P)a); }
template <class A, class B, if_arith<A> = 0, if_arith<B> = 0> inline typename promote<A, B>::type pow(A a, B b) { typedef typename promote<A, B>::type P; return std::pow((P)a, (P)b); }
/* min / max keep an all-integer call integer; otherwise they promote like the rest */
template <class A, class B> struct minmax_t { typedef typename std::conditional<std::is_integral<A>::value && std::is_integral<B>::value, typename std::common_type<A, B>::type, typename promote<A, B>::type>::type type; };
template <class A, class B, if_arith<A> = 0, if_arith<B> = 0> inline typename minmax_t<A, B>::type min(A a, B b) { typedef typename minmax_t<A, B>::type P; return (P)b < (P)a ? (P)b : (P)a; }
template <class A, class B, if_arith<A> = 0, if_arith<B> = 0> inline typename minmax_t<A, B>::type max(A a, B b) { typedef typename minmax_t<A, B>::type P; return (P)a < (P)b ? (P)b : (P)a; }
template <class A, class B, class C, if_arith<A> = 0, if_arith<B> = 0, if_arith<C> = 0> inline typename promote<A, B, C>::type clamp(A x, B lo, C hi) { typedef typename promote<A, B, C>::type P; return min(max((P)x, (P)lo), (P)hi); }
template <class A, class B, class C, if_arith<A> = 0, if_arith<B> = 0, if_arith<C> = 0> inline typename promote<A, B, C>::type lerp(A a, B b, C t) { typedef typename promote<A, B, C>::type P; return (P)a * (P(1) - (P)t) + (P)b * (P)t; }
inline int asint(float a) { int r; std::memcpy(&r, &a, 4); return r; }
inline float asfloat(int a) { float r; std::memcpy(&r, &a, 4); return r; }
inline float asfloat(uint a) { float r; std::memcpy(&r, &a, 4); return r; }

/* ---- matrices: R rows of C-vectors, row-major in memory ---- */
template <int R, int C> struct mat {
    vec<float, C> row[R];
    mat() {}
    mat(const vec<float, C> &a, const vec<float, C> &b, const vec<float, C> &c) { static_assert(R == 3, "three rows"); row[0] = a; row[1] = b; row[2] = c; }
};
typedef mat<3, 3> float3x3; typedef mat<3, 4> float3x4; typedef mat<4, 3> float4x3;
template <int R, int C> inline vec<float, R> mul(const mat<R, C> &m, const vec<float, C> &v) { vec<float, R> r; for (int i = 0; i < R; i++) r.d[i] = dot(m.row[i], v); return r; }
template <int R, int C> inline mat<C, R> transpose(const mat<R, C> &m) { mat<C, R> t; for (int i = 0; i < R; i++) for (int j = 0; j < C; j++) t.row[j].d[i] = m.row[i].d[j]; return t; }
#define row_major

/* ---- resources over host memory ---- */
enum AddressMode { ADDRESS_REPEAT = 0, ADDRESS_MIRRORED_REPEAT = 1 };
struct SamplerState { int address = ADDRESS_REPEAT; };

template <class T> struct texel_of;
template <> struct texel_of<float> { enum { n = 1 }; static float get(const float *p) { return p[0]; } };
template <int N> struct texel_of<vec<float, N> > { enum { n = N }; static vec<float, N> get(const float *p) { vec<float, N> r; for (int i = 0; i < N; i++) r.d[i] = p[i]; return r; } };

inline int wrap_texel(int i, int n, int mode) {
    if (mode == ADDRESS_MIRRORED_REPEAT) { int p = 2 * n, m = i % p; if (m < 0) m += p; return m < n ? m : p - 1 - m; }
    int m = i % n; return m < 0 ? m + n : m;
}

/* a texture of `stride` floats per stored texel (>= the components of T), mip l of (w >> l) x (h >> l) texels at mip[l] */
template <class T = float4> struct Texture2D {
    const float *mip[16] = {};
    uint w = 0, h = 0, levels = 0, stride = texel_of<T>::n;
    T fetch(int x, int y, uint level) const {
        if (level >= levels) return T(0.0f);
        const uint lw = w >> level ? w >> level : 1u, lh = h >> level ? h >> level : 1u;
        if (x < 0 || y < 0 || (uint)x >= lw || (uint)y >= lh) return T(0.0f);
        return texel_of<T>::get(mip[level] + (size_t)stride * ((size_t)y * lw + (size_t)x));
    }
    template <class I> T Load(const vec<I, 3> &p) const { return fetch((int)p.d[0], (int)p.d[1], (uint)p.d[2]); }
    template <class I> T operator[](const vec<I, 2> &p) const { return fetch((int)p.d[0], (int)p.d[1], 0); }
    void GetDimensions(uint &ow, uint &oh) const { ow = w; oh = h; }
    template <class L> T SampleLevel(const SamplerState &s, const float2 &uv, L) const {
        if (w == 1 && h == 1) return fetch(0, 0, 0);
        const float x = uv.x * (float)w - 0.5f, y = uv.y * (float)h - 0.5f;
        const float fx0 = std::floor(x), fy0 = std::floor(y);
        const float fx = x - fx0, fy = y - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int xa = wrap_texel(x0, (int)w, s.address), xb = wrap_texel(x0 + 1, (int)w, s.address);
        const int ya = wrap_texel(y0, (int)h, s.address), yb = wrap_texel(y0 + 1, (int)h, s.address);
        const T top = fetch(xa, ya, 0) * T(1.0f - fx) + fetch(xb, ya, 0) * T(fx);
        const T bot = fetch(xa, yb, 0) * T(1.0f - fx) + fetch(xb, yb, 0) * T(fx);
        return top * T(1.0f - fy) + bot * T(fy);
    }
};

template <class T> struct RWTexture2D {
    T *data = nullptr;
    uint w = 0, h = 0;
    template <class I> T &operator[](const vec<I, 2> &p) const { return data[(size_t)p.d[1] * w + (size_t)p.d[0]]; }
    void GetDimensions(uint &ow, uint &oh) const { ow = w; oh = h; }
};

template <class T> struct StructuredBuffer {
    const T *data = nullptr;
    uint count = 0;
    /* by value (HLSL methods are not const-qualified); an index past the end reads zeros, as robust buffer access does (and as the oracle's tables do) */
    T operator[](uint i) const { if (i < count) return data[i]; T zero; std::memset(static_cast<void *>(&zero), 0, sizeof zero); return zero; }
    void GetDimensions(uint &size, uint &stride) const { size = count; stride = (uint)sizeof(T); }
};
template <class T> struct RWStructuredBuffer {
    T *data = nullptr;
    uint count = 0;
    T &operator[](uint i) const { return data[i]; }
    void GetDimensions(uint &size, uint &stride) const { size = count; stride = (uint)sizeof(T); }
};
inline uint NonUniformResourceIndex(uint i) { return i; }

namespace vk {
/* buffer device addresses are host addresses here */
template <class T> inline T RawBufferLoad(uint64_t addr) { T r; std::memcpy(static_cast<void *>(&r), reinterpret_cast<const void *>((uintptr_t)addr), sizeof(T)); return r; }
}

/* ---- ray tracing: TraceRay hands the ray to two functions the caller supplies ---- */
struct RayDesc { float3 Origin; float TMin; float3 Direction; float TMax; };
struct RayHit { uint instanceIndex, geometryIndex, primitiveIndex; float2 barycentrics; };
typedef int (*ClosestHitFn)(void *user, const float origin[3], const float direction[3], float tmax, RayHit *hit);   /* 1 = hit, *hit filled */
typedef int (*AnyHitFn)(void *user, const float origin[3], const float direction[3], float tmax);                   /* 1 = something is hit */
struct RaytracingAccelerationStructure { void *user = nullptr; ClosestHitFn closest = nullptr; AnyHitFn any = nullptr; };
enum { RAY_FLAG_FORCE_OPAQUE = 0x01, RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH = 0x04, RAY_FLAG_SKIP_CLOSEST_HIT_SHADER = 0x08 };

/* the state of the shader invocation that is running on this thread */
struct Invocation { uint3 index = uint3(0u, 0u, 0u), dimensions = uint3(1u, 1u, 1u); RayHit hit = {}; };
inline Invocation &invocation() { static thread_local Invocation s; return s; }
inline uint3 DispatchRaysIndex() { return invocation().index; }
inline uint3 DispatchRaysDimensions() { return invocation().dimensions; }
inline uint InstanceIndex() { return invocation().hit.instanceIndex; }
inline uint GeometryIndex() { return invocation().hit.geometryIndex; }
inline uint PrimitiveIndex() { return invocation().hit.primitiveIndex; }

}  // namespace hlsl
