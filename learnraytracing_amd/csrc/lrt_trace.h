// Device restatement of the reference hot path (src/cpu/maths.{h,cpp}, parallel.cpp),
// written for one work-item per pixel on gfx950.
//
// Parity rules are kept literally: left-to-right RNG draw order,
// XorShift32 13/17/15, rejection tests, double normalisation, member vs free
// normalize, the reference's association order in every expression, glibc-exact
// transcendentals (lrt_libm.h), IEEE sqrt/div, and the build uses
// -ffp-contract=off so no a*b+c is fused. The recursive Trace() is flattened into a
// loop that pushes (matE + lightE, material) per scatter event and then folds the
// stack from the leaf outwards, which evaluates exactly the reference's
// `matE + lightE + attenuation * Trace(...)` (parallel.cpp:214) in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lrt_libm.h"

namespace lrt {

#define LRT_DEV __host__ __device__ __forceinline__

constexpr float kPI = 3.1415926f;     // maths.h:5
constexpr float kMinT = 0.001f;       // parallel.cpp:9
constexpr float kMaxT = 1.0e7f;       // parallel.cpp:10

// A/B builds only (profiles/r11_shade prices each with a build that has it alone taken out); the
// defaults are the kept state, and every setting gives the same bits.
#ifndef LRT_SHADE_HEAD
#define LRT_SHADE_HEAD 1    // ScatterDir: dot(r_in.dir, rec.normal) and reflect once for the three materials
#endif
#ifndef LRT_SHADE_DRAWS
#define LRT_SHADE_DRAWS 1   // ScatterDir: the scatter's first three draws taken once
#endif
#ifndef LRT_SHADE_ROOT1
#define LRT_SHADE_ROOT1 1   // SphereRoots: one root chosen first
#endif

struct float3_ { float x, y, z; };    // maths.h:10-61 (own type: no vendor operators)
using F3 = float3_;

LRT_DEV F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
LRT_DEV F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }   // maths.h:63
LRT_DEV F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }   // maths.h:67
LRT_DEV F3 operator*(F3 a, F3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }   // maths.h:71
LRT_DEV F3 operator*(F3 a, float b) { return f3(a.x * b, a.y * b, a.z * b); }      // maths.h:75
LRT_DEV F3 operator*(float a, F3 b) { return f3(a * b.x, a * b.y, a * b.z); }      // maths.h:79
LRT_DEV F3 operator-(F3 a) { return f3(-a.x, -a.y, -a.z); }                        // maths.h:27
LRT_DEV float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }        // maths.h:83
LRT_DEV F3 cross(F3 a, F3 b) {                                                      // maths.h:87-92
    return f3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x);
}
// Correctly rounded sqrt and reciprocal (the IEEE results the reference's sqrtf and 1/x
// give) in fewer instructions than LLVM's generic expansions, which also handle operands
// the path almost never produces:
//  * sqrt: v_sqrt_f32 is faithful (within 1 ulp); one residual check of each neighbour,
//    fma(-s', s, x), picks the correctly rounded root. This is LLVM's own sequence minus
//    the denormal scaling and the 0/inf class fix-up, and equals __builtin_sqrtf for
//    every float >= 2^-104 (checked exhaustively on gfx950: tools/fpexact.hip).
//  * reciprocal: v_rcp_f32 plus two Newton steps in fma, equal to 1.0f / x for every
//    float with |x| in [2^-125, 2^125] (exhaustive, tools/fpexact.hip).
// Operands outside those ranges (or NaN) send the whole wave through the generic
// sequence: a wave-uniform branch, essentially never taken. Host builds (the BVH
// diagnostics) use the plain operations.
// sqrt_fast / rcp_fast are the bare sequences, for call sites whose operand is proven to lie in
// the fast range (the proof stands at each site, and in DESIGN §2); sqrt_rn / rcp_rn add the
// range check and are what every other caller uses.
LRT_DEV float sqrt_fast(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __int_as_float(__float_as_int(s) - 1);
    const float su = __int_as_float(__float_as_int(s) + 1);
    const float rd = __builtin_fmaf(-sd, s, x);
    const float ru = __builtin_fmaf(-su, s, x);
    s = rd <= 0.0f ? sd : s;
    s = ru > 0.0f ? su : s;
    return s;
#else
    return __builtin_sqrtf(x);
#endif
}
LRT_DEV float rcp_fast(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r = __builtin_amdgcn_rcpf(x);
    float e = __builtin_fmaf(-x, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    e = __builtin_fmaf(-x, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    return r;
#else
    return 1.0f / x;
#endif
}
LRT_DEV float sqrt_rn(float x) {
    float s = sqrt_fast(x);
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_expect(__ballot(!(x >= 0x1p-96f)) != 0, 0)) s = __builtin_sqrtf(x);
#endif
    return s;
}
LRT_DEV float rcp_rn(float x) {
    float r = rcp_fast(x);
#if defined(__HIP_DEVICE_COMPILE__)
    const float ax = __builtin_fabsf(x);
    if (__builtin_expect(__ballot(!(ax >= 0x1p-125f && ax <= 0x1p125f)) != 0, 0)) r = 1.0f / x;
#endif
    return r;
}
// x / kPI, the constant divisor of the Lambert light sample (parallel.cpp:129), without the
// generic division: with c = RN(1 / kPI), q = x * c is within a few ulps of the quotient, the
// residual r = fma(-q, kPI, x) is exact, and fma(r, c, q) rounds to x / kPI. Equal to the
// division for x = +0 and every float in [2^-104, FLT_MAX] (every bit pattern swept on the
// host, tests/test_exact_div.py, and on gfx950, tools/fpexact.hip). Below 2^-104 the residual
// falls among the denormals and stops being exact, -0 comes out as +0 and infinity as NaN,
// and the path's operand max(0, l.nl) * omega is never negative: all of those (and NaN) take
// the division, wave-uniformly on the device like sqrt_rn. One unsigned compare of the bit
// pattern covers the range, as in rsqrt_len; +0 is the common operand (a light below the
// horizon) and is tested beside it.
constexpr float kRcpPI = 1.0f / kPI;
LRT_DEV float div_pi_fast(float x) {
    float q = x * kRcpPI;
    const float r = __builtin_fmaf(-q, kPI, x);
    return __builtin_fmaf(r, kRcpPI, q);
}
LRT_DEV bool div_pi_in_range(float x) {
    const uint32_t u = libm::f2u(x);
    return u - 0x0b800000u <= 0x7f7fffffu - 0x0b800000u || u == 0u;
}
LRT_DEV float div_pi(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    float q = div_pi_fast(x);
    if (__builtin_expect(__ballot(!div_pi_in_range(x)) != 0, 0)) q = x / kPI;
    return q;
#else
    return div_pi_in_range(x) ? div_pi_fast(x) : x / kPI;
#endif
}
LRT_DEV float length(F3 v) { return sqrt_rn(v.x * v.x + v.y * v.y + v.z * v.z); } // maths.h:15
// rcp_rn(sqrt_rn(d)), normalize's factor, with ONE range check for both steps: for a finite
// d >= 2^-96 the root is the fast sequence's, and it lies in [2^-48, 2^64], inside rcp_rn's
// [2^-125, 2^125], so neither of the two checks could fire. The test is one unsigned compare
// of the bit pattern, f2u(d) - f2u(2^-96) <= f2u(FLT_MAX) - f2u(2^-96): zero, denormals and
// smaller normals wrap around to large values, negatives (sign bit), infinity and NaN lie
// above the span by themselves. A lane outside sends the wave through the checked pair, as
// before.
LRT_DEV float rsqrt_len(float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    float k = rcp_fast(sqrt_fast(d));
    if (__builtin_expect(__ballot(libm::f2u(d) - 0x0f800000u > 0x7f7fffffu - 0x0f800000u) != 0, 0))
        k = rcp_rn(sqrt_rn(d));
    return k;
#else
    return 1.0f / __builtin_sqrtf(d);
#endif
}
LRT_DEV F3 normalize(F3 v) {                                                        // maths.h:93
    float k = rsqrt_len(v.x * v.x + v.y * v.y + v.z * v.z);   // length()'s sum, same order
    return f3(v.x * k, v.y * k, v.z * k);
}
// normalize() of a vector that is already unit length to a few ulps (the reference
// normalises twice: every Ray ctor normalises its direction again, maths.h:133-137).
// Its |y|^2 lies within kRenormR ulps of 1, so 1/sqrt(|y|^2) comes from a table of
// rcp_rn(sqrt_rn(d)) for those d, filled with the very same operations (renorm_lut_fill):
// same bits as normalize(y) with ~12 fewer instructions. Any other |y|^2 computes.
constexpr int kRenormR = 64;
constexpr int kRenormBytes = ((2 * kRenormR + 1) * 4 + 15) / 16 * 16;
LRT_DEV void renorm_lut_fill(float* lut, int tid, int block) {
    for (int j = tid; j <= 2 * kRenormR; j += block) {
        const float d = libm::u2f((uint32_t)(0x3f800000 + j - kRenormR));
        lut[j] = rcp_rn(sqrt_rn(d));
    }
}
constexpr int kPowTableBytes = 16 * 8 + 16 * 8 + 32 * 8;   // powf tables (lrt_libm.h) staged in LDS
// v / l for a divisor whose correctly rounded reciprocal r = RN(1 / l) is at hand: q = v * r is
// within 2 ulps, and two residual corrections q += fma(-q, l, v) * r reach the correctly rounded
// quotient (the second is Markstein's step: a faithful q, an exact residual, a correctly rounded
// r). This is LLVM's own division sequence without v_div_scale's scaling and v_div_fixup.
// Valid for l in [0.5, 2] and 2^-96 <= |v| <= 2^96: there q is normal and each residual, about
// 2^-24 |v|, is a normal float too, so both fmas are exact where the argument needs them; every
// significand of l in that range against dividends at the edges and across the range, and 2^30
// random pairs, on the host (tests/test_exact_div.py) and on gfx950 (tools/fpexact.hip).
// Not valid for a zero dividend: -0 / l is -0, the short form gives +0 (fma(+0, r, -0)).
LRT_DEV float div_by_rcp(float v, float l, float r) {
    float q = v * r;
    float e = __builtin_fmaf(-q, l, v);
    q = __builtin_fmaf(e, r, q);
    e = __builtin_fmaf(-q, l, v);
    return __builtin_fmaf(e, r, q);
}
// v / l for the three components of v with one reciprocal: rcp_fast(l) is RN(1 / l) for every l
// in div_by_rcp's range (above: |l| in [2^-125, 2^125]; the host divides). The range test is one
// unsigned compare of l's bit pattern (NaN and negatives lie outside) and the lower bound on the
// smallest |component|. The upper bound 2^96 is the caller's: normalize_member's l = length(v)
// in [0.5, 2] holds every |component| below 2 (1 + 2^-22). A lane outside the range sends the
// wave through the three plain divisions.
LRT_DEV bool member_quot_in_range(F3 v, float l) {
    const float lo = __builtin_fminf(__builtin_fminf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), __builtin_fabsf(v.z));
    return libm::f2u(l) - 0x3f000000u <= 0x40000000u - 0x3f000000u && lo >= 0x1p-96f;
}
LRT_DEV F3 member_quot(F3 v, float l) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (!member_quot_in_range(v, l)) return f3(v.x / l, v.y / l, v.z / l);
#endif
    const float r = rcp_fast(l);
    F3 q = f3(div_by_rcp(v.x, l, r), div_by_rcp(v.y, l, r), div_by_rcp(v.z, l, r));
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_expect(__ballot(!member_quot_in_range(v, l)) != 0, 0)) q = f3(v.x / l, v.y / l, v.z / l);
#endif
    return q;
}
// maths.h:19, f3(v.x / l, v.y / l, v.z / l). Its one caller, the Lambert light sample's
// l = su cos sin + sv sin sin + sw cos, has length 1 to a few ulps, so the range test is
// essentially never failed.
LRT_DEV F3 normalize_member(F3 v) { return member_quot(v, length(v)); }
// reflect and refract with their dot(v, n) handed in (ScatterDir computes it once for the three
// materials): every other operation, and its order, is the source's.
LRT_DEV F3 reflect_dn(F3 v, F3 n, float dn) { return v + 2.0f * (-dn * n); }
LRT_DEV F3 reflect(F3 v, F3 n) { return v + 2.0f * (-dot(v, n) * n); }             // maths.h:100-103
LRT_DEV bool refract_dt(F3 v, F3 n, float dt, float nint, F3& out) {
    float discr = 1.0f - nint * nint * (1.0f - dt * dt);
    if (discr > 0) {
        out = nint * (v - n * dt) - n * sqrt_rn(discr);
        return true;
    }
    return false;
}
LRT_DEV bool refract(F3 v, F3 n, float nint, F3& out) {                             // maths.h:106-118
    float dt = dot(v, n);
    float discr = 1.0f - nint * nint * (1.0f - dt * dt);
    if (discr > 0) {
        out = nint * (v - n * dt) - n * sqrt_rn(discr);
        return true;
    }
    return false;
}
// schlick's r0 depends on the material alone: pack_scene evaluates it once per Dielectric, with
// these very operations (IEEE on the host, contraction off), into the material row float a
// Dielectric does not otherwise use (the roughness slot), and the kernels read it there.
LRT_DEV float schlick_r0(float ri) {                                                // maths.h:124-125
    float r0 = (1.0f - ri) / (1.0f + ri);
    return r0 * r0;
}
LRT_DEV float schlick_with_r0(float cosine, float r0, const libm::PowTables& T) {  // maths.h:126
    return r0 + (1.0f - r0) * libm::powf5(1.0f - cosine, T);
}
LRT_DEV float schlick(float cosine, float ri, const libm::PowTables& T) {          // maths.h:122-127
    return schlick_with_r0(cosine, schlick_r0(ri), T);
}
LRT_DEV float schlick(float cosine, float ri) { return schlick(cosine, ri, libm::pow_tables()); }

struct Ray {                                                                        // maths.h:130-145
    F3 orig, dir;
};
LRT_DEV Ray make_ray(F3 o, F3 d) { Ray r; r.orig = o; r.dir = normalize(d); return r; }
LRT_DEV F3 renormalize(F3 y, const float* lut) {
    if (!lut) return normalize(y);
    const float d = y.x * y.x + y.y * y.y + y.z * y.z;   // length()'s sum, same order
    const int j = libm::f2u_i(d) - 0x3f800000 + kRenormR;
    float k;
    if ((unsigned)j <= 2u * kRenormR) k = lut[j];
    else k = rcp_rn(sqrt_rn(d));
    return f3(y.x * k, y.y * k, y.z * k);
}
LRT_DEV F3 point_at(const Ray& r, float t) { return r.orig + r.dir * t; }

struct Hit { F3 pos, normal; float t; };                                            // maths.h:148-153

// ---- RNG: maths.cpp:7-49 with the state in a register (one stream per pixel-sample)
LRT_DEV uint32_t XorShift32(uint32_t& s) {
    uint32_t x = s;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 15;
    s = x;
    return x;
}
LRT_DEV float RandomFloat01(uint32_t& s) { return (float)(XorShift32(s) & 0xFFFFFF) * (1.0f / 16777216.0f); }
// The draw's integer k = XorShift32 & 0xFFFFFF as a float, kf: exact (k < 2^24), and so is every
// product of kf with a power of two. Where a draw R = kf * 2^-24 only enters a sum or a product
// whose other steps are exact, the source's chain has ONE rounding, and the forms below take that
// rounding in one instruction (explicit fma: the build has contraction off). Each returns the bits
// of the source form for every k (swept on the host and on gfx950, lrt_rng_form_sweep):
//  * 2 R - 1 (the rejection candidates, RandomUnitVector's z): 2 R = kf * 2^-23 is exact, so the
//    source rounds kf * 2^-23 - 1 once, as fma(kf, 2^-23, -1) does.
//  * R * 2 * kPI and 2 * kPI * R: R * 2 and 2 * kPI are exact, so each is one rounding of the
//    real product kf * 2^-23 * kPI, as kf * (kPI * 2^-23) is (the constant is kPI's significand,
//    exact; the smallest non-zero product, 3.7e-7, is far above the denormals).
//  * (float)x + R (the camera's pixel offset) and 1 - R: one rounding of x + kf * 2^-24 and of
//    1 - kf * 2^-24.
LRT_DEV float RandomK24(uint32_t& s) { return (float)(XorShift32(s) & 0xFFFFFF); }
LRT_DEV float rng_signed(float kf) { return __builtin_fmaf(kf, 0x1p-23f, -1.0f); }            // 2 R - 1
LRT_DEV float rng_angle(float kf) { return kf * (kPI * 0x1p-23f); }                           // R * 2 * kPI
LRT_DEV float rng_offset(float kf, float x) { return __builtin_fmaf(kf, 0x1p-24f, x); }       // x + R
LRT_DEV float rng_one_minus(float kf) { return __builtin_fmaf(kf, -0x1p-24f, 1.0f); }         // 1 - R
LRT_DEV F3 RandomInUnitDisk(uint32_t& s) {
    F3 p;
    do {
        float a = RandomK24(s);
        float b = RandomK24(s);
        p = f3(rng_signed(a), rng_signed(b), 0.0f);   // 2.0f * f3(a, b, 0) - f3(1, 1, 0)
    } while (dot(p, p) >= 1.0f);
    return p;
}
// RandomUnitVector and RandomInUnitSphere from draws already taken (kz, ka; a, b, c: RandomK24's
// floats, in stream order). ScatterDir takes a scatter's first three draws once for whichever
// materials the wave's lanes hold; the functions of the source's names take their own draws.
LRT_DEV F3 UnitVectorOf(float kz, float ka) {
    float z = rng_signed(kz);   // RandomFloat01() * 2.0f - 1.0f
    float a = rng_angle(ka);    // RandomFloat01() * 2.0f * kPI
    float r = sqrt_rn(1.0f - z * z);
    float sa, ca;
    libm::sincosf(a, &sa, &ca);   // bit-identical to separate cosf(a), sinf(a)
    float x = r * ca;
    float y = r * sa;
    return f3(x, y, z);
}
LRT_DEV F3 RandomUnitVector(uint32_t& s) {
    float z = rng_signed(RandomK24(s));   // RandomFloat01() * 2.0f - 1.0f
    float a = rng_angle(RandomK24(s));    // RandomFloat01() * 2.0f * kPI
    float r = sqrt_rn(1.0f - z * z);
    float sa, ca;
    libm::sincosf(a, &sa, &ca);   // bit-identical to separate cosf(a), sinf(a)
    float x = r * ca;
    float y = r * sa;
    return f3(x, y, z);
}
// (a, b, c): the first candidate's draws; s: the state after them, from which the retries go on
LRT_DEV F3 InUnitSphereOf(float a, float b, float c, uint32_t& s) {
    F3 p;
    for (;;) {
        p = f3(rng_signed(a), rng_signed(b), rng_signed(c));   // 2.0f * f3(a, b, c) - f3(1, 1, 1)
        // the reference tests p.length() >= 1.0 (maths.cpp:47). With s = x*x + y*y + z*z
        // summed in the same order, the correctly rounded sqrt(s) >= 1 iff s >= 1:
        // sqrt(1 - 2^-24) = 1 - 2^-25 - 2^-51 rounds down to 1 - 2^-24, and sqrt is
        // monotonic, so the sqrt can go
        if (!(p.x * p.x + p.y * p.y + p.z * p.z >= 1.0f)) break;
        a = RandomK24(s);
        b = RandomK24(s);
        c = RandomK24(s);
    }
    return p;
}
LRT_DEV F3 RandomInUnitSphere(uint32_t& s) {
    F3 p;
    do {
        float a = RandomK24(s);
        float b = RandomK24(s);
        float c = RandomK24(s);
        p = f3(rng_signed(a), rng_signed(b), rng_signed(c));   // as InUnitSphereOf
    } while (p.x * p.x + p.y * p.y + p.z * p.z >= 1.0f);
    return p;
}

// ---- scene as the kernel sees it -------------------------------------------------
// Sphere: float4(center.xyz, radius*radius). The reference only ever uses the radius
// squared (maths.cpp:59, parallel.cpp:109), so r*r is folded once on the host.
// Material: three float4 rows: (albedo.xyz, type), (emissive.xyz, roughness),
// (attenuation.xyz, ri) where attenuation = albedo (Lambert, Metal) or 1 (Dielectric,
// parallel.cpp:90,144,192). Only Metal reads its roughness (parallel.cpp:137-148), so a
// Dielectric's row carries schlick_r0(ri) in that float instead (pack_scene).
struct Material {
    F3 albedo;
    int type;
    int id;   // the table index: the reference's `&mat == &smat` self test (parallel.cpp:98)
    F3 emissive;
    float roughness;   // Dielectric: schlick_r0(ri)
    F3 att;
    float ri;
};
LRT_DEV Material load_material(const float4* __restrict__ mats, int id) {
    float4 a = mats[3 * id + 0];
    float4 e = mats[3 * id + 1];
    float4 b = mats[3 * id + 2];
    Material m;
    m.albedo = f3(a.x, a.y, a.z);
    m.type = libm::f2u_i(a.w);
    m.id = id;
    m.emissive = f3(e.x, e.y, e.z);
    m.roughness = e.w;
    m.att = f3(b.x, b.y, b.z);
    m.ri = b.w;
    return m;
}

}  // namespace lrt
#include "lrt_bvh.h"
#include "lrt_grid.h"
namespace lrt {

// The closest-hit structure a kernel instance is compiled for (template parameter kAcc): the
// reference's linear scan, the 4-wide BVH (lrt_bvh.h) or the uniform grid (lrt_grid.h). All
// three return the scan's bits.
enum : int { kAccScan = 0, kAccBvh = 1, kAccGrid = 2 };

struct SceneView {
    const float4* sph;                 // LDS or global
    const float4* __restrict__ mats;   // global (per-lane gather, L1/L2 resident)
    const int* __restrict__ lights;    // emissive sphere ids in index order
    int count;
    int nlights;
    BvhView bv;                        // the BVH (kAcc == kAccBvh)
    GridView gv;                       // the uniform grid (kAcc == kAccGrid)
    unsigned short* bstk;              // this lane's BVH traversal stack (LDS)
    int bstride;
    libm::PowTables pow;               // powf tables for Dielectric's schlick (LDS copy)
    const float* rnlut;                // renormalize() table (LDS), null: plain normalize
#ifdef LRT_EXP_SECSTATS
    unsigned long long* secstats;      // diagnostic: per section {wave executions, active lanes, cycles}
    unsigned long long* sectime;       // this wave's LDS bookkeeping
#endif
};

// Diagnostic builds only (LRT_EXP_SECSTATS): per section, how many times a wave enters
// it, how many lanes are active then, and the shader cycles spent in it until the next
// section switch (s_memtime, bookkept in LDS by the first active lane so divergence
// cannot desynchronise it). sec_count enters and counts; sec_enter only switches time.
enum { kSecHit, kSecLambert, kSecShadow, kSecMetal, kSecDiel, kSecPost, kSecFold, kSecCamera, kSecOther, kSecHit0,
       kSecShadow0, kSecN };   // *0: a path's first closest hit / first shadow rays (coherent)
LRT_DEV void sec_enter(const SceneView& sc, int sec, bool count) {
#if defined(LRT_EXP_SECSTATS) && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long m = __ballot(1);
    if ((int)__lane_id() == __ffsll((long long)m) - 1) {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        // LDS, this wave: [0] section, [1] since, [2 + s] cycles, [2 + kSecN + s] entries,
        // [2 + 2 kSecN + s] active lanes -- no global atomics in the loop (they would sit
        // in vmcnt and be charged to whichever section waits next)
        unsigned long long* w = sc.sectime;
        const int cur = (int)w[0];
        w[2 + cur] += now - w[1];
        w[0] = (unsigned long long)sec;
        w[1] = now;
        if (count) {
            w[2 + kSecN + sec] += 1;
            w[2 + 2 * kSecN + sec] += (unsigned long long)__popcll(m);
        }
    }
#else
    (void)sc;
    (void)sec;
    (void)count;
#endif
}
LRT_DEV void sec_count(const SceneView& sc, int sec) { sec_enter(sc, sec, true); }

// HitSphere's root selection against the running closestT (maths.cpp:61-90): the first
// root if it lies in (tMin, closestT), else the second. (A branchless form -- sqrt for every
// lane, selects -- measured slower: the divergent branch around the sqrt is cheap when no
// lane takes it.)
// Inside, the reference's if / else-if is taken as selects over both roots, its && as bitwise
// ands: each short-circuit was a divergent region of its own, whose exec bookkeeping (scalar
// instructions, a branch) cost more than the second root's add (the grid walk: profiles/r4_y).
// kChk = false (a scene whose every r*r >= 2^-70: Context::roots_in_range): the root's operand
// -ifHit > 0, with ifHit = fl(fl(rr - p*p) - r2), is then never below 2^-94, so the fast sequence
// applies without its range check. Write A = fl(rr - p*p) (any float; NaN makes ifHit NaN, which
// fails ifHit < 0). If A <= r2 / 2 the exact difference r2 - A is at least r2 / 2 >= 2^-71, and
// so is its rounding. Otherwise r2 / 2 < A < r2, A - r2 is exact (Sterbenz) and non-zero, and
// both floats are at least 2^-71, hence multiples of 2^-94: so is their difference. (-ifHit =
// +inf, from an overflowed p*p, takes the fast sequence with the check too.) DESIGN §2.
template <bool kChk = true>
LRT_DEV void SphereRoots(float rsProj, float ifHit, float tMin, float& closestT, int& id, int i) {
    if (ifHit < 0.0f) {
        const float halfCut = kChk ? sqrt_rn(-ifHit) : sqrt_fast(-ifHit);
        const float t1 = rsProj - halfCut, t2 = rsProj + halfCut;
#if LRT_SHADE_ROOT1
        // One root chosen first: u = t1 > tMin ? t1 : t2, accepted iff t2 > tMin and u < closestT.
        // Three compares and three selects for the source's four and three. halfCut >= 0 (a root,
        // or +inf), so for a finite rsProj t2 = fl(p + h) >= fl(p - h) = t1: rounding is monotonic.
        //  * t1 > tMin: then t2 >= t1 > tMin holds too, u = t1, and the test is t1 < closestT, the
        //    source's first branch. Where it fails, t2 >= t1 >= closestT fails the second as well.
        //  * otherwise (t1 <= tMin, or t1 NaN): the first branch is not taken, u = t2, and the test
        //    is the second branch's, t2 > tMin && t2 < closestT.
        // Operands that are not finite: a NaN rsProj makes ifHit NaN and never gets here; rsProj =
        // +-inf makes ifHit -inf (or NaN), halfCut +inf, and one root NaN, the other +-inf: (NaN,
        // +inf) gives u = +inf, not below closestT; (-inf, NaN) gives u = NaN and fails t2 > tMin;
        // a finite rsProj with halfCut = +inf gives (-inf, +inf), u = +inf. The source accepts none
        // of these either, and a NaN closestT or tMin fails every compare in both forms. Checked on
        // the host over designed and random operands (lrt_sphere_roots_eval). DESIGN §2.
        const float u = t1 > tMin ? t1 : t2;
        const bool ok = (t2 > tMin) & (u < closestT);
        id = ok ? i : id;
        closestT = ok ? u : closestT;
#else
        const bool ok1 = (t1 > tMin) & (t1 < closestT);
        const bool ok2 = (t2 > tMin) & (t2 < closestT);
        id = (ok1 | ok2) ? i : id;
        closestT = ok1 ? t1 : ok2 ? t2 : closestT;
#endif
    }
}

// HitWorld + HitSphere (parallel.cpp:54-73, maths.cpp:51-94). The per-sphere test
// is the reference's; hit position and normal are computed once for the winner
// (they are pure functions of (ray, t, sphere), so this is bit-identical to the
// reference overwriting them on every closer hit).
// kNS > 0: the scene has exactly kNS spheres (the reference's kSphereCount is a compile-time
// 9, parallel.cpp:27): the scan is fully unrolled with constant LDS offsets.
template <int kAcc = 0, int kNS = 0>
LRT_DEV int ClosestHitSV(const Ray& r, float tMin, float tMax, const SceneView& sc, float& tOut,
                         bool coherent = false) {
    if constexpr (kAcc == kAccGrid)   // tMin/tMax = kMinT/kMaxT
        return ClosestHitGrid(r.orig, r.dir, sc.gv, tOut);
    if constexpr (kAcc == kAccBvh)
        return ClosestHitBVH(r.orig, r.dir, sc.bv, tOut, sc.bstk, sc.bstride, nullptr, coherent);
    float closestT = tMax;
    int id = -1;
    auto test = [&](int i, const float4& s) {
        F3 rs = f3(s.x, s.y, s.z) - r.orig;
        float rsProj = dot(rs, r.dir);
        float ifHit = dot(rs, rs) - rsProj * rsProj - s.w;
        SphereRoots(rsProj, ifHit, tMin, closestT, id, i);
    };
    if constexpr (kNS > 0) {
        float4 next = sc.sph[0];   // one sphere ahead (as DualClosestHit)
#pragma unroll
        for (int i = 0; i < kNS; ++i) {
            const float4 s = next;
            if (i + 1 < kNS) next = sc.sph[i + 1];
            test(i, s);
        }
    } else {
        float4 next = sc.sph[0];   // one sphere ahead
        for (int i = 0; i < sc.count; ++i) {
            const float4 s = next;
            if (i + 1 < sc.count) next = sc.sph[i + 1];
            test(i, s);
        }
    }
    tOut = closestT;
    return id;
}
// The plain scan over a sphere array (host diagnostics: lrt_bvh_stats checks the BVH
// against it). Same per-sphere arithmetic and strict-< replacement as HitWorld.
LRT_DEV int ClosestHit(const F3& o, const F3& d, const float4* sph, int count, float& tOut) {
    float closestT = kMaxT;
    int id = -1;
    for (int i = 0; i < count; ++i) {
        const float4 s = sph[i];
        const F3 rs = f3(s.x, s.y, s.z) - o;
        const float rsProj = dot(rs, d);
        const float ifHit = dot(rs, rs) - rsProj * rsProj - s.w;
        SphereRoots(rsProj, ifHit, kMinT, closestT, id, i);
    }
    tOut = closestT;
    return id;
}

template <int kAcc = 0, int kNS = 0>
LRT_DEV bool HitWorld(const Ray& r, float tMin, float tMax, const SceneView& sc, Hit& outHit, int& outID,
                      bool coherent = false) {
    float closestT;
    sec_count(sc, coherent ? kSecHit0 : kSecHit);
    const int id = ClosestHitSV<kAcc, kNS>(r, tMin, tMax, sc, closestT, coherent);
    if (id < 0) return false;
    float4 s = sc.sph[id];
    outHit.pos = point_at(r, closestT);
    outHit.normal = normalize(outHit.pos - f3(s.x, s.y, s.z));
    outHit.t = closestT;
    outID = id;
    return true;
}

// Scatter (parallel.cpp:78-196). The reference's `&mat == &smat` self test is the
// comparison of table indices (matId). lightE accumulates in the same order.
// Every material ends in `Ray(rec.pos, normalize(X))`, i.e. dir = normalize(normalize(X))
// (the Ray ctor normalises again, maths.h:133-137), so ScatterDir returns X and the
// caller forms the ray once for whichever materials the wave's lanes hold; Metal's
// absorption test (:147) is applied there too. The attenuation is the material's
// `att` row (albedo or 1), read back by the fold.
// The last light sample of a Lambert scatter, left for the caller to trace together with
// the next bounce ray (TraceDual): its direction, light index and the contribution
// (mat.albedo * emissive) * (max(0, l.nl) * omega / pi) it adds if the shadow ray's
// closest hit is that light (parallel.cpp:122-132; a pure function of values known
// before the shadow test, so precomputing it changes no bits).
struct DeferredLight {
    F3 l, contrib;   // l: the shadow ray's direction
    int li;
    bool on;
    int id;          // the scattering sphere (pool kernel: its stack entry's material)
};

// kNL > 0: the scene has exactly kNL lights (the pool kernel's one-light instance: the loop is
// its single deferred sample, and the undeferred shadow scan drops out).
template <int kAcc = 0, int kNS = 0, int kNL = 0>
LRT_DEV F3 ScatterDir(const Material& mat, int matId, const Ray& r_in, const Hit& rec, F3& outLightE,
                      int& inoutRayCount, uint32_t& rng, const SceneView& sc, DeferredLight* defer = nullptr,
                      bool coherent = false) {
    outLightE = f3(0.0f, 0.0f, 0.0f);
    // The three materials' branches run one after the other for the lanes that hold each, and
    // every instruction of a branch is issued whatever its lane count. What they share is issued
    // once here, for every lane that scatters:
    //  * dn = dot(r_in.dir, rec.normal). Metal's and Dielectric's reflect (maths.h:101) and
    //    Dielectric's side test and cosine (:163-172) take it in this operand order. Lambert's nl
    //    (:128) has dot(rec.normal, r_in.dir): each product has its operands commuted, which does
    //    not change a product's bits, and the three are summed in the same order. Dielectric's
    //    refract (maths.h:108) takes dot(rdir, outwardN) with outwardN = -rec.normal where dn > 0,
    //    else rec.normal: in the first case every product is the exact negation of dn's, a sum of
    //    negations is the negation of the sum under round-to-nearest unless the sum is zero (both
    //    are +0 then, and the third product added to either gives the same), and the final sum,
    //    -dn, is not zero; so dt = dn > 0 ? -dn : dn. Nothing is reassociated.
    //  * the scatter's first three draws k1, k2, k3 with the states s1, s2, s3 after each. Lambert
    //    consumes k1, k2 (RandomUnitVector) and, in the one-light instance, k3 as its light sample's
    //    eps1 where that sample is taken (a Lambert that is itself the light leaves s2); Metal's
    //    first candidate is (k1, k2, k3) and its retries go on from s3; Dielectric's decision is k1
    //    and leaves s1. Each branch writes back the state the source's draw count leaves.
    // The scan instances only: the BVH and grid instances walk their structure from in here with
    // every register taken, and keep each branch's own code (any reshaping moved their spills).
    constexpr bool kHead = LRT_SHADE_HEAD && kAcc == kAccScan;
    constexpr bool kDraws = LRT_SHADE_DRAWS && kAcc == kAccScan;
    // the one-light instance's single sample is the stream's third draw whenever it is taken
    constexpr bool kShareK3 = kDraws && kNL == 1;
    float dn = 0.0f;
    if constexpr (kHead) dn = dot(r_in.dir, rec.normal);
    uint32_t s1 = rng, s2 = rng, s3 = rng;
    float k1 = 0.0f, k2 = 0.0f, k3 = 0.0f;
    if constexpr (kDraws) {
        k1 = RandomK24(s1);
        s2 = s1;
        k2 = RandomK24(s2);
        s3 = s2;
        k3 = RandomK24(s3);
    }
    if (mat.type == 0) {  // Lambert :81-136
        sec_count(sc, kSecLambert);
        // the first light's index and sphere, read before RandomUnitVector: their two dependent
        // LDS reads are in flight across it instead of waited for at the light loop's start
        // (config 2 -0.3 % / -0.7 % on two streams / one, config 3 -0.5 %: profiles/r6_ao)
        const int nlights = kNL > 0 ? kNL : sc.nlights;
        const int i0 = nlights > 0 ? sc.lights[0] : 0;
        const float4 s0 = sc.sph[i0];
        F3 target;
        if constexpr (kDraws) {
            target = rec.pos + rec.normal + UnitVectorOf(k1, k2);
            rng = s2;
        } else {
            target = rec.pos + rec.normal + RandomUnitVector(rng);
        }
        auto dnl = [&]() {   // nl's dot (:128)
            if constexpr (kHead) return dn;
            else return dot(rec.normal, r_in.dir);
        };
        const F3 X = target - rec.pos;
        for (int k = 0; k < nlights; ++k) {
            int i = k == 0 ? i0 : sc.lights[k];
            if (i == matId) continue;  // :98
            float4 s = k == 0 ? s0 : sc.sph[i];
            F3 c = f3(s.x, s.y, s.z);
            // sw = normalize(c - pos) and len = length(pos - c) (:103,:108): pos - c is
            // -(c - pos) exactly, so both lengths are the same float -- computed once
            const F3 cp = c - rec.pos;
            const float len = length(cp);
            const float kinv = rcp_rn(len);
            F3 sw = f3(cp.x * kinv, cp.y * kinv, cp.z * kinv);
            F3 su = normalize(cross(__builtin_fabsf(sw.x) > 0.01f ? f3(0.0f, 1.0f, 0.0f) : f3(1.0f, 0.0f, 0.0f), sw));
            F3 sv = cross(sw, su);
            float cosAMax = sqrt_rn(1.0f - s.w / (len * len));                    // :109
            float ke;
            if constexpr (kShareK3) {
                ke = k3;
                rng = s3;
            } else {
                ke = RandomK24(rng);
            }
            float eps1 = ke * (1.0f / 16777216.0f);   // RandomFloat01
            float cosA = rng_one_minus(ke) + eps1 * cosAMax;   // 1.0f - eps1 + eps1 * cosAMax
            float sinA = sqrt_rn(1.0f - cosA * cosA);
            float phi = rng_angle(RandomK24(rng));   // 2.0f * kPI * eps2
            float sphi, cphi;
            libm::sincosf(phi, &sphi, &cphi);   // bit-identical to cosf(phi), sinf(phi)
            F3 l = su * cphi * sinA + sv * sphi * sinA + sw * cosA;                         // :116
            l = normalize_member(l);                                                      // :117
            float tLight;
            ++inoutRayCount;                                                              // :122
            if (defer && k == nlights - 1) {   // the last light: traced with the bounce ray
                float omega = 2.0f * kPI * (1.0f - cosAMax);
                F3 nl = dnl() < 0.0f ? rec.normal : -rec.normal;   // dot(rec.normal, rdir) < 0 (:128)
                float d = dot(l, nl);
                float mx = (0.0f < d) ? d : 0.0f;   // std::max(0.0f, d)
                const float4 e = sc.mats[3 * i + 1];
                defer->l = renormalize(l, sc.rnlut);   // the shadow Ray's ctor normalises again (maths.h:133-137)
                defer->contrib = (mat.albedo * f3(e.x, e.y, e.z)) * div_pi(mx * omega);   // mx * omega / kPI
                defer->li = i;
                defer->on = true;
                continue;
            }
            sec_count(sc, coherent ? kSecShadow0 : kSecShadow);
            bool lit;
            if constexpr (kAcc == kAccGrid) {
                lit = ShadowReachesLightGrid(rec.pos, renormalize(l, sc.rnlut), i, s, sc.gv);
            } else if constexpr (kAcc == kAccBvh) {
                Ray sr;
                sr.orig = rec.pos;
                sr.dir = renormalize(l, sc.rnlut);
                lit = ShadowReachesLightBVH(sr.orig, sr.dir, i, s, sc.bv, sc.bstk, sc.bstride, coherent);
            } else {
                Ray sr;
                sr.orig = rec.pos;
                sr.dir = renormalize(l, sc.rnlut);
                lit = ClosestHitSV<kAcc, kNS>(sr, kMinT, kMaxT, sc, tLight) == i;
            }
            sec_enter(sc, kSecLambert, false);
            if (lit) {   // HitWorld && hitID == i
                float omega = 2.0f * kPI * (1.0f - cosAMax);
                F3 nl = dnl() < 0.0f ? rec.normal : -rec.normal;   // dot(rec.normal, rdir) < 0 (:128)
                float d = dot(l, nl);
                float mx = (0.0f < d) ? d : 0.0f;   // std::max(0.0f, d)
                const float4 e = sc.mats[3 * i + 1];
                outLightE = outLightE + (mat.albedo * f3(e.x, e.y, e.z)) * div_pi(mx * omega);   // mx * omega / kPI
            }
        }
        return X;
    }
    if constexpr (!kHead && !kDraws) {   // each branch's own code, as the source has it
        if (mat.type == 1) {  // Metal :137-148
            sec_count(sc, kSecMetal);
            F3 refl = reflect(r_in.dir, rec.normal);
            return refl + mat.roughness * RandomInUnitSphere(rng);
        }
        // Dielectric :149-193 (validate() admits types 0-2 only)
        sec_count(sc, kSecDiel);
        F3 outwardN;
        F3 rdir = r_in.dir;
        F3 refl = reflect(rdir, rec.normal);
        float nint;
        F3 refr = f3(0.0f, 0.0f, 0.0f);
        float reflProb;
        float cosine;
        if (dot(rdir, rec.normal) > 0.0f) {
            outwardN = -rec.normal;
            nint = mat.ri;
            cosine = dot(rdir, rec.normal);
        } else {
            outwardN = rec.normal;
            nint = rcp_rn(mat.ri);
            cosine = -dot(rdir, rec.normal);
        }
        if (refract(rdir, outwardN, nint, refr))
            reflProb = schlick_with_r0(cosine, mat.roughness, sc.pow);   // the row's r0 = schlick_r0(mat.ri)
        else
            reflProb = 1.0f;
        return RandomFloat01(rng) < reflProb ? refl : refr;
    }
    // Metal's and Dielectric's reflect (:139,:153), once for the lanes of both
    F3 rdir = r_in.dir;
    F3 refl = f3(0.0f, 0.0f, 0.0f);
    if constexpr (kHead) refl = reflect_dn(rdir, rec.normal, dn);
    if (mat.type == 1) {  // Metal :137-148
        sec_count(sc, kSecMetal);
        if constexpr (!kHead) refl = reflect(rdir, rec.normal);
        if constexpr (kDraws) {
            rng = s3;
            return refl + mat.roughness * InUnitSphereOf(k1, k2, k3, rng);
        } else {
            return refl + mat.roughness * RandomInUnitSphere(rng);
        }
    }
    // Dielectric :149-193 (validate() admits types 0-2 only)
    sec_count(sc, kSecDiel);
    if constexpr (!kHead) {
        refl = reflect(rdir, rec.normal);
        dn = dot(rdir, rec.normal);
    }
    F3 outwardN;
    float nint;
    F3 refr = f3(0.0f, 0.0f, 0.0f);
    float reflProb;
    float cosine;
    if (dn > 0.0f) {   // dot(rdir, rec.normal) > 0
        outwardN = -rec.normal;
        nint = mat.ri;
        cosine = dn;
    } else {
        outwardN = rec.normal;
        nint = rcp_rn(mat.ri);
        cosine = -dn;
    }
    bool refracts;
    if constexpr (kHead) refracts = refract_dt(rdir, outwardN, dn > 0.0f ? -dn : dn, nint, refr);
    else refracts = refract(rdir, outwardN, nint, refr);
    if (refracts)
        reflProb = schlick_with_r0(cosine, mat.roughness, sc.pow);   // the row's r0 = schlick_r0(mat.ri)
    else
        reflProb = 1.0f;
    if constexpr (kDraws) {
        rng = s1;
        return k1 * (1.0f / 16777216.0f) < reflProb ? refl : refr;   // RandomFloat01() < reflProb
    } else {
        return RandomFloat01(rng) < reflProb ? refl : refr;
    }
}

// Scatter in the reference's shape (parallel.cpp:78-196): the attenuation, the scattered
// Ray (its ctor normalises the direction again, maths.h:133-137), the explicit light
// samples in outLightE, shadow rays counted in inoutRayCount; returns false where the
// reference absorbs (Metal scattered below the surface, :147). The RNG state and the scene
// are explicit parameters, as in the reference's own per-stream variant
// (src/cpu/README.md:42, fragmentShader.fs.glsl:175-218). `mat.id` is the material's table
// index, the reference's `&mat` identity. coherent: the active lanes' shadow rays start
// together (packet traversal, lrt_bvh.h).
template <int kAcc = 0, int kNS = 0>
LRT_DEV bool Scatter(const Material& mat, const Ray& r_in, const Hit& rec, F3& attenuation, Ray& scattered,
                     F3& outLightE, int& inoutRayCount, uint32_t& rng, const SceneView& sc, bool coherent = false) {
    const F3 X = ScatterDir<kAcc, kNS>(mat, mat.id, r_in, rec, outLightE, inoutRayCount, rng, sc, nullptr, coherent);
    scattered.orig = rec.pos;
    scattered.dir = renormalize(normalize(X), sc.rnlut);   // Ray(rec.pos, normalize(X))
    attenuation = mat.att;                                  // albedo, or (1, 1, 1) for Dielectric (:192)
    return mat.type != 1 || dot(scattered.dir, rec.normal) > 0.0f;
}

// Trace (parallel.cpp:200-227) as a loop. Scatter events are pushed on a per-lane
// stack of (matE + lightE, material id); the fold T = E + att * T from the leaf
// outwards reproduces the recursion's rounding exactly. maxDepth scatter events at
// most (the reference's depth < kMaxDepth test); MAXD >= maxDepth.
// lstk: this lane's LDS stack (kLdsLev levels, stride lstride float4); levels beyond
// it (only when MAXD > kLdsLev) go to this lane's slice of a global overflow stack
// (gstk, stride gstride; L2-resident -- few paths get that deep).
constexpr int kTraceLdsLevels = 8;
template <int MAXD, bool kFeat, int kLdsLev, int kNS>
LRT_DEV F3 TraceDual(Ray r, int maxDepth, int& inoutRayCount, uint32_t& rng, const SceneView& sc,
                     float4* lstk, int lstride, float4* gstk, size_t gstride, int ndl, F3* feat);
// ndl (LRT_F_NO_DOUBLE_LIGHT): the GL loop's doMaterialE rule (fragmentShader.fs.glsl:430,
// 456-457) -- a scatter event reached through a Lambert bounce adds no emissive; the
// terminating hit always does. kFeat: feat[0..2] receive the first hit's normal,
// position and albedo (fragmentShader.fs.glsl:444-451; left untouched on a miss).
template <int MAXD, int kAcc = 0, bool kFeat = false, int kLdsLev = kTraceLdsLevels, int kNS = 0>
LRT_DEV F3 Trace(Ray r, int maxDepth, int& inoutRayCount, uint32_t& rng, const SceneView& sc,
                 float4* lstk, int lstride, float4* gstk, size_t gstride, int ndl = 0, F3* feat = nullptr) {
    if constexpr (!kAcc)
        return TraceDual<MAXD, kFeat, kLdsLev, kNS>(r, maxDepth, inoutRayCount, rng, sc, lstk, lstride, gstk, gstride,
                                               ndl, feat);
    auto put = [&](int lvl, float4 v) {
        if (MAXD <= kLdsLev || lvl < kLdsLev) lstk[lvl * lstride] = v;
        else gstk[(size_t)(lvl - kLdsLev) * gstride] = v;
    };
    auto get = [&](int lvl) -> float4 {
        if (MAXD <= kLdsLev || lvl < kLdsLev) return lstk[lvl * lstride];
        return gstk[(size_t)(lvl - kLdsLev) * gstride];
    };
    int depth = 0;
    bool prevLambert = false;
    F3 leaf;
    for (;;) {
        Hit rec;
        int id = 0;
        ++inoutRayCount;
        // the first rays of a wave's paths start together: packet traversal (lrt_bvh.h)
        const bool coherent = depth < kPacketDepth;
        if (!HitWorld<kAcc, kNS>(r, kMinT, kMaxT, sc, rec, id, coherent)) {
            float t = 0.5f * (r.dir.y + 1.0f);
            leaf = ((1.0f - t) * f3(1.0f, 1.0f, 1.0f) + t * f3(0.5f, 0.7f, 1.0f)) * 0.3f;
            break;
        }
        Material mat = load_material(sc.mats, id);
        F3 matE = mat.emissive;
        if (kFeat && depth == 0) {   // the first hit (depth 0 is only ever seen once)
            feat[0] = rec.normal;
            feat[1] = rec.pos;
            feat[2] = mat.albedo;
        }
        F3 lightE, attenuation;
        Ray scattered;
        // :212 -- the attenuation is the material's `att` row, which the fold reads back by id
        if (depth < maxDepth &&
            Scatter<kAcc, kNS>(mat, r, rec, attenuation, scattered, lightE, inoutRayCount, rng, sc, coherent)) {
            sec_count(sc, kSecPost);
            if (ndl && prevLambert) matE = f3(0.0f, 0.0f, 0.0f);
            prevLambert = mat.type == 0;
            F3 e = matE + lightE;
            put(depth, make_float4(e.x, e.y, e.z, __int_as_float(id)));
            ++depth;
            r = scattered;
            continue;
        }
        leaf = matE;
        break;
    }
    F3 T = leaf;
    sec_count(sc, kSecFold);
    for (int d = depth - 1; d >= 0; --d) {
        float4 s = get(d);
        float4 b = sc.mats[3 * __float_as_int(s.w) + 2];
        T = f3(s.x, s.y, s.z) + f3(b.x, b.y, b.z) * T;
    }
    sec_enter(sc, kSecOther, false);
    return T;
}

// One pass over the spheres for two rays from the same origin: the next bounce ray and
// (hasShadow) a light's shadow ray. rs = c - o and dot(rs, rs) are shared -- the very
// values HitSphere computes for each ray (maths.cpp:54-59) -- and each ray keeps its own
// shrinking closestT exactly as HitWorld does, so both results are bit-identical to two
// separate scans. Saves the shadow ray's separate, partly occupied pass.
template <int kNS = 0, bool kChk = true>
LRT_DEV void DualClosestHit(const F3& o, const F3& db, bool hasShadow, const F3& ds, const SceneView& sc,
                            int& idB, float& tB, int& idS) {
    float closestB = kMaxT, closestS = kMaxT;
    idB = -1;
    idS = -1;
    auto test = [&](int i, const float4& s) {
        const F3 rs = f3(s.x, s.y, s.z) - o;
        const float rr = dot(rs, rs);
        {
            const float rsProj = dot(rs, db);
            const float ifHit = rr - rsProj * rsProj - s.w;
            SphereRoots<kChk>(rsProj, ifHit, kMinT, closestB, idB, i);
        }
        if (hasShadow) {
            const float rsProj = dot(rs, ds);
            const float ifHit = rr - rsProj * rsProj - s.w;
            SphereRoots<kChk>(rsProj, ifHit, kMinT, closestS, idS, i);
        }
    };
    if constexpr (kNS > 0) {
        // one sphere ahead: the next sphere's LDS read is in flight across this one's test (read
        // at its use, each read's latency sat between two tests: config 2 -2.7 %, config 3 -2.3 %,
        // profiles/r6_ak)
        float4 next = sc.sph[0];
#pragma unroll
        for (int i = 0; i < kNS; ++i) {
            const float4 s = next;
            if (i + 1 < kNS) next = sc.sph[i + 1];
            test(i, s);
        }
    } else {
        float4 next = sc.sph[0];
        for (int i = 0; i < sc.count; ++i) {
            const float4 s = next;
            if (i + 1 < sc.count) next = sc.sph[i + 1];
            test(i, s);
        }
    }
    tB = closestB;
}

// Trace for the linear scan with the closest hit of each bounce ray found at the end of
// the previous iteration, in one pass with the last light's shadow ray (DualClosestHit).
// Same events, draws, ray counts and accumulation order as Trace.
template <int MAXD, bool kFeat = false, int kLdsLev = kTraceLdsLevels, int kNS = 0>
LRT_DEV F3 TraceDual(Ray r, int maxDepth, int& inoutRayCount, uint32_t& rng, const SceneView& sc,
                     float4* lstk, int lstride, float4* gstk, size_t gstride, int ndl, F3* feat) {
    auto put = [&](int lvl, float4 v) {
        if (MAXD <= kLdsLev || lvl < kLdsLev) lstk[lvl * lstride] = v;
        else gstk[(size_t)(lvl - kLdsLev) * gstride] = v;
    };
    auto get = [&](int lvl) -> float4 {
        if (MAXD <= kLdsLev || lvl < kLdsLev) return lstk[lvl * lstride];
        return gstk[(size_t)(lvl - kLdsLev) * gstride];
    };
    int depth = 0;
    bool prevLambert = false;
    F3 leaf;
    Hit rec;
    int id = 0;
    ++inoutRayCount;
    bool hit = HitWorld<false, kNS>(r, kMinT, kMaxT, sc, rec, id);
    for (;;) {
        if (!hit) {
            float t = 0.5f * (r.dir.y + 1.0f);
            leaf = ((1.0f - t) * f3(1.0f, 1.0f, 1.0f) + t * f3(0.5f, 0.7f, 1.0f)) * 0.3f;
            break;
        }
        Material mat = load_material(sc.mats, id);
        F3 matE = mat.emissive;
        if (kFeat && depth == 0) {
            feat[0] = rec.normal;
            feat[1] = rec.pos;
            feat[2] = mat.albedo;
        }
        if (depth < maxDepth) {   // :212
            F3 lightE;
            DeferredLight dl;
            dl.on = false;
            const F3 X = ScatterDir<false, kNS>(mat, id, r, rec, lightE, inoutRayCount, rng, sc, &dl);
            sec_count(sc, kSecPost);
            const F3 dir = renormalize(normalize(X), sc.rnlut);
            if (mat.type != 1 || dot(dir, rec.normal) > 0.0f) {   // Metal absorbs (:147)
                // the next Trace's HitWorld (:204) and the deferred shadow ray (:122-123)
                ++inoutRayCount;
                sec_count(sc, kSecHit);
                int nid, sid;
                float nt;
                DualClosestHit<kNS>(rec.pos, dir, dl.on, dl.l, sc, nid, nt, sid);
                if (dl.on && sid == dl.li) lightE = lightE + dl.contrib;
                sec_enter(sc, kSecPost, false);
                if (ndl && prevLambert) matE = f3(0.0f, 0.0f, 0.0f);
                prevLambert = mat.type == 0;
                F3 e = matE + lightE;
                put(depth, make_float4(e.x, e.y, e.z, __int_as_float(id)));
                ++depth;
                r.orig = rec.pos;
                r.dir = dir;
                hit = nid >= 0;
                if (hit) {   // HitWorld's winner data (maths.cpp:74-76,86-88)
                    const float4 s = sc.sph[nid];
                    rec.pos = point_at(r, nt);
                    rec.normal = normalize(rec.pos - f3(s.x, s.y, s.z));
                    rec.t = nt;
                    id = nid;
                }
                continue;
            }
        }
        leaf = matE;
        break;
    }
    F3 T = leaf;
    sec_count(sc, kSecFold);
    for (int d = depth - 1; d >= 0; --d) {
        float4 s = get(d);
        float4 b = sc.mats[3 * __float_as_int(s.w) + 2];
        T = f3(s.x, s.y, s.z) + f3(b.x, b.y, b.z) * T;
    }
    sec_enter(sc, kSecOther, false);
    return T;
}

struct CameraDev {   // maths.h:217-224
    F3 origin, a, u, r, llc, horiz, vert;
    float lensRadius;
};
LRT_DEV Ray GetRay(const CameraDev& c, float s, float t, uint32_t& rng, const float* lut = nullptr) {   // maths.h:205-215
    F3 rd = c.lensRadius * RandomInUnitDisk(rng);
    F3 offset = c.r * rd.x + c.u * rd.y;
    Ray r;
    r.orig = c.origin + offset;
    r.dir = renormalize(normalize(c.llc + s * c.horiz + t * c.vert - c.origin - offset), lut);
    return r;
}

LRT_DEV uint32_t PixelSeed(uint32_t x, uint32_t y, uint32_t f) { return (x * 1973u + y * 9277u + f * 26699u) | 1u; }

}  // namespace lrt
