/* oracle/glsl_env.h — the C++ environment the reference's shader headers are written against.
 *
 * TEST INFRASTRUCTURE ONLY (see oracle/README.md).
 *
 * The reference's `src/app_*.h` are valid C++17 once something supplies vec2/vec3/vec4, mat2/mat3, the GLSL built-ins and
 * iResolution / iGlobalTime / iMouse (the author gets them from VML and vml/test/SDL_app/SDL_app.cpp, neither in the tree).
 * This header is that something, written here from SURVEY.md Appendix D's list: oracle/ref_driver.cpp includes it, opens
 * `namespace glsl` again and includes one reference header, verbatim, inside it (at global scope `float sin(float)` would
 * collide with <cmath>).  The result is the `_ref` build the restatement (ref_apps.h, ref_lib.h) is compared with bit for bit.
 *
 * Every operation follows the sbx math spec in the conventions of oracle/ovec.h:
 *   dot(a,b) = ((a0*b0 + a1*b1) + a2*b2) (+ a3*b3);  length = sqrt(dot(v,v));  normalize(v) = v / length(v);
 *   mat2/mat3 column-major, m[c][r];  M*v = sum_c col_c * v_c;  v*M = (dot(v,col0), ...);  reflect(I,N) = I - 2 dot(N,I) N.
 *
 * The translation unit that includes this header is compiled with -fsingle-precision-constant, as the reference is
 * (src/Makefile:12).  That flag must not reach oracle/sbx_math_ref.h, whose binary64 constants it would round; so the scalar
 * built-ins are only DECLARED here (sbxm_*) and defined in oracle/glsl_math.cpp, a translation unit compiled without it.
 */
#ifndef SBX_GLSL_ENV_H
#define SBX_GLSL_ENV_H

/* The aux uniforms (cbuffer b1).  In the reference's C++ form they are compile-time constants, `const type name = default`
 * (src/uniform_buffer.h:13); the copy of that header the make rule generates writes `= SBX_REF_AUX_<name>(default)` instead.  Each
 * of these is the default unless the build's command line says otherwise, -D'SBX_REF_AUX_cld_coverage(d)=(0.600000024)': the
 * aux-set builds of oracle/aux_sets.py.  The value stays a constant initialiser (app_clouds.h:15-17 initialises a const
 * thread_local from two of them, once per thread). */
#ifndef SBX_REF_AUX_wind_dir
#define SBX_REF_AUX_wind_dir(d) d
#endif
#ifndef SBX_REF_AUX_sun_dir
#define SBX_REF_AUX_sun_dir(d) d
#endif
#ifndef SBX_REF_AUX_sun_color
#define SBX_REF_AUX_sun_color(d) d
#endif
#ifndef SBX_REF_AUX_sun_power
#define SBX_REF_AUX_sun_power(d) d
#endif
#ifndef SBX_REF_AUX_cld_march_steps
#define SBX_REF_AUX_cld_march_steps(d) d
#endif
#ifndef SBX_REF_AUX_illum_march_steps
#define SBX_REF_AUX_illum_march_steps(d) d
#endif
#ifndef SBX_REF_AUX_sigma_scattering
#define SBX_REF_AUX_sigma_scattering(d) d
#endif
#ifndef SBX_REF_AUX_cld_coverage
#define SBX_REF_AUX_cld_coverage(d) d
#endif
#ifndef SBX_REF_AUX_cld_thick
#define SBX_REF_AUX_cld_thick(d) d
#endif
#ifndef SBX_REF_AUX_atm_radius
#define SBX_REF_AUX_atm_radius(d) d
#endif
#ifndef SBX_REF_AUX_atm_ground_y
#define SBX_REF_AUX_atm_ground_y(d) d
#endif
#ifndef SBX_REF_AUX_fog_density
#define SBX_REF_AUX_fog_density(d) d
#endif
#ifndef SBX_REF_AUX_fog_falloff
#define SBX_REF_AUX_fog_falloff(d) d
#endif

extern "C" {
float sbxm_sin(float), sbxm_cos(float), sbxm_tan(float), sbxm_acos(float), sbxm_exp(float), sbxm_sqrt(float), sbxm_abs(float),
    sbxm_floor(float), sbxm_fract(float), sbxm_radians(float);
float sbxm_pow(float, float), sbxm_atan2(float, float), sbxm_min(float, float), sbxm_max(float, float), sbxm_mod(float, float),
    sbxm_step(float, float);
float sbxm_clamp(float, float, float), sbxm_mix(float, float, float), sbxm_smoothstep(float, float, float);
}

namespace glsl {

struct vec2;
struct vec3;
struct vec4;
/* read-only swizzles: a view of the N floats of the vector they are a union member of */
template <int N, int A, int B> struct sw2 { float v[N]; operator vec2() const; };
template <int N, int A, int B, int C> struct sw3 { float v[N]; operator vec3() const; };
template <int N, int A, int B, int C, int D> struct sw4 { float v[N]; operator vec4() const; };

#define SBX_SW2_ALL(N) \
    sw2<N, 0, 0> xx; sw2<N, 0, 1> xy; sw2<N, 0, 2> xz; sw2<N, 1, 0> yx; sw2<N, 1, 1> yy; sw2<N, 1, 2> yz; \
    sw2<N, 2, 0> zx; sw2<N, 2, 1> zy; sw2<N, 2, 2> zz;
#define SBX_SW3_ROW(N, a, A, b, B) sw3<N, A, B, 0> a##b##x; sw3<N, A, B, 1> a##b##y; sw3<N, A, B, 2> a##b##z;
#define SBX_SW3_COL(N, a, A) SBX_SW3_ROW(N, a, A, x, 0) SBX_SW3_ROW(N, a, A, y, 1) SBX_SW3_ROW(N, a, A, z, 2)
#define SBX_SW3_ALL(N) SBX_SW3_COL(N, x, 0) SBX_SW3_COL(N, y, 1) SBX_SW3_COL(N, z, 2) sw3<N, 0, 1, 2> rgb;

struct vec2 {
    union {
        struct { float x, y; };
        struct { float r, g; };
        float v[2];
        sw2<2, 0, 0> xx; sw2<2, 0, 1> xy; sw2<2, 1, 0> yx; sw2<2, 1, 1> yy;
        sw3<2, 0, 0, 0> xxx; sw3<2, 1, 1, 1> yyy;                         /* snoise, src/app_clouds_best.h:484-498 */
    };
    vec2() : x(0), y(0) {}
    template <class S, class T> vec2(S a, T b) : x((float)a), y((float)b) {}
    explicit vec2(float a) : x(a), y(a) {}
    float& operator[](int i) { return v[i]; }
    const float& operator[](int i) const { return v[i]; }
};
struct vec3 {
    union {
        struct { float x, y, z; };
        struct { float r, g, b; };
        float v[3];
        SBX_SW2_ALL(3)
        SBX_SW3_ALL(3)
        sw4<3, 0, 0, 0, 0> xxxx; sw4<3, 1, 1, 1, 1> yyyy; sw4<3, 2, 2, 2, 2> zzzz;    /* :518-519 */
    };
    vec3() : x(0), y(0), z(0) {}
    template <class S, class T, class U> vec3(S a, T b, U c) : x((float)a), y((float)b), z((float)c) {}
    explicit vec3(float a) : x(a), y(a), z(a) {}
    template <class U> vec3(vec2 p, U c) : x(p.x), y(p.y), z((float)c) {}
    float& operator[](int i) { return v[i]; }
    const float& operator[](int i) const { return v[i]; }
};
struct vec4 {
    union {
        struct { float x, y, z, w; };
        struct { float r, g, b, a; };
        float v[4];
        SBX_SW2_ALL(4)
        SBX_SW3_ALL(4)
        sw2<4, 2, 3> zw; sw3<4, 3, 1, 2> wyz;                                         /* :511,523,535,537 */
        sw4<4, 0, 1, 2, 3> xyzw; sw4<4, 0, 2, 1, 3> xzyw; sw4<4, 0, 0, 1, 1> xxyy; sw4<4, 2, 2, 3, 3> zzww;   /* :531-532 */
    };
    vec4() : x(0), y(0), z(0), w(0) {}
    template <class S, class T, class U, class V> vec4(S a, T b, U c, V d) : x((float)a), y((float)b), z((float)c), w((float)d) {}
    explicit vec4(float a) : x(a), y(a), z(a), w(a) {}
    template <class U> vec4(vec3 p, U d) : x(p.x), y(p.y), z(p.z), w((float)d) {}
    vec4(vec2 p, vec2 q) : x(p.x), y(p.y), z(q.x), w(q.y) {}
    float& operator[](int i) { return v[i]; }
    const float& operator[](int i) const { return v[i]; }
};
template <int N, int A, int B> sw2<N, A, B>::operator vec2() const { return vec2(v[A], v[B]); }
template <int N, int A, int B, int C> sw3<N, A, B, C>::operator vec3() const { return vec3(v[A], v[B], v[C]); }
template <int N, int A, int B, int C, int D> sw4<N, A, B, C, D>::operator vec4() const { return vec4(v[A], v[B], v[C], v[D]); }

/* scalar built-ins: the math spec, through the separately compiled translation unit */
inline float sin(float x) { return sbxm_sin(x); }
inline float cos(float x) { return sbxm_cos(x); }
inline float tan(float x) { return sbxm_tan(x); }
inline float acos(float x) { return sbxm_acos(x); }
inline float atan(float y, float x) { return sbxm_atan2(y, x); }
inline float exp(float x) { return sbxm_exp(x); }
inline float pow(float x, float y) { return sbxm_pow(x, y); }
inline float sqrt(float x) { return sbxm_sqrt(x); }
inline float abs(float x) { return sbxm_abs(x); }
inline float floor(float x) { return sbxm_floor(x); }
inline float fract(float x) { return sbxm_fract(x); }
inline float mod(float x, float y) { return sbxm_mod(x, y); }
inline float min(float a, float b) { return sbxm_min(a, b); }
inline float max(float a, float b) { return sbxm_max(a, b); }
inline float clamp(float x, float lo, float hi) { return sbxm_clamp(x, lo, hi); }
inline float mix(float a, float b, float t) { return sbxm_mix(a, b, t); }
inline float step(float e, float x) { return sbxm_step(e, x); }
inline float smoothstep(float a, float b, float x) { return sbxm_smoothstep(a, b, x); }
inline float radians(float d) { return sbxm_radians(d); }

/* component-wise operators and built-ins of one vector type */
#define SBX_EACH(V, N, expr) { V r; for (int i = 0; i < N; i++) r.v[i] = expr; return r; }
#define SBX_VOPS(V, N) \
    inline V operator+(V a, V b) SBX_EACH(V, N, a.v[i] + b.v[i]) \
    inline V operator-(V a, V b) SBX_EACH(V, N, a.v[i] - b.v[i]) \
    inline V operator*(V a, V b) SBX_EACH(V, N, a.v[i] * b.v[i]) \
    inline V operator/(V a, V b) SBX_EACH(V, N, a.v[i] / b.v[i]) \
    inline V operator+(V a, float s) SBX_EACH(V, N, a.v[i] + s) \
    inline V operator-(V a, float s) SBX_EACH(V, N, a.v[i] - s) \
    inline V operator*(V a, float s) SBX_EACH(V, N, a.v[i] * s) \
    inline V operator/(V a, float s) SBX_EACH(V, N, a.v[i] / s) \
    inline V operator+(float s, V a) SBX_EACH(V, N, s + a.v[i]) \
    inline V operator-(float s, V a) SBX_EACH(V, N, s - a.v[i]) \
    inline V operator*(float s, V a) SBX_EACH(V, N, s * a.v[i]) \
    inline V operator/(float s, V a) SBX_EACH(V, N, s / a.v[i]) \
    inline V operator-(V a) SBX_EACH(V, N, -a.v[i]) \
    inline V& operator+=(V& a, V b) { a = a + b; return a; } \
    inline V& operator-=(V& a, V b) { a = a - b; return a; } \
    inline V& operator*=(V& a, V b) { a = a * b; return a; } \
    inline V& operator/=(V& a, V b) { a = a / b; return a; } \
    inline V& operator+=(V& a, float s) { a = a + s; return a; } \
    inline V& operator-=(V& a, float s) { a = a - s; return a; } \
    inline V& operator*=(V& a, float s) { a = a * s; return a; } \
    inline V& operator/=(V& a, float s) { a = a / s; return a; } \
    inline V abs(V a) SBX_EACH(V, N, sbxm_abs(a.v[i])) \
    inline V floor(V a) SBX_EACH(V, N, sbxm_floor(a.v[i])) \
    inline V fract(V a) SBX_EACH(V, N, sbxm_fract(a.v[i])) \
    inline V sin(V a) SBX_EACH(V, N, sbxm_sin(a.v[i])) \
    inline V cos(V a) SBX_EACH(V, N, sbxm_cos(a.v[i])) \
    inline V exp(V a) SBX_EACH(V, N, sbxm_exp(a.v[i])) \
    inline V sqrt(V a) SBX_EACH(V, N, sbxm_sqrt(a.v[i])) \
    inline V pow(V a, V b) SBX_EACH(V, N, sbxm_pow(a.v[i], b.v[i])) \
    inline V min(V a, V b) SBX_EACH(V, N, sbxm_min(a.v[i], b.v[i])) \
    inline V max(V a, V b) SBX_EACH(V, N, sbxm_max(a.v[i], b.v[i])) \
    inline V min(V a, float b) SBX_EACH(V, N, sbxm_min(a.v[i], b)) \
    inline V max(V a, float b) SBX_EACH(V, N, sbxm_max(a.v[i], b)) \
    inline V mod(V a, float b) SBX_EACH(V, N, sbxm_mod(a.v[i], b)) \
    inline V mod(V a, V b) SBX_EACH(V, N, sbxm_mod(a.v[i], b.v[i])) \
    inline V clamp(V a, float lo, float hi) SBX_EACH(V, N, sbxm_clamp(a.v[i], lo, hi)) \
    inline V mix(V a, V b, float t) SBX_EACH(V, N, sbxm_mix(a.v[i], b.v[i], t)) \
    inline V mix(V a, V b, V t) SBX_EACH(V, N, sbxm_mix(a.v[i], b.v[i], t.v[i])) \
    inline V step(float e, V a) SBX_EACH(V, N, sbxm_step(e, a.v[i])) \
    inline V step(V e, V a) SBX_EACH(V, N, sbxm_step(e.v[i], a.v[i])) \
    inline V smoothstep(float e0, float e1, V a) SBX_EACH(V, N, sbxm_smoothstep(e0, e1, a.v[i]))
SBX_VOPS(vec2, 2)
SBX_VOPS(vec3, 3)
SBX_VOPS(vec4, 4)
#undef SBX_VOPS
#undef SBX_EACH
#undef SBX_SW2_ALL
#undef SBX_SW3_ROW
#undef SBX_SW3_COL
#undef SBX_SW3_ALL

inline float dot(vec2 a, vec2 b) { return a.x * b.x + a.y * b.y; }
inline float dot(vec3 a, vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline float dot(vec4 a, vec4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
inline float length(vec2 a) { return sbxm_sqrt(dot(a, a)); }
inline float length(vec3 a) { return sbxm_sqrt(dot(a, a)); }
inline vec2 normalize(vec2 a) { return a / length(a); }
inline vec3 normalize(vec3 a) { return a / length(a); }
inline vec3 cross(vec3 a, vec3 b) { return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
/* APP_VINYL takes reflect from the environment (src/app_vinyl.h:316); the builds that include src/util_optics.h get the
 * reference's own (:16-22, the same formula), so this one is there only where the build asks for it */
#ifdef SBX_ENV_REFLECT
inline vec3 reflect(vec3 I, vec3 N) { return I - 2.0f * dot(N, I) * N; }
#endif

struct mat2 {
    vec2 c[2]; /* columns */
    mat2() {}
    mat2(vec2 a, vec2 b) { c[0] = a; c[1] = b; }
    mat2(float a0, float a1, float b0, float b1) { c[0] = vec2(a0, a1); c[1] = vec2(b0, b1); }
    vec2& operator[](int i) { return c[i]; }
    const vec2& operator[](int i) const { return c[i]; }
};
inline vec2 operator*(const mat2& m, vec2 v) { return m.c[0] * v.x + m.c[1] * v.y; }
inline vec2 operator*(vec2 v, const mat2& m) { return vec2(dot(v, m.c[0]), dot(v, m.c[1])); }
inline mat2 operator*(const mat2& a, const mat2& b) { return mat2(a * b.c[0], a * b.c[1]); }

struct mat3 {
    vec3 c[3]; /* columns */
    mat3() {}
    mat3(vec3 a, vec3 b, vec3 d) { c[0] = a; c[1] = b; c[2] = d; }
    mat3(float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2) {
        c[0] = vec3(a0, a1, a2); c[1] = vec3(b0, b1, b2); c[2] = vec3(c0, c1, c2);
    }
    vec3& operator[](int i) { return c[i]; }
    const vec3& operator[](int i) const { return c[i]; }
};
inline vec3 operator*(const mat3& m, vec3 v) { return (m.c[0] * v.x + m.c[1] * v.y) + m.c[2] * v.z; }
inline vec3 operator*(vec3 v, const mat3& m) { return vec3(dot(v, m.c[0]), dot(v, m.c[1]), dot(v, m.c[2])); }
inline mat3 operator*(const mat3& a, const mat3& b) { return mat3(a * b.c[0], a * b.c[1], a * b.c[2]); }

/* The 2-D texture of app_2d.h's USE_TEXTURE build (`sampler2D u_tex0("", sampler2D::Repeat); texture(u_tex0, uv)`,
 * src/app_2d.h:7,28).  One RGBA32F image is bound per process (ref_driver.cpp sbxr_set_texture2d; row 0 at v = 0); every
 * sampler reads it.  The filter is the build's texture spec: bilinear, WRAP, texel centres at (i + .5) / size,
 * mix in x then in y. */
struct tex2d_binding { const float* rgba; int width, height; };
extern tex2d_binding g_tex2d;
struct sampler2D {
    enum wrap_mode { Repeat, Clamp };
    sampler2D(const char*, wrap_mode) {}
};
struct tex_axis { int i0, i1; float f; };
inline tex_axis texture_axis(float c, int size) {
    const float fs = (float)size;
    const float u = c * fs - 0.5f;
    const float fl = sbxm_floor(u);
    tex_axis a;
    a.f = u - fl;
    float m = fl - fs * sbxm_floor(fl / fs);
    if (m < 0.0f) m = m + fs;
    if (m >= fs) m = m - fs;
    a.i0 = (m >= 0.0f && m < fs) ? (int)m : 0;          /* inf and NaN coordinates read texel 0 */
    a.i1 = a.i0 + 1 == size ? 0 : a.i0 + 1;
    return a;
}
inline vec4 texture(const sampler2D&, vec2 uv) {
    const tex2d_binding& T = g_tex2d;
    const tex_axis X = texture_axis(uv.x, T.width), Y = texture_axis(uv.y, T.height);
    auto at = [&](int x, int y) { const float* p = T.rgba + ((long)y * T.width + x) * 4; return vec4(p[0], p[1], p[2], p[3]); };
    return mix(mix(at(X.i0, Y.i0), at(X.i1, Y.i0), X.f), mix(at(X.i0, Y.i1), at(X.i1, Y.i1), X.f), Y.f);
}

/* the uniforms, per thread as the reference's own globals are (src/def.h:7) */
extern thread_local vec2 iResolution;
extern thread_local float iGlobalTime;
extern thread_local vec4 iMouse;

} /* namespace glsl */
#endif
