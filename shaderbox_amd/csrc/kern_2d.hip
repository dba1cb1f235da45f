// shaderbox_amd/csrc/kern_2d.hip — the tunnel / road UV demo src/app_2d.h (SBX_APP_2D, and SBX_APP_2D_TEX = its USE_TEXTURE build).
//
// Follows /root/reference/src/app_2d.h: mainImage :70-111, perturb_tunnel :49-62, perturb_road :37-47, tent_filter :64-68,
// sample() :22-35 (checkboard_pattern(uv, 2.), src/util.h:95-101, or the t0 texture hlsltoy binds, util/hlsltoy/src/hlsltoy.cpp:66-87,
// 217-223, 242-249, 434-437).  Math spec of DESIGN.md §3: binary32 in written order, never contracted; atan is atan2_ (binary64),
// mod / mix / floor / max are the GLSL forms of sbx_math.h, PI the binary32 value of 3.14159265359 (src/def.h:51).
//
// The phase of t = mod(u_time, 16) and its mix weight depend on the uniforms only: the host decides them once per frame
// (build_2d, sbx_frames.hip) and launches the kernel of that phase, so the road phase carries no atan2 and the undefined phase
// (t = 4, 8, 12 or NaN: no branch of :82-103 runs, `color` is uninitialised; the port writes (0, 0, 0, 0) times the tent) no
// sample at all.  NaN and Inf flow through as data (the r = 0 pixel of an odd frame size, points far outside the frame).
//
// MI355X shape: the only app here whose frame is not VALU-bound by a wide margin — 16 bytes per pixel against one binary64 atan2,
// one square root and three divisions in the tunnel phases, none of those in the road phase.  One thread per pixel, 64 x 1 wave
// tiles (one 1 KB run of float4 stores per wave), frame constants in kernel arguments (DESIGN.md §5.8 has the times).
#include "sbx_device.h"

namespace sbx {

// perturb_tunnel (:49-62); d = r
__device__ __forceinline__ v2 perturb_tunnel(float ux, float uy, float time, double rpi, float& r) {
    const float px = 2.f * ux - 1.f, py = 2.f * uy - 1.f;
    r = sqrt_(px * px + py * py);
    const float a = atan2_(py, px) + time;
    const float s = 1.f / r + time;
    const float t = 4.f * div_by(a, rpi);                          // 4. * (a / PI); a / PI through the binary64 reciprocal is the IEEE quotient
    return V2(s, t);
}
// perturb_road (:37-47)
__device__ __forceinline__ v2 perturb_road(float ux, float uy, float time) {
    const float px = 2.f * ux - 1.f, py = 2.f * uy - 1.f;
    const float ay = abs_(py);
    const float s = px / ay;
    const float t = 1.f / ay;
    return V2(s, t - time);
}

// the spec's WRAP on one axis of the t0 texture (DESIGN.md §3 "SampleLevel", kern_clouds_tex.hip tex_axis): u = c * size - .5,
// i = floor(u), f = u - i, i - size * floor(i / size) folded once into [0, size), NaN / Inf / |i| beyond 2^24 -> whatever that
// gives, and anything outside [0, size) -> texel 0: every coordinate reads inside the texture
__device__ __forceinline__ void tex2_axis(float c, int size, float fsize, double rsize, int& i0, int& i1, float& f) {
    const float u = c * fsize - .5f;
    const float fl = floor_(u);
    f = u - fl;
    float m = fl - fsize * floor_(div_by(fl, rsize));
    if (m < 0.f) m += fsize;
    if (m >= fsize) m -= fsize;
    const int i = (m >= 0.f && m < fsize) ? (int)m : 0;
    i0 = i;
    i1 = (i + 1 == size) ? 0 : i + 1;
}
__device__ __forceinline__ float4 mix4(float4 a, float4 b, float w) {
    return make_float4(mix_(a.x, b.x, w), mix_(a.y, b.y, w), mix_(a.z, b.z, w), mix_(a.w, b.w, w));
}
// sample() (:22-35)
template <bool TEX>
__device__ __forceinline__ float4 sample_2d(const Frame2d& F, v2 st) {
    if (TEX) {                                                     // u_tex0.Sample(u_sampler0, uv): bilinear, WRAP, mix in x then in y
        int x0, x1, y0, y1;
        float fx, fy;
        tex2_axis(st.x, F.tw, F.ftw, F.rtw, x0, x1, fx);
        tex2_axis(st.y, F.th, F.fth, F.rth, y0, y1, fy);
        const float4* r0 = F.tex + (size_t)y0 * F.tw;
        const float4* r1 = F.tex + (size_t)y1 * F.tw;
        return mix4(mix4(r0[x0], r0[x1], fx), mix4(r1[x0], r1[x1], fx), fy);
    }
    const float cb = mod_(floor_(st.x * 2.f) + floor_(st.y * 2.f), 2.f);     // checkboard_pattern(uv, 2.), util.h:95-101
    return make_float4(cb, cb, cb, 1.f);
}
__device__ __forceinline__ float4 scale4(float4 c, float k) { return make_float4(c.x * k, c.y * k, c.z * k, c.w * k); }

template <int PHASE, bool TEX>
__global__ void __launch_bounds__(WG_THREADS) k_2d(Frame2d F, RowMap M, float* __restrict__ out) {
    const Pixel px = pixel_of_thread<64>(M);
    if (!px.valid) return;
    const float ux = div_by(px.fx, F.rres_x), uy = div_by(px.fy, F.rres_y);     // uv = fragCoord / u_res.xy   :72
    float4 color;
    if (PHASE == 0) {                                              // t < 4                 :82-86
        float d;
        const v2 st = perturb_tunnel(ux, uy, F.time, F.rpi, d);
        color = scale4(sample_2d<TEX>(F, st), d);
    } else if (PHASE == 1 || PHASE == 3) {                         // 4 < t < 8, t > 12    :88-93, :99-104
        float d;
        const v2 st = perturb_tunnel(ux, uy, F.time, F.rpi, d);
        const v2 st2 = perturb_road(ux, uy, F.time);
        const v2 a = PHASE == 1 ? st : st2, b = PHASE == 1 ? st2 : st;
        const v2 m = V2(a.x * F.omw + b.x * F.w, a.y * F.omw + b.y * F.w);   // mix(a, b, w) = a (1 - w) + b w
        color = scale4(sample_2d<TEX>(F, m), d);
    } else if (PHASE == 2) {                                       // 8 < t < 12            :94-97
        color = sample_2d<TEX>(F, perturb_road(ux, uy, F.time));
    } else {                                                       // no branch ran: the port's (0, 0, 0, 0)
        color = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float g = 1.f - fmax_(1.f - abs_(2.f * uy - 1.f), 0.f);     // 1. - tent_filter(2.*uv.y - 1.)   :64-68,106
    store_rgba4(M, out, px.idx, scale4(color, g));                 // fragColor = color   :110
}

template <bool TEX>
static void launch_2d_phase(const Frame2d& F, const RowMap& M, float* out, hipStream_t s) {
    const dim3 g = grid_for<64>(M), b(WG_THREADS);
    switch (F.phase) {
    case 0: hipLaunchKernelGGL((k_2d<0, TEX>), g, b, 0, s, F, M, out); break;
    case 1: hipLaunchKernelGGL((k_2d<1, TEX>), g, b, 0, s, F, M, out); break;
    case 2: hipLaunchKernelGGL((k_2d<2, TEX>), g, b, 0, s, F, M, out); break;
    case 3: hipLaunchKernelGGL((k_2d<3, TEX>), g, b, 0, s, F, M, out); break;
    default: hipLaunchKernelGGL((k_2d<4, false>), g, b, 0, s, F, M, out); break;
    }
}
bool launch_2d(const Frame2d& F, const RowMap& M, float* out, hipStream_t s, bool tex) {
    if (M.rgb == 1 || M.rgb == 3) return false;                    // three-channel outputs: refused by the entry points already
    if (tex) launch_2d_phase<true>(F, M, out, s);
    else launch_2d_phase<false>(F, M, out, s);
    return true;
}

// sbx_set_texture2d: R8G8B8A8_UNORM words -> the context's RGBA32F copy, c / 255 correctly rounded per channel (the UNORM decode)
__global__ void __launch_bounds__(256) k_unorm8_to_float4(const unsigned* __restrict__ in, float4* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned w = in[i];
    out[i] = make_float4((float)(w & 255u) / 255.f, (float)((w >> 8) & 255u) / 255.f, (float)((w >> 16) & 255u) / 255.f,
                         (float)(w >> 24) / 255.f);
}
void launch_unorm8_to_float4(const unsigned* in, float4* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_unorm8_to_float4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
}

}  // namespace sbx
