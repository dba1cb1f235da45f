// shaderbox_amd/csrc/kern_func.hip — the tiled Worley fBm of src/app_func.h (SBX_APP_FUNC), its compiled `#if 1 // 2D` branch.
//
// Follows /root/reference/src/app_func.h: mainImage :63-111 (t = (fragCoord + .5) / u_res :72, no y flip outside HLSL :73-75,
// pos = (t, 0) :80, n = worley_fbm(pos) :81-83, fragColor = (n, n, n, 1) :110), worley_fbm and its three taps :17-47 over
// noise_w (src/noise_worley.h:20-51; sbx_worley.h).  Math spec of DESIGN.md §3: binary32 in written order, never contracted; mod
// is GLSL's x - y floor(x / y).  The shader writes its own fragColor, so there is no sRGB epilogue, and its alpha is 1.
//
// Where the time goes: worley_fbm makes nine noise_w calls over six distinct periods L, each 27 hash_w of three binary64 sin.
// Every hash_w argument is an integer cell mod L, and with pos.z = 0 the z cell is one of mod(-1, 0, 1; L) = L - 1, 0, 1: all
// 18 096 hashes the frame can need are in a table built once per context (k_func_table below, with this same hash_w), and the
// default kernel reads them instead of evaluating them.
//
//   * Per period it computes mod_(p + b, L) per axis exactly as noise_w does (three values per axis: the same operations on the
//     same operands, hoisted out of the 27-cell loop).  If all six are integers in [0, L) every cell is in the table: the hash is
//     the table's entry, the bits hash_w gives for that cell.  Otherwise (NaN, Inf, and |t L| so large that mod_'s quotient
//     rounds out of [0, L)) the lane runs noise_w itself.  Exact on every input; no domain proof is needed.
//   * Only F1 is tracked: F2 and the cell id of noise_w are unused by app_func.h (the minimum under d < r0 does not depend on the
//     visiting order, and a NaN d never replaces it).
//   * Every lane reads its 27 hashes with vector loads.  Reading them once per wave through uniform loads where the wave's
//     cells agree was measured no faster: the kernel is not bound by its loads.
//
// The plain kernel (sbx_set_variant 1) is worley_fbm of sbx_worley.h per pixel: hash_w in place for every cell, no table.
#include "sbx_device.h"
#include "sbx_worley.h"

namespace sbx {

// table layout: the periods in order 4, 8, 16, 24, 32, 64, each L * L * 3 float4 (hash_w in .xyz, .w = 0); inside a period the
// cell (x, y, z) sits at ((kz * L) + y) * L + x, kz = 0, 1, 2 for the z cells mod(-1, L) = L - 1, mod(0, L) = 0, mod(1, L) = 1
constexpr int FN_PERIODS = 6;
constexpr int FUNC_TABLE_CELLS = 3 * (4 * 4 + 8 * 8 + 16 * 16 + 24 * 24 + 32 * 32 + 64 * 64);      // 18 096 (289 536 bytes)
__host__ __device__ constexpr int fn_period(int l) { return l == 0 ? 4 : l == 1 ? 8 : l == 2 ? 16 : l == 3 ? 24 : l == 4 ? 32 : 64; }

// one thread per table cell, the same hash_w on the same operands as noise_w: the z cell is mod_(0 + (kz - 1), L) as noise_w
// computes it for pos.z = 0 (p.z = floor(0 * L) = 0, and 0 + b.z = b.z exactly)
__global__ void __launch_bounds__(256) k_func_table(float4* __restrict__ tab) {
    int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c >= FUNC_TABLE_CELLS) return;
    float4* const out = tab + c;
    int l = 0;
    while (c >= 3 * fn_period(l) * fn_period(l)) { c -= 3 * fn_period(l) * fn_period(l); ++l; }
    const int L = fn_period(l);
    const int x = c % L, y = (c / L) % L, kz = c / (L * L);
    const float fL = (float)L;
    const v3 h = hash_w(V3((float)x, (float)y, mod_((float)(kz - 1), fL)));
    *out = make_float4(h.x, h.y, h.z, 0.f);
}

// mod_(p + b, L) for b = -1, 0, 1 on one axis, and whether all three are table indices (integers in [0, L); NaN fails every test)
__device__ __forceinline__ bool fn_axis(float p, float L, float m[3], int idx[3]) {
    bool ok = true;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        m[b] = mod_(p + (float)(b - 1), L);
        ok = ok && m[b] >= 0.f && m[b] < L && m[b] == floor_(m[b]);
        idx[b] = (int)(m[b] >= 0.f && m[b] < L ? m[b] : 0.f);         // (in range whatever ok says: never an out-of-table address)
    }
    return ok;
}

// sqrt F1 of noise_w((tx, ty, 0), L), hashes from the table
__device__ __forceinline__ float fn_f1(float tx, float ty, int l, const float4* __restrict__ tab) {
    const int Li = fn_period(l);
    const float L = (float)Li;
    const v3 x = V3(tx, ty, 0.f) * L;                                          // noise_worley.h:22-24
    const v3 p = V3(floor_(x.x), floor_(x.y), floor_(x.z));
    const v3 f = V3(x.x - p.x, x.y - p.y, x.z - p.z);
    float mx[3], my[3];
    int ix[3], iy[3];
    const bool okx = fn_axis(p.x, L, mx, ix), oky = fn_axis(p.y, L, my, iy);
    if (!(okx && oky)) return noise_w(V3(tx, ty, 0.f), L).x;                 // a cell outside the table: hash_w in place
    int off = 0;
    for (int q = 0; q < l; ++q) off += 3 * fn_period(q) * fn_period(q);
    const float4* const T = tab + off;
    float r0 = 100.f;
#pragma unroll
    for (int k = -1; k <= 1; k++)
#pragma unroll
        for (int j = -1; j <= 1; j++)
#pragma unroll
            for (int i = -1; i <= 1; i++) {
                const float4 h = T[((k + 1) * Li + iy[j + 1]) * Li + ix[i + 1]];
                const v3 b = V3((float)i, (float)j, (float)k);
                const v3 r = b - f + V3(h.x, h.y, h.z);
                const float d = dot(r, r);
                if (d < r0) r0 = d;
            }
    return sqrt_(r0);
}

// TABLE false: the plain kernel (worley_fbm of sbx_worley.h, hash_w in place); true: the default, hashes from the table
template <bool TABLE>
__global__ void __launch_bounds__(WG_THREADS) k_func(FrameFunc F, RowMap M, float* __restrict__ out) {
    const Pixel px = pixel_of_thread<8>(M);
    if (!px.valid) return;
    const float tx = (px.fx + .5f) / F.res_x, ty = (px.fy + .5f) / F.res_y;   // :72
    float n;
    if (!TABLE) {
        n = worley_fbm(V3(tx, ty, 0.f));                                      // :80-83
    } else {
        // one copy of the period's code, not six (its table-miss path is a whole noise_w): the loop stays rolled, and the six
        // values land in named registers through selects rather than a dynamically indexed (scratch) array
        float w4 = 0.f, w8 = 0.f, w16 = 0.f, w24 = 0.f, w32 = 0.f, w64 = 0.f;
#pragma unroll 1
        for (int l = 0; l < FN_PERIODS; ++l) {
            const float w = 1.f - (fn_f1(tx, ty, l, F.tab) + .015f);   // 1. - (noise_w(pos, L).r + .015)  :19-37
            w4 = l == 0 ? w : w4; w8 = l == 1 ? w : w8; w16 = l == 2 ? w : w16;
            w24 = l == 3 ? w : w24; w32 = l == 4 ? w : w32; w64 = l == 5 ? w : w64;
        }
        n = worley_fbm_of(w4, w8, w16, w24, w32, w64);
    }
    store_rgba(M, out, px.idx, V3(n, n, n));                                  // fragColor = vec4(col, 1)   :110
}

void launch_func_table(float4* tab, hipStream_t s) {
    hipLaunchKernelGGL(k_func_table, dim3((FUNC_TABLE_CELLS + 255) / 256), dim3(256), 0, s, tab);
}
size_t func_table_bytes() { return (size_t)FUNC_TABLE_CELLS * sizeof(float4); }

void launch_func(const FrameFunc& F, const RowMap& M, float* out, hipStream_t s, int variant) {
    const dim3 g = grid_for<8>(M), b(WG_THREADS);
    if (variant == 1) hipLaunchKernelGGL(k_func<false>, g, b, 0, s, F, M, out);
    else hipLaunchKernelGGL(k_func<true>, g, b, 0, s, F, M, out);
}

}  // namespace sbx
