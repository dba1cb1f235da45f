// shaderbox_amd/csrc/sbx_worley.h — the Worley noise of src/noise_worley.h as device functions, shared by the noise library
// (kern_noise.hip) and APP_FUNC (kern_func.hip, whose hash table is built with this same hash_w).
//
// hash_w (/root/reference/src/noise_worley.h:5-17), noise_w (:20-51) and worley_fbm, the combination src/app_func.h:17-47 makes of
// nine noise_w calls over six distinct periods.  hash_w multiplies sin by 43758.5453123, so only the shared correctly rounded sin
// gives parity.
#pragma once
#include "sbx_vec.h"

namespace sbx {

__device__ __forceinline__ v3 hash_w(v3 x) {                               // noise_worley.h:5-17
    const v3 xx = V3(dot(x, V3(127.1f, 311.7f, 74.7f)), dot(x, V3(269.5f, 183.3f, 246.1f)),
                     dot(x, V3(113.5f, 271.9f, 124.6f)));
    return V3(fract_(sin_(xx.x) * 43758.5453123f), fract_(sin_(xx.y) * 43758.5453123f),
              fract_(sin_(xx.z) * 43758.5453123f));
}

// closest, second closest, |cell id| over the 27 neighbour cells, domain repeating every `rep`  :20-51
__device__ __forceinline__ v3 noise_w(v3 pos, float rep) {
    const v3 x = pos * rep;
    const v3 p = V3(floor_(x.x), floor_(x.y), floor_(x.z));
    const v3 f = V3(x.x - p.x, x.y - p.y, x.z - p.z);
    float id = 0.0f, r0 = 100.0f, r1 = 100.0f;
    for (int k = -1; k <= 1; k++)
        for (int j = -1; j <= 1; j++)
            for (int i = -1; i <= 1; i++) {
                const v3 b = V3((float)i, (float)j, (float)k);
                const v3 pb = p + b;
                const v3 r = b - f + hash_w(V3(mod_(pb.x, rep), mod_(pb.y, rep), mod_(pb.z, rep)));
                const float d = dot(r, r);
                if (d < r0) {
                    id = dot(p + b, V3(1.0f, 57.0f, 113.0f));
                    r1 = r0;
                    r0 = d;
                } else if (d < r1) {
                    r1 = d;
                }
            }
    return V3(sqrt_(r0), sqrt_(r1), abs_(id));
}

// app_func.h's worley_fbm (:41-47) over worley_tex_left / _middle / _right (:17-39), given w(L) = 1 - (noise_w(pos, L).r + .015)
// for the six distinct periods L = 4, 8, 16, 24, 32, 64 (w4 .. w64): every sum and product in the written order
__device__ __forceinline__ float worley_fbm_of(float w4, float w8, float w16, float w24, float w32, float w64) {
    const float left = w4 * .625f + w8 * .25f + w16 * .125f;                // :17-23
    const float middle = w8 * .625f + w16 * .25f + w32 * .125f;             // :25-31
    const float right = w24 * .625f + w32 * .25f + w64 * .125f;             // :33-39
    return left * .625f + middle * .25f + right * .125f;                    // :41-47
}
__device__ __forceinline__ float worley_w(v3 pos, float L) { return 1.f - (noise_w(pos, L).x + .015f); }
__device__ __forceinline__ float worley_fbm(v3 pos) {
    return worley_fbm_of(worley_w(pos, 4.f), worley_w(pos, 8.f), worley_w(pos, 16.f), worley_w(pos, 24.f), worley_w(pos, 32.f),
                         worley_w(pos, 64.f));
}

}  // namespace sbx
