// shaderbox_amd/csrc/sbx_witness.h — fast forms of sqrt / normalize with a RECORDED domain, for kernels that cannot prove the domain.
#pragma once
#include <type_traits>
#include "sbx_frame.h"

namespace sbx {

// WITNESSED SQUARE ROOTS (round 4).  The compiler's IEEE sqrt is 16 VALU instructions (input scaling for tiny arguments, v_sqrt_f32,
// a two-sided one-ulp fix-up, a class test for 0 / inf); sqrt_rs_ (sbx_math.h) is 5 and EQUAL to it for every argument in
// [2^-102, +inf) — all of them were run (profiles/r03_sqrt_rsq_exhaustive.txt) — but returns NaN for 0 and +inf and is inexact
// below 2^-102.  A squared length in an SDF is none of those except ON a primitive's axis or centre, which no kernel can rule out
// for an arbitrary frame.  So a lane RECORDS every argument outside the proved interval (two integer instructions, the flag
// accumulates in an SGPR pair); what a kernel does with the record is `witnessed` below.
// Wit<false> is the plain form (no record), what every caller without a witness gets.
template <bool FAST> struct Wit {
    static constexpr bool fast = FAST;
    bool bad = false;
    unsigned lo = 0x0C800000u;                                   // 2^-102; the test build raises it (witnessed<2>) to exercise the re-run
    __device__ __forceinline__ float sqrt(float x) {
        if (!FAST) return sqrt_(x);
        bad |= (f2u(x) - lo) >= (0x7F800000u - lo);              // 0, tiny, +inf, NaN, negative: all outside [lo, +inf)
        return sqrt_rs_(x);
    }
    __device__ __forceinline__ float length(v2 v) { return sqrt(dot(v, v)); }
    __device__ __forceinline__ float length(v3 v) { return sqrt(dot(v, v)); }
    // normalize(v) = v / length(v) (sbx_vec.h: IEEE root, then three IEEE quotients through one binary64 reciprocal: ~150 issue
    // cycles).  Fast form: sqrt_rs_, v_rcp_f32 + one Newton step, three div3_ (sbx_math.h divn_: EQUAL to the IEEE quotient for
    // every pair of significands, all 2^47 run, wherever nothing under- or overflows and the dividend is not a zero, whose sign
    // div3_ loses) — 22 instructions.  Recorded: a squared length outside [lo, 2^40) and any component whose SQUARE is not a normal
    // number (zero, denormal, NaN).  Without a record: l in [2^-51, 2^20], every |v_i| in [2^-63, l], every quotient in [2^-83, 1],
    // the residual a - q0 l a multiple of 2^-109 that fits 24 bits — all normal, which is the scale-free case the exhaustive run
    // covers.
    __device__ __forceinline__ v3 normalize(v3 v) {
        if (!FAST) return sbx::normalize(v);
        const float xx = v.x * v.x, yy = v.y * v.y, zz = v.z * v.z;
        const float x = (xx + yy) + zz;                          // dot(v, v), operation for operation (sbx_vec.h)
        const float mn = u2f(0x00800000u);                       // 2^-126
        bad |= !(xx >= mn) || !(yy >= mn) || !(zz >= mn);
        bad |= (f2u(x) - lo) >= (0x53800000u - lo);              // [lo, 2^40)
#if defined(__HIP_DEVICE_COMPILE__)
        const float l = sqrt_rs_(x);
        const float r0 = __builtin_amdgcn_rcpf(l);
        const float e = __builtin_fmaf(-l, r0, 1.0f);
        const float r = __builtin_fmaf(e, r0, r0);
        return V3(div3_(v.x, l, r), div3_(v.y, l, r), div3_(v.z, l, r));
#else
        return sbx::normalize(v);
#endif
    }
};

// primary_dir (sbx_frame.h) with the witness's normalisation
template <class W>
__device__ __forceinline__ v3 primary_dir(const Camera& c, v2 pc, W& w) {
    return w.normalize(c.fwd + c.up * pc.y + c.right * pc.x);    // util.h:17
}

// THE PROTOCOL, once, for every kernel that takes the fast roots.  body(w) is a kernel's whole pixel or element with the roots of
// witness `w` (a generic lambda over its pixel function; it may ask `w.fast`).  The wave runs it with the fast forms, and runs it
// AGAIN with the IEEE forms if any lane that counts (`on`) recorded an argument outside the proved interval: a wave-uniform branch,
// never taken on the frames measured.  No branch inside the SDF — a per-lane choice between the forms at each root cost more than it
// saved (sbx_math.h, sqrt_n_) — and the bits are the IEEE forms' either way: without a record every root the wave took is one of the
// exhaustively compared ones, and with one everything the first pass wrote is written again.
//   WIT  0 the IEEE forms only; 1 the protocol; 2 the same with the witness's lower edge at 1.0, so that waves near any primitive's
//        axis DO record and re-run (sbx_set_variant 2: the test of the re-run path)
//   on   false for a lane whose result is not stored (the tail of a ragged wave, which evaluated zeros); a kernel whose idle lanes
//        have returned passes true
// Returns whether the wave re-ran (wave-uniform; the eval kernels count it).
template <int WIT, class Body>
__device__ __forceinline__ bool witnessed(bool on, Body&& body) {
    bool rerun = false;
    if (WIT != 0) {
        Wit<true> w;
        if (WIT == 2) w.lo = 0x3F800000u;
        body(w);
        rerun = __builtin_amdgcn_ballot_w64(on && w.bad) != 0ull;
    }
    if (WIT == 0 || rerun) {
        Wit<false> w0;
        body(w0);
    }
    return rerun;
}

// THE ELEMENT WAVE of the witnessed eval kernels (k_egg_eval, k_vinyl_eval, k_raytracer_eval), between a kernel's own prologue and its end: one lane
// per element, one 64-lane wave per workgroup, a ragged last wave; a lane past n loads nothing, evaluates element zeros harmlessly
// and stores nothing.  element(cull, q, w, r) is one element — std::true_type / std::false_type for the field's CULL, q its WIN
// inputs, w the witness, r its WOUT outputs.
//   THE FORM OF A WAVE.  The frame kernels' culls and shortcuts are proved for finite frame constants and points of bounded scale.
//     The frame is the host's to judge: PLAIN (an untame block, sbx_set_variant 1) is the reference form — CULL false, IEEE roots —
//     for every wave.  The elements are the wave's to judge: it takes the culled form only if the first WPOS inputs (the
//     coordinates) of every committing lane are within 1e4 in magnitude, NaN failing; each kernel's head says what that bound buys
//     its marches.  Any other wave takes the plain form for all of its lanes.  Per wave, not per lane: one predicate, one branch,
//     no divergent copies.
//   THE WITNESS RE-RUN of a culled wave is `witnessed` over the committing lanes (still culled: no cull depends on the roots).
//   LOADS AND STORES.  `in` and `out` need only 4-byte alignment, so an element is read and written as dwords: lane i reads
//     in[WIN i + k], k < WIN.  A wave's WIN loads together cover 64 WIN contiguous floats — every cache line fetched is fully
//     used — and at 12-40 B per element against a march of tens of steps the traffic is noise beside the arithmetic
//     (profiles/egg_eval_timing.txt).  A staged, vectorised copy through LDS would need the alignment the contract does not give.
//   counts: NULL, or two zeroed words that receive the culled waves that did not / did re-run.
//   CAP: the capacity of q and r in dwords, ELEM_WORDS unless a kernel's widest element needs more (k_raytracer_eval's "illuminate": 10).
constexpr int ELEM_WORDS = 8;                                    // the default capacity of q and r
template <int WIN, int WPOS, int WOUT, bool PLAIN, int WIT, int CAP = ELEM_WORDS, class Element>
__device__ __forceinline__ void witnessed_elements(const float* __restrict__ in, float* __restrict__ out, size_t n,
                                                   unsigned* __restrict__ counts, Element&& element) {
    static_assert(WPOS <= WIN && WIN <= CAP && WOUT <= CAP, "an element is at most CAP dwords in and out");
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool on = i < n;
    float q[CAP] = {};
    if (on) {
#pragma unroll
        for (int k = 0; k < WIN; ++k) q[k] = in[(size_t)WIN * i + k];
    }
    float r[CAP] = {};
    bool tame = true;
#pragma unroll
    for (int k = 0; k < WPOS; ++k) tame = tame && abs_(q[k]) <= 1e4f;                     // a NaN compares false
    const bool culled = !PLAIN && __builtin_amdgcn_ballot_w64(on && !tame) == 0ull;      // wave-uniform
    bool rerun = false;
    if (culled) {
        rerun = witnessed<WIT>(on, [&](auto& w) { element(std::true_type{}, q, w, r); });
    } else {
        Wit<false> w0;
        element(std::false_type{}, q, w0, r);
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < WOUT; ++k) out[(size_t)WOUT * i + k] = r[k];
    }
    if (counts && (threadIdx.x & 63) == 0 && culled && WIT != 0) atomicAdd(counts + (rerun ? 1 : 0), 1u);
}

// THE HOST'S HALF: from the variant of a launch (sbx_ctx.h witness_variant: sbx_set_variant's value, 1 where the host judged the
// frame untame) to the instantiation, once:
//     variant         CULL    WIT
//     1               false   0              the reference form
//     2               true    2              the witness's test edge
//     3               true    0              the IEEE roots
//     anything else   true    WIT_DEFAULT    the launcher's *_WITNESS switch: what ships
// launch(cull, wit) receives them as std::integral_constant values.  A kernel with nothing to cull ignores `cull` (1 and 3 are then
// one kernel); the eval kernels' PLAIN is !CULL.
template <int WIT_DEFAULT, class Launch>
inline void witness_dispatch(int variant, Launch&& launch) {
    if (variant == 1) launch(std::false_type{}, std::integral_constant<int, 0>{});
    else if (variant == 2) launch(std::true_type{}, std::integral_constant<int, 2>{});
    else if (variant == 3) launch(std::true_type{}, std::integral_constant<int, 0>{});
    else launch(std::true_type{}, std::integral_constant<int, WIT_DEFAULT>{});
}

}  // namespace sbx
