/* oracle/glsl_math.cpp — the scalar built-ins of oracle/glsl_env.h: the sbx math spec (sbx_math_ref.h), behind C functions.
 *
 * TEST INFRASTRUCTURE ONLY (see oracle/README.md).
 *
 * A translation unit of its own because the `_ref` builds compile the reference's headers with -fsingle-precision-constant
 * (src/Makefile:12), and under that flag the binary64 constants of sbx_math_ref.h would be rounded to binary32: sin, exp and
 * pow would then differ from the oracle's by an ulp on a third of their arguments.  This file is compiled WITHOUT the flag.
 */
#include "sbx_math_ref.h"

using namespace sbxref;

extern "C" {
float sbxm_sin(float a) { return m_sin(a); }
float sbxm_cos(float a) { return m_cos(a); }
float sbxm_tan(float a) { return m_tan(a); }
float sbxm_acos(float a) { return m_acos(a); }
float sbxm_exp(float a) { return m_exp(a); }
float sbxm_sqrt(float a) { return m_sqrt(a); }
float sbxm_abs(float a) { return m_abs(a); }
float sbxm_floor(float a) { return m_floor(a); }
float sbxm_fract(float a) { return m_fract(a); }
float sbxm_radians(float a) { return m_radians(a); }
float sbxm_pow(float a, float b) { return m_pow(a, b); }
float sbxm_atan2(float a, float b) { return m_atan2(a, b); }
float sbxm_min(float a, float b) { return m_min(a, b); }
float sbxm_max(float a, float b) { return m_max(a, b); }
float sbxm_mod(float a, float b) { return m_mod(a, b); }
float sbxm_step(float a, float b) { return m_step(a, b); }
float sbxm_clamp(float a, float b, float c) { return m_clamp(a, b, c); }
float sbxm_mix(float a, float b, float c) { return m_mix(a, b, c); }
float sbxm_smoothstep(float a, float b, float c) { return m_smoothstep(a, b, c); }
}
