// vr_math_probe.h -- TEST HOOK: one numbered entry per function of vr_math.h, for the device probe kernels (vr_probe.hip) and for the host build of
// the same header (tests/hostkernel/math_host.cpp).  No render includes this file.
//
// r = f(x, y).  Integer arguments travel as the BIT PATTERN of a float operand ("bits(y)"), integer results as the bit pattern of the returned float, so
// that no entry converts an unchecked float to an integer.  Codes (the tests' CPU reference states the same table independently, in C):
//    0 log_  1 sin_  2 cos_  3 tan_  4 acos_  5 atan2_(x, y)  6 exp_  7 pow_(x, y)  8 asin_  9 x / y  10 sqrt_  11 fma_(x, y, x)  12 float(u8) / 255
//   13 sincos_: s * y + c  14 x * y + x (two roundings)  15 half2float(bits(x))  16 rcp_exact  17 rcp3_exact((x, y, x)).y (vr_probe.hip only)
//   18 sincos_: s   19 sincos_: c   20 neg_log_1m   21 log_unit_
//   22 floor2i -> int   23 voxel_index(x, bits(y)) -> int   24 round_mip -> int   25 round_mip_q(bits(x)) -> int   26 round_half_even -> int
//   27 scale2(x, bits(y))   28 sanitize   29 min_(x, y)   30 max_(x, y)   31 clamp_(x, y, 1)   32 clamp_(x, 0, y)
//   33 float_to_half_rne -> int   34 float_to_half_down -> int   35 float_to_half_up -> int   36 mul24(bits(x), bits(y)) -> int   37 unorm8(bits(x) & 255)
// Domains are the functions' own (vr_math.h): 24 and 25 take q = 4 * mip in 0..12, 26 takes |x| < 2^30, 36 takes operands below 2^24 whose product fits 32 bits.
#pragma once

#include "vr_math.h"

namespace vr {

constexpr int32_t kMathProbeCodes = 38;

VR_HD float math_probe_eval(int32_t fn, float x, float y) {
    float r;
    switch (fn) {
    case 0: r = log_(x); break;
    case 1: r = sin_(x); break;
    case 2: r = cos_(x); break;
    case 3: r = tan_(x); break;
    case 4: r = acos_(x); break;
    case 5: r = atan2_(x, y); break;
    case 6: r = exp_(x); break;
    case 7: r = pow_(x, y); break;
    case 8: r = asin_(x); break;
    case 9: r = x / y; break;
    case 10: r = sqrt_(x); break;
    case 11: r = fma_(x, y, x); break;
    case 12: r = (float)((uint32_t)x & 255u) / 255.0f; break;
    case 13: { float s, c; sincos_(x, s, c); r = s * y + c; break; }
    case 14: r = x * y + x; break;     // must stay two roundings (-ffp-contract=off)
    case 15: r = half2float(f2u(x)); break;     // bit pattern of x: low 16 bits = binary16
    case 16: r = rcp_exact(x); break;
    case 18: { float s, c; sincos_(x, s, c); r = s; break; }
    case 19: { float s, c; sincos_(x, s, c); r = c; break; }
    case 20: r = neg_log_1m(x); break;
    case 21: r = log_unit_(x); break;
    case 22: r = u2f((uint32_t)floor2i(x)); break;
    case 23: r = u2f((uint32_t)voxel_index(x, (int32_t)f2u(y))); break;
    case 24: r = u2f((uint32_t)round_mip(x)); break;
    case 25: r = u2f((uint32_t)round_mip_q((int32_t)f2u(x))); break;
    case 26: r = u2f((uint32_t)round_half_even(x)); break;
    case 27: r = scale2(x, (int)(int32_t)f2u(y)); break;
    case 28: r = sanitize(x); break;
    case 29: r = min_(x, y); break;
    case 30: r = max_(x, y); break;
    case 31: r = clamp_(x, y, 1.0f); break;
    case 32: r = clamp_(x, 0.0f, y); break;
    case 33: r = u2f(float_to_half_rne(x)); break;
    case 34: r = u2f(float_to_half_down(x)); break;
    case 35: r = u2f(float_to_half_up(x)); break;
    case 36: r = u2f(mul24(f2u(x), f2u(y))); break;
    case 37: r = unorm8(f2u(x) & 255u); break;
    default: r = nan_(); break;
    }
    return r;
}

}  // namespace vr
