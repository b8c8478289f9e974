// env_pack.h -- the compact (RGBE) form of an environment map: host helper shared by Environment::build and the CPU test harness.
//
// A texel whose three components are m_c * 2^(e - 136) with 8-bit integers m_c and one shared e in [10, 255] -- every texel of a Radiance file is; e >= 10
// keeps the scale a normal float -- packs into one dword r | g << 8 | b << 16 | e << 24 that env_texture (vr_trace.h) decodes to the same three floats
// exactly; a black texel packs to 0.  One texel that is not such a number -- a negative or -0.0 component, inf, NaN, a mantissa that needs more than 8 bits
// under the shared exponent, an exponent outside [10, 255] -- and the map keeps its float form only.
#pragma once

#include <stdint.h>

#include <cmath>
#include <cstddef>
#include <vector>

namespace vr {

// one texel; false: it has no compact form (q is unspecified then)
inline bool pack_rgbe_texel(const float c[3], uint32_t& q) {
    const float mx = std::fmax(c[0], std::fmax(c[1], c[2]));
    if (!(c[0] >= 0.0f && c[1] >= 0.0f && c[2] >= 0.0f) || std::signbit(c[0]) || std::signbit(c[1]) || std::signbit(c[2]) || !std::isfinite(mx)) return false;
    if (mx == 0.0f) { q = 0u; return true; }
    int k = 0;
    (void)std::frexp(mx, &k);                                   // mx = f * 2^k, f in [0.5, 1): its mantissa as an integer below 256 needs the scale 2^(k - 8)
    const int e = k - 8 + 136;
    if (e < 10 || e > 255) return false;
    const float scale = std::ldexp(1.0f, e - 136);
    q = (uint32_t)e << 24;
    for (int j = 0; j < 3; ++j) {
        const float m = c[j] / scale;                            // exact: a power of two
        const uint32_t mi = (uint32_t)m;
        if (m != (float)mi || mi > 255u || (float)mi * scale != c[j]) return false;
        q |= mi << (8 * j);
    }
    return true;
}

// a whole map of `stride` floats per texel; false (packed unspecified): the map keeps its float form
inline bool pack_rgbe_map(const float* tex, size_t n_texels, int stride, std::vector<uint32_t>& packed) {
    packed.resize(n_texels);
    for (size_t i = 0; i < n_texels; ++i)
        if (!pack_rgbe_texel(tex + (size_t)stride * i, packed[i])) return false;
    return true;
}

}  // namespace vr
