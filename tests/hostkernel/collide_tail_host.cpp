// tests/hostkernel/collide_tail_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// collide_finish of volren_amd/csrc/vr_trace.h -- the function the HIP kernels run at a tentative collision -- compiled for the host in BOTH of its orders: the
// reference's (EARLY = false: draw, decide, draw again where the outcome asks for it) and the one the hot pair of some kernel instances runs (EARLY = true: both LCG
// advances, the second draw's neg_log_1m and the shortcut's premises first, the outcome committed afterwards).  tests/test_collide_tail_host.py calls both on
// crafted states of camera and shadow segments of the DDA trackers, with and without a transfer function, and compares every field of Hot they may touch.
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../volren_amd/csrc/vr_trace.h"

using namespace vr;

namespace {
struct ColdHost {
    float v[C_COUNT];
    float ld(int32_t f) const { return v[f]; }
    void st(int32_t f, float x) { v[f] = x; }
};
constexpr int kIn = 9, kOut = 10;
template <class K, bool EARLY>
void run(const uint32_t* in, uint32_t* out) {
    // the transfer function: ONE entry, looked up at density 0 -- rgba = the entry exactly (mix with weight 0), so the collision's density is vol_majorant * alpha
    const float lut[4] = { 0.25f, 0.5f, 0.75f, u2f(in[4]) };
    SceneParams P{};
    P.u.vol_majorant = u2f(in[2]);
    P.u.vol_inv_majorant = 1.0f;
    P.u.vol_density_scale = 1.0f;
    P.u.tf_window_left = 0.0f;
    P.u.tf_window_width = 1.0f;
    P.u.tf_size = 1;
    Hot h{};
    h.seed = in[0];
    h.majorant = u2f(in[1]);
    h.Tr = u2f(in[3]);
    h.shadow = (int32_t)in[5];
    h.mipq = (int32_t)in[6];
    h.tau = u2f(in[7]);
    h.t = u2f(in[8]);
    h.state = ST_COLLIDE;
    h.far = 1.0f;
    CollideIO<K> io{};
    io.a.in = true;                     // no transfer function: the tap's value rmin + unorm8(0) * 0 = the density given
    io.d.rmin = u2f(in[4]);
    ColdHost c{};
    for (int i = 0; i < 3; ++i) c.v[C_COL + i] = -1.0f;
    collide_finish<K, ColdHost, false, EARLY>(h, c, P, io, lut);
    out[0] = (uint32_t)h.state; out[1] = h.seed; out[2] = f2u(h.tau); out[3] = f2u(h.t); out[4] = f2u(h.Tr); out[5] = (uint32_t)h.mipq; out[6] = f2u(h.majorant);
    for (int i = 0; i < 3; ++i) out[7 + i] = f2u(c.v[C_COL + i]);
}
}  // namespace

extern "C" {

int ct_shortcut_compiled() { return VR_SHADOW_BLOCKED_SHORTCUT ? 1 : 0; }

// in: [n][9] = RNG state, cell majorant, vol_majorant, Tr, density (tf: the alpha of the transfer function's one entry), shadow, mipq, tau, t (floats as bit patterns)
// out: [n][10] = state, RNG state, tau, t, Tr, mipq, majorant, the three floats of the collision colour's place on the cold line (-1 where nothing was stored)
// tf 0: the production brick kernel's configuration; 1: the same with a transfer function.  early: the order (see above)
int ct_collide(int tf, int early, long long n, const uint32_t* in, uint32_t* out) {
    using K0 = TraceCfg<false, 0, 0, 0, 0>;
    using K1 = TraceCfg<true, 0, 0, 0, 0>;
    for (long long i = 0; i < n; ++i) {
        const uint32_t* a = in + kIn * i;
        uint32_t* o = out + kOut * i;
        if (tf) { if (early) run<K1, true>(a, o); else run<K1, false>(a, o); }
        else { if (early) run<K0, true>(a, o); else run<K0, false>(a, o); }
    }
    return 0;
}

}  // extern "C"
