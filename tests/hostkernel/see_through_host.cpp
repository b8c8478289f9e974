// tests/hostkernel/see_through_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The see-through tile classifier (volren_amd/csrc/vr_sky_tiles.h: sky_live_cells, sky_touched_tiles, sky_split_tiles3) and the sample of such a tile
// (vr_trace.h sky_sample without its box test) compiled for the host: tests/test_see_through_host.py holds the classifier to a lattice of slab tests against
// the grown live bricks and to the oracle, and the sample to the oracle's trace_pixel_sample bit for bit.
#include <cstdint>
#include <vector>

#include "host_scene.h"
#include "../../volren_amd/csrc/vr_sky_tiles.h"

using namespace vr;

namespace {
// the uniforms as a launch hands them to the classifier: cam_z as RendererHIP::fill_params / host_scene.h form it
SceneParams params_of(const Uniforms* u) {
    SceneParams P{};
    P.u = *u;
    P.cam_z = -0.5f / tan_(0.5f * kPi * u->cam_fov / 180.f);
    return P;
}
// the live-cell pyramid of a range table of nb cells (range == nullptr: a grid whose table the host does not hold)
SkyLiveCells live_of(const uint32_t* range, const int32_t* nb) { return sky_live_cells(range, nb[0], nb[1], nb[2]); }
}  // namespace

extern "C" {

int hk_st_uniforms_size(void) { return (int)sizeof(Uniforms); }
double hk_st_cell_grow(void) { return kSkyCellGrow; }
double hk_st_tap_reach(void) { return kSkyTapReach; }

// cls[i] of tile tiles[i]: 0 march, 1 clear, 2 see-through.  Returns the pyramid cells the descent visited (-1: the fallback, nothing decided)
long long hk_st_classify(const Uniforms* u, const uint32_t* range, const int32_t* nb, const int32_t* tiles, int n, uint8_t* cls) {
    const SceneParams P = params_of(u);
    const SkyLiveCells L = live_of(range, nb);
    sky_classify_tiles3(P, L, tiles, n, cls);
    const SkyTouched T = sky_touched_tiles(P, L);
    return T.valid ? (long long)T.cells_visited : -1;
}

// level-0 liveness of the range table (1 live), and whether a half is NaN
int hk_st_live(const uint32_t* range, const int32_t* nb, uint8_t* live) {
    const SkyLiveCells L = live_of(range, nb);
    for (size_t i = 0; i < L.live[0].size(); ++i) live[i] = L.live[0][i];
    return L.nan ? 1 : 0;
}

// the three-way split of a list (n_ids == 0: the whole frame's n_tiles tiles): march, clear, see-through tiles into out; counts[3] = their numbers
void hk_st_split(const Uniforms* u, const uint32_t* range, const int32_t* nb, const int32_t* ids, int n_ids, int n_tiles, int32_t* out, int32_t* counts) {
    std::vector<int32_t> march, clear, see;
    sky_split_tiles3(params_of(u), live_of(range, nb), std::vector<int32_t>(ids, ids + n_ids), n_tiles, march, clear, see);
    size_t k = 0;
    for (int32_t t : march) out[k++] = t;
    for (int32_t t : clear) out[k++] = t;
    for (int32_t t : see) out[k++] = t;
    counts[0] = (int32_t)march.size(); counts[1] = (int32_t)clear.size(); counts[2] = (int32_t)see.size();
}

// sky_sample WITHOUT the box test of n (px, py, sample number) triples with hashed seeds: out[4 i ..] the sample
void hk_st_samples(const Uniforms* u, const hostscene::hk_grid_desc* density, const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim,
                   const int32_t* items, int n, float* out) {
    hostscene::HostScene S;
    hostscene::build_scene(S, u, density, nullptr, nullptr, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    for (int i = 0; i < n; ++i) {
        const int32_t px = items[3 * i], py = items[3 * i + 1], smp = items[3 * i + 2];
        float L[4] = { -1.0f, -1.0f, -1.0f, -1.0f };
        sky_sample(P, px, py, path_seed((uint32_t)P.u.seed, P.u.resolution[0], px, py, smp), L, false);
        for (int c = 0; c < 4; ++c) out[4 * i + c] = L[c];
    }
}

}
