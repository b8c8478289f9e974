// renderer.cpp -- RendererHIP (see renderer.h).  Host marshalling follows src/renderer.cpp:29-50 (init),
// :56-76 (commit), :78-145 (trace), :159-225 (grid upload), :227-242 (unit cube).
#include "renderer.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>

#include "vr_adaptive.h"
#include "vr_device.h"
#include "vr_math.h"
#include "vr_path_probe.h"
#include "vr_probe.h"
#include "vr_sky_tiles.h"
#include "vr_upsample.h"

namespace vr {

mat3 Camera::view_inverse() const {
    const vec3 f = normalize(dir);
    const vec3 s = normalize(cross(f, up));
    const vec3 u = cross(s, f);
    mat3 r(0.0f);
    r.m[0] = s.x; r.m[1] = s.y; r.m[2] = s.z;
    r.m[3] = u.x; r.m[4] = u.y; r.m[5] = u.z;
    r.m[6] = -f.x; r.m[7] = -f.y; r.m[8] = -f.z;
    return r;
}

RendererHIP::~RendererHIP() {
    // samples recorded by trace() and never looked at are dropped with the framebuffer
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    for (hipEvent_t e : pt_events_) (void)hipEventDestroy(e);
    if (seed_event_) (void)hipEventDestroy(seed_event_);
}

void RendererHIP::init() {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
        throw std::runtime_error("RendererHIP::init: no HIP device available (this renderer has no CPU path)");
    if (!volume) volume = std::make_shared<Volume>();
    if (!environment) {
        const float white[3] = { 1.f, 1.f, 1.f };             // renderer.cpp:36-38: 1x1 white background
        environment = std::make_shared<Environment>(white, 1, 1);
    }
    if (!ev0_) { VR_HIP(hipEventCreate(&ev0_)); VR_HIP(hipEventCreate(&ev1_)); }
    if (!status_) {
        status_ = make_device_buffer(16 * sizeof(uint32_t));         // [0] watchdog flag, [1..8] work-queue heads (one per XCD segment)
        VR_HIP(hipMemset(status_->get(), 0, 16 * sizeof(uint32_t)));
    }
    if (!color && resolution.x > 0 && resolution.y > 0) resize((uint32_t)resolution.x, (uint32_t)resolution.y);
}

void RendererHIP::resize(uint32_t w, uint32_t h) {
    if (w == 0 || h == 0) throw std::runtime_error("RendererHIP::resize: empty framebuffer");
    pending_n_ = 0; pending_ = LaunchInputs{};                   // samples recorded for the framebuffer that goes: nobody can see them any more
    resolution = { (int)w, (int)h };
    color = make_device_buffer((size_t)w * h * 4 * sizeof(float));
    display.reset();
    sized_ = Sized{};                                            // features, moments, the filters' buffers and the history, with what says they are valid
    drop_tile_samples();
    drop_seed_table();                                           // keyed by the frame size
    VR_HIP(hipMemset(color->get(), 0, color->size_bytes()));
    if (!tiles_host_.empty()) set_tiles(tiles_host_);
}

void RendererHIP::reset() { sample = 0; drop_tile_samples(); }

// ---------------------------------------------------------------------------------------------------
static void check_grid_bytes(size_t bytes, const char* what, const int32_t nb[3]);
constexpr size_t kBlockedMajorantBricks = (size_t)1 << 18;       // active bricks above which commit() picks the blocked majorant layout (512 KiB of fp16 level-0 cells: 1/8 of an XCD's L2)
static size_t brick_records(const BrickGridHIP& g);

void RendererHIP::commit() {
    flush_pending();                                              // recorded samples read the device grids that are about to be replaced
    rate_samples_per_ms_ = 0.0; rate_pending_samples_ = 0.0;      // a new volume: nothing measured yet
    density_grids.clear();
    emission_grids.clear();
    majorant_emission = 0.f;
    maj_key_ = MajKey{};
    ++commit_version_;                                            // a cached tile split belongs to the volume it was made from
    std::cout << "Preparing brick grids for HIP..." << std::endl;
    std::vector<size_t> with_emission;                              // frames that have an emission grid (index into both vectors' tails)
    for (const auto& frame : volume->grids) {
        Volume::GridPtr density_grid = frame.at("density");       // throws std::out_of_range like the reference
        density_grids.push_back(grid_to_device(density_grid));
        // the see-through tiles (vr_sky_tiles.h) go by the range table of the host grid the device copy was made from: a brick grid's or a dense fp16 grid's own;
        // a float grid is encoded on the device (or into a temporary brick grid) and the host holds no table of it
        if (auto bg = std::dynamic_pointer_cast<BrickGrid>(density_grid))
            density_grids.back().live_cells = std::make_shared<const SkyLiveCells>(sky_live_cells(bg->range.data.data(), (int32_t)bg->range.stride.x, (int32_t)bg->range.stride.y, (int32_t)bg->range.stride.z));
        else if (auto dg = std::dynamic_pointer_cast<DenseGridF16>(density_grid))
            density_grids.back().live_cells = std::make_shared<const SkyLiveCells>(sky_live_cells(dg->range.data.data(), (int32_t)dg->range.stride.x, (int32_t)dg->range.stride.y, (int32_t)dg->range.stride.z));
        Volume::GridPtr emission_grid;
        for (const char* name : { "flame", "flames", "temperature" }) {
            auto it = frame.find(name);
            if (it != frame.end()) { emission_grid = it->second; break; }
        }
        if (emission_grid) {
            emission_grids.push_back(grid_to_device(emission_grid));
            majorant_emission = std::max(majorant_emission, emission_grid->minorant_majorant().second);
            if (emission_grids.size() == density_grids.size()) with_emission.push_back(density_grids.size() - 1);
        }
    }
    // Second pass, after every grid the frames NEED is on the device (built inside the loop, the paired atlases of early frames could take the memory
    // a later frame's mandatory upload needs, and an animation that loaded before would fail commit()): for a frame whose density and emission grids are both in
    // brick form with the same brick layout, one paired atlas for the kernel compiled for that case (vr_scene.h).  The grids keep their own atlases too
    // (float-atlas decoder, the run-time variant); when a paired one does not fit, the run-time variant serves that frame.
    for (size_t f : with_emission) {
        BrickGridHIP& gd = density_grids[f];
        BrickGridHIP& ge = emission_grids[f];
        if (!(VR_BRICK_HEADERS && gd.atlas && ge.atlas && grids_can_pair(gd, ge))) continue;
        try {
            const size_t n_rec = brick_records(gd);
            check_grid_bytes(n_rec * kPairBlockBytes, "the paired density + emission atlas", gd.nb);
            auto paired = make_device_buffer(n_rec * kPairBlockBytes);
            launch_pair_atlas(gd.atlas->as<uint8_t>(), ge.atlas->as<uint8_t>(), paired->as<uint8_t>(), n_rec, stream);
            VR_HIP(hipGetLastError());
            VR_HIP(hipStreamSynchronize(stream));
            gd.atlas_paired = ge.atlas_paired = paired;
            // Layout of the density grid's majorant table for the kernel that serves this frame.  Levels 0-1 in 4x4x4-cell blocks of one cache line keep a DDA
            // walk's neighbouring cells in the line it has just fetched; that pays on large grids whose bricks are filled in bulk (BASELINE configs[4] as specified,
            // 350 000 active bricks of 2 M: +3 %) and costs 2 % where few bricks are active or the table is cache resident anyway (the 63 000-brick stand-in
            // grid, smoke.brick): profiles/r4d_blocked_majorants_nt_stores_unit_size.txt, profiles/r5_majorant_layout_per_grid.txt
            gd.maj_blocked = gd.n_active > kBlockedMajorantBricks;
        } catch (const std::exception& e) {
            (void)hipGetLastError();
            std::cerr << "volren_amd: no room for the paired density + emission atlas of frame " << f << " (" << e.what() << "): the run-time kernel variant serves it" << std::endl;
        }
    }
}

BrickGridHIP RendererHIP::grid_to_device(const Volume::GridPtr& grid) {
    if (auto f16 = std::dynamic_pointer_cast<DenseGridF16>(grid)) return dense_grid_to_device(f16);
    if (gpu_encoder)
        if (auto dense = std::dynamic_pointer_cast<DenseGrid>(grid)) return dense_to_bricks_on_device(dense);
    return brick_grid_to_device(Volume::to_brick_grid(grid));
}

// HBM a grid may take on the device before the upload is refused with a clear message instead of an out-of-memory error from deep inside
// (the brick-linear atlas is 512 bytes per brick of the grid's BOX, allocated or not: 1 GiB for 1024^3 voxels; the decoded float atlas of
// a transfer-function render is four times that).  Default: what the device reports free, less a reserve for framebuffers and pools.
static void check_grid_bytes(size_t bytes, const char* what, const int32_t nb[3]) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return; }
    const size_t reserve = (size_t)1 << 30;
    if (bytes + reserve > free_b)
        throw std::runtime_error(std::string("grid upload: ") + what + " of a grid of " + std::to_string(nb[0]) + " x " + std::to_string(nb[1]) + " x " + std::to_string(nb[2]) +
                                 " bricks needs " + std::to_string(bytes >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free");
}
// padded power-of-two extent of the majorant levels (vr_scene.h); brick records and atlas blocks have exact pitches
static void set_layout(BrickGridHIP& out) {
    for (int i = 0; i < 3; ++i) out.mshift[i] = std::max(3, ceil_log2((uint32_t)out.nb[i]));
    // (4e8 bricks: a tap addresses its cache line of the atlas by a 32-bit line index, 5 lines per brick -- 10 in a paired atlas --: vr_trace.h tap_load; such a
    // grid's atlas alone is 256 GB)
    if (out.mshift[0] + out.mshift[1] + out.mshift[2] > 30 || (uint64_t)out.nb[0] * out.nb[1] * out.nb[2] > 400000000ull)
        throw std::runtime_error("grid upload: more than 4e8 bricks");
    if ((uint64_t)out.nb[1] * out.nb[2] >= (1ull << 24) || out.nb[0] >= (1 << 24))
        throw std::runtime_error("grid upload: brick counts beyond the 24-bit index arithmetic of the kernels (n_bricks.y * n_bricks.z < 2^24)");
    const size_t cells = majorant_table_cells((uint32_t)(out.mshift[0] + out.mshift[1] + out.mshift[2]));
    out.majorant = make_device_buffer(cells * sizeof(float));
    out.majorant16 = make_device_buffer(cells * sizeof(uint16_t));
}
static size_t brick_records(const BrickGridHIP& g) { return (size_t)g.nb[0] * g.nb[1] * g.nb[2]; }

static void upload_range_words(BrickGridHIP& out, const uvec3 nb, const Buf3D<uint32_t>& range, const std::vector<Buf3D<uint32_t>>& mips) {
    if (mips.size() > 3) throw std::runtime_error("grid upload: at most 3 range mips are supported");
    std::vector<uint32_t> words(range.data);
    out.n_mips = (int)mips.size();
    for (int m = 0; m <= 3; ++m) out.mip_off[m] = 0;
    for (int m = 1; m <= out.n_mips; ++m) {
        const auto& mm = mips[m - 1];
        const uint32_t rnd = (1u << m) - 1u;
        if (mm.stride.x != ((nb.x + rnd) >> m) || mm.stride.y != ((nb.y + rnd) >> m) || mm.stride.z != ((nb.z + rnd) >> m))
            throw std::runtime_error("grid upload: range mip dimensions are not ceil(n_bricks / 2^m)");
        out.mip_off[m] = (int32_t)words.size();
        words.insert(words.end(), mm.data.begin(), mm.data.end());
    }
    out.n_cells = (int32_t)words.size();
    out.range_words = make_device_buffer(words.size() * sizeof(uint32_t));
    out.range_words->upload(words.data(), words.size() * sizeof(uint32_t));
    set_layout(out);
}

BrickGridHIP RendererHIP::dense_to_bricks_on_device(const std::shared_ptr<DenseGrid>& g) {
    BrickGridHIP out;
    auto up8 = [](uint32_t v) { return ((v + 7u) / 8u + 7u) / 8u * 8u; };
    const int32_t dim[3] = { (int32_t)g->dim.x, (int32_t)g->dim.y, (int32_t)g->dim.z };
    const int32_t nb[3] = { (int32_t)up8(g->dim.x), (int32_t)up8(g->dim.y), (int32_t)up8(g->dim.z) };
    const size_t n = (size_t)nb[0] * nb[1] * nb[2];
    for (int i = 0; i < 3; ++i) out.nb[i] = nb[i];
    out.transform = g->transform;
    DeviceBuffer dense(g->voxels.size() * sizeof(float)), flag(n * sizeof(uint32_t));
    dense.upload(g->voxels.data(), g->voxels.size() * sizeof(float), stream);
    // range words of all mips in one buffer (mip m has ceil(nb / 2^m) cells per axis)
    int32_t mdim[4][3];
    size_t total = 0;
    out.n_mips = 3;
    for (int m = 0; m <= 3; ++m) {
        for (int i = 0; i < 3; ++i) mdim[m][i] = (nb[i] + (1 << m) - 1) >> m;
        out.mip_off[m] = (int32_t)total;
        total += (size_t)mdim[m][0] * mdim[m][1] * mdim[m][2];
    }
    out.n_cells = (int32_t)total;
    out.range_words = make_device_buffer(total * sizeof(uint32_t));
    set_layout(out);
    uint32_t* words = out.range_words->as<uint32_t>();
    launch_encode_ranges(dense.as<float>(), dim, nb, words, flag.as<uint32_t>(), stream);
    VR_HIP(hipGetLastError());
    check_grid_bytes(brick_records(out) * (kBrickBlockBytes + sizeof(BrickRec) + 8), "the brick-linear atlas", out.nb);
    out.atlas = make_device_buffer(brick_records(out) * kBrickBlockBytes);   // brick-linear blocks (see brick_grid_to_device)
    VR_HIP(hipMemsetAsync(out.atlas->get(), 0, out.atlas->size_bytes(), stream));
    out.bricks = make_device_buffer(brick_records(out) * sizeof(BrickRec));
    VR_HIP(hipMemsetAsync(out.bricks->get(), 0, out.bricks->size_bytes(), stream));
    out.rng = make_device_buffer(brick_records(out) * 2 * sizeof(float));
    VR_HIP(hipMemsetAsync(out.rng->get(), 0, out.rng->size_bytes(), stream));
    launch_encode_bricks(dense.as<float>(), dim, nb, words, flag.as<uint32_t>(), out.bricks->as<BrickRec>(), out.rng->as<float>(), out.atlas->as<uint8_t>(), stream);
    for (int m = 1; m <= 3; ++m) launch_range_mip(words + out.mip_off[m - 1], mdim[m - 1], words + out.mip_off[m], mdim[m], stream);
    VR_HIP(hipGetLastError());
    VR_HIP(hipStreamSynchronize(stream));
    {   // bricks whose voxels matter (majorant layout choice, commit())
        std::vector<uint32_t> flags(n);
        flag.download(flags.data(), n * sizeof(uint32_t), stream);
        for (uint32_t f : flags) out.n_active += f != 0u;
    }
    return out;
}

// FNV-1a over `n` bytes, continuing from `h` (default: the start value): the checksums below, and the keys of tile_order and submit
constexpr uint64_t kFnv1aStart = 1469598103934665603ull;
static uint64_t fnv1a(const void* p, size_t n, uint64_t h = kFnv1aStart) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
void RendererHIP::grid_checksums(const BrickGridHIP& g, uint64_t out[3]) const {
    const DeviceBufferPtr bufs[3] = { g.bricks, g.atlas, g.range_words };
    for (int i = 0; i < 3; ++i) {
        out[i] = 0;
        if (!bufs[i]) continue;
        std::vector<uint8_t> h(bufs[i]->size_bytes());
        bufs[i]->download(h.data(), h.size(), stream);
        out[i] = fnv1a(h.data(), h.size());
    }
}

BrickGridHIP RendererHIP::dense_grid_to_device(const std::shared_ptr<DenseGridF16>& g) {
    BrickGridHIP out;
    const uvec3 nb = g->range.stride;
    out.nb[0] = (int)nb.x; out.nb[1] = (int)nb.y; out.nb[2] = (int)nb.z;
    out.dim[0] = (int)g->dim.x; out.dim[1] = (int)g->dim.y; out.dim[2] = (int)g->dim.z;
    if (g->dim.x > 65535u || g->dim.y > 65535u || g->dim.z > 65535u) throw std::runtime_error("dense_grid_to_device: more than 65535 voxels along an axis");
    out.transform = g->transform;
    // re-tile [z][y][x] into 4x4x4 blocks of 128 contiguous bytes (vr_scene.h), zero padded
    const uint32_t bx = (g->dim.x + 3u) / 4u, by = (g->dim.y + 3u) / 4u, bz = (g->dim.z + 3u) / 4u;
    if ((uint64_t)bx * by * bz > (1ull << 31)) throw std::runtime_error("dense_grid_to_device: more than 2^31 blocks");
    out.dblk[0] = (int)bx; out.dblk[1] = (int)by;
    std::vector<uint16_t> blocked((size_t)bx * by * bz * 64u, 0);
    for (uint32_t z = 0; z < g->dim.z; ++z)
        for (uint32_t y = 0; y < g->dim.y; ++y) {
            const uint16_t* row = &g->voxels[((size_t)z * g->dim.y + y) * g->dim.x];
            for (uint32_t x = 0; x < g->dim.x; ++x) blocked[dense_blocked_index(x, y, z, bx, by)] = row[x];
        }
    out.dense = make_device_buffer(blocked.size() * sizeof(uint16_t));
    out.dense->upload(blocked.data(), blocked.size() * sizeof(uint16_t));
    upload_range_words(out, nb, g->range, g->range_mipmaps);
    return out;
}

BrickGridHIP RendererHIP::brick_grid_to_device(const std::shared_ptr<BrickGrid>& g) {
    BrickGridHIP out;
    const uvec3 nb = g->n_bricks;
    const size_t n_bricks = (size_t)nb.x * nb.y * nb.z;
    if (n_bricks == 0) throw std::runtime_error("brick_grid_to_device: empty grid");
    out.nb[0] = (int)nb.x; out.nb[1] = (int)nb.y; out.nb[2] = (int)nb.z;
    out.transform = g->transform;
    // atlas: 3D texture of 8^3 blocks addressed through the indirection words -> brick-LINEAR blocks: the block of brick record i is bytes
    // [640 i, 640 i + 640), five cache lines of [rmin, rdiff | 120 voxels] (vr_scene.h), so that a tap fetches range and voxel from one line
    // instead of chasing the pointer (vr_trace.h tap_load).  A brick whose range is a single value keeps zero voxels (they never matter:
    // rmin + u * 0), and so does a pointer outside the atlas (GL: undefined fetch); every line of every brick carries the range.
    const uvec3 ad = g->atlas.stride;
    const uint32_t sx = ad.x / 8, sy = ad.y / 8, sz = ad.z / 8;
    upload_range_words(out, nb, g->range, g->range_mipmaps);        // also fixes the padded majorant layout (mshift)
    check_grid_bytes(brick_records(out) * (kBrickBlockBytes + sizeof(BrickRec) + 8), "the brick-linear atlas", out.nb);
    std::vector<BrickRec> recs(brick_records(out), BrickRec{ 0u, 0.f, 0.f, 0u });
    std::vector<uint8_t> atlas(recs.size() * (size_t)kBrickBlockBytes, 0);
    for (size_t i = 0; i < n_bricks; ++i) {
        const uint32_t ind = g->indirection.data[i], rg = g->range.data[i];
        const uint32_t px = ind >> 22, py = (ind >> 12) & 1023u, pz = (ind >> 2) & 1023u;
        const float lo = half2float(rg & 0xFFFFu), hi = half2float(rg >> 16);
        const size_t idx = i;                                        // record index = linear brick index (x fastest)
        BrickRec r;
        r.slot = (uint32_t)idx;
        r.rmin = lo;
        r.rdiff = hi - lo;
        r.range = rg;
        recs[idx] = r;
        uint8_t* dst = &atlas[idx * (size_t)kBrickBlockBytes];
        if (VR_BRICK_HEADERS)
            for (uint32_t l = 0; l < 5; ++l) { memcpy(dst + l * 128u, &r.rmin, 4); memcpy(dst + l * 128u + 4u, &r.rdiff, 4); }
        if (r.rdiff != 0.f && px < sx && py < sy && pz < sz) {
            ++out.n_active;
            for (uint32_t z = 0; z < 8; ++z)
                for (uint32_t y = 0; y < 8; ++y) {
                    const uint8_t* src = &g->atlas.data[g->atlas.index(px * 8, py * 8 + y, pz * 8 + z)];
                    for (uint32_t x = 0; x < 8; ++x) dst[brick_voxel_byte(z * 64 + y * 8 + x)] = src[x];
                }
        }
    }
    out.bricks = make_device_buffer(recs.size() * sizeof(BrickRec));
    out.bricks->upload(recs.data(), recs.size() * sizeof(BrickRec));
    std::vector<float> rng(recs.size() * 2);
    for (size_t i = 0; i < recs.size(); ++i) { rng[2 * i] = recs[i].rmin; rng[2 * i + 1] = recs[i].rdiff; }
    out.rng = make_device_buffer(rng.size() * sizeof(float));
    out.rng->upload(rng.data(), rng.size() * sizeof(float));
    out.atlas = make_device_buffer(atlas.size());
    out.atlas->upload(atlas.data(), atlas.size());
    return out;
}

void RendererHIP::scale_and_move_to_unit_cube() {
    // max AABB over the whole volume (animation); FLT_MIN start value is the reference's quirk (renderer.cpp:229)
    vec3 bb_min(FLT_MAX), bb_max(FLT_MIN);
    for (const auto& frame : volume->grids) {
        const auto grid = frame.at("density");
        const uvec3 e = grid->index_extent();
        bb_min = vmin(bb_min, transform_point(grid->transform, vec3(0.f, 0.f, 0.f)));
        bb_max = vmax(bb_max, transform_point(grid->transform, vec3((float)e.x, (float)e.y, (float)e.z)));
    }
    const vec3 extent = bb_max - bb_min;
    const float size = std::fmax(extent.x, std::fmax(extent.y, extent.z));
    if (size != 1.f) {
        volume->transform = scale_then_translate(1.f / size, -bb_min - extent * 0.5f);
        density_scale *= size;
    }
}

// ---------------------------------------------------------------------------------------------------
static void copy3(float* dst, vec3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

static GridView make_view(const BrickGridHIP& g, bool paired = false, bool maj_blocked = false) {
    GridView v;
    memset(&v, 0, sizeof v);                     // padding bytes too: launch inputs are compared byte by byte (LaunchInputs::same_launch_as)
    v.bricks = g.bricks ? g.bricks->as<BrickRec>() : nullptr;
    v.atlas = paired ? g.atlas_paired->as<uint8_t>() : (g.atlas ? g.atlas->as<uint8_t>() : nullptr);
    v.dense = g.dense ? g.dense->as<uint16_t>() : nullptr;
    for (int i = 0; i < 3; ++i) v.dim[i] = g.dim[i];
    for (int i = 0; i < 2; ++i) v.dblk[i] = g.dblk[i];
    v.majorant = g.majorant->as<float>();
    v.majorant16 = g.majorant16->as<uint16_t>();
    v.rng = g.rng ? g.rng->as<float>() : nullptr;
    v.atlas_f32 = g.atlas_f32 ? g.atlas_f32->as<float>() : nullptr;
    for (int i = 0; i < 3; ++i) v.nb[i] = g.nb[i];
    for (int i = 0; i < 3; ++i) { v.mshift[i] = g.mshift[i]; v.mlim[i] = (float)(8u << g.mshift[i]); }
    v.n_mips = g.n_mips;
    v.maj_blocked = maj_blocked ? 1 : 0;         // the layout the majorant table is (re)built in and the kernel variant reads (vr_variant.h)
    v.maj_outside = (int32_t)majorant_padded_cells((uint32_t)(g.mshift[0] + g.mshift[1] + g.mshift[2]));
    return v;
}

void RendererHIP::fill_params(SceneParams& P) {
    if (!volume || volume->grids.empty() || density_grids.empty())
        throw std::runtime_error("RendererHIP::trace: no volume committed");
    if (volume->grid_frame_counter >= density_grids.size())
        throw std::runtime_error("RendererHIP::trace: grid_frame_counter out of range (commit() after changing the volume)");
    memset(&P, 0, sizeof P);
    Uniforms& u = P.u;
    u.bounces = bounces;
    u.seed = seed;
    u.show_environment = show_environment ? 1 : 0;
    u.integrator = integrator;
    P.env_div_safe = environment->cdf_div_safe ? 1 : 0;      // (here already: with the density scale, what decides below which views of the grids the kernel is handed)
    // camera
    copy3(u.cam_pos, camera.pos);
    u.cam_fov = camera.fov_degree;
    const mat3 ct = camera.view_inverse();
    memcpy(u.cam_transform, ct.m, sizeof ct.m);
    P.cam_z = camera_z(camera.fov_degree);
    // volume
    const auto [bb_min, bb_max] = volume->AABB();
    const auto [mn, maj] = volume->minorant_majorant();
    copy3(u.vol_bb_min, bb_min + vol_clip_min * (bb_max - bb_min));
    copy3(u.vol_bb_max, bb_min + vol_clip_max * (bb_max - bb_min));
    u.vol_minorant = mn * density_scale;
    u.vol_majorant = maj * density_scale;
    u.vol_inv_majorant = 1.f / (maj * density_scale);
    copy3(u.vol_albedo, albedo);
    u.vol_phase_g = phase;
    u.vol_density_scale = density_scale;
    u.vol_emission_scale = emission_scale;
    u.vol_emission_norm = majorant_emission > 0.f ? 1.f / std::fmax(majorant_emission, 1e-4f) : 1.f;
    // density brick grid data
    const BrickGridHIP& density = density_grids[volume->grid_frame_counter];
    const mat4 dt = volume->transform * density.transform;
    const mat4 dti = inverse(dt);
    memcpy(u.vol_density_transform, dt.m, sizeof dt.m);
    memcpy(u.vol_density_inv_transform, dti.m, sizeof dti.m);
    P.density = make_view(density);
    // emission brick grid data
    if (volume->grid_frame_counter < emission_grids.size()) {
        const BrickGridHIP& emission = emission_grids[volume->grid_frame_counter];
        const mat4 et = volume->transform * emission.transform;
        const mat4 eti = inverse(et);
        memcpy(u.vol_emission_transform, et.m, sizeof et.m);
        memcpy(u.vol_emission_inv_transform, eti.m, sizeof eti.m);
        const mat4 efd = eti * dt;
        memcpy(P.emission_from_density, efd.m, sizeof efd.m);
        // the kernel compiled for two brick grids (DDA trackers) reads them from their paired atlas; every other kernel reads each grid's own
        // (a scene that goes to the run-time variant whatever its grids -- integrator, warp table, density scale: vr_variant.h -- is rendered from the grids' own atlases)
        P.paired = (density.atlas_paired && density.atlas_paired == emission.atlas_paired && pathtrace_scene_reasons(P) == 0) ? 1 : 0;
        // ... and is the one kernel compiled for both layouts of the majorant table's fine levels: blocked for the grids commit() marked (or as majorant_layout says)
        if (P.paired) P.density = make_view(density, true, majorant_layout < 0 ? density.maj_blocked : majorant_layout == 1);
        P.emission = make_view(emission, P.paired != 0);
        u.has_emission = 1;
    }
    // transfer function
    if (transferfunc) {
        u.use_tf = 1;
        u.tf_size = transferfunc->size();
        u.tf_window_left = transferfunc->window_left;
        u.tf_window_width = transferfunc->window_width;
        P.tf_lut = transferfunc->lut_ssbo->as<float>();
    }
    // environment
    const mat3 eit = inverse(environment->transform);
    memcpy(u.env_transform, environment->transform.m, sizeof eit.m);
    memcpy(u.env_inv_transform, eit.m, sizeof eit.m);
    u.env_strength = environment->strength;
    u.env_imp_inv_dim[0] = u.env_imp_inv_dim[1] = 1.f / (float)environment->dimension();
    u.env_imp_base_mip = (int)std::floor(std::log2((float)environment->dimension()));
    P.envmap = environment->envmap->as<float>();
    P.env_rgbe = environment->envmap_rgbe ? environment->envmap_rgbe->as<uint32_t>() : nullptr;
    P.env_w = environment->width; P.env_h = environment->height;
    P.env_avg_w = environment->avg_importance; P.env_avg_w_set = 1;
    P.impmap = environment->impmap->as<float>();
    P.imp_dim = (int)environment->dimension();
    P.env_cdf = environment->cdf->as<float>();
    u.resolution[0] = resolution.x; u.resolution[1] = resolution.y;
}

void RendererHIP::update_majorants(const LaunchInputs& in, BrickGridHIP& g) {
    if (in.maj == maj_key_) return;
    launch_majorants(in.P, g.range_words->as<uint32_t>(), g.nb, g.mip_off, g.n_mips, g.mshift, g.majorant->as<float>(), g.majorant16->as<uint16_t>(), in.stream);
    VR_HIP(hipGetLastError());
    maj_key_ = in.maj;
}

void RendererHIP::set_tiles(const std::vector<int32_t>& tile_ids) {
    flush_pending();
    tiles_host_ = tile_ids;
    tiles_dev_.reset();
    if (tile_ids.empty()) return;
    if (resolution.x > 0) {
        const int n_all = tile_count(resolution.x, resolution.y);
        for (int32_t t : tile_ids)
            if (t < 0 || t >= n_all) throw std::runtime_error("set_tiles: tile id out of range");   // never launch out-of-bounds tiles
    }
    tiles_dev_ = make_device_buffer(tile_ids.size() * sizeof(int32_t));
    tiles_dev_->upload(tile_ids.data(), tile_ids.size() * sizeof(int32_t));
}

// The order in which a launch works through its tiles.  The persistent wavefronts pull work units from a queue (vr_pathtrace.h) whose positions enumerate the
// tile list front to back in 8 contiguous segments, one per XCD; when the queue runs empty every wavefront still has to finish the paths in its pool, and
// the launch ends with its deepest path (4-5 ms on the bench scene: 2 % of a frame on one GPU, 15 % of a rank's share on eight).  With the costly tiles --
// long chords through the volume's box -- at the FRONT of every segment and the tiles whose rays miss the box at its end, what is left at that point are
// camera rays that escape at once.  Cost estimate: the longest chord of five rays of the tile (corners and centre, no jitter) through the clipped box.
// Sorted (stably) inside each eighth of the list, so that an XCD keeps its band of tile rows.  tile_order caches the device list per (camera, box,
// frame size, tile list); ids empty = the n_tiles tiles of the whole frame.
std::vector<int32_t> RendererHIP::costliest_first(const SceneParams& P, const std::vector<int32_t>& tile_ids, int n_tiles) const {
    const Uniforms& u = P.u;
    const int W = u.resolution[0], H = u.resolution[1], tiles_x = vr::tiles_x(W);
    std::vector<int32_t> ids(tile_ids);
    if (ids.empty()) { ids.resize((size_t)n_tiles); for (int i = 0; i < n_tiles; ++i) ids[(size_t)i] = i; }
    auto chord = [&](float px, float py) {
        float d[3] = { (px - 0.5f * (float)W) / (float)H, (py - 0.5f * (float)H) / (float)H, P.cam_z };
        float w[3];
        for (int i = 0; i < 3; ++i) w[i] = u.cam_transform[i] * d[0] + u.cam_transform[3 + i] * d[1] + u.cam_transform[6 + i] * d[2];      // direction up to its length: only t-ratios matter
        const float len = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        float t0 = 0.f, t1 = FLT_MAX;
        for (int i = 0; i < 3; ++i) {
            const float inv = 1.f / (w[i] / len);
            const float a = (u.vol_bb_min[i] - u.cam_pos[i]) * inv, b = (u.vol_bb_max[i] - u.cam_pos[i]) * inv;
            t0 = std::fmax(t0, std::fmin(a, b)); t1 = std::fmin(t1, std::fmax(a, b));
        }
        return t1 > t0 ? t1 - t0 : 0.f;
    };
    std::vector<float> cost(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) {
        const float x0 = (float)((ids[k] % tiles_x) * 16), y0 = (float)((ids[k] / tiles_x) * 16);
        const float x1 = std::fmin(x0 + 16.f, (float)W), y1 = std::fmin(y0 + 16.f, (float)H);
        cost[k] = std::fmax(std::fmax(std::fmax(chord(x0, y0), chord(x1, y0)), std::fmax(chord(x0, y1), chord(x1, y1))), chord(0.5f * (x0 + x1), 0.5f * (y0 + y1)));
    }
    std::vector<int32_t> perm(ids.size());
    for (size_t k = 0; k < perm.size(); ++k) perm[k] = (int32_t)k;
    const size_t seg = (ids.size() + 7) / 8;                                  // the queue's segments are eighths of the unit list = of the tile list
    for (size_t b = 0; b < ids.size(); b += seg)
        std::stable_sort(perm.begin() + (ptrdiff_t)b, perm.begin() + (ptrdiff_t)std::min(ids.size(), b + seg), [&](int32_t x, int32_t y) { return cost[(size_t)x] > cost[(size_t)y]; });
    std::vector<int32_t> ordered(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) ordered[k] = ids[(size_t)perm[k]];
    return ordered;
}

uint64_t RendererHIP::tile_order_key(const SceneParams& P, const std::vector<int32_t>& ids, int n_tiles) const {
    const Uniforms& u = P.u;
    uint64_t key = kFnv1aStart;
    auto mix = [&key](const void* p, size_t nbytes) { key = fnv1a(p, nbytes, key); };
    mix(u.cam_pos, sizeof u.cam_pos); mix(u.cam_transform, sizeof u.cam_transform); mix(&P.cam_z, sizeof P.cam_z);
    mix(u.vol_bb_min, sizeof u.vol_bb_min); mix(u.vol_bb_max, sizeof u.vol_bb_max); mix(u.resolution, sizeof u.resolution); mix(&n_tiles, sizeof n_tiles);
    if (!ids.empty()) mix(ids.data(), ids.size() * sizeof(int32_t));
    return key ? key : 1;
}

// The three-way split (vr_sky_tiles.h sky_split_tiles3) with the live cells of the launch's density grid -- or with none, which leaves the see-through class
// empty and the other two what sky_split_tiles gives: when the class is switched off, or the host holds no range table of the grid.
void RendererHIP::split_three(const LaunchInputs& in, const std::vector<int32_t>& ids, int n_tiles, std::vector<int32_t>& march, std::vector<int32_t>& clear, std::vector<int32_t>& see) const {
    static const SkyLiveCells none;
    const std::shared_ptr<const SkyLiveCells>& held = density_grids.at(in.frame).live_cells;
    sky_split_tiles3(in.P, in.see_through_tiles != 0 && held ? *held : none, ids, n_tiles, march, clear, see);
}

// Clear and see-through tiles (vr_sky_tiles.h) are no work for the path scheduler: split_tiles takes them out of a submit's list.  What costliest_first says about
// order applies to the march tiles that stay.  The clear class reads what tile_order's key hashes and nothing else; the see-through class also reads the density
// grid's live cells (the grid frame of one committed volume), its switch, the index-to-world transform and the uniforms its fallbacks look at.  The device list --
// and the answer "nothing to split off", which needs none -- is cached under the key of all of that.
RendererHIP::SplitTiles RendererHIP::split_tiles(const LaunchInputs& in, const std::vector<int32_t>& ids, int n_tiles, bool ordered) {
    const SceneParams& P = in.P;
    const int tag = ordered ? 2 : 1;
    uint64_t key = fnv1a(&tag, sizeof tag, tile_order_key(P, ids, n_tiles));
    {
        const Uniforms& u = P.u;
        const uint64_t frame = in.frame, version = commit_version_;
        auto mix = [&key](const void* p, size_t nbytes) { key = fnv1a(p, nbytes, key); };
        mix(&frame, sizeof frame); mix(&version, sizeof version); mix(&in.see_through_tiles, sizeof in.see_through_tiles);
        mix(u.vol_density_transform, sizeof u.vol_density_transform); mix(&u.vol_density_scale, sizeof u.vol_density_scale);
        mix(&u.integrator, sizeof u.integrator); mix(&u.has_emission, sizeof u.has_emission); mix(&u.use_tf, sizeof u.use_tf);
    }
    key = key ? key : 1;
    if (split_key_ != key) {
        std::vector<int32_t> march, clear, see;
        split_three(in, ids, n_tiles, march, clear, see);
        if (!clear.empty() || !see.empty()) {
            if (ordered && !march.empty()) march = costliest_first(P, march, (int)march.size());
            march.insert(march.end(), clear.begin(), clear.end());
            march.insert(march.end(), see.begin(), see.end());
            ensure_buffer(split_dev_, march.size() * sizeof(int32_t));
            split_dev_->upload(march.data(), march.size() * sizeof(int32_t), stream);
        }
        split_n_sky_ = (int)clear.size();
        split_n_see_ = (int)see.size();
        split_key_ = key;
    }
    SplitTiles s;
    if (split_n_sky_ + split_n_see_ > 0) {
        s.n_sky = split_n_sky_;
        s.n_see = split_n_see_;
        s.n_march = n_tiles - split_n_sky_ - split_n_see_;
        s.march = split_dev_->as<int32_t>();
        s.sky = s.march + s.n_march;
    }
    return s;
}

const int32_t* RendererHIP::tile_order(const SceneParams& P, const std::vector<int32_t>& ids, int n_tiles) {
    const uint64_t key = tile_order_key(P, ids, n_tiles);
    if (order_dev_ && order_key_ == key && order_dev_->size_bytes() == (size_t)n_tiles * sizeof(int32_t)) return order_dev_->as<int32_t>();
    const std::vector<int32_t> ordered = costliest_first(P, ids, n_tiles);
    ensure_buffer(order_dev_, ordered.size() * sizeof(int32_t));
    order_dev_->upload(ordered.data(), ordered.size() * sizeof(int32_t), stream);
    order_key_ = key;
    return order_dev_->as<int32_t>();
}

bool RendererHIP::LaunchInputs::same_launch_as(const LaunchInputs& o) const {
    return memcmp(&P, &o.P, sizeof P) == 0 && frame == o.frame && maj == o.maj && tuning == o.tuning && order_tiles == o.order_tiles && launch_target_ms == o.launch_target_ms &&
           fast_math == o.fast_math && variance == o.variance && sky_tiles == o.sky_tiles && see_through_tiles == o.see_through_tiles && sample_pool_bytes == o.sample_pool_bytes && stream == o.stream;
}

// What a launch reads from the renderer's public, freely mutable state -- taken when trace() / render() is CALLED (the reference issues its dispatch at that
// point: src/renderer.cpp:78-145), used when the samples are launched.
void RendererHIP::capture(LaunchInputs& in) {
    if (!color) throw std::runtime_error("RendererHIP::trace: no framebuffer (call resize first)");
    if (integrator == 2 && !transferfunc) throw std::runtime_error("RendererHIP::trace: integrator 2 (direct volume rendering) needs a transfer function");
    if (integrator < 0 || integrator > 3) throw std::runtime_error("RendererHIP::trace: unknown integrator");
    // the tolerance mode is offered where it stays within 1e-3 relative L2 of the reference's kernels; behind a transfer function it does
    // not (a dark image carried by a few bright pixels: 1.9e-3 at 64x48x1024 spp), so it is refused there rather than shipped
    if (fast_math && transferfunc) throw std::runtime_error("RendererHIP::trace: fast_math is not available while a transfer function is bound (it misses the 1e-3 bound there); set fast_math 0");
    if (!volume || volume->grids.empty() || density_grids.empty()) throw std::runtime_error("RendererHIP::trace: no volume committed");
    if (volume->grid_frame_counter >= density_grids.size()) throw std::runtime_error("RendererHIP::trace: grid_frame_counter out of range (commit() after changing the volume)");
    {   // transfer-function renders of brick grids read a decoded float atlas (vr_trace.h trilinear_load): build it on first use.
        // 4 bytes per voxel of every brick; when that does not fit, the byte atlas keeps serving (same values either way).
        BrickGridHIP& g = density_grids[volume->grid_frame_counter];
        const bool build = transferfunc && tf_float_atlas && !g.dense && g.atlas && g.rng && !g.atlas_f32 && !g.atlas_f32_failed;
        const bool drop = (!transferfunc || !tf_float_atlas) && (g.atlas_f32 || g.atlas_f32_failed);
        if (build || drop) flush_pending();                          // recorded samples may read the atlas that goes, or need the memory that comes
        if (build) {
            try {
                // decoded atlases of the other animation frames stay while they fit: a looping animation behind a transfer function (the reference cycles
                // its frames) decodes every frame once, not at every frame change (hipFree synchronises the device).  Budget: half of what the device
                // has free, and at the latest when the allocation fails, all others go (least recently decoded = lowest index first: no LRU bookkeeping)
                const size_t n_blocks = g.atlas->size_bytes() / kBrickBlockBytes, want = n_blocks * 512u * sizeof(float);
                auto drop_others = [&] { for (BrickGridHIP& other : density_grids) if (&other != &g) other.atlas_f32.reset(); };
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = ~(size_t)0; }
                if (want > free_b / 2) drop_others();
                try { g.atlas_f32 = make_device_buffer(want); }
                catch (const std::exception&) { (void)hipGetLastError(); drop_others(); g.atlas_f32 = make_device_buffer(want); }
                launch_decode_atlas(g.rng->as<float>(), g.atlas->as<uint8_t>(), g.atlas_f32->as<float>(), n_blocks, stream);
                VR_HIP(hipGetLastError());
            } catch (const std::exception& e) {
                (void)hipGetLastError();
                g.atlas_f32.reset();
                g.atlas_f32_failed = true;      // not retried per launch: a per-sample trace() loop would pay a failing multi-GB hipMalloc every call
                std::cerr << "volren_amd: no room for the decoded float atlas (" << (g.atlas->size_bytes() / kBrickBlockBytes * 2048u >> 20) << " MiB): transfer-function taps read the byte atlas (" << e.what() << ")" << std::endl;
            }
        }
        if (drop) { g.atlas_f32.reset(); g.atlas_f32_failed = false; }
    }
    fill_params(in.P);
    in.frame = volume->grid_frame_counter;
    in.maj = MajKey{};
    in.maj.density_scale = density_scale;
    in.maj.tf_version = transferfunc ? transferfunc->version : 0;
    in.maj.wl = transferfunc ? transferfunc->window_left : 0.f;
    in.maj.ww = transferfunc ? transferfunc->window_width : 0.f;
    in.maj.frame = in.frame;
    in.maj.blocked = in.P.density.maj_blocked;
    in.tuning = tuning;
    in.order_tiles = order_tiles; in.launch_target_ms = launch_target_ms; in.fast_math = fast_math ? 1 : 0; in.variance = variance != 0 ? 1 : 0; in.sky_tiles = sky_tiles != 0 ? 1 : 0;
    in.see_through_tiles = see_through_tiles != 0 ? 1 : 0;
    in.sample_pool_bytes = sample_pool_bytes;
    in.stream = stream;
    in.env = environment; in.tf = transferfunc;
    in.keep[0] = environment->envmap; in.keep[1] = environment->impmap; in.keep[2] = environment->cdf;
    in.keep[3] = transferfunc ? transferfunc->lut_ssbo : DeviceBufferPtr();
    in.keep[4] = environment->envmap_rgbe;
}

// samples of one sub-launch as the sample pool and the 32-bit item indices allow (before any sizing by time)
int RendererHIP::samples_per_launch(const LaunchInputs& in, int n_tiles) const {
    const size_t per_sample = pathtrace_pool_floats(in.tuning, n_tiles, 1) * sizeof(float);
    int per_launch = (int)std::max<size_t>(1, in.sample_pool_bytes / per_sample);
    // item indices inside a sub-launch are 32-bit (WorkUnit::base, C_ITEM): keep n_tiles * 256 * (per_launch rounded up to whole units of at most 8 samples)
    // below 2^32.  Saturating: for frames beyond 2^27 pixels the quotient is smaller than the margin (the unsigned difference wrapped and the clamp
    // stopped limiting anything); launch_pathtrace refuses a launch whose items do not fit.
    const size_t lim = (size_t)0xFFFFFFFFu / ((size_t)n_tiles * 256u);
    per_launch = (int)std::min<size_t>((size_t)per_launch, lim > 8 ? lim - 8 : 1);
    if (per_launch > 32) per_launch -= per_launch % 32;          // whole sample chunks (32 is a multiple of every unit size)
    return per_launch;
}

void RendererHIP::submit_tile_set(const LaunchInputs& in, int first, int n) {
    if (n <= 0) return;
    const int n_tiles = tile_set_size();
    const bool ordered = in.order_tiles >= 2 || (in.order_tiles == 1 && tiles_dev_);
    const SplitTiles split = in.splits_sky() ? split_tiles(in, tiles_dev_ ? tiles_host_ : std::vector<int32_t>(), n_tiles, ordered) : SplitTiles{};
    if (split.n_sky + split.n_see > 0) {                         // the march tiles to the path tracer, the clear and the see-through ones to the sky kernel
        const int per_launch = prepare_submit(in, first, n, split.n_march, split.n_sky + split.n_see);
        open_timing_window(in.stream);
        submit(in, first, n, split.march, split.n_march, per_launch, split.sky, split.n_sky, split.n_see);
        close_timing_window(in.stream);
        return;
    }
    const int32_t* tiles = ordered ? tile_order(in.P, tiles_host_, n_tiles) : (tiles_dev_ ? tiles_dev_->as<int32_t>() : nullptr);
    const int per_launch = prepare_submit(in, first, n, n_tiles);      // (a throw here leaves the last call's window as it is)
    open_timing_window(in.stream);
    submit(in, first, n, tiles, n_tiles, per_launch);
    close_timing_window(in.stream);                              // (not after a throw: a call that failed leaves no time to read)
}

int RendererHIP::tile_set_size() const { return tiles_dev_ ? (int)tiles_host_.size() : tile_count(resolution.x, resolution.y); }

// The timing window of one call (last_launches, last_kernel_ms, last_pathtrace_ms) spans its launches: render() and trace() open it between prepare_submit and
// submit, so that it holds the sub-launches alone; render_adaptive opens it before its first group and closes it after its last.
void RendererHIP::open_timing_window(hipStream_t s) { VR_HIP(hipEventRecord(ev0_, s)); last_launches = 0; pt_events_used_ = 0; }
void RendererHIP::close_timing_window(hipStream_t s) { VR_HIP(hipEventRecord(ev1_, s)); timing_pending_ = true; }

// What a submit needs in place before its launches: the majorant table, the sample pool, the workspace and the moments; and the rate of the last sub-launch
// enqueued, read while the window that goes still holds its events.  Returns the samples of one sub-launch as the pool allows.
int RendererHIP::prepare_submit(const LaunchInputs& in, int first, int n, int n_tiles, int n_sky) {
    if (n <= 0) return 0;
    hipStream_t stream = in.stream;                              // (shadows the member: the launch goes where it was recorded for)
    update_majorants(in, density_grids.at(in.frame));
    // per-sample radiances live in a device pool; split the request so that one sub-launch fits the pool
    // (n_sky: clear tiles split off the submit.  They put nothing into the pool, so the pool is allocated for the n_tiles march tiles alone; the samples of a
    // sub-launch stay what sample_pool_bytes gives the WHOLE tile set, so that the split moves no sub-launch boundary a caller has sized by that budget.
    // n_tiles == 0: every tile is clear -- the sky kernel needs neither pool nor workspace, and takes the samples in one launch)
    int per_launch = n_tiles > 0 ? std::min(samples_per_launch(in, n_tiles + n_sky), n) : n;
    for (; n_tiles > 0;) {                                       // a pool that does not fit the free HBM: halve the sub-launch, never fail for it
        const size_t need = pathtrace_pool_floats(in.tuning, n_tiles, per_launch) * sizeof(float);
        if (pool_ && pool_->size_bytes() >= need) break;
        if (pool_) { VR_HIP(hipStreamSynchronize(stream)); pool_.reset(); }
        try { pool_ = make_device_buffer(need); break; }
        catch (const std::exception&) {
            (void)hipGetLastError();
            if (per_launch <= 1) throw;
            per_launch = std::max(1, per_launch / 2);
            if (per_launch > 32) per_launch -= per_launch % 32;
        }
    }
    if (!workspace_ && n_tiles > 0) {
        workspace_ = make_device_buffer(pathtrace_workspace_floats() * sizeof(float));
        // test hook: no path may depend on what its cold line held before the path wrote it (tests/test_gpu_parity.py)
        if (const char* e = std::getenv("VR_TEST_POISON_WORKSPACE"); e && *e == '1') VR_HIP(hipMemsetAsync(workspace_->get(), 0xFF, workspace_->size_bytes(), stream));
    }
    // test hook, value 2: NaN patterns in the workspace AND the sample pool before EVERY submit -- a frame must not depend on what an earlier frame (of this or of
    // another mode's kernels) left in either (tests/tools_determinism.py, test_frames_are_reproducible_on_every_compiled_instance)
    if (const char* e = std::getenv("VR_TEST_POISON_WORKSPACE"); e && *e == '2' && n_tiles > 0) {
        VR_HIP(hipMemsetAsync(workspace_->get(), 0xFF, workspace_->size_bytes(), stream));
        VR_HIP(hipMemsetAsync(pool_->get(), 0xFF, pool_->size_bytes(), stream));
    }
    if (in.launch_target_ms > 0 && in.kernel().item_integrator == 0) harvest_rate(false);      // what submit plans with
    // second moments: valid while every launch since sample 1 has kept them (a launch from sample 1 starts them afresh)
    if (in.variance && ensure_buffer(sized_.moments, color->size_bytes())) {
        VR_HIP(hipMemsetAsync(sized_.moments->get(), 0, color->size_bytes(), stream));
        if (first > 0) sized_.moments_n = -1;
    }
    sized_.moments_n = !in.variance ? -1 : (first == 0 ? n : (sized_.moments_n == first ? first + n : -1));
    return per_launch;
}

void RendererHIP::submit(const LaunchInputs& in, int first, int n, const int32_t* tiles, int n_tiles, int per_launch, const int32_t* sky, int n_sky, int n_see) {
    const SceneParams& P = in.P;
    last_sky_tiles = n_sky;
    last_see_through_tiles = n_see;
    hipStream_t stream = in.stream;
    const PathtraceKernel kernel = in.kernel();
    const bool pt_kernel = kernel.item_integrator == 0;          // launch_pathtrace records the events around the path-tracing kernel only
    // Launch sizing by time (round 4): no sub-launch is PLANNED to take longer than launch_target_ms.  The plan uses the rate of this renderer's last
    // finished sub-launch; when there is none for the current settings and the request is large, a short probe launch measures it first (one
    // synchronisation, once per change of settings).  A plan can still be off -- the rate is a property of the scene AND the view -- which costs nothing
    // but the bound: the kernel's watchdog watches progress, not duration (vr_pathtrace.h).
    const double px_samples = (double)(n_tiles + n_sky + n_see) * 256.0;        // samples per spp of this launch: the clear and see-through tiles' too -- the events whose time gives the
                                                                                 // rate span the path-tracing kernel AND the sky kernel, and the plan divides by the same count
    const uint64_t key = [&] {
        uint64_t h = kFnv1aStart;
        auto mix = [&h](const void* p, size_t nbytes) { h = fnv1a(p, nbytes, h); };
        const Uniforms& u = P.u;
        mix(&u.bounces, sizeof u.bounces); mix(u.vol_albedo, sizeof u.vol_albedo); mix(&u.vol_phase_g, sizeof u.vol_phase_g); mix(&u.vol_density_scale, sizeof u.vol_density_scale);
        mix(&u.use_tf, sizeof u.use_tf); mix(&u.tf_window_left, sizeof u.tf_window_left); mix(&u.tf_window_width, sizeof u.tf_window_width); mix(&u.integrator, sizeof u.integrator);
        mix(&u.has_emission, sizeof u.has_emission); mix(u.resolution, sizeof u.resolution); mix(u.vol_bb_min, sizeof u.vol_bb_min); mix(u.vol_bb_max, sizeof u.vol_bb_max);
        const size_t frame = in.frame; mix(&frame, sizeof frame); mix(&n_tiles, sizeof n_tiles);
        const uint64_t tfv = in.maj.tf_version; mix(&tfv, sizeof tfv);
        return h ? h : 1ull;
    }();
    auto cap_by_rate = [&](int planned) {
        if (in.launch_target_ms <= 0 || rate_samples_per_ms_ <= 0.0) return planned;
        const double cap = rate_samples_per_ms_ * (double)in.launch_target_ms / px_samples;
        int c = cap >= (double)planned ? planned : std::max(1, (int)cap);
        if (c > 32) c -= c % 32;
        return c;
    };
    int probe = 0;
    if (pt_kernel && in.launch_target_ms > 0) {
        const bool known = rate_samples_per_ms_ > 0.0 && rate_key_ == key;
        if (!known && px_samples * (double)std::min(per_launch, n) > (double)(1u << 26)) {
            rate_samples_per_ms_ = 0.0;                                          // measured under other settings: not a basis for a plan
            probe = (int)std::min<double>(32.0, std::max(1.0, (double)(1u << 24) / px_samples));
            probe = std::min(probe, n);
        } else per_launch = cap_by_rate(per_launch);
    }
    float* moments = in.variance ? sized_.moments->as<float>() : nullptr;
    for (int done = 0; done < n;) {
        if (n_tiles > 0) ++last_launches;
        const int m = probe > 0 ? probe : std::min(per_launch, n - done);
        hipEvent_t eb = nullptr, ee = nullptr;
        if (pt_kernel) {
            while (pt_events_.size() < pt_events_used_ + 2) { hipEvent_t e; VR_HIP(hipEventCreate(&e)); pt_events_.push_back(e); }
            eb = pt_events_[pt_events_used_]; ee = pt_events_[pt_events_used_ + 1];
            pt_events_used_ += 2;
        }
        int seed_samples = 0;
        const uint32_t* seed_table = kernel.reads_seed_table ? seed_table_for(P, first + done, m, stream, &seed_samples) : nullptr;
        launch_pathtrace(in.tuning, P, color->as<float>(), n_tiles > 0 ? pool_->as<float>() : nullptr, n_tiles > 0 ? workspace_->as<float>() : nullptr, status_->as<uint32_t>() + 1, tiles, n_tiles, first + 1 + done, m,
                         status_->as<uint32_t>(), stream, in.fast_math != 0, eb, ee, moments, seed_table, seed_samples, sky, n_sky, n_see);
        VR_HIP(hipGetLastError());
        done += m;
        if (pt_kernel) { rate_pending_samples_ = px_samples * (double)m; rate_pending_key_ = key; }
        if (probe > 0) {                                                         // the probe: wait for it, then plan the rest
            probe = 0;
            harvest_rate(true);
            per_launch = cap_by_rate(per_launch);
        }
    }
}

// ---- seed table (renderer.h) ------------------------------------------------------------------------------------------------------------------
int RendererHIP::seed_table_samples_for(long long mb, int w, int h) {
    if (mb <= 0 || w <= 0 || h <= 0) return 0;
    const long long per_sample = (long long)tile_count(w, h) * 256 * (long long)sizeof(uint32_t);
    return (int)std::min<long long>((mb << 20) / per_sample, 1 << 24);
}

void RendererHIP::drop_seed_table() {
    seed_table_.reset();                               // (freeing device memory waits for the work that reads it)
    seed_cap_ = seed_filled_ = 0;
    seed_failed_ = false;
}

const uint32_t* RendererHIP::seed_table_for(const SceneParams& P, int s0, int n, hipStream_t stream, int* samples) {
    *samples = 0;
    const int W = P.u.resolution[0], H = P.u.resolution[1], budget_mb = seed_table_budget_mb();
    if (seed_key_[0] != P.u.seed || seed_key_[1] != W || seed_key_[2] != H || seed_budget_mb_ != budget_mb || seed_max_samples_ != seed_table_max_samples) {
        drop_seed_table();
        seed_key_[0] = P.u.seed; seed_key_[1] = W; seed_key_[2] = H; seed_budget_mb_ = budget_mb; seed_max_samples_ = seed_table_max_samples;
    }
    int max_samples = seed_table_samples_for(budget_mb, W, H);
    if (seed_table_max_samples > 0) max_samples = std::min(max_samples, seed_table_max_samples);
    if (max_samples <= 0 || (seed_failed_ && !seed_table_) || s0 < 0 || n <= 0) return nullptr;
    const size_t per_sample = (size_t)tile_count(W, H) * 256u * sizeof(uint32_t);
    const int want = (int)std::min<long long>((long long)s0 + n, max_samples);
    if (!seed_event_) VR_HIP(hipEventCreateWithFlags(&seed_event_, hipEventDisableTiming));
    // a launch on another stream than the last fill's: ordered behind that fill
    if (seed_table_ && seed_filled_ > 0 && stream != seed_stream_) { VR_HIP(hipStreamWaitEvent(stream, seed_event_, 0)); seed_stream_ = stream; }
    if (want > seed_cap_ && !seed_failed_) {
        // grow: at least double (a caller that asks for one sample more per call does not pay an allocation per call), the filled prefix moves over
        const int cap = (int)std::min<long long>(max_samples, std::max<long long>(want, 2ll * seed_cap_));
        DeviceBufferPtr grown;
        try { grown = make_device_buffer((size_t)cap * per_sample); }
        catch (const std::exception& e) {
            (void)hipGetLastError();
            seed_failed_ = true;
            static std::once_flag once;
            std::call_once(once, [&] { fprintf(stderr, "volren_amd: note: no memory for the path-seed table (%zu MiB: %s); new paths hash their seeds (slower; results unchanged)\n", ((size_t)cap * per_sample) >> 20, e.what()); });
            if (!seed_table_) return nullptr;
        }
        if (grown) {
            // test hook (see submit): no launch may depend on what an entry held before its fill
            if (const char* e = std::getenv("VR_TEST_POISON_WORKSPACE"); e && *e == '2') VR_HIP(hipMemsetAsync(grown->get(), 0xFF, grown->size_bytes(), stream));
            if (seed_filled_ > 0) VR_HIP(hipMemcpyAsync(grown->get(), seed_table_->get(), (size_t)seed_filled_ * per_sample, hipMemcpyDeviceToDevice, stream));
            if (seed_table_) VR_HIP(hipStreamSynchronize(stream));      // the copy has left the old buffer before it goes
            seed_table_ = grown;
            seed_cap_ = cap;
        }
    }
    const int upto = std::min(want, seed_cap_);
    if (upto > seed_filled_) {
        launch_seed_fill(seed_table_->as<uint32_t>(), (uint32_t)P.u.seed, W, H, seed_filled_, upto, stream);
        VR_HIP(hipGetLastError());
        VR_HIP(hipEventRecord(seed_event_, stream));
        seed_stream_ = stream;
        seed_filled_ = upto;
        ++seed_fills_;
    }
    *samples = seed_filled_;
    return seed_filled_ > 0 ? seed_table_->as<uint32_t>() : nullptr;
}

// rate of the last path-tracing sub-launch that was enqueued, if it has finished (wait: block until it has)
void RendererHIP::harvest_rate(bool wait) {
    if (rate_pending_samples_ <= 0.0 || pt_events_used_ < 2) return;
    hipEvent_t eb = pt_events_[pt_events_used_ - 2], ee = pt_events_[pt_events_used_ - 1];
    if (wait) VR_HIP(hipEventSynchronize(ee));
    else if (hipEventQuery(ee) != hipSuccess) { (void)hipGetLastError(); return; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, eb, ee) != hipSuccess || !(ms > 0.f)) { (void)hipGetLastError(); return; }
    rate_samples_per_ms_ = rate_pending_samples_ / (double)ms;
    rate_key_ = rate_pending_key_;
    rate_pending_samples_ = 0.0;
}

// One more sample (src/renderer.cpp:78-145).  The reference issues one dispatch per call; here a call records its launch inputs and consecutive calls that
// record the same bytes are launched together (renderer.h).  What a caller can observe is unchanged: `sample` advances by one per call, invalid
// state throws at the call, and every way of looking at the frame launches the recorded samples first -- with the values they were recorded with.
void RendererHIP::trace() {
    if (ragged())
        throw std::runtime_error("trace: the frame holds per-tile sample counts of render_adaptive (a ragged frame): reset(), or continue with render_adaptive");
    if (!coalesce_trace) { flush_pending(); LaunchInputs in; capture(in); submit_tile_set(in, sample, 1); sample += 1; return; }
    LaunchInputs now;
    capture(now);
    if (pending_n_ > 0 && (sample != pending_first_ + pending_n_ || !now.same_launch_as(pending_))) flush_pending();
    if (pending_n_ == 0) {
        pending_ = std::move(now);
        pending_first_ = sample;
        pending_cap_ = samples_per_launch(pending_, tile_set_size());     // a full sub-launch goes out at once: the GPU works while the caller keeps calling
    }
    ++pending_n_;
    ++sample;
    if (pending_n_ >= pending_cap_) flush_pending();
}

void RendererHIP::flush_pending() {
    if (pending_n_ <= 0) return;
    const int n = pending_n_, first = pending_first_;
    pending_n_ = 0;                                              // (first: submit may throw, and must not be retried with half of it enqueued)
    LaunchInputs in = std::move(pending_);
    pending_ = LaunchInputs{};
    submit_tile_set(in, first, n);
}

void RendererHIP::render(int n) {
    flush_pending();
    if (ragged()) throw std::runtime_error("render: the frame holds per-tile sample counts of render_adaptive (a ragged frame): reset(), or continue with render_adaptive");
    if (n <= 0) n = sppx - sample;
    if (n <= 0) return;
    LaunchInputs in;
    capture(in);
    submit_tile_set(in, sample, n);
    sample += n;
}

void RendererHIP::draw() {
    flush_pending();
    if (!color) return;
    draw_from(*color);
}

void RendererHIP::draw_from(const DeviceBuffer& src) {
    ensure_buffer(display, src.size_bytes());
    VR_HIP(hipMemcpyAsync(display->get(), src.get(), src.size_bytes(), hipMemcpyDeviceToDevice, stream));
    if (tonemapping) {
        launch_tonemap(display->as<float>(), (int32_t)(src.size_bytes() / (4 * sizeof(float))), 1, tonemap_exposure, tonemap_gamma, stream);      // src's own texels: upsample()'s frame is larger than the renderer's
        VR_HIP(hipGetLastError());
    }
}

double RendererHIP::last_kernel_ms() {
    flush_pending();
    if (timing_pending_) {
        VR_HIP(hipEventSynchronize(ev1_));
        float ms = 0.f;
        VR_HIP(hipEventElapsedTime(&ms, ev0_, ev1_));
        last_ms_ = (double)ms;
        last_pathtrace_ms_ = 0.0;
        for (size_t i = 0; i + 1 < pt_events_used_; i += 2)
            if (hipEventElapsedTime(&ms, pt_events_[i], pt_events_[i + 1]) == hipSuccess) last_pathtrace_ms_ += (double)ms;
        (void)hipGetLastError();
        timing_pending_ = false;
    }
    return last_ms_;
}

double RendererHIP::last_pathtrace_ms() { (void)last_kernel_ms(); return last_pathtrace_ms_; }

void RendererHIP::sched_stats(bool enable, unsigned long long out[32]) {
    flush_pending();
    if (out) {
        for (int i = 0; i < 32; ++i) out[i] = 0ull;
        if (stats_) { VR_HIP(hipStreamSynchronize(stream)); stats_->download(out, 32 * sizeof(unsigned long long), stream); }
    }
    if (enable) {
        if (!stats_) stats_ = make_device_buffer((32 + 3 * 8192) * sizeof(unsigned long long));      // 32 counters + (begin, queue empty, end) per wavefront (vr_pathtrace.h kStatsWaveBase)
        VR_HIP(hipMemsetAsync(stats_->get(), 0, stats_->size_bytes(), stream));
        tuning.stats = stats_->as<unsigned long long>();
    } else {
        tuning.stats = nullptr;
    }
}

void RendererHIP::wave_timeline(unsigned long long* out, size_t n_words) {
    if (!stats_) throw std::runtime_error("wave_timeline: statistics are not enabled");
    flush_pending();
    VR_HIP(hipStreamSynchronize(stream));
    const size_t have = stats_->size_bytes() / sizeof(unsigned long long) - 32;
    std::vector<unsigned long long> all(32 + have);
    stats_->download(all.data(), all.size() * sizeof(unsigned long long), stream);
    for (size_t i = 0; i < n_words; ++i) out[i] = i < have ? all[32 + i] : 0ull;
}

void RendererHIP::synchronize() { flush_pending(); VR_HIP(hipStreamSynchronize(stream)); }

void RendererHIP::download(float* rgba) {
    if (!color) throw std::runtime_error("RendererHIP::download: no framebuffer");
    flush_pending();
    color->download(rgba, color->size_bytes(), stream);
}
void RendererHIP::download_display(float* rgba) const {
    if (!display) throw std::runtime_error("RendererHIP::download_display: draw() first");
    display->download(rgba, display->size_bytes(), stream);
}

// The feature pass reads the scene as a render() would: capture() (which also decodes the float atlas under a transfer function) and the majorant
// table of the current density scale and LUT.  It runs the lane code of the run-time kernel variant, which reads every grid from its own atlas
// (unpair_views).
// feature_scene: P = that scene, and nothing else -- upsample() marches a pass at another resolution into a buffer of its own with it.
// begin_feature_pass: what both feature passes do before their launch -- P = that scene; the feature buffer exists (zero-filled when it is new); returns the
// number of tiles of the tile set.
void RendererHIP::feature_scene(SceneParams& P) {
    flush_pending();
    LaunchInputs in;
    capture(in);
    update_majorants(in, density_grids.at(in.frame));
    P = in.P;
    unpair_views(P, in.frame);
}

// the scene with each grid's own atlas: the views of a frame whose grids share a paired atlas, made again without it (the majorant layout stays the one the table is built in)
void RendererHIP::unpair_views(SceneParams& P, size_t frame) const {
    if (!P.paired) return;
    P.density = make_view(density_grids.at(frame), false, P.density.maj_blocked != 0);
    P.emission = make_view(emission_grids.at(frame), false);
    P.paired = 0;
}

int RendererHIP::begin_feature_pass(SceneParams& P) {
    feature_scene(P);
    const size_t bytes = (size_t)resolution.x * resolution.y * 8 * sizeof(float);
    if (ensure_buffer(sized_.features, bytes)) {
        VR_HIP(hipMemsetAsync(sized_.features->get(), 0, bytes, stream));
    }
    return tile_set_size();
}

void RendererHIP::render_features(int spp) {
    if (spp <= 0) throw std::runtime_error("render_features: spp must be positive");
    SceneParams P;
    const int n_tiles = begin_feature_pass(P);
    sized_.pass = 1; sized_.rays = 0;
    launch_features(P, tiles_dev_ ? tiles_dev_->as<int32_t>() : nullptr, n_tiles, spp, sized_.features->as<float>(), status_->as<uint32_t>(), stream);
    VR_HIP(hipGetLastError());
}

// The expected values of the same features (vr_expected.h), into the same buffer: whatever reads the feature buffer reads either pass's output.
void RendererHIP::render_features_expected(int rays) {
    if (rays < 1 || rays > kExpectedMaxRays) throw std::runtime_error("render_features_expected: rays must be 1.." + std::to_string(kExpectedMaxRays));
    SceneParams P;
    const int n_tiles = begin_feature_pass(P);
    sized_.pass = 2; sized_.rays = rays;
    launch_expected(P, tiles_dev_ ? tiles_dev_->as<int32_t>() : nullptr, n_tiles, rays, sized_.features->as<float>());
}

void RendererHIP::launch_expected(const SceneParams& P, const int32_t* tiles, int n_tiles, int rays, float* out) {
    ClearTable clear = { nullptr, { 0, 0, 0 } };
    const bool cubic = expected_field != 0 && !P.u.use_tf;       // the tracker's field: under a LUT the trilinear one (vr_expected.h)
    if (expected_skip) clear = clear_table_of(density_grids.at(volume->grid_frame_counter), P.density, cubic ? 2 : 1);
    expected_stats_valid_ = false;
    unsigned long long* counters = nullptr;
    if (expected_stats) {
        ensure_buffer(expected_stats_, 4 * sizeof(unsigned long long));
        VR_HIP(hipMemsetAsync(expected_stats_->get(), 0, expected_stats_->size_bytes(), stream));
        counters = expected_stats_->as<unsigned long long>();
    }
    launch_features_expected(P, tiles, n_tiles, rays, out, stream, &clear, counters, cubic);
    VR_HIP(hipGetLastError());
    expected_stats_valid_ = counters != nullptr;
}

// The clear-distance table of a density grid (vr_clear.h), made by the first pass that asks for it: the table lives with the grid's device arrays, so
// commit() -- which every change of the volume goes through -- leaves the new grids without one, and each frame of an animation keeps its own.
ClearTable RendererHIP::clear_table_of(BrickGridHIP& g, const GridView& view, int reach) {
    ClearTable t;
    clear_cells(view, t.n);
    const size_t cells = (size_t)t.n[0] * (size_t)t.n[1] * (size_t)t.n[2];
    DeviceBufferPtr& cached = g.clear_table[reach == 2 ? 1 : 0];        // one table per grid and reach
    if (!cached && cells > 0) {
        auto table = make_device_buffer(cells);
        DeviceBuffer scratch(cells);
        launch_clear_table(view, table->as<uint8_t>(), scratch.as<uint8_t>(), stream, reach == 2 ? 2 : 1);
        VR_HIP(hipGetLastError());
        VR_HIP(hipStreamSynchronize(stream));                   // the scratch half goes with this scope
        cached = table;
    }
    t.d = cached ? cached->as<uint8_t>() : nullptr;
    return t;
}

void RendererHIP::expected_stats_read(uint64_t out[4]) {
    if (!expected_stats_valid_ || !expected_stats_) throw std::runtime_error("expected_stats: the last expected-value pass did not count (set expected_stats 1 before it)");
    unsigned long long v[4];
    expected_stats_->download(v, sizeof v, stream);
    for (int i = 0; i < 4; ++i) out[i] = (uint64_t)v[i];
}

void RendererHIP::expected_clear_table(uint8_t* out, int cells[3]) {
    flush_pending();
    LaunchInputs in;
    capture(in);                                                 // the scene as the pass reads it (the decoded float atlas under a transfer function)
    BrickGridHIP& g = density_grids.at(in.frame);
    const int reach = expected_field != 0 && !in.P.u.use_tf ? 2 : 1;      // the table the current setting marches with (launch_expected)
    const ClearTable t = clear_table_of(g, make_view(g, false, in.P.density.maj_blocked != 0), reach);
    for (int i = 0; i < 3; ++i) cells[i] = t.n[i];
    const DeviceBufferPtr& table = g.clear_table[reach - 1];
    if (out && table) table->download(out, table->size_bytes(), stream);
}

// Test hook (vr_probe.h).  The scene as the next launch reads it: capture() and the majorant table as submit() / render_features() bring them up to date.  A PAIR form
// reads the views of the kernel compiled for the paired atlas; every other form the grids' own atlases, as the run-time variant and the feature pass do.
void RendererHIP::probe(int what, int form, const uint32_t* in, float* out, size_t n) {
    if (!in || !out) throw std::runtime_error("probe: null array");
    if (n > (size_t)1 << 28) throw std::runtime_error("probe: more than 2^28 items");
    flush_pending();
    LaunchInputs li;
    capture(li);
    update_majorants(li, density_grids.at(li.frame));
    SceneParams P = li.P;
    if (const char* why = probe_form_error(P, what, form)) throw std::runtime_error(std::string("probe: this scene cannot serve that form: ") + why);
    if (const char* why = probe_items_error(P, what, form, in, n)) throw std::runtime_error(std::string("probe: bad item: ") + why);
    if (probe_decode_form(what, form).pair == 0) unpair_views(P, li.frame);
    if (n == 0) return;
    const size_t in_bytes = n * kProbeInWords * sizeof(uint32_t), out_bytes = n * (size_t)probe_out_words(what) * sizeof(float);
    DeviceBuffer din(in_bytes), dout(out_bytes);
    din.upload(in, in_bytes, stream);
    launch_probe(P, what, form, din.as<uint32_t>(), dout.as<float>(), (uint32_t)n, stream);
    VR_HIP(hipGetLastError());
    dout.download(out, out_bytes, stream);
    VR_HIP(hipStreamSynchronize(stream));
}

// Test hook (vr_path_probe.h): the scene as probe() takes it.  The instance is judged on the views the launch would get (the paired ones where they exist).
void RendererHIP::path_probe(int kind, int form, const uint32_t* in, uint32_t* out, size_t n) {
    if (!in || !out) throw std::runtime_error("path_probe: null array");
    if (n > (size_t)1 << 24) throw std::runtime_error("path_probe: more than 2^24 items");
    flush_pending();
    LaunchInputs li;
    capture(li);
    update_majorants(li, density_grids.at(li.frame));
    SceneParams P = li.P;
    if (const char* why = path_probe_form_error(P, kind, form)) throw std::runtime_error(std::string("path_probe: this scene cannot serve that form: ") + why);
    if (const char* why = path_probe_items_error(P, kind, form, in, n)) throw std::runtime_error(std::string("path_probe: bad item: ") + why);
    if (!(kind == PATH_SEGMENT && (form == 4 || form == 5))) unpair_views(P, li.frame);
    if (n == 0) return;
    const size_t in_bytes = n * (size_t)path_probe_in_words(kind) * sizeof(uint32_t), out_bytes = n * (size_t)path_probe_out_words(kind) * sizeof(uint32_t);
    DeviceBuffer din(in_bytes), dout(out_bytes);
    din.upload(in, in_bytes, stream);
    launch_path_probe(P, kind, form, din.as<uint32_t>(), dout.as<uint32_t>(), (uint32_t)n, stream);
    VR_HIP(hipGetLastError());
    dout.download(out, out_bytes, stream);
    VR_HIP(hipStreamSynchronize(stream));
}

// Test hook (include/volren_amd.h vr_filter_probe).  Every array goes through a DeviceBuffer of this call's own; nothing of sized_ is read or written.  The two
// scene-bound stages take the scene as run_resolve and upsample take it.
void RendererHIP::filter_probe(int stage, int W, int H, const void* const* in, float* const* out, const float* params) {
    flush_pending();
    const size_t px = (size_t)W * (size_t)H, F4 = sizeof(float);
    const DenoiseSigma sg{ params[0], params[1], params[2], params[3], params[4] };
    const int32_t i0 = (int32_t)params[5], i1 = (int32_t)params[8];
    const float x = params[6], tau = params[7];
    const bool demod = params[35] != 0.0f;            // vr_demod.h: the DEMOD instance of prepare, split, merge and upsample
    std::vector<std::unique_ptr<DeviceBuffer>> held;
    auto fresh = [&](size_t bytes) { held.push_back(std::make_unique<DeviceBuffer>(bytes)); return held.back().get(); };
    auto up = [&](const void* src, size_t bytes) -> DeviceBuffer* {       // nullptr stays nullptr
        if (!src) return nullptr;
        DeviceBuffer* b = fresh(bytes);
        b->upload(src, bytes, stream);
        return b;
    };
    auto fl = [](DeviceBuffer* b) { return b ? b->as<float>() : nullptr; };
    struct Back { DeviceBuffer* b; float* to; size_t bytes; };
    std::vector<Back> back;
    auto down = [&](float* to, size_t bytes) -> DeviceBuffer* {           // an output: zeroed, so that a word the launch leaves alone reads 0
        if (!to) return nullptr;
        DeviceBuffer* b = fresh(bytes);
        VR_HIP(hipMemsetAsync(b->get(), 0, bytes, stream));
        back.push_back({ b, to, bytes });
        return b;
    };
    switch (stage) {
    case 0: {
        const size_t tiles = (size_t)tile_count(W, H);
        DeviceBuffer *m = up(in[0], px * 4 * F4), *f = up(in[1], px * 8 * F4), *c = up(in[2], tiles * sizeof(int32_t));
        DeviceBuffer *v = down(out[0], px * F4), *g = down(out[1], px * 8 * F4);
        launch_denoise_prepare(fl(m), fl(f), W, H, i0, x, c ? c->as<int32_t>() : nullptr, fl(v), fl(g), stream, demod);
        break;
    }
    case 1: {
        DeviceBuffer *c = up(in[0], px * 4 * F4), *v = up(in[1], px * F4), *g = up(in[2], px * 8 * F4);
        DeviceBuffer *oc = down(out[0], px * 4 * F4), *ov = down(out[1], px * F4);
        launch_denoise_atrous(fl(c), fl(v), fl(g), W, H, i0, sg, fl(oc), fl(ov), stream);
        break;
    }
    case 2: {
        TemporalPass t;
        DeviceBuffer* v = up(in[1], px * F4);                            // read and written in place, as dn_var[0] is
        back.push_back({ v, out[2], px * F4 });
        t.color = fl(up(in[0], px * 4 * F4)); t.v = fl(v); t.guide = fl(up(in[2], px * 8 * F4));
        t.hist_color = fl(up(in[3], px * 4 * F4)); t.hist_record = fl(up(in[4], px * 4 * F4)); t.hist_moments = fl(up(in[5], px * 4 * F4));
        t.same_cam = i1 != 0;
        memcpy(&t.cur, params + 9, 13 * F4); memcpy(&t.prev, params + 22, 13 * F4);
        t.W = W; t.H = H; t.alpha = x; t.tau = tau; t.sigma = sg;
        t.out_color = fl(down(out[0], px * 4 * F4)); t.out_record = fl(down(out[1], px * 4 * F4)); t.out_moments = fl(down(out[3], px * 4 * F4));
        if (tau > 0.0f) {
            DeviceBuffer* scratch = fresh(px * 8 * F4);
            VR_HIP(hipMemsetAsync(scratch->get(), 0, px * 8 * F4, stream));
            t.scratch = scratch->as<float>();
        }
        launch_denoise_temporal(t, stream);
        if (tau > 0.0f) {
            VR_HIP(hipGetLastError());
            VR_HIP(hipMemcpyAsync(out[4], t.scratch + px * 4, px * 4 * F4, hipMemcpyDeviceToHost, stream));
        }
        break;
    }
    case 3: {
        LaunchInputs li;
        capture(li);
        DeviceBuffer *fb = up(in[0], px * 4 * F4), *f = up(in[1], px * 8 * F4);
        DeviceBuffer *B = down(out[0], px * 4 * F4), *Pq = down(out[1], px * 4 * F4), *y = down(out[2], px * 4 * F4);
        launch_resolve(li.P, fl(fb), fl(f), i0, fl(B), fl(Pq), fl(y), stream);
        break;
    }
    case 4: {
        DeviceBuffer *y = up(in[0], px * 4 * F4), *B = up(in[1], px * 4 * F4), *f = up(in[2], px * 8 * F4);
        launch_layers_split(fl(y), fl(B), fl(f), W, H, fl(down(out[0], px * 4 * F4)), stream, demod);
        break;
    }
    case 5: {
        DeviceBuffer *Fq = up(in[0], px * 4 * F4), *B = up(in[1], px * 4 * F4), *f = up(in[2], px * 8 * F4);
        DeviceBuffer *o = down(out[0], px * 4 * F4), *L = down(out[1], px * 4 * F4);
        launch_layers_merge(fl(Fq), fl(B), fl(f), W, H, fl(o), fl(L), stream, demod);
        break;
    }
    case 6: {
        DeviceBuffer *S = up(in[0], px * 4 * F4), *g = up(in[1], px * 8 * F4);
        launch_denoise_regress(fl(S), fl(g), W, H, sg, x, fl(down(out[0], px * 4 * F4)), stream);
        break;
    }
    case 7: {
        const int32_t f = i1;
        const size_t hi = px * (size_t)f * (size_t)f;
        SceneParams P;
        feature_scene(P);
        P.u.resolution[0] = f * W; P.u.resolution[1] = f * H;
        DeviceBuffer *l = up(in[0], px * 4 * F4), *g = up(in[1], px * 8 * F4), *hf = up(in[2], hi * 8 * F4);
        DeviceBuffer *o = down(out[0], hi * 4 * F4), *L = down(out[1], hi * 4 * F4);
        launch_upsample(P, fl(l), fl(g), W, H, f, fl(hf), i0, sg, fl(o), fl(L), stream, demod);
        break;
    }
    case 8: {
        DeviceBuffer *fb = up(in[0], px * 4 * F4), *m = up(in[1], px * 4 * F4), *t = up(in[2], (size_t)i0 * sizeof(int32_t)), *c = up(in[3], (size_t)i0 * sizeof(int32_t));
        launch_adaptive_error(fl(fb), fl(m), t->as<int32_t>(), c->as<int32_t>(), i0, W, H, fl(down(out[0], (size_t)i0 * F4)), stream);
        break;
    }
    default: throw std::invalid_argument("filter_probe: unknown stage");
    }
    VR_HIP(hipGetLastError());
    for (const Back& b : back) b.b->download(b.to, b.bytes, stream);
    VR_HIP(hipStreamSynchronize(stream));
}

// the common body of the download_* of whole buffers: the refusal comes before the flush
void RendererHIP::download_whole(const DeviceBufferPtr& b, float* out, const char* absent) {
    if (!b) throw std::runtime_error(absent);
    flush_pending();
    b->download(out, b->size_bytes(), stream);
}

void RendererHIP::download_features(float* out) { download_whole(sized_.features, out, "features: no feature pass since the last resize (call render_features first)"); }

void RendererHIP::check_moments(const char* who) {
    if (ragged() && sized_.moments) return;                 // render_adaptive keeps the moments of every launch: they cover each tile's own count
    if (sample < 1 || !sized_.moments || sized_.moments_n != sample)
        throw std::runtime_error(std::string(who) + ": the moments do not cover samples 1.." + std::to_string(sample) +
                                 " (variance was off for some of them, e.g. switched on mid-frame): reset() and render with variance = 1");
}

void RendererHIP::download_variance(float* rgba) {
    flush_pending();
    check_moments("variance");
    sized_.moments->download(rgba, sized_.moments->size_bytes(), stream);
    const bool per_tile = ragged();                   // each tile's own count and factor
    const int W = resolution.x, H = resolution.y;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int32_t c = per_tile ? tile_n_[(size_t)tile_of_pixel(x, y, W)] : sample;
            const float f = variance_scale(c);
            float* px = rgba + 4 * ((size_t)y * W + x);
            for (int k = 0; k < 4; ++k) px[k] = c >= 2 ? px[k] * f : 0.0f;
        }
}

// The a-trous denoiser (vr_denoise.h) on whole frames: prepare (variance of the mean, guide) once, then `denoise_iterations` passes at steps
// 1, 2, 4, ...  Iteration 0 reads the framebuffer itself; colour and variance ping-pong between buffers of their own, and the last iteration
// writes `denoised` (N = 0: a copy of the framebuffer).
// temporal (denoise_temporal, vr_temporal.h): between prepare and the iterations the frame is blended with the history, and the iterations start
// from the new history's colour and variance instead.  layers (denoise_layers, vr_layers.h): the frame all of this reads is the resolved frame's
// scattered layer S (resolve, then a split), the last iteration writes a buffer F of its own, and a merge writes `denoised` and the layer from F.
// regress (denoise_filter, vr_regress.h; with layers only): one kernel from what iteration 0 would read to F takes the iterations' place.
// demod (denoise_demodulate, vr_demod.h; with layers only): split, prepare and merge run their DEMOD instances; the launches and buffers are the same.
// Every buffer the call needs is allocated before its first launch, so a failed allocation
// leaves the last result and the history as they were.
static const char* const kDemodulateRange = "denoise_demodulate: 0 (the filter reads the scattered layer as it is) or 1 (divided by the guide's albedo, multiplied back afterwards; needs denoise_layers = 1)";
void RendererHIP::denoise() { run_denoise("denoise", false); }
void RendererHIP::denoise_temporal() { run_denoise("denoise_temporal", true); }

void RendererHIP::run_denoise(const char* who, bool temporal, bool whole_frame_gathered) {
    flush_pending();
    const std::string me = std::string(who) + ": ";
    if (!tiles_host_.empty() && !whole_frame_gathered) throw std::runtime_error(me + "a tile subset is set (set_tiles); the filter needs every pixel's neighbours and runs on whole frames only");
    if (!sized_.features) throw std::runtime_error(me + "no feature pass since the last resize (call render_features first)");
    if (sample < 1) throw std::runtime_error(me + "the framebuffer holds no samples (sample < 1)");
    check_moments(who);
    if (temporal && denoise_moments != 0 && denoise_reject > 0.0f)
        throw std::runtime_error(me + "denoise_moments = 1 and denoise_reject > 0 do not go together: the rejection statistic needs the frames' sample variance, and the moment variance of 1-spp frames is too heavy-tailed for it (DESIGN.md 5)");
    if (denoise_resolve != 0) check_resolve(me + "denoise_resolve = 1: ", whole_frame_gathered);
    const bool layers = denoise_layers != 0;          // vr_layers.h: the filter runs on the scattered layer, between a split and a merge
    if (layers) check_resolve(me + "denoise_layers = 1: ", whole_frame_gathered);
    const bool regress = denoise_filter != 0;         // vr_regress.h: one pass of local regression in the place of the iterations
    if (regress && !layers) throw std::runtime_error(me + "denoise_filter = 1 needs denoise_layers = 1: the regression is defined on the scattered layer S with S.a = the expected coverage");
    if (regress && !regress_ridge_ok(denoise_ridge)) throw std::runtime_error(me + "denoise_ridge must be 0 (zero order) or in [2^-20, 2^20]");
    if (denoise_demodulate != 0 && denoise_demodulate != 1) throw std::runtime_error(me + kDemodulateRange);
    const bool demod = denoise_demodulate != 0;       // vr_demod.h: the DEMOD instances of split, prepare and merge
    if (demod && !layers) throw std::runtime_error(me + "denoise_demodulate = 1 needs denoise_layers = 1: the albedo divides the scattered layer S, not a frame with the background in it");
    const int32_t* counts = nullptr;                  // a ragged frame: every tile's own count (uploaded here: waits for the frame)
    if (ragged()) {
        for (int32_t c : tile_n_)
            if (c < 1) throw std::runtime_error(me + "a tile of the frame holds no samples (sample < 1 there: render_adaptive over a tile subset from sample 0)");
        const size_t bytes = tile_n_.size() * sizeof(int32_t);
        ensure_buffer(sized_.tile_n_dev, bytes);
        sized_.tile_n_dev->upload(tile_n_.data(), bytes, stream);
        counts = sized_.tile_n_dev->as<int32_t>();
    }
    const int32_t W = resolution.x, H = resolution.y, N = denoise_iterations;
    if ((size_t)W * (size_t)H * 2u > (size_t)INT32_MAX) throw std::runtime_error(me + "frame too large (32-bit pixel indices)");
    if (N < 0 || N > kDenoiseMaxIterations) throw std::runtime_error(me + "denoise_iterations out of range");
    const size_t px = (size_t)W * H;
    Sized::History& hist = sized_.hist;
    // a history without moment records cannot continue one with them, nor the other way round (denoise_moments set as a field, past set_denoise_moments);
    // nor one of composites one of layers, nor a demodulated layer a plain one (denoise_layers, denoise_demodulate set as fields, past their setters)
    if (temporal && hist.cur >= 0 && ((hist.moments[hist.cur] != nullptr) != (denoise_moments != 0) || hist.layers != layers || hist.demod != demod)) drop_history();
    const int to = hist.cur < 0 ? 0 : 1 - hist.cur;      // the half of the history pair this call writes
    const bool reject = temporal && denoise_reject > 0.0f;      // vr_temporal.h steps 2a, 3a: the fetch / resolve pair instead of the one kernel
    const bool moments = temporal && denoise_moments != 0;      // vr_moments.h: the temporal kernel with the moment records, then the variance kernel
    if (moments) ensure_buffer(hist.moments[to], px * 4 * sizeof(float));
    if (temporal) { ensure_buffer(hist.color[to], px * 4 * sizeof(float)); ensure_buffer(hist.record[to], px * 4 * sizeof(float)); }
    if (reject) ensure_buffer(sized_.dn_reject, px * 8 * sizeof(float));
    ensure_buffer(sized_.dn_guide, px * 8 * sizeof(float));
    ensure_buffer(sized_.dn_var[0], px * sizeof(float));
    ensure_buffer(sized_.denoised, px * 4 * sizeof(float));
    const int32_t passes = regress ? 0 : N;           // the a-trous iterations this call launches
    if (passes >= 2) { ensure_buffer(sized_.dn_var[1], px * sizeof(float)); ensure_buffer(sized_.dn_color[0], px * 4 * sizeof(float)); }
    if (passes >= 3) ensure_buffer(sized_.dn_color[1], px * 4 * sizeof(float));
    if (layers) { ensure_buffer(sized_.ly_split, px * 4 * sizeof(float)); ensure_buffer(sized_.ly_filtered, px * 4 * sizeof(float)); ensure_buffer(sized_.layer, px * 4 * sizeof(float)); }
    const float vscale = variance_scale(sample);      // download_variance's factor
    if (denoise_resolve != 0 || layers) run_resolve();      // vr_resolve.h: the filter starts from y, with the frame's own variance
    const DeviceBuffer* frame = denoise_resolve != 0 ? sized_.resolved.get() : color.get();
    if (layers) {                                     // ... or from y's scattered layer S; the last iteration then writes F, and the merge writes `denoised` and the layer
        launch_layers_split(sized_.resolved->as<float>(), sized_.rs_bg->as<float>(), sized_.features->as<float>(), W, H, sized_.ly_split->as<float>(), stream, demod);
        VR_HIP(hipGetLastError());
        frame = sized_.ly_split.get();
    }
    DeviceBuffer* const result = layers ? sized_.ly_filtered.get() : sized_.denoised.get();
    sized_.layer_guided = false;                      // the guide is this call's from here on; a call with layers pairs it with its layer below
    launch_denoise_prepare(sized_.moments->as<float>(), sized_.features->as<float>(), W, H, sample, vscale, counts, sized_.dn_var[0]->as<float>(), sized_.dn_guide->as<float>(), stream, demod);
    VR_HIP(hipGetLastError());
    const DenoiseSigma sg = sigma();
    const DeviceBuffer* first = frame;                // what iteration 0 reads
    if (temporal) {
        TemporalCamera cur;
        memset(&cur, 0, sizeof cur);
        copy3(cur.pos, camera.pos);
        const mat3 ct = camera.view_inverse();
        memcpy(cur.m, ct.m, sizeof ct.m);
        cur.cam_z = camera_z(camera.fov_degree);
        const bool have = hist.cur >= 0;
        TemporalPass t;
        t.color = frame->as<float>(); t.v = sized_.dn_var[0]->as<float>(); t.guide = sized_.dn_guide->as<float>();
        if (have) { t.hist_color = hist.color[hist.cur]->as<float>(); t.hist_record = hist.record[hist.cur]->as<float>(); }
        if (have && moments) t.hist_moments = hist.moments[hist.cur]->as<float>();
        t.same_cam = have && memcmp(&cur, &hist.cam, sizeof cur) == 0;
        t.cur = cur; t.prev = have ? hist.cam : cur;
        t.W = W; t.H = H; t.alpha = denoise_alpha;
        if (reject) { t.tau = denoise_reject; t.scratch = sized_.dn_reject->as<float>(); }
        t.sigma = sg;
        t.out_color = hist.color[to]->as<float>(); t.out_record = hist.record[to]->as<float>();
        if (moments) t.out_moments = hist.moments[to]->as<float>();
        launch_denoise_temporal(t, stream);
        VR_HIP(hipGetLastError());
        sized_.reject_stat = reject;
        hist.cur = to; hist.cam = cur; hist.layers = layers; hist.demod = demod;
        first = hist.color[to].get();
    }
    if (N == 0) VR_HIP(hipMemcpyAsync(result->get(), first->get(), first->size_bytes(), hipMemcpyDeviceToDevice, stream));
    if (regress && N > 0) {                           // the iterations' input in, the merge's input out: no ping-pong, no variance
        launch_denoise_regress(first->as<float>(), sized_.dn_guide->as<float>(), W, H, sg, denoise_ridge, result->as<float>(), stream);
        VR_HIP(hipGetLastError());
    }
    for (int32_t k = 0; k < passes; ++k) {
        const float* cin = k == 0 ? first->as<float>() : sized_.dn_color[(k - 1) & 1]->as<float>();
        float* cout = k == N - 1 ? result->as<float>() : sized_.dn_color[k & 1]->as<float>();
        float* vout = k == N - 1 ? nullptr : sized_.dn_var[(k + 1) & 1]->as<float>();
        launch_denoise_atrous(cin, sized_.dn_var[k & 1]->as<float>(), sized_.dn_guide->as<float>(), W, H, 1 << k, sg, cout, vout, stream);
        VR_HIP(hipGetLastError());
    }
    if (layers) {
        launch_layers_merge(result->as<float>(), sized_.rs_bg->as<float>(), sized_.features->as<float>(), W, H, sized_.denoised->as<float>(), sized_.layer->as<float>(), stream, demod);
        VR_HIP(hipGetLastError());
        sized_.layer_valid = true;
        sized_.layer_guided = true;
        sized_.layer_gathered = whole_frame_gathered;
    }
}

void RendererHIP::drop_history() { sized_.hist = Sized::History{}; }

// The switches that decide what the history holds: 0 or 1, and a change drops the history.
void RendererHIP::set_history_switch(int& field, int v, const char* refusal) {
    if (v != 0 && v != 1) throw std::runtime_error(refusal);
    if (v == field) return;
    flush_pending();
    drop_history();
    field = v;
}
void RendererHIP::set_denoise_moments(int v) {
    set_history_switch(denoise_moments, v, "denoise_moments: 0 (the frames' sample variance) or 1 (luminance moments kept in the history)");
}
void RendererHIP::set_denoise_resolve(int v) {
    set_history_switch(denoise_resolve, v, "denoise_resolve: 0 (the filter starts from the framebuffer) or 1 (from the frame resolved against the expected coverage)");
}
void RendererHIP::set_denoise_filter(int v) {
    set_history_switch(denoise_filter, v, "denoise_filter: 0 (the a-trous iterations) or 1 (one pass of local regression on the scattered layer; needs denoise_layers = 1)");
}
void RendererHIP::set_denoise_ridge(float v) {
    if (!regress_ridge_ok(v)) throw std::runtime_error("denoise_ridge must be 0 (zero order) or in [2^-20, 2^20]");
    denoise_ridge = v;
}
void RendererHIP::set_denoise_demodulate(int v) { set_history_switch(denoise_demodulate, v, kDemodulateRange); }
void RendererHIP::set_denoise_layers(int v) {
    set_history_switch(denoise_layers, v, "denoise_layers: 0 (the filter runs on the frame) or 1 (on the scattered layer, the background of the expected coverage put back afterwards)");
}

// The control variate on the expected coverage (vr_resolve.h): prepare (B, P) and resolve, two launches on the whole frame.
void RendererHIP::check_resolve(const std::string& me, bool whole_frame_gathered) {
    if (sample < 1) throw std::runtime_error(me + "the framebuffer holds no samples (sample < 1)");
    if (!tiles_host_.empty() && !whole_frame_gathered) throw std::runtime_error(me + "a tile subset is set (set_tiles); the coefficient pools every pixel's neighbours and is formed on whole frames only");
    if (integrator == 2) throw std::runtime_error(me + "integrator = 2 (direct volume rendering) writes an opacity into alpha, not the share of samples that hit");
    if (!sized_.features || sized_.pass != 2)
        throw std::runtime_error(me + "the feature buffer was not last filled by render_features_expected since the last resize (the expected coverage is what replaces the frame's)");
    if (sized_.rays < 2)
        throw std::runtime_error(me + "the expected-value pass ran with rays = " + std::to_string(sized_.rays) + "; rays >= 2 is needed (one ray gives the coverage of the pixel's centre, not of its area)");
    if ((size_t)resolution.x * (size_t)resolution.y * 2u > (size_t)INT32_MAX) throw std::runtime_error(me + "frame too large (32-bit pixel indices)");
}

void RendererHIP::run_resolve() {
    LaunchInputs in;
    capture(in);                                                 // the scene as a launch reads it: the environment's arrays, strength and transform, the camera
    const size_t bytes = (size_t)resolution.x * resolution.y * 4 * sizeof(float);
    ensure_buffer(sized_.rs_bg, bytes); ensure_buffer(sized_.rs_part, bytes); ensure_buffer(sized_.resolved, bytes);
    launch_resolve(in.P, color->as<float>(), sized_.features->as<float>(), sized_.rays, sized_.rs_bg->as<float>(), sized_.rs_part->as<float>(), sized_.resolved->as<float>(), stream);
    VR_HIP(hipGetLastError());
}

void RendererHIP::resolve() {
    flush_pending();
    check_resolve("resolve: ", false);
    run_resolve();
}

void RendererHIP::download_resolved(float* rgba) { download_whole(sized_.resolved, rgba, "resolved: no resolve since the last resize (call resolve first)"); }

void RendererHIP::download_resolve_background(float* rgba) {
    download_whole(sized_.resolved ? sized_.rs_bg : nullptr, rgba, "resolve_background: no resolve since the last resize (call resolve first)");
}

void RendererHIP::download_denoised_layer(float* rgba) {
    download_whole(sized_.layer_valid ? sized_.layer : nullptr, rgba, "denoised_layer: no denoise with denoise_layers = 1 since the last resize");
}

// The layer upsampled under a full-resolution guide (vr_upsample.h): the expected-value pass at the hi size into the call's own buffer, then one kernel.
void RendererHIP::upsample(int factor, int rays) {
    if (factor < kUpsampleMinFactor || factor > kUpsampleMaxFactor) throw std::runtime_error("upsample: factor must be 2..4");
    if (rays < 1 || rays > kExpectedMaxRays) throw std::runtime_error("upsample: rays must be 1.." + std::to_string(kExpectedMaxRays));
    if (denoise_demodulate != 0 && denoise_demodulate != 1) throw std::runtime_error(std::string("upsample: ") + kDemodulateRange);
    flush_pending();
    if (!sized_.layer_valid) throw std::runtime_error("upsample: no denoise with denoise_layers = 1 since the last resize (its layer is what the call upsamples)");
    if (!sized_.layer_guided)
        throw std::runtime_error("upsample: the last denoise ran with denoise_layers = 0 and its guide has replaced the layer's (denoise with denoise_layers = 1 again; denoised_layer stays readable)");
    if (!tiles_host_.empty() && !sized_.layer_gathered) throw std::runtime_error("upsample: a tile subset is set (set_tiles); the call rebuilds whole frames only");
    const int32_t w = resolution.x, h = resolution.y, W = factor * w, H = factor * h;
    const size_t px = (size_t)W * (size_t)H;
    if (px * 2u > (size_t)INT32_MAX) throw std::runtime_error("upsample: the upsampled frame is too large (32-bit pixel indices)");
    SceneParams P;
    feature_scene(P);
    P.u.resolution[0] = W; P.u.resolution[1] = H;         // all else as it is: the kernels take the frame's size from here alone
    if (sized_.up_factor != factor) { sized_.up_factor = 0; sized_.up_features.reset(); sized_.up_out.reset(); sized_.up_layer.reset(); }
    ensure_buffer(sized_.up_features, px * 8 * sizeof(float));
    ensure_buffer(sized_.up_out, px * 4 * sizeof(float));
    ensure_buffer(sized_.up_layer, px * 4 * sizeof(float));
    launch_expected(P, nullptr, tile_count(W, H), rays, sized_.up_features->as<float>());
    const DenoiseSigma sg = sigma();
    launch_upsample(P, sized_.layer->as<float>(), sized_.dn_guide->as<float>(), w, h, factor, sized_.up_features->as<float>(), rays, sg, sized_.up_out->as<float>(),
                    sized_.up_layer->as<float>(), stream, denoise_demodulate != 0);      // vr_demod.h: the lo layer demodulated inside the kernel, whatever produced it
    VR_HIP(hipGetLastError());
    sized_.up_factor = factor;
}

static const char* const kNoUpsample = "upsampled: no upsample since the last resize (call upsample first)";
void RendererHIP::download_upsampled(float* rgba) { download_whole(sized_.up_factor ? sized_.up_out : nullptr, rgba, kNoUpsample); }
void RendererHIP::download_upsampled_layer(float* rgba) { download_whole(sized_.up_factor ? sized_.up_layer : nullptr, rgba, kNoUpsample); }
void RendererHIP::download_upsampled_features(float* out) { download_whole(sized_.up_factor ? sized_.up_features : nullptr, out, kNoUpsample); }
void RendererHIP::upsampled_size(int wh[2]) const {
    if (!sized_.up_factor) throw std::runtime_error(kNoUpsample);
    wh[0] = sized_.up_factor * resolution.x; wh[1] = sized_.up_factor * resolution.y;
}

void RendererHIP::download_history_moments(float* out) {
    const Sized::History& hist = sized_.hist;
    download_whole(hist.cur < 0 ? nullptr : hist.moments[hist.cur], out,
                   "denoise_history_moments: no history with moment records (no denoise_temporal with denoise_moments = 1 since the last resize, history reset or change of the setting)");
}

void RendererHIP::download_history(float* rgba, float* var, float* length) {
    const Sized::History& hist = sized_.hist;
    if (hist.cur < 0) throw std::runtime_error("denoise_history: no history (no denoise_temporal since the last resize or history reset)");
    flush_pending();
    if (rgba) hist.color[hist.cur]->download(rgba, hist.color[hist.cur]->size_bytes(), stream);
    if (!var && !length) return;
    const size_t px = (size_t)resolution.x * resolution.y;
    std::vector<float> rec(px * 4);
    hist.record[hist.cur]->download(rec.data(), rec.size() * sizeof(float), stream);
    for (size_t i = 0; i < px; ++i) {
        if (var) var[i] = rec[4 * i];
        if (length) length[i] = rec[4 * i + 1];
    }
}

void RendererHIP::download_reject_stat(float* out) {
    if (!sized_.reject_stat) throw std::runtime_error("denoise_reject_stat: the last denoise_temporal since the resize did not run with denoise_reject > 0");
    flush_pending();
    const size_t px = (size_t)resolution.x * resolution.y;
    std::vector<float> rec(px * 4);      // the scratch's second half, (T, N_h, z2, has) per pixel
    VR_HIP(hipMemcpyAsync(rec.data(), sized_.dn_reject->as<float>() + px * 4, rec.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < px; ++i) out[i] = rec[4 * i];
}

void RendererHIP::download_denoised(float* rgba) { download_whole(sized_.denoised, rgba, "denoised: no denoise since the last resize (call denoise first)"); }

// ---- adaptive sampling (vr_adaptive.h) -----------------------------------------------------------------------------------------------------------
bool RendererHIP::ragged() {
    if (!tile_n_.empty() && sample != tile_n_sample_) drop_tile_samples();
    return !tile_n_.empty();
}

void RendererHIP::drop_tile_samples() { tile_n_.clear(); tile_n_sample_ = -1; }

std::vector<int32_t> RendererHIP::tile_samples() {
    flush_pending();
    if (ragged()) return tile_n_;
    return std::vector<int32_t>((size_t)tile_count(resolution.x, resolution.y), sample);
}

std::vector<float> RendererHIP::tile_error() {
    flush_pending();
    if (!color) throw std::runtime_error("tile_error: no framebuffer");
    check_moments("tile_error");
    const std::vector<int32_t> counts = tile_samples();
    const int n_all = (int)counts.size();
    std::vector<int32_t> lists((size_t)n_all * 2);
    for (int t = 0; t < n_all; ++t) { lists[(size_t)t] = t; lists[(size_t)(n_all + t)] = counts[(size_t)t]; }
    ensure_buffer_at_least(sized_.adaptive_lists, lists.size() * sizeof(int32_t));
    ensure_buffer_at_least(sized_.adaptive_err, (size_t)n_all * sizeof(float));
    sized_.adaptive_lists->upload(lists.data(), lists.size() * sizeof(int32_t), stream);
    launch_adaptive_error(color->as<float>(), sized_.moments->as<float>(), sized_.adaptive_lists->as<int32_t>(), sized_.adaptive_lists->as<int32_t>() + n_all, n_all, resolution.x,
                          resolution.y, sized_.adaptive_err->as<float>(), stream);
    VR_HIP(hipGetLastError());
    std::vector<float> e((size_t)n_all);
    sized_.adaptive_err->download(e.data(), e.size() * sizeof(float), stream);
    return e;
}

// The schedule of vr_adaptive.h.  Per round: the live tiles and their counts go up in one copy, the error kernel runs, its values come back
// (the round's one wait), then one submit per group of equal counts, each group's tiles costliest first (unless order_tiles is 0) and all
// groups' lists in one more copy.  The tile counts are the bookkeeping of what has been enqueued; `sample` follows at the end (or on a throw).
void RendererHIP::render_adaptive(int min_spp, int max_spp, float threshold) {
    if (min_spp < 2 || min_spp > max_spp || !(threshold >= 0.0f) || !std::isfinite(threshold))
        throw std::invalid_argument("render_adaptive: needs 2 <= min_spp <= max_spp and a finite threshold >= 0");
    flush_pending();
    if (!color) throw std::runtime_error("render_adaptive: no framebuffer (call resize first)");
    const bool was_ragged = ragged();
    if (sample > 0 && !was_ragged && !(sized_.moments && sized_.moments_n == sample))
        throw std::runtime_error("render_adaptive: the moments do not cover samples 1.." + std::to_string(sample) +
                                 " (variance was off for some of them): reset() and render with variance = 1");
    LaunchInputs in;
    capture(in);
    in.variance = 1;                                  // the error estimate needs the moments of every launch
    const int W = resolution.x, H = resolution.y, n_all = tile_count(W, H);
    if (!was_ragged) tile_n_.assign((size_t)n_all, std::max(sample, 0));
    std::vector<int32_t> set(tiles_host_);
    if (set.empty()) { set.resize((size_t)n_all); for (int t = 0; t < n_all; ++t) set[(size_t)t] = t; }
    ensure_buffer_at_least(sized_.adaptive_lists, (size_t)n_all * 2 * sizeof(int32_t));
    ensure_buffer_at_least(sized_.adaptive_err, (size_t)n_all * sizeof(float));
    const bool ordered = in.order_tiles >= 1, split = in.splits_sky();
    open_timing_window(in.stream);                    // one window over all the call's submits
    adaptive_rounds = 0;
    // every group of `ids` from its count n to to(n), as one submit each
    auto launch_groups = [&](const std::vector<int32_t>& ids, const auto& to) {
        const auto groups = adaptive_groups(ids, tile_n_);
        std::vector<int32_t> packed;
        std::vector<int> n_sky, n_see;                // per group: its clear and its see-through tiles, which lie in that order behind its march tiles in `packed`
        for (const auto& g : groups) {
            std::vector<int32_t> march = g.second, sky, see;
            if (split) split_three(in, g.second, (int)g.second.size(), march, sky, see);
            if (ordered && !march.empty()) march = costliest_first(in.P, march, (int)march.size());
            packed.insert(packed.end(), march.begin(), march.end());
            packed.insert(packed.end(), sky.begin(), sky.end());
            packed.insert(packed.end(), see.begin(), see.end());
            n_sky.push_back((int)sky.size());
            n_see.push_back((int)see.size());
        }
        if (packed.empty()) return;
        sized_.adaptive_lists->upload(packed.data(), packed.size() * sizeof(int32_t), in.stream);
        size_t off = 0, k = 0;
        for (const auto& g : groups) {
            const int32_t n = g.first, next = to(n);
            const int n_clear = n_sky[k], n_through = n_see[k], n_tiles = (int)g.second.size() - n_clear - n_through;      // the march tiles
            ++k;
            const int32_t* list = sized_.adaptive_lists->as<int32_t>() + off;
            submit(in, n, next - n, list, n_tiles, prepare_submit(in, n, next - n, n_tiles, n_clear + n_through), n_clear + n_through > 0 ? list + n_tiles : nullptr, n_clear, n_through);
            for (int32_t t : g.second) tile_n_[(size_t)t] = next;
            off += g.second.size();
        }
    };
    auto finish = [&] {
        close_timing_window(in.stream);               // (on a throw too)
        const auto mm = std::minmax_element(tile_n_.begin(), tile_n_.end());
        sample = *mm.second;
        if (*mm.first == *mm.second) { drop_tile_samples(); sized_.moments_n = sample; }      // every tile at one count: an ordinary uniform frame
        else { tile_n_sample_ = sample; sized_.moments_n = -1; }
    };
    try {
        std::vector<int32_t> low;                     // step 1: the set to min_spp
        for (int32_t t : set) if (tile_n_[(size_t)t] < min_spp) low.push_back(t);
        launch_groups(low, [&](int32_t) { return min_spp; });
        std::vector<int32_t> live, go;
        for (int32_t t : set) if (tile_n_[(size_t)t] < max_spp) live.push_back(t);
        while (!live.empty()) {                       // step 2: rounds
            ++adaptive_rounds;
            const size_t m = live.size();
            std::vector<int32_t> lists(live);
            for (int32_t t : live) lists.push_back(tile_n_[(size_t)t]);
            sized_.adaptive_lists->upload(lists.data(), lists.size() * sizeof(int32_t), in.stream);
            launch_adaptive_error(color->as<float>(), sized_.moments->as<float>(), sized_.adaptive_lists->as<int32_t>(), sized_.adaptive_lists->as<int32_t>() + m, (int32_t)m, W, H,
                                  sized_.adaptive_err->as<float>(), in.stream);
            VR_HIP(hipGetLastError());
            std::vector<float> e(m);
            sized_.adaptive_err->download(e.data(), m * sizeof(float), in.stream);
            check_watchdog();
            go.clear();
            for (size_t k = 0; k < m; ++k) if (!adaptive_converged(e[k], threshold)) go.push_back(live[k]);
            launch_groups(go, [&](int32_t n) { return adaptive_next_count(n, max_spp); });
            live.clear();
            for (int32_t t : go) if (tile_n_[(size_t)t] < max_spp) live.push_back(t);
        }
    } catch (...) {
        finish();
        throw;
    }
    finish();
}

void RendererHIP::check_watchdog() {
    const uint32_t st = watchdog_status();
    if (st & kSkyHitStatus) throw std::runtime_error("sky tiles: a camera ray of a tile classified clear hit the volume's box (vr_sky_tiles.h sky_tile_clear is wrong for this view); the pixels concerned stopped at that sample. Render with sky_tiles 0");
    if (st & kFeatureLostStatus) throw std::runtime_error("feature pass: a camera segment exceeded its step budget (vr_render_features); the pixels concerned cover only their samples before it");
    if (st != 0) throw std::runtime_error("path-tracing kernel watchdog tripped (a wavefront exceeded its step budget)");
}

uint32_t RendererHIP::watchdog_status() {
    // bit 0: a wavefront gave up (iteration / shader-clock budget), bit 1: a path ended in an impossible state, bit 2 (kFeatureLostStatus): a feature
    // sample's tracker exceeded its step budget, bit 3 (kSkyHitStatus): a camera ray of a tile classified clear hit the box.
    // Read-and-clear, so that one bad launch does not poison the renderer.
    flush_pending();
    uint32_t s = 0;
    status_->download(&s, sizeof s, stream);
    if (s != 0) {
        VR_HIP(hipMemsetAsync(status_->get(), 0, sizeof(uint32_t), stream));
        VR_HIP(hipStreamSynchronize(stream));
    }
    return s;
}

}  // namespace vr
