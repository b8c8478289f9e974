// sharded.h -- ShardedRenderer: one process, N RendererHIP parts on N devices, one frame.
//
// No reference counterpart (the reference drives one GL context, src/main.cpp:524-557); this is SURVEY 8(e) inside the product
// rather than inside a benchmark harness: the scene is replicated on every device, the frame's 16x16 tiles (the reference's work
// group, shader/pathtracer_brick.glsl:3) are dealt diagonally, owner(tx, ty) = (tx + ty) mod N, every part renders all samples of
// its tiles with no communication on its own stream, and ONE gather per frame (RCCL over xGMI: grouped ncclSend / ncclRecv to part 0; round 4-5: a grouped
// ncclAllGather, still there behind VR_SHARDED_COLLECTIVE=allgather) of the compact
// per-part tile buffers puts the accumulated radiance together; part 0 scatters it back into its framebuffer, which then holds the
// whole frame -- bit-identical to a single-device render, because a pixel-sample depends on (seed, pixel, sample) only
// (pathtracer_brick.glsl:28-36).  The denoiser's guide buffers (per-pixel moments, features) travel the same way on request, and part 0 filters the frame.
//
// Transport: "rccl" when the parts sit on distinct devices (librccl.so.1 is opened at run time: the library has no link-time
// dependency on it), "copy" when two parts share a device (logical shards of one GPU: device-to-device copies ordered by events
// stand in for the collective -- RCCL refuses a communicator with duplicate devices) or when VR_SHARDED_TRANSPORT=copy asks for it
// (peer copies across devices).  VR_SHARDED_TRANSPORT=rccl forces the collective also for a single part.
#pragma once

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "renderer.h"

namespace vr {

// raster tile ids (row 0 = bottom) owned by each of n parts: owner(tx, ty) = (tx + ty) mod n
std::vector<std::vector<int32_t>> tile_owner_lists(int width, int height, int n_parts);

struct ShardedRenderer {
    // parts[i] renders on devices[i] (repeats allowed); the renderers belong to the caller and must outlive this object.
    // Every part must have been init()-ed at the same resolution; scene state is the caller's to replicate (for_each).
    ShardedRenderer(const std::vector<RendererHIP*>& parts, const std::vector<int>& devices);
    ~ShardedRenderer();
    ShardedRenderer(const ShardedRenderer&) = delete;
    ShardedRenderer& operator=(const ShardedRenderer&) = delete;

    size_t n_parts() const { return parts_.size(); }
    RendererHIP& part(size_t i) { return *parts_[i]; }
    int device(size_t i) const { return devices_[i]; }
    // fn(part, index) with that part's device current: replicate scene calls
    template <class F> void for_each(F fn) {
        for (size_t i = 0; i < parts_.size(); ++i) { VR_HIP(hipSetDevice(devices_[i])); fn(*parts_[i], i); }
    }
    void reset();                         // every part: sample = 0
    // `spp` more samples per pixel (<= 0: up to sppx): every part renders its tiles (asynchronously, its own stream; issued from one host thread
    // per part), then the gather; returns when everything is enqueued -- the first frame on new settings after every part's probe launch has been
    // waited for (launch_target_ms; all parts at once, set the parts' launch_target_ms to 0 to have none).  The whole frame is in part(0).color once
    // synchronize() returns.  More parts than the frame has tile diagonals: the surplus parts own no tile and render nothing.
    void render(int spp = 0);
    void synchronize();                   // waits for all parts; throws if a kernel watchdog tripped
    // Denoising on several devices (renderer.h render_features / denoise / denoise_temporal): bit for bit what one device gives, because the filter is
    // deterministic per pixel and part 0 runs it on the gathered whole frame.  Asynchronous like render(); no host synchronisation is needed anywhere in
    // reset, render, render_features, denoise, reset, render, ... (stream order and the exchange's events keep the frames apart).
    // render_features: every part that owns tiles runs its feature pass over them on its own stream (one host thread per part); no exchange.
    // render_features_expected: the same with every part's render_features_expected(rays), rays in 1..4.
    void render_features(int spp);
    void render_features_expected(int rays);
    // gather_guides: every part's moments and features of its own tiles -> part 0's moments and features, which then cover the whole frame
    // (part(0).download_variance / download_features): one pack per part, ONE exchange of 3x the colour's size through the transport render() uses,
    // one unpack on part 0.  The buffers are allocated by the first call at a resolution: a caller that only renders pays nothing.
    void gather_guides();
    // denoise / denoise_temporal: gather_guides(), then part 0's filter on the whole frame, with part 0's settings (denoise_iterations, denoise_sigma,
    // denoise_alpha) and -- temporal -- part 0's camera and history: the history lives in part 0 and is read and dropped there (part(0).download_history,
    // part(0).drop_history), as is the result (part(0).download_denoised).  Refused before anything is launched, with a message that names the part, unless
    // all parts agree on resolution and sample, sample >= 1, and every part that owns tiles has moments covering samples 1..sample (`variance` on for all of
    // them), a feature pass since the last resize and no ragged frame (render_adaptive: adaptive sampling stays a single-device feature).  A refused call
    // leaves the last result and the history as they were.  One part without a forced transport: the plain renderer's calls.
    // (RendererHIP::denoise() on a part keeps refusing the part's tile subset.)
    void denoise();
    void denoise_temporal();
    const std::string& transport() const { return transport_; }      // "rccl" | "copy" | "none" (one part, nothing to exchange)
    const std::string& collective() const { return collective_; }    // of the rccl transport: "gather" (ncclSend / ncclRecv to part 0) | "allgather"

private:
    void setup(int width, int height);   // tile deal + buffers for the current resolution
    void prepare(const char* who);        // throws unless the parts agree on resolution and sample; setup() on a new resolution
    void issue_on_parts(const std::function<void(size_t)>& issue);
    void feature_pass_on_parts(const char* who, const std::function<void(RendererHIP&)>& pass);      // `pass` on every part that owns tiles, on its device
    void check_guides(const char* who);   // what gather_guides and the filter need of every part, before the first launch
    void exchange_guides();               // gather_guides after the checks
    void run_denoise(const char* who, bool temporal);
    void release();                       // everything this object created; the parts get their previous streams back
    std::vector<RendererHIP*> parts_;
    std::vector<int> devices_;
    std::string transport_, collective_;
    int width_ = 0, height_ = 0, n_max_ = 0;
    struct PartBuffers {
        hipStream_t stream = nullptr;     // owned
        hipEvent_t packed_ready = nullptr;
        int n_own = 0;                    // tiles this part renders
        DeviceBufferPtr pack_ids, packed, gathered;      // gathered: on part 0 (every part under VR_SHARDED_COLLECTIVE=allgather)
        DeviceBufferPtr guides_packed, guides_gathered;  // the same pair for the denoiser's guides, kGuidePlanes x as large; made by the first gather_guides
    };
    std::vector<PartBuffers> buf_;
    // every part's `packed` (count floats) into part 0's `gathered`, on the transport: rccl gather, rccl allgather, or copies ordered by events
    void exchange(DeviceBufferPtr PartBuffers::*packed, DeviceBufferPtr PartBuffers::*gathered, size_t count);
    DeviceBufferPtr unpack_ids_;          // on part 0's device: every part's tile ids in part order, -1 = padding
    std::vector<void*> comms_;            // ncclComm_t per part (rccl transport)
    std::vector<hipStream_t> prev_streams_;      // what the parts' `stream` fields held before this object took them
};

}  // namespace vr
