"""The multi-rank flow of bench.py with real HIP renderers, executed on the ONE GPU a test box has.

Every run is a fresh child `python bench.py --gpus N ...`: for N > 1 the launcher spawns its ranks (torch.distributed.run on
127.0.0.1) before anything in it touches the GPU, the ranks share device 0 (VOLREN_DIST_BACKEND=gloo: the collective is staged
through the host, everything else -- set_tiles, the fused render of the rank's tiles, pack_tiles, all_gather, unpack_tiles, and the
same frames pipelined over two streams -- is the path an 8-GPU node runs), and rank 0 prints the JSON line with `frame_crc32` of its RGBA32F frame after
the last step.  A pixel-sample depends on (seed, pixel, sample) only (shader/pathtracer_brick.glsl:28-36), so the CRC must be the
same for every N -- and equal to the CRC of the oracle's frame.  RCCL itself carries one rank's tiles in the `--force-dist` run
(nccl backend, world size 1): init_process_group, all_gather_into_tensor and the stream ordering around it run on the box.

A GPU box admits at most 6 processes of one user on its card (the pytest process and the launcher's elastic agent count: pytest + agent + 4 ranks would sit
exactly at the limit): the largest world here is 3; tests/tools_multirank_log.sh records 4 and 5 ranks (profiles/r4_multirank_*).
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 256, 192, 8


def run_bench(n, backend=None, extra=(), config="c2", w=W, h=H, spp=SPP, steps=2, timeout=900, full=True):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    if backend:
        env["VOLREN_DIST_BACKEND"] = backend
    else:
        env.pop("VOLREN_DIST_BACKEND", None)
    env["VOLREN_SAMPLE_POOL_MB"] = "1024"               # several ranks x two pipelined renderers share one GPU
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--config", config, "--width", str(w), "--height", str(h), "--spp", str(spp),
           "--steps", str(steps), "--warmup", "1", "--cpu-budget", "0", "--extra-configs", "none"] + (["--full"] if full else []) + list(extra)
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, "bench.py --gpus %d failed (rc %d)\n%s\n%s" % (n, out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:]
    return json.loads(lines[-1])


@pytest.fixture(scope="module")
def oracle_crc():
    ref = scenes.oracle_scene("c2", W, H).render(SPP)
    return zlib.crc32(np.ascontiguousarray(ref, np.float32).tobytes()) & 0xFFFFFFFF


@pytest.mark.timeout(1800)
def test_bench_multirank_frames_equal_the_single_gpu_frame(oracle_crc):
    j1 = run_bench(1)
    assert j1["n_gpus"] == 1 and j1["rccl_ranks"] == 1 and j1["dist_backend"] is None
    assert j1["frame_crc32"] == oracle_crc, "N=1 frame differs from the oracle's"
    assert j1["value"] > 0 and j1["value_pipelined"] is None            # one GPU: frames one after the other, nothing else measured
    # the reference's protocol, spp x vr_trace + one vr_synchronize per frame: ONE fused launch, the same frame
    tl = j1["trace_loop"]
    assert j1["value_trace_loop"] == tl["value"] > 0 and tl["same_frame"] and tl["launches_per_step"] == 1 and tl["calls_per_step"] == SPP
    assert j1["roofline"]["frac_fused_fb"] < j1["roofline"]["frac"]
    for n in (2, 3):
        j = run_bench(n, backend="gloo")
        # the product's own host (vr_sharded_*, one process) runs as a child once the ranks are done: here as logical shards of device 0
        leg = j["sharded"]
        assert "error" not in leg, leg
        assert leg["host"] == "sharded" and leg["n_gpus"] == n and leg["devices"] == [0] * n and leg["transport"] == "copy"
        assert leg["frame_crc32"] == oracle_crc and j["sharded_same_frame"] and j["value_sharded"] == leg["value"] > 0
        assert j["n_gpus"] == n and j["rccl_ranks"] == n and j["dist_backend"] == "gloo"
        assert j["value_pipelined"] > 0 and j["scaling"] == "strong"    # N > 1: also the frames pipelined over two renderers / streams
        assert j["frame_crc32"] == oracle_crc, "N=%d frame differs from the N=1 frame" % n
        assert j["roofline"]["samples_per_launch"] < W * H * SPP          # a rank rendered its share, not the frame


@pytest.mark.timeout(900)
def test_bench_plain_run_dumps_the_frame_of_the_last_step(oracle_crc, tmp_path):
    """Without --full the line carries the headline only; --dump-outputs writes the frame the last timed step left -- the oracle's frame."""
    j = run_bench(1, full=False, extra=["--dump-outputs", str(tmp_path)])
    assert j["steps"] == 2 and j["value"] > 0 and j["ms_per_step"] > 0 and j["frame_crc32"] == oracle_crc
    assert not {"value_pipelined", "trace_loop", "value_trace_loop", "roofline", "cpu_baseline", "fast_math", "configs", "sharded"} & set(j), sorted(j)
    fb = np.load(tmp_path / "framebuffer.npy")
    assert fb.dtype == np.float32 and fb.shape == (H, W, 4)
    assert zlib.crc32(fb.tobytes()) & 0xFFFFFFFF == oracle_crc


@pytest.mark.timeout(900)
def test_bench_one_rank_process_group_over_rccl(oracle_crc):
    """`--force-dist`: world size 1 on the nccl backend -- librccl loads, the communicator comes up on the device, and the frame that went
    through pack_tiles -> all_gather_into_tensor (RCCL) -> unpack_tiles on the renderer's stream is the frame."""
    j = run_bench(1, extra=["--force-dist"])
    assert j["n_gpus"] == 1 and j["rccl_ranks"] == 1 and j["dist_backend"] == "nccl"
    assert j["frame_crc32"] == oracle_crc


@pytest.mark.timeout(900)
def test_bench_pipelining_switch(oracle_crc, monkeypatch):
    """VOLREN_PIPELINE=0: N > 1 without the second renderer; =1: N = 1 with it.  The frame is the frame either way."""
    monkeypatch.setenv("VOLREN_PIPELINE", "0")
    j = run_bench(2, backend="gloo")
    assert j["value_pipelined"] is None and j["frame_crc32"] == oracle_crc
    monkeypatch.setenv("VOLREN_PIPELINE", "1")
    j = run_bench(1)
    assert j["value_pipelined"] > 0 and j["frame_crc32"] == oracle_crc


@pytest.mark.timeout(900)
def test_bench_host_sharded(oracle_crc):
    """`bench.py --gpus N --host sharded`: the product's multi-GPU host under the bench (verdict r4 #4) -- one process, vr_sharded_*; on a one-GPU box
    the parts are logical shards (`--devices 0,0,0`, copy transport) and RCCL carries a one-part group (VR_SHARDED_TRANSPORT=rccl)."""
    j = run_bench(3, extra=["--host", "sharded", "--devices", "0,0,0"])
    assert j["host"] == "sharded" and j["n_gpus"] == 3 and j["transport"] == "copy" and j["rccl_ranks"] == 0 and j["distinct_devices"] == 1
    assert j["frame_crc32"] == oracle_crc and j["value"] > 0 and len(j["parts"]) == 3
    assert all(p["launches"] >= 1 and p["pathtrace_ms"] > 0 for p in j["parts"])
    os.environ["VR_SHARDED_TRANSPORT"] = "rccl"
    try:
        j = run_bench(1, extra=["--host", "sharded"])
    finally:
        del os.environ["VR_SHARDED_TRANSPORT"]
    assert j["transport"] == "rccl" and j["rccl_ranks"] == 1 and j["frame_crc32"] == oracle_crc
