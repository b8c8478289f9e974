"""What the GPU tests of the temporal accumulation share (test_gpu_temporal.py, test_gpu_reject.py, test_gpu_sharded_denoise.py): a scene with moments,
one frame of a sequence, the renderer's camera, an orbit, and the comparison of a denoise_temporal() call with its replay on the host."""
import numpy as np

import hk_temporal as ht
import scenes
from hk_common import bits as _bits


def _scene(name, w, h):
    r = scenes.hip_scene(name, w, h)
    r.variance = 1
    return r


def _frame(r, spp, seed=None, fspp=None, fseed=None):
    """one frame of a sequence, up to the denoise call: reset, render, render_features"""
    if seed is not None:
        r.seed = seed
    r.reset()
    r.render(spp)
    if fseed is not None:
        r.seed = fseed
    r.render_features(fspp or spp)


def _camera(r):
    """the renderer's own camera from its uniform block (vr_get_uniforms): 3 ints, then cam_pos, cam_fov, cam_transform"""
    f = np.frombuffer(r.uniforms_bytes(), np.float32)
    return ht.camera(f[3:6], f[7:16], fov_degree=float(f[6]))


def _orbit(r, degrees, yaw=0.0):
    """cam_pos = (1, 0, 1) turned about +y, cam_dir towards the origin (yaw: turned away from it about +y, degrees)"""
    a = np.radians(45.0 + degrees)
    pos = np.array([np.sqrt(2.0) * np.sin(a), 0.0, np.sqrt(2.0) * np.cos(a)])
    b = np.radians(yaw)
    d = -pos / np.linalg.norm(pos)
    r.cam_pos = pos
    r.cam_dir = (np.cos(b) * d[0] + np.sin(b) * d[2], 0.0, -np.sin(b) * d[0] + np.cos(b) * d[2])


def _check_against_replay(r, replay, what, n=None):
    """after r.denoise_temporal(): history, result and statistic equal the host lane code fed with the renderer's own buffers, camera and threshold.
    -> (N, T; T is None at a threshold of 0)"""
    tau = r.denoise_reject
    hc, hv, hn = r.denoise_history()
    want = replay.frame(_camera(r), r.framebuffer(), r.variance(), r.features(), r.sample if n is None else n, r.denoise_alpha, r.denoise_iterations,
                        tuple(r.denoise_sigma), tau=tau)
    parts = [(hc, want[0], "C"), (hv, want[1], "V"), (hn, want[2], "N"), (r.denoised(), want[3], "denoised")]
    if tau > 0:
        parts.append((r.denoise_reject_stat(), replay.stat, "T"))
    for got, ref, part in parts:
        bad = _bits(got) != _bits(ref)
        assert not bad.any(), (what, part, int(bad.sum()))
    return hn, replay.stat
