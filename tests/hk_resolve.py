"""ctypes binding of tests/hostkernel/libresolve_host.so: the control variate on the expected coverage (volren_amd/csrc/vr_resolve.h) built for the
host, plus a float64 numpy statement of the same definition, written from the header's text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_features
from hk_common import _f32, _p

_lib = None
WINDOW = 3


def build():
    return hk_common.build(__file__, "resolve_host.cpp", "libresolve_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def prepare(o, rays, fb):
    """Prepare on an oracle.binding.OracleRenderer's scene and the frame fb [H][W][4]: -> (B, P), [H][W][4] float32 each."""
    args, keep = hk_features._args(o)
    fb = _f32(fb, (o.h, o.w, 4))
    B, P = np.zeros((o.h, o.w, 4), np.float32), np.zeros((o.h, o.w, 4), np.float32)
    lib().hk_resolve_prepare(*args, int(rays), _p(fb), _p(B), _p(P))
    del keep
    return B, P


def part(fb, B):
    """Prepare's second half from a B of the caller's: P [H][W][4]."""
    h, w = fb.shape[:2]
    P = np.zeros((h, w, 4), np.float32)
    lib().hk_resolve_part(w, h, _p(_f32(fb, (h, w, 4))), _p(_f32(B, (h, w, 4))), _p(P))
    return P


def resolve(fb, B, P, kappa):
    """Resolve: fb, B, P [H][W][4], kappa [H][W] -> y [H][W][4] float32."""
    h, w = fb.shape[:2]
    out = np.zeros((h, w, 4), np.float32)
    lib().hk_resolve(w, h, _p(_f32(fb, (h, w, 4))), _p(_f32(B, (h, w, 4))), _p(_f32(P, (h, w, 4))), _p(_f32(kappa, (h, w))), _p(out))
    return out


def resolved(o, rays, fb, guide):
    """Both steps: the frame fb of o's scene against the coverage of guide [H][W][8] (an expected-value pass of `rays` rays): -> (y, B)."""
    B, P = prepare(o, rays, fb)
    return resolve(fb, B, P, guide[..., 3]), B


# ---- the float64 statement -----------------------------------------------------------------------------------------------------------------------
def spec_background(o, rays):
    """B [H][W][3] float64: the mean over the rays x rays sub-rays of the environment radiance along the sub-ray (vr_trace.h lookup_environment: the
    inverse transform, the equirectangular (u, v), a bilinear fetch that repeats in u and clamps in v, times the strength); 0 with the environment hidden."""
    p = o.params()
    W, H, n = o.w, o.h, int(rays)
    if not p.show_environment:
        return np.zeros((H, W, 3))
    cam_z = -0.5 / np.tan(0.5 * np.pi * float(p.cam_fov) / 180.0)
    y, x, j, i = np.meshgrid(np.arange(H), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    x, y, i, j = (a.reshape(-1).astype(np.float64) for a in (x, y, i, j))
    fx = ((x + (i + 0.5) / n) - W * 0.5) / H
    fy = ((y + (j + 0.5) / n) - H * 0.5) / H
    d = np.stack([fx, fy, np.full(len(x), cam_z)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ct = np.array(list(p.cam_transform), np.float64).reshape(3, 3).T                 # column-major
    d = d @ ct.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inv = np.array(list(p.env_inv_transform), np.float64).reshape(3, 3).T
    e = d @ inv.T
    u = np.arctan2(e[:, 2], e[:, 0]) / (2.0 * np.pi) + 0.5
    v = 1.0 - np.arccos(np.clip(e[:, 1], -1.0, 1.0)) / np.pi
    tex = np.asarray(o.env_tex, np.float64)
    th, tw = tex.shape[:2]
    tx, ty = u * tw - 0.5, v * th - 0.5
    ix, iy = np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)
    ax, ay = (tx - ix)[:, None], (ty - iy)[:, None]
    x0, x1 = ix % tw, (ix + 1) % tw
    y0, y1 = np.clip(iy, 0, th - 1), np.clip(iy + 1, 0, th - 1)
    c = (tex[y0, x0] * (1 - ax) + tex[y0, x1] * ax) * (1 - ay) + (tex[y1, x0] * (1 - ax) + tex[y1, x1] * ax) * ay
    return (float(p.env_strength) * c).reshape(H, W, n * n, 3).mean(axis=2)


def _window_sum(a):
    """sum over the 7 x 7 window, taps outside the frame skipped"""
    h, w = a.shape[:2]
    s = np.zeros_like(a)
    for dy in range(-WINDOW, WINDOW + 1):
        for dx in range(-WINDOW, WINDOW + 1):
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 < y1 and x0 < x1:
                s[y0:y1, x0:x1] += a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return s


def spec_resolve(fb, B, kappa):
    """vr_resolve.h's header comment in float64: fb [H][W][4], B [H][W][3], kappa [H][W] -> y [H][W][4]."""
    x = np.asarray(fb, np.float64)
    B = np.asarray(B, np.float64)[..., :3]
    kappa = np.asarray(kappa, np.float64)
    kh = x[..., 3]
    P = np.concatenate([x[..., :3] - (1.0 - kh)[..., None] * B, kh[..., None]], axis=2)
    S = _window_sum(P)
    D = S[..., 3]
    Ct = np.where((D > 0)[..., None], S[..., :3] / np.where(D > 0, D, 1.0)[..., None], 0.0)
    beta = B - Ct
    y = np.zeros_like(x)
    y[..., :3] = np.maximum(0.0, x[..., :3] + beta * (kh - kappa)[..., None])
    y[..., 3] = kappa
    return y
