"""The catalogue of crafted frames for the image-space kernels (volren_amd/csrc/vr_filters.hip), one list per stage of vr_filter_probe, and the two ways to run a
case: host(case), the host build of the stage's header (tests/hk_*.py, range-checked where the binding offers it), and device(renderer, case), the kernel through
Renderer.filter_probe.  tests/test_filter_cases_host.py runs every case through host() and holds it to the float64 statement and to its non-triviality
conditions; tests/test_gpu_filter_probe.py compares device() with host() bit for bit.  A case goes near a device only after it passed the CPU file.
TEST HARNESS ONLY.

Every case is deterministic and inside what the product's own passes can hand these kernels: coverage in [0, 1], depth finite and >= 0, albedo finite, normals
finite (not necessarily unit, possibly zero), colour and moments >= 0.  The exceptions carry nonfinite = True and are of four kinds only: inf moments from
overflow in prepare (and the inf v behind it), a NaN or inf colour texel in atrous, regress and temporal, a NaN moment in the adaptive error, and -- in the
group "demod", in the DEMOD instances of split, prepare and merge alone -- a NaN or +inf albedo word of the features (and a quotient or product of finite words
that overflows).  Those three stages are per-pixel and index nothing by the albedo.  No such word goes into upsample, a guide input, a camera or a history record,
and no other case puts a non-finite value into a feature: those feed the edge weights and the index arithmetic.

The group "demod" (par["demod"] = 1: vr_filter_probe's params[35], hk_demod on the host) draws its albedo words per channel from ALBEDOS -- zeros of both signs,
a subnormal, the floor 2^-6 and its two neighbours, values above 1, a negative one -- and its coverage from KAPPAS, and keeps the albedo where the coverage is 0.

Frames: 47x33 (test_denoise_host.hostile's size: 3 x 3 tiles, ragged on both axes); 33x31, 17x16, 1x37 and 37x1 where the stage reads neighbours or stages a
window; nothing holds more pixels than 64x48."""
import numpy as np

import hk_adaptive as ha
import hk_demod as hd
import hk_denoise
import hk_layers as hl
import hk_moments as hm
import hk_regress as hg
import hk_resolve as hr
import hk_temporal as ht
import hk_upsample as hu
from test_denoise_host import SIGMA2, hostile
from test_temporal_host import orbit_camera

SIGMA = hk_denoise.DEFAULT_SIGMA
W0, H0 = 47, 33
SMALL = ((33, 31), (17, 16), (1, 37), (37, 1))
MAX_PIXELS = 64 * 48
STAGES = ("prepare", "atrous", "temporal", "resolve", "split", "merge", "regress", "upsample", "adaptive_error")


class Case:
    """stage, name, frame size, the input arrays (inp) and the parameters (par).  scene: the scene-bound stages' scene name (test_resolve_host._oracle's names).
    nonfinite: the case holds one of the four sanctioned non-finite inputs.  ill: why the float64 statement does not apply, or None."""

    def __init__(self, stage, name, w, h, inp, par=None, scene=None, nonfinite=False, ill=None):
        assert stage in STAGES and w * h <= MAX_PIXELS
        self.stage, self.name, self.w, self.h, self.inp, self.par = stage, name, w, h, inp, dict(par or {})
        self.scene, self.nonfinite, self.ill = scene, nonfinite, ill

    @property
    def id(self):
        return "%s-%s" % (self.stage, self.name)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def variance_scale(n):
    """vr_tiles.h variance_scale in float32"""
    return np.float32(n) / np.float32(n - 1) if n >= 2 else np.float32(0.0)


def frame(w=W0, h=H0, seed=11):
    """hostile() at a size: (colour, moments or variance, features)"""
    return hostile(h=h, w=w, seed=seed)


_BASE = {}


def base(w=W0, h=H0, seed=11, n=8):
    """the hostile frame with prepare's v and guide behind it (host build): colour, v, guide, features"""
    key = (w, h, seed, n)
    if key not in _BASE:
        c, var, f = frame(w, h, seed)
        v, g = hk_denoise.prepare(var, f, n)
        _BASE[key] = (c, v, g, f)
    return _BASE[key]


# ---- prepare ----------------------------------------------------------------------------------------------------------------------------------------------
def prepare_cases():
    _, S, feat = frame()
    out = [Case("prepare", "hostile-n%d" % n, W0, H0, {"S": S, "feat": feat}, {"n": n}) for n in (1, 2, 2 ** 20)]
    counts = np.array([[1, 2, 3], [8, 1, 1000], [2 ** 20, 5, 2]], np.int32)      # 1 among them, neighbours differ
    out.append(Case("prepare", "counts", W0, H0, {"S": S, "feat": feat, "counts": counts}, {"n": 7}))
    rng = np.random.default_rng(21)
    tiny = rng.choice(np.array([0.0, 1e-38, 1e-39, 1e-44, 1e-30], np.float32), (H0, W0, 4)).astype(np.float32)
    for n in (2, 2 ** 20):
        out.append(Case("prepare", "tiny-n%d" % n, W0, H0, {"S": tiny, "feat": feat}, {"n": n}))
    big = rng.choice(np.array([0.0, 1e-38, 1.0, 3e38], np.float32), (H0, W0, 4)).astype(np.float32)
    out.append(Case("prepare", "overflow", W0, H0, {"S": big, "feat": feat}, {"n": 2}, nonfinite=True))
    out.append(Case("prepare", "overflow-counts", W0, H0, {"S": big, "feat": feat, "counts": counts}, {"n": 2}, nonfinite=True))
    return out


def _prepare_host(c):
    S, feat, counts, n = c.inp["S"], c.inp["feat"], c.inp.get("counts"), c.par["n"]
    with np.errstate(over="ignore", invalid="ignore"):
        if counts is None:
            var = S * variance_scale(n) if n >= 2 else np.zeros_like(S)
            v, g = hk_denoise.prepare(f32(var), feat, n)
            n_px = n
        else:
            n_px = ha.per_pixel(counts, c.w, c.h)
            scale = np.array([variance_scale(int(k)) for k in counts.reshape(-1)], np.float32).reshape(counts.shape)
            scale_px = np.repeat(np.repeat(scale, 16, axis=0), 16, axis=1)[:c.h, :c.w]
            var = np.where((n_px >= 2)[..., None], S * scale_px[..., None], np.float32(0.0))
            v, g = ha.prepare(f32(var), feat, n_px)
        if c.par.get("demod"):                           # the variance of the divided layer; the guide stays prepare's
            v = hd.variance(f32(var), feat, n_px)
    return {"v": v, "guide": g}


def _prepare_device(r, c):
    n = c.par["n"]
    counts = c.inp.get("counts")
    v, g = r.filter_probe("prepare", c.w, c.h, [c.inp["S"], c.inp["feat"], None if counts is None else np.ascontiguousarray(counts.reshape(-1), np.int32)],
                          [(c.h, c.w), (c.h, c.w, 8)], i0=n, x=variance_scale(n), demod=bool(c.par.get("demod")))
    return {"v": v, "guide": g}


# ---- atrous -----------------------------------------------------------------------------------------------------------------------------------------------
def atrous_cases():
    col, v, g, _ = base()
    out = []

    def add(name, color=col, var=v, guide=g, w=W0, h=H0, step=1, sigma=SIGMA, vout=True, **kw):
        out.append(Case("atrous", name, w, h, {"color": color, "v": var, "guide": guide}, {"step": step, "sigma": tuple(float(s) for s in sigma), "vout": vout}, **kw))

    for step in (1, 2, 4, 16):                           # 16: past every edge of the frame from every pixel but the middle ones
        add("step%d" % step, step=step)
    add("step2-no-vout", step=2, vout=False)
    add("step16-no-vout", step=16, vout=False)
    for step in (1, 4):
        add("sigma2-step%d" % step, step=step, sigma=SIGMA2)
    lo, hi = hk_denoise.sigma_range()
    for which, tag in enumerate("cndka"):
        for end, val in (("lo", lo), ("hi", hi)):
            sg = list(SIGMA)
            sg[which] = val
            add("sigma-%s-%s" % (tag, end), step=2, sigma=sg,
                ill="sigma_n = 2^60: any rounding of dot(g_p, g_q) below 1 turns w_n from 1 into 0, and float32 and float64 round differently "
                    "(test_denoise_host.test_sigma_limits_give_finite_output)" if (which, end) == (1, "hi") else None)
    zero = np.zeros_like(v)
    half = v.copy()
    half[:, : W0 // 2] = 0.0
    for step in (1, 4):
        add("v0-step%d" % step, var=zero, step=step)
        add("v0-half-step%d" % step, var=half, step=step)
    for w, h in SMALL:
        c2, v2, g2, _ = base(w, h, seed=13)
        for step in (1, 16):
            add("%dx%d-step%d" % (w, h, step), c2, v2, g2, w, h, step)
    bad = col.copy()
    bad[10, 20, 1] = np.nan
    bad[25, 40, 0] = np.inf
    for step in (1, 4):
        add("nan-inf-texel-step%d" % step, color=bad, step=step, nonfinite=True)
    vinf = v.copy()
    vinf[5:8, 30:33] = np.inf                            # prepare's v behind overflowed moments
    add("inf-v-step2", var=vinf, step=2, nonfinite=True)
    return out


def _atrous_host(c):
    with np.errstate(all="ignore"):
        col, v = hk_denoise.atrous(c.inp["color"], c.inp["v"], c.inp["guide"], c.par["step"], c.par["sigma"])
    return {"color": col, "v": v} if c.par["vout"] else {"color": col}


def _atrous_device(r, c):
    px = (c.h, c.w)
    col, v = r.filter_probe("atrous", c.w, c.h, [c.inp["color"], c.inp["v"], c.inp["guide"]], [px + (4,), px if c.par["vout"] else None], sigma=c.par["sigma"], i0=c.par["step"])
    return {"color": col, "v": v} if c.par["vout"] else {"color": col}


# ---- temporal (plain, rejection, moments) -----------------------------------------------------------------------------------------------------------------
LENGTHS = np.array([0, 1, 2, 3, 4, 7, 2 ** 20 - 1, 2 ** 20], np.float32)


def history(rng, cur, prev, k, d, w, h, moments):
    """A history that mostly matches what `cur` sees (test_temporal_host.synthetic_history without its NaN depths): depths of the reprojected points, a few
    percent off on some taps (most pass the 0.1 bound, some fail), coverage flipped to 0 or from 0 on a tenth, lengths from LENGTHS -- 0, 1 and 2^20 among them."""
    hc = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    V = rng.uniform(0.0, 0.1, (h, w))
    _, _, sdp, _ = ht.spec_reproject(cur, prev, k, d)
    sdp = np.where(np.isfinite(sdp), sdp, 1.4)
    K = np.where(rng.random((h, w)) < 0.1, np.where(k > 0, 0.0, 0.5), k)
    D = np.where(K > 0, np.where(k > 0, sdp, 1.4) * rng.choice([1.0, 1.0, 1.0, 1.03, 0.95, 1.3, 0.7], (h, w)), 0.0)
    N = rng.choice(LENGTHS, (h, w))
    rec = f32(np.stack([V, N, K, D], axis=-1))
    if not moments:
        return (f32(prev), hc, rec)
    m1 = rng.uniform(0.2, 1.5, (h, w))
    mom = f32(np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.5, (h, w)), rng.uniform(0.05, 1.0, (h, w)), rng.uniform(0.0, 0.5, (h, w))], axis=-1))
    return (f32(prev), hc, rec, mom)


def _translated(cam, right, up):
    """the camera moved by `right` along its own x axis and `up` along its own y axis (13 float32: pos, columns right / up / -forward, cam_z)"""
    out = cam.copy()
    out[0:3] = cam[0:3] + np.float32(right) * cam[3:6] + np.float32(up) * cam[6:9]
    return out


def taps_inside(u, w, ok, W, H):
    """how many of a pixel's four taps lie inside the frame, from the host build's reprojection; 0 where it has none"""
    x0, y0 = np.floor(u).astype(np.int64), np.floor(w).astype(np.int64)
    nx = ((x0 >= 0) & (x0 < W)).astype(int) + ((x0 + 1 >= 0) & (x0 + 1 < W)).astype(int)
    ny = ((y0 >= 0) & (y0 < H)).astype(int) + ((y0 + 1 >= 0) & (y0 + 1 < H)).astype(int)
    return np.where(ok, nx * ny, 0)


FORMS = ("plain", "reject", "moments")


def temporal_cases(form):
    assert form in FORMS
    moments = form == "moments"
    col, v, g, _ = base()
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    out = []
    cur0, prev0 = orbit_camera(11.0, height=0.3), orbit_camera(10.0, height=0.25)

    def add(name, cur=cur0, hist="prev0", color=col, var=v, guide=g, w=W0, h=H0, alpha=0.1, tau=3.0, seed=0, **kw):
        rng = np.random.default_rng(4000 + seed)
        gk, gd = np.ascontiguousarray(guide[..., 3]), np.ascontiguousarray(guide[..., 7])
        if isinstance(hist, str):
            hist = history(rng, cur, prev0, gk, gd, w, h, moments)
        elif hist is not None and not isinstance(hist, tuple):
            hist = history(rng, cur, hist, gk, gd, w, h, moments)
        out.append(Case("temporal", "%s-%s" % (form, name), w, h, {"color": color, "v": var, "guide": guide, "hist": hist},
                        {"cur": f32(cur), "alpha": alpha, "tau": tau if form == "reject" else 0.0, "form": form, "sigma": SIGMA}, **kw))

    add("no-history", hist=None)
    add("same-camera", hist=cur0, seed=1)
    add("orbit-1deg", seed=2)
    add("translated", hist=_translated(cur0, 0.035, 0.02), seed=3)          # a band reprojects to u in [-1, 0) and [W - 1, W), w likewise: one, two and four taps
    add("translated-back", hist=_translated(cur0, -0.05, -0.03), seed=4)
    add("turned-180", cur=orbit_camera(10.0, yaw_deg=180.0), hist=orbit_camera(10.0), seed=5)      # everything lies behind the history's camera
    add("fov", cur=orbit_camera(10.0, fov=50.0), hist=orbit_camera(10.0, fov=40.0), seed=6)
    for w, h in SMALL:
        c2, v2, g2, _ = base(w, h, seed=13)
        add("%dx%d" % (w, h), color=c2, var=v2, guide=g2, w=w, h=h, seed=7)
    # depths that differ by exactly 10 % and by one ulp either side, under the unchanged camera (u = px, d' = d bit for bit): D = d / 0.9 rounded, and its neighbours
    rng = np.random.default_rng(4100)
    hist = list(history(rng, cur0, cur0, k, d, W0, H0, moments))
    rec = hist[2].copy()
    edge = f32(d / np.float32(0.9))
    x = np.arange(W0)[None, :] % 3
    D = np.where(x == 0, edge, np.where(x == 1, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))))
    rec[..., 2] = k
    rec[..., 3] = np.where((k > 0) & (d > 0), D, 0.0)
    rec[..., 1] = 5.0
    hist[2] = f32(rec)
    add("depth-bound", hist=tuple(hist))
    for alpha in (2.0 ** -20, 1.0):
        add("alpha-%g" % alpha, alpha=alpha, seed=8)
    if form == "reject":
        for tau in (2.0 ** -10, 2.0 ** 20):
            add("tau-%g" % tau, tau=tau, seed=9)
        add("tau-3-same-camera", hist=cur0, tau=3.0, seed=9)
    if form != "moments":
        add("v0", var=np.zeros_like(v), seed=10)                             # with a zero history variance too: z2 = difference^2 / 1e-12
        h0 = list(history(np.random.default_rng(4110), cur0, cur0, k, d, W0, H0, False))
        h0[2] = h0[2].copy()
        h0[2][..., 0] = 0.0
        add("v0-both", hist=tuple(h0), var=np.zeros_like(v))
    else:
        rng = np.random.default_rng(4120)
        hist = list(history(rng, cur0, cur0, k, d, W0, H0, True))
        rec, mom = hist[2].copy(), hist[3].copy()
        rec[..., 1] = np.where(np.arange(W0)[None, :] % 2 == 0, 2.0, 3.0)     # N + 1 = 3 and 4 side by side: pass 2 pools the one and not the other
        m1 = mom[..., 0]
        sq = m1 * m1                                                         # m2 = m1^2 but for a rounding, down or up row by row: S is clamped at 0, or just is not
        mom[..., 1] = np.where(np.arange(H0)[:, None] % 2 == 0, np.nextafter(sq, np.float32(0.0)), np.nextafter(np.nextafter(sq, np.float32(4.0)), np.float32(4.0)))
        hist[2], hist[3] = f32(rec), f32(mom)
        grey = f32(np.repeat(m1[..., None], 4, axis=-1))                     # the frame's luminance is the history's m1: the blended m2 - m1^2 is rounding alone, of either sign
        add("n3-n4-clamped", hist=tuple(hist), color=grey, alpha=2.0 ** -20)
        one = np.zeros_like(g)
        one[H0 // 2, W0 // 2] = g[g[..., 3] > 0][0]
        add("one-covered-pixel", guide=one, hist=None)
        add("one-covered-pixel-history", guide=one, hist=cur0, seed=11)
    bad = col.copy()
    bad[10:12, 20:22, 1] = np.nan                        # 2 x 2 texels each, so that one of them at least has a history
    bad[25:27, 40:42, 0] = np.inf
    add("nan-inf-texel", color=bad, hist=cur0, seed=12, nonfinite=True)
    add("nan-inf-texel-moved", color=bad, seed=12, nonfinite=True)
    return out


def _temporal_host(c):
    p, i = c.par, c.inp
    g = i["guide"]
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    with np.errstate(all="ignore"):
        if p["form"] == "moments":
            C, R, M = hm.step(p["cur"], i["color"], g, p["alpha"], p["sigma"], i["hist"], checked=True)
            return {"color": C, "record": R, "v": np.ascontiguousarray(R[..., 0]), "moments": M}
        if p["form"] == "reject":
            C, R, T = ht.step_reject(p["cur"], i["color"], i["v"], k, d, p["alpha"], p["tau"], i["hist"], checked=True)
            return {"color": C, "record": R, "v": np.ascontiguousarray(R[..., 0]), "T": T}
        C, R = ht.step(p["cur"], i["color"], i["v"], k, d, p["alpha"], i["hist"], checked=True)
    return {"color": C, "record": R, "v": np.ascontiguousarray(R[..., 0])}


def _temporal_device(r, c):
    p, i = c.par, c.inp
    hist = i["hist"]
    px = (c.h, c.w)
    moments, reject = p["form"] == "moments", p["form"] == "reject"
    ins = [i["color"], i["v"], i["guide"]] + ([None] * 3 if hist is None else [hist[1], hist[2], hist[3] if moments else None])
    prev = p["cur"] if hist is None else hist[0]
    same = hist is not None and f32(prev).tobytes() == f32(p["cur"]).tobytes()      # as the renderer decides it: byte for byte
    C, R, v, M, scratch = r.filter_probe("temporal", c.w, c.h, ins, [px + (4,), px + (4,), px, px + (4,) if moments else None, px + (4,) if reject else None],
                                         sigma=p["sigma"], x=p["alpha"], tau=p["tau"], i1=int(same), cur=p["cur"], prev=prev)
    out = {"color": C, "record": R, "v": v}
    if moments:
        out["moments"] = M
    if reject:
        out["T"] = np.ascontiguousarray(scratch[..., 0])
    return out


# ---- resolve ----------------------------------------------------------------------------------------------------------------------------------------------
_ORACLES = {}


def oracle(scene, w, h):
    """the CPU oracle's renderer of a scene at a size, for the environment behind each pixel: c2 (the sky shown), c3env (under the LUT, the sky shown), c2hid (hidden)"""
    from test_resolve_host import _oracle
    if (scene, w, h) not in _ORACLES:
        _ORACLES[(scene, w, h)] = _oracle(scene, w, h)
    return _ORACLES[(scene, w, h)]


def _thirds(rng, w, h, axis):
    """0, 1 and a fraction by the pixel's raster index i: i % 3 (axis 0) or (i // 3) % 3 (axis 1), so that the two arrays together run through all nine
    combinations every nine pixels, on a frame one pixel wide too"""
    y, x = np.mgrid[0:h, 0:w]
    sel = (y * w + x) % 3 if axis == 0 else ((y * w + x) // 3) % 3
    return f32(np.where(sel == 0, 0.0, np.where(sel == 1, 1.0, rng.integers(1, 8, (h, w)) / 8.0)))


def resolve_cases():
    out = []
    for scene, sizes, rays_of in (("c2", ((W0, H0),) + SMALL, (2, 4)), ("c3env", ((W0, H0),), (2,)), ("c2hid", ((W0, H0), (17, 16)), (2, 4))):
        for w, h in sizes:
            rng = np.random.default_rng(5000 + 7 * w + h)
            fb = f32(rng.uniform(0.0, 1.0, (h, w, 4)))
            fb[..., 3] = _thirds(rng, w, h, 0)
            sky = hr.prepare(oracle(scene, w, h), 2, np.zeros((h, w, 4), np.float32))[0]
            fb[..., :3] = (1.0 - fb[..., 3:4]) * sky[..., :3] + fb[..., 3:4] * fb[..., :3]      # the samples that missed saw the sky: a frame the path tracer can leave
            feat = frame(w, h, seed=17)[2]
            feat[..., 3] = _thirds(rng, w, h, 1)
            for rays in rays_of if (w, h) == (W0, H0) else (2,):
                out.append(Case("resolve", "%s-%dx%d-rays%d" % (scene, w, h, rays), w, h, {"fb": fb, "feat": feat}, {"rays": rays}, scene=scene))
    return out


def _resolve_host(c):
    fb = c.inp["fb"]
    B, P = hr.prepare(oracle(c.scene, c.w, c.h), c.par["rays"], fb)
    return {"B": B, "P": P, "y": hr.resolve(fb, B, P, np.ascontiguousarray(c.inp["feat"][..., 3]))}


def _resolve_device(r, c):
    px = (c.h, c.w, 4)
    B, P, y = r.filter_probe("resolve", c.w, c.h, [c.inp["fb"], c.inp["feat"]], [px, px, px], i0=c.par["rays"])
    return {"B": B, "P": P, "y": y}


# ---- split / merge ----------------------------------------------------------------------------------------------------------------------------------------
KAPPAS = np.array([0.0, 2.0 ** -21, 2.0 ** -20, 2.0 ** -19, 1.0, 0.375], np.float32)


def layers_cases():
    rng = np.random.default_rng(6000)
    feat = frame()[2]
    feat[..., 3] = rng.choice(KAPPAS, (H0, W0))
    B = f32(rng.uniform(0.0, 3.0, (H0, W0, 4)))
    B[..., 3] = 0.0
    y = f32(rng.uniform(0.0, 2.0, (H0, W0, 4)))             # below B on about half the pixels: S is signed
    y[..., 3] = feat[..., 3]
    out = [Case("split", "kappas", W0, H0, {"y": y, "B": B, "feat": feat}),
           Case("split", "levels", W0, H0, {"y": f32(base()[0]), "B": f32(B * 1e3), "feat": feat})]
    S = hl.split(y, B, np.ascontiguousarray(feat[..., 3]))
    other = S.copy()
    other[..., 3] = rng.choice(KAPPAS, (H0, W0))            # F.a different from kappa: what the a-trous leaves
    out.append(Case("merge", "alpha-differs", W0, H0, {"F": other, "B": B, "feat": feat}))
    out.append(Case("merge", "alpha-is-kappa", W0, H0, {"F": S, "B": B, "feat": feat}))      # what the regression leaves
    return out


def _split_host(c):
    with np.errstate(all="ignore"):
        if c.par.get("demod"):
            return {"S": hd.split(c.inp["y"], c.inp["B"], c.inp["feat"])}
        return {"S": hl.split(c.inp["y"], c.inp["B"], np.ascontiguousarray(c.inp["feat"][..., 3]))}


def _split_device(r, c):
    return {"S": r.filter_probe("split", c.w, c.h, [c.inp["y"], c.inp["B"], c.inp["feat"]], [(c.h, c.w, 4)], demod=bool(c.par.get("demod")))[0]}


def _merge_host(c):
    with np.errstate(all="ignore"):
        if c.par.get("demod"):
            out, L = hd.merge(c.inp["F"], c.inp["B"], c.inp["feat"])
        else:
            out, L = hl.merge(c.inp["F"], c.inp["B"], np.ascontiguousarray(c.inp["feat"][..., 3]))
    return {"out": out, "L": L}


def _merge_device(r, c):
    out, L = r.filter_probe("merge", c.w, c.h, [c.inp["F"], c.inp["B"], c.inp["feat"]], [(c.h, c.w, 4)] * 2, demod=bool(c.par.get("demod")))
    return {"out": out, "L": L}


# ---- regress ----------------------------------------------------------------------------------------------------------------------------------------------
RIDGES = (0.0, 2.0 ** -20, 0.01, 1.0, 2.0 ** 20)


def regress_guides():
    """name -> (S, guide) at 47x33.  S: the hostile colour as a layer, alpha = the guide's coverage unless the guide's name says otherwise."""
    col, _, g, _ = base()
    rng = np.random.default_rng(7000)
    y, x = np.mgrid[0:H0, 0:W0]

    def layer(guide, alpha=None):
        S = f32(rng.uniform(0.0, 2.0, (H0, W0, 4)))
        S[..., 3] = guide[..., 3] if alpha is None else alpha
        S[..., :3] *= S[..., 3:4]                         # premultiplied, as the split leaves it
        return S

    flat = np.zeros_like(g)
    flat[...] = np.array([0.5, 0.25, 0.75, 1.0, 0.0, 0.0, 1.0, 2.0], np.float32)      # exactly constant over whole windows: every slope column is empty
    albedo = g.copy()
    albedo[..., 0:3] = np.array([0.5, 0.25, 0.75], np.float32)
    albedo[..., 3] = np.where(g[..., 3] > 0, g[..., 3], 0.5)
    albedo[..., 7] = np.where(g[..., 7] > 0, g[..., 7], 1.5)
    multiple = flat.copy()                                    # albedo.g = 2 * albedo.r exactly, all else constant: one regressor an exact multiple of another
    multiple[..., 0] = f32(rng.integers(0, 64, (H0, W0)) / 256.0)
    multiple[..., 1] = multiple[..., 0] * np.float32(2.0)
    lone = flat.copy()                                        # exactly one covered tap per window, the centre: covered pixels 11 apart
    lone[..., 3] = np.where((x % 11 == 5) & (y % 11 == 5), 1.0, 0.0)
    faint = flat.copy()                                       # the same, but the centre's S.a is at or below 2^-20 while its guide is covered: A_00 <= 2^-20
    faint[..., 3] = lone[..., 3]
    faint_alpha = np.where((x // 11) % 2 == 0, 2.0 ** -20, 2.0 ** -21) * lone[..., 3]
    depth0 = albedo.copy()
    depth0[..., 7] = np.where((x + y) % 2 == 0, 0.0, albedo[..., 7])      # depth 0 at every other centre: rd = 2^20
    checker = g.copy()
    checker[..., 3] = np.where((x + y) % 2 == 0, np.maximum(g[..., 3], 0.125), 0.0)
    # pits: every other pixel has depth 0 and a layer without coverage under a covered guide (what a blended history can leave), all others the depth 2^-10
    # exactly.  At a pit rd = 2^20 and every tap that counts has the depth regressor 1024 exactly: its column is the intercept's times 1024, the pivot is the ridge
    # plus the rounding of A_11 - l A_01, about 2^-24 * 2^20 A_00 -- above lambda A_00 for the small ridges, so the pivot's sign is rounding's and columns drop
    pit = flat.copy()
    at_pit = (x + y) % 2 == 0
    pit[..., 7] = np.where(at_pit, 0.0, 2.0 ** -10)
    pit_alpha = np.where(at_pit, 0.0, 1.0)
    return {"flat": (layer(flat), flat), "albedo-flat": (layer(albedo), albedo), "multiple": (layer(multiple), multiple), "lone": (layer(lone), lone),
            "faint": (layer(faint, faint_alpha), faint), "depth0": (layer(depth0), depth0), "hostile": (f32(np.concatenate([col[..., :3], g[..., 3:4]], axis=-1)), g),
            "checker": (layer(checker), checker), "pit": (layer(pit, pit_alpha), pit)}


def regress_cases():
    out = []
    for name, (S, g) in regress_guides().items():
        for ridge in RIDGES:
            out.append(Case("regress", "%s-ridge%g" % (name, ridge), W0, H0, {"S": S, "guide": g}, {"ridge": ridge, "sigma": SIGMA}))
    for w, h in SMALL:
        c2, _, g2, _ = base(w, h, seed=13)
        S = f32(np.concatenate([c2[..., :3], g2[..., 3:4]], axis=-1))
        for ridge in (0.0, 0.01):
            out.append(Case("regress", "%dx%d-ridge%g" % (w, h, ridge), w, h, {"S": S, "guide": g2}, {"ridge": ridge, "sigma": SIGMA}))
    S, g = regress_guides()["albedo-flat"]
    bad = S.copy()
    bad[10, 20, 1] = np.nan
    bad[25, 40, 0] = np.inf
    for ridge in (0.0, 0.01):
        out.append(Case("regress", "nan-inf-texel-ridge%g" % ridge, W0, H0, {"S": bad, "guide": g}, {"ridge": ridge, "sigma": SIGMA}, nonfinite=True))
    return out


def _regress_host(c):
    with np.errstate(all="ignore"):
        return {"F": hg.regress(c.inp["S"], c.inp["guide"], c.par["ridge"], c.par["sigma"])}


def _regress_device(r, c):
    return {"F": r.filter_probe("regress", c.w, c.h, [c.inp["S"], c.inp["guide"]], [(c.h, c.w, 4)], sigma=c.par["sigma"], x=c.par["ridge"])[0]}


# ---- upsample ---------------------------------------------------------------------------------------------------------------------------------------------
# lo size -> factors: every f of 2..4 on at least two lo sizes and on a frame with corners (f = 4: 12x12, a hi frame of 3 x 3 tiles), and no hi frame of more
# pixels than 64x48 (17x16 and 12x20 times 4 would hold more)
UPSAMPLE_SHAPES = (((1, 37), (2, 3, 4)), ((37, 1), (2, 3, 4)), ((17, 16), (2, 3)), ((12, 20), (2, 3)), ((12, 12), (4,)))


def _upsample_case(scene, w, h, f, demod=False):
    """demod: the albedo words of the lo and of the hi features drawn per channel from ALBEDOS (under the hi checkerboard the lo pixel's own), kept where the
    coverage is 0"""
    rng = np.random.default_rng(8000 + 100 * f + 7 * w + h)
    lo_feat = frame(w, h, seed=19)[2]
    hi = frame(f * w, f * h, seed=23)[2]
    if demod:
        arng = np.random.default_rng(8500 + 100 * f + 7 * w + h)
        lo_feat[..., 0:3] = arng.choice(ALBEDOS, (h, w, 3))
        hi[..., 0:3] = arng.choice(ALBEDOS, (f * h, f * w, 3))
    glo = hu.guide(lo_feat)
    L = f32(rng.uniform(0.0, 1.0, (h, w, 4)))
    L[..., 3] = glo[..., 3]
    L[..., :3] *= L[..., 3:4]                 # premultiplied, as the merge leaves it
    rep = np.repeat(np.repeat(lo_feat, f, axis=0), f, axis=1)      # the lo features under every hi pixel: a hi guide equal to a lo tap's bit for bit
    y, x = np.mgrid[0:f * h, 0:f * w]
    hi = np.where(((x // 4 + y // 4) % 2 == 0)[..., None], rep, hi)
    flip = rng.random((f * h, f * w)) < 0.15                       # hi coverage 0 where lo is covered, and the reverse
    hi[..., 3] = np.where(flip, np.where(rep[..., 3] > 0, 0.0, 0.625), hi[..., 3])
    albedo = hi[..., 0:3].copy()
    hi[hi[..., 3] == 0] = 0.0
    if demod:
        hi[..., 0:3] = albedo
    par = {"f": f, "rays": 2, "sigma": SIGMA}
    if demod:
        par["demod"] = 1
    return Case("upsample", "%s%s-%dx%d-f%d" % ("demod-" if demod else "", scene, w, h, f), w, h, {"L": L, "glo": glo, "feat_hi": f32(hi)}, par, scene=scene)


def upsample_cases():
    out = []
    for scene in ("c2", "c3env"):
        for (w, h), factors in UPSAMPLE_SHAPES:
            for f in factors:
                if scene == "c3env" and (w, h) != (17, 16):
                    continue
                out.append(_upsample_case(scene, w, h, f))
    return out


def _upsample_host(c):
    f = c.par["f"]
    B, _ = hr.prepare(oracle(c.scene, f * c.w, f * c.h), c.par["rays"], np.zeros((f * c.h, f * c.w, 4), np.float32))
    up = (lambda *a: hd.upsample(*a, staged=False)) if c.par.get("demod") else hu.upsample
    out, L = up(c.inp["L"], c.inp["glo"], hu.guide(c.inp["feat_hi"]), B, f, c.par["sigma"])
    return {"out": out, "L": L}


def _upsample_device(r, c):
    f = c.par["f"]
    hi = (f * c.h, f * c.w, 4)
    out, L = r.filter_probe("upsample", c.w, c.h, [c.inp["L"], c.inp["glo"], c.inp["feat_hi"]], [hi, hi], sigma=c.par["sigma"], i0=c.par["rays"], i1=f, demod=bool(c.par.get("demod")))
    return {"out": out, "L": L}


# ---- adaptive error ---------------------------------------------------------------------------------------------------------------------------------------
def adaptive_cases():
    rng = np.random.default_rng(9000)
    col, S, _ = frame()
    mu = col.copy()
    mu[16:32, 16:32, :3] = 0.0                              # tile (1, 1): luma 0, the divisor is the floor 2^-10
    mu[0:8, 40:47, :3] = 0.0                                # and a part of the ragged tile (0, 2)
    tiles = np.array([8, 0, 4, 2, 6, 1, 7, 3, 5], np.int32)      # every tile, the ragged ones (2, 5, 6, 7, 8) among them, out of order
    counts = np.array([1000, 1, 2, 2, 1, 1000, 3, 2 ** 20, 2], np.int32)
    out = [Case("adaptive_error", "all-tiles", W0, H0, {"fb": mu, "S": S, "tiles": tiles, "counts": counts}),
           Case("adaptive_error", "edge-tiles", W0, H0, {"fb": mu, "S": S, "tiles": np.array([8, 2, 6], np.int32), "counts": np.array([2, 1000, 2], np.int32)}),
           Case("adaptive_error", "tiny-moments", W0, H0, {"fb": mu, "S": f32(rng.choice(np.array([0.0, 1e-38, 1e-44, 1e-30], np.float32), (H0, W0, 4))), "tiles": tiles, "counts": counts})]
    bad = S.copy()
    bad[20, 20, 1] = np.nan                                 # tile (1, 1): e_t is NaN, as the header says
    out.append(Case("adaptive_error", "nan-moment", W0, H0, {"fb": mu, "S": bad, "tiles": tiles, "counts": np.full(9, 2, np.int32)}, nonfinite=True))
    return out


def _adaptive_host(c):
    ty, tx = ha.tiles_of(c.w, c.h)
    counts = np.full(ty * tx, 2, np.int32)
    counts[c.inp["tiles"]] = c.inp["counts"]
    with np.errstate(all="ignore"):
        e = ha.tile_error(c.inp["fb"], c.inp["S"], counts.reshape(ty, tx))
    return {"e": np.ascontiguousarray(e.reshape(-1)[c.inp["tiles"]])}


def _adaptive_device(r, c):
    n = len(c.inp["tiles"])
    return {"e": r.filter_probe("adaptive_error", c.w, c.h, [c.inp["fb"], c.inp["S"], c.inp["tiles"], c.inp["counts"]], [(n,)], i0=n)[0]}


# ---- the DEMOD instances of prepare, split, merge and upsample (vr_demod.h; par["demod"] = 1) -----------------------------------------------------------------
_FLOOR = np.float32(2.0 ** -6)
# per channel: nothing, a signed nothing, a subnormal, below the floor, the floats around the floor, ordinary, 1 and the float above it, above 1, far above, negative
ALBEDOS = np.array([0.0, -0.0, 1e-40, 2.0 ** -7, np.nextafter(_FLOOR, np.float32(0)), _FLOOR, np.nextafter(_FLOOR, np.float32(1)), 0.5, 1.0,
                    np.nextafter(np.float32(1), np.float32(2)), 4.0, 1e5, -0.25], np.float32)


def demod_features(seed, w=W0, h=H0):
    """the hostile features with the coverage drawn from KAPPAS and every albedo word from ALBEDOS -- on the pixels without coverage too: d = 1 has to ignore them"""
    rng = np.random.default_rng(seed)
    feat = frame(w, h)[2]
    feat[..., 3] = rng.choice(KAPPAS, (h, w))
    feat[..., 0:3] = rng.choice(ALBEDOS, (h, w, 3))
    return feat


def poisoned(feat):
    """the fourth non-finite kind: one albedo channel NaN on some pixels and +inf on others, covered and uncovered ones among both.  -> (features, NaN mask
    [H][W][3], inf mask [H][W][3])"""
    h, w = feat.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    ch = (x + y) % 3
    nan_px, inf_px = (x % 5 == 1) & (y % 4 == 2), (x % 5 == 3) & (y % 4 == 0)
    is_nan, is_inf = (nan_px[..., None] & (ch[..., None] == np.arange(3))), (inf_px[..., None] & (ch[..., None] == np.arange(3)))
    out = feat.copy()
    out[..., 0:3] = np.where(is_nan, np.float32(np.nan), np.where(is_inf, np.float32(np.inf), feat[..., 0:3]))
    return out, is_nan, is_inf


def demod_cases():
    rng = np.random.default_rng(6500)
    par = {"demod": 1}
    out = []
    kap, lev = (c for c in layers_cases() if c.stage == "split")
    # -- split
    feat = demod_features(6501)
    y = kap.inp["y"].copy()
    y[..., 3] = feat[..., 3]
    out.append(Case("split", "demod-albedos", W0, H0, {"y": y, "B": kap.inp["B"], "feat": feat}, par))
    out.append(Case("split", "demod-levels", W0, H0, {"y": lev.inp["y"], "B": lev.inp["B"], "feat": demod_features(6502)}, par))
    # no background, so S = y / d: 1e-36 .. 1e-38 over 1e5 in the left half of the frame lands in the subnormal range, where the division's result is denormalised
    sub = demod_features(6503)
    sub[:, : W0 // 2, 0:3] = np.float32(1e5)
    tiny = f32(rng.choice(np.array([1e-36, 1e-37, 1e-38], np.float32), (H0, W0, 4)))
    tiny[..., 3] = sub[..., 3]
    out.append(Case("split", "demod-subnormal-quotient", W0, H0, {"y": tiny, "B": np.zeros_like(tiny), "feat": sub}, par))
    huge = f32(rng.choice(np.array([3e38, 1e30, 1.0], np.float32), (H0, W0, 4)))         # 3e38 over the floor overflows, over 4 and 1e5 it does not
    huge[..., 3] = feat[..., 3]
    out.append(Case("split", "demod-overflow-quotient", W0, H0, {"y": huge, "B": np.zeros_like(huge), "feat": feat}, par, nonfinite=True))
    bad, _, _ = poisoned(feat)
    out.append(Case("split", "demod-nan-inf-albedo", W0, H0, {"y": y, "B": kap.inp["B"], "feat": bad}, par, nonfinite=True))
    # -- prepare
    pfeat = demod_features(6504)
    for c in prepare_cases():
        if c.name == "tiny-n1048576":
            continue
        out.append(Case("prepare", "demod-" + c.name, W0, H0, dict(c.inp, feat=pfeat), dict(c.par, demod=1), nonfinite=c.nonfinite))
    hostile_counts = next(c for c in prepare_cases() if c.name == "counts")
    out.append(Case("prepare", "demod-nan-inf-albedo", W0, H0, dict(hostile_counts.inp, feat=poisoned(pfeat)[0]), dict(hostile_counts.par, demod=1), nonfinite=True))
    # -- merge, on the demodulated S
    S = hd.split(y, kap.inp["B"], feat)
    other = S.copy()
    other[..., 3] = rng.choice(KAPPAS, (H0, W0))
    out.append(Case("merge", "demod-alpha-differs", W0, H0, {"F": other, "B": kap.inp["B"], "feat": feat}, par))
    out.append(Case("merge", "demod-alpha-is-kappa", W0, H0, {"F": S, "B": kap.inp["B"], "feat": feat}, par))
    big = S.copy()
    big[..., :3] = f32(rng.choice(np.array([1e34, 1.0, -1e34, 1e-3], np.float32), (H0, W0, 3)))      # 1e34 times 1e5 overflows, times 4 it does not
    out.append(Case("merge", "demod-overflow", W0, H0, {"F": big, "B": kap.inp["B"], "feat": feat}, par, nonfinite=True))
    out.append(Case("merge", "demod-nan-inf-albedo", W0, H0, {"F": other, "B": kap.inp["B"], "feat": bad}, par, nonfinite=True))
    # -- upsample: no non-finite word here, the guides feed the edge weights of every tap
    for scene, (w, h), factors in (("c3env", (17, 16), (2, 3)), ("c2", (1, 37), (2, 3, 4)), ("c2", (37, 1), (2, 3, 4)), ("c2", (12, 12), (4,))):
        for f in factors:
            out.append(_upsample_case(scene, w, h, f, demod=True))
    return out


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------------------------
_HOST ={"prepare": _prepare_host, "atrous": _atrous_host, "temporal": _temporal_host, "resolve": _resolve_host, "split": _split_host, "merge": _merge_host,
         "regress": _regress_host, "upsample": _upsample_host, "adaptive_error": _adaptive_host}
_DEVICE = {"prepare": _prepare_device, "atrous": _atrous_device, "temporal": _temporal_device, "resolve": _resolve_device, "split": _split_device,
           "merge": _merge_device, "regress": _regress_device, "upsample": _upsample_device, "adaptive_error": _adaptive_device}
# the groups the two test files parametrise over: the three temporal forms apart, split and merge together
GROUPS = {"prepare": prepare_cases, "atrous": atrous_cases, "temporal-plain": lambda: temporal_cases("plain"), "temporal-reject": lambda: temporal_cases("reject"),
          "temporal-moments": lambda: temporal_cases("moments"), "resolve": resolve_cases, "layers": layers_cases, "regress": regress_cases,
          "upsample": upsample_cases, "adaptive_error": adaptive_cases, "demod": demod_cases}
_CASES, _RESULTS = {}, {}


def cases(group):
    if group not in _CASES:
        _CASES[group] = GROUPS[group]()
        ids = [c.id for c in _CASES[group]]
        assert len(set(ids)) == len(ids), ids
    return _CASES[group]


def host(case):
    """the host build's outputs of a case, name -> float32 array; computed once per process and not to be changed"""
    if case.id not in _RESULTS:
        _RESULTS[case.id] = _HOST[case.stage](case)
    return _RESULTS[case.id]


def device(r, case):
    """the kernel's outputs of a case through r.filter_probe, under the same names"""
    return _DEVICE[case.stage](r, case)


def first_difference(case, name, got, want):
    """where and how a device output differs from the host build's: the stage, the case, the first differing pixel and its inputs (None: they agree).  Bit for bit,
    but for a non-finite case, where a NaN may be any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (case.id, name, got.shape, want.shape)
    ok = got.view(np.uint32) == want.view(np.uint32)
    if case.nonfinite:
        ok |= np.isnan(got) & np.isnan(want)
    if ok.all():
        return None
    at = tuple(int(i) for i in np.argwhere(~ok)[0])
    lines = ["%s: output %r differs from the host build in %d of %d words; first at %r: device %r (0x%08x), host %r (0x%08x)"
             % (case.id, name, int((~ok).sum()), ok.size, at, float(got[at]), int(got.view(np.uint32)[at]), float(want[at]), int(want.view(np.uint32)[at]))]
    px = at[:2] if got.ndim >= 2 else None
    for key, a in case.inp.items():
        if isinstance(a, tuple):
            for j, part in enumerate(a[1:]):
                if px is not None and part.shape[:2] == got.shape[:2]:
                    lines.append("  hist[%d] at %r = %r" % (j + 1, px, part[px].tolist()))
        elif a is not None and px is not None and np.asarray(a).shape[:2] == got.shape[:2]:
            lines.append("  %s at %r = %r" % (key, px, np.asarray(a)[px].tolist()))
    lines.append("  parameters: %r" % ({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in case.par.items()},))
    return "\n".join(lines)
