"""One host model of the image-space state of a renderer (include/volren_amd.h): which frame a denoise call starts from, what it leaves in
`denoised`, the layer, the history, the statistic, the resolved frame and the upsampled frames, which setting drops the history, and what every refused call
says and leaves behind.  The arithmetic is the host builds' (hk_denoise, hk_adaptive, hk_temporal, hk_moments, hk_resolve, hk_layers, hk_regress,
hk_upsample, hk_demod); nothing of the path tracer is stated here: a frame, its variance, its features and its sample counts are inputs (new_frame).  Plus the two
generators the tests of the pipeline share: a greedy all-pairs array over the denoiser's settings and random call sequences.  TEST HARNESS ONLY.

Written from the header's text, not from RendererHIP::run_denoise.  Where several refusals apply at once the header ranks none of them: Refused carries every
reason that holds, and the product's message has to be one of them."""
import itertools

import numpy as np

import hk_adaptive
import hk_common
import hk_demod
import hk_denoise
import hk_layers
import hk_moments
import hk_regress
import hk_resolve
import hk_temporal
import hk_upsample

# the distinguishing words of every refusal, as the refused(...) helpers of the GPU tests match them
REFUSALS = {
    "tiles": "a tile subset is set",
    "no_features": "no feature pass since the last resize",
    "no_samples": "the framebuffer holds no samples",
    "moments_cover": "the moments do not cover",
    "moments_reject": "do not go together",
    "not_expected": "was not last filled by render_features_expected",
    "one_ray": "rays >= 2 is needed",
    "filter_layers": "denoise_filter = 1 needs denoise_layers = 1",
    "demod_layers": "denoise_demodulate = 1 needs denoise_layers = 1",
    "empty_tile": "a tile of the frame holds no samples",
    "no_layer": "no denoise with denoise_layers = 1 since the last resize",
    "stale_guide": "the last denoise ran with denoise_layers = 0",
    "no_denoised": "no denoise since the last resize",
    "no_history": "no history",
    "no_history_moments": "no history with moment records",
    "no_stat": "did not run with denoise_reject > 0",
    "no_resolve": "no resolve since the last resize",
    "no_upsample": "no upsample since the last resize",
}
CALL_REFUSALS = ("tiles", "no_features", "no_samples", "moments_cover", "moments_reject", "not_expected", "one_ray", "filter_layers", "demod_layers", "empty_tile",
                 "no_layer", "stale_guide")
SWITCHES = ("denoise_moments", "denoise_resolve", "denoise_layers", "denoise_filter", "denoise_demodulate")      # 0 or 1; a change drops the history
DROP_RULES = tuple("switch:" + s for s in SWITCHES) + ("history_reset", "resize", "mismatch")
SIGMA2 = (2.0, 3.0, 0.3, 0.5, 0.5)


class Refused(Exception):
    """A call the header refuses.  kinds: every reason that holds (keys of REFUSALS); words: their distinguishing words."""

    def __init__(self, who, kinds):
        self.who, self.kinds = who, tuple(kinds)
        self.words = tuple(REFUSALS[k] for k in self.kinds)
        Exception.__init__(self, "%s: %s" % (who, " | ".join(self.words)))

    def matches(self, message):
        return any(w in message for w in self.words)


# ---- the scene: what the two scene-bound stages (resolve, upsample) need, kept under the renderer's camera ------------------------------------------------
def _orbit(x, degrees):
    import gpu_frames
    gpu_frames._orbit(x, degrees)


class OracleScene:
    """The oracle's scene `name` at the renderer's size and at the upsampled sizes, all under one camera."""

    def __init__(self, name, w, h):
        self.name, self.w, self.h, self.degrees, self._o = name, int(w), int(h), None, {}

    def _at(self, w, h):
        import test_resolve_host
        if (w, h) not in self._o:
            self._o[w, h] = [test_resolve_host._oracle(self.name, w, h), None]
        slot = self._o[w, h]
        if slot[1] != self.degrees:
            _orbit(slot[0], self.degrees)
            slot[1] = self.degrees
        return slot[0]

    def orbit(self, degrees):
        self.degrees = float(degrees)

    def resize(self, w, h):
        self.w, self.h = int(w), int(h)

    def lo(self):
        return self._at(self.w, self.h)

    def camera(self):
        p = self.lo().params()
        return hk_temporal.camera(list(p.cam_pos), list(p.cam_transform), fov_degree=float(p.cam_fov))

    def resolved(self, rays, fb, feat):
        return hk_resolve.resolved(self.lo(), rays, fb, feat)

    def upsampled(self, layer, feat_lo, f, rays, sigma, demod=False):
        """-> (out, L, hi features); demod: "denoise_demodulate" at the call"""
        chain = hk_demod.chain if demod else hk_upsample.chain
        return chain(layer, feat_lo, self._at(f * self.w, f * self.h), rays, f, sigma)[:3]


class BlankScene:
    """A scene without light, for runs that count calls and never compare pixels: B = 0, y = the frame with the guide's coverage."""

    def __init__(self, w, h):
        self.w, self.h = int(w), int(h)

    def orbit(self, degrees):
        pass

    def resize(self, w, h):
        self.w, self.h = int(w), int(h)

    def resolved(self, rays, fb, feat):
        y = np.array(fb, np.float32)
        y[..., 3] = feat[..., 3]
        return y, np.zeros_like(y)

    def upsampled(self, layer, feat_lo, f, rays, sigma, demod=False):
        H, W = f * self.h, f * self.w
        return np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W, 8), np.float32)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, scene, w, h):
        self.scene = scene
        self.denoise_moments = self.denoise_resolve = self.denoise_layers = self.denoise_filter = self.denoise_demodulate = 0
        self.denoise_reject = self.denoise_ridge = 0.0
        self.denoise_iterations, self.denoise_alpha, self.denoise_sigma = 5, 0.1, hk_denoise.DEFAULT_SIGMA
        self.tiles = False                            # a tile subset is set (kept across a resize)
        self.log = []                                 # ("op", kind) | ("drop", rule) | ("refused", kind): what the counting tests tally
        self._size(w, h)

    def _size(self, w, h):
        """everything that belongs to one frame size"""
        self.w, self.h = int(w), int(h)
        self.fb = self.var = self.feat = self.camera = None
        self.pass_kind, self.rays, self.n = "none", 0, None       # n: keeps the caller's count across a resize (new_frame says what it is)
        self.hist = None                              # dict(cam, c, rec, mom | None, layers, demod)
        self.guide_feat = None                        # the features behind the last guide
        self.guide_of_layer = False                   # ... and that guide is the layer's
        self._denoised = self._layer = self._stat = self._resolved = self._bg = self._up = None

    # -- inputs --
    def new_frame(self, fb, variance, features, pass_kind, rays, n_or_counts, camera):
        """What the path tracer and the feature passes left: fb [H][W][4]; variance [H][W][4] as vr_variance gives it, None where vr_variance is refused;
        features [H][W][8] or None before the first pass; pass_kind "none" | "stochastic" | "expected" with its rays; n: the sample count, or the per-tile
        counts of a ragged frame; camera: 13 floats (hk_temporal.camera)."""
        self.fb, self.var, self.feat, self.pass_kind, self.rays, self.camera = fb, variance, features, pass_kind, int(rays), np.array(camera, np.float32)
        self.n = int(n_or_counts) if np.ndim(n_or_counts) == 0 else np.array(n_or_counts, np.int32)

    def set_tiles(self, subset):
        self.tiles = bool(len(subset))
        self.log.append(("op", "tiles"))

    def ragged(self):
        return np.ndim(self.n) != 0

    # -- settings --
    def set(self, name, value):
        self.log.append(("op", "set"))
        if name in SWITCHES:
            assert value in (0, 1)
            if value != getattr(self, name):
                self._drop("switch:" + name)
            setattr(self, name, int(value))
        elif name == "denoise_sigma":
            self.denoise_sigma = tuple(float(x) for x in value)
        elif name == "denoise_iterations":
            self.denoise_iterations = int(value)
        else:
            assert name in ("denoise_reject", "denoise_ridge", "denoise_alpha"), name
            setattr(self, name, float(value))

    def _drop(self, rule):
        if self.hist is not None:
            self.log.append(("drop", rule))
        self.hist = None

    def _refuse(self, who, kinds):
        if kinds:
            for k in kinds:
                self.log.append(("refused", k))
            raise Refused(who, kinds)

    # -- calls --
    def _resolve_refusals(self):
        out = []
        if self.n is None or (not self.ragged() and self.n < 1):
            out.append("no_samples")
        if self.tiles:
            out.append("tiles")
        if self.feat is None or self.pass_kind != "expected":
            out.append("not_expected")
        elif self.rays < 2:
            out.append("one_ray")
        return out

    def resolve(self):
        self.log.append(("op", "resolve"))
        self._refuse("resolve", self._resolve_refusals())
        self._resolved, self._bg = self.scene.resolved(self.rays, self.fb, self.feat)

    def denoise(self):
        self._denoise("denoise", False)

    def denoise_temporal(self):
        self._denoise("denoise_temporal", True)

    def _denoise(self, who, temporal):
        self.log.append(("op", who))
        layers, regress, moments = bool(self.denoise_layers), bool(self.denoise_filter), temporal and bool(self.denoise_moments)
        demod = bool(self.denoise_demodulate)
        reject = self.denoise_reject if temporal else 0.0
        no = []
        if self.tiles:
            no.append("tiles")
        if self.feat is None:
            no.append("no_features")
        if self.n is None or (not self.ragged() and self.n < 1):
            no.append("no_samples")
        if self.var is None:
            no.append("moments_cover")
        if moments and reject > 0:
            no.append("moments_reject")
        if self.denoise_resolve or layers:
            no += [k for k in self._resolve_refusals() if k not in no]
        if regress and not layers:
            no.append("filter_layers")
        if demod and not layers:
            no.append("demod_layers")
        if self.ragged() and (self.n < 1).any():
            no.append("empty_tile")
        self._refuse(who, no)
        fb, var, feat, sigma, N = self.fb, self.var, self.feat, self.denoise_sigma, self.denoise_iterations
        kappa = np.ascontiguousarray(feat[..., 3])
        frame, B = fb, None
        if self.denoise_resolve or layers:             # vr_resolve first, whatever denoise_resolve says with layers
            y, B = self.scene.resolved(self.rays, fb, feat)
            self._resolved, self._bg = y, B
            frame = (hk_demod.split(y, B, feat) if demod else hk_layers.split(y, B, kappa)) if layers else y
        if self.ragged():
            v, g = hk_adaptive.prepare(var, feat, hk_adaptive.per_pixel(self.n, self.w, self.h))
        else:
            v, g = hk_denoise.prepare(var, feat, self.n)
        if demod:                                      # the variance of the divided layer, every pixel with its own tile's count; the guide stays prepare's
            v = hk_demod.variance(var, feat, hk_adaptive.per_pixel(self.n, self.w, self.h) if self.ragged() else self.n)
        if temporal:
            if self.hist is not None and ((self.hist["mom"] is not None) != moments or self.hist["layers"] != layers or
                                          self.hist["demod"] != demod):
                self._drop("mismatch")                # one kind of history cannot continue the other
            h = self.hist
            if moments:
                c, rec, mom = hk_moments.step(self.camera, frame, g, self.denoise_alpha, sigma, h and (h["cam"], h["c"], h["rec"], h["mom"]))
                stat = None
            elif reject > 0:
                (c, rec, stat), mom = hk_temporal.step_reject(self.camera, frame, v, g[..., 3], g[..., 7], self.denoise_alpha, reject, h and (h["cam"], h["c"], h["rec"])), None
            else:
                (c, rec), stat, mom = hk_temporal.step(self.camera, frame, v, g[..., 3], g[..., 7], self.denoise_alpha, h and (h["cam"], h["c"], h["rec"])), None, None
            self.hist = dict(cam=self.camera.copy(), c=c, rec=rec, mom=mom, layers=layers, demod=demod)
            self._stat = stat                         # T of the last denoise_temporal, or none
            frame, v = c, np.ascontiguousarray(rec[..., 0])
        if regress:
            F = hk_regress.regress(frame, g, self.denoise_ridge, sigma) if N > 0 else frame
        else:
            F = frame
            for k in range(N):
                F, v = hk_denoise.atrous(F, v, g, 1 << k, sigma)
        if layers:
            self._denoised, self._layer = hk_demod.merge(F, B, feat) if demod else hk_layers.merge(F, B, kappa)
        else:
            self._denoised = np.array(F, np.float32)
        self.guide_feat, self.guide_of_layer = feat, layers

    def denoise_history_reset(self):
        self.log.append(("op", "history_reset"))
        self._drop("history_reset")

    def upsample(self, f, rays):
        self.log.append(("op", "upsample"))
        assert 2 <= f <= 4 and 1 <= rays <= 4
        no = []
        if self._layer is None:
            no.append("no_layer")
        elif not self.guide_of_layer:
            no.append("stale_guide")
        if self.tiles:
            no.append("tiles")
        self._refuse("upsample", no)
        demod = bool(self.denoise_demodulate)          # read at the call, whatever made the layer
        if demod:
            self.log.append(("op", "upsample_demod"))
        self._up = (int(f),) + tuple(self.scene.upsampled(self._layer, self.guide_feat, int(f), int(rays), self.denoise_sigma, demod))

    def resize(self, w, h):
        self.log.append(("op", "resize"))
        self._drop("resize")
        n = self.n
        self._size(w, h)
        self.n = n if np.ndim(n) == 0 else int(np.max(n))
        self.scene.resize(w, h)

    # -- read-backs --
    def _read(self, who, value, kind):
        if value is None:
            raise Refused(who, (kind,))
        return value

    def denoised(self):
        return self._read("denoised", self._denoised, "no_denoised")

    def denoised_layer(self):
        return self._read("denoised_layer", self._layer, "no_layer")

    def denoise_history(self):
        h = self._read("denoise_history", self.hist, "no_history")
        return h["c"], np.ascontiguousarray(h["rec"][..., 0]), np.ascontiguousarray(h["rec"][..., 1])

    def denoise_history_moments(self):
        return self._read("denoise_history_moments", self.hist and self.hist["mom"], "no_history_moments")

    def denoise_reject_stat(self):
        return self._read("denoise_reject_stat", self._stat, "no_stat")

    def resolved(self):
        return self._read("resolved", self._resolved, "no_resolve")

    def resolve_background(self):
        return self._read("resolve_background", self._bg, "no_resolve")

    def upsampled_size(self):
        f = self._read("upsampled_size", self._up, "no_upsample")[0]
        return f * self.w, f * self.h

    def upsampled(self):
        return self._read("upsampled", self._up, "no_upsample")[1]

    def upsampled_layer(self):
        return self._read("upsampled_layer", self._up, "no_upsample")[2]

    def upsampled_features(self):
        return self._read("upsampled_features", self._up, "no_upsample")[3]


READERS = ("denoised", "denoised_layer", "denoise_history", "denoise_history_moments", "denoise_reject_stat", "resolved", "resolve_background", "upsampled_size",
           "upsampled", "upsampled_layer", "upsampled_features")


SHARDED_READERS = READERS[:5]                        # what volren_amd.ShardedRenderer offers


def read_all(x, error, readers=READERS):
    """every read-back of a Model or a Renderer: name -> value, or the refusal (an exception of type `error`)"""
    out = {}
    for name in readers:
        try:
            out[name] = getattr(x, name)()
        except error as e:
            out[name] = e
    return out


def same_value(a, b):
    if isinstance(a, tuple) and not isinstance(a[0], np.ndarray):
        return tuple(a) == tuple(b)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return np.shape(a) == np.shape(b) and hk_common.same(a, b)


def mismatches(got, want):
    """the read-backs of a renderer (read_all) that are not the model's: [] when every value is the model's bit for bit and every refusal says the model's words"""
    bad = []
    for name in got:
        g, w = got[name], want[name]
        if isinstance(w, Refused):
            if not (isinstance(g, Exception) and w.matches(str(g))):
                bad.append((name, "the model refuses: %s" % w, "got a value" if not isinstance(g, Exception) else str(g)))
        elif isinstance(g, Exception):
            bad.append((name, "the model has a value", str(g)))
        elif not same_value(g, w):
            bad.append((name, "values differ"))
    return bad


def unchanged(before, after):
    """two read_all() of one object: every value bit for bit what it was, every refusal still a refusal"""
    return [n for n in before if isinstance(before[n], Exception) != isinstance(after[n], Exception) or
            (not isinstance(before[n], Exception) and not same_value(before[n], after[n]))]


# ---- the all-pairs array -------------------------------------------------------------------------------------------------------------------------------------
FACTORS = (("call", ("denoise", "denoise_temporal")), ("moments", (0, 1)), ("reject", (0.0, 3.0)), ("resolve", (0, 1)), ("layers", (0, 1)), ("filter", (0, 1)),
           ("demodulate", (0, 1)), ("ridge", (0.0, 1.0)), ("iterations", (0, 1, 2, 3, 5)), ("frame", ("uniform", "ragged")), ("features", ("stochastic", "expected")),
           ("camera", ("fixed", "orbit")), ("shape", ((33, 31), (17, 16), (1, 37))))
NAMES = tuple(n for n, _ in FACTORS)
# what the product refuses: each a set of (factor, value) that no accepted row holds together
FORBIDDEN = ((("filter", 1), ("layers", 0)), (("layers", 1), ("features", "stochastic")), (("resolve", 1), ("features", "stochastic")),
             (("call", "denoise_temporal"), ("moments", 1), ("reject", 3.0)), (("demodulate", 1), ("layers", 0)))
FORBIDDEN_KINDS = ("filter_layers", "not_expected", "not_expected", "moments_reject", "demod_layers")


def row_dict(row):
    return dict(zip(NAMES, row))


def violated(row):
    """the indices of FORBIDDEN the row holds"""
    d = row_dict(row)
    return [i for i, combo in enumerate(FORBIDDEN) if all(d[f] == v for f, v in combo)]


def all_pairs(rows=None):
    """every ((factor, value), (factor, value)) of two different factors, in the factors' order -- of `rows`, or of the whole product"""
    if rows is not None:
        return {(a, b) for r in rows for a, b in itertools.combinations(tuple(zip(NAMES, r)), 2)}
    return {((f, v), (g, u)) for (f, vs), (g, us) in itertools.combinations(FACTORS, 2) for v in vs for u in us}


def covering_array():
    """-> (accepted rows, refusal rows), tuples in FACTORS' order.  Greedy and deterministic: of all rows the product accepts, the first in the product's order
    that holds the most pairs no chosen row holds yet, until none adds one; then, per pair no accepted row can hold and per entry of FORBIDDEN, the first row
    of the product that holds it and no other entry of FORBIDDEN (or, where the pair implies another entry, the fewest)."""
    product = list(itertools.product(*[vs for _, vs in FACTORS]))
    nv = [len(vs) for _, vs in FACTORS]
    idx = np.array(list(itertools.product(*[range(n) for n in nv])), np.int64)
    pairs = list(itertools.combinations(range(len(FACTORS)), 2))
    offset, total = [], 0
    for i, j in pairs:
        offset.append(total)
        total += nv[i] * nv[j]
    ids = np.stack([off + idx[:, i] * nv[j] + idx[:, j] for off, (i, j) in zip(offset, pairs)], axis=1)
    ok = np.array([not violated(r) for r in product])
    open_ = np.zeros(total, bool)
    open_[np.unique(ids[ok])] = True                   # the pairs some accepted row holds
    allowed = open_.copy()
    accepted = []
    while open_.any():
        gain = np.where(ok, open_[ids].sum(axis=1), -1)
        best = int(np.argmax(gain))
        accepted.append(product[best])
        open_[ids[best]] = False
    refusals = []
    n_bad = np.array([len(violated(r)) for r in product])
    wanted = [np.flatnonzero(~allowed)[k:k + 1] for k in range(int((~allowed).sum()))]
    for target in wanted:                              # the pairs no accepted row can hold
        if any((ids[product.index(r)] == target[0]).any() for r in refusals):
            continue
        has = (ids == target[0]).any(axis=1)
        best = int(np.flatnonzero(has)[np.argmin(n_bad[has])])
        refusals.append(product[best])
    for i in range(len(FORBIDDEN)):                    # and every entry itself (the triple is no pair)
        if not any(i in violated(r) for r in refusals):
            refusals.append(next(r for r in product if violated(r) == [i]))
    return accepted, refusals


PIVOT = dict(call="denoise_temporal", moments=0, reject=3.0, resolve=1, layers=1, filter=0, demodulate=0, ridge=0.0, iterations=3, frame="uniform", features="expected",
             camera="orbit", shape=(33, 31))


def factor_pairs():
    """Per factor two accepted rows that differ in that factor alone, at a pivot where the factor is live: everything on, and per factor what it needs --
    no rejection next to the moments, the regression next to the ridge, no layers next to the resolve, no resolve and no layers next to a stochastic pass, iterations 2 against 3."""
    return _pairs_at(PIVOT, NAMES)


DEMODULATED = ("call", "moments", "reject", "filter", "ridge", "iterations", "frame", "camera", "shape")


def factor_pairs_demodulated():
    """The same at the pivot with "demodulate" 1, for every factor that stays accepted there with layers 1 (the resolve runs whatever its switch says, a
    stochastic pass and no layers are refused): the history, the rejection, the moments, the regression and the counts of a ragged frame on the divided layer."""
    return _pairs_at(dict(PIVOT, demodulate=1), DEMODULATED)


def _pairs_at(pivot, names):
    out = {}
    for name, values in FACTORS:
        if name not in names:
            continue
        base = dict(pivot)
        a, b = values[0], values[1]
        if name == "moments":
            base["reject"] = 0.0
        if name == "ridge":
            base["filter"] = 1
        if name == "resolve":
            base["layers"] = 0                         # with layers the resolve runs whatever denoise_resolve says
        if name == "features":
            base["resolve"] = base["layers"] = 0
        if name == "iterations":
            a, b = 2, 3
        rows = tuple(tuple(dict(base, **{name: v})[n] for n in NAMES) for v in (a, b))
        assert not violated(rows[0]) and not violated(rows[1]), name
        out[name] = rows
    return out


# ---- random call sequences -----------------------------------------------------------------------------------------------------------------------------------
SEEDS = (41, 42, 43, 44, 45, 59, 149, 156, 175, 351)             # replaced until test_pipeline_model_host.py counted every kind twice
LENGTH = 25
SIZES = ((33, 31), (17, 16))
OP_KINDS = ("set", "frame", "features", "denoise", "denoise_temporal", "history_reset", "resolve", "upsample", "upsample_demod", "resize", "tiles")
# (upsample_demod: an upsample that ran with "denoise_demodulate" = 1 at its call, logged besides "upsample")


REPAIRS = {"tiles": ("tiles", ()), "no_features": ("features", "expected", 2), "not_expected": ("features", "expected", 2), "one_ray": ("features", "expected", 2),
           "no_samples": ("frame", "uniform"), "moments_cover": ("frame", "uniform"), "empty_tile": ("frame", "uniform"), "moments_reject": ("set", "denoise_reject", 0.0),
           "filter_layers": ("set", "denoise_layers", 1), "demod_layers": ("set", "denoise_layers", 1), "no_layer": ("set", "denoise_layers", 1), "stale_guide": ("denoise",)}


def sequence(seed, length=LENGTH):
    """About `length` operations drawn by numpy's Mersenne twister of `seed`; every one is a call the header defines.  Drawn one by one and blindly, most calls
    would be refused for the same two reasons and few histories would live long enough to be dropped.  So the draw is of short motifs -- one blind operation; a
    run of temporal frames; a switch flipped between two temporal calls; a reset; a resize; a temporal call without rejection after one with it; a layer upsampled under the other
    value of "denoise_demodulate" than the one that made it; each refusal's own preparation -- whose parameters, order and
    neighbours are random, and it runs a Model over a StubTracer alongside: `call` answers a refusal with the call that lifts its first reason and tries again,
    so that the refusal, the repair and the accepted call all stand in the sequence.  A motif that has begun is finished, repairs included: a sequence has length .. length + 10
    operations."""
    rs = np.random.RandomState(seed)
    sim, tracer = Model(BlankScene(*SIZES[0]), *SIZES[0]), StubTracer(*SIZES[0])
    ops, size = [], [0]
    pick = lambda xs: xs[rs.randint(len(xs))]         # noqa: E731

    def emit(op):
        if op[0] == "frame" and len(op) == 2:
            op = ("frame", op[1], 1000 * seed + len(ops), float(rs.randint(0, 4)))
        ops.append(op)
        return apply(sim, op, tracer)

    def call(op):
        for _ in range(4):
            refusal = emit(op)
            if refusal is None:
                return
            emit(REPAIRS[refusal.kinds[0]])

    def blind():
        u = rs.uniform()
        if u < 0.30:
            name = pick(SWITCHES + ("denoise_reject", "denoise_ridge", "denoise_alpha", "denoise_iterations", "denoise_sigma"))
            value = {"denoise_reject": (0.0, 3.0), "denoise_ridge": (0.0, 1.0), "denoise_alpha": (0.1, 0.5), "denoise_iterations": (0, 1, 2, 3, 5),
                     "denoise_sigma": (hk_denoise.DEFAULT_SIGMA, SIGMA2)}.get(name, (0, 1))
            emit(("set", name, pick(value)))
        elif u < 0.45:
            emit(("frame", pick(("uniform", "adaptive"))))
        elif u < 0.55:
            emit(pick((("features", "stochastic", 2), ("features", "expected", 1), ("features", "expected", 2))))
        else:
            emit(pick((("denoise",), ("denoise_temporal",), ("denoise_temporal",), ("history_reset",), ("resolve",), ("upsample", 2, 2), ("upsample", 3, 2))))

    def temporal_run():
        for _ in range(2):
            emit(("frame", pick(("uniform", "uniform", "adaptive"))))
            emit(("features", "expected", 2))
            call(("denoise_temporal",))

    def flip():
        name = pick(SWITCHES)
        call(("denoise_temporal",))
        emit(("set", name, 1 - getattr(sim, name)))
        call(("denoise_temporal",))

    def reset():
        call(("denoise_temporal",))
        emit(("history_reset",))
        emit(("denoise_temporal",))

    def resize():
        call(("denoise_temporal",))
        size[0] = 1 - size[0]
        emit(("resize",) + SIZES[size[0]])
        emit(pick((("denoise",), ("frame", "uniform"), ("upsample", 2, 2))))

    def moments_reject():
        emit(("set", "denoise_moments", 1))
        emit(("set", "denoise_reject", 3.0))
        call(("denoise_temporal",))

    def statistic_goes():
        emit(("set", "denoise_reject", 3.0))
        call(("denoise_temporal",))
        emit(pick((("denoise",), ("history_reset",), ("set", "denoise_alpha", 0.5))))
        emit(("set", "denoise_reject", 0.0))
        call(("denoise_temporal",))

    def one_ray():
        emit(("features", "expected", 1))
        emit(("set", pick(("denoise_layers", "denoise_resolve")), 1))
        call(pick((("denoise",), ("resolve",))))

    def empty_tile():
        emit(("tiles", (0, 1)))
        emit(("frame", "adaptive"))
        emit(("tiles", ()))
        call(("denoise",))

    def stale_guide():
        emit(("set", "denoise_layers", 1))
        call(("denoise",))
        emit(("upsample", pick((2, 3)), 2))
        emit(("set", "denoise_filter", 0))
        emit(("set", "denoise_layers", 0))
        call(pick((("denoise",), ("denoise_temporal",))))
        emit(("upsample", 2, 2))

    def filter_layers():
        emit(("set", "denoise_filter", 1))
        emit(("set", "denoise_layers", pick((0, 0, 1))))
        call(("denoise",))

    def demod_layers():
        emit(("set", "denoise_demodulate", 1))
        emit(("set", "denoise_layers", pick((0, 0, 1))))
        call(("denoise",))

    def demod_upsample():
        made_with = pick((0, 1))                      # the layer made under one value of the setting, upsampled under the other: the call's value counts
        emit(("set", "denoise_layers", 1))
        emit(("set", "denoise_demodulate", made_with))
        call(pick((("denoise",), ("denoise_temporal",))))
        emit(("set", "denoise_demodulate", 1 - made_with))
        emit(("upsample", pick((2, 3)), 2))

    def tiles():
        emit(("tiles", (0, 1)))
        emit(pick((("denoise",), ("resolve",), ("upsample", 2, 2), ("frame", "uniform"))))
        emit(("tiles", ()))

    def stochastic():
        emit(("features", "stochastic", 2))
        emit(pick((("denoise",), ("denoise_temporal",), ("resolve",))))

    motifs = (blind, blind, blind, blind, temporal_run, flip, flip, reset, resize, moments_reject, statistic_goes, one_ray, empty_tile, stale_guide, filter_layers, demod_layers,
              demod_upsample, tiles, stochastic)
    while len(ops) < length:
        pick(motifs)()
    return ops


class StubTracer:
    """The path tracer's side of a sequence without a device, for the runs that count: blank frames of the counts the calls would leave.  A uniform frame has
    3 samples; an adaptive one 2 and 4 by turns over the tiles it renders and 0 over the others; a resize leaves the count and no moments, no features."""

    def __init__(self, w, h):
        self.tiles, self.n = (), 0
        self._size(w, h)

    def _size(self, w, h):
        self.w, self.h, self.var, self.feat, self.pass_kind, self.rays = w, h, None, None, "none", 0
        self.n = self.n if np.ndim(self.n) == 0 else int(np.max(self.n))

    def apply(self, op):
        if op[0] == "frame":
            if op[1] == "uniform":
                self.n = 3
            else:
                ty, tx = hk_adaptive.tiles_of(self.w, self.h)
                live = self.tiles or range(ty * tx)
                self.n = np.array([(2, 4)[t & 1] if t in live else 0 for t in range(ty * tx)], np.int32)
            self.var = np.zeros((self.h, self.w, 4), np.float32)
        elif op[0] == "features":
            self.feat, self.pass_kind, self.rays = np.zeros((self.h, self.w, 8), np.float32), op[1], op[2]
        elif op[0] == "resize":
            self._size(op[1], op[2])
        elif op[0] == "tiles":
            self.tiles = tuple(op[1])

    def inputs(self):
        cam = hk_temporal.camera((1, 0, 1), np.eye(3).reshape(9), z=-1.0)
        return np.zeros((self.h, self.w, 4), np.float32), self.var, self.feat, self.pass_kind, self.rays, self.n, cam


def apply(m, op, tracer):
    """One operation of a sequence on the model: the image-space calls on the model itself, the others on `tracer` (apply(op), then inputs() -> new_frame's
    arguments).  -> None, or the Refused the call raised."""
    kind = op[0]
    try:
        if kind == "set":
            m.set(op[1], op[2])
        elif kind in ("denoise", "denoise_temporal", "resolve"):
            getattr(m, kind)()
        elif kind == "history_reset":
            m.denoise_history_reset()
        elif kind == "upsample":
            m.upsample(op[1], op[2])
        else:
            if kind == "resize":
                m.resize(op[1], op[2])
            elif kind == "tiles":
                m.set_tiles(op[1])
            else:
                m.log.append(("op", kind))
            tracer.apply(op)
            m.new_frame(*tracer.inputs())
    except Refused as e:
        return e
    return None


def tally(logs):
    """{("op" | "drop" | "refused", kind): how often} over the models' logs"""
    out = {}
    for log in logs:
        for entry in log:
            out[entry] = out.get(entry, 0) + 1
    return out
