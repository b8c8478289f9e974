"""GPU: RendererHIP::run_denoise and the calls around it (renderer.cpp: which kernel runs on which buffer, what survives from one call to the next, what a
refusal leaves behind) against one host model of that state (tests/hk_pipeline.py, itself held to the existing replays by tests/test_pipeline_model_host.py):
(a) an all-pairs array over the denoiser's settings, frames, feature passes, cameras and shapes, three frames per row, every read-back after every frame bit for
bit, and a refusal row per combination the product refuses; (b) committed random call sequences, every read-back or the refusal after every operation; (c) the
rule of include/volren_amd.h on vr_upsample after a denoise call without layers, and its rule that vr_upsample reads "denoise_demodulate" at the call; (d) the rows and one sequence a ShardedRenderer of three logical parts can
express.  The kernels themselves are tests/test_gpu_filter_probe.py's subject; nothing here has a tolerance."""
import functools

import numpy as np
import pytest

import hk_pipeline as hp
import volren_amd
from gpu_frames import _camera, _orbit
from hk_common import same as _same
from test_gpu_resolve import _configure
from volren_amd import VolrenError

pytestmark = pytest.mark.gpu

NAME, SPP, RAYS = "c3env", 3, 2
ACCEPTED, REFUSED = hp.covering_array()
SETTINGS = (("denoise_moments", "moments"), ("denoise_reject", "reject"), ("denoise_resolve", "resolve"), ("denoise_layers", "layers"), ("denoise_filter", "filter"),
            ("denoise_demodulate", "demodulate"), ("denoise_ridge", "ridge"), ("denoise_iterations", "iterations"))


def _id(row):
    return "-".join("x".join(str(c) for c in v) if isinstance(v, tuple) else str(v) for v in row)


def _renderer(w, h):
    r = _configure(volren_amd.Renderer(w, h), NAME, False)
    r.variance = 1
    return r


def _inputs(r, pass_kind, rays, fb=None):
    """new_frame's arguments from the renderer's own read-backs"""
    def or_none(read):
        try:
            return read()
        except VolrenError:
            return None
    counts = r.tile_samples()
    n = int(counts.flat[0]) if (counts == counts.flat[0]).all() else counts
    return (r.framebuffer() if fb is None else fb), or_none(r.variance), or_none(r.features), pass_kind, rays, n, _camera(r)


def _split_threshold(r):
    """a threshold between the tiles' errors at 2 spp, so that render_adaptive leaves some tiles at 2 samples and takes the others further"""
    e = np.unique(r.tile_error())
    e = e[np.isfinite(e)]
    assert len(e) >= 2, e
    return float(0.5 * (e[len(e) // 2 - 1] + e[len(e) // 2]))


def _render(x, d, i, scene, parts=None):
    """frame i of a row on a Renderer or a ShardedRenderer; -> (pass kind, rays)"""
    for p in parts or (x,):
        if d["camera"] == "orbit":
            _orbit(p, 1.0 * i)
        p.seed = 100 + i
    if d["camera"] == "orbit":
        scene.orbit(1.0 * i)
    x.reset()
    if d["frame"] == "uniform":
        x.render(SPP)
    else:
        x.render(2)
        x.render_adaptive(2, 8, _split_threshold(x))
        assert len(np.unique(x.tile_samples())) >= 2
    if d["features"] == "stochastic":
        x.render_features(2)
        return "stochastic", 0
    x.render_features_expected(RAYS)
    return "expected", RAYS


def _compare(r, m, what, readers=hp.READERS):
    bad = hp.mismatches(hp.read_all(r, VolrenError, readers), hp.read_all(m, hp.Refused, readers))
    assert not bad, (what, bad)


@functools.lru_cache(maxsize=None)
def _run_row(row):
    """three frames of an accepted row, every read-back against the model after each; -> the read-backs after the last frame"""
    d = hp.row_dict(row)
    w, h = d["shape"]
    r, scene = _renderer(w, h), hp.OracleScene(NAME, w, h)
    m = hp.Model(scene, w, h)
    for field, factor in SETTINGS:
        setattr(r, field, d[factor])
        m.set(field, d[factor])
    for i in range(3):
        kind, rays = _render(r, d, i, scene)
        m.new_frame(*_inputs(r, kind, rays))
        getattr(r, d["call"])()
        getattr(m, d["call"])()
        _compare(r, m, (row, i))
    out = hp.read_all(m, hp.Refused)
    r.close()
    return out


# ---- a: the all-pairs array ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ACCEPTED, ids=_id)
def test_every_read_back_of_an_accepted_row_is_the_models(row):
    out = _run_row(row)
    assert not isinstance(out["denoised"], Exception) and np.isfinite(out["denoised"]).all()


@pytest.mark.parametrize("row", REFUSED, ids=_id)
def test_a_refused_row_says_why_and_leaves_every_read_back(row):
    """on a renderer whose every read-back but the moment records holds a value: a temporal frame with layers and rejection, upsampled"""
    d = hp.row_dict(row)
    w, h = d["shape"]
    r, scene = _renderer(w, h), hp.OracleScene(NAME, w, h)
    m = hp.Model(scene, w, h)
    for field, v in (("denoise_layers", 1), ("denoise_reject", 3.0)):
        setattr(r, field, v)
        m.set(field, v)
    kind, rays = _render(r, dict(d, features="expected"), 0, scene)
    m.new_frame(*_inputs(r, kind, rays))
    for x in (r, m):
        x.denoise_temporal()
        x.upsample(2, RAYS)
    for field, factor in SETTINGS:
        setattr(r, field, d[factor])
        m.set(field, d[factor])
    kind, rays = _render(r, d, 1, scene)
    m.new_frame(*_inputs(r, kind, rays))
    _compare(r, m, (row, "before"))
    before = hp.read_all(r, VolrenError)
    assert sum(isinstance(v, Exception) for v in before.values()) <= 4       # (the settings dropped the history: its three read-backs, and the moments)
    with pytest.raises(hp.Refused) as want:
        getattr(m, d["call"])()
    assert set(hp.FORBIDDEN_KINDS[i] for i in hp.violated(row)) <= set(want.value.kinds)
    with pytest.raises(VolrenError) as got:
        getattr(r, d["call"])()
    assert want.value.matches(str(got.value)), (str(got.value), want.value.words)
    assert hp.unchanged(before, hp.read_all(r, VolrenError)) == []
    _compare(r, m, (row, "after"))
    r.close()


@pytest.mark.parametrize("factor", hp.NAMES + tuple("demodulated-" + n for n in hp.DEMODULATED))
def test_every_factor_changes_the_result(factor):
    """two accepted rows that differ in the factor alone (hk_pipeline.factor_pairs: iterations 2 against 3): some read-back differs.  demodulated-*: the same
    at the pivot with "denoise_demodulate" = 1 (hk_pipeline.factor_pairs_demodulated)"""
    pairs = hp.factor_pairs()
    if factor.startswith("demodulated-"):
        factor, pairs = factor[len("demodulated-"):], hp.factor_pairs_demodulated()
    a, b = (_run_row(row) for row in pairs[factor])
    differ = [n for n in hp.READERS if isinstance(a[n], Exception) != isinstance(b[n], Exception) or
              (not isinstance(a[n], Exception) and not hp.same_value(a[n], b[n]))]
    print(factor, differ)
    assert "denoised" in differ if factor != "reject" else ("denoise_history" in differ and "denoise_reject_stat" in differ)


# ---- b: random call sequences --------------------------------------------------------------------------------------------------------------------------------------
class _Tracer:
    """the path tracer's side of a sequence on the product (hk_pipeline.StubTracer's counterpart)"""

    def __init__(self, r, scene, parts=None):
        self.r, self.scene, self.parts, self.pass_kind, self.rays = r, scene, parts, "none", 0

    def apply(self, op):
        r = self.r
        if op[0] == "frame":
            for p in self.parts or (r,):
                _orbit(p, op[3])
                p.seed = op[2]
            self.scene.orbit(op[3])
            r.reset()
            if op[1] == "uniform":
                r.render(SPP)
            else:
                r.render_adaptive(2, 8, 0.3)
        elif op[0] == "features":
            self.pass_kind, self.rays = op[1], (op[2] if op[1] == "expected" else 0)
            r.render_features(op[2]) if op[1] == "stochastic" else r.render_features_expected(op[2])
        elif op[0] == "resize":
            r.resize(op[1], op[2])
            self.pass_kind, self.rays = "none", 0
        elif op[0] == "tiles":
            r.set_tiles(list(op[1]))

    def inputs(self):
        return _inputs(self.r, self.pass_kind, self.rays)


def _on_product(r, op, upsampler=None):
    """an image-space operation on the renderer: -> None, or the VolrenError"""
    try:
        if op[0] == "set":
            setattr(r, op[1], op[2])
        elif op[0] == "history_reset":
            r.denoise_history_reset()
        elif op[0] == "upsample":
            (upsampler or r).upsample(op[1], op[2])
        else:
            getattr(r, op[0])()
    except VolrenError as e:
        return e
    return None


IMAGE_OPS = ("set", "denoise", "denoise_temporal", "history_reset", "resolve", "upsample")


def _run_sequence(ops, r, m, tracer, what, readers=hp.READERS, upsampler=None, reader=None):
    for k, op in enumerate(ops):
        before = hp.read_all(reader or r, VolrenError, readers)
        want = hp.apply(m, op, tracer)
        if op[0] in IMAGE_OPS:
            got = _on_product(r, op, upsampler)
            assert (got is None) == (want is None), (what, k, op, str(got), str(want))
            if want is not None:
                assert want.matches(str(got)), (what, k, op, str(got), want.words)
                assert hp.unchanged(before, hp.read_all(reader or r, VolrenError, readers)) == [], (what, k, op)
        _compare(reader or r, m, (what, k, op), readers)


@pytest.mark.parametrize("seed", hp.SEEDS)
def test_a_random_call_sequence_is_the_models_after_every_operation(seed):
    w, h = hp.SIZES[0]
    r, scene = _renderer(w, h), hp.OracleScene(NAME, w, h)
    m = hp.Model(scene, w, h)
    _run_sequence(hp.sequence(seed), r, m, _Tracer(r, scene), seed)
    count = hp.tally([m.log])
    print("seed %d: %s" % (seed, ", ".join("%s %s %d" % (k + (v,)) for k, v in sorted(count.items()) if k[0] != "op")))
    r.close()


# ---- c: the suspect -------------------------------------------------------------------------------------------------------------------------------------------------
def test_upsample_is_refused_once_a_denoise_without_layers_has_replaced_the_guide():
    """denoise_layers = 1, denoise, denoise_layers = 0, render_features(spp), denoise, upsample(2, 2): the layer is the first call's and the guide would be the
    second's, from another feature pass.  include/volren_amd.h: refused with words of its own; vr_denoised_layer and vr_upsampled* keep what they held; a refused
    denoise call in between changes nothing of this; a denoise call with layers makes the call available again, and it is the host chain's."""
    w, h = hp.SIZES[0]
    r, scene = _renderer(w, h), hp.OracleScene(NAME, w, h)
    m = hp.Model(scene, w, h)
    tracer = _Tracer(r, scene)
    ops = [("frame", "uniform", 7, 0.0), ("features", "expected", 2), ("set", "denoise_layers", 1), ("denoise",), ("upsample", 2, 2)]
    _run_sequence(ops, r, m, tracer, "with layers")
    layer, up, guide = r.denoised_layer(), r.upsampled(), r.features()
    _run_sequence([("set", "denoise_layers", 0), ("features", "stochastic", SPP), ("denoise",)], r, m, tracer, "without layers")
    assert not _same(r.features(), guide)
    with pytest.raises(VolrenError, match="the last denoise ran with denoise_layers = 0"):
        r.upsample(2, 2)
    assert _same(r.denoised_layer(), layer) and _same(r.upsampled(), up)
    _run_sequence([("upsample", 2, 2), ("set", "denoise_layers", 1), ("upsample", 3, 2), ("denoise",), ("upsample", 2, 2)], r, m, tracer, "refused")
    assert hp.tally([m.log])[("refused", "stale_guide")] == 3 and hp.tally([m.log])[("refused", "not_expected")] == 1
    assert _same(r.denoised_layer(), layer) and _same(r.upsampled(), up)
    _run_sequence([("features", "expected", 2), ("denoise",), ("upsample", 2, 2)], r, m, tracer, "again")
    assert _same(r.upsampled(), up)                           # (the same frame, the same guide: the same picture)
    r.close()


def test_upsample_reads_denoise_demodulate_at_its_call_and_a_flip_between_two_temporal_calls_drops_the_history():
    """include/volren_amd.h, "Albedo demodulation": a layer made with the setting 0, upsampled with it at 1 (the lo layer is divided inside the call) and at 0
    again (the plain call's picture: the first upsample's, had it run); then two temporal calls with the setting flipped in between -- the second starts a
    history of its own -- and two more under the new value, which continue it.  Every read-back against the model after every operation."""
    w, h = hp.SIZES[0]
    r, scene = _renderer(w, h), hp.OracleScene(NAME, w, h)
    m = hp.Model(scene, w, h)
    tracer = _Tracer(r, scene)
    _run_sequence([("frame", "uniform", 7, 0.0), ("features", "expected", 2), ("set", "denoise_layers", 1), ("set", "denoise_demodulate", 0), ("denoise",),
                   ("upsample", 2, 2)], r, m, tracer, "made without")
    plain, layer = r.upsampled(), r.denoised_layer()
    _run_sequence([("set", "denoise_demodulate", 1), ("upsample", 2, 2)], r, m, tracer, "upsampled with")
    assert not _same(r.upsampled(), plain) and _same(r.denoised_layer(), layer)
    _run_sequence([("set", "denoise_demodulate", 0), ("upsample", 2, 2)], r, m, tracer, "upsampled without")
    assert _same(r.upsampled(), plain)
    _run_sequence([("denoise_temporal",), ("frame", "uniform", 8, 1.0), ("features", "expected", 2), ("denoise_temporal",)], r, m, tracer, "temporal without")
    assert (r.denoise_history()[2] == 2).sum() > 50
    _run_sequence([("set", "denoise_demodulate", 1), ("frame", "uniform", 9, 2.0), ("features", "expected", 2), ("denoise_temporal",)], r, m, tracer, "flipped")
    assert (r.denoise_history()[2] == 1).all()                # a history of its own
    _run_sequence([("frame", "uniform", 10, 3.0), ("features", "expected", 2), ("denoise_temporal",), ("upsample", 2, 2)], r, m, tracer, "temporal with")
    assert (r.denoise_history()[2] == 2).sum() > 50
    count = hp.tally([m.log])
    assert count[("drop", "switch:denoise_demodulate")] == 1 and count[("op", "upsample_demod")] == 2 and not any(k[0] == "refused" for k in count)
    r.close()


def test_the_statistic_is_the_last_temporal_calls():
    """vr_denoise_reject_stat after unrelated later calls: kept across vr_denoise, a history reset and a change of a switch, the next temporal call's own after
    one with rejection, and refused after a temporal call without"""
    w, h = hp.SIZES[0]
    r, scene = _renderer(w, h), hp.OracleScene(NAME, w, h)
    m = hp.Model(scene, w, h)
    ops = [("frame", "uniform", 7, 0.0), ("features", "expected", 2), ("set", "denoise_reject", 3.0), ("denoise_temporal",), ("frame", "uniform", 8, 1.0),
           ("features", "expected", 2), ("denoise_temporal",)]
    _run_sequence(ops, r, m, _Tracer(r, scene), "with rejection")
    stat = r.denoise_reject_stat()
    assert (stat >= 0).mean() > 0.5
    _run_sequence([("denoise",), ("history_reset",), ("set", "denoise_layers", 1), ("denoise",), ("upsample", 2, 2)], r, m, _Tracer(r, scene, ), "unrelated")
    assert _same(r.denoise_reject_stat(), stat)
    tracer = _Tracer(r, scene)
    tracer.pass_kind, tracer.rays = "expected", 2
    _run_sequence([("denoise_temporal",)], r, m, tracer, "afresh")
    assert (r.denoise_reject_stat() == -1).all()
    _run_sequence([("set", "denoise_reject", 0.0), ("denoise_temporal",)], r, m, tracer, "without")
    with pytest.raises(VolrenError, match="did not run with denoise_reject > 0"):
        r.denoise_reject_stat()
    r.close()


# ---- d: sharded ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _sharded(w, h):
    s = volren_amd.ShardedRenderer(w, h, [0, 0, 0])

    def configure(p):
        _configure(p, NAME, False)
        p.variance = 1
    s.each(configure)
    return s


class _ShardedFace:
    """a ShardedRenderer behind the names a sequence uses: settings on every part, the calls and read-backs the sharded object offers, upsample on part 0"""

    def __init__(self, s):
        object.__setattr__(self, "s", s)

    def __setattr__(self, name, value):
        for p in self.s.parts:
            setattr(p, name, value)

    def __getattr__(self, name):
        return getattr(self.s, name)

    def tile_samples(self):
        return self.s.parts[0].tile_samples()


def _sharded_inputs(s, kind, rays):
    n = int(s.parts[0].tile_samples().flat[0])
    return s.framebuffer(), s.variance(), s.features(), kind, rays, n, _camera(s.parts[0])


SHARDED_ROWS = [row for row in ACCEPTED if hp.row_dict(row)["frame"] == "uniform"]
SHARDED_ROWS += [row for row in hp.factor_pairs_demodulated()["moments"] if row not in SHARDED_ROWS]      # the divided layer's history, plain and under the moments


@pytest.mark.parametrize("row", SHARDED_ROWS, ids=_id)
def test_three_logical_parts_give_the_single_device_models_rows(row):
    d = hp.row_dict(row)
    w, h = d["shape"]
    s, scene = _sharded(w, h), hp.OracleScene(NAME, w, h)
    face, m = _ShardedFace(s), hp.Model(scene, w, h)
    for field, factor in SETTINGS:
        setattr(face, field, d[factor])
        m.set(field, d[factor])
    for i in range(3):
        kind, rays = _render(s, d, i, scene, parts=s.parts)
        if i == 1:
            s.gather_guides()                          # (a gather of the caller's own in front of the call's changes nothing)
        m.new_frame(*_sharded_inputs(s, kind, rays))
        getattr(s, d["call"])()
        getattr(m, d["call"])()
        _compare(s, m, (row, i), hp.SHARDED_READERS)
    if d["layers"]:
        s.parts[0].upsample(2, RAYS)                   # vr_upsample is on vr_sharded_part(s, 0)
        m.upsample(2, RAYS)
        _compare(s.parts[0], m, (row, "upsample"))
    s.close()


class _ShardedTracer(_Tracer):
    def inputs(self):
        try:
            return _sharded_inputs(self.r, self.pass_kind, self.rays)
        except VolrenError:                            # nothing to gather yet: what the parts hold is not the model's to see
            n = int(self.r.parts[0].tile_samples().flat[0])
            return self.r.framebuffer(), None, None, self.pass_kind, self.rays, n, _camera(self.r.parts[0])


def test_a_random_call_sequence_on_three_logical_parts():
    """the first seed's sequence restricted to what the sharded object expresses: settings, uniform frames, the feature passes, denoise, denoise_temporal, the
    history reset, and upsample on part 0"""
    w, h = hp.SIZES[0]
    ops = [("frame", "uniform") + op[2:] if op[0] == "frame" else op for op in hp.sequence(hp.SEEDS[0]) if op[0] not in ("resize", "tiles", "resolve")]
    s, scene = _sharded(w, h), hp.OracleScene(NAME, w, h)
    face, m = _ShardedFace(s), hp.Model(scene, w, h)
    _run_sequence(ops, face, m, _ShardedTracer(s, scene, parts=s.parts), "sharded", hp.SHARDED_READERS, upsampler=s.parts[0], reader=s)
    s.close()
