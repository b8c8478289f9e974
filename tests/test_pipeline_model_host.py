"""CPU: the host model of the renderer's image-space state (tests/hk_pipeline.py) held to what exists, before tests/test_gpu_pipeline.py lets it judge the
product: with one switch on at a time its three-frame sequences are the existing replays' (hk_temporal.Replay, hk_moments.Replay, hk_layers.Replay and layered,
hk_regress.Replay, hk_resolve.resolved, hk_upsample.chain; with "denoise_demodulate" on top of the layers hk_demod.layered, Replay and chain) bit for bit; the all-pairs array holds every pair the product accepts and every combination it
refuses; and the committed seeds' call sequences fire every kind of operation, every rule that drops the history and every refusal at least twice.  The counts
are printed.  No device is touched.

The frames are test_denoise_host.oracle_inputs' (the oracle's per-sample radiances replayed through the accumulation pass's arithmetic, the host feature pass)
with a seed and a camera per frame, plus the host build of the expected-value pass: c2 and c3env at 33x31, 4 spp, the camera turned 1 degree per frame."""
import numpy as np
import pytest

import hk_adaptive
import hk_demod
import hk_denoise
import hk_expected
import hk_features
import hk_layers
import hk_moments
import hk_pipeline as hp
import hk_regress
import hk_resolve
import hk_temporal
import hk_upsample
import test_resolve_host as trh
from hk_common import same as _same

W, H, SPP, RAYS, FRAMES = 33, 31, 4, 2, 3
SCENES = ("c2", "c3env")
_CACHE = {}


def _frames(name):
    """[(fb, variance, stochastic features, expected features, camera)] of the three frames, and the scene (left under the last frame's camera)"""
    if name not in _CACHE:
        from test_gpu_features import _replay
        scene, frames = hp.OracleScene(name, W, H), []
        for i in range(FRAMES):
            scene.orbit(1.0 * i)
            o = scene.lo()
            o.seed = 100 + i
            mu, S = _replay(trh._radiance(o, SPP))
            var = (S * (np.float32(SPP) / np.float32(SPP - 1))).astype(np.float32)
            frames.append((mu, var, hk_features.feature_pass(o, SPP), hk_expected.expected_pass(o, RAYS), scene.camera()))
        _CACHE[name] = (scene, frames)
    return _CACHE[name]


def _model(name, **settings):
    scene, frames = _frames(name)
    m = hp.Model(scene, W, H)
    for k, v in settings.items():
        m.set(k, v)
    return m, scene, frames


def _feed(m, scene, frames, i, expected):
    fb, var, fs, fe, cam = frames[i]
    scene.orbit(1.0 * i)
    m.new_frame(fb, var, fe if expected else fs, "expected" if expected else "stochastic", RAYS if expected else 0, SPP, cam)
    return fb, var, (fe if expected else fs), cam


# ---- one switch at a time: the model is the existing replay ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tau", (0.0, 3.0))
def test_temporal_is_the_temporal_replay(name, tau):
    m, scene, frames = _model(name, denoise_reject=tau)
    replay = hk_temporal.Replay()
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, False)
        m.denoise_temporal()
        want = replay.frame(cam, fb, var, feat, SPP, 0.1, 5, hk_denoise.DEFAULT_SIGMA, tau=tau)
        assert all(_same(a, b) for a, b in zip(m.denoise_history() + (m.denoised(),), want)), i
        if tau > 0:
            assert _same(m.denoise_reject_stat(), replay.stat)
        else:
            with pytest.raises(hp.Refused, match="did not run with denoise_reject > 0"):
                m.denoise_reject_stat()
    assert (m.denoise_history()[2] >= 2).mean() > 0.5                     # (the history was found again under the turning camera)


@pytest.mark.parametrize("name", SCENES)
def test_moments_are_the_moments_replay(name):
    m, scene, frames = _model(name, denoise_moments=1)
    replay = hk_moments.Replay()
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, False)
        m.denoise_temporal()
        c, V, N, mom, out = replay.frame(cam, fb, var, feat, SPP, 0.1)
        assert all(_same(a, b) for a, b in zip(m.denoise_history() + (m.denoise_history_moments(), m.denoised()), (c, V, N, mom, out))), i


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("ridge", (None, 0.0, 1.0))
def test_layers_are_the_layered_replays(name, ridge):
    """ridge None: the a-trous iterations on the layer; otherwise the regression"""
    m, scene, frames = _model(name, denoise_layers=1, **({} if ridge is None else {"denoise_filter": 1, "denoise_ridge": ridge}))
    replay = hk_layers.Replay() if ridge is None else hk_regress.Replay()
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, True)
        y, B = hk_resolve.resolved(scene.lo(), RAYS, fb, feat)
        m.denoise()
        if ridge is None:
            out, L = hk_layers.layered(y, B, var, feat, SPP)[:2]
        else:
            out, L = hk_regress.layered(y, B, feat, ridge)[:2]
        assert _same(m.denoised(), out) and _same(m.denoised_layer(), L), i
        if i == 0:
            with pytest.raises(hp.Refused, match="no history"):                  # denoise neither reads nor writes it
                m.denoise_history()
        m.denoise_temporal()
        want = replay.frame(cam, y, B, var, feat, SPP, 0.1) if ridge is None else replay.frame(cam, y, B, var, feat, SPP, 0.1, ridge)
        assert all(_same(a, b) for a, b in zip(m.denoise_history() + (m.denoised(), m.denoised_layer()), want)), i
        assert _same(m.resolved(), y) and _same(m.resolve_background(), B)


@pytest.mark.parametrize("name", SCENES)
def test_resolve_is_the_host_resolve(name):
    m, scene, frames = _model(name)
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, True)
        y, B = hk_resolve.resolved(scene.lo(), RAYS, fb, feat)
        m.resolve()
        assert _same(m.resolved(), y) and _same(m.resolve_background(), B)
        m.denoise()
        assert _same(m.denoised(), hk_denoise.denoise(fb, var, feat, SPP))
        m.set("denoise_resolve", 1)
        m.denoise()
        assert _same(m.denoised(), hk_denoise.denoise(y, var, feat, SPP)) and not _same(y, fb)
        m.set("denoise_resolve", 0)


@pytest.mark.parametrize("name", SCENES)
def test_upsample_by_two_is_the_host_chain(name):
    m, scene, frames = _model(name, denoise_layers=1)
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, True)
        m.denoise()
        m.upsample(2, RAYS)
        out, Lh, fh, _ = hk_upsample.chain(m.denoised_layer(), feat, scene._at(2 * W, 2 * H), RAYS, 2)
        assert m.upsampled_size() == (2 * W, 2 * H)
        assert _same(m.upsampled(), out) and _same(m.upsampled_layer(), Lh) and _same(m.upsampled_features(), fh), i


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("ridge", (None, 0.0, 1.0))
def test_demodulated_layers_are_the_demodulated_call(name, ridge):
    """denoise_layers and denoise_demodulate on; ridge None: the a-trous iterations on the divided layer, otherwise the regression.  vr_denoise is
    hk_demod.layered, vr_denoise_temporal hk_demod.Replay (with a ridge too) over the three frames."""
    m, scene, frames = _model(name, denoise_layers=1, denoise_demodulate=1, **({} if ridge is None else {"denoise_filter": 1, "denoise_ridge": ridge}))
    replay = hk_demod.Replay(ridge=ridge)
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, True)
        y, B = hk_resolve.resolved(scene.lo(), RAYS, fb, feat)
        m.denoise()
        out, L = hk_demod.layered(y, B, var, feat, SPP, ridge=ridge)[:2]
        assert _same(m.denoised(), out) and _same(m.denoised_layer(), L), i
        if name == "c3env":                                   # (under the LUT the divided layer filters differently)
            assert not _same(out, hk_layers.layered(y, B, var, feat, SPP)[0] if ridge is None else hk_regress.layered(y, B, feat, ridge)[0])
        m.denoise_temporal()
        want = replay.frame(cam, y, B, var, feat, SPP, 0.1)
        assert all(_same(a, b) for a, b in zip(m.denoise_history() + (m.denoised(), m.denoised_layer()), want)), i
        assert _same(m.resolved(), y) and _same(m.resolve_background(), B)
    assert (m.denoise_history()[2] >= 2).mean() > 0.5


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("form", ("plain", "tau3", "moments"))
def test_the_demodulated_history_is_the_demodulated_replay(name, form):
    """the temporal pass on the divided layer: plain, with rejection (the statistic too), with the moments (the moment records too)"""
    tau = 3.0 if form == "tau3" else 0.0
    m, scene, frames = _model(name, denoise_layers=1, denoise_demodulate=1, denoise_reject=tau, denoise_moments=int(form == "moments"))
    replay = hk_demod.Replay(moments=form == "moments")
    for i in range(FRAMES):
        fb, var, feat, cam = _feed(m, scene, frames, i, True)
        y, B = hk_resolve.resolved(scene.lo(), RAYS, fb, feat)
        m.denoise_temporal()
        want = replay.frame(cam, y, B, var, feat, SPP, 0.1, tau=tau)
        assert all(_same(a, b) for a, b in zip(m.denoise_history() + (m.denoised(), m.denoised_layer()), want)), i
        if form == "tau3":
            assert _same(m.denoise_reject_stat(), replay.stat)
        if form == "moments":
            assert _same(m.denoise_history_moments(), replay.hist[3])
    assert (m.denoise_history()[2] >= 2).mean() > 0.5


@pytest.mark.parametrize("name", SCENES)
def test_a_ragged_demodulated_frame_takes_each_tiles_own_count(name):
    """synthetic per-tile counts of 2 and 8 by turns over the 3 x 2 tiles: hk_demod.layered on hk_adaptive.per_pixel of them, and not the call of either count"""
    m, scene, frames = _model(name, denoise_layers=1, denoise_demodulate=1)
    fb, var, feat, cam = _feed(m, scene, frames, 0, True)
    ty, tx = hk_adaptive.tiles_of(W, H)
    counts = np.array([(2, 8)[t & 1] for t in range(ty * tx)], np.int32)
    m.new_frame(fb, var, feat, "expected", RAYS, counts, cam)
    assert m.ragged()
    y, B = hk_resolve.resolved(scene.lo(), RAYS, fb, feat)
    m.denoise()
    out, L = hk_demod.layered(y, B, var, feat, hk_adaptive.per_pixel(counts, W, H))[:2]
    assert _same(m.denoised(), out) and _same(m.denoised_layer(), L)
    assert not _same(out, hk_demod.layered(y, B, var, feat, 2)[0]) and not _same(out, hk_demod.layered(y, B, var, feat, 8)[0])


@pytest.mark.parametrize("name", SCENES)
def test_upsample_reads_the_setting_at_its_call(name):
    """by 2: hk_demod.chain with the setting 1 at the call and hk_upsample.chain with 0, on a layer made with it and on one made without"""
    for made_with in (1, 0):
        m, scene, frames = _model(name, denoise_layers=1, denoise_demodulate=made_with)
        for i in range(FRAMES):
            fb, var, feat, cam = _feed(m, scene, frames, i, True)
            m.denoise()
            layer = m.denoised_layer()
            for at_call in (1, 0):
                m.set("denoise_demodulate", at_call)
                m.upsample(2, RAYS)
                chain = hk_demod.chain if at_call else hk_upsample.chain
                out, Lh, fh, _ = chain(layer, feat, scene._at(2 * W, 2 * H), RAYS, 2)
                assert m.upsampled_size() == (2 * W, 2 * H)
                assert _same(m.upsampled(), out) and _same(m.upsampled_layer(), Lh) and _same(m.upsampled_features(), fh), (made_with, at_call, i)
                assert _same(m.denoised_layer(), layer)
            if name == "c3env":                               # (under the LUT the two calls differ)
                assert not _same(out, hk_demod.chain(layer, feat, scene._at(2 * W, 2 * H), RAYS, 2)[0])
            m.set("denoise_demodulate", made_with)
    assert hp.tally([m.log])[("op", "upsample_demod")] == FRAMES


def test_a_refused_call_leaves_the_model_as_it_was_and_the_rule_on_the_stale_guide():
    """every refusal in turn on a model that holds every read-back; and the sequence of the header's rule: after a denoise without layers the upsample is refused
    with words of its own, the layer stays readable, and a denoise with layers makes the call available again"""
    m, scene, frames = _model("c3env", denoise_layers=1, denoise_reject=3.0)
    _feed(m, scene, frames, 0, True)
    m.denoise_temporal()
    m.upsample(2, RAYS)
    before = hp.read_all(m, hp.Refused)
    assert not any(isinstance(v, Exception) for k, v in before.items() if k != "denoise_history_moments")
    m.set("denoise_moments", 1)                                           # (drops the history: read again)
    m.set("denoise_moments", 0)
    before = hp.read_all(m, hp.Refused)
    for prepare, call, words in ((lambda: m.set_tiles((0, 1)), m.denoise, "a tile subset is set"),
                                 (lambda: m.set_tiles((0, 1)), lambda: m.upsample(2, 2), "a tile subset is set"),
                                 (lambda: m.set_tiles(()), None, None),
                                 (lambda: _feed(m, scene, frames, 0, False), m.denoise_temporal, "was not last filled by render_features_expected"),
                                 (lambda: _feed(m, scene, frames, 0, False), m.resolve, "was not last filled by render_features_expected"),
                                 (lambda: _feed(m, scene, frames, 0, True), None, None),
                                 (lambda: (m.set("denoise_layers", 0), m.set("denoise_demodulate", 1)), m.denoise, "denoise_demodulate = 1 needs denoise_layers = 1"),
                                 (lambda: None, m.denoise_temporal, "denoise_demodulate = 1 needs denoise_layers = 1"),
                                 (lambda: (m.set("denoise_demodulate", 0), m.set("denoise_filter", 1)), m.denoise, "denoise_filter = 1 needs denoise_layers = 1"),
                                 (lambda: (m.set("denoise_filter", 0), m.set("denoise_layers", 1)), None, None)):
        prepare()
        if call is not None:
            with pytest.raises(hp.Refused, match=words):
                call()
        assert hp.unchanged(before, hp.read_all(m, hp.Refused)) == []
    assert hp.tally([m.log])[("refused", "demod_layers")] == 2 and hp.tally([m.log])[("refused", "filter_layers")] == 1      # neither message is the other's kind
    assert hp.REFUSALS["filter_layers"] not in hp.REFUSALS["demod_layers"] and hp.REFUSALS["demod_layers"] not in hp.REFUSALS["filter_layers"]
    m.set("denoise_layers", 0)
    layer = m.denoised_layer()
    m.denoise()
    with pytest.raises(hp.Refused, match="the last denoise ran with denoise_layers = 0"):
        m.upsample(2, RAYS)
    assert _same(m.denoised_layer(), layer) and _same(m.upsampled(), before["upsampled"])
    m.set("denoise_layers", 1)
    with pytest.raises(hp.Refused, match="the last denoise ran with denoise_layers = 0"):      # the setting alone changes nothing
        m.upsample(2, RAYS)
    m.denoise()
    m.upsample(2, RAYS)


# ---- the all-pairs array -------------------------------------------------------------------------------------------------------------------------------------
def test_the_array_holds_every_accepted_pair_and_every_refused_combination():
    accepted, refusals = hp.covering_array()
    assert all(not hp.violated(r) for r in accepted) and all(hp.violated(r) for r in refusals)
    held, every = hp.all_pairs(accepted), hp.all_pairs()
    # a pair is forbidden iff it is an entry of FORBIDDEN or implies one: no accepted row of the whole product holds it (brute force, apart from the generator)
    import itertools
    possible = hp.all_pairs([r for r in itertools.product(*[vs for _, vs in hp.FACTORS]) if not hp.violated(r)])
    assert held == possible
    forbidden = every - possible
    assert {p for p in forbidden} <= hp.all_pairs(refusals)
    for combo in hp.FORBIDDEN:
        assert any(all(hp.row_dict(r)[f] == v for f, v in combo) for r in refusals), combo
    in_order = lambda p: tuple(sorted(p, key=lambda fv: hp.NAMES.index(fv[0])))      # noqa: E731
    assert {in_order(combo) for combo in hp.FORBIDDEN if len(combo) == 2} <= forbidden
    assert (hp.covering_array()[0], hp.covering_array()[1]) == (accepted, refusals)      # deterministic
    for name, (a, b) in hp.factor_pairs().items():
        assert [n for n, x, y in zip(hp.NAMES, a, b) if x != y] == [name]
    assert set(hp.factor_pairs()) == set(hp.NAMES) and all(hp.row_dict(r)["demodulate"] == 0 for n, p in hp.factor_pairs().items() if n != "demodulate" for r in p)
    assert set(hp.factor_pairs_demodulated()) == set(hp.DEMODULATED)
    for name, (a, b) in hp.factor_pairs_demodulated().items():
        assert [n for n, x, y in zip(hp.NAMES, a, b) if x != y] == [name] and not hp.violated(a) and not hp.violated(b)
        assert all(hp.row_dict(r)["demodulate"] == 1 and hp.row_dict(r)["layers"] == 1 for r in (a, b))
    with_setting = [hp.row_dict(r) for r in accepted if hp.row_dict(r)["demodulate"] == 1]
    assert len(with_setting) >= 4 and any(d["frame"] == "ragged" for d in with_setting) and all(d["layers"] == 1 for d in with_setting)
    assert any(hp.row_dict(r)["demodulate"] == 1 and hp.row_dict(r)["layers"] == 0 for r in refusals)
    print("all-pairs array: %d accepted rows, %d refusal rows, %d pairs held, %d pairs forbidden" % (len(accepted), len(refusals), len(held), len(forbidden)))
    assert len(accepted) <= 24 and len(refusals) <= 8


# ---- the sequences ---------------------------------------------------------------------------------------------------------------------------------------------
def _run(seed):
    m, tracer = hp.Model(hp.BlankScene(*hp.SIZES[0]), *hp.SIZES[0]), hp.StubTracer(*hp.SIZES[0])
    before = hp.read_all(m, hp.Refused)
    for op in hp.sequence(seed):
        refusal = hp.apply(m, op, tracer)
        after = hp.read_all(m, hp.Refused)
        if refusal is not None:
            assert hp.unchanged(before, after) == [], (seed, op)
        before = after
    return m.log


def test_the_seeds_fire_every_operation_every_drop_rule_and_every_refusal_twice():
    """counted on the model alone, over blank frames.  The mismatch clause (a history of one kind met by a call of the other) is counted too and stays at 0: every
    way the header offers to change "denoise_moments" or "denoise_layers" drops the history at the change, so no sequence of its calls reaches the clause."""
    assert len(hp.SEEDS) >= 8 and all(hp.sequence(s) == hp.sequence(s) for s in hp.SEEDS)
    lengths = [len(hp.sequence(s)) for s in hp.SEEDS]
    assert all(hp.LENGTH <= n <= hp.LENGTH + 10 for n in lengths)
    count = hp.tally(_run(s) for s in hp.SEEDS)
    for group, kinds in (("op", hp.OP_KINDS), ("drop", hp.DROP_RULES), ("refused", hp.CALL_REFUSALS)):
        print("%s: %s" % (group, ", ".join("%s %d" % (k, count.get((group, k), 0)) for k in kinds)))
    for group, kinds in (("op", hp.OP_KINDS), ("drop", [k for k in hp.DROP_RULES if k != "mismatch"]), ("refused", hp.CALL_REFUSALS)):
        for k in kinds:
            assert count.get((group, k), 0) >= 2, (group, k)
    assert count.get(("drop", "mismatch"), 0) == 0
