"""CPU: the host model of the renderer's image-space state (tests/hk_pipeline.py) held to what exists, before tests/test_gpu_pipeline.py lets it judge the
product: with one switch on at a time its three-frame sequences are the existing replays' (hk_temporal.Replay, hk_moments.Replay, hk_layers.Replay and layered,
hk_regress.Replay, hk_resolve.resolved, hk_upsample.chain) bit for bit; the all-pairs array holds every pair the product accepts and every combination it
refuses; and the committed seeds' call sequences fire every kind of operation, every rule that drops the history and every refusal at least twice.  The counts
are printed.  No device is touched.

The frames are test_denoise_host.oracle_inputs' (the oracle's per-sample radiances replayed through the accumulation pass's arithmetic, the host feature pass)
with a seed and a camera per frame, plus the host build of the expected-value pass: c2 and c3env at 33x31, 4 spp, the camera turned 1 degree per frame."""
import numpy as np
import pytest

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
                                 (lambda: _feed(m, scene, frames, 0, True), None, None)):
        prepare()
        if call is not None:
            with pytest.raises(hp.Refused, match=words):
                call()
        assert hp.unchanged(before, hp.read_all(m, hp.Refused)) == []
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
