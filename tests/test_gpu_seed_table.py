"""GPU: the path-seed table never changes a frame.  smoke.brick (the brick kernel, which reads the table; units of 8 samples) and a 64^3 dense grid (the
dense kernel, which was measured no faster with it and goes on hashing: its launches make no table, whatever the settings; units of 4) at 72x56 -- ragged, 5 x 4 tiles -- and 24 spp, every frame against the CPU oracle bit for bit: table on and off, a cap inside a work unit, frames that
reuse the table, changes of seed, size, tile set, call protocol and stream, a poisoned table, and both arithmetic modes on one table."""
import numpy as np
import pytest

from hk_common import bits as _bits
import scenes

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 56, 24
SCENES = ("c2", "c4:64")
_REF = {}


def _ref(name, w=W, h=H, seed=42, spp=SPP):
    """the oracle's frame, computed once per (scene, size, seed, spp) and never written to"""
    key = (name, w, h, seed, spp)
    if key not in _REF:
        o = scenes.oracle_scene(name, w, h)
        o.seed = seed
        f = o.render(spp).copy()
        f.setflags(write=False)
        _REF[key] = f
    return _REF[key]


def _same(r, ref, what):
    hip = r.framebuffer()
    nbad = int((_bits(hip) != _bits(ref)).any(-1).sum())
    assert nbad == 0, "%s: %d of %d pixels differ from the oracle" % (what, nbad, ref.shape[0] * ref.shape[1])


def _n(name, n):
    """what a counter of the table reads on scene `name`: n where the scene's kernel reads the table (smoke.brick), 0 where it hashes (the dense grid)"""
    return n if name == "c2" else 0


def _frame(r, spp=SPP):
    r.reset()
    r.render(spp)


@pytest.mark.parametrize("name", SCENES)
def test_table_on_and_off(name):
    r = scenes.hip_scene(name, W, H)
    assert r.seed_table_mb == 4096 and r.seed_table_samples == 0
    _frame(r)
    assert r.seed_table_samples == _n(name, SPP) and r.seed_table_fills == _n(name, 1) and r.kernel_variant == (0 if name == "c2" else 1)
    _same(r, _ref(name), "table on")
    r.seed_table_mb = 0
    _frame(r)
    assert r.seed_table_samples == 0 and r.seed_table_fills == _n(name, 1)
    _same(r, _ref(name), "table off")


@pytest.mark.parametrize("cap", (12, 10, 1))
@pytest.mark.parametrize("name", SCENES)
def test_a_cap_inside_a_work_unit(name, cap):
    """12: the brick kernel's unit of samples 9..16 straddles it; 10: so does the dense kernel's unit 9..12; 1: every unit but a sample"""
    r = scenes.hip_scene(name, W, H)
    r.seed_table_max_samples = cap
    _frame(r)
    assert r.seed_table_samples == _n(name, cap)
    _same(r, _ref(name), "cap %d" % cap)
    r.seed_table_max_samples = 0                     # the setting changes: the table starts over
    _frame(r)
    assert r.seed_table_samples == _n(name, SPP)
    _same(r, _ref(name), "cap lifted")


def test_a_budget_sets_the_cap():
    """1 MiB on a 640x16 frame (40 tiles, 40 KiB per sample): samples 1..25 of 32"""
    r = scenes.hip_scene("c2", 640, 16)
    r.seed_table_mb = 1
    _frame(r, 32)
    assert r.seed_table_samples == 25 == (1 << 20) // (40 * 1024)
    _same(r, _ref("c2", 640, 16, spp=32), "1 MiB")


@pytest.mark.parametrize("name", SCENES)
def test_the_second_frame_launches_no_fill(name):
    r = scenes.hip_scene(name, W, H)
    _frame(r)
    _same(r, _ref(name), "first frame")
    assert r.seed_table_fills == _n(name, 1)
    _frame(r)                                        # reset() keeps the table
    assert r.seed_table_fills == _n(name, 1) and r.seed_table_samples == _n(name, SPP)
    _same(r, _ref(name), "second frame")
    _frame(r, 8)                                     # fewer samples: nothing to fill either
    assert r.seed_table_fills == _n(name, 1) and r.seed_table_samples == _n(name, SPP)
    _same(r, _ref(name, spp=8), "shorter frame")


def test_the_table_grows_with_the_samples_asked_for():
    r = scenes.hip_scene("c2", W, H)
    r.render(8)
    assert r.seed_table_samples == 8 and r.seed_table_fills == 1
    r.render(16)                                     # samples 9..24 of the same frame: the uncovered part is filled, the rest moves over
    assert r.seed_table_samples == SPP and r.seed_table_fills == 2
    _same(r, _ref("c2"), "8 + 16")
    _frame(r)
    assert r.seed_table_fills == 2
    _same(r, _ref("c2"), "the grown table, read in full")


def test_a_seed_change_drops_the_table():
    r = scenes.hip_scene("c2", W, H)
    _frame(r)
    r.seed = 7
    _frame(r)
    assert r.seed_table_fills == 2 and r.seed_table_samples == SPP
    _same(r, _ref("c2", seed=7), "seed 7")
    r.seed = 42
    _frame(r)
    assert r.seed_table_fills == 3
    _same(r, _ref("c2"), "seed 42 again")


def test_a_resize_and_back():
    r = scenes.hip_scene("c2", W, H)
    _frame(r)
    r.resize(40, 40)
    assert r.seed_table_samples == 0
    _frame(r)
    _same(r, _ref("c2", 40, 40), "40x40")
    r.resize(W, H)
    _frame(r)
    assert r.seed_table_fills == 3
    _same(r, _ref("c2"), "72x56 again")


def _tile_mask(tiles):
    mask = np.zeros((H, W), bool)
    for t in tiles:
        tx, ty = t % 5, t // 5
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    return mask


@pytest.mark.parametrize("name", SCENES)
def test_every_other_tile(name):
    """a tile subset indexes the whole frame's table: its launch fills the table for the whole frame, and a launch over the frame reads what it filled"""
    ref = _ref(name)
    sub = list(range(1, 20, 2))
    mask = _tile_mask(sub)
    r = scenes.hip_scene(name, W, H)
    r.set_tiles(sub)
    _frame(r)
    fb = r.framebuffer()
    assert r.seed_table_fills == _n(name, 1) and r.seed_table_samples == _n(name, SPP)
    assert np.array_equal(_bits(fb[mask]), _bits(ref[mask])) and not fb[~mask].any()
    r.set_tiles([])
    _frame(r)
    assert r.seed_table_fills == _n(name, 1)
    _same(r, ref, "whole frame after the subset")
    r.set_tiles(list(range(0, 20, 2)))               # the other half, over the finished frame: the same pixels again
    _frame(r)
    assert r.seed_table_fills == _n(name, 1)
    _same(r, ref, "the other tiles over the whole frame")


def test_the_trace_protocol_one_sample_per_call():
    r = scenes.hip_scene("c2", W, H)
    r.coalesce_trace = 0
    for k in range(SPP):
        r.trace()
        assert r.seed_table_samples == k + 1          # grows with every call ...
    assert r.seed_table_fills == SPP
    _same(r, _ref("c2"), "24 x trace()")
    r.reset()
    for _ in range(SPP):
        r.trace()
    assert r.seed_table_fills == SPP                 # ... and the next frame fills nothing
    _same(r, _ref("c2"), "24 x trace() again")
    r.coalesce_trace = 1
    r.reset()
    for _ in range(SPP):
        r.trace()
    _same(r, _ref("c2"), "coalesced")


def test_a_stream_change_between_frames():
    import torch
    r = scenes.hip_scene("c2", W, H)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r.set_stream(s1.cuda_stream)
    r.reset()
    r.render(SPP, sync=False)                        # the fill and the frame on s1; the host does not wait for them
    s2.wait_stream(s1)                               # the caller's part: the frames share the renderer's framebuffer and pools, so s2 goes behind s1
    r.set_stream(s2.cuda_stream)
    r.reset()
    r.render(SPP, sync=False)                        # no fill: the table is the one s1 filled
    r.synchronize()
    assert r.seed_table_fills == 1
    _same(r, _ref("c2"), "second stream")
    r.set_stream(s1.cuda_stream)                     # (everything on s2 has finished: synchronize above)
    _frame(r)
    assert r.seed_table_fills == 1
    _same(r, _ref("c2"), "first stream again")
    r.set_stream(None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", SCENES)
def test_a_poisoned_table(name, monkeypatch):
    """the table is filled with a NaN pattern when it is allocated: no launch reads an entry its fill has not written"""
    monkeypatch.setenv("VR_TEST_POISON_WORKSPACE", "2")
    r = scenes.hip_scene(name, W, H)
    r.render(8)
    r.render(16)
    _same(r, _ref(name), "poisoned, grown")
    r.seed_table_max_samples = 12
    _frame(r)
    _same(r, _ref(name), "poisoned, capped")


def test_both_arithmetic_modes_share_one_table():
    r = scenes.hip_scene("c2", W, H)
    r.fast_math = 1
    _frame(r)
    fast_on = r.framebuffer().copy()
    assert r.seed_table_fills == 1
    r.fast_math = 0
    _frame(r)
    assert r.seed_table_fills == 1                   # the same table
    _same(r, _ref("c2"), "bit-exact mode after the tolerance mode")
    r.seed_table_mb = 0
    r.fast_math = 1
    _frame(r)
    assert np.array_equal(_bits(r.framebuffer()), _bits(fast_on))      # the tolerance mode's frame is the same with and without the table
    assert scenes.rel_l2(fast_on[..., :3], _ref("c2")[..., :3]) <= 1e-3
