"""GPU: the two addressing forms of the hot pair's gathers, and the shortcut for blocked shadow rays, against the oracle.

Kernel variants 0 and 1 form the byte offsets of their gathers into the grids' tables in 32 bits and exist a second time with 64-bit addresses for tables
of 4 GiB or more (vr_trace.h table_load, vr_variant.h pathtrace_kernel_of); vr_set_int "wide_addressing" forces the second set, so both run here on small
grids: every frame below is rendered once per form and must be the oracle's, bit for bit.  The last scene -- 1000 bounces at albedo 1 -- ends most of its
shadow rays blocked, which is where collide_finish takes its shortcut (tests/test_collide_shadow_host.py holds the code behind it to the reference)."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 56, 8      # ragged in both directions against the 16x16 tiles and the 8x8 work units


def _volume_smoke(r, o, lut=False, bounces=100, albedo=None):
    for x, is_oracle in ((r, False), (o, True)):
        scenes.configure(x, "c3" if lut else "c2", is_oracle)
        x.bounces = bounces
        if albedo is not None:
            x.albedo = (albedo,) * 3


def _volume_dense64(r, o):
    import encoder_ref
    dens = scenes.synthetic_density(64)
    r.load_envmap(scenes.HDR)
    o.load_envmap(scenes.HDR)
    r.set_volume_dense_f16(dens)
    o.set_volume(encoder_ref.encode_dense_fp16(dens))
    for x in (r, o):
        x.cam_fov, x.bounces, x.albedo, x.phase, x.density_scale = 40.0, 16, (0.8, 0.8, 0.8), 0.3, 20.0


def _volume_odd_bricks(r, o):
    from oracle import binding as ob
    import encoder_ref
    a = scenes.crop_bricks(encoder_ref.encode_arrays(scenes.synthetic_density(64)), (5, 3, 7))
    r.load_envmap(scenes.HDR)
    o.load_envmap(scenes.HDR)
    r.set_volume_brick(a["transform"], a["n_bricks"], a["min_maj"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"], commit=True)
    g = ob.Grid()
    g.set(a["transform"], a["n_bricks"], a["min_maj"], a["brick_counter"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"])
    o.set_volume(g)
    for x in (r, o):
        x.cam_fov, x.bounces = 40.0, 6


SCENES = {
    "smoke_brick": (lambda r, o: _volume_smoke(r, o), 0),
    "smoke_brick_lut": (lambda r, o: _volume_smoke(r, o, lut=True), 0),
    "dense_64": (_volume_dense64, 1),
    "odd_brick_counts": (_volume_odd_bricks, 0),
    "blocked_shadow_rays": (lambda r, o: _volume_smoke(r, o, bounces=1000, albedo=1.0), 0),
}
_made = {}


def _scene(name):
    """(HIP renderer, the oracle's frame): built and rendered once, shared by both forms"""
    if name not in _made:
        import volren_amd
        from oracle import binding as ob
        r, o = volren_amd.Renderer(W, H), ob.OracleRenderer(W, H)
        SCENES[name][0](r, o)
        _made[name] = (r, o.render(SPP).copy())
    return _made[name]


@pytest.mark.parametrize("wide", (0, 1), ids=("offsets32", "addresses64"))
@pytest.mark.parametrize("name", list(SCENES))
def test_frame_matches_oracle_in_both_addressing_forms(name, wide):
    r, ref = _scene(name)
    r.wide_addressing = wide
    assert r.get_int("wide_addressing") == wide
    assert r.kernel_variant == SCENES[name][1]
    assert r.kernel_wide == wide                    # small tables: the form is the switch's
    r.reset()
    r.render(SPP)
    fb = r.framebuffer()
    assert ref[..., 3].max() > 0
    nbad = int((fb.view(np.uint32) != ref.view(np.uint32)).any(-1).sum())
    assert nbad == 0, "%s, wide_addressing %d: %d pixels differ from the oracle (relative L2 %.3e)" % (name, wide, nbad, scenes.rel_l2(fb[..., :3], ref[..., :3]))


def test_switch_refuses_other_values():
    r, _ = _scene("smoke_brick")
    with pytest.raises(Exception):
        r.wide_addressing = 2
    r.wide_addressing = 0
