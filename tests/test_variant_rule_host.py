"""The product's own rule for which compiled path-tracing kernel serves a scene (volren_amd/csrc/vr_variant.h pathtrace_kernel_of), built for the host
and held to a table.  The launch, the renderer's marshalling, the C ABI's read-outs and the host harness (hk_binding.FORMS: form = 2 * instance + tf) all
ask that one function, so an edit to the rule shows here, without a GPU.  The expected values are written out, not computed: each is what the rule
answered when it still lived in vr_launch.hip (pathtrace_variant_of, pathtrace_wide_of, pathtrace_reads_seed_table), checked by reading those."""
import numpy as np
import pytest

import hk_variant as hv
from hk_variant import brick_grid as B
from hk_variant import dense_grid as D

INTEGRATOR, ENV_DIVISION, DENSITY_SCALE, GRID_FORMS = 1, 2, 4, 8      # vr_variant.h PathtraceVariantReason

F32 = np.float32
SCALE_MIN, SCALE_MAX = F32(2.0 ** -16), F32(2.0 ** 24)
BELOW_MIN, ABOVE_MAX = np.nextafter(SCALE_MIN, F32(0)), np.nextafter(SCALE_MAX, F32(np.inf))


def _k(variant, reason, instance, wide, item=0, seed=0, unit=8):
    return dict(variant=variant, reason=reason, instance=instance, wide=wide, item_integrator=item, reads_seed_table=seed, samples_per_unit=unit)


BLOCKED = B(maj_blocked=True)
RUN_TIME = dict(instance=6, wide=1, unit=8)      # variant 3: one build, which is wide, units of 8

# (what, scene, force_wide, instrumented, expected answer)
KERNELS = [
    # a brick grid, no emission grid, everything in range
    ("bricks", hv.scene(B()), False, False, _k(0, 0, 0, 0, seed=1)),
    ("bricks, instrumented", hv.scene(B()), False, True, _k(0, 0, 0, 0, seed=0)),
    ("bricks, forced wide", hv.scene(B()), True, False, _k(0, 0, 1, 1, seed=1)),
    ("bricks + LUT", hv.scene(B(), use_tf=1), False, False, _k(0, 0, 0, 0, seed=1)),
    # a dense grid, no emission grid
    ("dense", hv.scene(D()), False, False, _k(1, 0, 2, 0, unit=4)),
    ("dense, forced wide", hv.scene(D()), True, False, _k(1, 0, 3, 1, unit=4)),
    # two brick grids
    ("paired", hv.scene(B(), B(), paired=1), False, False, _k(2, 0, 4, 1, unit=4)),
    ("paired, blocked majorants", hv.scene(BLOCKED, B(), paired=1), False, False, _k(4, 0, 5, 1, unit=4)),
    ("not paired", hv.scene(B(), B(), paired=0), False, False, _k(3, GRID_FORMS, **RUN_TIME)),
    ("dense density + emission", hv.scene(D(), B(), paired=1), False, False, _k(3, GRID_FORMS, **RUN_TIME)),
    ("density + dense emission", hv.scene(B(), D(), paired=1), False, False, _k(3, GRID_FORMS, **RUN_TIME)),
    # integrator and environment
    ("integrator 1", hv.scene(B(), integrator=1), False, False, _k(3, INTEGRATOR, **RUN_TIME)),
    ("integrator 3", hv.scene(B(), integrator=3), False, False, _k(3, INTEGRATOR, item=3, **RUN_TIME)),
    ("integrator 2 + LUT", hv.scene(B(), integrator=2, use_tf=1), False, False, _k(3, INTEGRATOR, item=2, **RUN_TIME)),
    ("integrator 2, no LUT", hv.scene(B(), integrator=2), False, False, _k(3, INTEGRATOR, **RUN_TIME)),
    ("unsafe warp table", hv.scene(B(), env_div_safe=0), False, False, _k(3, ENV_DIVISION, **RUN_TIME)),
    # (a reason of the first three keeps GRID_FORMS out)
    ("all three, mixed emission grids", hv.scene(B(), D(), integrator=1, env_div_safe=0, density_scale=BELOW_MIN), False, False,
     _k(3, INTEGRATOR | ENV_DIVISION | DENSITY_SCALE, **RUN_TIME)),
    # the density scale: [2^-16, 2^24], both ends in range
    ("scale 2^-16", hv.scene(B(), density_scale=SCALE_MIN), False, False, _k(0, 0, 0, 0, seed=1)),
    ("scale below 2^-16", hv.scene(B(), density_scale=BELOW_MIN), False, False, _k(3, DENSITY_SCALE, **RUN_TIME)),
    ("scale 2^24", hv.scene(B(), density_scale=SCALE_MAX), False, False, _k(0, 0, 0, 0, seed=1)),
    ("scale above 2^24", hv.scene(B(), density_scale=ABOVE_MAX), False, False, _k(3, DENSITY_SCALE, **RUN_TIME)),
    ("scale NaN", hv.scene(B(), density_scale=np.nan), False, False, _k(3, DENSITY_SCALE, **RUN_TIME)),
    # wide by size, variants 0 and 1: a table of 2^32 bytes or more.  Atlas blocks of 640 bytes: 256 x 256 x 102 of them are 4278190080 bytes, x 103 4320133120
    ("byte atlas below 4 GiB", hv.scene(B((256, 256, 102), (8, 8, 7))), False, False, _k(0, 0, 0, 0, seed=1)),
    ("byte atlas above 4 GiB", hv.scene(B((256, 256, 103), (8, 8, 7))), False, False, _k(0, 0, 1, 1, seed=1)),
    # the decoded float atlas, 2048 bytes per brick: 128^3 bricks are exactly 2^32 bytes, and the bound is inclusive
    ("float atlas below 4 GiB", hv.scene(B((128, 128, 127), (7, 7, 7), atlas_f32=True), use_tf=1), False, False, _k(0, 0, 0, 0, seed=1)),
    ("float atlas of 4 GiB", hv.scene(B((128, 128, 128), (7, 7, 7), atlas_f32=True), use_tf=1), False, False, _k(0, 0, 1, 1, seed=1)),
    # dense blocks of 128 bytes: 512 x 512 x 127 of them are below, x 128 exactly 2^32 bytes
    ("dense below 4 GiB", hv.scene(D((2048, 2048, 508), (256, 256, 64), (8, 8, 6))), False, False, _k(1, 0, 2, 0, unit=4)),
    ("dense of 4 GiB", hv.scene(D((2048, 2048, 512), (256, 256, 64), (8, 8, 6))), False, False, _k(1, 0, 3, 1, unit=4)),
]


@pytest.mark.parametrize("what,scene,force_wide,instrumented,want", KERNELS, ids=[row[0] for row in KERNELS])
def test_kernel_of_scene(what, scene, force_wide, instrumented, want):
    got = hv.kernel_of(scene, force_wide, instrumented)
    assert {k: got[k] for k in want} == want, what
    assert got["scene_reasons"] == want["reason"] & ~GRID_FORMS


# "the scene's two grids are read from a paired atlas": an emission grid, both grids in brick form with the same brick layout, and nothing that sends the
# scene to the run-time variant whatever its grids
PAIRS = [
    ("two brick grids of one layout", hv.scene(B(), B()), 1),
    ("no emission grid", hv.scene(B()), 0),
    ("dense density grid", hv.scene(D(), B()), 0),
    ("dense emission grid", hv.scene(B(), D()), 0),
    ("other brick layout", hv.scene(B((4, 4, 4)), B((4, 4, 5))), 0),
    ("integrator", hv.scene(B(), B(), integrator=1), 0),
    ("unsafe warp table", hv.scene(B(), B(), env_div_safe=0), 0),
    ("density scale", hv.scene(B(), B(), density_scale=ABOVE_MAX), 0),
]


@pytest.mark.parametrize("what,scene,want", PAIRS, ids=[row[0] for row in PAIRS])
def test_which_scenes_pair_their_atlases(what, scene, want):
    assert hv.kernel_of(scene)["pairs"] == want, what


def test_the_bounds_of_the_density_scale_are_the_neighbours_the_table_names():
    assert float(SCALE_MIN) == 1.0 / 65536.0 and float(SCALE_MAX) == 16777216.0 and float(ABOVE_MAX) == 16777218.0 and BELOW_MIN < SCALE_MIN
