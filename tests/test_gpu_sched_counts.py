"""GPU: the scheduler's work counts, instrumented instances against the host build of the lane code.

pathtrace_kernel (csrc/vr_pathtrace.h) -- persistent wavefronts, the work queue in 8 segments, the slot stacks, the event batches -- is judged by its frames, and a
frame cannot see how OFTEN work was done: a unit handed out twice, an item started twice write the same bits to the same pool slot.  The per-path state machine is
deterministic, so the lanes each block of the scheduler ran for are a property of the frame: tests/test_sched_counts_host.py holds the host build's counts of exactly
those to the oracle, and this file holds every instrumented (STATS) instance to the host's -- on every frame, call split and threshold set below, among them the
smallest launches: 4 units (one tile, one chunk: segments 4 to 7 of the queue are empty ranges), 12 units (3 workgroups: segments 3 to 5 are reached only by
stealing), a partial last chunk (11 samples in units of 4 or 8), a second call with first_sample > 1.  Per cell, under sched_stats(True):

  1. the frame is the uninstrumented frame, bit for bit (and that one the host build's)
  2. new lanes == listed tiles x 256 x samples, summed over the calls
  3. the lanes of march, collide, nee, postnee and escape == the host build's counts for the same tile list, exactly
  4. pool conservation: after the resume block every slot is held by a lane or on exactly one stack, so the raw occupancy words 26..31 summed == pool x iterations;
     the pool is the threshold set's cap where it has one below the instance's own, else the instance's own: one integer in (64, 189], the same in every run
  5. executions <= lanes <= 64 executions per block; new executions >= units x ceil(items per unit / 64) (a NEW batch never crosses a unit); resumes and parks <=
     iterations; waves == 4 ceil(units / 4) per launch (launches of at most 256 units)

The tolerance-mode twins (fast_math = 1) trace other paths than the host build: laws 2, 4 and 5 only.  What the laws cannot see: DESIGN.md section 10."""
import numpy as np
import pytest

from hk_common import bits as _bits
import scenes
import sched_cases as sc

pytestmark = pytest.mark.gpu

# row -> (config, transfer function on top, majorant_layout, integrator, expected kernel_variant, the wide_addressing values the variant has a build for): the rows of
# tests/test_gpu_general_forms.py, and the run-time variant behind the global-majorant trackers as tests/test_host_kernel.py FORM_SCENES selects it
ROWS = {
    "c2": ("c2", False, 0, 0, 0, (0, 1)),
    "c3": ("c3", False, 0, 0, 0, (0, 1)),                    # (the config brings its LUT)
    "c4": ("c4:64", False, 0, 0, 1, (0, 1)),
    "c4_lut": ("c4:64", True, 0, 0, 1, (0, 1)),
    "c5": ("c5:64", False, 0, 0, 2, (0,)),
    "c5_lut": ("c5:64", True, 0, 0, 2, (0,)),
    "c5_blocked": ("c5:64", False, 1, 0, 4, (0,)),
    "c5_blocked_lut": ("c5:64", True, 1, 0, 4, (0,)),
    "c2_global": ("c2", False, 0, 1, 3, (0,)),
    "c3_global": ("c3", False, 0, 1, 3, (0,)),
}
INSTANCES = [(row, wide) for row in ROWS for wide in ROWS[row][5]]
TOLERANCE = [(row, wide) for row, wide in INSTANCES if not (ROWS[row][1] or row.startswith("c3"))]
_ids = lambda v: "%s-%s" % (v[0], "addresses64" if v[1] else "offsets32") if isinstance(v, tuple) else v
SCHED_DEFAULT = [64, 0, 56, 0, 60, 60, 64, 0]
BLOCKS = ("march", "collide", "nee", "postnee", "escape")


def _fuzz_row(seed):
    """one row of tests/test_gpu_parity.py::test_scheduler_and_launch_fuzz_against_the_oracle's generator"""
    rs = np.random.RandomState(seed)
    cap = int(rs.choice([0, 0, 70, 100, 150]))
    new = int(rs.randint(1, 65))
    if cap:
        new = min(new, cap)
    return [new, cap, int(rs.randint(1, 65)), int(rs.randint(1, 65)), int(rs.randint(1, 65)), int(rs.randint(1, 65)), int(rs.randint(1, 65)), 0]


# (the defaults first: they show the instance's own pool, which the capped sets are judged by)
SCHEDS = [SCHED_DEFAULT, [1, 66, 1, 1, 1, 1, 1, 0], [64, 0, 64, 64, 64, 64, 64, 0]] + [_fuzz_row(s) for s in (11, 12, 13)]
_made = {}
_own_pool = {}
_no_occupancy = []


def _skip_without_occupancy():
    if _no_occupancy:
        pytest.skip("law 4 (pool conservation) not checked, every other law held: the library reports zero cycles, it was built with VR_STATS_LEVEL 1")


def _form(row, wide):
    config, lut, _, _, variant, _ = ROWS[row]
    return (variant, bool(wide) or variant >= 2, lut or config == "c3")


def _renderer(row, wide, frame, fast=False):
    """The row's HIP renderer at the frame's size with the instance selected: the intended instance serves the next launch"""
    config, lut, layout, integrator, variant, _ = ROWS[row]
    w, h, tiles = sc.FRAMES[frame]
    if (config, lut) not in _made:
        r = scenes.hip_scene(config, w, h)
        if lut:
            r.load_transferfunc(scenes.LUT)
        _made[(config, lut)] = r
    r = _made[(config, lut)]
    if (r.width, r.height) != (w, h):
        r.resize(w, h)
    r.set_tiles(list(tiles) if tiles is not None else [])
    r.integrator = integrator
    r.majorant_layout = layout
    r.wide_addressing = wide
    r.fast_math = 1 if fast else 0
    r.set_sched(SCHED_DEFAULT)
    assert r.kernel_variant == variant, (row, r.kernel_variant)
    assert r.kernel_wide == (1 if (wide or variant >= 2) else 0)
    assert r.kernel_variant_reason == (1 if integrator else 0)
    return r


def _render(r, ns):
    """a frame in the split's calls: (frame, path-tracing launches)"""
    r.reset()
    launches = 0
    for n in ns:
        r.render(n)
        launches += r.last_launches
    return r.framebuffer().copy(), launches


def _units(variant, n_tiles, n):
    spu = min(n, 4 if variant in (1, 2, 4) else 8)                               # vr_variant.h pathtrace_unit_samples
    return n_tiles * 4 * ((n + spu - 1) // spu)


def _scheduler_laws(what, st, variant, n_tiles, ns, sched, instance):
    """laws 2, 4 and 5: what holds whatever paths the instance traces"""
    samples = sum(ns)
    assert st["new"][1] == n_tiles * 256 * samples, (what, st["new"])            # 2
    raw = st["raw"]
    occupied, iterations = sum(raw[26:32]), st["iterations"]
    assert iterations > 0, what
    if st["wave_cycles"] != 0:                                                   # 4 (a library built with VR_STATS_LEVEL 1 keeps no occupancy words: _no_occupancy)
        assert occupied % iterations == 0, (what, occupied, iterations)
        pool = occupied // iterations
        if sched is SCHED_DEFAULT:
            assert 64 < pool <= 189, (what, pool)
            assert _own_pool.setdefault(instance, pool) == pool, (what, pool, _own_pool[instance])
        own = _own_pool[instance]
        assert pool == (sched[1] if 0 < sched[1] < own else own), (what, pool, sched[1], own)
    else:
        _no_occupancy.append(what)
    for block in ("new",) + BLOCKS:                                              # 5
        ex, lanes = st[block]
        assert ex <= lanes <= 64 * ex, (what, block, ex, lanes)
    assert st["new"][0] >= n_tiles * 4 * samples, (what, st["new"])              # units x ceil(items per unit / 64), summed: a unit holds 64 items per sample
    assert st["resumes"] <= iterations and st["parks"] <= iterations, (what, st["resumes"], st["parks"], iterations)
    units = [_units(variant, n_tiles, n) for n in ns]
    assert max(units) <= 256
    assert st["waves"] == sum(4 * ((u + 3) // 4) for u in units), (what, st["waves"], units)
    return units


@pytest.mark.parametrize("frame", list(sc.FRAMES))
@pytest.mark.parametrize("instance", INSTANCES, ids=_ids)
def test_instrumented_counts_match_the_host_build(instance, frame):
    row, wide = instance
    variant, form, n_tiles = ROWS[row][4], _form(row, wide), len(sc.tiles_of(frame))
    r = _renderer(row, wide, frame)
    seen_units = set()
    try:
        for split, ns in sc.SPLITS.items():
            host, host_frame = sc.host_total(form, frame, split), sc.host_counts(form, frame, split)[1]
            plain, _ = _render(r, ns)
            assert np.array_equal(_bits(plain), _bits(host_frame)), (instance, frame, split, "uninstrumented frame against the host build's")
            for sched in SCHEDS:
                what = (instance, frame, split, sched)
                r.set_sched(sched)
                r.sched_stats(True)
                try:
                    got, launches = _render(r, ns)
                finally:
                    st = r.sched_stats(False, read=True)
                assert launches == len(ns), what                                 # one launch per call: the laws on `waves` and the unit counts rest on it
                print(what, {k: st[k] for k in ("new",) + BLOCKS + ("resumes", "parks", "iterations", "waves")}, sum(st["raw"][26:32]))
                assert np.array_equal(_bits(got), _bits(plain)), (what, "instrumented frame")          # 1
                assert st["new"][1] == host["new"] == n_tiles * 256 * sum(ns), (what, "law 2", st["new"], host["new"])      # 2
                for block in BLOCKS:                                                                  # 3
                    assert st[block][1] == host[block], (what, "law 3", block, st[block], host[block])
                seen_units.update(_scheduler_laws(what, st, variant, n_tiles, ns, sched, ("exact",) + instance))
    finally:
        r.set_sched(SCHED_DEFAULT)
        r.set_tiles([])
    if frame in ("16x16", "1x1"):
        assert 4 in seen_units           # one tile, one chunk
    if frame == "48x32_tiles":
        assert 12 in seen_units          # three workgroups
    _skip_without_occupancy()


@pytest.mark.parametrize("frame", list(sc.FRAMES))
@pytest.mark.parametrize("instance", TOLERANCE, ids=_ids)
def test_tolerance_mode_twins_obey_the_scheduler_laws(instance, frame):
    row, wide = instance
    variant, n_tiles = ROWS[row][4], len(sc.tiles_of(frame))
    r = _renderer(row, wide, frame, fast=True)
    try:
        for split, ns in sc.SPLITS.items():
            for sched in SCHEDS:
                what = (instance, frame, split, sched, "fast_math")
                r.set_sched(sched)
                r.sched_stats(True)
                try:
                    _, launches = _render(r, ns)
                finally:
                    st = r.sched_stats(False, read=True)
                assert launches == len(ns)
                _scheduler_laws(what, st, variant, n_tiles, ns, sched, ("fast",) + instance)
    finally:
        r.fast_math = 0
        r.set_sched(SCHED_DEFAULT)
        r.set_tiles([])
    _skip_without_occupancy()
