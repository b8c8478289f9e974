"""What tests/test_sched_counts_host.py (CPU) and tests/test_gpu_sched_counts.py (GPU) share: the scenes of the 14 compiled forms of the lane code, the frames,
the call splits, and the host build's counts per (form, frame, split) -- made once, cached, and never changed afterwards.

The per-path state machine is deterministic: which lane runs a path never changes the path.  So the number of lane steps entered in each state is a property of the
frame, not of the scheduler: the host harness (tests/hostkernel/host_kernel.cpp run_unit) counts it walking exactly the device's items (hk_render_tiles), the oracle
counts the same events in the reference's own terms (orc_counters), and the device's instrumented instances count the lanes each block of the scheduler ran for."""
import numpy as np

import hk_binding as hk
import scenes
from test_host_kernel import FORM_SCENES

# name -> (width, height, tile list or None = every tile).  40x24: six tiles, ragged both ways; 48x32 under a tile list: tile 5 is the top right one
FRAMES = {"40x24": (40, 24, None), "16x16": (16, 16, None), "1x1": (1, 1, None), "48x32_tiles": (48, 32, (0, 2, 5))}
# samples per call.  "4": one sample chunk whatever the kernel's unit (vr_variant.h pathtrace_unit_samples: 4 or 8 samples) -- the launches of 4 and of 12 units
SPLITS = {"11": (11,), "6+5": (6, 5), "4": (4,)}
RAGGED = "40x24"

_oracles = {}
_host = {}
_oracle_counts = {}


def form_id(f):
    return "v%d%s%s" % (f[0], "w" if f[1] and f[0] < 2 else "", "_lut" if f[2] else "")


def tiles_of(frame):
    w, h, tiles = FRAMES[frame]
    return list(tiles) if tiles is not None else list(range(((w + 15) // 16) * ((h + 15) // 16)))


def tile_rect(frame, t):
    w, h, _ = FRAMES[frame]
    tx = (w + 15) // 16
    x0, y0 = (t % tx) * 16, (t // tx) * 16
    return x0, y0, min(x0 + 16, w), min(y0 + 16, h)


def pixels_of(frame):
    return sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in (tile_rect(frame, t) for t in tiles_of(frame)))


def oracle_scene(form, frame):
    """The oracle renderer of the scene FORM_SCENES serves `form` with, at the frame's size and the scene's own camera: one per (scene, frame), shared by its forms"""
    config, lut, integrator, _ = FORM_SCENES[form]
    key = (config, lut, integrator, frame)
    if key not in _oracles:
        w, h, _ = FRAMES[frame]
        o = scenes.oracle_scene(config, w, h)
        if lut:
            o.load_transferfunc(scenes.LUT)
        o.integrator = integrator
        _oracles[key] = o
    return key, _oracles[key]


def host_counts(form, frame, split):
    """(per call: the host build's counters of `form` for the device's items of the frame's tile list, the frame after the last call): cached"""
    key = (form, frame, split)
    if key not in _host:
        _, o = oracle_scene(form, frame)
        variant, wide, _ = form
        tiles = FRAMES[frame][2]
        calls, fb, first = [], None, 1
        for n in SPLITS[split]:
            hk.form_steps(reset=True)
            fb, steps = hk.render_tiles(o, n, tiles=tiles, fb=fb, first_sample=first, wide=wide and variant < 2, blocked=FORM_SCENES[form][3])
            assert hk.forms_that_ran() == {form: steps}, (form, hk.forms_that_ran())      # the intended form served the scene, and no other
            calls.append(hk.form_steps()[form])
            first += n
        fb.setflags(write=False)
        _host[key] = (calls, fb)
    return _host[key]


def host_total(form, frame, split):
    calls, _ = host_counts(form, frame, split)
    return {k: sum(c[k] for c in calls) for k in calls[0]}


def oracle_counts(form, frame, split):
    """(per call: the oracle's counters over the pixels of the frame's tile list, the oracle's frame after the last call): cached per scene"""
    skey, o = oracle_scene(form, frame)
    key = (skey, split)
    if key not in _oracle_counts:
        o.reset()
        o.fb[:] = 0
        calls = []
        for n in SPLITS[split]:
            before, s0 = o.counters.as_dict(), o.sample
            for t in tiles_of(frame):
                o.sample = s0
                o.render(n, rect=tile_rect(frame, t))
            after = o.counters.as_dict()
            calls.append({k: after[k] - before[k] for k in after})
        fb = o.fb.copy()
        fb.setflags(write=False)
        _oracle_counts[key] = (calls, fb)
    return _oracle_counts[key]
