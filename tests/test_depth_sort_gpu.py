"""The per-tile depth sort of csrc/binning.hip at every size class, tie and fallback.

The frames of tests/depth_sort_cases.py put a chosen number of Gaussians with a chosen depth pattern into each tile
(tests/test_depth_sort_cases_cpu.py checks that they do, and that together they stand on every tier edge).  Each frame is
rendered forward and ``L``, the tile ranges and the whole sorted list are compared with the CPU oracle's stable sort by
(tile, depth bits) over ascending ids -- the (depth bits, id) order -- exactly: no tolerance, no entry left out.

Three ways per frame: the two-stage forward (the host rule sees the frame's own ``L``), the speculative single-call
forward (it routes by its capacity: quad and heavy kernels on these small grids, whatever the frame), and ``debug=True``
(the one-wave kernel also writes the tile-id column).  One more test reads the kernels' own counters (HGS_SORT_DEBUG) in
a child process per frame family: the route the restated host rule predicts is the route that ran."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import depth_sort_cases as dc

pytestmark = pytest.mark.gpu

FRAMES = list(dc.FRAME_SPECS)


def _check(name, L, ranges, plist, how):
    m = dc.mismatches(name, L, ranges, plist)
    tiles = "; ".join("tile %(tile)d n %(n)d %(pattern)s %(sorter)s: %(bad)d wrong" % t for t in m["tiles_bad"][:8])
    assert dc.clean(m), (f"{how}: {name}: L {m['L']} (oracle {m['L_ref']}), {m['ranges_bad']} range words and "
                         f"{m['list_bad']} list entries differ -- {tiles}")


@pytest.mark.parametrize("name", FRAMES)
def test_exact_L_route(gpu, monkeypatch, name):
    """Two-stage forward: launch_tile_depth_sort is handed the frame's own L and takes the route the frame was built for."""
    import diff_gaussian_rasterization as dgr
    C = dgr._C
    monkeypatch.setattr(C, "SPECULATIVE", False)
    C._last_L.clear()
    call, L, ranges, plist = dc.render(name, gpu)
    assert call.L_ws == call.L == L
    _check(name, L, ranges, plist, "exact L")


@pytest.mark.parametrize("name", FRAMES)
def test_speculative_repeat_routes_by_capacity(gpu, monkeypatch, name):
    """The second call of a shape goes through hgs_raster_fwd with a capacity of at least SPEC_SLACK = 65536 > 1024 T: the
    quad kernel, the mid kernel and the big kernel sort every frame, a light one too, and must produce the identical list."""
    import diff_gaussian_rasterization as dgr
    C = dgr._C
    monkeypatch.setattr(C, "SPECULATIVE", True)
    C._last_L.clear()
    fr = dc.build(name)
    call, L, ranges, plist = dc.render(name, gpu)
    assert call.L_ws == L                                                  # first call of the shape: two-stage
    _check(name, L, ranges, plist, "first call")
    spec0, miss0 = C.stats["speculative_calls"], C.stats["capacity_misses"]
    call, L, ranges, plist = dc.render(name, gpu)
    assert C.stats["speculative_calls"] == spec0 + 1 and C.stats["capacity_misses"] == miss0
    assert call.L_ws >= C.SPEC_SLACK > 1024 * fr.route["T"] and call.L == L
    _check(name, L, ranges, plist, "speculative repeat")


@pytest.mark.parametrize("name", ["light_tiers", "quad_tiers"])
def test_debug_forward_keeps_the_lists(gpu, monkeypatch, name):
    """debug=True: the one-wave kernel also writes every instance's tile id (and every launch is checked synchronously)."""
    import diff_gaussian_rasterization as dgr
    C = dgr._C
    monkeypatch.setattr(C, "SPECULATIVE", False)
    C._last_L.clear()
    call, L, ranges, plist = dc.render(name, gpu, debug=True)
    _check(name, L, ranges, plist, "debug")
    # the column itself (raster_views derives its tile ids from the ranges whenever those add up): the raw words
    import ctypes
    import torch
    from hgs import _lib
    v = _lib.RasterViews()
    _lib.check(_lib.lib().hgs_raster_views_get(call.P, call.W, call.H, call.L_ws, call.p_geom, call.p_bin, call.p_img,
                                               ctypes.byref(v)), "hgs_raster_views_get")
    off = v.tile_ids_sorted - call.binb.data_ptr()
    tiles = call.binb[off:off + 4 * L].view(torch.int32).cpu().numpy().astype(np.int64)
    assert np.array_equal(tiles, np.repeat(np.arange(ranges.shape[0]), dc.build(name).lengths))


_CHILD = r"""
import json, os, sys
root = sys.argv[1]
for p in (root, os.path.join(root, "hierarchical-3d-gaussians_amd"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
import depth_sort_cases as dc
import diff_gaussian_rasterization as dgr
dgr._C.SPECULATIVE = False
for name in sys.argv[2:]:
    call, L, ranges, plist = dc.render(name, "cuda:0")
    print("frame " + json.dumps(dc.mismatches(name, L, ranges, plist)), flush=True)
"""
_LINE = re.compile(r"\[hgs\] tile_depth_sort: L (\d+) T (\d+) quad (\d+): large (\d+) huge (\d+) network fallbacks (\d+)")


def test_the_predicted_route_is_the_route_that_ran(gpu):
    """HGS_SORT_DEBUG (read once per process) makes launch_tile_depth_sort print, after the one-wave / quad kernel, the
    frame's L, T, its choice of kernel and the three counters the kernel left: large and huge tiles filed, tiles the sample
    sort handed to the network.  Per family a fresh child renders the frames on the exact-L path; the parent checks

      * quad, large and huge against the restated host rule (large = huge = 0 on a light frame: it files nothing);
      * fallbacks >= the number of sample-sort-class tiles that hold more than kSsMaxBucket equal depths (all_equal,
        two_values, block65): equal depths share a fine bucket, so those tiles MUST have gone to the network;
      * fallbacks == 0 where every depth pattern is smooth or wide: the sort's design claim that fine buckets hold a few
        keys (an overflow needs more than 64 keys in one of 32 or 8 slices of a coarse bucket of about n / 64);
      * block64 and ulps (and outlier): correctness only.
    """
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = {}
    for family in dc.FAMILIES:
        names = dc.family_frames(family)
        r = subprocess.run([sys.executable, "-c", _CHILD, root] + names, env={**os.environ, "HGS_SORT_DEBUG": "1"},
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (family, r.returncode, r.stderr[-2000:])       # (no further child after a failure)
        frames = [json.loads(l[6:]) for l in r.stdout.splitlines() if l.startswith("frame ")]
        lines = [tuple(int(x) for x in m.groups()) for m in _LINE.finditer(r.stderr)]
        assert [f["frame"] for f in frames] == names and len(lines) == len(names), (family, r.stdout, r.stderr[-2000:])
        for name, m, (L, T, quad, large, huge, fallbacks) in zip(names, frames, lines):
            fr = dc.build(name)
            rt = fr.route
            seen[name] = dict(route=rt["name"], L=L, T=T, quad=quad, large=large, huge=huge, fallbacks=fallbacks,
                              min_fallbacks=fr.min_fallbacks)
            print("depth-sort route", name, json.dumps(seen[name]))
            assert dc.clean(m), m
            assert (L, T) == (rt["L"], rt["T"]), (name, L, T)
            assert (quad, large, huge) == (int(rt["quad"]), rt["large"], rt["huge"]), (name, seen[name], rt)
            assert fallbacks >= fr.min_fallbacks, (name, seen[name])
            if fr.zero_fallbacks:
                assert fallbacks == 0, (name, seen[name])
    assert set(seen) == set(FRAMES)
    assert {s["route"] for s in seen.values()} == {"light", "quad", "heavy"}
    assert any(s["min_fallbacks"] > 0 for s in seen.values())
