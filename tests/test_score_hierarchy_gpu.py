"""hgs.importance.score_hierarchy / low_contribution_mask and ``python -m hgs.score_hierarchy`` on the 2 000-leaf
hierarchy (tests/contribution_cases.py) with three 64 x 48 orbit cameras, and the scores' use by the pruner."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import contribution_cases as cc
import frustum_cases as fc
from hgs import hierarchy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hierarchical-3d-gaussians_amd")
FAINT = 50


def _bits_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in ((a.wmax, b.wmax), (a.wsum, b.wsum), (a.count, b.count), (a.entries, b.entries))) and a.views == b.views


@functools.lru_cache(maxsize=None)
def _base():
    """(device hierarchy, Scores at tau_px = 0 without the frustum cull) of the untouched scene."""
    from hgs.importance import score_hierarchy
    dev = torch.device("cuda:0")
    h = cc.on_device(cc.hier2000(), dev)
    return h, score_hierarchy(h, cc.orbit(), tau_px=0.0, frustum=False)


@functools.lru_cache(maxsize=None)
def _faint():
    """The scene with FAINT leaves -- the ones that reach the largest weights -- set to opacity 1e-4: (their ids, the
    host hierarchy, the device hierarchy, its Scores)."""
    from hgs.importance import score_hierarchy
    h, base = _base()
    leaf = h.nodes[:, 6] == 0
    ids = torch.argsort(torch.where(leaf, base.wmax, torch.full_like(base.wmax, -1.0)), descending=True)[:FAINT].cpu()
    host = cc.hier2000()
    alpha = host.alpha.clone()
    alpha[ids] = 1e-4
    hd = cc.on_device(host, h.nodes.device, alpha=alpha)
    return ids, hd, score_hierarchy(hd, cc.orbit(), tau_px=0.0, frustum=False)


def test_leaf_cut_scores_equal_a_loop_of_score_view_calls(gpu):
    from hgs.importance import Scores, _settings, activated, score_view, tau_of, view_cut
    h, got = _base()
    N = h.num_nodes
    leaf = h.nodes[:, 6] == 0
    assert got.views == 3 and not bool(got.entries[~leaf].any()) and bool((got.entries[leaf] == 3).all())
    assert not bool(got.count[~leaf].any()) and int((got.count[leaf] > 0).sum()) > 1000
    ref = Scores.zeros(N, gpu)
    att = activated(h)
    for cam in cc.orbit():
        ri, pi, w, kids = view_cut(h, cam, tau_of(0.0, cam.tanfovx, cam.image_width), frustum=False)
        assert int(ri.numel()) == int(leaf.sum())                                  # at tau_px = 0 the cut is the leaves
        score_view(ref, _settings(cam, gpu, ri.contiguous(), pi.contiguous(), w.contiguous(), kids.contiguous()), **att)
    torch.cuda.synchronize()
    assert _bits_equal(got, ref)
    # with the cull the same statistics for everything it keeps: it drops only what the rasterizer would not draw
    from hgs.importance import score_hierarchy
    culled = score_hierarchy(h, cc.orbit(), tau_px=0.0, frustum=True)
    assert torch.equal(culled.count, got.count) and torch.equal(culled.wmax, got.wmax) and torch.equal(culled.wsum, got.wsum)
    assert bool((culled.entries <= got.entries).all())


def test_entries_are_the_histogram_of_the_cuts(gpu):
    from hgs.importance import score_hierarchy, tau_of, view_cut
    h, _ = _base()
    N = h.num_nodes
    got = score_hierarchy(h, cc.orbit(), tau_px=3.0, frustum=False)
    hist = torch.zeros(N, dtype=torch.int64, device=gpu)
    for cam in cc.orbit():
        ri = view_cut(h, cam, tau_of(3.0, cam.tanfovx, cam.image_width), frustum=False)[0]
        assert 0 < int(ri.numel()) < 2000
        hist += torch.bincount(ri.long(), minlength=N)
    assert torch.equal(got.entries, hist) and int(hist.max()) == 3
    assert bool((got.entries[h.nodes[:, 6] != 0] > 0).any())                        # interior nodes are in these cuts
    assert not bool(got.count[hist == 0].any())


def test_faint_leaves_are_the_new_marks_and_the_pruner_takes_them(gpu):
    """Fifty leaves at opacity 1e-4 never reach alpha = 1/255: count 0.  Taking them out of the compositing only raises the
    transmittance in front of the others, so no other leaf's largest weight drops: they are exactly the new marks.
    Pruning by the mask removes exactly the marked leaves.

    The pruned hierarchy's scores are compared after pruning by ``pixels_below=1``, the mask of the leaves that blend
    into NO pixel (the fifty among them).  Survivors that a removed leaf overlapped are then no exception: at tau_px = 0
    every entry of the three cuts has interpolation weight exactly 1 (asserted for both hierarchies), so every survivor is
    rendered from its own row, which the pruner copies bit for bit, whatever became of its parent; the removed leaves
    blended nowhere, so every pixel composites the same survivors in the same order with the same transmittances.  An
    instance record does not depend on what else is in its list and a row's run is added in run order: the survivors'
    three statistics are equal BIT FOR BIT.  (Under the weight mask the removed leaves do blend, faintly; what would hold
    there is only ``count`` away from their footprints and from every knife edge, which is weaker than this.)"""
    from hgs.importance import low_contribution_mask, score_hierarchy, tau_of, view_cut
    h, base = _base()
    ids, hd, faint = _faint()
    ids_d = ids.to(gpu)
    assert not bool(faint.count[ids_d].any()) and bool((base.count[ids_d] > 0).all())
    m0 = low_contribution_mask(h.nodes, base, max_weight_below=1 / 255)
    m1 = low_contribution_mask(hd.nodes, faint, max_weight_below=1 / 255)
    assert m1.dtype == torch.uint8 and m1.is_cuda
    new = (m1 != 0) & (m0 == 0)
    assert torch.equal(torch.nonzero(new).flatten(), torch.sort(ids_d).values)
    assert not bool(m1[hd.nodes[:, 6] != 0].any())
    leaf = hd.nodes[:, 6] == 0
    r = hierarchy.prune_hierarchy_gpu(hd, remove=m1)
    marked = m1 != 0
    assert r.removed_leaves == int(marked.sum()) and bool((r.new_of_old[marked] == -1).all())
    assert bool((r.new_of_old[leaf & ~marked] >= 0).all())
    # the leaves that blend nowhere
    m2 = low_contribution_mask(hd.nodes, faint, pixels_below=1)
    gone = m2 != 0
    assert torch.equal(gone, leaf & (faint.count == 0)) and bool(gone[ids_d].all())
    r = hierarchy.prune_hierarchy_gpu(hd, remove=m2)
    assert r.removed_leaves == int(gone.sum())
    for hh in (hd, r.hierarchy):
        for cam in cc.orbit():
            assert bool((view_cut(hh, cam, tau_of(0.0, cam.tanfovx, cam.image_width), frustum=False)[2] == 1.0).all())
    after = score_hierarchy(r.hierarchy, cc.orbit(), tau_px=0.0, frustum=False)
    surv = torch.nonzero(leaf & ~gone).flatten()
    to = r.new_of_old[surv].long()
    assert bool((to >= 0).all()) and int(surv.numel()) > 1000
    assert torch.equal(after.count[to], faint.count[surv])
    assert torch.equal(after.wmax[to].view(torch.int32), faint.wmax[surv].view(torch.int32))
    assert torch.equal(after.wsum[to].view(torch.int64), faint.wsum[surv].view(torch.int64))
    assert bool((after.entries[to] == 3).all())


def test_leaves_a_camera_looks_away_from_are_unseen(gpu):
    from hgs.importance import low_contribution_mask, score_hierarchy
    h, _ = _base()
    cam = fc.yaw_camera((0.0, 0.0, 0.0), 55.0, width=cc.W, height=cc.H)
    s = score_hierarchy(h, [cam], tau_px=0.0, frustum=True)
    leaf = h.nodes[:, 6] == 0
    unseen = leaf & (s.entries == 0)
    assert int(unseen.sum()) > 300 and int((leaf & (s.entries > 0)).sum()) > 300
    assert not bool(s.count[unseen].any())
    keep = low_contribution_mask(h.nodes, s, pixels_below=1, unseen="keep")
    remove = low_contribution_mask(h.nodes, s, pixels_below=1, unseen="remove")
    assert not bool(keep[unseen].any()) and bool((remove[unseen] == 1).all())
    assert torch.equal(remove != 0, (keep != 0) | unseen)
    assert torch.equal(keep != 0, leaf & (s.entries > 0) & (s.count < 1))


def test_command_end_to_end(gpu, tmp_path):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from hgs import score_hierarchy as cmd
    from hgs.importance import low_contribution_mask, score_hierarchy
    ids, hd, _ = _faint()
    host = {k: getattr(hd, k).cpu() for k in cc.FIELDS}
    src = str(tmp_path / "in.hier")
    write_hierarchy(src, *[host[k] for k in cc.FIELDS])
    cams_json = tmp_path / "cameras.json"
    cams_json.write_text(json.dumps([cc.camera_entry(c) for c in cc.orbit()]))
    npz, mask_path, pruned = str(tmp_path / "out" / "scores.npz"), str(tmp_path / "out" / "mask.npy"), str(tmp_path / "p.hier")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    run = lambda *argv: subprocess.run([sys.executable, "-m", *argv], capture_output=True, text=True, env=env, timeout=300)
    r = run("hgs.score_hierarchy", src, npz, "--cameras", str(cams_json), "--no-frustum", "--mask-out", mask_path,
            "--max-weight-below", repr(1 / 255))
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("\n") == 1 and "3 views at 0 px" in r.stdout and "leaves marked" in r.stdout
    # the function on what the command read
    loaded = hierarchy.Hierarchy(*load_hierarchy(src))
    hl = cc.on_device(loaded, gpu, boxes=loaded.boxes.reshape(-1, 2, 4))
    want = score_hierarchy(hl, cmd.read_cameras(str(cams_json)), tau_px=0.0, frustum=False)
    got = np.load(npz)
    for k, v in want.numpy().items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
    assert int(got["views"]) == 3
    mask = np.load(mask_path)
    want_mask = low_contribution_mask(hl.nodes, want, max_weight_below=1 / 255).cpu().numpy()
    assert mask.dtype == np.uint8 and np.array_equal(mask, want_mask) and mask[ids.numpy()].all()
    r = run("hgs.prune_hierarchy", src, pruned, "--mask", mask_path)
    assert r.returncode == 0, r.stderr
    assert f"{int(mask.sum())} leaves removed" in r.stdout
    assert hierarchy.Hierarchy(*load_hierarchy(pruned)).num_nodes < loaded.num_nodes
