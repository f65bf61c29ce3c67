#!/usr/bin/env python
"""Sparse against dense TSDF volumes, one JSON line per case.  The yardstick is the existing
dense path on the same scene and views in the same run; no threshold is fixed.

  dense_512       scripts/bench_tsdf.py's scene (a sphere in front of a plane, 8 orbit cameras at 1920 x 1080, analytic
                  depth maps), its "full" volume of --size^3 samples inside every frustum.  For hgs.meshing.TsdfVolume
                  and hgs.meshing.SparseTsdfVolume alike: integrate with 1 view and with 8 views, each without and with colour;
                  extract (plan, its host wait, the allocation, apply) of the fused volume; the bytes held.  For the
                  sparse volume also the allocation (allocate 8 views + commit, with its host wait), the blocks, the
                  over-allocation |A| / |R| (R by brute force: the blocks holding a sample within one lattice step of a
                  near sample, from a torch statement of the projection over the dense lattice) and the share of the
                  allocated samples some view ever observed (weight > 0).  Before anything is timed, the allocated
                  samples are compared with the dense ones (`differing`: words of tsdf and weight whose bits differ) and
                  the vertex and face counts of the two meshes.
  virtual         a lattice the dense path cannot hold: --virtual samples (default 8192 8192 1024) at a voxel of 0.05
                  around a terrain-like depth set (a rippled ground plane 30 away under the same 8 cameras): blocks,
                  bytes, allocation, integrate and extract times.
  each            --reps alternated repetitions after one warm-up of each, device events around the whole call: median,
                  min and max

    python scripts/bench_sparse_tsdf.py [--size 512] [--reps 15] [--out profiles/f28_sparse_tsdf_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_tsdf import CENTRE, H, SIDE, VIEWS, W, sphere_depth, summary, timed, torch_project   # noqa: E402
from hgs import meshing, synth   # noqa: E402


def alternated(calls, reps, dev):
    for fn in calls.values():                   # warm-up
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            ms[name].append(timed(fn, dev))
    return {k + "_ms": summary(v) for k, v in ms.items()}


def dense_bytes(vol):
    return sum(a.numel() * a.element_size() for a in (vol.tsdf, vol.weight, vol.colour) if a is not None)


def allocated_sparse(lo, hi, voxel, colour, depths, cams, dev):
    return meshing.SparseTsdfVolume(lo, hi, voxel, colour=colour, device=dev).allocate(depths, cams).commit()


def required_blocks(vol, depths, cams):
    """|R| by brute force over the dense lattice (torch): blocks holding a sample within one step of a near sample."""
    near = torch.zeros_like(vol.tsdf, dtype=torch.bool)
    for d, cam in zip(depths, cams):
        ok, z, pix = torch_project(vol, cam)
        dd = d.reshape(-1)[pix]
        sdf = dd - z
        near |= ok & (dd > 0) & (sdf >= -vol.trunc) & (sdf < vol.trunc)
        del ok, z, pix, dd, sdf
    wide = torch.nn.functional.max_pool3d(near[None, None].float(), 3, stride=1, padding=1)
    blocks = torch.nn.functional.max_pool3d(wide, 8, stride=8, ceil_mode=True)
    return int((blocks > 0).sum())


def dense_case(n, cams, depths, images, reps, dev):
    half = 0.5 * SIDE
    lo = (CENTRE[0] - half, CENTRE[1] - half, CENTRE[2] - half)
    voxel = SIDE / (n - 1)
    hi = tuple(l + voxel * (n - 1) + 0.25 * voxel for l in lo)
    dense = lambda colour=False: meshing.TsdfVolume(lo, hi, voxel, colour=colour, device=dev)
    sparse = lambda colour=False: allocated_sparse(lo, hi, voxel, colour, depths, cams, dev)
    # ---- the two paths agree
    dv, sv = dense().integrate(depths, cams), sparse().integrate(depths, cams)
    assert dv.dims == sv.dims == (n, n, n)
    back, allocated = sv.to_dense(return_allocated=True)
    differing = int(((back.tsdf.view(torch.int32) != dv.tsdf.view(torch.int32)) & allocated).sum()
                    + ((back.weight.view(torch.int32) != dv.weight.view(torch.int32)) & allocated).sum())
    del back, allocated
    dm, sm = dv.extract(), sv.extract()
    res = dict(case="dense_512", samples_per_edge=n, samples=n ** 3, views=VIEWS, image=[W, H], reps=reps, differing=differing,
               dense_vertices=int(dm.vertices.shape[0]), sparse_vertices=int(sm.vertices.shape[0]),
               dense_faces=int(dm.faces.shape[0]), sparse_faces=int(sm.faces.shape[0]),
               blocks=sv.n_blocks, grid_blocks=sv.grid[0] * sv.grid[1] * sv.grid[2],
               required_blocks=required_blocks(dv, depths, cams),
               observed_share=round(float((sv.weight[:sv.n_blocks] > 0).float().mean()), 4),
               dense_bytes=dense_bytes(dv), sparse_bytes=sv.nbytes)
    res["over_allocation"] = round(res["blocks"] / max(res["required_blocks"], 1), 3)
    del dm, sm
    dc, sc = dense(True), sparse(True)
    res.update(dense_colour_bytes=dense_bytes(dc), sparse_colour_bytes=sc.nbytes)
    dw, sw = dense(), sparse()
    calls = {
        "dense_v1": lambda: dw.integrate(depths[:1], cams[:1]), "sparse_v1": lambda: sw.integrate(depths[:1], cams[:1]),
        "dense_v8": lambda: dw.integrate(depths, cams), "sparse_v8": lambda: sw.integrate(depths, cams),
        "dense_v1_colour": lambda: dc.integrate(depths[:1], cams[:1], images=images[:1]),
        "sparse_v1_colour": lambda: sc.integrate(depths[:1], cams[:1], images=images[:1]),
        "dense_v8_colour": lambda: dc.integrate(depths, cams, images=images),
        "sparse_v8_colour": lambda: sc.integrate(depths, cams, images=images),
        "dense_extract": lambda: dv.extract(), "sparse_extract": lambda: sv.extract(),
        "sparse_allocate": lambda: sparse(),
    }
    res.update(alternated(calls, reps, dev))
    return res


def terrain_depth(cam, dev):
    """A rippled ground plane about 30 away: the plane z = 30 through the pixel's ray, then a ripple of 1.5."""
    x = ((2.0 * torch.arange(W, dtype=torch.float64, device=dev) + 1.0) / W - 1.0) * cam.tanfovx
    y = ((2.0 * torch.arange(H, dtype=torch.float64, device=dev) + 1.0) / H - 1.0) * cam.tanfovy
    gx, gy = 30.0 * x[None, :].expand(H, W), 30.0 * y[:, None].expand(H, W)
    return (30.0 + 1.5 * torch.sin(0.4 * gx) * torch.cos(0.3 * gy)).float().contiguous()


def virtual_case(dims, cams, reps, dev):
    voxel = 0.05
    lo = (-0.5 * voxel * dims[0], -0.5 * voxel * dims[1], 0.0)
    hi = tuple(l + voxel * (n - 1) + 0.25 * voxel for l, n in zip(lo, dims))
    depths = [terrain_depth(cam, dev) for cam in cams]
    new = lambda: allocated_sparse(lo, hi, voxel, False, depths, cams, dev)
    vol = new().integrate(depths, cams)
    assert vol.dims == tuple(dims)
    mesh = vol.extract()
    res = dict(case="virtual", dims=list(dims), samples=dims[0] * dims[1] * dims[2], voxel=voxel, views=VIEWS, image=[W, H],
               reps=reps, blocks=vol.n_blocks, grid_blocks=vol.grid[0] * vol.grid[1] * vol.grid[2], bytes=vol.nbytes,
               table_bytes=int(vol._table.numel()), vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]),
               observed_share=round(float((vol.weight[:vol.n_blocks] > 0).float().mean()), 4))
    del mesh
    work = new()
    res.update(alternated({"allocate": new, "integrate_v8": lambda: work.integrate(depths, cams),
                           "extract": lambda: vol.extract()}, reps, dev))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--virtual", type=int, nargs=3, default=[8192, 8192, 1024])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cams = [synth.orbit_camera(W, H, k, VIEWS, radius=0.3) for k in range(VIEWS)]
    depths = [sphere_depth(cam, dev) for cam in cams]
    images = [torch.stack((d * 0.2, (d > 0).float() * 0.5, 1.0 - d * 0.2)).contiguous() for d in depths]
    for res in (dense_case(args.size, cams, depths, images, args.reps, dev), virtual_case(args.virtual, cams, args.reps, dev)):
        res["device"] = torch.cuda.get_device_name(dev)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
