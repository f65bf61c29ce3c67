#!/usr/bin/env python
"""TSDF fusion and extraction figures, one JSON line per volume size and placement:

  scene           a sphere (radius 0.6 at depth 3) in front of the plane z = 3.7, seen by 8 orbit cameras at 1920 x 1080,
                  analytic depth maps; the volume is a cube of side 1.6 with --sizes samples per edge, "full": centred
                  on the sphere (inside every frustum), "half": moved sideways until the frustum's edge runs through its
                  middle (`seen` = the share of samples some view's image holds: they are loaded; `updated` = the share
                  some view changes: they are stored -- a sample more than the truncation behind every surface is not)
  integrate       hgs.meshing.TsdfVolume.integrate (hgs_tsdf_integrate) with 1 view and with 8 views per call, and with 8
                  views into a colour volume; against this project's torch statement of the same rule on the same GPU
                  (torch_integrate below: the rule's operations one by one on whole-volume tensors, one view after the
                  other).  Before anything is timed the two volumes are compared (`differing`: words of tsdf and
                  weight whose bits differ, `worst_ulp`; `torch_div_misrounded_of_4M`: quotients of torch's float32
                  division that are not the correctly rounded ones -- the rule's division is, and the GPU tests hold the
                  kernel to the numpy spec bit for bit).
  extract         TsdfVolume.extract (plan, its host wait, the allocation, apply) on the fused "full" volume; against a
                  torch statement of the marking and compaction alone (torch_mark below: observed and inside flags, the
                  active cells, the three quad masks, their nonzero()s) -- it computes no vertex, so it is a lower bound
                  on any torch statement of the whole
  each            --reps alternated repetitions after one warm-up of each, device events around the whole call: median,
                  min and max
  floor_ms        integrate: tsdf and weight (8 bytes; 20 with colour) read once per seen sample and written once per
                  updated sample, at 8 TB/s; extract: tsdf and weight once (8 bytes per sample) plus the outputs;
                  share = floor_ms / the HIP median

    python scripts/bench_tsdf.py [--sizes 256 512] [--reps 15] [--out profiles/f27_tsdf_bench.jsonl]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))

from hgs import meshing, synth   # noqa: E402

PEAK_BYTES_PER_MS = 8.0e9           # 8 TB/s
W, H, VIEWS = 1920, 1080, 8
CENTRE, RADIUS, SIDE, PLANE_Z = (0.0, 0.0, 3.0), 0.6, 1.6, 3.7


def sphere_depth(cam, dev):
    """float32 [H,W]: the view-space depth of the sphere's near side, of the plane behind it elsewhere (float64 inside)."""
    m = cam.world_view_transform.double().to(dev)
    c = torch.tensor(CENTRE, dtype=torch.float64, device=dev) @ m[:3, :3] + m[3, :3]
    x = ((2.0 * torch.arange(W, dtype=torch.float64, device=dev) + 1.0) / W - 1.0) * cam.tanfovx
    y = ((2.0 * torch.arange(H, dtype=torch.float64, device=dev) + 1.0) / H - 1.0) * cam.tanfovy
    d = torch.stack((x[None, :].expand(H, W), y[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64, device=dev)), -1)
    a, b, cc = (d * d).sum(-1), d @ c, c @ c - RADIUS * RADIUS
    disc = b * b - a * cc
    z = (b - disc.clamp(min=0).sqrt()) / a
    n = torch.tensor((0.0, 0.0, 1.0), dtype=torch.float64, device=dev)
    inv = torch.linalg.inv(m[:3, :3])
    plane = (PLANE_Z + n @ (m[3, :3] @ inv)) / (d @ inv @ n)
    return torch.where((disc > 0) & (z > 0), z, plane).float().contiguous()


def torch_project(vol, cam):
    """Steps 1 and 2 on the whole volume -> (ok, z, pixel index)."""
    dev = vol.tsdf.device
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    m = cam.world_view_transform.float().to(dev)
    ax = [f(float(vol.lo[a])) + f(vol.voxel) * torch.arange(n, dtype=torch.float32, device=dev)
          for a, n in enumerate(vol.dims)]
    x0, x1, x2 = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    p = [((x0 * m[0, c] + x1 * m[1, c]) + x2 * m[2, c]) + m[3, c] for c in range(3)]
    z = p[2]
    fx = ((p[0] / (z * f(cam.tanfovx)) + 1.0) * float(W) - 1.0) * 0.5
    fy = ((p[1] / (z * f(cam.tanfovy)) + 1.0) * float(H) - 1.0) * 0.5
    px, py = torch.floor(fx + 0.5), torch.floor(fy + 0.5)
    ok = (z > cam.znear) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    pix = torch.where(ok, py * W + px, torch.zeros_like(px)).long()
    return ok, z, pix


def torch_integrate(vol, depths, cams):
    """The integrate rule (no weight plane, no colour) in torch ops, view after view, into vol.tsdf / vol.weight."""
    for d, cam in zip(depths, cams):
        ok, z, pix = torch_project(vol, cam)
        dd = d.reshape(-1)[pix]
        sdf = dd - z
        ok = ok & (dd > 0) & (sdf >= -vol.trunc)
        # (a tensor divisor: torch turns a division by a Python number into a multiplication by its reciprocal)
        t = torch.clamp(sdf / torch.tensor(vol.trunc, dtype=torch.float32, device=sdf.device), max=1.0)
        Wn = vol.weight + 1.0
        vol.tsdf = torch.where(ok, (vol.weight * vol.tsdf + t) / Wn, vol.tsdf)
        vol.weight = torch.where(ok, torch.clamp(Wn, max=vol.max_weight), vol.weight)


def torch_mark(vol, min_weight=1.0):
    """Marking and compaction alone: -> (active cell indices, the quad edges' indices per axis)."""
    obs, ins = vol.weight >= min_weight, vol.tsdf < 0
    nz, ny, nx = obs.shape
    c = lambda a, s: a[(s >> 2):nz - 1 + (s >> 2), ((s >> 1) & 1):ny - 1 + ((s >> 1) & 1), (s & 1):nx - 1 + (s & 1)]
    all_obs, any_in, all_in = c(obs, 0).clone(), c(ins, 0).clone(), c(ins, 0).clone()
    for s in range(1, 8):
        all_obs &= c(obs, s)
        any_in |= c(ins, s)
        all_in &= c(ins, s)
    active = torch.zeros((nz + 1, ny + 1, nx + 1), dtype=torch.bool, device=obs.device)
    active[1:nz, 1:ny, 1:nx] = all_obs & any_in & ~all_in
    out = [torch.nonzero(active.reshape(-1))]
    sl = lambda lo, n: slice(lo, lo + n)
    for axis, (dk, dj, di) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
        a, b = (slice(0, nz - dk), slice(0, ny - dj), slice(0, nx - di)), (slice(dk, nz), slice(dj, ny), slice(di, nx))
        edge = obs[a] & obs[b] & (ins[a] != ins[b])
        ez, ey, ex = edge.shape
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            o = [0, 0, 0]
            o[u], o[v] = du, dv
            edge &= active[sl(1 + o[2], ez), sl(1 + o[1], ey), sl(1 + o[0], ex)]
        out.append(torch.nonzero(edge.reshape(-1)))
    return out


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def figures(n, placement, cams, depths, images, reps, dev):
    half = 0.5 * SIDE
    # "half": camera 0 stands 0.3 to this side and sees the most of it; 0.62 past the axis' frustum edge half is seen
    shift = 0.0 if placement == "full" else cams[0].tanfovx * CENTRE[2] + 0.62
    lo = (CENTRE[0] + shift - half, CENTRE[1] - half, CENTRE[2] - half)
    voxel = SIDE / (n - 1)
    hi = tuple(l + voxel * (n - 1) + 0.25 * voxel for l in lo)
    new = lambda colour=False: meshing.TsdfVolume(lo, hi, voxel, colour=colour, device=dev)
    vol = new()
    assert vol.dims == (n, n, n), vol.dims
    N = n ** 3
    # ---- the two statements agree; the share of samples the views hold
    ref = new()
    vol.integrate(depths, cams)
    torch_integrate(ref, depths, cams)
    differing = int((vol.tsdf.view(torch.int32) != ref.tsdf.view(torch.int32)).sum()
                    + (vol.weight.view(torch.int32) != ref.weight.view(torch.int32)).sum())
    differing_weights = int((vol.weight.view(torch.int32) != ref.weight.view(torch.int32)).sum())
    ulp = lambda t: (lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i))(t.contiguous().view(torch.int32).long())
    worst_ulp = int((ulp(vol.tsdf) - ulp(ref.tsdf)).abs().max())
    # is torch's float32 division the correctly rounded one?  (the rule's is; a quotient that is not explains `differing`)
    g = torch.Generator(device=dev).manual_seed(1)
    qa, qb = torch.rand(1 << 22, generator=g, device=dev) - 0.5, torch.rand(1 << 22, generator=g, device=dev) + 0.25
    torch_div_misrounded = int(((qa / qb) != (qa.double() / qb.double()).float()).sum())
    del qa, qb
    seen = torch.zeros_like(vol.tsdf, dtype=torch.bool)
    for cam in cams:
        seen |= torch_project(vol, cam)[0]
    seen_1, seen_all = float(torch_project(vol, cams[0])[0].float().mean()), float(seen.float().mean())
    upd_all = float((vol.weight > 0).float().mean())
    first = new()
    first.integrate(depths[:1], cams[:1])
    upd_1 = float((first.weight > 0).float().mean())
    del seen, first
    col = new(True)
    work, twork = new(), new()
    calls = {
        "hip_v1": lambda: work.integrate(depths[:1], cams[:1]),
        "hip_v8": lambda: work.integrate(depths, cams),
        "hip_v8_colour": lambda: col.integrate(depths, cams, images=images),
        "torch_v1": lambda: torch_integrate(twork, depths[:1], cams[:1]),
        "torch_v8": lambda: torch_integrate(twork, depths, cams),
    }
    if placement == "full":
        mesh = vol.extract()
        V, Q = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0]) // 2
        marks = torch_mark(vol)
        marked = (int(marks[0].numel()), sum(int(m.numel()) for m in marks[1:]))
        del mesh, marks
        calls["hip_extract"] = lambda: vol.extract()
        calls["torch_mark"] = lambda: torch_mark(vol)
    for fn in calls.values():                   # warm-up
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):                       # alternated
        for name, fn in calls.items():
            ms[name].append(timed(fn, dev))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = dict(samples_per_edge=n, samples=N, placement=placement, views=VIEWS, image=[W, H], reps=reps,
               seen_by_view_0=round(seen_1, 4), updated_by_view_0=round(upd_1, 4), seen=round(seen_all, 4),
               updated=round(upd_all, 4), differing=differing, differing_weights=differing_weights,
               worst_ulp=worst_ulp, torch_div_misrounded_of_4M=torch_div_misrounded)
    for k, v in ms.items():
        res[k + "_ms"] = summary(v)
    for name, loaded, stored, per in (("hip_v1", seen_1, upd_1, 8), ("hip_v8", seen_all, upd_all, 8),
                                      ("hip_v8_colour", seen_all, upd_all, 20)):
        floor = per * (loaded + stored) * N / PEAK_BYTES_PER_MS
        res[name + "_floor_ms"] = round(floor, 4)
        res[name + "_share"] = round(floor / med[name], 3)
    for v in ("v1", "v8"):
        res[f"speedup_{v}"] = round(med[f"torch_{v}"] / med[f"hip_{v}"], 2)
        res[f"ranges_apart_{v}"] = max(ms[f"hip_{v}"]) < min(ms[f"torch_{v}"])
    if placement == "full":
        floor = (8 * N + 24 * V + 24 * Q) / PEAK_BYTES_PER_MS
        res.update(vertices=V, quads=Q, torch_marked=list(marked), extract_floor_ms=round(floor, 4),
                   extract_share=round(floor / med["hip_extract"], 3),
                   extract_vs_torch_mark=round(med["torch_mark"] / med["hip_extract"], 2),
                   ranges_apart_extract=max(ms["hip_extract"]) < min(ms["torch_mark"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cams = [synth.orbit_camera(W, H, k, VIEWS, radius=0.3) for k in range(VIEWS)]
    depths = [sphere_depth(cam, dev) for cam in cams]
    images = [torch.stack((d * 0.2, (d > 0).float() * 0.5, 1.0 - d * 0.2)).contiguous() for d in depths]
    for n in args.sizes:
        for placement in ("full", "half"):
            res = figures(n, placement, cams, depths, images, args.reps, dev)
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
