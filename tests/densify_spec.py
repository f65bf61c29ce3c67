"""The yardstick of hgs.densify (test infrastructure; the product never imports it): adaptive density control stated in
whole-array float32 torch ops, device-agnostic.  Written from the rule of DESIGN.md section 7 f-8, not transcribed from
the reference's method chain; tests/golden/ref_densify_golden.npz pins it to the reference's own code on the CPU, and
on the GPU it stands in for the reference (values, and the baseline of scripts/bench_densify.py).

Per row r of P, F protected leading rows, tau = max_grad, d = percent_dense * extent:
    g = accum (NaN -> 0);  o = sigmoid(opacity);  m = max_k exp(scaling_k);  w = max_radii2D * o^(1/5)
    clone = (|g| w >= tau) and (o > 0.15) and (m <= d) and (r >= F)
    split = ( g  w >= tau) and (o > 0.15) and (m >  d) and (r >= F)
    low   = o < min_opacity
Output rows, each block in ascending r: originals with not split and not (low and r >= F); clones with not low; child 0
of splits with not low; child 1 of the same rows.  The k-th split row owns noise rows z[k] and z[S + k]."""
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def classes(accum, radii, opacity, scaling, F, max_grad, min_opacity, d):
    """-> boolean [P] masks clone, split, low, open (r >= F)."""
    P = opacity.shape[0]
    g = torch.nan_to_num(accum.reshape(P), nan=0.0, posinf=float("inf"), neginf=float("-inf"))
    o = torch.sigmoid(opacity.reshape(P))
    m = torch.exp(scaling).max(dim=1).values if P else scaling.new_zeros(0)
    w = radii.reshape(P) * torch.pow(o, 1 / 5.0)
    is_open = torch.arange(P, device=opacity.device) >= (F or 0)
    hot = o > 0.15
    clone = (g.abs() * w >= max_grad) & hot & (m <= d) & is_open
    split = (g * w >= max_grad) & hot & (m > d) & is_open
    low = o < min_opacity
    return clone, split, low, is_open


def rotation_matrix(q):
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q.unbind(dim=1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def densify_and_prune_spec(tensors, moments, accum, radii, F, max_grad, min_opacity, d, noise=None, generator=None):
    """The arguments and the result of hgs.densify.densify_and_prune_tensors."""
    if not max_grad > 0:
        raise ValueError("max_grad must be positive")
    moments = moments or {}
    clone, split, low, is_open = classes(accum, radii, tensors["opacity"], tensors["scaling"], F, max_grad, min_opacity, d)
    keep_orig = ~split & ~(low & is_open)
    keep_clone = clone & ~low
    keep_split = split & ~low
    S = int(split.sum())
    dev = tensors["xyz"].device
    if noise is None:
        noise = torch.randn((2 * S, 3), generator=generator, device=dev, dtype=torch.float32)
    if tuple(noise.shape) != (2 * S, 3):
        raise ValueError(f"noise has shape {tuple(noise.shape)}; ({2 * S},3) expected")
    kept_of_split = keep_split[split]                 # over the S split rows, in ascending r
    z = (noise[:S][kept_of_split], noise[S:][kept_of_split])
    sigma = torch.exp(tensors["scaling"][keep_split])
    R = rotation_matrix(tensors["rotation"][keep_split])
    out, out_m = {}, {}
    for n in NAMES:
        t = tensors[n]
        base, cl, sp = t[keep_orig], t[keep_clone], t[keep_split]
        if n == "xyz":
            kids = [sp + (R * (sigma * zj)[:, None, :]).sum(dim=2) for zj in z]
        elif n == "scaling":
            kids = [torch.log(sigma / 1.6)] * 2
        else:
            kids = [sp, sp]
        out[n] = torch.cat([base, cl] + kids, dim=0)
        mv = moments.get(n)
        if mv is None:
            out_m[n] = None
        else:
            new = out[n].shape[0] - base.shape[0]
            out_m[n] = tuple(torch.cat([m[keep_orig], m.new_zeros((new,) + tuple(m.shape[1:]))], dim=0) for m in mv)
    totals = (int(keep_orig.sum()), int(keep_clone.sum()), S, int(keep_split.sum()))
    return out, out_m, totals


def threshold_distance(accum, radii, opacity, scaling, max_grad, min_opacity, d):
    """float64 [P]: every row's smallest relative distance to any of the four thresholds (|g| w against tau, o against
    0.15 and min_opacity, m against d).  The contract lets a row within 1e-5 of one take either class; tests keep every
    row at 1e-4 or more."""
    P = opacity.shape[0]
    g = torch.nan_to_num(accum.reshape(P).double(), nan=0.0)
    o = torch.sigmoid(opacity.reshape(P).double())
    m = torch.exp(scaling.double()).max(dim=1).values
    v = g.abs() * radii.reshape(P).double() * o.pow(0.2)
    rel = lambda a, t: (a - t).abs() / abs(t) if t != 0 else torch.full_like(a, float("inf"))
    return torch.stack([rel(v, max_grad), rel(o, 0.15), rel(o, min_opacity), rel(m, d)]).min(dim=0).values
