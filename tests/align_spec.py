"""The rotation-alignment rule of hgs.hierarchy.align_hierarchy stated with torch ops, on whatever device the hierarchy
lives on (a helper module, not a test): a stable sort of the node ids by depth, then per level a gather of the nodes' and
their parents' quaternions, the 24 candidates as one batched Hamilton product in float64, the first argmax of |dot|,
and a gather of the chosen candidate and scale permutation.  scripts/bench_align.py times it beside the HIP call;
tests/test_hier_align_*.py hold it against the numpy spec and the HIP call."""
import torch

from hgs import hierarchy


def _mul(a, b):
    a0, a1, a2, a3 = a.unbind(-1)
    b0, b1, b2, b3 = b.unbind(-1)
    return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                        a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                        a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                        a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def align_torch(h):
    """In place on ``h.log_scales`` and ``h.rots`` (float32, rows at index >= N untouched); -> h."""
    dev = h.nodes.device
    g, perms = hierarchy.align_group()
    g, perms = torch.from_numpy(g).to(dev), torch.from_numpy(perms).to(dev)
    N = h.nodes.shape[0]
    depth, parent = h.nodes[:, 0].long(), h.nodes[:, 1].long()
    order = torch.argsort(depth, stable=True)
    counts = torch.bincount(depth, minlength=1).tolist()          # the one host wait
    first = counts[0]
    for n in counts[1:]:
        ids = order[first:first + n]
        first += n
        q32 = h.rots[ids]
        p = h.rots[parent[ids]].double()
        c = _mul(q32.double()[:, None, :], g[None])                                           # [n,24,4]
        d = c[..., 0] * p[:, None, 0] + c[..., 1] * p[:, None, 1] + c[..., 2] * p[:, None, 2] + c[..., 3] * p[:, None, 3]
        j = d.abs().argmax(1)                                                                 # the first maximum
        neg = d.gather(1, j[:, None]) < 0
        best = c.gather(1, j[:, None, None].expand(-1, 1, 4))[:, 0]
        best = torch.where(neg, -best, best).float()
        best = torch.where((j == 0)[:, None], torch.where(neg, -q32, q32), best)
        h.rots[ids] = best
        h.log_scales[ids] = h.log_scales[ids].gather(1, perms[j])
    return h
