"""VRAM-budgeted residency of a hierarchy's attribute rows ("VRAM-budgeted streaming LOD", BASELINE configs[4]; the
``--budget <MB>`` of the reference's hierarchy viewer, README.md:233-235, whose implementation is in the un-vendored
SIBR viewer).  Opt-in, beside the drop-in path: ``render_hierarchy.py`` itself loads the whole hierarchy onto the GPU
(scene/gaussian_model.py:329,376-399) and so does ``bench.py``'s configs[4] loop -- 15 GB of 288 GB.

The full attributes live in pinned host memory that the GPU can read directly, as ONE PACKED ROW of 64 floats per
Gaussian (SH, rotation, mean, scale, opacity: 4 (3 M + 11) useful bytes in 256 -- four 64-byte PCIe reads per row instead
of seven from five separate arrays); the GPU holds ``budget`` rows in slot arrays plus one int32 per Gaussian (its
slot, or "absent").  Per view::

    sel = bh.select(nodes, boxes, tau, viewpoint_gpu, viewpoint_cpu)   # cut, weights, residency; raises tau if needed
    rs  = GaussianRasterizationSettings(..., render_indices=sel.render_indices, parent_indices=sel.parent_indices,
                                        interpolation_weights=sel.weights, num_node_kids=sel.kids)
    GaussianRasterizer(rs)(means3D=bh.means3D, shs=bh.shs, opacities=bh.opacities, scales=bh.scales,
                           rotations=bh.rotations, means2D=...)

``select`` runs the reference's two LOD calls (``expand_to_size`` / ``get_interpolation_weights``), marks the rows the
cut needs (the node row of every entry, and its parent row unless the entry's weight is exactly 1 -- the in-op LOD gather
does not read that parent), fetches the missing ones over PCIe with ONE kernel that reads the host
arrays itself (no host-side gather, no staging buffer), recycles the slots that have gone unused for the longest when the
free list runs out, and returns the cut's indices translated to slots.  A view whose rows do not fit the budget is cut
again at a coarser granularity (tau x 1.2 per attempt, x 1.05 once the cut is within a tenth of the budget), as the
reference's viewer "auto-regulates and raises the granularity until the scene can fit inside the defined VRAM budget".
The rasterizer's in-op LOD path runs on the slot arrays unchanged: rows are rows.

``prefetch(nodes, boxes, tau, next_viewpoint_gpu, next_viewpoint_cpu)``, called once the CURRENT view's render has been
enqueued, runs the NEXT view's cut, weights and residency on a second stream while the render occupies the first: the rows
a camera jump needs (1.4 M rows = 360 MB over PCIe in the 50 M-node fly-through) cross the bus under the previous frame
instead of in front of the next one, and ``select`` for that viewpoint reuses the prefetched cut.

``select(..., frustum=(planes, radius_scale))`` / ``prefetch(..., frustum=...)`` (the pair of hgs.frustum.frustum_planes): the
cut, every retry of the regulator and the prefetch drop the entries the view cannot draw (hgs.frustum.cut_view), so rows
beside and behind the camera are neither fetched nor held and the budget goes to a finer cut of what is in view.

``select(..., fit="budget")`` / ``prefetch(..., fit="budget")`` replace the regulator's search by ONE
``hgs.frustum.cut_to_budget(tau_min=tau, budget=B, cost="rows")``: the finest granularity at or above the request whose
rows fit the budget is selected on the device from the node sizes ("Budget-exact cut"), so
``make_resident`` runs once, nothing is retried and ``Selection.tau`` does not depend on the views before.  It needs a
hierarchy whose boxes nest; the default ``fit="regulate"`` is the path described above.

``rows="half"`` (constructor, ``from_hier_file``, ``from_device_arrays``) keeps the host rows in the 128-byte half layout
of include/hgs.h (HGS_RESID_HOST_ROW_BYTES_HALF: SH, rotation, scale and opacity as IEEE half, the mean as float32): half
the pinned memory and two 64-byte PCIe reads per row instead of four.  The fetch kernel widens the rows into the same
float32 slot arrays, so everything behind the slots -- and the number of rows a budget buys -- is unchanged; what the
viewer sees is ``round_rows_to_half`` of the attributes.  ``pack_rows_half`` is the layout's specification in numpy.

``slots="half"`` (same three places; needs ``rows="half"``) keeps the SLOT arrays in half precision too: the fetch kernel
copies the bits of the host row (hgs_resid_fetch_half_slots) -- SH, rotation, scale and opacity stay IEEE half
(``bh.shs`` ... are ``torch.float16``), the mean float32 -- and the rasterizer's in-op LOD path widens them in registers
(hgs_raster_args.lod_half_rows).  A slot then costs ``6 M + 28`` bytes instead of ``4 (3 M + 11)`` -- 124 against 236 at
M = 16 -- so the same ``budget_mb`` buys 1.90 times the rows, which ``fit="budget"`` and the regulator turn into a finer
cut.  Nothing is lost against ``rows="half"`` with float slots: widening a half is exact and the interpolation stays in
float32, so at an equal ROW budget the two render the same image bit for bit.  Forward only (a viewer's path): the
tensors are handed to ``GaussianRasterizer`` as they are, without gradients."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib


def _host_array(shape, dtype=np.float32):
    """A numpy array over pinned, device-mapped host memory (hgs_host_alloc) and the owner that frees it."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = _lib.lib().hgs_host_alloc(n)
    if not p:
        raise RuntimeError(f"cannot allocate {n} bytes of pinned host memory")
    buf = (C.c_char * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    return arr, p


HOST_ROW_BYTES = {"float": 4 * _lib.RESID_HOST_ROW_FLOATS, "half": _lib.RESID_HOST_ROW_BYTES_HALF}
HALF_MAX = 65504.0


def narrow_to_half(a) -> np.ndarray:
    """float32 -> IEEE half bits (uint16) under the narrowing rule of include/hgs.h: round to nearest even with subnormal
    halves kept; a finite value beyond +-65504 becomes +-65504; NaN becomes 0x7e00 under its sign; an infinity stays."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        bits = np.where(np.isfinite(a), np.clip(a, -HALF_MAX, HALF_MAX), a).astype(np.float16).view(np.uint16).copy()
    nan = np.isnan(a)
    bits[nan] = ((a.view(np.uint32)[nan] >> 16) & 0x8000).astype(np.uint16) | np.uint16(0x7E00)
    return bits


def widen_half(bits) -> np.ndarray:
    """IEEE half bits (uint16) -> float32, exact."""
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32)


def _as_rows(means3D, shs, opacities, scales, rotations):
    """The five attribute arrays (numpy or CPU tensors, float32) as 2-D float32 numpy arrays [G,3], [G,3M], [G,1], [G,3],
    [G,4]; ValueError on another dtype or shape."""
    _check_arrays(means3D, shs, opacities, scales, rotations, on_gpu=False)
    G = int(means3D.shape[0])
    a = lambda t: np.ascontiguousarray((t.detach() if torch.is_tensor(t) else t).reshape(G, -1))
    return tuple(np.asarray(a(t)) for t in (means3D, shs, opacities, scales, rotations))


def pack_rows_half(means3D, shs, opacities, scales, rotations) -> np.ndarray:
    """The half host rows of include/hgs.h (HGS_RESID_HOST_ROW_BYTES_HALF) as uint8 [G, 128] -- the specification of the
    layout, in numpy: halves [0, 3 M) SH in the slot array's order, [48, 52) rotation, [52, 55) scale, [55] opacity, then
    the mean as three float32 at bytes 112..123; padding is zero.  Inputs: numpy arrays or CPU tensors, float32,
    activated as the rasterizer takes them."""
    m, sh, op, sc, rot = _as_rows(means3D, shs, opacities, scales, rotations)
    G = m.shape[0]
    out = np.zeros((G, HOST_ROW_BYTES["half"]), np.uint8)
    halves = out[:, :112].view(np.uint16)
    halves[:, :sh.shape[1]] = narrow_to_half(sh)
    halves[:, 48:52] = narrow_to_half(rot)
    halves[:, 52:55] = narrow_to_half(sc)
    halves[:, 55:56] = narrow_to_half(op)
    out[:, 112:124] = m.view(np.uint8)
    return out


def round_rows_to_half(means3D, shs, opacities, scales, rotations):
    """The five arrays as a ``rows="half"`` viewer sees them: every value but the mean narrowed to half and widened again.
    Shapes are kept; tensors in, CPU tensors out (numpy in, numpy out)."""
    arrays = (means3D, shs, opacities, scales, rotations)
    rows = _as_rows(*arrays)
    out = []
    for k, (t, r) in enumerate(zip(arrays, rows)):
        r = (r.copy() if k == 0 else widen_half(narrow_to_half(r))).reshape(tuple(t.shape))
        out.append(torch.from_numpy(r) if torch.is_tensor(t) else r)
    return tuple(out)


def _check_rows(rows):
    if rows not in HOST_ROW_BYTES:
        raise ValueError(f"rows must be 'float' or 'half', not {rows!r}")


def _check_slots(slots, rows):
    if slots not in ("float", "half"):
        raise ValueError(f"slots must be 'float' or 'half', not {slots!r}")
    if slots == "half" and rows != "half":
        raise ValueError("slots='half' needs rows='half': the fetch copies the half host row's bits into the slot, and "
                         "narrowing float host rows on fetch is not part of it")


def _check_arrays(means3D, shs, opacities, scales, rotations, on_gpu):
    """ValueError unless the five arrays are float32, agree on G, have the rasterizer's shapes and live where the
    constructor expects them (``on_gpu``); nothing here touches the device.  -> (G, M)"""
    named = dict(means3D=means3D, shs=shs, opacities=opacities, scales=scales, rotations=rotations)
    for k, t in named.items():
        if on_gpu and not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{k}: from_device_arrays takes GPU tensors (host arrays go to BudgetedHierarchy(...))")
        if not on_gpu and torch.is_tensor(t) and t.is_cuda:
            raise ValueError(f"{k}: a GPU tensor; this constructor copies CPU tensors (GPU tensors go to "
                             f"BudgetedHierarchy.from_device_arrays)")
        if not (torch.is_tensor(t) or isinstance(t, np.ndarray)):
            raise ValueError(f"{k}: a tensor is expected, not {type(t).__name__}")
        if t.dtype not in (torch.float32, np.float32):
            raise ValueError(f"{k}: float32 expected, not {t.dtype}")
    if means3D.ndim != 2 or means3D.shape[1] != 3:
        raise ValueError(f"means3D: [G,3] expected, not {tuple(means3D.shape)}")
    G = int(means3D.shape[0])
    if shs.ndim != 3 or shs.shape[0] != G or shs.shape[2] != 3 or not 1 <= shs.shape[1] <= 16:
        raise ValueError(f"shs: [{G},M,3] with M in 1..16 expected, not {tuple(shs.shape)}")
    for k, shape in (("opacities", ((G,), (G, 1))), ("scales", ((G, 3),)), ("rotations", ((G, 4),))):
        if tuple(named[k].shape) not in shape:
            raise ValueError(f"{k}: {' or '.join(str(list(x)) for x in shape)} expected, not {tuple(named[k].shape)}")
    return G, int(shs.shape[1])


class _CutBuffers:
    """Index / weight buffers of one cut (Gaussian rows in, slots out)."""

    def __init__(self, cap, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        self.ri = torch.zeros(cap, **i32); self.pi = torch.zeros(cap, **i32); self.ni = torch.zeros(cap, **i32)
        self.ro = torch.zeros(cap, **i32); self.po = torch.zeros(cap, **i32)
        self.w = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.ns = torch.zeros(cap, **i32)


@dataclass
class Selection:
    """What one view renders.  The index / weight tensors are views of buffers the BudgetedHierarchy owns: valid until
    its next ``select`` / ``make_resident`` (enqueue the render first -- stream order does the rest; a ``prefetch`` in
    between writes the other set of buffers)."""
    n: int                              # entries of the cut
    tau: float                          # the granularity that was rendered (>= the requested one)
    render_indices: torch.Tensor        # int32 [n]: SLOT of the node row
    parent_indices: torch.Tensor        # int32 [n]: SLOT of the parent row
    weights: torch.Tensor               # f32 [>= n]
    kids: torch.Tensor                  # int32 [>= n]
    misses: int                         # rows fetched for this view
    attempts: int                       # cuts tried (1 = the requested granularity fitted)
    cost: int = 0                       # fit="budget": rows the cut was counted at (entries + parent rows, <= budget)


class BudgetedHierarchy:
    def __init__(self, means3D, shs, opacities, scales, rotations, device, budget_mb: Optional[float] = None,
                 budget_rows: Optional[int] = None, index_capacity: Optional[int] = None, rows: str = "float",
                 slots: str = "float"):
        """The five attribute arrays as CPU tensors ([G,3], [G,M,3], [G] or [G,1], [G,3], [G,4], float32, already in the
        form the rasterizer takes: activated).  They are COPIED into pinned host memory.  ``budget_mb``: megabytes of
        GPU memory for the attribute rows (the reference's ``--budget``); or ``budget_rows`` directly.  ``rows``:
        ``"float"`` -- 256-byte host rows -- or ``"half"`` -- 128-byte host rows (module docstring).  ``slots``:
        ``"float"`` -- float32 slot arrays, 4 (3 M + 11) bytes a row -- or, with ``rows="half"``, ``"half"`` -- the slots
        keep the halves, 6 M + 28 bytes a row: the same budget buys 1.90 times the rows at M = 16."""
        _check_rows(rows)
        _check_slots(slots, rows)
        G, M = _check_arrays(means3D, shs, opacities, scales, rotations, on_gpu=False)
        self._setup(G, M, device, budget_mb, budget_rows, index_capacity, rows, slots)
        if rows == "half":
            step = 1 << 20              # narrowed block by block: no second copy of the whole hierarchy
            for a in range(0, G, step):
                self._rows[a:a + step] = pack_rows_half(*[t[a:a + step] for t in (means3D, shs, opacities, scales, rotations)])
            return
        f = lambda t, shape: t.detach().to("cpu", torch.float32).reshape(shape).numpy()
        r = self._rows
        r[:, :3 * M] = f(shs, (G, 3 * M))
        r[:, 3 * M:48] = 0.0
        r[:, 48:52] = f(rotations, (G, 4))
        r[:, 52:55] = f(means3D, (G, 3))
        r[:, 55:58] = f(scales, (G, 3))
        r[:, 58] = f(opacities, (G,))
        r[:, 59:] = 0.0

    def _setup(self, G, M, device, budget_mb, budget_rows, index_capacity, rows, slots="float"):
        """Everything but the contents of the host rows: the pinned rows, the slot arrays, the bookkeeping."""
        self.dev = torch.device(device)
        self.lib = _lib.lib()
        self.G, self.M = G, M
        self.rows_format, self.slots_format = rows, slots
        # bytes of a row in the SLOT arrays -- what a budget is counted in: five float32 arrays, or halves beside a float32 mean
        self.row_bytes = 6 * M + 28 if slots == "half" else 4 * (3 * M + 11)
        self.host_row_bytes = HOST_ROW_BYTES[rows]          # bytes of a row in pinned host memory, and over PCIe
        if budget_rows is None:
            if budget_mb is None:
                raise ValueError("budget_mb or budget_rows")
            budget_rows = int(budget_mb * 1e6 // self.row_bytes)
        self.B = B = max(1, min(int(budget_rows), G))
        assert 3 * M <= 48
        # the packed host rows (include/hgs.h): float32 [G, 64] or, rows="half", bytes [G, 128]
        if rows == "half":
            self._rows, self._rows_ptr = _host_array((G, self.host_row_bytes), np.uint8)
            self._fetch, self._fetch_name = self.lib.hgs_resid_fetch_half, "hgs_resid_fetch_half"
            if slots == "half":
                self._fetch, self._fetch_name = self.lib.hgs_resid_fetch_half_slots, "hgs_resid_fetch_half_slots"
        else:
            self._rows, self._rows_ptr = _host_array((G, _lib.RESID_HOST_ROW_FLOATS))
            self._fetch, self._fetch_name = self.lib.hgs_resid_fetch, "hgs_resid_fetch"
        f32 = dict(dtype=torch.float32, device=self.dev)
        att = dict(dtype=torch.float16 if slots == "half" else torch.float32, device=self.dev)
        self.means3D = torch.zeros(B, 3, **f32)
        self.shs = torch.zeros(B, M, 3, **att)
        self.opacities = torch.zeros(B, 1, **att)
        self.scales = torch.ones(B, 3, **att)
        self.rotations = torch.zeros(B, 4, **att)
        self.rotations[:, 0] = 1.0
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.slot_of = torch.full((G,), -1, **i32)
        self.id_of_slot = torch.full((B,), -1, **i32)
        self.stamp = torch.zeros(B, **i32)
        self.free_list = torch.arange(B - 1, -1, -1, **i32)
        self.free_top = B
        self.counters = torch.zeros(_lib.RESID_COUNTER_WORDS, **i32)
        cap = int(index_capacity or G)
        # two sets of cut buffers: the view being rendered reads one (its Selection aliases it), ``prefetch`` fills the other
        self._sets = [_CutBuffers(cap, self.dev), _CutBuffers(cap, self.dev)]
        self._cur = 0
        self.miss_ids = torch.zeros(2 * cap, **i32)
        self.frame = 0
        self._side = None               # the prefetch stream (created on first use)
        self._resid_done = None         # event: the residency kernels of the last select are enqueued (before its render)
        self._prefetch_done = None      # event: the last prefetch has finished on the side stream
        self._prefetched = None         # (viewpoint + frustum key, tau, t, (n, culled), fit, cost) of the cut waiting in the other buffer set
        self._regulated = None          # granularity the previous view was coarsened to (None: the request fitted)
        self._skip_batch = 0            # evictions left that skip the batch attempt (it failed recently)
        self._since_probe, self.probe_every = 0, 16
        self.stats = dict(views=0, rows_fetched=0, bytes_fetched=0, evictions=0, retries=0, entries_culled=0)
        self._bounds = None             # (key of the node list, float32 [N,4] culling balls): built on first frustum use
        self.profile_fetch = False      # True: (rows, start event, end event) of every fetch launch -> self.fetch_events
        self.fetch_events = []
        self._slot_rows = (_lib.ResidRowsHalf if slots == "half" else _lib.ResidRows)(
            *[C.c_void_p(t.data_ptr()) for t in (self.means3D, self.shs, self.opacities, self.scales, self.rotations)])

    @classmethod
    def from_device_arrays(cls, means3D, shs, opacities, scales, rotations, *, rows: str = "float",
                           slots: str = "float", budget_mb: Optional[float] = None, budget_rows: Optional[int] = None,
                           index_capacity: Optional[int] = None):
        """The constructor for attributes that are already on the GPU (a hierarchy built or merged there): float32 GPU
        tensors of the constructor's shapes, on one device.  The host rows are written by a kernel through the mapped
        pointer (hgs_resid_pack_rows) in either format -- the same bytes the constructor writes -- and no float copy of
        the attributes is made on the host.  ``slots``: as in the constructor."""
        _check_rows(rows)
        _check_slots(slots, rows)
        G, M = _check_arrays(means3D, shs, opacities, scales, rotations, on_gpu=True)
        dev = means3D.device
        if any(t.device != dev for t in (shs, opacities, scales, rotations)):
            raise ValueError("from_device_arrays: the five tensors must live on one device")
        self = cls.__new__(cls)
        self._setup(G, M, dev, budget_mb, budget_rows, index_capacity, rows, slots)
        src = [t.detach().contiguous() for t in (means3D, shs, opacities, scales, rotations)]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _lib.check(self.lib.hgs_resid_pack_rows(C.byref(_lib.ResidRows(*[C.c_void_p(t.data_ptr()) for t in src])), G, M,
                                                    int(rows == "half"), C.c_void_p(self._rows_ptr),
                                                    C.c_void_p(stream.cuda_stream), dev.index or 0), "hgs_resid_pack_rows")
            stream.synchronize()        # the host reads the rows (culling balls) and ``src`` may be freed
        return self

    @classmethod
    def from_hier_file(cls, path: str, device, budget_mb: Optional[float] = None, budget_rows: Optional[int] = None,
                       rows: str = "float", slots: str = "float"):
        """A ``.hier`` file (gaussian_hierarchy._C.load_hierarchy, scene/gaussian_model.py:329) straight into the
        budgeted form, with the activations the reference applies to a loaded hierarchy: opacity = |alpha|
        (scene/gaussian_model.py:393), scales = exp(log-scales), rotations normalised (scene/gaussian_model.py:108-116).
        Returns (BudgetedHierarchy, nodes, boxes) with nodes / boxes on ``device`` (they stay resident: 60 B per node).
        ``rows="half"``: 128-byte host rows, narrowed from the ACTIVATED values (a file written with ``half=True`` stores
        log-scales as halves; its activated scales are narrowed once more here).  ``slots``: as in the constructor."""
        from gaussian_hierarchy._C import load_hierarchy
        _check_rows(rows)
        _check_slots(slots, rows)
        xyz, shs, alpha, log_scales, rots, nodes, boxes = load_hierarchy(path)
        bh = cls(xyz, shs, alpha.abs(), torch.exp(log_scales), torch.nn.functional.normalize(rots), device,
                 budget_mb=budget_mb, budget_rows=budget_rows, rows=rows, slots=slots)
        return bh, nodes.to(device), boxes.to(device)

    def __del__(self):
        try:
            p = getattr(self, "_rows_ptr", None)
            if p:
                self._rows = None
                self.lib.hgs_host_free(C.c_void_p(p))
                self._rows_ptr = None
        except Exception:
            pass

    # ---------------------------------------------------------------------------------------------------------------
    @property
    def budget_bytes(self):
        return self.B * self.row_bytes

    @property
    def resident_rows(self):
        return self.B - self.free_top

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    # the CURRENT set's buffers under their old names (tests and callers read them)
    ri = property(lambda s: s._sets[s._cur].ri)
    pi = property(lambda s: s._sets[s._cur].pi)
    ni = property(lambda s: s._sets[s._cur].ni)
    ro = property(lambda s: s._sets[s._cur].ro)
    po = property(lambda s: s._sets[s._cur].po)
    w = property(lambda s: s._sets[s._cur].w)
    ns = property(lambda s: s._sets[s._cur].ns)

    def make_resident(self, render_indices: torch.Tensor, parent_indices: torch.Tensor,
                      weights: Optional[torch.Tensor] = None, _bufs=None, _new_frame=True, _best_effort=False):
        """Rows of a cut (int32 GPU tensors of Gaussian rows, equal length) -> (slots of the node rows, slots of the
        parent rows, rows fetched).  ``weights`` (float32 GPU tensor, one interpolation weight per entry, optional): the
        parent row of an entry of weight exactly 1 is not read by the rasterizer's in-op LOD gather and is therefore
        neither fetched nor stamped -- its slot is reported as the node's own.  Raises _lib.HgsError with code
        HGS_ERR_CAPACITY when the rows do not fit the budget."""
        n = int(render_indices.numel())
        bufs = self._sets[self._cur] if _bufs is None else _bufs
        ro_buf, po_buf = bufs.ro, bufs.po
        assert parent_indices.numel() >= n and n <= ro_buf.numel()
        if weights is not None:
            assert weights.is_cuda and weights.dtype == torch.float32 and weights.is_contiguous() and weights.numel() >= n
        p, dev_i, s = _lib.ptr, self.dev.index or 0, self._stream()
        if _new_frame:                  # (a prefetch stamps with the frame being rendered: its rows are protected with it)
            self.frame += 1
        miss = C.c_uint32(0)

        def unqueue(first=0):
            # the rows queued by the mark pass (slot_of = -2) go back to "absent" (from entry `first` of the miss list on)
            k = int(miss.value)
            if k > first:
                ids = self.miss_ids[first:k].long()
                self.slot_of[ids] = torch.where(self.slot_of[ids] == -2, torch.full_like(self.slot_of[ids], -1),
                                                self.slot_of[ids])

        try:
            _lib.check(self.lib.hgs_resid_mark(p(render_indices), p(parent_indices), p(weights), n, self.G, p(self.slot_of),
                                               p(self.stamp), self.frame, p(self.miss_ids), p(self.counters), p(ro_buf),
                                               p(po_buf), C.byref(miss), s, dev_i), "hgs_resid_mark")
        except _lib.HgsError:
            unqueue()                   # a bad index is reported after the valid rows of the cut were queued
            raise
        m = int(miss.value)
        if m:
            if m > 4096:
                # slots are handed out in miss-list order: sorted by row, a bulk fetch (cold start, a jump of the camera)
                # lays the rows out in the hierarchy's own order and K1's gathers stay as local as on the full arrays
                self.miss_ids[:m] = torch.sort(self.miss_ids[:m]).values
            try:
                if m > self.free_top:
                    # An eviction costs two passes over the slots and two host round trips: free a batch (1 / 32 of
                    # the budget) beyond what this view needs, so that a camera in motion evicts every few frames
                    # instead of on every frame; if that many old rows do not exist, exactly what is needed.
                    # A view whose working set nearly fills the budget has no such batch to give: after a failed
                    # batch attempt the next 16 evictions ask for exactly what they need (one pass, one round trip).
                    batch = max(m, min(self.B, m + self.B // 32))
                    if self._skip_batch > 0:
                        self._skip_batch -= 1
                        batch = m
                    # best effort (a prefetch: the rows of the view being rendered carry this frame's stamp and stay): what
                    # cannot be freed is left to the next select
                    tries = (batch, m) if not _best_effort else (m, max(1, m // 2), max(1, m // 4), max(1, m // 8))
                    for need in dict.fromkeys(tries):
                        top = C.c_uint32(self.free_top)
                        rc = self.lib.hgs_resid_evict(p(self.stamp), p(self.id_of_slot), p(self.slot_of), self.B,
                                                      self.frame, need, p(self.free_list), p(self.counters),
                                                      C.byref(top), s, dev_i)
                        if rc == _lib.ERR_CAPACITY and (need > m or _best_effort):
                            if not _best_effort:
                                self._skip_batch = 16
                            continue
                        _lib.check(rc, "hgs_resid_evict")
                        break
                    self.stats["evictions"] += int(top.value) - self.free_top
                    self.free_top = int(top.value)
                if _best_effort and m > self.free_top:
                    # The mark pass queues rows in the order its atomics complete.  A pass that can only bring in PART of
                    # the list takes the lowest rows, not whichever were queued first: which rows are resident afterwards
                    # (and so what later views fetch and evict) is then a function of the views alone.
                    if m <= 4096:
                        self.miss_ids[:m] = torch.sort(self.miss_ids[:m]).values
                    unqueue(self.free_top)
                    m = self.free_top
                    if m == 0:
                        return None, None, 0
                if self.profile_fetch:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                _lib.check(self._fetch(p(self.miss_ids), m, p(self.free_list), self.free_top, p(self.slot_of),
                                       p(self.id_of_slot), p(self.stamp), self.frame, C.c_void_p(self._rows_ptr),
                                       C.byref(self._slot_rows), self.M, s, dev_i), self._fetch_name)
                if self.profile_fetch:
                    e1.record()
                    self.fetch_events.append((m, e0, e1))
            except _lib.HgsError:
                unqueue()
                raise
            self.free_top -= m
            if _best_effort and m < int(miss.value):
                self.stats["rows_fetched"] += m
                self.stats["bytes_fetched"] += m * self.host_row_bytes
                return None, None, m            # (part of the view is still missing: no slot indices)
            _lib.check(self.lib.hgs_resid_remap(p(render_indices), p(parent_indices), p(weights), n, p(self.slot_of),
                                                p(ro_buf), p(po_buf), s, dev_i), "hgs_resid_remap")
            self.stats["rows_fetched"] += m
            self.stats["bytes_fetched"] += m * self.host_row_bytes
        return ro_buf[:n], po_buf[:n], m

    @staticmethod
    def _vp_key(viewpoint_cpu, frustum=None):
        key = tuple(float(x) for x in viewpoint_cpu.reshape(-1)[:3])
        if frustum is not None:         # a prefetched cut is only reused under the frustum it was culled with
            key += tuple(float(x) for x in torch.as_tensor(frustum[0]).reshape(-1)) + (float(frustum[1]),)
        return key

    def _cull_bounds(self, nodes):
        """The culling balls of ``nodes`` (hgs.frustum.cull_bounds) from the constructor's arrays: computed once, on the
        first use of a frustum; the means and scales are uploaded for that one launch and freed."""
        key = (nodes.data_ptr(), int(nodes.shape[0]), nodes._version)
        if self._bounds is None or self._bounds[0] != key:
            from .frustum import cull_bounds
            if self.rows_format == "half":
                means = np.ascontiguousarray(self._rows[:, 112:124]).view(np.float32)
                scales = widen_half(np.ascontiguousarray(self._rows[:, 104:110]).view(np.uint16))
            else:
                means, scales = np.ascontiguousarray(self._rows[:, 52:55]), np.ascontiguousarray(self._rows[:, 55:58])
            means, scales = torch.from_numpy(means).to(self.dev), torch.from_numpy(scales).to(self.dev)
            self._bounds = (key, cull_bounds(nodes, means, scales))
            del means, scales
        return self._bounds[1]

    def _cut(self, nodes, boxes, t, viewpoint_gpu, viewpoint_cpu, bufs, frustum):
        """One cut at ``t`` into ``bufs``: (entries, entries the frustum dropped, are the weights already in bufs?)."""
        if frustum is None:
            from gaussian_hierarchy._C import expand_to_size
            return expand_to_size(nodes, boxes, t, viewpoint_gpu, torch.zeros(3), bufs.ri, bufs.pi, bufs.ni), 0, False
        from .frustum import cut_view
        cv = cut_view(nodes, boxes, self._cull_bounds(nodes), t, viewpoint_cpu, frustum[0], frustum[1], out=bufs)
        return cv.n, cv.n_unculled - cv.n, True

    def _join_prefetch(self):
        """The current stream waits for a prefetch in flight (it owns slot_of / stamp / the free list until it is done)."""
        if self._prefetch_done is not None:
            torch.cuda.current_stream(self.dev).wait_event(self._prefetch_done)
            self._prefetch_done = None

    def _start_tau(self, tau, fine_growth):
        """Where the regulator starts for a request of ``tau``: (granularity, probing a finer step?)."""
        t = float(tau)
        probing = False
        if self._regulated is not None and self._regulated > t:
            # the previous view had to be coarsened: start from what fitted then, and only every `probe_every`-th view
            # one step finer (a cut that does not fit costs a cut, its weights and a pass over its rows with every miss
            # queued and taken back: 10 ms at 25 M entries).  A probe that fails doubles the interval (up to 256 views), one
            # that fits resets it: a camera that stays in a region the budget cannot show finer stops paying for asking.
            self._since_probe += 1
            probing = self._since_probe >= self.probe_every
            if probing:
                self._since_probe = 0
            t = max(t, self._regulated / fine_growth if probing else self._regulated)
        return t, probing

    def _fit(self, nodes, boxes, tau, t, probing, viewpoint_gpu, viewpoint_cpu, bufs, new_frame, max_attempts, growth,
             fine_growth, reuse_n=None, frustum=None):
        """Cut + weights + residency into ``bufs``, coarsening until the rows fit: (n, t, ro, po, rows fetched, attempts).
        ``reuse_n``: the cut and its weights at ``t`` are already in ``bufs`` (a prefetch left them): (entries, culled).
        ``frustum``: the (planes, radius_scale) pair of hgs.frustum.frustum_planes -- every cut is then a ``cut_view``."""
        from gaussian_hierarchy._C import get_interpolation_weights
        zero3 = torch.zeros(3)
        for attempt in range(1, max_attempts + 1):
            reuse = attempt == 1 and reuse_n is not None
            n, culled, weighted = (reuse_n[0], reuse_n[1], True) if reuse else \
                self._cut(nodes, boxes, t, viewpoint_gpu, viewpoint_cpu, bufs, frustum)
            near = n <= 1.1 * self.B
            try:
                if n > self.B:          # more node rows than slots: no need to look at them
                    raise _lib.HgsError(f"a cut of {n} entries cannot fit a budget of {self.B} rows", _lib.ERR_CAPACITY)
                # the weights first: an entry of weight 1 does not need its parent row (make_resident)
                if not weighted:
                    get_interpolation_weights(bufs.ni[:n], t, nodes, boxes, viewpoint_cpu, zero3, bufs.w, bufs.ns)
                ro, po, m = self.make_resident(bufs.ri[:n], bufs.pi[:n], bufs.w, _bufs=bufs, _new_frame=new_frame)
            except _lib.HgsError as e:
                if e.code != _lib.ERR_CAPACITY:
                    raise
                self.stats["retries"] += 1
                if probing and attempt == 1:
                    self.probe_every = min(2 * self.probe_every, 256)
                t = t * (fine_growth if near else growth) if t > 0 else 1e-4
                continue
            if probing and attempt == 1:
                self.probe_every = 16
            self._regulated = t if t > float(tau) else None
            self.stats["entries_culled"] += culled
            return n, t, ro, po, m, attempt
        raise RuntimeError(f"no granularity up to tau = {t:g} fits a budget of {self.B} rows")

    def _cut_budget(self, nodes, boxes, tau, viewpoint_cpu, bufs, frustum):
        """fit="budget": the one cut of a view into ``bufs`` -> hgs.frustum.BudgetCut (its tau is >= ``tau``, its cost
        <= the budget).  The coarsest cut not fitting raises _lib.HgsError (ERR_CAPACITY)."""
        from .frustum import cut_to_budget
        if frustum is None:
            return cut_to_budget(nodes, boxes, None, self.B, viewpoint_cpu, tau_min=tau, cost="rows", out=bufs)
        return cut_to_budget(nodes, boxes, self._cull_bounds(nodes), self.B, viewpoint_cpu, frustum[0], frustum[1],
                             tau_min=tau, cost="rows", out=bufs)

    @staticmethod
    def _check_fit(fit):
        if fit not in ("regulate", "budget"):
            raise ValueError(f"fit must be 'regulate' or 'budget', not {fit!r}")

    def prefetch(self, nodes, boxes, tau, viewpoint_gpu, viewpoint_cpu, frustum=None, fit="regulate") -> int:
        """The NEXT view's cut, weights and residency on a second stream, to be called right after the current view's
        render was enqueued (its pose known or predicted: a viewer extrapolates its camera).  BEST EFFORT: rows the
        current view uses are never evicted (they carry the current frame's stamp; so do the rows fetched here), nothing
        the render reads is written -- free slots and slots of older frames are filled, the other set of cut buffers
        receives the indices -- and no granularity is changed.  When everything the next view needs became resident,
        ``select`` for the same viewpoint and request starts from this cut (its mark pass only stamps the rows); otherwise
        it finds that many fewer rows missing.  ``frustum``: the NEXT view's (planes, radius_scale) pair; ``select`` reuses
        the cut only when it is given the same one.  ``fit="budget"``: the cut is the one ``cut_to_budget`` of
        ``select(..., fit="budget")`` -- a function of the viewpoint, the frustum and the request alone, so ``select``
        reuses it under the same three and the same ``fit``.  Returns the rows fetched."""
        from gaussian_hierarchy._C import get_interpolation_weights
        self._check_fit(fit)
        if frustum is not None:
            self._cull_bounds(nodes)    # (a first use builds the balls on the current stream, before the side stream waits)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        side, zero3 = self._side, torch.zeros(3)
        self._join_prefetch()
        if self._resid_done is not None:
            side.wait_event(self._resid_done)       # the last select's residency kernels -- NOT the render behind them
        else:
            side.wait_stream(torch.cuda.current_stream(self.dev))
        other = self._sets[1 - self._cur]
        self._prefetched = None
        t = max(float(tau), self._regulated or 0.0)
        m = 0
        with torch.cuda.stream(side):
            try:
                if fit == "budget":
                    cut = self._cut_budget(nodes, boxes, float(tau), viewpoint_cpu, other, frustum)
                    ro, _, m = self.make_resident(other.ri[:cut.n], other.pi[:cut.n], other.w, _bufs=other,
                                                  _new_frame=False, _best_effort=True)
                    if ro is not None:
                        self._prefetched = (self._vp_key(viewpoint_cpu, frustum), float(tau), cut.tau,
                                            (cut.n, cut.n_unculled - cut.n), fit, cut.cost)
                    self.stats["prefetched_rows"] = self.stats.get("prefetched_rows", 0) + m
                    return m
                n, culled, weighted = self._cut(nodes, boxes, t, viewpoint_gpu, viewpoint_cpu, other, frustum)
                if n <= self.B:
                    if not weighted:
                        get_interpolation_weights(other.ni[:n], t, nodes, boxes, viewpoint_cpu, zero3, other.w, other.ns)
                    ro, _, m = self.make_resident(other.ri[:n], other.pi[:n], other.w, _bufs=other, _new_frame=False,
                                                  _best_effort=True)
                    if ro is not None:
                        self._prefetched = (self._vp_key(viewpoint_cpu, frustum), float(tau), t, (n, culled), fit, 0)
                    self.stats["prefetched_rows"] = self.stats.get("prefetched_rows", 0) + m
            finally:
                self._prefetch_done = torch.cuda.Event()
                self._prefetch_done.record(side)
        return m

    def select(self, nodes, boxes, tau, viewpoint_gpu, viewpoint_cpu, max_attempts: int = 96, growth: float = 1.2,
               fine_growth: float = 1.05, frustum=None, fit="regulate") -> Selection:
        """expand_to_size + get_interpolation_weights at ``tau`` (train_post.py:91-113, render_hierarchy.py:58-80), the
        cut's rows made resident; a cut that does not fit the budget is repeated at ``growth`` x tau (from 1e-4 when the
        request was tau = 0: every leaf) -- at ``fine_growth`` x tau once the cut is within a tenth of the budget, so that
        the regulator settles on the last few per cent of it.  ``frustum``: the view's (planes, radius_scale) pair of
        hgs.frustum.frustum_planes -- the cut and every retry of the regulator then drop the entries outside it
        (hgs.frustum.cut_view: the kept entries are those of the plain cut, unchanged), ``stats["entries_culled"]`` counts
        them, and rows no view looks at are neither fetched nor held.
        ``fit="budget"``: no search -- one ``hgs.frustum.cut_to_budget(tau_min=tau, budget=B, cost="rows")`` selects the
        finest granularity >= ``tau`` whose rows fit (``Selection.tau``; ``tau`` itself when the request fits) and
        ``make_resident`` runs once: ``attempts`` is 1, nothing is retried, and ``max_attempts``, ``growth``,
        ``fine_growth`` and the state the regulator keeps between views play no part.  Needs boxes that nest."""
        self._check_fit(fit)
        self._join_prefetch()
        pre, self._prefetched = self._prefetched, None
        if fit == "budget":
            return self._select_budget(nodes, boxes, tau, viewpoint_cpu, frustum, pre)
        (t, probing), reuse_n = self._start_tau(tau, fine_growth), None
        if not probing and pre is not None and pre[4] == fit and pre[0] == self._vp_key(viewpoint_cpu, frustum) and pre[1] == float(tau) and pre[2] == t:
            self._cur = 1 - self._cur   # the cut and its weights are waiting in the other buffer set
            reuse_n = pre[3]
        bufs = self._sets[self._cur]
        n, t, ro, po, m, attempt = self._fit(nodes, boxes, tau, t, probing, viewpoint_gpu, viewpoint_cpu, bufs, True,
                                             max_attempts, growth, fine_growth, reuse_n, frustum)
        self.stats["views"] += 1
        self._resid_done = torch.cuda.Event()
        self._resid_done.record(torch.cuda.current_stream(self.dev))
        return Selection(n, t, ro, po, bufs.w, bufs.ns, m, attempt)

    def _select_budget(self, nodes, boxes, tau, viewpoint_cpu, frustum, pre) -> Selection:
        if pre is not None and pre[4] == "budget" and pre[0] == self._vp_key(viewpoint_cpu, frustum) and pre[1] == float(tau):
            self._cur = 1 - self._cur   # the cut and its weights are waiting in the other buffer set
            bufs = self._sets[self._cur]
            t, (n, culled), cost = pre[2], pre[3], pre[5]
        else:
            bufs = self._sets[self._cur]
            cut = self._cut_budget(nodes, boxes, float(tau), viewpoint_cpu, bufs, frustum)
            t, n, culled, cost = cut.tau, cut.n, cut.n_unculled - cut.n, cut.cost
        ro, po, m = self.make_resident(bufs.ri[:n], bufs.pi[:n], bufs.w, _bufs=bufs)
        self.stats["entries_culled"] += culled
        self.stats["views"] += 1
        self._resid_done = torch.cuda.Event()
        self._resid_done.record(torch.cuda.current_stream(self.dev))
        return Selection(n, t, ro, po, bufs.w, bufs.ns, m, 1, cost)
