"""Guarded device allocations for the workspace-bounds tests (a helper module, not a fixture).

``guarded(nbytes, device, fill)`` allocates ONE uint8 tensor laid out as

    [head guard >= 4096 bytes][body: nbytes][tail guard 4096 bytes]

with the body starting on a 256-byte boundary (the alignment the C ABI's callers give their workspaces).  Both guards
hold 0xA5 -- deliberately non-zero: an overrun that stores zeros (rows past P of a whole-wave store) is then visible.
The body is filled with ``fill`` (0x00 or 0xFF; an all-0xFF float32 is a NaN), so that running the same chain with
both fills also shows whether a kernel reads bytes it did not write.  ``check(g)`` synchronises and asserts that both
guards are intact; a failure names the first and last corrupted byte relative to the body's end (tail) or start (head).
"""
import torch

GUARD = 4096
PATTERN = 0xA5
_ALIGN = 256


class Guarded:
    __slots__ = ("name", "raw", "off", "nbytes")

    def __init__(self, name, raw, off, nbytes):
        self.name, self.raw, self.off, self.nbytes = name, raw, off, nbytes

    @property
    def addr(self):
        return self.raw.data_ptr() + self.off

    @property
    def body(self):
        return self.raw[self.off:self.off + self.nbytes]

    def view(self, dtype, *shape):
        """The body as a tensor of ``dtype`` and ``shape`` (must cover the body exactly)."""
        t = self.body.view(dtype)
        return t.view(*shape) if shape else t


def guarded(nbytes, device, fill, name="buffer"):
    nbytes = int(nbytes)
    assert fill in (0x00, 0xFF)
    raw = torch.full((GUARD + _ALIGN + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=device)
    off = GUARD + (-(raw.data_ptr() + GUARD)) % _ALIGN
    raw[off:off + nbytes] = fill
    return Guarded(name, raw, off, nbytes)


def check(*gs):
    """Every guard of every ``Guarded`` in ``gs`` still holds PATTERN (after a device synchronisation)."""
    torch.cuda.synchronize()
    for g in gs:
        head = g.raw[:g.off]
        tail = g.raw[g.off + g.nbytes:]
        for part, what, base in ((head, "head", -g.off), (tail, "tail", 0)):
            bad = torch.nonzero(part != PATTERN).flatten()
            if bad.numel():
                first, last = int(bad[0]) + base, int(bad[-1]) + base
                if what == "head":
                    msg = f"bytes [{first}, {last}] before the body's start"
                else:
                    msg = f"bytes [+{first}, +{last}] past the body's end"
                raise AssertionError(f"{g.name} ({g.nbytes} bytes): {what} guard corrupted, {bad.numel()} bytes, {msg}")
