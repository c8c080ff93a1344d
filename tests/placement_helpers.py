"""Placements of batch arrays with canaries, for the tests of the C-ABI's addressing promise (include/fbstab_hip.h:
QP b of an array lives at base + b * stride; records and separate arrays both work; stride 0 shares an array).

A layout is built from a dict of packed ``(B, len)`` arrays and gives strided views onto fresh backing buffers:

  records   one record per QP holding all arrays of the dict back to back, GAP doubles behind each: every view has
            the same row stride (the record length), larger than its length; slot starts are 8-byte aligned and only
            sometimes 16-byte aligned (odd lengths, an odd gap)
  spread    one buffer per array, row stride len + pad with another odd pad per array (1, 3, 5, ...)
  shared    the named arrays as ONE ``(1, len)`` row (stride 0 in the block), the others spread; returned with the
            packed twin in which the row is repeated B times

Every buffer is rows x stride doubles, so the last QP's slot is followed by a gap INSIDE the allocation: a write one
element past a slot lands in a canary, not outside the buffer.  The gaps hold CANARY, one quiet-NaN bit pattern with a
recognisable payload: a write there changes bits (``assert_gaps_intact`` compares the gaps as uint64), and a read
there that reaches arithmetic produces NaN.  Slots named in ``canary`` start as CANARY too (outputs that the call
does not read).

Plain numpy; ``Placed.on(device)`` moves the buffers to a torch device (byte copies: payloads survive) and rebuilds
the views there, ``Placed.read`` / ``assert_intact`` look at whatever the buffers hold now."""
import numpy as np

CANARY = np.uint64(0x7FF8C0DEFACE5EED)   # quiet NaN, payload 0xC0DEFACE5EED
GAP = 3


class Buffer:
    """``n`` doubles, CANARY everywhere until ``place`` puts slots in; ``gap`` marks what is still no slot."""

    def __init__(self, n):
        self.bits = np.full(n, CANARY, dtype=np.uint64)
        self.data = self.bits.view(np.float64)
        self.gap = np.ones(n, dtype=bool)
        self.dev = None   # the torch twin, once `to` has made it

    def view(self, offset, stride, rows, length):
        """The ``(rows, length)`` view at ``offset`` with row stride ``stride`` (doubles), on the host or the device."""
        assert 0 <= offset and (rows - 1) * stride + offset + length <= self.data.size
        if self.dev is not None:
            return self.dev.as_strided((rows, length), (stride, 1), offset)
        return np.lib.stride_tricks.as_strided(self.data[offset:], shape=(rows, length), strides=(8 * stride, 8))

    def place(self, offset, stride, rows, length, values=None):
        """Makes the slots of one array (they must not overlap earlier ones) and fills them (None: left CANARY)."""
        assert self.dev is None
        idx = (offset + stride * np.arange(rows)[:, None] + np.arange(length)[None, :]).reshape(-1)
        assert self.gap[idx].all() and np.unique(idx).size == idx.size, "slots overlap"
        self.gap[idx] = False
        v = self.view(offset, stride, rows, length)
        if values is not None:
            v[...] = values
        return v

    def to(self, device):
        import torch
        self.dev = torch.from_numpy(self.bits.view(np.int64).copy()).to(device).view(torch.float64)

    def host_bits(self):
        """What the buffer holds now, as uint64 on the host."""
        if self.dev is None:
            return self.bits
        import torch
        return self.dev.view(torch.int64).cpu().numpy().view(np.uint64)


def assert_gaps_intact(buf, what=""):
    """Every double of ``buf`` (a Buffer) outside its slots still holds CANARY, compared as uint64."""
    bits = buf.host_bits()
    bad = np.nonzero(buf.gap & (bits != CANARY))[0]
    assert bad.size == 0, "%s: %d canaries overwritten, first at double %d (0x%016x)" % (
        what or "buffer", bad.size, bad[0], int(bits[bad[0]]))


class Placed:
    """A dict of views (``views[name]``: ``(rows, len)``, numpy or torch) with where they live:
    ``slots[name] = (buffer, offset, stride, rows, len)``, ``shared``: the names given as one row."""

    def __init__(self):
        self.views, self.slots, self.buffers, self.shared = {}, {}, [], ()

    def _add(self, name, buf, offset, stride, rows, length, values):
        if buf not in self.buffers:
            self.buffers.append(buf)
        self.views[name] = buf.place(offset, stride, rows, length, values)
        self.slots[name] = (buf, offset, stride, rows, length)

    def _add_empty(self, name, rows):
        self.views[name] = np.zeros((rows, 0))
        self.slots[name] = None

    def on(self, device):
        """Moves every buffer to ``device`` (None: stays on the host) and rebuilds the views there."""
        if device is None:
            return self
        import torch
        for b in self.buffers:
            b.to(device)
        for k, s in self.slots.items():
            self.views[k] = (torch.zeros(self.views[k].shape, dtype=torch.float64, device=device) if s is None
                             else s[0].view(*s[1:]))
        return self

    def read(self, name):
        """The packed ``(rows, len)`` copy of what the slots of ``name`` hold now (uint64 bits viewed as float64)."""
        s = self.slots[name]
        if s is None:
            return np.zeros(self.views[name].shape)
        buf, offset, stride, rows, length = s
        idx = offset + stride * np.arange(rows)[:, None] + np.arange(length)[None, :]
        return buf.host_bits()[idx].view(np.float64)

    def write(self, name, values):
        """Overwrites the slots of ``name`` with the packed ``(rows, len)`` array ``values``, where they live."""
        v = self.views[name]
        if isinstance(v, np.ndarray):
            v[...] = values
        else:
            import torch
            v.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(v.device))

    def assert_intact(self, what=""):
        for i, b in enumerate(self.buffers):
            assert_gaps_intact(b, "%s buffer %d" % (what, i))

    def __getitem__(self, name):
        return self.views[name]


def _rows(arrays):
    return next(iter(arrays.values())).shape[0]


def records(arrays, canary=(), gap=GAP):
    """All arrays of the dict in one record per QP, ``gap`` doubles behind each array."""
    p = Placed()
    B = _rows(arrays)
    rec = sum(a.shape[1] + gap for a in arrays.values() if a.shape[1] > 0)
    buf = Buffer(B * rec)
    off = 0
    for k, a in arrays.items():
        assert a.shape[0] == B, (k, a.shape, B)
        if a.shape[1] == 0:
            p._add_empty(k, B)
            continue
        p._add(k, buf, off, rec, B, a.shape[1], None if k in canary else a)
        off += a.shape[1] + gap
    return p


def spread(arrays, canary=(), first_pad=1):
    """One buffer per array, row stride len + pad, pad = first_pad, first_pad + 2, ... in the order of the dict."""
    p = Placed()
    pad = first_pad
    for k, a in arrays.items():
        B, n = a.shape
        if n == 0:
            p._add_empty(k, B)
            continue
        p._add(k, Buffer(B * (n + pad)), 0, n + pad, B, n, None if k in canary else a)
        pad += 2
    return p


def packed(arrays, canary=()):
    """The twin every placement is compared with: one buffer per array, stride = length, no gap anywhere."""
    p = Placed()
    for k, a in arrays.items():
        B, n = a.shape
        if n == 0:
            p._add_empty(k, B)
            continue
        p._add(k, Buffer(B * n), 0, n, B, n, None if k in canary else a)
    return p


def shared(arrays, names, canary=(), gap=GAP, rest=spread):
    """``(placed, twin)``: the arrays of ``names`` as one ``(1, len)`` row each (row 0 of the packed array, followed
    by ``gap`` canaries), the others laid out by ``rest``; ``twin`` is the packed dict with that row repeated for
    every QP."""
    B = _rows(arrays)
    p = rest({k: a for k, a in arrays.items() if k not in names}, canary)
    twin = {k: np.ascontiguousarray(a) for k, a in arrays.items()}
    for k in names:
        a = arrays[k]
        if a.shape[1] == 0:
            p._add_empty(k, 1)
            continue
        p._add(k, Buffer(a.shape[1] + gap), 0, a.shape[1] + gap, 1, a.shape[1], None if k in canary else a[:1])
        twin[k] = np.ascontiguousarray(np.repeat(a[:1], B, axis=0))
    p.shared = tuple(names)
    # (the order of the dict is the order of the block's slots for whoever iterates the views)
    p.views = {k: p.views[k] for k in arrays}
    return p, twin


def merge(*parts, order=None):
    """One Placed of several (disjoint names); ``order``: the order of the names in ``views``."""
    p = Placed()
    for q in parts:
        p.views.update(q.views)
        p.slots.update(q.slots)
        p.buffers += [b for b in q.buffers if b not in p.buffers]
        p.shared += tuple(q.shared)
    if order is not None:
        p.views = {k: p.views[k] for k in order}
    return p


LAYOUTS = {"records": records, "spread": spread}


def fill_block(block, names, lens, placed, B, dev_flags, optional=False, only=None):
    """hip_api._fill_block on the views as they are (``shared=False``: every view's own row stride stands), then
    stride 0 for the names that ``placed`` holds as one shared row.  ``only``: the names that go into the block (the
    others stay NULL; needs ``optional``).  Returns what _fill_block returns."""
    from fbstab_amd import hip_api
    views = placed.views if isinstance(placed, Placed) else placed
    if only is not None:
        views = {k: a for k, a in views.items() if k in only}
    B = hip_api._fill_block(block, names, lens, views, B, dev_flags, optional=optional, shared=False)
    for k in getattr(placed, "shared", ()):
        if k in views and block.base[list(names).index(k)]:
            block.stride[list(names).index(k)] = 0
    return B
