"""Caller memory as a caller has it: named arrays laid out in ONE slab -- a ``uint8`` tensor filled with the guard byte 0xA5 -- each at
a chosen residue of its address modulo 16, with at least 256 guard bytes of its own before and after it (more than one 16-byte vector
and more than one 128-byte line: a condition, not a measurement).  An ``in`` array is initialised and a copy is kept; an ``out`` array
is filled with a second pattern, 0x5C, over its documented room.  ``Slab.check()`` copies the slab back once and says what was written
outside the arrays and which input changed.  A fresh ``torch`` allocation is 256-byte aligned and nobody looks at what follows it; a
view of this slab is neither.  tests/test_caller_views.py holds the helper to its word on the CPU."""
import collections

import numpy as np

GUARD, FILL, MARGIN = 0xA5, 0x5C, 256

#: one thing ``Slab.check()`` found: the array's name, ``before`` / ``after`` / ``input changed``, and the first offending byte counted
#: from the array's first byte (negative before it, at or beyond its size after it)
Finding = collections.namedtuple("Finding", "name side offset")
_View = collections.namedtuple("_View", "name lo start nbytes role copy")


def _torch_dtype(dt):
    import torch
    return {("u", 1): torch.uint8, ("i", 1): torch.int8, ("i", 4): torch.int32, ("u", 4): torch.int32, ("i", 8): torch.int64,
            ("u", 8): torch.int64, ("f", 8): torch.float64, ("f", 4): torch.float32}[(dt.kind, dt.itemsize)]


class Slab(object):
    """``Slab(device).place(name, array_or_shape, dtype, residue, role)`` -> a contiguous typed view with ``data_ptr() % 16 == residue``.
    (uint32 / uint64 arrays come back as int32 / int64 tensors: the same bytes.)  ``nbytes``: the slab's size, allocated at once.
    ``skew`` (a multiple of 8) starts the slab that many bytes into its allocation: the residues are worked out from the address the slab
    really has, whatever the allocator's alignment."""

    def __init__(self, device, nbytes=1 << 22, skew=0):
        import torch
        if skew % 8:
            raise ValueError("skew must be a multiple of 8")
        self._raw = torch.full((nbytes + skew,), GUARD, dtype=torch.uint8, device=device)
        self.mem = self._raw[skew:]
        self.base = self.mem.data_ptr()
        if self.base % 8:
            raise ValueError("the slab's allocation is not 8-byte aligned: no typed view can be taken")
        self.views = []
        self._cursor = 0                                 # first byte no view owns yet

    def place(self, name, array_or_shape, dtype, residue, role):
        import torch
        dt = np.dtype(dtype)
        if role not in ("in", "out"):
            raise ValueError("role is 'in' or 'out'")
        if not 0 <= residue < 16 or residue % dt.itemsize:
            raise ValueError("residue %r does not suit %s: a multiple of %d below 16" % (residue, dt, dt.itemsize))
        if any(v.name == name for v in self.views):
            raise ValueError("two arrays named %r" % name)
        if role == "in":
            arr = np.ascontiguousarray(array_or_shape, dtype=dt)
            shape = arr.shape
        else:
            shape = tuple(array_or_shape.shape) if hasattr(array_or_shape, "shape") else tuple(np.atleast_1d(array_or_shape).tolist())
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        lo = self._cursor
        start = lo + MARGIN
        start += (residue - (self.base + start)) % 16
        if start + nbytes + MARGIN > self.mem.numel():
            raise ValueError("the slab of %d bytes is full" % self.mem.numel())
        raw = self.mem[start:start + nbytes]
        if role == "in":
            raw.copy_(torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()))
            copy = arr.reshape(-1).view(np.uint8).copy()
        else:
            raw.fill_(FILL)
            copy = None
        if raw.is_cuda:
            torch.cuda.synchronize()                     # (the library works on streams of its own: the patterns are in place before it starts)
        view = raw.view(_torch_dtype(dt)).view(shape)
        assert view.data_ptr() == self.base + start and view.data_ptr() % 16 == residue and view.is_contiguous()
        self.views.append(_View(name, lo, start, nbytes, role, copy))
        self._cursor = start + nbytes + MARGIN
        return view

    def zones(self, name):
        """((first, end) of the guard bytes before, (first, end) of those after) array ``name``, as offsets into the slab."""
        k = [v.name for v in self.views].index(name)
        v = self.views[k]
        end = v.start + v.nbytes
        return (v.lo, v.start), (end, self.views[k + 1].lo if k + 1 < len(self.views) else self.mem.numel())

    def host(self):
        """The slab as it is now, on the host (one copy)."""
        return self.mem.cpu().numpy()

    def room(self, name, host=None):
        """The bytes of array ``name`` (from ``host``, a copy of the slab made earlier, or from a fresh one)."""
        v = self.views[[x.name for x in self.views].index(name)]
        return (self.host() if host is None else host)[v.start:v.start + v.nbytes]

    def untouched(self, name, host=None):
        """Whether the whole room of the ``out`` array ``name`` still holds the fill pattern."""
        return bool((self.room(name, host) == FILL).all())

    def freeze(self, name):
        """The ``out`` array ``name`` becomes an ``in`` array holding what it holds now (what one call wrote, the next must only read)."""
        k = [v.name for v in self.views].index(name)
        self.views[k] = self.views[k]._replace(role="in", copy=self.room(name).copy())

    def check(self, host=None):
        """One copy of the slab back (or ``host``, one made just now); -> the list of findings, empty when no guard byte was touched and no
        input changed."""
        host = self.host() if host is None else host
        found = []
        for v in self.views:
            (b0, b1), (a0, a1) = self.zones(v.name)
            for side, z0, z1 in (("before", b0, b1), ("after", a0, a1)):
                bad = np.flatnonzero(host[z0:z1] != GUARD)
                if len(bad):
                    found.append(Finding(v.name, side, int(bad[0]) + z0 - v.start))
            if v.role == "in":
                bad = np.flatnonzero(host[v.start:v.start + v.nbytes] != v.copy)
                if len(bad):
                    found.append(Finding(v.name, "input changed", int(bad[0])))
        return found
