"""Caller memory WHEN a caller calls (``tests/caller_views.py``: where it sits): tensors that a kernel queued on torch's current stream
has not written yet when the Python layer is called, and memory that torch reuses the moment the call returns.

``Late`` holds, for every input of a call, a device tensor pre-filled with a *decoy* and the real content in a second tensor.
``Late.arm(stream)`` queues a delay kernel on ``stream`` and behind it one copy per input, real over decoy, then an event;
``Late.in_flight()`` is ``not event.query()``.  A layer that does not order the library behind the caller's stream hands it the decoy.

The decoy rule keeps that a wrong answer and never a fault: decoy and real content have the same shapes and every element-wise mixture
of the two is a valid input -- the arrays that index (``indptr``, ``indices``, ``read_id``, ``cell_ptr`` ...) keep their content, the
value arrays differ within their ranges -- and the decoy's own answer differs from the real one (asserted by every case on its CPU
checker, so that none is vacuous).  ``check_rule`` holds a case to the shapes.

The delay is ``torch.cuda._sleep(cycles)``, calibrated once per session with two events.  Its length is not chosen: it is ten times the
slowest call it has to outlast.  Measured at the parent of the commit that added this file, on the default stream with nothing in
flight, host clock from the wrapper's entry to its return, every case of ``test_gpu_inflight_tensors.py`` at its shape:

    the slowest case, ``combine``, its third call (no first-use cost left):  2.76 ms    -> CALL_MS = 2.8
    (the others: 0.02 ms, ``export_device``, to 2.65 ms, ``bundle``; the Python prologue is part of each)
    DELAY_MS = FACTOR x CALL_MS = 28 ms,  FACTOR = 10

A case makes the same call on finished tensors first, so that what a first call costs on top (up to 215 ms: the library's scratch, a
module's first launch) does not fall into the delay.
Every iterative entry is capped at ``max_iters`` of a few steps, so that no call takes longer than that.

``reuse_after`` is the other end of the call: right after it returns, on the caller's stream and without a host wait, the outputs are
cloned, every input is overwritten in place with its decoy, and tensors of the inputs' and the conversion temporaries' sizes are
allocated and filled with 0x5A -- the caching allocator hands the blocks the wrapper just freed out again.  The clones are compared
afterwards: a wrapper that returned with work still reading its inputs or its temporaries gives the wrong answer here."""
import numpy as np

FACTOR = 10
CALL_MS = 2.8                # measured: see the docstring
DELAY_MS = FACTOR * CALL_MS
REUSE_BYTE = 0x5A
MODES = ("off", "default-late", "default-converted-i64", "default-converted-strided", "default-converted-cpu",
         "side-late", "side-converted-i64", "side-converted-strided", "side-converted-cpu")
_cycles_per_ms = []


def cycles_per_ms():
    """``torch.cuda._sleep``'s cycles per millisecond on this device: one sleep timed between two events, once per session."""
    import torch
    if not _cycles_per_ms:
        probe = 20_000_000
        torch.cuda._sleep(1000)                       # (the kernel's first launch is not the one timed)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.05, "torch.cuda._sleep(%d) took %.3f ms: nothing to calibrate on" % (probe, ms)
        _cycles_per_ms.append(probe / ms)
    return _cycles_per_ms[0]


def delay(ms=None):
    """Queue the delay on torch's current stream."""
    import torch
    torch.cuda._sleep(int((DELAY_MS if ms is None else ms) * cycles_per_ms()))


class Input(object):
    """One input of a call: ``real`` and ``decoy`` (numpy, equal shape and dtype; ``decoy`` None: the array indexes and keeps its
    content), and what a converted mode may do to it -- ``wide``: the wrapper takes it as int32 and converts an int64 tensor;
    ``fixed``: the wrapper takes it as it is and nothing else (an in-place argument)."""

    def __init__(self, name, real, decoy=None, wide=False, fixed=False):
        self.name, self.real = name, real if hasattr(real, "data_ptr") else np.ascontiguousarray(real)
        self.decoy = self.real if decoy is None else decoy if hasattr(decoy, "data_ptr") else np.ascontiguousarray(decoy, dtype=self.real.dtype)
        self.wide, self.fixed = wide, fixed


def check_rule(inputs):
    """The part of the decoy rule that is about the arrays themselves: equal shapes and types, and at least one array that differs."""
    for i in inputs:
        assert i.decoy.shape == i.real.shape and i.decoy.dtype == i.real.dtype, i.name
    assert any(i.decoy is not i.real and not np.array_equal(_host(i.decoy), _host(i.real)) for i in inputs), "no input has a decoy of its own"


def _signed(a):
    """(torch computes with no unsigned words: the signed ones hold the same bytes)"""
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "u" else a


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def _tensor(a, device="cuda"):
    """(what is a tensor already -- something the library wrote -- is copied)"""
    import torch
    return a.to(device, copy=True) if hasattr(a, "data_ptr") else torch.from_numpy(_signed(np.ascontiguousarray(a)).copy()).to(device)


class Late(object):
    """``Late(inputs, convert, outs)``: per input the tensor the call is handed (``.v[name]``), holding the decoy now, and the real
    content beside it.  ``convert``: None, or how the wrapper must convert what it is handed -- ``"i64"`` (int64 where it wants int32),
    ``"strided"`` (every array a stride-2 view) or ``"cpu"`` (the second array a CPU tensor, the others as they are).  ``outs``:
    ``(name, shape, numpy dtype)`` of the outputs the caller allocates: each holds 0xA5 now, and its fill with 0x5C -- a caller's
    ``zeros()`` -- is part of the producer; a library that writes before the fill has landed loses its result to it."""

    def __init__(self, inputs, convert=None, outs=()):
        import torch
        from caller_views import FILL, GUARD, _torch_dtype
        self.inputs, self.convert, self.event = list(inputs), convert, None
        self.v, self._real, self._decoy, self._outs, self._fill = {}, {}, {}, [], FILL
        for name, shape, dt in outs:
            raw = torch.full((int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize,), GUARD, dtype=torch.uint8, device="cuda")
            self.v[name] = raw.view(_torch_dtype(np.dtype(dt))).view(tuple(shape))
            self._outs.append(raw)
        for k, i in enumerate(self.inputs):
            real, decoy = _tensor(i.real), _tensor(i.decoy)
            if convert == "cpu" and k == 1 and not i.fixed:
                self.v[i.name] = _tensor(i.real, "cpu")            # (finished by nature: what is late is its copy to the device)
                continue
            if convert == "i64" and i.wide and not i.fixed:
                real, decoy = real.to(torch.int64), decoy.to(torch.int64)
            if convert == "strided" and not i.fixed:
                base = torch.empty(tuple(decoy.shape) + (2,), dtype=decoy.dtype, device="cuda")
                base[...] = decoy.unsqueeze(-1)
                dst = base[..., 0]
                assert not dst.is_contiguous() or dst.numel() <= 1
            else:
                dst = decoy.clone()
            self.v[i.name], self._real[i.name], self._decoy[i.name] = dst, real, decoy
        torch.cuda.synchronize()                                  # (the decoys are in place and finished)

    @property
    def converted(self):
        """Whether the wrapper has a conversion to queue for at least one input."""
        import torch
        return any(not t.is_cuda or not t.is_contiguous() or (i.wide and t.dtype == torch.int64) for i in self.inputs for t in [self.v[i.name]])

    def arm(self, stream):
        """The producer, on ``stream``: the delay, then real over decoy for every input, then the event."""
        import torch
        with torch.cuda.stream(stream):
            delay()
            self._produce()
            self.event = torch.cuda.Event()
            self.event.record(stream)

    def _produce(self):
        for name, dst in self.v.items():
            if name in self._real:
                dst.copy_(self._real[name])
        for raw in self._outs:
            raw.fill_(self._fill)

    def settle(self):
        """Nothing in flight: the producer's work done, and waited for."""
        import torch
        self._produce()
        torch.cuda.synchronize()

    def in_flight(self):
        return not self.event.query()

    def temporaries(self):
        """The sizes in bytes of what the wrapper allocates to convert what it was handed: one contiguous array of the wanted type per
        input that is not one already."""
        import torch
        out = []
        for i in self.inputs:
            t = self.v[i.name]
            if not t.is_cuda or not t.is_contiguous() or (i.wide and t.dtype == torch.int64):
                out.append(t.numel() * (4 if i.wide else t.element_size()))
        return out


def _tensors(x):
    """Every tensor of a result: tuples, lists and dicts walked in order."""
    if hasattr(x, "data_ptr"):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _tensors(x[k])]
    if isinstance(x, (tuple, list)):
        return [t for y in x for t in _tensors(y)]
    return []


def _cloned(x):
    if hasattr(x, "data_ptr"):
        return x.clone()
    if isinstance(x, dict):
        return {k: _cloned(y) for k, y in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(_cloned(y) for y in x)
    return x


def reuse_after(outputs, late):
    """Right after the call returned, on torch's current stream and without a host wait: the outputs cloned, every input overwritten in
    place with its decoy, tensors of the inputs' and the temporaries' sizes allocated and filled -> (the outputs with every tensor
    replaced by its clone, the fills: kept alive by the caller until it has compared)."""
    import torch
    cloned = _cloned(outputs)
    for name, dst in late.v.items():
        if name in late._decoy:
            dst.copy_(late._decoy[name])
    sizes = [t.numel() * t.element_size() for t in late.v.values()] + late.temporaries()
    fills = [torch.full((max(n, 1),), REUSE_BYTE, dtype=torch.uint8, device="cuda") for n in sizes]
    return cloned, fills


def flat(result):
    """A result as a list of numpy arrays (tensors copied back) and plain values, in the order of :func:`_tensors` for the tensors."""
    if hasattr(result, "data_ptr"):
        return [result.cpu().numpy()]
    if isinstance(result, np.ndarray):
        return [result]
    if isinstance(result, dict):
        return [x for k in sorted(result) for x in flat(result[k])]
    if isinstance(result, (tuple, list)):
        return [x for y in result for x in flat(y)]
    return [result]


def same(got, want):
    """Two flat results bit for bit: arrays by shape, item size and bytes (an int32 tensor holds a uint32 array's bytes), values by ==."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if isinstance(g, np.ndarray) != isinstance(w, np.ndarray):
            return False
        if isinstance(g, np.ndarray):
            if g.shape != w.shape or g.dtype.itemsize != w.dtype.itemsize or np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(w).tobytes():
                return False
        elif g != w and not (g != g and w != w):
            return False
    return True
