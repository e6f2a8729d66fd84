"""Poisoned, fenced outputs for the GPU parity tests.

Every wrapper method of SvtHipDsp begins with ``t = self.torch`` and allocates its outputs with ``t.empty`` /
``t.empty_like``.  While the ``poisoned_outputs`` fixture is active, ``dsp.torch`` is a PoisonTorch: those two calls hand out
the middle of a larger byte buffer that is filled with one byte value, everything else is the real torch module.

  * an entry the kernel never wrote still reads as the fill pattern (an int32 as 0x5A5A5A5A), so the test's existing
    comparison with the oracle fails: nothing a previous call left in a recycled block can stand in for the answer;
  * the GUARD bytes before and after the output must still hold the fill byte when the test ends (check_guards).

A test module switches this on by importing the fixture by name:

    from poison import poisoned_outputs  # noqa: F401

The fill byte is 0x5A.  A module that compares 8-bit samples, where one fill value can be a true pixel, ends with

    poison.add_second_fill(globals())

which gives each of its tests a twin ``<name>_fillA5`` that runs with 0xA5.  A module allocates the outputs it passes in
itself with ``poison.tensor(shape, dtype, device)``, and tests that compare two device results with each other call
``poison.assert_written`` on them as well.

What the fence does not see: it catches a contiguous overrun of up to GUARD bytes and any write into the guards, not a
stray write further away.  Requests above CAP bytes, requests for another device than the one under test, and requests made
while the current stream is capturing a graph (the fill would become a graph node) go to the real ``empty`` untouched.
"""
import contextlib
import types

import pytest

GUARD = 4096            # a multiple of every element size and of the kernels' 16-byte alignment needs
CAP = 256 << 20         # larger requests are not poisoned (spacers of alloc_spread, the full-size working sets)
FILLS = (0x5A, 0xA5)

_active = None          # the PoisonTorch of the running test (what tensor() and check_guards() use)


class PoisonTorch:
    """Forwards every attribute to the real torch module except ``empty`` and ``empty_like``."""

    def __init__(self, real_torch, fill, device=None, cap=CAP):
        self._real = real_torch
        self.fill_byte = int(fill) & 0xFF
        self.cap_bytes = cap
        self.target = real_torch.device(device) if device is not None else None      # the GPU under test
        self.records = []                                                             # (base, nbytes) per allocation
        self.views = []                                                               # (shape, dtype) of the same

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _is_target(self, dev):
        if dev.type == "cpu":
            return True
        d = self.target
        return d is not None and dev.type == d.type and (dev.index is None or d.index is None or dev.index == d.index)

    def _guarded(self, shape, dtype, device):
        """the guarded, filled allocation, or None where the request passes through"""
        real = self._real
        dev = real.device(device) if device is not None else real.empty(0).device
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * real.empty((), dtype=dtype).element_size()
        if not self._is_target(dev) or nbytes > self.cap_bytes:
            return None
        if dev.type == "cuda" and real.cuda.is_current_stream_capturing():
            return None
        base = real.full((GUARD + nbytes + GUARD,), self.fill_byte, dtype=real.uint8, device=dev)
        self.records.append((base, nbytes))
        self.views.append((shape, dtype))
        return base[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def empty(self, *size, dtype=None, device=None, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list)) else size
        out = None if kw else self._guarded(shape, dtype if dtype is not None else self._real.get_default_dtype(), device)
        return out if out is not None else self._real.empty(*size, dtype=dtype, device=device, **kw)

    def empty_like(self, x, dtype=None, device=None, **kw):
        out = None if kw else self._guarded(x.shape, dtype if dtype is not None else x.dtype, device if device is not None else x.device)
        return out if out is not None else self._real.empty_like(x, dtype=dtype, device=device, **kw)

    def check_guards(self):
        """every guard of every recorded allocation still holds the fill byte"""
        real = self._real
        if not self.records:
            return
        if any(b.is_cuda for b, _ in self.records):
            real.cuda.synchronize()
        by_dev = {}
        for b, n in self.records:
            by_dev.setdefault(b.device, []).extend((b[:GUARD], b[GUARD + n:]))
        if not any(bool((real.cat(g) != self.fill_byte).any()) for g in by_dev.values()):
            return
        for (b, n), (shape, dtype) in zip(self.records, self.views):
            for side, lo in (("before", 0), ("after", GUARD + n)):
                bad = (b[lo:lo + GUARD] != self.fill_byte).nonzero()
                if bad.numel():
                    k = lo + int(bad[0])
                    raise AssertionError(f"write outside an output: the guard {side} the {dtype} tensor of shape {shape} ({n} bytes) no longer "
                                         f"holds 0x{self.fill_byte:02X} at byte {k - GUARD} from the tensor's start "
                                         f"(guard byte {k - lo} of {GUARD}, now 0x{int(b[k]):02X})")


def check_guards():
    assert _active is not None, "poison.check_guards() outside the poisoned_outputs fixture"
    _active.check_guards()


def tensor(shape, dtype, device):
    """the same guarded, filled allocation for an output that a test allocates itself"""
    assert _active is not None, "poison.tensor() outside the poisoned_outputs fixture"
    return _active.empty(tuple(shape) if isinstance(shape, (tuple, list)) else (shape,), dtype=dtype, device=device)


def assert_guards(t, fill, what=""):
    """For a tensor from tensor() / a poisoned empty() that outlives the block it was allocated in (whose records the block
    drops when it ends): the GUARD bytes before and after it still hold the fill byte it was allocated with."""
    import torch
    raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    at, n = t.storage_offset() * t.element_size(), t.numel() * t.element_size()
    assert at == GUARD and raw.numel() >= GUARD + n + GUARD, f"{what}: not a guarded allocation"
    assert bool((raw[:GUARD] == fill).all()) and bool((raw[GUARD + n:GUARD + n + GUARD] == fill).all()), f"write outside the output {what}"


def fill_value(dtype):
    """what an untouched element of a poisoned tensor of this torch dtype reads as (0x5A5A for int16, ...)"""
    assert _active is not None, "poison.fill_value() outside the poisoned_outputs fixture"
    return int(_active._real.full((8,), _active.fill_byte, dtype=_active._real.uint8).view(dtype)[0])


def assert_written(*outputs):
    """For comparisons of two device results with each other (kernel A against kernel B), where an entry that neither wrote
    would compare equal: no element of a 16-, 32- or 64-bit output still reads as the fill pattern.  Takes tensors, None and
    (nested) tuples / lists / dicts of them; 8-bit tensors are left out (the pattern is an ordinary sample value there)."""
    for o in outputs:
        if o is None:
            continue
        if isinstance(o, dict):
            assert_written(*o.values())
        elif isinstance(o, (tuple, list)):
            assert_written(*o)
        elif o.element_size() > 1 and not o.is_floating_point():
            left = int((o == fill_value(o.dtype)).sum())
            assert left == 0, f"{left} entries of the {o.dtype} output of shape {tuple(o.shape)} were never written"


@contextlib.contextmanager
def poisoned(dsp, fill=FILLS[0]):
    """dsp.torch is a PoisonTorch inside the block; the guards are checked when the block ends and dsp.torch is restored
    whatever happens"""
    global _active
    real, before = dsp.torch, _active
    proxy = PoisonTorch(real, fill, device=getattr(dsp, "device", None))
    dsp.torch = _active = proxy
    try:
        yield proxy
        proxy.check_guards()
    finally:
        dsp.torch, _active = real, before
        del proxy.records[:], proxy.views[:]


def fixture_body(dsp, fill):
    """what both fixtures run (a generator, so that it can be driven by hand as pytest drives a fixture)"""
    with poisoned(dsp, fill) as proxy:
        yield proxy


@pytest.fixture(autouse=True)
def poisoned_outputs(request, dsp):
    yield from fixture_body(dsp, getattr(request.function, "poison_fill", FILLS[0]))


def add_second_fill(namespace):
    """Last line of a module whose compared outputs are 8-bit samples (``poison.add_second_fill(globals())``): every test
    function the module defines gets a twin ``<name>_fillA5`` with the same body, marks and parameters that the fixture runs
    with the second fill byte.  A twin and not a parameter of the fixture: a fixture parameter would change the id of every
    existing test of the module."""
    for name, fn in list(namespace.items()):
        if name.startswith("test_") and isinstance(fn, types.FunctionType) and fn.__module__ == namespace["__name__"]:
            twin_name = f"{name}_fill{FILLS[1]:02X}"
            twin = types.FunctionType(fn.__code__, fn.__globals__, twin_name, fn.__defaults__, fn.__closure__)
            twin.__dict__.update(fn.__dict__)
            twin.__kwdefaults__, twin.__doc__, twin.__qualname__, twin.__module__ = fn.__kwdefaults__, fn.__doc__, twin_name, fn.__module__
            twin.poison_fill = FILLS[1]
            namespace[twin_name] = twin
