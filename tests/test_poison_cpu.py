"""tests/poison.py on CPU tensors: what the proxy hands out, that both detections fire (an unwritten entry reads as the fill
pattern, a write into either guard fails check_guards and names the allocation), what passes through, and that the seam is
put back.  The stand-in below has what the fixture touches of an SvtHipDsp: a ``torch`` attribute."""
import numpy as np
import pytest
import torch

import poison
from poison import GUARD, PoisonTorch


class StandIn:
    """allocates as the wrapper methods do: t = self.torch, then t.empty / t.zeros"""

    def __init__(self):
        self.torch = torch

    def outputs(self, n):
        t = self.torch
        return t.empty((n, 4), dtype=t.int32), t.empty(n, dtype=t.int16, device="cpu"), t.empty_like(t.zeros((n, 3), dtype=t.uint8))


@pytest.mark.parametrize("fill", poison.FILLS)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64])
def test_views_are_contiguous_filled_and_fenced(fill, dtype):
    p = PoisonTorch(torch, fill)
    es = torch.empty((), dtype=dtype).element_size()
    pattern = int.from_bytes(bytes([fill]) * es, "little", signed=dtype != torch.uint8)
    for shape, make in (((3, 5), lambda: p.empty((3, 5), dtype=dtype)), ((3, 5), lambda: p.empty(3, 5, dtype=dtype, device="cpu")),
                        ((7,), lambda: p.empty(7, dtype=dtype)), ((2, 3, 4), lambda: p.empty_like(torch.zeros((2, 3, 4), dtype=dtype))),
                        ((0, 32, 32), lambda: p.empty((0, 32, 32), dtype=dtype)), ((), lambda: p.empty((), dtype=dtype))):
        got = make()
        assert tuple(got.shape) == shape and got.dtype == dtype and got.is_contiguous()
        assert got.storage_offset() * es == GUARD and got.data_ptr() % es == 0
        assert isinstance(got, p.Tensor)
        assert bool((got == pattern).all())
        base, nbytes = p.records[-1]
        assert nbytes == got.numel() * es and base.numel() == GUARD + nbytes + GUARD and base.dtype == torch.uint8
        assert (base.data_ptr() + GUARD == got.data_ptr() or not got.numel()) and bool((base == fill).all())
    assert len(p.records) == 6
    p.check_guards()


def test_an_unwritten_entry_reads_as_the_fill_pattern():
    p = PoisonTorch(torch, 0x5A)
    out = p.empty(37, dtype=torch.int32)
    out[:36] = torch.arange(36, dtype=torch.int32)              # a "kernel" that skips its last block
    expect = np.arange(37, dtype=np.int32)
    assert not np.array_equal(out.numpy(), expect)
    assert int(out[36]) == 0x5A5A5A5A and np.array_equal(out.numpy()[:36], expect[:36])
    eob = p.empty(5, dtype=torch.int16)                         # an expected 0 (zero-residual block) is not met by poison either
    assert int(eob[2]) == 0x5A5A != 0
    p.check_guards()                                            # nothing was written outside


@pytest.mark.parametrize("side", ["before", "after"])
def test_a_write_into_a_guard_fails_and_names_the_allocation(side):
    p = PoisonTorch(torch, 0x5A)
    p.empty((4, 4), dtype=torch.int64)
    out = p.empty((3, 85), dtype=torch.int32)
    p.empty(9, dtype=torch.uint8)
    base, nbytes = p.records[1]
    assert nbytes == 3 * 85 * 4
    out.zero_()
    p.check_guards()                                            # the whole output may be written
    base[GUARD + nbytes if side == "after" else GUARD - 1] = 0
    with pytest.raises(AssertionError) as e:
        p.check_guards()
    msg = str(e.value)
    assert "(3, 85)" in msg and "torch.int32" in msg and f"guard {side}" in msg
    assert (f"at byte {nbytes} " if side == "after" else "at byte -1 ") in msg


def test_a_write_at_the_far_end_of_a_guard_is_seen():
    p = PoisonTorch(torch, 0xA5)
    p.empty(3, dtype=torch.int16)
    base, nbytes = p.records[0]
    base[-1] = 0
    with pytest.raises(AssertionError, match=f"at byte {nbytes + GUARD - 1} "):
        p.check_guards()


def test_everything_else_passes_through():
    p = PoisonTorch(torch, 0x5A)
    for name in ("zeros", "zeros_like", "full", "from_numpy", "int16", "int32", "uint8", "Tensor", "cuda", "device", "cat", "fill"):
        assert getattr(p, name) is getattr(torch, name), name
    assert not p.zeros(4, dtype=p.int32).any() and p.zeros(4).storage_offset() == 0
    assert not p.records


def test_requests_that_are_not_poisoned():
    p = PoisonTorch(torch, 0x5A, cap=1 << 16)
    big = p.empty((1 << 16) + 1, dtype=torch.uint8)            # above the size cap
    assert big.storage_offset() == 0 and not p.records
    assert p.empty(1 << 16, dtype=torch.uint8).storage_offset() == GUARD and len(p.records) == 1
    meta = p.empty((4, 4), dtype=torch.int32, device="meta")    # neither the GPU under test nor "cpu"
    assert meta.device.type == "meta" and meta.storage_offset() == 0 and len(p.records) == 1
    assert poison.CAP == 256 << 20 and PoisonTorch(torch, 0).cap_bytes == poison.CAP


def test_the_seam_is_swapped_checked_and_restored():
    d = StandIn()
    with poison.poisoned(d, 0xA5) as proxy:
        assert d.torch is proxy
        a, b, c = d.outputs(3)
        assert len(proxy.records) == 3 and int(b[0]) == int.from_bytes(b"\xa5\xa5", "little", signed=True)
        own = poison.tensor((2, 2), torch.int32, "cpu")
        assert len(proxy.records) == 4 and own.storage_offset() * 4 == GUARD
        poison.check_guards()
    assert d.torch is torch and not proxy.records
    with pytest.raises(AssertionError):
        poison.tensor((1,), torch.uint8, "cpu")                 # no fixture active any more


def test_the_seam_is_restored_after_a_failing_body_and_after_a_damaged_guard():
    d = StandIn()
    with pytest.raises(ZeroDivisionError):
        with poison.poisoned(d):
            d.outputs(2)
            1 / 0
    assert d.torch is torch
    with pytest.raises(AssertionError, match="guard after"):
        with poison.poisoned(d) as proxy:
            d.outputs(2)
            base, nbytes = proxy.records[0]
            base[GUARD + nbytes] ^= 0xFF
    assert d.torch is torch and not proxy.records


def test_the_fixture_restores_the_seam_after_a_failing_test_body():
    """the fixture's own generator, driven as pytest drives it: a failing body is not thrown into it, teardown just resumes it"""
    d = StandIn()

    gen = poison.fixture_body(d, 0xA5)
    proxy = next(gen)
    assert d.torch is proxy and proxy.fill_byte == 0xA5
    try:
        d.outputs(1)
        assert False, "the test body fails"
    except AssertionError:
        pass
    with pytest.raises(StopIteration):
        next(gen)
    assert d.torch is torch


def test_fill_value_and_assert_written():
    d = StandIn()
    with poison.poisoned(d, 0xA5):
        assert poison.fill_value(torch.uint8) == 0xA5 and poison.fill_value(torch.int16) == -0x5A5B
        assert poison.fill_value(torch.int32) == int.from_bytes(b"\xa5" * 4, "little", signed=True)
        a, b, c = d.outputs(3)
        a.zero_(); b[:2] = 7
        poison.assert_written(a, None, {"x": (a, c)})            # c is 8-bit: not judged
        with pytest.raises(AssertionError, match="1 entries of the torch.int16 output of shape \\(3,\\)"):
            poison.assert_written([a, b])


def test_add_second_fill_makes_a_twin_of_every_test_of_the_module_only():
    def test_a(dsp, x=3):
        """doc"""
        return x + 1
    test_a.pytestmark = [pytest.mark.parametrize("x", [1, 2])]
    ns = {"__name__": __name__, "test_a": test_a, "test_imported": pytest.raises, "helper": test_a, "test_elsewhere": poison.tensor}
    poison.add_second_fill(ns)
    assert sorted(ns) == ["__name__", "helper", "test_a", "test_a_fillA5", "test_elsewhere", "test_imported"]
    twin = ns["test_a_fillA5"]
    assert twin is not test_a and twin.__name__ == "test_a_fillA5" and twin.poison_fill == 0xA5 and not hasattr(test_a, "poison_fill")
    assert twin.pytestmark is test_a.pytestmark and twin.__doc__ == "doc" and twin(None) == 4 and twin(None, x=7) == 8
