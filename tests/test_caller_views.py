"""``caller_views.Slab`` -- the memory every test of tests/test_gpu_caller_views.py hands to the library -- held to its word on the CPU:
the residue asked for is the residue obtained, whatever the slab's own address; a residue that does not suit the element type is
refused; one byte written just before, just after and 255 bytes after an array is found and named, and so is a changed input; an
untouched slab gives no finding; no two arrays share a guard byte."""
import numpy as np
import pytest

from caller_views import FILL, GUARD, MARGIN, Finding, Slab

import torch  # noqa: E402

TYPES = {1: np.uint8, 4: np.int32, 8: np.int64}


def _slab(skew=0):
    """Three inputs and two outputs of the three element sizes, at residues off 16 bytes."""
    s = Slab("cpu", nbytes=1 << 16, skew=skew)
    rng = np.random.default_rng(1)
    v = {"text": s.place("text", rng.integers(0, 256, 1001).astype(np.uint8), np.uint8, 7, "in"),
         "ix": s.place("ix", rng.integers(-9, 9, 333).astype(np.int32), np.int32, 4, "in"),
         "out": s.place("out", 77, np.int32, 12, "out"),
         "wide": s.place("wide", rng.integers(-9, 9, (5, 13)), np.int64, 8, "in"),
         "theta": s.place("theta", (3, 11), np.float64, 0, "out")}
    return s, v


@pytest.mark.parametrize("skew", [0, 8, 24])
@pytest.mark.parametrize("size", [1, 4, 8])
def test_every_residue_asked_for_is_the_residue_obtained(size, skew):
    s = Slab("cpu", nbytes=1 << 16, skew=skew)
    assert s.base % 16 == (s._raw.data_ptr() + skew) % 16            # (24: the slab itself sits 8 bytes off a 16-byte boundary)
    for k, residue in enumerate(range(0, 16, size)):
        a = np.arange(1 + 3 * k, dtype=TYPES[size])
        for role, what in (("in", a), ("out", len(a))):
            v = s.place("%s%d" % (role, residue), what, TYPES[size], residue, role)
            assert v.data_ptr() % 16 == residue and v.is_contiguous() and v.element_size() == size and tuple(v.shape) == a.shape
            assert v.contiguous().data_ptr() == v.data_ptr()           # (what the wrappers of alntools_amd/ecb.py do to a tensor
            if size == 4:                                              #  leaves it where it is)
                assert v.to(torch.int32).data_ptr() == v.data_ptr()
            if role == "in":
                assert np.array_equal(v.numpy(), a)
            else:
                assert (v.numpy().view(np.uint8) == FILL).all()
    assert s.check() == []


@pytest.mark.parametrize("size,residue", [(4, 1), (4, 2), (4, 7), (8, 4), (8, 12), (8, 1), (1, 16), (4, 16), (1, -1)])
def test_a_residue_that_does_not_suit_the_type_is_refused(size, residue):
    s = Slab("cpu", nbytes=1 << 12)
    with pytest.raises(ValueError):
        s.place("x", np.zeros(4, TYPES[size]), TYPES[size], residue, "in")
    assert s.views == [] and s.check() == []


def test_bad_roles_names_and_a_full_slab_are_refused():
    s = Slab("cpu", nbytes=2048)
    with pytest.raises(ValueError):
        s.place("x", 4, np.int32, 0, "inout")
    s.place("x", 4, np.int32, 0, "out")
    with pytest.raises(ValueError):
        s.place("x", 4, np.int32, 0, "out")
    with pytest.raises(ValueError):
        s.place("y", 2048, np.uint8, 0, "out")                         # (the room is there; the guard bytes around it are not)
    assert [v.name for v in s.views] == ["x"] and s.check() == []


def test_an_untouched_slab_gives_no_finding_and_writes_inside_an_output_are_none():
    s, v = _slab()
    assert s.check() == []
    assert s.untouched("out") and s.untouched("theta")
    v["out"][:] = 3
    v["theta"][2, 10] = 1.5
    assert s.check() == []
    assert not s.untouched("out") and not s.untouched("theta")


@pytest.mark.parametrize("name", ["text", "ix", "out", "wide", "theta"])
@pytest.mark.parametrize("where,side", [(-1, "before"), (0, "after"), (255, "after"), (-MARGIN, "before")])
def test_one_byte_written_outside_a_view_is_found_and_named(name, where, side):
    s, v = _slab(skew=8)
    nbytes = v[name].numel() * v[name].element_size()
    off = v[name].data_ptr() - s.base
    at = off + (where if where < 0 else nbytes + where)
    assert s.mem[at] == GUARD
    s.mem[at] = GUARD ^ 1
    assert s.check() == [Finding(name, side, at - off)]
    s.mem[at] = GUARD
    assert s.check() == []


def test_the_first_offending_byte_is_the_one_reported():
    s, v = _slab()
    off = v["ix"].data_ptr() - s.base
    nbytes = 333 * 4
    for at in (off + nbytes + 40, off + nbytes + 3, off - 9, off - 200):
        s.mem[at] = 0
    assert s.check() == [Finding("ix", "before", -200), Finding("ix", "after", nbytes + 3)]


@pytest.mark.parametrize("name,element", [("text", 1000), ("ix", 0), ("wide", 64)])
def test_a_changed_input_element_is_found_and_named(name, element):
    s, v = _slab()
    flat = v[name].view(-1)
    flat[element] = flat[element] + 1
    assert s.check() == [Finding(name, "input changed", element * flat.element_size())]


def test_an_output_that_was_frozen_is_watched_like_an_input():
    s, v = _slab()
    v["out"][:] = torch.arange(77, dtype=torch.int32)
    s.freeze("out")
    assert s.check() == []
    v["out"][76] = 0
    assert s.check() == [Finding("out", "input changed", 76 * 4)]


def test_two_views_never_share_guard_bytes():
    s, v = _slab(skew=8)
    owned = np.zeros(s.mem.numel(), np.int32)
    for view in s.views:
        (b0, b1), (a0, a1) = s.zones(view.name)
        assert b1 - b0 >= MARGIN and a1 - a0 >= MARGIN
        assert b1 == view.start == v[view.name].data_ptr() - s.base and a0 == view.start + view.nbytes
        owned[b0:b1] += 1
        owned[a0:a1] += 1
        owned[b1:a0] += 1
    assert (owned == 1).all()                                          # (every byte of the slab: one array's room or one array's guard)
    # a byte in the gap between two arrays is charged to exactly one of them
    (_, _), (a0, a1) = s.zones("ix")
    (b0, b1), _ = s.zones("out")
    assert a1 == b0
    s.mem[a1 - 1] = 0
    assert [f.name for f in s.check()] == ["ix"]
    s.mem[a1 - 1] = GUARD
    s.mem[b0] = 0
    assert [f.name for f in s.check()] == ["out"]
