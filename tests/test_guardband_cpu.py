"""CPU: the guard-band helper itself (tests/guardband.py) on CPU tensors."""
import pytest

from guardband import Guarded, GuardBandError


@pytest.mark.parametrize("align,skew", [(1, 0), (4, 0), (8, 1), (8, 3), (16, 0), (256, 0)])
@pytest.mark.parametrize("nbytes", [0, 1, 17, 4097])
def test_placement_and_untouched(align, skew, nbytes):
    g = Guarded(nbytes, align, lead=64, tail=96, device="cpu", skew=skew)
    assert (g.ptr - skew) % align == 0 and (g.ptr - skew) % (2 * align) != 0
    assert g.view.numel() == nbytes and g.start >= 64 and g.buf.numel() == g.end + 96
    assert g.view.data_ptr() == g.ptr or nbytes == 0
    assert bool((g.view == 0xA5).all())
    g.view.fill_(0)  # the payload is the callee's to write
    g.check()


@pytest.mark.parametrize("where", ["lead_last", "tail_first", "lead_far", "tail_far"])
def test_one_flipped_byte_is_reported_with_its_offset(where):
    g = Guarded(100, 16, lead=64, tail=96, device="cpu")
    index, band, first = {
        "lead_last": (g.start - 1, "lead", -1),
        "tail_first": (g.end, "tail", 0),
        "lead_far": (0, "lead", -g.start),
        "tail_far": (g.end + 95, "tail", 95),
    }[where]
    g.buf[index] ^= 0xFF
    with pytest.raises(GuardBandError) as e:
        g.check()
    assert (e.value.band, e.value.count, e.value.first) == (band, 1, first)
    assert "1 byte(s)" in str(e.value)
    g.buf[index] ^= 0xFF
    g.check()


def test_count_and_first_of_several():
    g = Guarded(8, 8, lead=32, tail=32, device="cpu")
    g.buf[g.end + 3:g.end + 10] = 0
    with pytest.raises(GuardBandError) as e:
        g.check()
    assert (e.value.band, e.value.count, e.value.first) == ("tail", 7, 3)
