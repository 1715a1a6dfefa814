"""CPU: the comparison of the stream-ordering harness (tests/streamorder.py)."""
import numpy as np
import pytest

from streamorder import OUT_FILL, StreamOrderError, check, sptr


def test_equal_bytes_pass_whatever_the_dtype():
    want = np.arange(100, dtype=np.uint32)
    check(want.copy().view(np.uint8), want)
    check(np.zeros(0, np.uint8), np.zeros((0, 16), np.uint8))


def test_differences_are_counted_and_untouched_bytes_told_apart():
    want = np.arange(1, 65, dtype=np.uint8)  # (no byte equals 0xA5)
    got = want.copy()
    got[10:14] = OUT_FILL  # never written: the consumer ran first
    got[40] ^= 0xFF        # written from other inputs
    with pytest.raises(StreamOrderError) as e:
        check(got, want, "answers")
    assert (e.value.count, e.value.untouched, e.value.first) == (5, 4, 10)
    assert "answers: 5 of 64 byte(s)" in str(e.value)


def test_sizes_must_match():
    with pytest.raises(AssertionError):
        check(np.zeros(3, np.uint8), np.zeros(4, np.uint8))


def test_no_stream_is_null():
    assert sptr(None) is None
