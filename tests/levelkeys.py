"""Keys the level-index tests share (tests/test_gpu_level_index.py,
tests/test_gpu_level_index_scale.py, tests/test_level_index_cpu.py): inner
keys, and boundary user keys with the features a comparison has to get right."""
import struct


def inner(user: bytes, seq: int, op: int) -> bytes:
    return user + struct.pack("<q", seq) + bytes([op])


def max_tail(i):
    """(seq, op) of table i's max inner key: every seq case against 24, 25, 26."""
    return [(24, 0), (25, 0), (25, 1), (26, 0), (26, 1), (24, 1)][i % 6]


P40 = bytes(range(0x30, 0x58))  # 40 bytes
assert len(P40) == 40


def special_users():
    """Boundary user keys with the features the comparison has to get right,
    sorted: the empty key, "ab" / "ab\\0", bytes >= 0x80 next to bytes < 0x80
    (a signed comparison orders them the other way), keys of exactly 16 and 24
    bytes, keys that share 16, 17 and 40 bytes, a 300-byte key."""
    s = {b"", b"ab", b"ab\0", b"ab\0\0", b"\x7f\x10", b"\x80\x01", b"\x7f\xff\x01", b"\xff", b"\xfe\x80",
         P40[:16], P40[:16] + b"\x80", P40[:16] + b"\x7f", P40[:17] + b"\x01", P40[:17] + b"\xf0", P40[:24],
         P40[:23] + b"\x81", P40, P40 + b"\0", P40 + b"\x80tail", P40 + b"\x7ftail", P40 + bytes(260),
         b"q" * 16, b"q" * 24, b"q" * 15 + b"\x90", b"q" * 16 + b"\x90" * 8}
    return sorted(s)
