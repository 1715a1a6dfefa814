"""CPU: adl_bloom_probe_batch_workspace_bytes for keys that are not 16-byte keys.

key_stride == 0 (variable-length keys, what adlbloom.probe_batch passes with
offsets) and a stride other than 16 take the tile-binned pipeline from
ADL_BLOOM_PROBE_BATCH_VAR_MIN queries on; their plan is the 16-byte plan plus
one array of n hash pairs.  The stride-16 sizes are the ones the library gave
before that array existed (constants below, recorded from that library).
Needs the built library, no GPU.
"""
import pytest

F, N = 8, 1 << 20
KNOB = "ADL_BLOOM_PROBE_BATCH_VAR_MIN"

# (n, filters, bits_per_key) -> adl_bloom_probe_batch_workspace_bytes(..., 16) before this array was added
STRIDE16 = {
    (1 << 20, 8, 10): 39773696,
    (1 << 20, 8, 3): 22406656,
    ((1 << 20) + 777, 1, 10): 39136512,
    (3_000_000, 256, 10): 139222016,
    (100_000_000, 256, 10): 3752984832,
    (5_000_000, 4096, 20): 1010283520,
    ((1 << 31) - 2, 16, 10): 79498836736,
}


@pytest.fixture(scope="module")
def wsb():
    import adlbloom

    return adlbloom.lib().adl_bloom_probe_batch_workspace_bytes


def round_up(v, a):
    return (v + a - 1) // a * a


@pytest.mark.parametrize("bpk", [10, 3])
@pytest.mark.parametrize("stride", [0, 24])
def test_plan_is_the_16_byte_plan_plus_the_pairs(wsb, knobs, bpk, stride):
    knobs.set(KNOB, 1)
    assert wsb(N, F, bpk, 16) > 256
    assert wsb(N, F, bpk, stride) == wsb(N, F, bpk, 16) + round_up(N * 8, 256)


@pytest.mark.parametrize("bpk", [10, 3])
@pytest.mark.parametrize("stride", [0, 24])
def test_monotone_in_n(wsb, knobs, bpk, stride):
    knobs.set(KNOB, 1)
    sizes = [wsb(n, F, bpk, stride) for n in (N, N + 1, N + 511, N + 512, N + 8192, 3 * N + 5, 50 * N, (1 << 31) - 2)]
    assert sizes[0] > 256 and sizes == sorted(sizes), sizes


@pytest.mark.parametrize("bpk", [10, 3])
@pytest.mark.parametrize("stride", [0, 24])
def test_direct_outside_the_pipeline(wsb, knobs, bpk, stride):
    knobs.set(KNOB, 1)
    assert wsb(N - 1, F, bpk, stride) == 256
    assert wsb(N, 0, bpk, stride) == 256
    assert wsb(N, 4096, bpk, stride) > 256
    assert wsb(N, 4097, bpk, stride) == 256
    assert wsb((1 << 31) - 2, F, bpk, stride) > 256
    assert wsb((1 << 31) - 1, F, bpk, stride) == 256


@pytest.mark.parametrize("bpk", [10, 3])
@pytest.mark.parametrize("stride", [0, 24])
def test_knob_zero_is_never(wsb, knobs, bpk, stride):
    knobs.set(KNOB, 0)
    for n in (N, 20_000_000, (1 << 31) - 2):
        assert wsb(n, F, bpk, stride) == 256
    assert wsb(N, F, bpk, 16) > 256  # the knob is not about 16-byte keys


def test_knob_is_a_threshold(wsb, knobs):
    knobs.set(KNOB, 5_000_000)
    assert wsb(4_999_999, F, 10, 0) == 256 and wsb(5_000_000, F, 10, 0) > 256
    knobs.set(KNOB, 1000)  # 1 .. 2^20 mean 2^20
    assert wsb(N - 1, F, 10, 24) == 256 and wsb(N, F, 10, 24) > 256


@pytest.mark.parametrize("knob", [None, 0, 1])
def test_stride_16_sizes_unchanged(wsb, knobs, knob):
    if knob is None:
        knobs.unset(KNOB)
    else:
        knobs.set(KNOB, knob)
    for (n, f, bpk), want in STRIDE16.items():
        assert wsb(n, f, bpk, 16) == want, (n, f, bpk)
