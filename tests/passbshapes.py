"""Build shapes whose filters have more chunks than pass B stages per batch
(bloom_tile_kernel's SEGB, adlsm-tree_amd/csrc/bloom_build.hip: 2048 segment
descriptors at one workgroup per CU, 1024 at two), shared by
tests/test_pass_b_batches_cpu.py, which proves through the `adl_bloom plan:`
line that every shape plans the chunk counts it is named for, and
tests/test_gpu_pass_b_batches.py, which builds them.

With ADL_BLOOM_CHUNK_KEYS=256 the plan picks C = 256 whenever the chunks of
all filters together fill whole rounds of the 256-workgroup pass-A grid and no
filter wastes much of its last chunk (pick_c: C = round_up(keys / (rounds *
256), 4), raised while the chunks exceed the rounds).  So every multi-filter
shape ends in a filler filter that brings the total to a multiple of 256
chunks, and a filter of W chunks holds (W - 1) * 256 + r keys, 1 <= r <= 256.
A single filter cannot be given an odd chunk count that way: the plan evens
its chunks out, which is why the odd counts ride in segmented builds.
"""
S = 2048   # SEGB at one pass-B workgroup per CU
S2 = 1024  # ... at two
CHUNK = 256
KNOB = {"ADL_BLOOM_CHUNK_KEYS": str(CHUNK)}

# keys in a filter's last chunk, taken in turn: full, one key, odd, one short, ...
_LAST = (256, 1, 129, 255, 7, 200, 64, 253)


def sizes_for(ws):
    """Key counts for filters of ws[f] chunks of 256 keys (0: empty; a filter
    named ONE holds a single key), then the filler that rounds the total up to
    a multiple of 256 chunks."""
    out = []
    for i, w in enumerate(ws):
        if w == 0:
            out.append(0)
        elif w is ONE:
            out.append(1)
        else:
            out.append((w - 1) * CHUNK + _LAST[i % len(_LAST)])
    return out


class _One(int):
    """The chunk count of a 1-key filter: 1, but the filter holds one key."""


ONE = _One(1)


def _filled(ws):
    ws = list(ws)
    ws.append(-sum(ws) % 256 or 256)
    return ws


class Shape:
    """sizes: keys per filter; chunks: the chunk count per filter the plan has
    to give; C, tl, claim, occ: the rest of the plan line; env: the knobs."""

    def __init__(self, chunks=None, sizes=None, C=CHUNK, tl=None, claim=False, occ=1, bpk=10, env=KNOB, keys="k16"):
        self.chunks = [int(w) for w in (_filled(chunks) if sizes is None else chunks)]
        self.sizes = sizes_for(_filled(chunks)) if sizes is None else list(sizes)
        self.C, self.tl, self.claim, self.occ, self.bpk, self.env, self.keys = C, tl, claim, occ, bpk, dict(env), keys
        self.dt = len(self.sizes) > 8  # descriptors from the device FilterTable

    @property
    def batches(self):
        """Segment batches of the filter with the most chunks."""
        segb = S if self.occ == 1 else S2
        return -(-max(self.chunks) // segb)


# a. the chunk-count sweep at 16-byte keys, bpk 10: every count of
# 1, 15, 16, 17, 255, 256, 257, S-1, S, S+1, S+15, S+16, S+17, 2S-1, 2S, 2S+1,
# 2S+17, 3S+1 in one of K1-K4 (at most 8 filters: kernarg descriptors) and
# again in one of D1, D2 (more than 8: the device FilterTable).  An empty and a
# 1-key filter stand directly after and directly before a multi-batch filter,
# in both orders.
_K1 = [2 * S + 1, 0, ONE, S + 1, 15, S - 1, 17]
_K2 = [S + 15, ONE, 0, S + 16, 16, S, 255]
_K3 = [3 * S + 1, 257, S + 17, 256]
_K4 = [2 * S - 1, 2 * S, 2 * S + 17]
_TIGHT = {**KNOB, "ADL_BLOOM_CLAIM": "2", "ADL_BLOOM_CLAIM_CAP": "101", "ADL_BLOOM_TILE_LOG2": "20"}
# b. the claim layout: S-1, S, S+1, 2S+1
_C1 = [S + 1, 0, ONE, 2 * S + 1, S - 1, S]
# c. other pass-A sources: S+1 and 2S+1
_P = [S + 1, 2 * S + 1]
# d. two pass-B workgroups per CU (bpk 0: k = 1, every filter one 56-bit tile):
# 1023, 1024, 1025, 1040, 2049, 3073; 8 and 16 filters, so that the pass-B grid
# is a multiple of 8 and the queued kernel runs
_M8 = [S2 + 1, 0, ONE, 2 * S2 + 1, S2 - 1, S2, S2 + 16]
_M16 = [3 * S2 + 1, ONE, 0, S2 + 1, S2 + 16, S2 - 1, S2, 2 * S2 + 1, ONE, 0, 15, 17, S2 + 1, 2 * S2 + 1, 255]

SHAPES = {
    "K1": Shape(_K1, tl=18),
    "K2": Shape(_K2, tl=18),
    "K3": Shape(_K3, tl=18),
    "K4": Shape(_K4, tl=18),
    "D1": Shape(_K1 + _K2, tl=18),
    "D2": Shape(_K4 + [0, ONE] + _K3, tl=18),
    "C1": Shape(_C1, tl=18, claim=True, env={**KNOB, "ADL_BLOOM_CLAIM": "2"}),
    "C1-tight": Shape(_C1, tl=20, claim=True, env=_TIGHT),
    "var": Shape(_P, tl=17, keys="var"),
    "bpk44": Shape(_P, tl=20, bpk=44),
    "stride24": Shape(_P, tl=17, keys="s24"),
    "M8": Shape(_M8, tl=10, bpk=0, occ=2, keys="marked"),
    "M16": Shape(_M16, tl=10, bpk=0, occ=2, keys="marked"),
    # d. one bpk-0 filter, whose chunks the plan evens out: 1023 and 1024 (one
    # batch of 1024, not and exactly full), 1261 (a second of 237), 2301 (three),
    # 3278 (four; the last of 206); and with no knob 9 M keys in 1280 chunks of 7032
    "B1023": Shape([1023], [1023 * 256], tl=10, bpk=0, occ=2, keys="marked"),
    "B1024": Shape([1024], [1024 * 256], tl=10, bpk=0, occ=2, keys="marked"),
    "B1261": Shape([1261], [1024 * 256 + 1], C=208, tl=10, bpk=0, occ=2, keys="marked"),
    "B2301": Shape([2301], [2049 * 256], C=228, tl=10, bpk=0, occ=2, keys="marked"),
    "B3278": Shape([3278], [3073 * 256], C=240, tl=10, bpk=0, occ=2, keys="marked"),
    "B9M": Shape([1280], [9_000_000], C=7032, tl=10, bpk=0, occ=2, keys="marked", env={}),
    # e. production plans, no knob: exactly one full batch; a second of 255; an
    # odd count just past 2048 beside a second filter (bpk 44: k = 30)
    "P2048": Shape([2048], [10_013_958], C=4892, tl=20, env={}),
    "P2303": Shape([2303], [12_000_000], C=5212, tl=20, env={}),
    "P2049+1023": Shape([2049, 1023], [2_458_200, 1_227_000], C=1200, tl=20, bpk=44, env={}),
}
