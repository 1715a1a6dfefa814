"""tests/golden/make_filter_block_ref.py -- regenerate filter_block_ref.json.

Source (never the restatement under test): the reference's own
src/filter_block.cpp, src/murmur3_hash.cpp and src/encode.cpp, compiled
unmodified into oracle/_ref/libref_filter_block.so by oracle/Makefile (needs
the reference's sources; spdlog is replaced by oracle/spdlog_stand_in).  The
cases and their inputs are defined in tests/refcases.py; this script records
what the reference answers:

  * inputs: SHA-256 of every key set, so a test can prove it regenerated it;
  * builds: BloomFilter(bpk).Keys2Block -- the bitmap's length and SHA-256 --
    and IsKeyExists on max(n, 1000) non-members: packed bits in hex (LSB
    first) for 1000 queries, count and SHA-256 of the 0/1 answer bytes for
    more (that keeps the file small).  Every member answers 1: checked here,
    not stored;
  * blocks: FilterBlockWriter (Update, Keys2Block() per filter, Final) -- the
    block's length and SHA-256, those of each bitmap in it -- and
    FilterBlockReader::IsKeyExists for ids 0..F+1, packed bits in hex;
  * binned: the reader's answers to 2^20 + 777 queries over the 70-filter
    block, as one SHA-256 of the 0/1 answer bytes;
  * mutations: FilterBlockReader::Init's RC for each trailer mutation (-1: the
    harness refused, the reference would read outside the block) and, where
    it is OK, one character per (id, key): 0, 1, o (would read outside), z
    (an empty range: would divide by zero).

Run: python tests/golden/make_filter_block_ref.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402  (its loader only: no restated arithmetic is called here)
import refcases as C  # noqa: E402


def main():
    R = O.ref_filter_block_lib()
    if R is None:
        raise SystemExit("oracle/_ref/libref_filter_block.so missing: make -C oracle ref (needs the reference's sources)")
    ref = C.Ref(R)
    out = {"source": "reference src/filter_block.cpp + murmur3_hash.cpp + encode.cpp via oracle/_ref (unmodified)",
           "inputs": {}, "builds": {}, "blocks": {}, "mutations": {}}
    both, one_sided = 0, []

    for shape in C.SHAPES + ("fixed24",):
        mem = C.members(shape, C.NMAX)
        qs = C.queries(shape, C.NMAX)
        memset = {mem.key(i) for i in range(mem.n)}
        assert len(memset) == mem.n or shape == "varlen"  # (short random keys repeat)
        assert not any(qs.key(i) in memset for i in range(qs.n)), "a query is a member"
        ns = sorted({n for s, _, n in C.all_builds() if s == shape})
        out["inputs"][shape] = {"members": {str(n): C.members(shape, n).sha() for n in ns},
                                "queries": {str(q): C.queries(shape, q).sha() for q in sorted({max(n, C.MIN_QUERIES)
                                                                                                for n in ns})}}
        for bpk in sorted({b for s, b, _ in C.all_builds() if s == shape}):
            for n in ns:
                k = C.members(shape, n)
                bm = ref.keys2block(bpk, k)
                assert len(bm) == n * bpk + 7
                rec = {"bytes": len(bm), "sha256": C.sha(bm)}
                if n >= 1:
                    assert ref.probe(bpk, k, bm).all(), "a member answers 0"
                    q = C.queries(shape, n)
                    a = ref.probe(bpk, q, bm)
                    # The non-members of a case of 1000 keys or more must include both answers.  Two
                    # kinds of case cannot: bpk = 0 is a 56-bit bitmap, which that many keys fill (every
                    # query answers 1), and the printable keys spread so well that from bpk = 5 on a
                    # bitmap of (n * bpk + 7) * 8 bits gives no false positive at all.
                    if n >= 1000 and bpk == 0:
                        assert a.all() and bm == b"\xff" * 7
                        one_sided.append(C.build_id(shape, bpk, n))
                    elif n >= 1000 and shape == "ascii" and not 0 < int(a.sum()) < q.n:
                        assert bpk >= 5 and not a.any()
                        one_sided.append(C.build_id(shape, bpk, n))
                    elif n >= 1000:
                        assert 0 < int(a.sum()) < q.n, "the non-members must include both answers"
                        both += 1
                    if q.n <= C.MIN_QUERIES:
                        rec["q_bits"] = C.bits_hex(a)
                    else:
                        rec["q_ones"] = int(a.sum())
                        rec["q_sha256"] = C.sha(a.tobytes())
                out["builds"][C.build_id(shape, bpk, n)] = rec

    for name, (shape, bpk, counts) in C.BLOCKS.items():
        k = C.block_keys(name)
        blk = ref.block(bpk, k, counts)
        assert ref.reader_init(blk) == 0
        ids, q = C.block_queries(name)
        a = ref.reader_probe(blk, ids, q)
        assert ((a == 0) | (a == 1)).all()
        out["blocks"][name] = {"keys_sha256": k.sha(), "bytes": len(blk), "sha256": C.sha(blk),
                               "bitmaps": [[len(b), C.sha(b)] for b in C.split_block(blk)[0]],
                               "queries_sha256": C.sha(ids.astype("<i4").tobytes() + bytes.fromhex(q.sha())),
                               "answers": C.bits_hex(a)}

    fid, keys = C.binned_queries()
    blk = ref.block(C.BLOCKS[C.BINNED_BLOCK][1], C.block_keys(C.BINNED_BLOCK), C.BLOCKS[C.BINNED_BLOCK][2])
    qk = C.Keys(keys.reshape(-1), np.arange(C.BINNED_N + 1, dtype=np.uint64) * np.uint64(16))
    a = ref.reader_probe(blk, fid, qk)
    assert ((a == 0) | (a == 1)).all() and a[::2].all() and not a[1::2].all()
    out["binned"] = {"block": C.BINNED_BLOCK, "n": C.BINNED_N,
                     "queries_sha256": C.sha(fid.astype("<i4").tobytes() + keys.tobytes()),
                     "ones": int(a.sum()), "answers_sha256": C.sha(a.astype(np.uint8).tobytes())}

    k3, counts3 = C.base3()
    base = ref.block(C.BASE3_BPK, k3, counts3)
    cases = {}
    for name, blk in C.mutations(base).items():
        rc, ans = ref.mutation(blk)
        cases[name] = {"rc": rc, "answers": ans}
    out["mutations"] = {"base": {"bytes": len(base), "sha256": C.sha(base)}, "ids": list(C.MUT_IDS),
                        "keys": [k.hex() for k in C.MUT_KEYS], "cases": cases}

    print("cases of >= 1000 keys whose non-members give both answers:", both, "-- one answer only:", one_sided)
    with open(C.JSON_PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", C.JSON_PATH, os.path.getsize(C.JSON_PATH), "bytes;", len(out["builds"]), "builds,",
          len(out["blocks"]), "blocks,", len(cases), "mutations")


if __name__ == "__main__":
    main()
