"""CPU: what tests/test_gpu_revision_scale.py builds its expectations from, held
against the oracle and numpy where no GPU is needed.

* the closed form of the disjoint level's candidate lists
  (revisionkeys.disjoint_list) equals oracle.level_candidates: every "m", "n"
  and "zz" key of 300 tables at seq 24, 25, 26 and INT64_MAX, and the tables
  around 256, 4 096 and 8 192 and the last one of 9 000; every key that starts
  with "d" has one t16 list per seq, and no key that does not has a
  candidate in the disjoint level;
* the torch reference of the grouping (revisionkeys.torch_plan) equals numpy's
  (test_read_plan_cpu.expected_plan) on test_gpu_read_plan._synthetic's cases;
* the comparers that run where the outputs live (revisionkeys.compare_hits,
  compare_plan, and test_gpu_level_index_scale.device_compare on global-id
  lists) report one corrupted entry with its index;
* the expected hit lists gathered from a truth table
  (revisionkeys.expected_hits) equal oracle.probe_multi on the expanded pairs.
Nothing here calls the library."""
import numpy as np
import pytest
import torch

import revisionkeys as rk
from test_gpu_level_index_scale import device_compare
from test_gpu_read_plan import _synthetic
from test_read_plan_cpu import expected_plan

SEQ_MAX = 2**63 - 1


# ------------------------------------------------------------------ the closed form
def test_closed_form_of_300_disjoint_tables(oracle):
    tables = rk.tables("d300")
    assert len(tables) == 300
    for seq in (24, 25, 26, SEQ_MAX):
        for i in range(300):
            for kind in rk.DISJOINT_KINDS:
                got = oracle.level_candidates(tables, rk.disjoint_key(i, kind), seq)
                assert got == rk.disjoint_list(i, kind), (seq, i, kind, got)


def test_closed_form_of_9000_disjoint_tables(oracle):
    T = 9000
    tables = rk.tables("d9000")
    for i in (0, 1, 255, 256, 257, 4095, 4096, 8191, 8192, T - 1):
        for kind in rk.DISJOINT_KINDS:
            for seq in (24, 26):
                got = oracle.level_candidates(tables, rk.disjoint_key(i, kind), seq)
                assert got == rk.disjoint_list(i, kind), (seq, i, kind, got)


def test_closed_form_of_keys_outside_the_disjoint_level(oracle):
    """No key of t16's pool that does not start with "d" has a candidate in the disjoint level."""
    others = [k for k in rk.pool(("t16",)) if not k.startswith(b"d")]
    assert len(others) >= 50 and any(k < b"d" for k in others) and any(k > b"e" for k in others)
    assert b"" in others and b"c\xff" < b"d" < b"d\x00" < b"e"
    for T, keys, seqs in ((300, others, (24, 25, 26, SEQ_MAX)), (9000, others[::6], (25,))):
        tables = rk.tables("d%d" % T)
        for seq in seqs:
            for k in keys:
                assert oracle.level_candidates(tables, k, seq) == rk.disjoint_list_of_other(k) == [], (T, seq, k)


def test_one_t16_list_for_every_d_key(oracle):
    """The lowest and the highest key that starts with "d" agree (asserted inside), and so do keys between."""
    t16 = rk.tables("t16")
    for seq in (24, 25, 26, SEQ_MAX):
        want = rk.t16_list_of_d(oracle, seq)
        assert want, "no t16 table covers the d keys: the last groups of the scale revisions would be empty"
        for k in (rk.disjoint_key(0, b"m"), rk.disjoint_key(65599, b"zz"), rk.disjoint_key(8192, b"n")):
            assert oracle.level_candidates(t16, k, seq) == want
        assert rk.scale_list(oracle, 9000, 8192, b"m", seq) == [8192] + [9000 + t for t in want]
        assert rk.scale_list(oracle, 9000, 8192, b"zz", seq) == [9000 + t for t in want]
    assert rk.table_base(rk.SCALE_REVISIONS["d8176"])[-1] == 8192
    assert rk.table_base(rk.SCALE_REVISIONS["d8177"])[-1] == 8193
    assert int(rk.table_base(rk.SCALE_REVISIONS["d65600"])[-1] - 1).bit_length() == 17


# ------------------------------------------------------------------ the grouping
@pytest.mark.parametrize("T", (2, 300, 65537))
@pytest.mark.parametrize("H", (0, 1, 65, 3 * 2048 + 17))
def test_torch_plan_equals_numpy(H, T):
    hb, ht = _synthetic(H, T, 1000 + H % 997)
    want_t, want_b, want_k = expected_plan(hb, ht)
    got_t, got_b, got_k = rk.torch_plan(torch, torch.from_numpy(hb.astype(np.int64)),
                                        torch.from_numpy(ht.astype(np.int64)))
    assert np.array_equal(got_t.numpy(), want_t.astype(np.int64))
    assert np.array_equal(got_b.numpy(), want_b.astype(np.int64))
    assert np.array_equal(got_k.numpy(), want_k.astype(np.int64))
    if H > 64 and T > 2:
        assert len(want_t) > 2 and not np.array_equal(want_k, np.sort(want_k))  # the sort did move entries


def test_gather_lists_equals_csr():
    rng = np.random.default_rng(3)
    lists = [list(rng.integers(0, 1000, int(n))) for n in rng.integers(0, 7, 40)] + [[]]
    sel = rng.integers(0, len(lists), 5000)
    begin, flat = rk.gather_lists(lists, sel)
    want_b, want_f = rk.csr([lists[int(i)] for i in sel])
    assert np.array_equal(begin, want_b) and np.array_equal(flat, want_f)


# ------------------------------------------------------------------ the comparers
def _i32(a):
    """A u32 numpy array as the int32 tensor a library output is viewed as."""
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy())


def test_plan_comparer_sees_one_wrong_entry():
    hb, ht = _synthetic(3 * 2048 + 17, 300, 5)
    ids = ht.copy()
    ids[::2] |= np.uint32(0x80000000)  # ids above 2^31: negative as int32
    want = rk.torch_plan(torch, torch.from_numpy(hb.astype(np.int64)), torch.from_numpy(ids.astype(np.int64)))
    G, H = want[0].numel(), want[2].numel()
    assert G > 100 and int(want[0].max()) > 2**31
    good = [_i32(w.numpy()) for w in want]
    rk.assert_same(rk.compare_plan(torch, good, want), "untouched")
    for part, at in ((1, 7), (0, 3), (2, H - 12), (0, G - 1), (1, G)):  # a begin entry, a table id, an entry key,
        got = [g.clone() for g in good]                                  # the last group (its id, its end)
        got[part][at] ^= 1
        cmp = rk.compare_plan(torch, got, want)
        name = ("table", "begin", "key")[part]
        assert (cmp[name + "_bad"], cmp[name + "_first"]) == (1, at), (part, at, cmp)
        assert sum(v for k, v in cmp.items() if k.endswith("_bad")) == 1
        with pytest.raises(AssertionError, match=name):
            rk.assert_same(cmp, "corrupted")
    # one group too few
    cmp = rk.compare_plan(torch, [good[0][:G - 1], good[1], good[2]], want)
    assert (cmp["table_bad"], cmp["table_first"]) == (G, G - 1)


def test_hits_comparer_sees_one_wrong_entry():
    rng = np.random.default_rng(9)
    K = 70000
    pb = np.concatenate([[0], np.cumsum(rng.integers(0, 4, K))]).astype(np.int64)
    pf = rng.integers(0, 40, int(pb[-1]))
    truth = torch.from_numpy(np.concatenate([rng.integers(0, 2, (64, 40)), np.zeros((64, 1), np.int64)], 1)
                             .astype(np.uint8))
    sel = torch.from_numpy(rng.integers(0, 64, K))
    hb, hf, _ = rk.expected_hits(torch, truth, sel, torch.from_numpy(pb), torch.from_numpy(pf))
    H = hf.numel()
    assert 0 < H < len(pf) and int(hb[-1]) == H
    good_b, good_f = _i32(hb.numpy()), _i32(hf.numpy())
    rk.assert_same(rk.compare_hits(torch, good_b, good_f, hb, hf), "untouched")
    for which, at in (("begin", 1), ("begin", K), ("filter", 0), ("filter", H - 1), ("filter", H // 2)):
        b, f = good_b.clone(), good_f.clone()
        (b if which == "begin" else f)[at] += 1
        cmp = rk.compare_hits(torch, b, f, hb, hf)
        assert (cmp[which + "_bad"], cmp[which + "_first"]) == (1, at), (which, at, cmp)
        assert cmp["begin_bad"] + cmp["filter_bad"] == 1


def test_device_compare_on_global_id_lists(oracle):
    """test_gpu_level_index_scale.device_compare with a revision's lists (global ids, lists longer than a
    level's): one wrong pair_table entry, one wrong pair_begin entry."""
    names = rk.REVISIONS["five"]
    pool = rk.pool(names)[:60]
    case = {"pool": pool, "want": {25: rk.revision_lists(oracle, names, pool, 25)}, "dev": {}}
    len_of, lists = (t.cpu() for t in _expect_cpu(case, 25))
    sel = torch.from_numpy(np.random.default_rng(1).integers(0, len(pool), 3000))
    begin, flat = rk.gather_lists(case["want"][25], sel.numpy())
    assert int(flat.max()) >= 19  # ids of the last level
    pb, pt = _i32(begin), _i32(flat)
    cmp = device_compare(torch, sel, len_of, lists, pb, pt, chunk=700)
    assert (cmp["total"], cmp["begin_bad"], cmp["table_bad"]) == (len(flat), 0, 0)
    pt[len(flat) - 5] += 1
    cmp = device_compare(torch, sel, len_of, lists, pb, pt, chunk=700)
    assert (cmp["table_bad"], cmp["table_first"], cmp["begin_bad"]) == (1, len(flat) - 5, 0)
    pt[len(flat) - 5] -= 1
    pb[2999] += 1
    cmp = device_compare(torch, sel, len_of, lists, pb, pt, chunk=700)
    assert (cmp["begin_bad"], cmp["begin_first"], cmp["table_bad"]) == (1, 2999, 0)


def _expect_cpu(case, seq):
    """test_gpu_level_index_scale._expect's tensors without a device."""
    lists = case["want"][seq]
    longest = max(1, max(len(x) for x in lists))
    m = np.full((len(lists), longest), -1, np.int32)
    for i, x in enumerate(lists):
        m[i, :len(x)] = x
    return torch.tensor([len(x) for x in lists], dtype=torch.int64), torch.from_numpy(m)


# ------------------------------------------------------------------ the expected answers
def test_expected_hits_equal_the_oracle_on_expanded_pairs(oracle):
    """5 000 keys drawn from 64, 0 to 3 pairs each over 40 filters (bits_per_key 3, 10 and 44 mixed, one filter
    empty) and ids >= 40: the gathered answers are oracle.probe_multi's on the expanded pairs."""
    rng = np.random.default_rng(21)
    pool, bitmaps, off, bpk = rk.filters_of_a_pool(oracle, rng, 64, 40, (3, 10, 44), None, empty=17)
    truth = rk.truth_table(oracle, pool, bitmaps, off, bpk)
    assert truth.shape == (64, 41) and not truth[:, 40].any() and not truth[:, 17].any()
    assert 0 < int(truth.sum()) < 64 * 39
    K = 5000
    sel = rng.integers(0, 64, K)
    pb = np.concatenate([[0], np.cumsum(rng.integers(0, 4, K))]).astype(np.int64)
    pf = rng.integers(0, 43, int(pb[-1]))  # 40, 41, 42: no such filter
    hb, hf, ans = rk.expected_hits(torch, torch.from_numpy(truth), torch.from_numpy(sel), torch.from_numpy(pb),
                                   torch.from_numpy(pf))
    owner = np.repeat(np.arange(K), np.diff(pb))
    want = np.zeros(len(pf), np.uint8)
    for b in (3, 10, 44):
        s = np.flatnonzero((pf < 40) & (pf != 17) & (bpk[np.minimum(pf, 39)] == b))
        want[s] = oracle.probe_multi([pool[int(sel[int(o)])] for o in owner[s]], pf[s], bitmaps, off, bits_per_key=b)
    assert np.array_equal(ans.numpy(), want)
    assert 0 < int(want.sum()) < len(pf)
    keep = want.astype(bool)
    assert np.array_equal(hf.numpy(), pf[keep])
    assert np.array_equal(hb.numpy(), np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=K))]))
