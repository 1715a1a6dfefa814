#!/usr/bin/env python3
"""tools/probe_shapes.py -- the large-batch probe (adl_bloom_probe_batch_device)
on several batch shapes, each answer array checked against the oracle on a
sample, timed with HIP events around the call (median of reps).  ADL_BLOOM_LIB
selects the library (tools/ab_lib.sh style A/B).  One JSON line per shape.

usage: python tools/probe_shapes.py [reps]
       python tools/probe_shapes.py [reps] --keys [--ab] [--queries N[,N...]]

--keys: the key shapes that are not 16-byte keys instead -- variable-length
keys (filters built from, and queries drawn from, adl_synth_varlen_*_device
with BASELINE configs[2]'s Zipf parameters) over 16 and 256 filters, and a
fixed stride of 24 bytes over 16 filters; half the queries are members of
their filter, in random order.  --ab: the same inputs timed with
ADL_BLOOM_PROBE_BATCH_VAR_MIN at 0 (the direct kernel) and at 1 (the binned
pipeline), in one process, interleaved rep by rep; both answer arrays are
checked against the oracle on the sample.  PROBE_SHAPES selects shapes here
too.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adlsm-tree_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import adlbloom as ab  # noqa: E402
import oracle as O  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and args[0].isdigit() else 5
torch.cuda.set_device(0)
KNOB = "ADL_BLOOM_PROBE_BATCH_VAR_MIN"
SAMPLE = 200_000


def gather(src, starts, lens):
    """The byte ranges src[starts[i] : starts[i] + lens[i]] packed back to back: (bytes + 16 of padding, offsets)."""
    off = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=src.device)
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1].item())
    idx = torch.repeat_interleave(starts - off[:-1], lens) + torch.arange(total, device=src.device)
    out = torch.zeros(total + 16, dtype=torch.uint8, device=src.device)
    out[:total] = src[idx]
    return out, off


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def key_shapes():
    """(name, filters, keys per filter): the shapes of --keys."""
    return [("zipf", 16, 1_000_000), ("zipf", 256, 100_000), ("stride24", 16, 1_000_000)]


def run_key_shape(name, F, per, n, ab_switch):
    g = torch.Generator(device="cuda")
    g.manual_seed(F * 1000 + n % 997)
    kb = np.arange(F + 1, dtype=np.uint64) * per
    fid = torch.randint(0, F, (n,), device="cuda", generator=g, dtype=torch.int64)
    member = torch.rand(n, device="cuda", generator=g) < 0.5
    pick = fid * per + torch.randint(0, per, (n,), device="cuda", generator=g, dtype=torch.int64)  # a key of filter fid
    if name == "zipf":
        kdata, koff = ab.synth_varlen(F * per, seed=0x5EED)
        bms, boff, nbytes = ab.build_segmented(kdata, kb, offsets=koff)
        qdata, qoff = ab.synth_varlen(n, seed=0xFEED)
        kbytes = int(koff[-1].item())
        src = torch.cat([kdata[:kbytes], qdata])
        starts = torch.where(member, koff[:-1][pick], kbytes + qoff[:-1])
        lens = torch.where(member, (koff[1:] - koff[:-1])[pick], qoff[1:] - qoff[:-1])
        q, offs = gather(src, starts, lens)
        del kdata, qdata, src, starts
        stride = 0
    else:
        stride = 24
        keys_t = torch.randint(0, 256, (F * per, stride), device="cuda", generator=g, dtype=torch.uint8)
        bms, boff, nbytes = ab.build_segmented(keys_t, kb)
        q = torch.randint(0, 256, (n, stride), device="cuda", generator=g, dtype=torch.uint8)
        q[member] = keys_t[pick[member]]
        offs = None
        del keys_t
    d_fid = fid.to(torch.int32)
    d_off = torch.from_numpy(np.asarray(boff, dtype=np.uint64).view(np.int64)).cuda()
    d_end = torch.from_numpy((np.asarray(boff, dtype=np.uint64) + np.asarray(nbytes, dtype=np.uint64)).view(np.int64)).cuda()
    # the sample's keys, filter ids and the filter bytes on the host, for the oracle
    idx = torch.from_numpy(np.sort(np.random.default_rng(F).choice(n, min(SAMPLE, n), replace=False))).cuda()
    h_bm = bms.cpu().numpy()
    h_off = np.asarray(boff, dtype=np.uint64)
    arena = np.concatenate([h_bm[int(h_off[f]):int(h_off[f]) + int(nbytes[f])] for f in range(F)] + [np.zeros(16, np.uint8)])
    aoff = np.concatenate([[0], np.cumsum(np.asarray(nbytes, dtype=np.uint64))]).astype(np.uint64)
    h_fid = d_fid[idx].cpu().numpy().view(np.uint32)
    if offs is None:
        want = O.probe_multi(q[idx].cpu().numpy(), h_fid, arena, aoff)
    else:
        sdata, soff = gather(q, offs[:-1][idx], (offs[1:] - offs[:-1])[idx])
        want = O.probe_multi(sdata.cpu().numpy(), h_fid, arena, aoff, offsets=soff.cpu().numpy().view(np.uint64))
    assert want[member[idx].cpu().numpy()].all()

    def call(out=None):
        return ab.probe_batch(q, d_fid, bms, d_off, offsets=offs, bitmap_end=d_end, out=out)

    modes = [("direct", "0"), ("binned", "1")] if ab_switch else [("default", None)]
    saved = os.environ.get(KNOB)
    ts, ok, outs = {m: [] for m, _ in modes}, {}, {}
    for r in range(reps + 1):  # rep 0 warms each mode up
        for m, v in modes:
            if v is not None:
                os.environ[KNOB] = v
                ab.reload_knobs()
            t, outs[m] = timed(lambda: call(outs.get(m)))
            if r:
                ts[m].append(t)
            else:
                ok[m] = bool(np.array_equal(outs[m][idx].cpu().numpy(), want))
    if ab_switch:
        if saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = saved
        ab.reload_knobs()
    line = {"keys": name, "key_stride": stride, "filters": F, "keys_per_filter": per, "queries": n,
            "mean_key_bytes": round(float((offs[-1].item() / n) if offs is not None else stride), 2)}
    for m, _ in modes:
        line[f"ms_{m}_median"] = round(float(np.median(ts[m])), 4)
        line[f"ms_{m}_all"] = [round(t, 4) for t in ts[m]]
        line[f"sampled_answers_equal_oracle_{m}"] = ok[m]
    if ab_switch:
        line["binned_over_direct"] = round(line["ms_binned_median"] / line["ms_direct_median"], 4)
    print(json.dumps(line), flush=True)


if "--keys" in args:
    sizes = [20_000_000]
    if "--queries" in args:
        sizes = [int(x) for x in args[args.index("--queries") + 1].split(",")]
    only = os.environ.get("PROBE_SHAPES")
    for si, (name, F, per) in enumerate(key_shapes()):
        if only and str(si) not in only.split(","):
            continue
        for n in sizes:
            run_key_shape(name, F, per, n, "--ab" in args)
            torch.cuda.empty_cache()
    sys.exit(0)

# (filters, keys per filter, queries, share of queries to filter 0 or None for uniform)
SHAPES = [(1, 1_000_000, 20_000_000, None), (16, 1_000_000, 20_000_000, None), (256, 100_000, 20_000_000, None),
          (4096, 5_000, 20_000_000, None), (64, 300_000, 20_000_000, 0.9)]
only = os.environ.get("PROBE_SHAPES")  # e.g. "3" or "0,3": indices into SHAPES
for si, (F, per, n, skew) in enumerate(SHAPES):
    if only and str(si) not in only.split(","):
        continue
    keys_t = ab.synth_keys16(F * per, seed=0x5EED, device="cuda")
    kb = np.arange(F + 1, dtype=np.uint64) * per
    bms, boff, nbytes = ab.build_segmented(keys_t, kb)
    rng = np.random.default_rng(F)
    if skew is None:
        fid = rng.integers(0, F, n).astype(np.uint32)
    else:
        fid = np.where(rng.random(n) < skew, 0, rng.integers(0, F, n)).astype(np.uint32)
    q = ab.synth_keys16(n, seed=0xFEED, device="cuda")
    d_fid = torch.from_numpy(fid.view(np.int32)).cuda()
    d_off = torch.from_numpy(np.asarray(boff, dtype=np.uint64).view(np.int64)).cuda()
    d_end = torch.from_numpy((np.asarray(boff, dtype=np.uint64) + np.asarray(nbytes, dtype=np.uint64)).view(np.int64)).cuda()
    out = ab.probe_batch(q, d_fid, bms, d_off, bitmap_end=d_end)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ab.probe_batch(q, d_fid, bms, d_off, bitmap_end=d_end, out=out)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    # sampled check against the oracle (the filter bytes and 200K queries)
    idx = rng.choice(n, 200_000, replace=False)
    h_bm = bms.cpu().numpy()
    h_off = np.asarray(boff, dtype=np.uint64)
    arena = np.concatenate([h_bm[int(h_off[f]):int(h_off[f]) + int(nbytes[f])] for f in range(F)] + [np.zeros(16, np.uint8)])
    aoff = np.concatenate([[0], np.cumsum(np.asarray(nbytes, dtype=np.uint64))]).astype(np.uint64)
    want = O.probe_multi(q.cpu().numpy()[idx], fid[idx], arena, aoff)
    ok = bool(np.array_equal(out.cpu().numpy()[idx], want))
    print(json.dumps({"filters": F, "keys_per_filter": per, "queries": n, "skew_to_filter0": skew,
                      "ms_median": round(float(np.median(ts)), 4), "ms_all": [round(t, 4) for t in ts],
                      "sampled_answers_equal_oracle": ok}), flush=True)
    del keys_t, bms, q, d_fid, out
    torch.cuda.empty_cache()
