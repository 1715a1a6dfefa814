#!/usr/bin/env python3
"""The streamed filter build against the parent commit's host-to-host build
("Streamed build").  Needs a GPU and a build of the parent commit.

  python tools/stream_build_ab.py [OUTDIR] --parent DIR [--reps N] [--shapes a,b,..]

DIR holds the parent's build (DIR/adlsm-tree_amd/lib/libadlbloom.so and
bin/sstable_test); the comparison is always against that library, never
against this tree's.  Every measurement is a process of its own (one library
per process); the configurations are interleaved, REPS rounds (default 5, at
least 5), and the tables give the median of the rounds with their min-max.

Shapes: k16 (configs[1]: 10 M x 16 B keys), var (configs[2]: 10 M Zipf-length
keys), mem (a 100 000-key memtable of 16 B keys), and sstable_test pipebench's
two shapes (8 x 100 K, 4 x 1 M entries) with ADL_BLOOM_STREAM_BUILD off and on.

Figures per shape, bits_per_key 10:
  parent  adl_bloom_build, keys in pageable host memory to bitmap in host memory
  (a)     streamed Final latency: from the last append's return to the bitmap in host memory
  (b)     total: the sum of the append calls' wall time plus (a)
  (c)     pass A + pass B of the device-resident finish against the parent's
          adl_bloom_build_device pair, the repeated-pair table off and on
  (d)     device bytes held per key
  (e)     (a), (b) at ADL_BLOOM_STREAM_BATCH_KEYS-sized appends of 4 096, 65 536, 1 048 576 keys
JSON lines go to OUTDIR/stream_build_ab.jsonl, the tables to OUTDIR/summary.txt
(OUTDIR defaults to profiles/stream_build)."""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"k16": 10_000_000, "var": 10_000_000, "mem": 100_000}
BATCHES = (4096, 65536, 1048576)
PIPE = ((100_000, 8), (1_000_000, 4))
WARM = 3   # discarded runs per process: the first allocates the thread's staging and workspace, and the parent's
           # build still ran a quarter slower in its second run than from the third on
ITERS = 5
BPK = 10


def spread(v, fmt="%.3f"):
    return (fmt + " (" + fmt + "-" + fmt + ")") % (statistics.median(v), min(v), max(v))


# ---------------------------------------------------------------- workers
def _sigs(L):
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    L.adl_synth_keys16_device.argtypes = [vp, u64, u64, u64, vp]
    L.adl_synth_varlen_lengths_device.argtypes = [vp, u64, u64, ctypes.c_double, vp]
    L.adl_synth_varlen_fill_device.argtypes = [vp, u64, u64, vp]
    L.adl_bloom_build.argtypes = [vp, vp, u64, u32, i32, vp, vp]
    L.adl_bloom_build_device.argtypes = [vp, vp, u64, u32, i32, vp, vp, u64, vp]
    L.adl_bloom_build_workspace_bytes.argtypes = [vp, u32, i32]
    L.adl_bloom_build_workspace_bytes.restype = u64
    L.adl_bloom_bitmap_bytes.argtypes = [u64, i32]
    L.adl_bloom_bitmap_bytes.restype = u64
    L.adl_bloom_profile_enable.argtypes = [u32]
    L.adl_bloom_profile_each.argtypes = [ctypes.POINTER(ctypes.c_double), u32, ctypes.POINTER(u32)]


def _keys(L, shape, n):
    """(device keys, device offsets | None, host keys, host offsets | None, stride), made by the library under test."""
    import torch

    if shape == "var":
        lengths = torch.empty(n, dtype=torch.int32, device="cuda")
        assert L.adl_synth_varlen_lengths_device(lengths.data_ptr(), 0x5EED, n, 1.1, None) == 0
        offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        offs[1:] = torch.cumsum(lengths.to(torch.int64), 0)
        total = int(offs[-1].item())
        data = torch.empty(((total + 15) // 16) * 16 + 16, dtype=torch.uint8, device="cuda")
        assert L.adl_synth_varlen_fill_device(data.data_ptr(), 0x5EED, total, None) == 0
        torch.cuda.synchronize()
        return data, offs, data.cpu().numpy(), offs.cpu().numpy().view("uint64"), 0
    data = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    assert L.adl_synth_keys16_device(data.data_ptr(), 0x5EED, 0, n, None) == 0
    torch.cuda.synchronize()
    return data, None, data.cpu().numpy(), None, 16


def _kernel_pair(L, run, reps=4):
    """pass A + pass B (ms) of `run()`'s launch pairs, the best of `reps` after a warm-up."""
    import torch

    run()
    torch.cuda.synchronize()
    assert L.adl_bloom_profile_enable(64) == 0
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    ms = (ctypes.c_double * 128)()
    pairs = ctypes.c_uint32()
    assert L.adl_bloom_profile_each(ms, 64, ctypes.byref(pairs)) == 0
    per = pairs.value // reps
    tot = [sum(ms[2 * (r * per + i)] + ms[2 * (r * per + i) + 1] for i in range(per)) for r in range(reps)]
    return min(tot)


def worker_parent(libpath, shape):
    import numpy as np
    import torch

    L = ctypes.CDLL(libpath)
    _sigs(L)
    n = SHAPES[shape]
    dk, do, hk, ho, stride = _keys(L, shape, n)
    nbytes = L.adl_bloom_bitmap_bytes(n, BPK)
    out = np.empty(nbytes, dtype=np.uint8)
    times = []
    for it in range(WARM + ITERS):
        t0 = time.perf_counter()
        rc = L.adl_bloom_build(hk.ctypes.data, None if ho is None else ho.ctypes.data, n, stride, BPK, out.ctypes.data, None)
        t1 = time.perf_counter()
        assert rc == 0, rc
        if it >= WARM:
            times.append((t1 - t0) * 1e3)
    cnt = np.array([n], dtype=np.uint64)
    ws_bytes = L.adl_bloom_build_workspace_bytes(cnt.ctypes.data, 1, BPK)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    bm = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    pair = _kernel_pair(L, lambda: L.adl_bloom_build_device(dk.data_ptr(), None if do is None else do.data_ptr(), n, stride,
                                                            BPK, bm.data_ptr(), ws.data_ptr(), ws_bytes, None))
    print(json.dumps({"side": "parent", "shape": shape, "n": n, "host_to_host_ms": times, "kernel_pair_ms": pair,
                      "checksum": int(out.astype(np.uint64).sum())}))


def worker_this(shape, batch):
    sys.path[:0] = [os.path.join(ROOT, "adlsm-tree_amd")]
    import numpy as np
    import torch

    import adlbloom as A

    L = A.lib()
    n = SHAPES[shape]
    dk, do, hk, ho, stride = _keys(L, shape, n)
    nbytes = A.bitmap_bytes(n, BPK)
    out = np.empty(nbytes, dtype=np.uint8)
    off = np.zeros(1, dtype=np.uint64)
    sb = A.StreamBuilder(reserve_keys=n)
    st = torch.cuda.Stream()
    edges = list(range(0, n, batch)) + [n]
    final_ms, total_ms, append_ms = [], [], []
    for it in range(WARM + ITERS):
        sb.reset()
        app = 0.0
        for a, b in zip(edges, edges[1:]):
            t0 = time.perf_counter()
            if ho is None:
                sb.append(hk[a:b], stream=st)
            else:
                sb.append(hk, ho[a:b + 1], stream=st)
            app += time.perf_counter() - t0
        t1 = time.perf_counter()
        sb.finish_host(out, off, BPK, stream=st)
        t2 = time.perf_counter()
        if it >= WARM:
            final_ms.append((t2 - t1) * 1e3)
            append_ms.append(app * 1e3)
            total_ms.append((app + t2 - t1) * 1e3)
    res = {"side": "this", "shape": shape, "n": n, "batch_keys": batch, "final_ms": final_ms, "append_ms": append_ms,
           "total_ms": total_ms, "device_bytes_per_key": 8.0, "checksum": int(out.astype(np.uint64).sum())}
    if batch == BATCHES[1]:  # the device-resident finish's kernels, once per round
        sb.reset()
        sb.append(dk, do)
        ws_bytes = sb.workspace_bytes(BPK)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        bm = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
        for name, val in (("off", "0"), ("on", "1")):
            os.environ["ADL_BLOOM_STREAM_HASH_DEDUP"] = val
            A.reload_knobs()
            res["kernel_pair_ms_dedup_" + name] = _kernel_pair(
                L, lambda: L.adl_bloom_stream_finish_device(sb._h, BPK, 0, bm.data_ptr(), off.ctypes.data, ws.data_ptr(),
                                                            ws_bytes, None))
    sb.close()
    print(json.dumps(res))


# ---------------------------------------------------------------- driver
def main(argv):
    if len(argv) > 1 and argv[1] == "--worker":
        if argv[2] == "parent":
            worker_parent(argv[3], argv[4])
        else:
            worker_this(argv[3], int(argv[4]))
        return 0
    out, parent, reps, shapes = os.path.join(ROOT, "profiles", "stream_build"), None, 5, list(SHAPES) + ["pipe"]
    args = argv[1:]
    while args:
        a = args.pop(0)
        if a == "--parent":
            parent = os.path.abspath(args.pop(0))
        elif a == "--reps":
            reps = max(5, int(args.pop(0)))
        elif a == "--shapes":
            shapes = args.pop(0).split(",")
        else:
            out = a
    if not parent:
        print(__doc__)
        return 2
    plib = os.path.join(parent, "adlsm-tree_amd", "lib", "libadlbloom.so")
    os.makedirs(out, exist_ok=True)
    rows = []

    def run(cmd, env_extra, tag):
        env = {k: v for k, v in os.environ.items() if not k.startswith("ADL_BLOOM_STREAM")}
        env.update(env_extra)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
        if r.returncode != 0:
            print("FAILED", tag, r.returncode, r.stdout[-500:], r.stderr[-2000:])
            return None
        d = json.loads(r.stdout.splitlines()[-1])
        d.update(tag)
        rows.append(d)
        log.write(json.dumps(d) + "\n")
        log.flush()
        return d

    me = [sys.executable, os.path.abspath(__file__), "--worker"]
    with open(os.path.join(out, "stream_build_ab.jsonl"), "w") as log:
        for rnd in range(reps):  # interleaved: a drift of the machine meets every configuration alike
            for shape in [s for s in shapes if s in SHAPES]:
                if run(me + ["parent", plib, shape], {}, {"round": rnd}) is None:
                    return 1  # nothing more on the GPU after a failure
                for b in BATCHES:
                    if run(me + ["this", shape, str(b)], {}, {"round": rnd}) is None:
                        return 1
            if "pipe" in shapes:
                for n, t in PIPE:
                    for who, root, env in (("parent", parent, {}), ("this, streaming off", ROOT, {}),
                                           ("this, streaming on", ROOT, {"ADL_BLOOM_STREAM_BUILD": "1"})):
                        exe = os.path.join(root, "adlsm-tree_amd", "bin", "sstable_test")
                        if run([exe, "pipebench", str(n), str(t)], env, {"round": rnd, "side": who, "shape": "pipe"}) is None:
                            return 1

    lines = ["streamed build against the parent's host-to-host adl_bloom_build, bits_per_key %d, %d interleaved rounds,"
             % (BPK, reps), "median (min-max) over the rounds of each process's median of %d runs after %d warm-up runs; ms" % (ITERS, WARM), ""]
    med = statistics.median
    for shape in [s for s in shapes if s in SHAPES]:
        par = [r for r in rows if r["shape"] == shape and r["side"] == "parent"]
        lines.append("%s, n = %d" % (shape, SHAPES[shape]))
        lines.append("  parent host to host            %s" % spread([med(r["host_to_host_ms"]) for r in par]))
        for b in BATCHES:
            th = [r for r in rows if r["shape"] == shape and r["side"] == "this" and r["batch_keys"] == b]
            lines.append("  appends of %7d keys: (a) Final %s   appends %s   (b) total %s" % (
                b, spread([med(r["final_ms"]) for r in th]), spread([med(r["append_ms"]) for r in th]),
                spread([med(r["total_ms"]) for r in th])))
            assert len({r["checksum"] for r in th + par}) == 1, "the bitmaps differ"
        th = [r for r in rows if r["shape"] == shape and r["side"] == "this" and "kernel_pair_ms_dedup_on" in r]
        lines.append("  (c) pass A + B: parent build_device %s   finish, table off %s   on %s" % (
            spread([r["kernel_pair_ms"] for r in par]), spread([r["kernel_pair_ms_dedup_off"] for r in th]),
            spread([r["kernel_pair_ms_dedup_on"] for r in th])))
        lines.append("  (d) device bytes per key: 8 (the pair store) against %.1f of key bytes"
                     % {"k16": 16.0, "mem": 16.0, "var": 48.0}[shape])
        lines.append("")
    for n, t in PIPE if "pipe" in shapes else ():
        lines.append("sstable_test pipebench, %d tables of %d entries (s)" % (t, n))
        for who in ("parent", "this, streaming off", "this, streaming on"):
            pr = [r for r in rows if r["shape"] == "pipe" and r["side"] == who and r["entries_per_table"] == n]
            lines.append("  %-20s Final per table %s   BeginFinal/EndFinal %s" % (
                who, spread([r["final_per_table_s"] for r in pr]), spread([r["overlapped_s"] for r in pr])))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(out, "summary.txt"), "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
