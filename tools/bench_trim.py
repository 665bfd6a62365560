#!/usr/bin/env python3
"""Times kh_trim_fixed_device against kh_median_counts_fixed_device on one GPU.

Both kernels issue the same table gathers (n_tables one-byte lookups per
k-mer), so the unchanged median query is the yardstick for the trim kernel.
The worker builds one table from the synthetic stream (C2 geometry by default:
Countgraph k=21, 4 x 1e9, 150-base reads), then runs both queries over the
same device-resident reads and the same table, in one process, interleaved:
`--warmup` untimed rounds, then `--repeats` timed rounds of (median, trim).
It prints the ms per pass of every round, their medians, and the `median` and
`trim` lines of the kernel stats, as one JSON line.

The GPU work runs in a child process under its own `timeout`; this process
never opens the device.

    python tools/bench_trim.py                      # C2, 50M reads
    python tools/bench_trim.py --reads 2000000 -x 1e8 --genome 3e6
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="Countgraph")
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("-x", type=float, default=1e9)
    ap.add_argument("--tables", type=int, default=4)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=float, default=0, help="genomic stream over a genome of this many bases")
    ap.add_argument("--cutoff", type=int, default=2)
    ap.add_argument("--below", action="store_true", help="trim_below_abundance")
    ap.add_argument("--no-gate", dest="gate", action="store_false", help="no median_at_least gate")
    ap.add_argument("--normalize-to", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the GPU child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    return a


def worker(a):
    import numpy as np
    import khmer_amd
    from khmer_amd import synth
    from khmer_amd._lib import lib, check, default_device
    dev = default_device()
    murmur = a.graph.endswith("table")
    g = getattr(khmer_amd, a.graph)(a.k, a.x, a.tables)
    if a.graph == "Countgraph":
        g.set_use_bigcount(True)

    def alloc(n):
        p = ctypes.c_void_p()
        check(lib.kh_device_malloc(dev, n, ctypes.byref(p)))
        return p

    n, L = a.reads, a.read_len
    words, koff = alloc((n * L // 32 + 2) * 8), alloc((n + 1) * 8)
    ks = min(a.k, 32)
    if a.genome:
        check(lib.kh_synth_genomic_device(dev, synth.SEED, int(a.genome), 0, n, L, ks, words, koff))
    else:
        check(lib.kh_synth_packed_device(dev, synth.SEED, 0, n, L, ks, words, koff))
    reads = words
    if murmur:
        reads = alloc(n * L + 64)
        check(lib.kh_unpack_ascii_device(dev, words, n * L, reads))
        check(lib.kh_consume_bytes_fixed_device(g._g, reads, n, L))
    else:
        check(lib.kh_consume_packed_fixed_device(g._g, words, n, L))
    med, avg, sd, at = alloc(n * 2 + 64), alloc(n * 4 + 64), alloc(n * 4 + 64), alloc(n * 4 + 64)

    def timed(fn):
        check(lib.kh_device_synchronize(dev))
        t = time.perf_counter()
        fn()
        check(lib.kh_device_synchronize(dev))
        return (time.perf_counter() - t) * 1e3

    def run_median():
        check(lib.kh_median_counts_fixed_device(g._g, reads, n, L, med, avg, sd))

    def run_trim():
        check(lib.kh_trim_fixed_device(g._g, reads, n, L, a.cutoff, 1 if a.below else 0, 1 if a.gate else 0,
                                       a.normalize_to, at))

    for _ in range(a.warmup):
        run_median()
        run_trim()
    check(lib.kh_graph_set_profiling(g._g, 1))
    ms_median, ms_trim = [], []
    for _ in range(a.repeats):
        ms_median.append(timed(run_median))
        ms_trim.append(timed(run_trim))
    buf = ctypes.create_string_buffer(1 << 16)
    got = ctypes.c_size_t()
    check(lib.kh_graph_kernel_stats(g._g, buf, len(buf), ctypes.byref(got)))
    stats = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split("\t")
        if name in ("median", "trim"):
            stats[name] = {"launches": int(cnt), "ms_total": float(ms), "ms_per_launch": float(ms) / max(int(cnt), 1)}
    sample = min(n, 1 << 20)
    host = ctypes.create_string_buffer(sample * 4)
    check(lib.kh_device_copy(dev, host, at, sample * 4))
    t_at = np.frombuffer(host.raw, dtype=np.uint32)
    nk = n * (L - a.k + 1)
    mm, mt = float(np.median(ms_median)), float(np.median(ms_trim))
    print(json.dumps({
        "workload": "%s k=%d %dx%.0e, %d x %d bp %sreads" % (a.graph, a.k, a.tables, a.x, n, L,
                                                           "genomic " if a.genome else ""),
        "cutoff": a.cutoff, "below": bool(a.below), "gate": bool(a.gate), "normalize_to": a.normalize_to,
        "ms_median_pass": [round(v, 2) for v in ms_median], "ms_trim_pass": [round(v, 2) for v in ms_trim],
        "median_pass_ms": round(mm, 2), "trim_pass_ms": round(mt, 2), "trim_over_median": round(mt / mm, 4),
        "trim_kmers_per_s": nk / (mt * 1e-3), "kernel_stats": stats,
        "trim_at_sample": {"reads": int(sample), "zero": int((t_at == 0).sum()), "full": int((t_at == L).sum())},
    }))


def main():
    a = parse_args()
    if a.worker:
        worker(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
