#!/usr/bin/env python3
"""Times kh_normalize_by_median (digital normalization on the device) on one GPU.

The stream is the genomic synthetic one (khmer_amd/synth.py genomic_codes):
reads of `--read-len` bases sampled from a random genome of `--genome` bases.
Three conditions, each timed over `--repeats` batches of `--batch` reads:

  early       from an empty table: almost every read is kept (and consumed);
  mid         the table first takes `--mid-coverage`-fold coverage of the
              genome (device-generated reads, plain consume): part of the
              reads is kept, the fixed point has work to do;
  saturated   after `--coverage`-fold coverage almost every read is rejected
              by the cheap pass.

For every `--window` value (units per window, 0 = the library's default) it
prints reads per second, the kept fraction and the mean fixed-point iterations
per window.  Two baselines run over the first `--baseline-reads` reads of the
same batches: the per-read median_at_least + consume loop of the Python API
(one device round trip per call), and the same loop on the CPU oracle
(get_median_count >= C, which is the same test, and consume).  One JSON line.

The GPU work runs in a child process under its own `timeout`; this process
never opens the device.

    python tools/bench_diginorm.py
    python tools/bench_diginorm.py --window 0,1024,65536 --cutoff 20
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
    ap.add_argument("-k", type=int, default=21)
    ap.add_argument("-x", type=float, default=1e8)
    ap.add_argument("--tables", type=int, default=4)
    ap.add_argument("--genome", type=float, default=2e7)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--cutoff", type=int, default=20)
    ap.add_argument("--batch", type=int, default=65536, help="reads per call")
    ap.add_argument("--repeats", type=int, default=5, help="timed batches per condition")
    ap.add_argument("--coverage", type=float, default=60, help="coverage consumed before the saturated condition")
    ap.add_argument("--mid-coverage", type=float, default=25, help="coverage consumed before the mid condition")
    ap.add_argument("--window", default="0", help="comma-separated window sizes in units (0: default)")
    ap.add_argument("--max-iters", type=int, default=0)
    ap.add_argument("--baseline-reads", type=int, default=2000)
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
    from oracle import oracle as O
    dev = default_device()
    L, B, G = a.read_len, a.batch, int(a.genome)
    primes = khmer_amd.get_n_primes_near_x(a.tables, a.x)

    # the timed batches: reads 0 .. repeats * B of the genomic stream
    batches = [synth.genomic_batch(i * B, B, L, G) for i in range(a.repeats)]
    offsets = [(ctypes.c_uint64 * (B + 1))(*[int(v) for v in offs]) for _, offs in batches]

    def new_graph():
        return khmer_amd.Countgraph(a.k, 0, 0, primes=primes)

    def saturate(g, coverage):
        """coverage-fold coverage of the genome from reads far behind the timed ones"""
        n = int(coverage * G / L)
        if not n:
            return
        words, koff = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.kh_device_malloc(dev, (n * L // 32 + 2) * 8, ctypes.byref(words)))
        check(lib.kh_device_malloc(dev, (n + 1) * 8, ctypes.byref(koff)))
        check(lib.kh_synth_genomic_device(dev, synth.SEED, G, 100000000, n, L, min(a.k, 32), words, koff))
        check(lib.kh_consume_packed_fixed_device(g._g, words, n, L))
        check(lib.kh_device_free(dev, words))
        check(lib.kh_device_free(dev, koff))

    def run_call(g, window):
        """every batch through kh_normalize_by_median: per-call seconds, stats, kept reads"""
        keep, status = (ctypes.c_uint8 * B)(), (ctypes.c_uint8 * B)()
        stats = (ctypes.c_uint64 * 4)()
        secs, tot, kept = [], [0, 0, 0, 0], 0
        for (blob, _), offs in zip(batches, offsets):
            check(lib.kh_device_synchronize(dev))
            t = time.perf_counter()
            check(lib.kh_normalize_by_median(g._g, blob, offs, B, None, a.cutoff, window, a.max_iters, keep, status,
                                             stats))
            secs.append(time.perf_counter() - t)
            tot = [x + y for x, y in zip(tot, stats)]
            kept += sum(keep)
        med = float(np.median(secs))
        return {"window": window, "reads_per_s": round(B / med), "call_ms": [round(s * 1e3, 2) for s in secs],
                "kept_fraction": round(kept / float(B * len(batches)), 4), "windows": tot[0], "iterations": tot[1],
                "iterations_per_window": round(tot[1] / max(tot[0], 1), 2), "candidate_units": tot[2],
                "records": tot[3]}

    def reads_of(n):
        blob = batches[0][0]
        return [blob[i * L:(i + 1) * L].decode() for i in range(n)]

    def loop_device(g, n):
        """the loop the per-read API allows: one round trip per call"""
        seqs, kept = reads_of(n), 0
        t = time.perf_counter()
        for s in seqs:
            if not g.median_at_least(s, a.cutoff):
                g.consume(s)
                kept += 1
        return {"reads": n, "reads_per_s": round(n / (time.perf_counter() - t)), "kept_fraction": round(kept / n, 4)}

    def loop_oracle(ref, n):
        seqs, kept = reads_of(n), 0
        t = time.perf_counter()
        for s in seqs:
            if ref.median(s)[0] < a.cutoff:
                ref.consume(s)
                kept += 1
        return {"reads": n, "reads_per_s": round(n / (time.perf_counter() - t)), "kept_fraction": round(kept / n, 4)}

    windows = [int(w) for w in a.window.split(",")]
    nb = min(a.baseline_reads, B)
    out = {"workload": "Countgraph k=%d %dx%.0e, genomic stream, genome %.0e, %d bp reads, C=%d, %d reads per call"
                       % (a.k, a.tables, a.x, G, L, a.cutoff, B)}

    warm = new_graph()                      # first-use costs (workspaces, code objects) stay out of the timings
    run_call(warm, 0)
    del warm
    ref = O.Table(O.BYTE, a.k, primes)
    for name, coverage in (("early", 0.0), ("mid", a.mid_coverage), ("saturated", a.coverage)):
        res = {"coverage_before": coverage, "device": []}
        for w in windows:
            g = new_graph()                 # every window size starts from the same table
            saturate(g, coverage)
            if w == windows[0]:
                tables = [bytes(t) for t in g.get_raw_tables()]
            res["device"].append(run_call(g, w))
            del g
        g = new_graph()
        saturate(g, coverage)
        res["loop_device"] = loop_device(g, nb)
        del g
        for i, t in enumerate(tables):
            ref.set_table_bytes(i, t)
        res["loop_oracle"] = loop_oracle(ref, nb)
        out[name] = res
    print(json.dumps(out))


def main():
    a = parse_args()
    if a.worker:
        worker(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
