"""bench.py end to end on a small workload: the plain run's result line, the
--dump-outputs arrays against the oracle, their run-to-run identity, and what
--full adds.  One bench.py process per case (the benchmark is the subject)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS, L, K, NT, X = 3000, 150, 21, 4, 1e5
WORKLOAD = ["--reads", str(READS), "-x", str(X), "--batch-kmers", "100000"]   # several device passes


def _bench(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + argv,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def oracle_table():
    import khmer_amd
    from khmer_amd import synth
    from oracle import oracle as O
    seqs, offs = synth.batch(0, READS, L)
    t = O.Table(O.BYTE, K, khmer_amd.get_n_primes_near_x(NT, X))
    t.set_use_bigcount(True)
    t.consume_batch(seqs, [int(v) for v in offs])
    return t


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_and_dump(tmp_path, oracle_table):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", d1] + WORKLOAD)
    assert (line["steps"], line["warmup"], line["full"]) == (3, 1, False)
    assert line["unit"] == "k-mers/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    kmers = READS * (L - K + 1)
    assert line["value"] == pytest.approx(kmers / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # a plain run leaves out what --full adds; the roofline comes from the timed steps' own events
    assert line["cpu_baseline"] is None and line["check"] is None and line["ms_per_step_unprofiled"] is None
    launches = line["roofline"]["launches"]
    assert launches > 0 and launches % 3 == 0   # the timed steps, not the warmup
    out = _load(d1)
    assert sorted(out) == ["n_occupied", "n_unique_kmers"] + ["table%d" % i for i in range(NT)]
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    for i in range(NT):
        assert out["table%d" % i].dtype == np.float32
        ref = np.frombuffer(oracle_table.table_bytes(i), np.uint8)
        assert np.array_equal(out["table%d" % i], ref.astype(np.float32)), "table %d" % i
    assert out["n_unique_kmers"].dtype == np.float64
    assert out["n_unique_kmers"].tolist() == [oracle_table.n_unique_kmers()]
    assert out["n_occupied"].tolist() == [oracle_table.n_occupied()]
    # the same arguments: the same inputs, the same outputs
    _bench(["--steps", "1", "--warmup", "0", "--dump-outputs", d2] + WORKLOAD)
    again = _load(d2)
    assert sorted(again) == sorted(out)
    for name in out:
        assert np.array_equal(out[name], again[name]), name


def test_full_run(oracle_table):
    line = _bench(["--full", "--steps", "2", "--warmup", "0", "--cpu-reads", "2000"] + WORKLOAD)
    assert line["full"] is True and line["steps"] == 2
    assert line["ms_per_step_unprofiled"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["check"]["n_unique_kmers"] == oracle_table.n_unique_kmers()
    assert line["check"]["n_occupied"] == oracle_table.n_occupied()
