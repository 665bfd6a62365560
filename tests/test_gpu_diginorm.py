"""kh_normalize_by_median / Hashtable.normalize_by_median_batch against the
sequential loop of scripts/normalize-by-median.py:155-179 run on the oracle:
for each unit in order, median_at_least on every read against the table as it
stands (Table.kmer_hashes + get), consume() of a kept unit's reads.  Keep
flags, table bytes, n_unique_kmers, n_occupied and bigcounts must be equal,
whatever the schedule (window size, iteration cap)."""
import ctypes

import pytest

from oracle import oracle as O
from tests.conftest import data

khmer = pytest.importorskip("khmer_amd")
from khmer_amd._lib import lib, check  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 7
KINDS = {"byte": (O.BYTE, "Countgraph", "Counttable"), "nibble": (O.NIBBLE, "SmallCountgraph", "SmallCounttable"),
         "bit": (O.BIT, "Nodegraph", "Nodetable")}

# genome, reads, L, k, C, table sizes, storage, paired, units the oracle keeps
ROWS = [
    (2000, 600, 60, 17, 5, (4999, 5003), "byte", False, 317),
    (2000, 600, 60, 17, 1, (4999, 5003), "byte", False, 95),
    (2000, 600, 60, 17, 5, (499, 503), "byte", False, 79),      # heavy collisions
    (2000, 600, 60, 17, 5, (4999, 5003), "byte", True, 183),    # pairs (2i, 2i+1)
    (300, 1500, 40, 15, 3, (997, 1009), "nibble", False, 147),
    (100, 2500, 40, 15, 255, (997, 1009), "byte", False, 1144),  # reaches saturation
    (100, 400, 40, 15, 15, (997, 1009), "nibble", False, 99),
    (100, 200, 40, 15, 1, (997, 1009), "bit", False, 25),
]
SCHEDULES = [(w, m) for w in (0, 1, 7, 64) for m in (0, 1, 2)]


def at_least(tab, seq, cutoff):
    """Hashtable::median_at_least (src/oxli/hashtable.cc:333-364) on the oracle."""
    hashes = tab.kmer_hashes(seq)
    n = len(hashes)
    min_req = int(0.5 + float(n) / 2)
    return sum(1 for h in hashes if tab.get(h) >= cutoff) >= min_req


def sequential(tab, seqs, pairs, cutoff):
    """The reference's loop over units; returns one keep flag per read (None
    for a read shorter than k, which is left out of its unit)."""
    keep = [None] * len(seqs)
    r = 0
    while r < len(seqs):
        members = [r, r + 1] if pairs and pairs[r] else [r]
        unit = [q for q in members if len(seqs[q]) >= tab.k]
        kept = not all(at_least(tab, seqs[q], cutoff) for q in unit)
        for q in unit:
            keep[q] = kept
            if kept:
                tab.consume(seqs[q])
        r += len(members)
    return keep


def make_tables(storage, k, sizes, murmur=False, bigcount=False):
    kind, graph_cls, table_cls = KINDS[storage]
    ref = O.Table(kind, k, list(sizes), hash=O.MURMUR if murmur else O.TWOBIT)
    g = getattr(khmer, table_cls if murmur else graph_cls)(k, 0, 0, primes=list(sizes))
    if bigcount:
        ref.set_use_bigcount(True)
        g.set_use_bigcount(True)
    return ref, g


def bigcounts(g):
    n = ctypes.c_uint64()
    check(lib.kh_graph_get_bigcounts(g._g, None, None, 0, ctypes.byref(n)))
    keys = (ctypes.c_uint64 * max(n.value, 1))()
    vals = (ctypes.c_uint16 * max(n.value, 1))()
    check(lib.kh_graph_get_bigcounts(g._g, keys, vals, n.value, ctypes.byref(n)))
    return dict(zip(keys[:n.value], vals[:n.value]))


def assert_same_state(g, ref):
    tables = g.get_raw_tables()
    for i in range(len(ref.sizes)):
        assert bytes(tables[i]) == ref.table_bytes(i), "table %d differs from the oracle" % i
    assert g.n_unique_kmers() == ref.n_unique_kmers()
    assert g.n_occupied() == ref.n_occupied()
    assert bigcounts(g) == ref.bigcounts()


_expected = {}


def expected(row):
    """The oracle's answer for a row, computed once: reads, pair flags, keep
    flags and the final oracle table (left unchanged afterwards)."""
    if row not in _expected:
        genome, nreads, L, k, C, sizes, storage, paired, _ = row
        seqs = [O.synth_read(SEED, r, L, genome) for r in range(nreads)]
        pairs = [r % 2 == 0 for r in range(nreads)] if paired else None
        ref = O.Table(KINDS[storage][0], k, list(sizes))
        keep = sequential(ref, seqs, pairs, C)
        _expected[row] = (seqs, pairs, keep, ref)
    return _expected[row]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "g%d-n%d-C%d-%s-%d%s" % (r[0], r[1], r[4], r[6], r[5][0],
                                                                           "-pairs" if r[7] else ""))
def test_oracle_outcome_is_mixed(row):
    """The sequential loop keeps exactly the number of units the cases were chosen for."""
    seqs, pairs, keep, _ = expected(row)
    units = keep[::2] if row[7] else keep
    assert sum(units) == row[8] and 0 < row[8] < len(units)
    if pairs:
        assert keep[::2] == keep[1::2]


@pytest.mark.parametrize("window,max_iters", SCHEDULES)
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "g%d-n%d-C%d-%s-%d%s" % (r[0], r[1], r[4], r[6], r[5][0],
                                                                           "-pairs" if r[7] else ""))
def test_rows_every_schedule(row, window, max_iters):
    genome, nreads, L, k, C, sizes, storage, paired, _ = row
    seqs, pairs, keep, ref = expected(row)
    _, g = make_tables(storage, k, sizes)
    stats = {}
    got = g.normalize_by_median_batch(seqs, C, pairs=pairs, window=window, max_iters=max_iters, stats=stats)
    assert got == keep
    assert_same_state(g, ref)
    if row is ROWS[0] and (window, max_iters) == (0, 0):
        assert stats["iterations"] > stats["windows"], stats     # the iteration really ran
    if max_iters == 1:
        assert stats["windows"] > 1, stats                       # the partial commit really ran


def test_partial_commit_with_one_iteration():
    """max_iters = 1 in one default window: the stable prefix is committed and
    the next window starts behind it."""
    row = ROWS[0]
    seqs, pairs, keep, ref = expected(row)
    _, g = make_tables(row[6], row[3], row[5])
    stats = {}
    assert g.normalize_by_median_batch(seqs, row[4], max_iters=1, stats=stats) == keep
    assert stats["windows"] > 1 and stats["iterations"] == stats["windows"], stats
    assert_same_state(g, ref)


def test_murmur_counttable():
    genome, nreads, L, k, C, sizes = 2000, 600, 60, 17, 5, (4999, 5003)
    seqs = [O.synth_read(SEED, r, L, genome) for r in range(nreads)]
    ref, g = make_tables("byte", k, sizes, murmur=True)
    keep = sequential(ref, seqs, None, C)
    assert 0 < sum(keep) < nreads
    assert g.normalize_by_median_batch(seqs, C) == keep
    assert_same_state(g, ref)


def test_two_consecutive_calls():
    """The second call starts from the table the first one left."""
    row = ROWS[0]
    seqs, _, keep, ref = expected(row)
    _, g = make_tables(row[6], row[3], row[5])
    half = 250
    got = g.normalize_by_median_batch(seqs[:half], row[4])
    got += g.normalize_by_median_batch(seqs[half:], row[4], window=33)
    assert got == keep
    assert 0 < sum(keep[half:]) < len(keep) - half
    assert_same_state(g, ref)


@pytest.mark.parametrize("window", [0, 5])
def test_bigcount_cutoff_above_255(window):
    """Byte storage with bigcount on and C = 300: only the bigcount map can
    hold such counts, the call decides unit by unit and stays exact."""
    genome, nreads, L, k, C, sizes = 60, 1200, 40, 15, 300, (997, 1009)
    seqs = [O.synth_read(SEED, r, L, genome) for r in range(nreads)]
    ref, g = make_tables("byte", k, sizes, bigcount=True)
    keep = sequential(ref, seqs, None, C)
    assert 0 < sum(keep) < nreads, sum(keep)
    assert ref.bigcounts()
    assert g.normalize_by_median_batch(seqs, C, window=window) == keep
    assert_same_state(g, ref)


def test_bigcount_cutoff_within_the_table():
    """bigcount on and C = 255: the table bytes decide, bigcounts stay exact."""
    row = ROWS[5]
    genome, nreads, L, k, C, sizes = row[:6]
    seqs = expected(row)[0]
    ref, g = make_tables("byte", k, sizes, bigcount=True)
    keep = sequential(ref, seqs, None, C)
    assert g.normalize_by_median_batch(seqs, C) == keep
    assert_same_state(g, ref)


@pytest.mark.parametrize("storage,cutoff", [("nibble", 16), ("bit", 2), ("byte", 256)])
def test_cutoff_above_the_storage_maximum_keeps_everything(storage, cutoff):
    genome, nreads, L, k, sizes = 100, 400, 40, 15, (997, 1009)
    seqs = [O.synth_read(SEED, r, L, genome) for r in range(nreads)]
    ref, g = make_tables(storage, k, sizes)
    keep = sequential(ref, seqs, None, cutoff)
    assert all(keep)
    assert g.normalize_by_median_batch(seqs, cutoff) == keep
    assert_same_state(g, ref)


def test_variable_length_batch_with_short_reads():
    """Real reads of many lengths in pairs, one of exactly k bases, one
    shorter than k: the short read gets status 1, is not consumed, and its
    mate is decided alone."""
    k, C, sizes = 20, 2, (1499, 1511)
    seqs = []
    for _, s, _ in O.read_fastx(data("25k.fq.gz")):
        seqs.append(s.upper().replace("N", "A"))
        if len(seqs) == 300:
            break
    seqs[10] = seqs[10][:k]            # exactly k bases: one k-mer
    seqs[21] = seqs[21][:k - 1]        # shorter than k, the mate of read 20
    seqs[40] = seqs[40][:5]            # short first read of a pair
    assert len(set(len(s) for s in seqs)) > 3
    pairs = [r % 2 == 0 for r in range(len(seqs))]
    ref, g = make_tables("byte", k, sizes)
    keep = sequential(ref, seqs, pairs, C)
    assert keep[21] is None and keep[40] is None and keep[20] is not None and keep[41] is not None
    assert 0 < sum(1 for v in keep if v) < len(seqs) - 2
    with pytest.raises(ValueError):
        g.normalize_by_median_batch(seqs, C, pairs=pairs)
    assert g.n_occupied() == 0           # nothing was consumed before the error
    for window in (0, 3):
        g2 = make_tables("byte", k, sizes)[1]
        assert g2.normalize_by_median_batch(seqs, C, pairs=pairs, window=window, allow_short=True) == keep
        assert_same_state(g2, ref)


def test_c_abi_status_and_errors():
    k = 15
    g = khmer.Countgraph(k, 0, 0, primes=[997, 1009])
    seqs = [O.synth_read(SEED, r, 40, 100) for r in range(4)] + [b"ACGT"]
    blob = b"".join(seqs)
    offs = [0]
    for s in seqs:
        offs.append(offs[-1] + len(s))
    n = len(seqs)
    keep, status = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)()
    stats = (ctypes.c_uint64 * 4)()
    offsets = (ctypes.c_uint64 * (n + 1))(*offs)
    check(lib.kh_normalize_by_median(g._g, blob, offsets, n, None, 1, 0, 0, keep, status, stats))
    assert list(status) == [0, 0, 0, 0, 1] and keep[0] == 1 and keep[4] == 0
    assert stats[0] >= 1 and stats[2] >= 1 and stats[3] >= 2 * (40 - k + 1)
    # the last read cannot be paired with a following one
    pw = (ctypes.c_uint8 * n)(0, 0, 0, 0, 1)
    assert lib.kh_normalize_by_median(g._g, blob, offsets, n, pw, 1, 0, 0, keep, status, None) == 1
    # nothing to do
    check(lib.kh_normalize_by_median(g._g, blob, offsets, 0, None, 1, 0, 0, keep, status, stats))
    assert list(stats) == [0, 0, 0, 0]
    assert g.normalize_by_median_batch([], 1) == []
