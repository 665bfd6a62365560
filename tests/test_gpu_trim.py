"""Abundance trimming on the device against the oracle (GPU):
trim_on_abundance, trim_below_abundance, find_spectral_error_positions
(src/oxli/hashtable.cc:504-612), the median_at_least gate of
khmer/trimming.py:38-67, and the fused one-wave-per-read kernel over
device-resident reads (kh_trim_fixed_device).

The expected values come from the oracle's k-mer counts and the restatements
of the reference's loops in tests/test_trim_cpu.py (checked there against the
reference's known answers); the same known answers are replayed here through
the khmer_amd classes.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import data
from tests.test_trim_cpu import DNA, oracle_counts, ref_min_req, ref_spectral, ref_trim, ref_trim_gated

pytestmark = pytest.mark.gpu

khmer = pytest.importorskip("khmer_amd")

SEED = 0x6b686d6572
ALL_CLASSES = ["Countgraph", "SmallCountgraph", "Nodegraph", "Counttable"]
COUNTING_CLASSES = ["Countgraph", "SmallCountgraph", "Counttable"]


def _any(cls, k):
    return getattr(khmer, cls)(k, 1e6, 4)


# ---- 1. the reference's known answers through the classes ---------------------

@pytest.mark.parametrize("cls", ALL_CLASSES)
def test_trim_kats_tabletype(cls):
    """tests/test_tabletype.py:314-375."""
    x = "ATGGCAGTAGCAGTGAGC"
    hi = _any(cls, 6)
    hi.consume(x[:10])
    assert hi.trim_on_abundance(x, 1) == (x[:10], 10)
    hi = _any(cls, 6)
    hi.consume(khmer.reverse_complement(x)[:10])
    assert hi.trim_below_abundance(x, 0) == (x[:13], 13)
    for parts, want in (([DNA[:30]], [30]), ([DNA[1:]], [0]), ([DNA[:10], DNA[11:]], [10])):
        kh = _any(cls, 8)
        for p in parts:
            kh.consume(p)
        assert kh.find_spectral_error_positions(DNA, 0) == want


def test_trim_kats_countgraph():
    """tests/test_countgraph.py:788-877."""
    hi = khmer.Countgraph(6, 1e6, 2)
    hi.consume(DNA)
    hi.consume(DNA)
    assert hi.trim_on_abundance(DNA, 2) == (DNA, 70)
    hi = khmer.Countgraph(6, 1e6, 2)
    hi.consume(DNA)
    hi.consume(DNA[:50])
    seq, pos = hi.trim_on_abundance(DNA, 2)
    assert (seq, pos) == (DNA[:50], 50)
    assert hi.get(seq[-6:]) == 2 and hi.get(DNA[:51][-6:]) == 1
    for parts, m, want in (([DNA, DNA[:30]], 1, [30]), ([DNA, DNA], 2, []), ([DNA, DNA[1:]], 1, [0]),
                           ([DNA], 2, []), ([DNA, DNA[:10], DNA[11:]], 1, [10]), ([DNA, DNA[8:]], 1, [7])):
        hi = khmer.Countgraph(8, 1e6, 2)
        for p in parts:
            hi.consume(p)
        assert hi.find_spectral_error_positions(DNA, m) == want, (parts, m)


def _valid_reads_table(cls):
    x = _any(cls, 8)
    for read in khmer.ReadParser(data("valid-read-testing.fq")):
        x.consume(read.cleaned_seq)
    return x


@pytest.mark.parametrize("cls", ALL_CLASSES)
def test_trim_kats_lowercase(cls):
    """tests/test_sequence_validation.py:127-144: lowercase is not cleaned."""
    x = _valid_reads_table(cls)
    s = "caggcgcccaccaccgtgccctccaacctgatggt"
    assert x.trim_on_abundance(s, 1)[1] == 0
    assert x.trim_below_abundance(s, 0) == (s, 35)
    assert x.find_spectral_error_positions(s, 1) == []


@pytest.mark.parametrize("cls", COUNTING_CLASSES)
def test_trim_kats_n(cls):
    """tests/test_sequence_validation.py:147-163 (counting types)."""
    x = _valid_reads_table(cls)
    s = "ACTGGGCGTAGNCGGTGTCCTCATCGGCACCAGC"
    assert x.trim_on_abundance(s, 1) == (s[:11], 11)
    assert x.trim_below_abundance(s, 2)[1] == 34
    assert x.find_spectral_error_positions(s, 1) == [11]


def test_trim_short_and_single_kmer():
    hi = khmer.Countgraph(20, 1e6, 2)
    for fn in (hi.trim_on_abundance, hi.trim_below_abundance, hi.find_spectral_error_positions):
        with pytest.raises(ValueError):
            fn("ACGT", 1)
    read = "ACGTTGCAAGGCTTAACCGG"
    hi.consume(read)
    assert hi.get(read) == 1
    assert hi.trim_on_abundance(read, 1) == ("", 0)     # a single k-mer: 0 though it is abundant
    assert hi.trim_below_abundance(read, 5) == ("", 0)
    assert hi.find_spectral_error_positions(read, 0) == []
    assert hi.trim_on_abundance_batch(["ACGT", read, read + "A"], 1) == [None, 0, 20]
    assert hi.trim_on_abundance_batch(["ACGT", read], 1, normalize_to=1) == [None, 0]
    assert hi.trim_on_abundance_batch(["ACGT", read], 1, normalize_to=2) == [None, 20]   # gate before the rule
    assert hi.find_spectral_error_positions_batch(["ACGT", read], 0) == [None, []]
    assert hi.trim_on_abundance_batch([], 1) == [] and hi.find_spectral_error_positions_batch([], 1) == []


# ---- 2. host batches against the oracle ----------------------------------------

CUTOFFS = (0, 1, 2, 3, 5, 8, 20, 100, 255, 256, 1000, 65535)


@pytest.mark.parametrize("cls,k,x,n", [("Countgraph", 20, 1e3, 2), ("Countgraph", 12, 1e5, 4),
                                       ("SmallCountgraph", 15, 5e3, 3), ("Counttable", 17, 2e3, 2),
                                       ("Nodegraph", 20, 1e4, 2)])
def test_trim_batch_matches_oracle(cls, k, x, n):
    """The saturated small tables of test_median_at_least_matches_oracle
    (counts spread over 0..255 and bigcounts): every cutoff, both directions,
    without the gate and with it at two medians."""
    from tests.test_gpu_parity import KIND, HASH
    sizes = O.get_n_primes_near_x(n, x)
    g = getattr(khmer, cls)(k, 1, 1, primes=sizes)
    o = O.Table(KIND[cls], k, sizes, hash=HASH[cls])
    if cls == "Countgraph":
        g.set_use_bigcount(True)
        o.set_use_bigcount(True)
    for f in ("test-abund-read-2.fa", "random-20-a.fa"):
        g.consume_seqfile(data(f))
        o.consume_fastx(data(f))
    reads = [s for _, s, _ in O.read_fastx(data("test-abund-read-2.fa"))][:300]
    reads += [s for _, s, _ in O.read_fastx(data("random-20-a.fa"))]
    reads = [r for r in reads if len(r) >= k]
    reads += [reads[0][:k], reads[-1][:k + 1]]            # one and two k-mers
    counts = [oracle_counts(o, r) for r in reads]
    for cut in CUTOFFS:
        for below in (False, True):
            for z in (None, 2, 20):
                got = g.trim_on_abundance_batch(reads, cut, below=below, normalize_to=z)
                want = [ref_trim_gated(c, k, cut, below, z) for c in counts]
                assert got == want, (cut, below, z)
        assert g.find_spectral_error_positions_batch(reads, cut) == [ref_spectral(c, k, cut) for c in counts], cut
    # the single-read methods agree with the batch
    for r, c in list(zip(reads, counts))[:20]:
        for cut in (1, 2, 20):
            at = ref_trim(c, k, cut)
            assert g.trim_on_abundance(r, cut) == (r[:at], at)
            at = ref_trim(c, k, cut, below=True)
            assert g.trim_below_abundance(r, cut) == (r[:at], at)
            assert g.find_spectral_error_positions(r, cut) == ref_spectral(c, k, cut)


def test_spectral_capacity():
    """The CSR call reports the capacity it needs when `cap` is too small."""
    from khmer_amd._lib import lib
    g = khmer.Countgraph(8, 1e6, 2)
    g.consume(DNA)
    g.consume(DNA[:10])
    g.consume(DNA[11:])
    seqs = [DNA, "ACGT", DNA]
    blob = "".join(seqs).encode()
    offs = (ctypes.c_uint64 * 4)(0, 70, 74, 144)
    poff = (ctypes.c_uint64 * 4)()
    pos = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    st = (ctypes.c_uint8 * 3)()
    assert lib.kh_find_spectral_error_positions(g._g, blob, offs, 3, 1, poff, pos, 1, st) == khmer._lib.KH_EVALUE
    assert list(poff) == [0, 1, 1, 2] and list(pos) == [9, 9, 9, 9] and list(st) == [0, 1, 0]
    assert lib.kh_find_spectral_error_positions(g._g, blob, offs, 3, 1, poff, pos, 2, st) == khmer._lib.KH_OK
    assert list(poff) == [0, 1, 1, 2] and list(pos[:2]) == [10, 10]


# ---- 3. the fused kernel over device reads -------------------------------------

# cls, k, x, genome, bigcount, A, Z, then what the oracle gives for these inputs:
# reads trimmed to (zero, inside, full) by trim_on_abundance(A), reads passing
# median_at_least(Z)
FIXED = [
    ("Countgraph", 21, 5e4, 3000, False, 3, 20, (461, 1476, 563), 2431),
    ("Countgraph", 21, 5e4, 1000, True, 300, 20, (1259, 1218, 23), 2432),
    ("SmallCountgraph", 31, 3e4, 4000, False, 5, 10, (640, 1301, 559), 2064),
    ("Nodegraph", 25, 5e4, 3000, False, 1, 1, (309, 1447, 744), 2492),
    ("SmallCounttable", 51, 4e4, 3000, False, 4, 10, (961, 980, 559), 1360),
]


def fixed_oracle(cls, k, sizes, genome, bigcount, n, L):
    """Oracle table built from stream reads 0..n-1 of the genomic stream, and
    the k-mer counts of reads n..2n-1."""
    from tests.test_gpu_parity import KIND, HASH
    from khmer_amd import synth
    o = O.Table(KIND[cls], k, sizes, hash=HASH[cls])
    o.set_use_bigcount(bigcount)
    o.consume_batch(synth.genomic_batch(0, n, L, genome)[0], [i * L for i in range(n + 1)])
    return [oracle_counts(o, O.synth_read(SEED, r, L, genome)) for r in range(n, 2 * n)]


def fixed_variants(counts, k, A, Z):
    """{(below, gate): expected trim_at per read}"""
    return {(below, gate): [ref_trim_gated(c, k, A, bool(below), Z if gate else None) for c in counts]
            for below in (0, 1) for gate in (0, 1)}


def check_fixed_conditions(counts, want, Z, L, classes, passes, gate_min=50):
    """An all-zero or all-L kernel cannot pass: the oracle's own answers hold
    at least 20 reads of every class, and the gate splits the reads, at least
    50 on either side.  The Nodegraph inputs cannot meet the second condition
    (counts are 0 or 1, so only the 8 reads that are mostly novel fail
    median_at_least(1)); every configuration is pinned to its exact figures
    instead, which for the other four imply both conditions."""
    plain = want[(0, 0)]
    zero = sum(1 for a in plain if a == 0)
    full = sum(1 for a in plain if a == L)
    got_classes = (zero, len(plain) - zero - full, full)
    got_passes = sum(1 for c in counts if sum(1 for v in c if v >= Z) >= ref_min_req(len(c)))
    assert (got_classes, got_passes) == (classes, passes)
    assert min(got_classes) >= 20
    assert min(got_passes, len(counts) - got_passes) >= gate_min


@pytest.mark.parametrize("cls,k,x,genome,bigcount,A,Z,classes,passes", FIXED)
def test_trim_fixed_device(cls, k, x, genome, bigcount, A, Z, classes, passes):
    from khmer_amd._lib import check
    from tests.test_gpu_device_paths import _Dev
    d = _Dev()
    try:
        n, L = 2500, 150
        murmur = cls == "SmallCounttable"
        g = getattr(khmer, cls)(k, x, 4)
        if bigcount:
            g.set_use_bigcount(True)

        def stream(r0):
            words = d.alloc((n * L // 32 + 2) * 8)
            koff = d.alloc((n + 1) * 8)
            # the packed stream itself does not depend on k (the generator takes k <= 32)
            check(d.lib.kh_synth_genomic_device(d.dev, SEED, genome, r0, n, L, min(k, 32), words, koff))
            if not murmur:
                return words
            asc = d.alloc(n * L + 64)
            check(d.lib.kh_unpack_ascii_device(d.dev, words, n * L, asc))
            return asc

        build, query = stream(0), stream(n)
        if murmur:
            check(d.lib.kh_consume_bytes_fixed_device(g._g, build, n, L))
        else:
            check(d.lib.kh_consume_packed_fixed_device(g._g, build, n, L))
        counts = fixed_oracle(cls, k, g.hashsizes(), genome, bigcount, n, L)
        if bigcount:
            assert max(max(c) for c in counts) > 255, "the case should reach bigcount values"
        want = fixed_variants(counts, k, A, Z)
        check_fixed_conditions(counts, want, Z, L, classes, passes, gate_min=8 if cls == "Nodegraph" else 50)
        out = d.alloc(n * 4 + 64)
        for (below, gate), exp in sorted(want.items()):
            check(d.lib.kh_trim_fixed_device(g._g, query, n, L, A, below, gate, Z, out))
            got = np.frombuffer(d.get(out, n * 4), dtype=np.uint32)
            bad = np.nonzero(got != np.array(exp, dtype=np.uint32))[0]
            assert not len(bad), (below, gate, int(bad[0]), int(got[bad[0]]), exp[bad[0]])
    finally:
        d.free()


# ---- 4. slot and lane boundaries ------------------------------------------------

BOUNDARY_T = (1, 63, 64, 65, 127, 128, 191, 192, 255)
K4 = 21


def boundary_case(kpr):
    """kpr + 1 random reads of kpr k-mers (stream reads kpr * 1000 ..): read r
    has its k-mer t = r left out of the table (read kpr: nothing left out).
    Returns (reads, pieces to consume)."""
    from khmer_amd import synth
    L = kpr + K4 - 1
    blob = synth.batch(kpr * 1000, kpr + 1, L)[0]
    reads = [blob[r * L:(r + 1) * L] for r in range(kpr + 1)]
    pieces = []
    for t, read in enumerate(reads):
        if t == kpr:
            pieces.append(read)
            continue
        if t >= 1:
            pieces.append(read[:K4 + t - 1])
        if len(read) - (t + 1) >= K4:
            pieces.append(read[t + 1:])
    return reads, pieces


def boundary_oracle(kpr, sizes):
    reads, pieces = boundary_case(kpr)
    o = O.Table(O.BYTE, K4, sizes)
    offs = [0]
    for p in pieces:
        offs.append(offs[-1] + len(p))
    o.consume_batch(b"".join(pieces), offs)
    want = [ref_trim(oracle_counts(o, r), K4, 1) for r in reads]
    # the oracle's own answers hold every boundary position of this kpr;
    # with a single k-mer per read the reference returns 0 for every read
    L = kpr + K4 - 1
    need = {0} | ({L} if kpr >= 2 else set()) | {K4 + t - 1 for t in BOUNDARY_T if t < kpr}
    assert need <= set(want), sorted(need - set(want))
    return reads, pieces, offs, want


@pytest.mark.parametrize("kpr", [1, 2, 63, 64, 65, 128, 129, 255, 256])
def test_trim_fixed_boundaries(kpr):
    from khmer_amd._lib import check
    from tests.test_gpu_device_paths import _Dev
    d = _Dev()
    try:
        g = khmer.Countgraph(K4, 1e6, 4)
        reads, pieces, offs, want = boundary_oracle(kpr, g.hashsizes())
        consumed = ctypes.c_uint64()
        check(d.lib.kh_consume_seqs(g._g, b"".join(pieces), (ctypes.c_uint64 * len(offs))(*offs), len(pieces), 0,
                                    ctypes.byref(consumed)))
        n, L = kpr + 1, kpr + K4 - 1
        words = d.alloc((n * L // 32 + 2) * 8)
        koff = d.alloc((n + 1) * 8)
        check(d.lib.kh_synth_packed_device(d.dev, SEED, kpr * 1000, n, L, K4, words, koff))
        out = d.alloc(n * 4 + 64)
        check(d.lib.kh_trim_fixed_device(g._g, words, n, L, 1, 0, 0, 0, out))
        got = [int(v) for v in np.frombuffer(d.get(out, n * 4), dtype=np.uint32)]
        assert got == want
        # the host batch path agrees on the same reads
        assert g.trim_on_abundance_batch(reads, 1) == want
    finally:
        d.free()


# ---- 5. errors -------------------------------------------------------------------

def test_trim_fixed_device_errors():
    from khmer_amd._lib import check, lib
    from tests.test_gpu_device_paths import _Dev
    d = _Dev()
    try:
        g = khmer.Countgraph(21, 1e4, 2)
        buf = d.alloc(4096)
        with pytest.raises(ValueError):
            check(lib.kh_trim_fixed_device(g._g, buf, 1, 20, 1, 0, 0, 0, buf))    # read shorter than k
        with pytest.raises(ValueError):
            check(lib.kh_trim_fixed_device(g._g, buf, 1, 300, 1, 0, 0, 0, buf))   # > 256 k-mers per read
        with pytest.raises(ValueError):
            check(lib.kh_consume_bytes_fixed_device(g._g, buf, 1, 30))            # ASCII input, 2-bit graph
        check(lib.kh_trim_fixed_device(g._g, buf, 0, 30, 1, 0, 0, 0, buf))        # no reads: nothing to do
    finally:
        d.free()
