"""Abundance trimming without a device: the restatements of the reference's
three loops (src/oxli/hashtable.cc:504-612) that the GPU tests compare
against, replayed over the oracle's counts on the reference's own known
answers; khmer_amd.trimming against a stub graph; filter-abund's options.

The restatements work on c[0..n-1], the counts of a raw read's k-mers
(get_kmer_counts).  Both k-mer iterators are done() after k-mer n-1 and report
start j / end k + j after k-mer j (include/oxli/kmer_hash.hh:364-377, 469-479).
"""
import struct

import pytest

from oracle import oracle as O

DNA = "AGCTTTTCATTCTGACTGCAACGGGCAATATGTCTCTGTGTGGATTAAAAAAAGAGTGTCTGATAGCAGC"   # tests/test_tabletype.py:339


def ref_trim(counts, k, cutoff, below=False):
    """trim_on_abundance (below: trim_below_abundance), hashtable.cc:504-563."""
    n = len(counts)
    if n <= 1:
        return 0
    bad = (lambda c: c > cutoff) if below else (lambda c: c < cutoff)
    if bad(counts[0]):
        return 0
    for j in range(1, n):
        if bad(counts[j]):
            return k + j - 1
    return n + k - 1


def ref_spectral(counts, k, max_count):
    """find_spectral_error_positions, hashtable.cc:565-612."""
    n = len(counts)
    t0 = next((j for j in range(n - 1) if counts[j] > max_count), None)
    if t0 is None:
        return []
    out = [t0 - 1] if t0 > 0 else []
    prev_bad = False
    for j in range(t0 + 1, n):
        bad = counts[j] <= max_count
        if bad and not prev_bad:
            out.append(k + j - 1)
        prev_bad = bad
    return out


def ref_min_req(n):
    """median_at_least's unsigned(0.5 + float(n) / 2), float32 (hashtable.cc:333-364)."""
    half = struct.unpack("<f", struct.pack("<f", struct.unpack("<f", struct.pack("<f", float(n)))[0] / 2.0))[0]
    return int(0.5 + half)


def ref_trim_gated(counts, k, cutoff, below, normalize_to):
    """khmer/trimming.py:44-48: a read failing median_at_least(normalize_to)
    is left alone (trim_at = its length); the gate comes before the n <= 1
    rule.  normalize_to None: no gate."""
    if normalize_to is not None:
        if sum(1 for c in counts if c >= normalize_to) < ref_min_req(len(counts)):
            return len(counts) + k - 1
    return ref_trim(counts, k, cutoff, below)


def oracle_counts(o, seq):
    return [o.get(h) for h in o.kmer_hashes(seq)]


def _table(k, hash=O.TWOBIT, kind=O.BYTE):
    return O.Table(kind, k, O.get_n_primes_near_x(2, 1e6), hash=hash)


@pytest.mark.parametrize("hash", [O.TWOBIT, O.MURMUR])
def test_restatement_trim_tabletype(hash):
    """tests/test_tabletype.py:314-336."""
    x = "ATGGCAGTAGCAGTGAGC"
    o = _table(6, hash)
    o.consume(x[:10])
    assert ref_trim(oracle_counts(o, x), 6, 1) == 10
    o = _table(6, hash)
    o.consume(O.reverse_complement(x)[:10])
    assert ref_trim(oracle_counts(o, x), 6, 0, below=True) == 13 == len(x) - 6 + 1


@pytest.mark.parametrize("hash", [O.TWOBIT, O.MURMUR])
@pytest.mark.parametrize("parts,want", [([DNA[:30]], [30]), ([DNA[1:]], [0]), ([DNA[:10], DNA[11:]], [10])])
def test_restatement_spectral_tabletype(hash, parts, want):
    """tests/test_tabletype.py:342-375."""
    o = _table(8, hash)
    for p in parts:
        o.consume(p)
    assert ref_spectral(oracle_counts(o, DNA), 8, 0) == want


def test_restatement_trim_countgraph():
    """tests/test_countgraph.py:788-808 (test_trim_full, test_trim_short)."""
    o = _table(6)
    o.consume(DNA)
    o.consume(DNA)
    assert ref_trim(oracle_counts(o, DNA), 6, 2) == 70 == len(DNA)
    o = _table(6)
    o.consume(DNA)
    o.consume(DNA[:50])
    assert ref_trim(oracle_counts(o, DNA), 6, 2) == 50


@pytest.mark.parametrize("parts,m,want", [
    ([DNA, DNA[:30]], 1, [30]),
    ([DNA, DNA], 2, []),
    ([DNA, DNA[1:]], 1, [0]),
    ([DNA], 2, []),
    ([DNA, DNA[:10], DNA[11:]], 1, [10]),
    ([DNA, DNA[8:]], 1, [7]),
])
def test_restatement_spectral_countgraph(parts, m, want):
    """tests/test_countgraph.py:811-877."""
    o = _table(8)
    for p in parts:
        o.consume(p)
    assert ref_spectral(oracle_counts(o, DNA), 8, m) == want


def test_restatement_edges():
    assert ref_trim([5], 4, 1) == 0                       # a read of exactly k bases
    assert ref_trim([], 4, 1) == 0
    assert ref_trim([5, 5, 0], 4, 1) == 5
    assert ref_trim_gated([5], 4, 1, False, 6) == 4       # gate before the n <= 1 rule
    assert ref_trim_gated([5], 4, 1, False, 5) == 0
    assert ref_spectral([9], 4, 1) == []
    assert ref_spectral([0, 9], 4, 1) == []               # the last k-mer is never a candidate
    assert ref_spectral([0, 9, 0], 4, 1) == [0, 5]
    assert [ref_min_req(n) for n in (1, 2, 3, 4, 130, 255, 256)] == [1, 1, 2, 2, 65, 128, 128]


# ---- khmer_amd.trimming over a stub graph -------------------------------------

class _StubGraph(object):
    """trim_on_abundance_batch of a table in which a k-mer's count is 5 unless
    it contains 'T' (then 0); counts the batch calls."""

    def __init__(self, k):
        self.k, self.calls = k, 0

    def ksize(self):
        return self.k

    def _counts(self, s):
        return [0 if "T" in s[i:i + self.k] else 5 for i in range(len(s) - self.k + 1)]

    def trim_on_abundance_batch(self, sequences, abundance, below=False, normalize_to=None):
        self.calls += 1
        return [None if len(s) < self.k else ref_trim_gated(self._counts(s), self.k, abundance, below, normalize_to)
                for s in sequences]


def test_trim_record_contract():
    khmer = pytest.importorskip("khmer_amd")
    from khmer_amd.trimming import trim_record, trim_records
    g = _StubGraph(4)
    dropped = khmer.Read(name="d", sequence="ACTCCCCC")          # first failing k-mer 0
    whole = khmer.Read(name="w", sequence="ACGCCGCA")
    cut = khmer.Read(name="c", sequence="ACGCCGCATCC", quality="abcdefghijk")
    cut_fa = khmer.Read(name="f", sequence="ACGCCGnATCC")        # cleaned_seq decides, the raw sequence is cut
    assert trim_record(g, dropped, 2) == (None, True)
    rec, did = trim_record(g, whole, 2)
    assert rec is whole and did is False
    rec, did = trim_record(g, cut, 2)
    assert did is True and (rec.name, rec.sequence, rec.quality) == ("c", "ACGCCGCA", "abcdefgh")
    rec, did = trim_record(g, cut_fa, 2)
    assert did is True and rec.sequence == "ACGCCGnA" and not hasattr(rec, "quality")
    # the gate: 5 of cut's 8 k-mers have a count >= 5 (min_req 4), none >= 6
    rec, did = trim_record(g, cut, 2, variable_coverage=True, normalize_to=5)
    assert did is True and rec.sequence == "ACGCCGCA"
    rec, did = trim_record(g, cut, 2, variable_coverage=True, normalize_to=6)
    assert rec is cut and did is False
    # normalize_to is ignored without variable_coverage
    assert trim_record(g, cut, 2, normalize_to=6)[1] is True
    g.calls = 0
    res = trim_records(g, [dropped, whole, cut, cut_fa], 2)
    assert g.calls == 1
    assert [r is not None and r.sequence for r, _ in res] == [False, "ACGCCGCA", "ACGCCGCA", "ACGCCGnA"]
    assert [d for _, d in res] == [True, False, True, True]
    assert res[1][0] is whole
    assert trim_records(g, [], 2) == []
    with pytest.raises(ValueError):
        trim_record(g, khmer.Read(name="s", sequence="ACG"), 2)


# ---- filter-abund.py's options ------------------------------------------------

def test_filter_abund_parser(capsys):
    pytest.importorskip("khmer_amd")
    from khmer_amd.scripts import filter_abund_parser
    args = filter_abund_parser().parse_args(["-q", "graph", "a.fa", "b.fa"])
    assert (args.cutoff, args.normalize_to, args.variable_coverage) == (2, 20, False)
    assert args.input_graph == "graph" and args.input_filename == ["a.fa", "b.fa"]
    assert args.single_output_file is None and not args.gzip and not args.bzip and not args.force
    args = filter_abund_parser().parse_args(["-q", "-C", "255", "-V", "-Z", "25", "-o", "out", "--gzip", "-T", "4",
                                             "graph", "a.fa"])
    assert (args.cutoff, args.normalize_to, args.variable_coverage) == (255, 25, True)
    assert args.single_output_file == "out" and args.gzip and args.threads == 4
    with pytest.raises(SystemExit) as e:
        filter_abund_parser().parse_args(["-q", "-C", "300", "graph", "a.fa"])
    assert e.value.code == 1
    assert "khmer only supports 0 <= cutoff < 256" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        filter_abund_parser().parse_args(["-q", "--gzip", "--bzip", "graph", "a.fa"])
