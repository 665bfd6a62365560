"""Host-side pieces of normalize-by-median: broken_paired_reader and
check_is_pair (khmer/utils.py:48-118, khmer/_oxli/parsing.pyx:436-488 of the
reference, over the cases of its tests/test_cython_parsing.py:141-330), the
script's argument parser, and the
replay of keep flags into the -R report lines.  Nothing here creates a device
table."""
import pytest

pytest.importorskip("khmer_amd")
from khmer_amd import Read  # noqa: E402
from khmer_amd import scripts as S  # noqa: E402
from khmer_amd import khmer_args as KA  # noqa: E402
from khmer_amd.utils import UnpairedReadsError, broken_paired_reader, check_is_pair  # noqa: E402


def gather(records, **kw):
    x, n = [], 0
    for n, is_pair, read1, read2 in broken_paired_reader(iter(records), **kw):
        assert is_pair == (read2 is not None)
        x.append((read1.name, read2.name if read2 is not None else None))
    return x, n


READS = [Read(name="seq1/1", sequence="A" * 5),
         Read(name="seq1/2", sequence="A" * 4),
         Read(name="seq2/1", sequence="A" * 5),
         Read(name="seq3/1", sequence="A" * 3),
         Read(name="seq3/2", sequence="A" * 5)]


def test_reader_default_and_min_length_that_drops_nothing():
    want = [("seq1/1", "seq1/2"), ("seq2/1", None), ("seq3/1", "seq3/2")]
    assert gather(READS) == (want, 3)
    assert gather(READS, min_length=1) == (want, 3)
    assert gather(READS, min_length=3) == (want, 3)


def test_reader_min_length_breaks_a_pair():
    """A pair with a short read is not yielded as a pair; its second read goes
    on alone when it is long enough (khmer/utils.py:84-106)."""
    x, n = gather(READS, min_length=4)
    assert x == [("seq1/1", "seq1/2"), ("seq2/1", None), ("seq3/2", None)]
    assert n == 3
    # the short read second: the first is dropped with it, the second is too short to go on
    reads = READS[:3] + [Read(name="seq3/1", sequence="A" * 5), Read(name="seq3/2", sequence="A" * 3)]
    assert gather(reads, min_length=4)[0] == [("seq1/1", "seq1/2"), ("seq2/1", None)]


def test_reader_force_single():
    x, n = gather(READS, force_single=True)
    assert x == [(r.name, None) for r in READS] and n == 4
    x, n = gather(READS, min_length=5, force_single=True)
    assert x == [("seq1/1", None), ("seq2/1", None), ("seq3/2", None)] and n == 2


def test_reader_force_single_and_require_paired_conflict():
    with pytest.raises(ValueError, match="cannot both be set"):
        list(broken_paired_reader(iter(READS), force_single=True, require_paired=True))


def test_reader_require_paired_errors():
    with pytest.raises(UnpairedReadsError, match="Unpaired reads when require_paired is set!") as e:
        list(broken_paired_reader(iter(READS), require_paired=True))
    assert e.value.read1.name == "seq2/1" and e.value.read2.name == "seq3/1"
    assert isinstance(e.value, ValueError)
    # an orphan at the end
    with pytest.raises(UnpairedReadsError) as e:
        list(broken_paired_reader(iter(READS[:3]), require_paired=True))
    assert e.value.read1.name == "seq2/1" and e.value.read2 is None
    got = list(broken_paired_reader(iter(READS[:2]), require_paired=True))
    assert [(n, p, a.name, b.name) for n, p, a, b in got] == [(0, True, "seq1/1", "seq1/2")]


@pytest.mark.parametrize("second_pair", [
    (3, 5),     # first read short
    (5, 3),     # second read short
    (3, 3),     # both short
])
def test_reader_require_paired_drops_short_pairs_silently(second_pair):
    reads = [Read(name="seq1/1", sequence="A" * 5), Read(name="seq1/2", sequence="A" * 4),
             Read(name="seq3/1", sequence="A" * second_pair[0]), Read(name="seq3/2", sequence="A" * second_pair[1])]
    got = list(broken_paired_reader(iter(reads), min_length=4, require_paired=True))
    assert [(n, a.name, b.name) for n, _, a, b in got] == [(0, "seq1/1", "seq1/2")]
    # the short pair first, the good pair second
    got = list(broken_paired_reader(iter(reads[2:] + reads[:2]), min_length=4, require_paired=True))
    assert [(n, a.name, b.name) for n, _, a, b in got] == [(0, "seq1/1", "seq1/2")]


def test_reader_counts_records_yielded():
    reads = [Read(name="a/1", sequence="ACGT"), Read(name="a/2", sequence="ACGT"),
             Read(name="b", sequence="ACGT"), Read(name="c/1", sequence="ACGT"), Read(name="c/2", sequence="ACGT")]
    got = [(n, p) for n, p, _, _ in broken_paired_reader(iter(reads))]
    assert got == [(0, True), (2, False), (3, True)]
    assert list(broken_paired_reader(iter([]))) == []


@pytest.mark.parametrize("name1,name2,want", [
    ("seq/1", "seq/2", True),
    ("seq/2", "seq/1", False),
    ("seq/1", "seq2/2", False),
    ("seq", "seq2", False),
    ("/1", "/2", False),                                   # no stem before the suffix
    ("seq 1::", "seq 2::", True),                          # Casava 1.8
    ("@HWI:1:2 1:N:0:ATCACG", "@HWI:1:2 2:N:0:ATCACG", True),
    ("seq 1::", "seq2 2::", False),
    ("seq 2::", "seq 1::", False),
    ("seq\t1:N", "seq\t2:N", True),
    ("SRR001 name/1", "SRR001 name/2", True),              # fastq-dump
    ("SRR001 name/1", "SRR002 name/2", False),
    ("SRR001 name/1", "SRR001 other/2", False),
    ("seq/1 extra", "seq/2 extra", True),
])
def test_check_is_pair_names(name1, name2, want):
    assert check_is_pair(Read(name=name1, sequence="AAA"), Read(name=name2, sequence="AAA")) is want
    assert check_is_pair(Read(name=name1, sequence="AAA", quality="###"),
                         Read(name=name2, sequence="AAA", quality="###")) is want


def test_check_is_pair_mixed_formats():
    with pytest.raises(ValueError, match="both records must be same type"):
        check_is_pair(Read(name="seq/1", sequence="AAA", quality="###"), Read(name="seq/2", sequence="AAA"))


def nbm_args(argv):
    return S.normalize_by_median_args(argv)


def test_parser_defaults():
    a = nbm_args(["-q", "reads.fa"])
    assert (a.cutoff, a.paired, a.force_single, a.unpaired_reads, a.savegraph, a.loadgraph) == \
        (20, False, False, None, None, None)
    assert (a.report, a.report_frequency, a.force, a.single_output_file) == (None, 100000, False, None)
    assert (a.ksize, a.n_tables, a.max_tablesize, a.small_count, a.gzip, a.bzip) == (32, 4, 1e6, False, False, False)
    assert a.input_filenames == ["reads.fa"]


def test_parser_options():
    a = nbm_args(["-q", "-C", "5", "-p", "-u", "orphans.fa", "-s", "out.ct", "-R", "rep.txt", "--report-frequency",
                  "100", "-f", "-o", "-", "-l", "in.ct", "-k", "17", "-N", "2", "-x", "1e5", "--gzip", "a.fa", "b.fa"])
    assert (a.cutoff, a.paired, a.unpaired_reads, a.savegraph, a.report, a.report_frequency) == \
        (5, True, "orphans.fa", "out.ct", "rep.txt", 100)
    assert (a.force, a.single_output_file, a.loadgraph, a.ksize, a.n_tables, a.max_tablesize, a.gzip) == \
        (True, "-", "in.ct", 17, 2, 1e5, True)
    assert a.input_filenames == ["a.fa", "b.fa"]
    assert nbm_args(["-q", "--savegraph", "x", "--loadgraph", "y", "--output", "z", "--cutoff", "3",
                     "--unpaired-reads", "u", "--paired", "a.fa"]).cutoff == 3


def test_parser_rejects_paired_with_force_single(capsys):
    KA.configure_logging(False)
    with pytest.raises(SystemExit) as e:
        nbm_args(["-q", "-C", "1", "-k", "17", "--force_single", "-p", "reads.fa"])
    assert e.value.code == 1
    assert "cannot both be set" in capsys.readouterr().err


def test_parser_rejects_cutoff_out_of_range(capsys):
    with pytest.raises(SystemExit) as e:
        nbm_args(["-q", "-C", "256", "reads.fa"])
    assert e.value.code == 1
    assert "ERROR: khmer only supports 0 <= cutoff < 256" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        nbm_args(["-q", "--gzip", "--bzip", "reads.fa"])


def test_progress_replays_keep_flags():
    """Units of 1, 2, 2, 1, 1, 2, 1 reads with flags K, K, -, -, K, K, -;
    report every 3 reads.  By hand: totals 1, 3, 5, 6, 7, 9, 10 and kept
    1, 3, 3, 3, 4, 6, 6; a report is due when the total reaches 3 (then the
    mark moves to 6), at 6 (-> 9) and at 9 (-> 12)."""
    p = S.DiginormProgress(3)
    sizes = [1, 2, 2, 1, 1, 2, 1]
    flags = [True, True, False, False, True, True, False]
    assert p.advance(sizes[:3], flags[:3]) == [(3, 3)]          # two batches give what one would
    assert p.advance(sizes[3:], flags[3:]) == [(6, 3), (9, 6)]
    assert (p.total, p.kept, p.last_report_at, p.next_report_at) == (10, 6, 9, 12)
    q = S.DiginormProgress(3)
    assert q.advance(sizes, flags) == [(3, 3), (6, 3), (9, 6)]
    # a pair that jumps over the mark reports once, at its own total
    r = S.DiginormProgress(3)
    assert r.advance([2, 2, 2], [True, False, True]) == [(4, 2), (6, 4)]
    assert S.DiginormProgress(100).advance([1] * 5, [True] * 5) == []


def test_report_line_format():
    """The reference's '{total},{kept},{f_kept:.4}' (its tests pin these strings)."""
    assert S.report_line(1001, 1) == "1001,1,0.000999"
    assert S.report_line(2002, 1) == "2002,1,0.0004995"
    assert S.report_line(100, 1) == "100,1,0.01"
    assert S.report_line(200, 1) == "200,1,0.005"
    assert S.report_line(2, 2) == "2,2,1.0"
