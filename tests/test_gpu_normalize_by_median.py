"""scripts/normalize-by-median.py on the device, in-process, pinned to the
reference's own script tests (reference tests/test_normalize_by_median.py):
outputs land in the working directory as basename(input) + '.keep'."""
import gzip
import os
import shutil
import subprocess
import sys

import pytest

from oracle import oracle as O
from tests.conftest import ROOT, data

khmer = pytest.importorskip("khmer_amd")
from khmer_amd import scripts as S  # noqa: E402
from khmer_amd import khmer_args as KA  # noqa: E402

pytestmark = pytest.mark.gpu

READ2 = data("test-abund-read-2.fa")
PAIRED = data("test-abund-read-paired.fa")


def run(argv, capsys):
    KA.configure_logging(False)
    try:
        status = S.normalize_by_median(argv)
    except SystemExit as e:
        status = e.code if isinstance(e.code, int) else 1
    out, err = capsys.readouterr()
    return status, out, err


def records(path):
    return list(O.read_fastx(path))


def seqs(path):
    return [s for _, s, _ in records(path)]


def names(path):
    return [n for n, _, _ in records(path)]


def test_normalize_by_median(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", READ2], capsys)
    assert st == 0, err
    assert "Total number of unique k-mers: 98" in err
    assert "DONE with " + READ2 + "; kept 1 of 1001 or 0.1%" in err
    assert "output in test-abund-read-2.fa.keep" in err
    assert "fp rate estimated to be 0.000" in err
    assert "I/O Errors" not in err
    got = seqs("test-abund-read-2.fa.keep")
    assert len(got) == 1 and got[0].startswith("GGTTGACGGGGCTCAGGGGG")


def test_normalize_by_median_quiet(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, out, err = run(["-C", "1", "-k", "17", "--quiet", "-M", "2e6", READ2], capsys)
    assert (st, out) == (0, "") and len(err) < 460
    got = seqs("test-abund-read-2.fa.keep")
    assert len(got) == 1 and got[0].startswith("GGTTGACGGGGCTCAGGGGG")


def test_normalize_by_median_2(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert run(["-C", "2", "-k", "17", READ2], capsys)[0] == 0
    got = seqs("test-abund-read-2.fa.keep")
    assert len(got) == 2 and got[0].startswith("GGTTGACGGGGCTCAGGGGG") and got[1] == "GGTTGACGGGGCTCAGGG"


def test_normalize_by_median_paired(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert run(["-C", "1", "-p", "-k", "17", PAIRED], capsys)[0] == 0
    got = seqs("test-abund-read-paired.fa.keep")
    assert len(got) == 2
    assert got[0].startswith("GGTTGACGGGGCTCAGGGGG") and got[1].startswith("GGTTGACGGGGCTCAGGG")


def test_normalize_by_median_unpaired_and_paired(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", "-u", data("random-20-a.fa"), "-p", PAIRED], capsys)
    assert st == 0, err
    assert "Total number of unique k-mers: 4061" in err
    assert os.path.exists("test-abund-read-paired.fa.keep") and os.path.exists("random-20-a.fa.keep")


def test_normalize_by_median_paired_fq(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert run(["-C", "20", "-p", "-k", "17", data("test-abund-read-paired.fq")], capsys)[0] == 0
    recs = records("test-abund-read-paired.fq.keep")
    assert len(recs) == 6
    assert recs[0][1].startswith("GGTTGACGGGGCTCAGGGGG") and recs[1][1].startswith("GGTTGACGGGGCTCAGGG")
    got = [n for n, _, _ in recs]
    assert "895:1:37:17593:9954 1::FOO" in got and "895:1:37:17593:9954 2::FOO" in got
    assert all(q and len(q) == len(s) for _, s, q in recs)
    assert open("test-abund-read-paired.fq.keep").read().startswith("@")


def test_normalize_by_median_count_kmers_PE(tmp_path, monkeypatch, capsys):
    """One pair of reads identical but for the last base: the second is
    dropped when single, kept with -p (one more unique k-mer)."""
    monkeypatch.chdir(tmp_path)
    infile = data("paired_one.base.dif.fa")
    st, _, err = run(["-C", "1", "-k", "17", "--force_single", infile], capsys)
    assert st == 0 and "Total number of unique k-mers: 98" in err and "kept 1 of 2 or 50.0%" in err
    st, _, err = run(["-C", "1", "-k", "17", "-p", infile], capsys)
    assert st == 0 and "Total number of unique k-mers: 99" in err and "kept 2 of 2 or 100.0%" in err


def test_normalize_by_median_impaired(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-p", "-k", "17", data("test-abund-read-impaired.fa")], capsys)
    assert st != 0
    assert "ERROR: Unpaired reads " in err and "** Exiting!" in err
    assert not os.path.exists("test-abund-read-impaired.fa.keep")     # removed on failure


def test_normalize_by_median_unpaired_final_read(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", "-p", data("single-read.fq")], capsys)
    assert st != 0 and "ERROR: Unpaired reads when require_paired" in err


def test_normalize_by_median_contradictory_args(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", "--force_single", "-p", "-R", "report.out", READ2], capsys)
    assert st != 0 and "cannot both be set" in err


@pytest.mark.parametrize("infile,pairing,want", [
    # every pair holds a multicopy and a random read: with -p all are kept
    ("dn-test-all-paired-all-keep.fa", ["-p"], {"a/1", "a/2", "b/1", "b/2", "c/1", "c/2", "d/1", "d/2"}),
    # single: the random reads and one copy of the multicopy one
    ("dn-test-all-paired-all-keep.fa", ["--force_single"], {"a/1", "a/2", "b/2", "c/1", "d/2"}),
    # all unpaired, one duplicate
    ("dn-test-none-paired.fa", [], {"a/1", "b/2", "d/1"}),
    # mixed paired / unpaired
    ("dn-test-some-paired-all-keep.fa", [], {"a/1", "a/2", "b/2", "c/1", "c/2", "d/2"}),
    # pairs recognised without -p
    ("dn-test-all-paired-all-keep.fa", [], {"a/1", "a/2", "b/1", "b/2", "c/1", "c/2", "d/1", "d/2"}),
])
def test_diginorm_basic_functionality(infile, pairing, want, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1"] + pairing + ["-k", "15", data(infile)], capsys)
    assert st == 0, err
    assert set(names(infile + ".keep")) == want


def test_normalize_by_median_report_fp(tmp_path, monkeypatch, capsys):
    """-R over two input files: one line at the end of each, aggregate counts."""
    monkeypatch.chdir(tmp_path)
    os.mkdir("copyDataTwo")
    copy = shutil.copy(READ2, os.path.join("copyDataTwo", "reads-two.fa"))
    assert run(["-C", "1", "-k", "17", "-R", "report.out", READ2, copy], capsys)[0] == 0
    assert open("report.out").read().splitlines() == ["total,kept,f_kept", "1001,1,0.000999", "2002,1,0.0004995"]


def test_normalize_by_median_report_fp_hifreq(tmp_path, monkeypatch, capsys):
    """--report-frequency 100: the sequential total,kept at every hundredth
    read, although the reads go to the device in one batch."""
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", "-R", "report.out", READ2, "--report-frequency", "100"], capsys)
    assert st == 0
    lines = open("report.out").read().splitlines()
    assert lines[:3] == ["total,kept,f_kept", "100,1,0.01", "200,1,0.005"]
    assert lines[-2:] == ["1000,1,0.001", "1001,1,0.000999"] and len(lines) == 12
    assert "... kept 1 of 100 or 1.0% sofar" in err and "... in file " + READ2 in err


def test_normalize_by_median_report_matches_sequential_loop(tmp_path, monkeypatch, capsys):
    """A report with kept counts that move: the lines of the per-unit loop
    over the same reads on the oracle."""
    monkeypatch.chdir(tmp_path)
    infile = data("random-20-a.fa")
    assert run(["-C", "1", "-k", "17", "-x", "1e5", "-N", "2", "-R", "report.out", "--report-frequency", "7",
                infile], capsys)[0] == 0
    ref = O.Table(O.BYTE, 17, O.get_n_primes_near_x(2, 1e5))
    want, total, kept, mark = ["total,kept,f_kept"], 0, 0, 7
    for _, s, _ in O.read_fastx(infile):
        s = s.upper().replace("N", "A")
        hashes = ref.kmer_hashes(s)
        total += 1
        if sum(1 for h in hashes if ref.get(h) >= 1) < int(0.5 + len(hashes) / 2.0):
            ref.consume(s)
            kept += 1
        if total >= mark:
            mark += 7
            want.append(S.report_line(total, kept))
            last = total
    if total != last:
        want.append(S.report_line(total, kept))
    assert open("report.out").read().splitlines() == want
    assert kept > 1


def test_normalize_by_median_single_output_and_gzip(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert run(["-C", "2", "-k", "17", READ2], capsys)[0] == 0
    per_file = open("test-abund-read-2.fa.keep", "rb").read()
    os.remove("test-abund-read-2.fa.keep")
    st, _, err = run(["-C", "2", "-k", "17", "-o", "single.fa", READ2, PAIRED], capsys)
    assert st == 0 and "output in single.fa" in err
    assert not os.path.exists("test-abund-read-2.fa.keep")
    assert open("single.fa", "rb").read().startswith(per_file)
    assert run(["-C", "2", "-k", "17", "-o", "single.fa.gz", "--gzip", READ2], capsys)[0] == 0
    assert gzip.decompress(open("single.fa.gz", "rb").read()) == per_file
    assert run(["-C", "2", "-k", "17", "--gzip", READ2], capsys)[0] == 0
    assert gzip.decompress(open("test-abund-read-2.fa.keep", "rb").read()) == per_file
    # -o over an existing file replaces it (reference test_normalize_by_median_overwrite)
    shutil.copy(READ2, "old.fa")
    assert run(["-C", "1", "-k", "17", "-o", "old.fa", data("test-abund-read-3.fa")], capsys)[0] == 0
    got = seqs("old.fa")
    assert len(got) == 1 and "GACAGCgtgCCGCA" in got[0]


def test_normalize_by_median_outfile_two_inputs(tmp_path, monkeypatch, capsys):
    """reference test_normalize_by_median_outfile_closed_err"""
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-o", "outfile_xxx", data("paired-mixed.fa.pe"), READ2], capsys)
    assert st == 0, err
    assert os.path.getsize("outfile_xxx") > 0


def test_normalize_by_median_savegraph_loadgraph(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", "-x", "1e5", "-N", "2", "-s", "saved.ct", READ2], capsys)
    assert st == 0 and "...saving to saved.ct" in err
    ref = O.Table(O.BYTE, 17, O.get_n_primes_near_x(2, 1e5))
    first = seqs("test-abund-read-2.fa.keep")[0]
    ref.consume(first.upper().replace("N", "A"))
    g = khmer.Countgraph.load("saved.ct")
    assert [bytes(t) for t in g.get_raw_tables()] == [ref.table_bytes(i) for i in range(2)]
    # a second pass over the same reads from the saved table keeps nothing
    st, _, err = run(["-C", "1", "--loadgraph", "saved.ct", "-o", "second.fa", READ2], capsys)
    assert st == 0 and "loading k-mer countgraph from saved.ct" in err
    assert "kept 0 of 1001" in err and os.path.getsize("second.fa") == 0
    # table options next to --loadgraph are ignored, with the reference's warning
    st, _, err = run(["--ksize", "7", "--loadgraph", "saved.ct", "-U", "83", "-o", "third.fa", READ2], capsys)
    assert st == 0
    assert "WARNING: You are loading a saved k-mer countgraph from" in err
    assert "WARNING: You have asked that the graph size be auto" in err and "NOT be set automatically" in err
    assert " - kmer size =     17 " in err


def test_normalize_by_median_indent(tmp_path, monkeypatch, capsys):
    """reference test_normalize_by_median_indent: a saved k = 20 table."""
    monkeypatch.chdir(tmp_path)
    with gzip.open(data("normC20k20.ct.gz"), "rb") as src, open("normC20k20.ct", "wb") as dst:
        shutil.copyfileobj(src, dst)
    st, _, err = run(["--loadgraph", "normC20k20.ct", "-o", "out.keep", data("paired-mixed.fa.pe")], capsys)
    assert st == 0, err
    assert os.path.exists("out.keep")


def test_normalize_by_median_force_skips_bad_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    bad = data("truncated.fq")
    st, _, err = run(["-f", "-C", "1", "-k", "17", bad, READ2], capsys)
    assert st == 0, err
    assert "** ERROR: " in err and "** Failed on " + bad in err
    assert "*** Skipping error file, moving on..." in err
    assert "** I/O Errors occurred in the following files:" in err and "\t" + bad in err
    assert not os.path.exists("truncated.fq.keep")
    assert len(seqs("test-abund-read-2.fa.keep")) == 1
    # without -f the first bad file ends the run
    st, _, err = run(["-C", "1", "-k", "17", bad, READ2], capsys)
    assert st == 1 and "** Exiting!" in err and "Skipping" not in err


def test_normalize_by_median_unforced_badfile(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-C", "1", "-k", "17", str(tmp_path / "potatoes")], capsys)
    assert st != 0
    assert "ERROR: [Errno 2] No such file or directory:" in err
    assert not os.path.exists("potatoes.keep")


def test_normalize_by_median_stdin_no_out(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    for name in ("-", "/dev/stdin"):
        st, _, err = run([name], capsys)
        assert st != 0 and "Accepting input from stdin; output filename" in err
    assert os.listdir(str(tmp_path)) == []


def test_normalize_by_median_double_file_name(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    copy = shutil.copy(READ2, str(tmp_path / "test-abund-read-2.fa"))
    st, _, err = run([READ2, copy], capsys)
    assert st != 0 and "Duplicate filename--Cannot handle this!" in err
    # one output file for all: the same base name twice is fine
    assert run(["-C", "1", "-k", "17", "-o", "both.fa", READ2, copy], capsys)[0] == 0


def test_normalize_by_median_empty_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run([data("empty-file")], capsys)
    assert st == 0, err
    assert "WARNING:" in err and "is empty" in err and "SKIPPED" in err
    assert os.path.exists("empty-file.keep")


def test_normalize_by_median_Ns(tmp_path, monkeypatch, capsys):
    """test-filter-abund-Ns.fq: N counts as A (reference
    test_normalize_by_median_streaming_1 and sanity_check_2)."""
    monkeypatch.chdir(tmp_path)
    infile = data("test-filter-abund-Ns.fq")
    st, _, err = run(["-C", "20", "-k", "17", "-o", "outfile", infile], capsys)
    assert st == 0 and "Total number of unique k-mers: 98" in err
    st, _, err = run(["-U", "83", infile], capsys)
    assert st == 0
    assert "*** INFO: set memory ceiling automatically." in err and "*** Ceiling is: 1e+06 bytes" in err


def test_normalize_by_median_fpr(tmp_path, monkeypatch, capsys):
    """A table far too small: the .keep file is there, the run fails."""
    monkeypatch.chdir(tmp_path)
    st, _, err = run(["-f", "-k", "17", "-x", "12", READ2], capsys)
    assert st != 0
    assert os.path.exists("test-abund-read-2.fa.keep")
    assert "** ERROR: the graph structure is too small" in err


def test_normalize_by_median_entry_point(tmp_path):
    script = os.path.join(ROOT, "scripts", "normalize-by-median.py")
    r = subprocess.run([sys.executable, script, "-C", "1", "-k", "17", READ2],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Total number of unique k-mers: 98" in r.stderr
    out = str(tmp_path / "test-abund-read-2.fa.keep")
    assert len(seqs(out)) == 1
    # reads from stdin, with -o; '-o -' writes to stdout
    with open(READ2, "rb") as fh:
        r = subprocess.run([sys.executable, script, "-q", "-C", "1", "-k", "17", "-", "-o", "-"], stdin=fh,
                           cwd=str(tmp_path), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(out, "rb").read()
    r = subprocess.run([sys.executable, script, "--version"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert [ln for ln in r.stderr.splitlines() if ln.strip() and not ln.startswith("||")][0].startswith("khmer ")
