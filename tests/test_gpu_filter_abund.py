"""scripts/filter-abund.py on the device, in-process, pinned to the reference's
own script tests (reference tests/test_filter_abund.py:42-148, 224-322): the
table comes from `load-into-counting.py -k 17 -x 1e7 -N 2`, outputs land in
the working directory as basename(input) + '.abundfilt'."""
import gzip
import os
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
READ3 = data("test-abund-read-3.fa")
READ2_FQ = data("test-abund-read-2.fq")
TRIMMED = "GGTTGACGGGGCTCAGGGGGCGGCTGACTCCGAGAGACAGC"
STDIN_MESSAGE = "Accepting input from stdin; output filename must be provided with -o."


@pytest.fixture(scope="module")
def counting(tmp_path_factory):
    """_make_counting(infile, K=17) of the reference's tests, one table per input."""
    made = {}

    def make(infile):
        if infile not in made:
            out = str(tmp_path_factory.mktemp("ct") / "counting.ct")
            assert S.load_into_counting(["-q", "-x", "1e7", "-N", "2", "-k", "17", out, infile]) == 0
            made[infile] = out
        return made[infile]
    return make


def run(argv, capsys):
    KA.configure_logging(False)
    try:
        status = S.filter_abund(argv)
    except SystemExit as e:
        status = e.code if isinstance(e.code, int) else 1
    out, err = capsys.readouterr()
    return status, out, err


def records(path):
    return list(O.read_fastx(path))


def seqs(path):
    return set(s for _, s, _ in records(path))


def test_filter_abund_1(counting, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, _, err = run([counting(READ2), READ2], capsys)
    assert st == 0 and "output in test-abund-read-2.fa.abundfilt" in err
    assert seqs("test-abund-read-2.fa.abundfilt") == {"GGTTGACGGGGCTCAGGG"}
    raw = open("test-abund-read-2.fa.abundfilt").read()
    assert raw.startswith(">") and raw.count("\n") == 2 * raw.count(">")   # >name\nseq\n


def test_filter_abund_2(counting, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert run(["-C", "1", counting(READ2), READ2, READ2], capsys)[0] == 0
    got = seqs("test-abund-read-2.fa.abundfilt")
    assert len(got) == 2 and "GGTTGACGGGGCTCAGGG" in got


def test_filter_abund_quiet(counting, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    st, out, err = run(["-q", counting(READ2), READ2], capsys)
    assert (st, out, err) == (0, "", "") and os.path.exists("test-abund-read-2.fa.abundfilt")


def test_filter_abund_3_fq_retained(counting, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert run(["-C", "1", counting(READ2_FQ), READ2_FQ, READ2_FQ], capsys)[0] == 0
    recs = records("test-abund-read-2.fq.abundfilt")
    got = set(s for _, s, _ in recs)
    assert len(got) == 2 and "GGTTGACGGGGCTCAGGG" in got
    quals = set(q for _, _, q in recs)
    assert len(quals) == 2 and "#" * 18 in quals
    assert all(len(s) == len(q) for _, s, q in recs)
    assert open("test-abund-read-2.fq.abundfilt").read().startswith("@")


def test_filter_abund_4_retain_low_abund(counting, tmp_path, monkeypatch, capsys):
    """-V does not trim reads of low coverage."""
    monkeypatch.chdir(tmp_path)
    assert run(["-V", counting(READ2), READ2], capsys)[0] == 0
    got = seqs("test-abund-read-2.fa.abundfilt")
    assert len(got) == 2 and "GGTTGACGGGGCTCAGGG" in got


def test_filter_abund_5_trim_high_abund(counting, tmp_path, monkeypatch, capsys):
    """-V does trim reads of high coverage."""
    monkeypatch.chdir(tmp_path)
    assert run(["-V", counting(READ3), READ3], capsys)[0] == 0
    got = seqs("test-abund-read-3.fa.abundfilt")
    assert len(got) == 2 and TRIMMED in got


def test_filter_abund_6_trim_high_abund_Z(counting, tmp_path, monkeypatch, capsys):
    """-Z high enough: no trimming."""
    monkeypatch.chdir(tmp_path)
    assert run(["-V", "-Z", "25", counting(READ3), READ3], capsys)[0] == 0
    got = seqs("test-abund-read-3.fa.abundfilt")
    assert len(got) == 2 and TRIMMED not in got
    assert TRIMMED + "gtgCCGCAGCTGTCGTCAGGGGATTTCCGGGCGG" in got     # there, untrimmed


def test_filter_abund_single_output_and_gzip(counting, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    ct = counting(READ2)
    assert run(["-C", "1", ct, READ2, READ2], capsys)[0] == 0
    per_file = open("test-abund-read-2.fa.abundfilt", "rb").read()
    os.remove("test-abund-read-2.fa.abundfilt")
    out = str(tmp_path / "sub" / "single.fa")
    os.mkdir(os.path.dirname(out))
    assert run(["-C", "1", ct, READ2, READ2, "-o", out], capsys)[0] == 0
    assert not os.path.exists("test-abund-read-2.fa.abundfilt")
    # the per-input file is rewritten for every input; -o holds both passes
    assert open(out, "rb").read() == per_file + per_file
    assert run(["-C", "1", ct, READ2, "-o", out + ".gz", "--gzip"], capsys)[0] == 0
    assert gzip.decompress(open(out + ".gz", "rb").read()) == per_file
    assert run(["-C", "1", ct, READ2, "--gzip"], capsys)[0] == 0
    assert gzip.decompress(open("test-abund-read-2.fa.abundfilt", "rb").read()) == per_file


def test_filter_abund_matches_trim_record(counting, tmp_path, monkeypatch, capsys):
    """The batched script writes what the reference's per-read loop would:
    trim_record over every read of at least k bases, in order."""
    from khmer_amd.trimming import trim_record
    monkeypatch.chdir(tmp_path)
    ct = counting(READ3)
    assert run(["-V", ct, READ3], capsys)[0] == 0
    g = khmer.Countgraph.load(ct)
    want, trimmed = [], 0
    for read in khmer.ReadParser(READ3):
        if len(read.sequence) < 17:
            continue
        rec, did = trim_record(g, read, 2, True, 20)
        if rec:
            want.append((rec.name, rec.sequence, ""))
            trimmed += 1 if did else 0
    assert records("test-abund-read-3.fa.abundfilt") == want
    assert trimmed > 0 and len(want) - trimmed > 0, (len(want), trimmed)


def test_filter_abund_stdin_needs_output(counting, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    for name in ("-", "/dev/stdin"):
        st, _, err = run(["-C", "1", counting(READ2), name], capsys)
        assert st == 1 and STDIN_MESSAGE in err
    assert os.listdir(str(tmp_path)) == []


def test_filter_abund_entry_point(counting, tmp_path):
    script = os.path.join(ROOT, "scripts", "filter-abund.py")
    r = subprocess.run([sys.executable, script, counting(READ2), READ2],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "filtering " + READ2 in r.stderr
    out = str(tmp_path / "test-abund-read-2.fa.abundfilt")
    assert seqs(out) == {"GGTTGACGGGGCTCAGGG"}
    # reads from stdin, with -o
    with open(READ2, "rb") as fh:
        r = subprocess.run([sys.executable, script, "-q", counting(READ2), "-", "-o", "piped.fa"], stdin=fh,
                           cwd=str(tmp_path), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "piped.fa"), "rb").read() == open(out, "rb").read()
