"""The drop-in scripts on the hot path, as importable functions.

`load_into_counting(argv)` is scripts/load-into-counting.py
(reference scripts/load-into-counting.py:60-218), `load_graph(argv)` is
scripts/load-graph.py (reference scripts/load-graph.py + oxli/build_graph.py:
40-123) and `filter_abund(argv)` is scripts/filter-abund.py (reference
scripts/filter-abund.py:68-168; it trims FILTER_BATCH_READS reads per device
pass instead of one call per read, and spools stdin to a temporary file);
`normalize_by_median(argv)` is scripts/normalize-by-median.py (reference
scripts/normalize-by-median.py:72-419; NORMALIZE_BATCH_READS reads per device
call of Hashtable.normalize_by_median_batch, the progress report replayed
from the keep flags).
Options, stderr messages, the saved table, the `.info` file, the
`.info.json` / `.info.tsv` summaries and the `.tagset` file match the
reference's.  Each input file is consumed as the reference does it: `-T`
Python threads all call consume_seqfile[_and_tag] on one shared ReadParser
(scripts/load-into-counting.py:143-158, oxli/functions.py:56-66).  The first
call drains the parser into the device pipeline; the others find it drained
and return their (empty) share, so the tables and counters do not depend on
-T.  One deliberate difference: an exception in a consuming thread is
re-raised in the main thread after the join (the reference's thread prints
it and the script carries on).  The tests call these functions in-process;
the files under scripts/ are two-line wrappers.
"""
import json
import os
import shutil
import sys
import tempfile
import threading

from . import khmer_args as KA


def consume_threads(eat, parser, num_threads):
    """`num_threads` threads calling eat(parser) on one shared parser; their
    (reads, k-mers) shares, and the first exception re-raised after the join."""
    shares, errors = [], []

    def run():
        try:
            shares.append(eat(parser))
        except BaseException as e:   # re-raised in the caller below
            errors.append(e)

    threads = [threading.Thread(target=run) for _ in range(max(1, int(num_threads)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return shares


# ---------------------------------------------------------------------------
# load-into-counting.py

_LIC_EPILOG = """\
    Note: with -b/--no-bigcount the output will be the exact size of the
    k-mer countgraph and this script will use a constant amount of memory.
    In exchange k-mer counts will stop at 255.

    Example:

        load-into-counting.py -k 20 -x 5e7 out data/100k-filtered.fa
    """


def load_into_counting_parser():
    parser = KA.build_counting_args("Build a k-mer countgraph from the given sequences.",
                                    epilog=KA.dedent(_LIC_EPILOG))
    parser.prog = "load-into-counting.py"
    KA.add_threading_args(parser)
    parser.add_argument("output_countgraph_filename",
                        help="The name of the file to write the k-mer countgraph to.")
    parser.add_argument("input_sequence_filename", nargs="+",
                        help="The names of one or more FAST[AQ] input sequence files.")
    parser.add_argument("-b", "--no-bigcount", dest="bigcount", default=True,
                        action="store_false",
                        help="Turn bigcount off, limiting counts to 255.")
    parser.add_argument("-s", "--summary-info", type=str, default=None, metavar="FORMAT",
                        choices=["json", "tsv"],
                        help="What format should the machine readable run summary be in? "
                             "(`json` or `tsv`, disabled by default)")
    parser.add_argument("-f", "--force", default=False, action="store_true",
                        help="Overwrite output file if it exists")
    parser.add_argument("-q", "--quiet", dest="quiet", default=False, action="store_true")
    return parser


def _write_summary(fmt, path, base, fp_rate, n_kmers, n_reads, filenames):
    with open(path, "w") as fh:
        if fmt == "json":
            json.dump({"ht_name": os.path.basename(base), "fpr": fp_rate, "num_kmers": n_kmers,
                       "files": filenames, "mrinfo_version": "0.2.0", "num_reads": n_reads}, fh)
            fh.write("\n")
        else:
            fh.write("ht_name\tfpr\tnum_kmers\tnum_reads\tfiles\n")
            fh.write("\t".join([os.path.basename(base), "{:1.3f}".format(fp_rate), str(n_kmers),
                                str(n_reads), ";".join(filenames)]) + "\n")


def load_into_counting(argv=None):
    import khmer_amd
    args = load_into_counting_parser().parse_args(argv)
    KA.configure_logging(args.quiet)
    KA.report_on_config(args)

    base = args.output_countgraph_filename
    filenames = args.input_sequence_filename
    for name in filenames:
        KA.check_input_files(name, args.force)
    KA.check_space_for_graph(base, KA.calculate_graphsize(args, "countgraph"), args.force)
    info_filename = base + ".info"
    KA.check_file_writable(base)
    KA.check_file_writable(info_filename)

    KA.log_info("Saving k-mer countgraph to {base}", base=base)
    KA.log_info("Loading kmers from sequences in {filenames}", filenames=repr(filenames))
    with open(info_filename, "w") as fh:
        print("khmer version:", khmer_amd.__version__, file=fh)

    KA.log_info("making countgraph")
    countgraph = KA.create_countgraph(args)

    total_reads = 0
    for index, filename in enumerate(filenames):
        parser = khmer_amd.ReadParser(filename)
        KA.log_info("consuming input {input}", input=filename)
        consume_threads(countgraph.consume_seqfile, parser, args.threads)
        if index > 0 and index % 10 == 0:     # periodic checkpoint, as the reference
            KA.check_space_for_graph(base, KA.calculate_graphsize(args, "countgraph"), args.force)
            KA.log_info("mid-save {base}", base=base)
            countgraph.save(base)
        with open(info_filename, "a") as fh:
            print("through", filename, file=fh)
        total_reads += parser.num_reads
        parser.close()

    n_kmers = countgraph.n_unique_kmers()
    KA.log_info("Total number of unique k-mers: {nk}", nk=n_kmers)
    with open(info_filename, "a") as fh:
        print("Total number of unique k-mers:", n_kmers, file=fh)

    KA.log_info("saving {base}", base=base)
    countgraph.save(base)

    fp_rate = khmer_amd.calc_expected_collisions(countgraph, args.force, max_false_pos=.2)
    with open(info_filename, "a") as fh:
        print("fp rate estimated to be %1.3f\n" % fp_rate, file=fh)

    if args.summary_info:
        fmt = args.summary_info.lower()
        mr_file = base + ".info." + fmt
        KA.log_info("Writing summmary info to {mr_file}", mr_file=mr_file)
        _write_summary(fmt, mr_file, base, fp_rate, n_kmers, total_reads, filenames)

    KA.log_info("fp rate estimated to be {fpr:1.3f}", fpr=fp_rate)
    KA.log_info("DONE.")
    KA.log_info("wrote to: {filename}", filename=info_filename)
    return 0


# ---------------------------------------------------------------------------
# load-graph.py


def load_graph_parser():
    parser = KA.build_nodegraph_args(
        descr="Load sequences into the compressible graph format plus optional tagset.")
    parser.prog = "load-graph.py"
    KA.add_threading_args(parser)
    parser.add_argument("--no-build-tagset", "-n", default=False, action="store_true",
                        dest="no_build_tagset",
                        help="Do NOT construct tagset while loading sequences")
    parser.add_argument("output_filename", metavar="output_nodegraph_filename",
                        help="output k-mer nodegraph filename.")
    parser.add_argument("input_filenames", metavar="input_sequence_filename", nargs="+",
                        help="input FAST[AQ] sequence filename")
    parser.add_argument("-f", "--force", default=False, action="store_true",
                        help="Overwrite output file if it exists")
    return parser


def build_graph(filenames, graph, num_threads=1, tags=False):
    """Consume every file into graph, tagging when asked
    (oxli/functions.py:42-66)."""
    import khmer_amd
    eat = graph.consume_seqfile_and_tag if tags else graph.consume_seqfile
    for name in filenames:
        parser = khmer_amd.ReadParser(name)
        consume_threads(eat, parser, num_threads)
        parser.close()


def load_graph(argv=None):
    import khmer_amd
    args = load_graph_parser().parse_args(argv)
    KA.report_on_config(args, graphtype="nodegraph")
    base = args.output_filename
    filenames = args.input_filenames
    for name in filenames:
        KA.check_input_files(name, args.force)
    size = KA.calculate_graphsize(args, "nodegraph")
    KA.check_space_for_graph(base, args.n_tables * size / khmer_amd._buckets_per_byte["nodegraph"],
                             args.force)

    err = sys.stderr
    print("Saving k-mer nodegraph to %s" % base, file=err)
    print("Loading kmers from sequences in %s" % repr(filenames), file=err)
    if args.no_build_tagset:
        print("We WILL NOT build the tagset.", file=err)
    else:
        print("We WILL build the tagset (for partitioning/traversal).", file=err)

    print("making nodegraph", file=err)
    nodegraph = KA.create_nodegraph(args)
    build_graph(filenames, nodegraph, args.threads, not args.no_build_tagset)

    n_unique = nodegraph.n_unique_kmers()
    print("Total number of unique k-mers: {0}".format(n_unique), file=err)
    print("saving k-mer nodegraph in", base, file=err)
    nodegraph.save(base)
    if not args.no_build_tagset:
        print("saving tagset in", base + ".tagset", file=err)
        nodegraph.save_tagset(base + ".tagset")

    with open(base + ".info", "w") as info:
        info.write("%d unique k-mers" % n_unique)
        fp_rate = khmer_amd.calc_expected_collisions(nodegraph, args.force, max_false_pos=.15)
        print("false positive rate estimated to be %1.3f" % fp_rate, file=err)
        print("\nfalse positive rate estimated to be %1.3f" % fp_rate, file=info)

    print("wrote to " + base + ".info and " + base, file=err)
    if not args.no_build_tagset:
        print("and " + base + ".tagset", file=err)
    return 0


# ---------------------------------------------------------------------------
# filter-abund.py

DEFAULT_NORMALIZE_LIMIT = 20
DEFAULT_CUTOFF = 2
FILTER_BATCH_READS = 1 << 16     # reads per device pass of filter_abund

_FA_EPILOG = """\
    Every input file gets its own output, named after the input's base name
    plus ``.abundfilt`` and written to the working directory, unless -o names
    one file for all of them.  Use --variable-coverage for data of uneven
    coverage (transcriptomes, metagenomes).

    Example:

        load-into-counting.py -k 20 -x 5e7 countgraph reads.fa
        filter-abund.py -C 2 countgraph reads.fa
    """


def filter_abund_parser():
    parser = KA.KhmerArgumentParser(description="Trim reads at their first k-mer of low abundance.",
                                    epilog=KA.dedent(_FA_EPILOG), citations=["counting"])
    parser.prog = "filter-abund.py"
    parser.add_argument("input_graph", metavar="input_count_graph_filename",
                        help="countgraph file written by load-into-counting.py")
    parser.add_argument("input_filename", metavar="input_sequence_filename", nargs="+",
                        help="FASTA / FASTQ file of reads to trim")
    KA.add_threading_args(parser)
    parser.add_argument("-C", "--cutoff", dest="cutoff", default=DEFAULT_CUTOFF,
                        type=KA.check_argument_range(0, 256, "cutoff"),
                        help="cut a read at its first k-mer counted fewer times than this")
    parser.add_argument("-V", "--variable-coverage", action="store_true", dest="variable_coverage",
                        default=False,
                        help="leave reads alone unless their median k-mer count reaches -Z")
    parser.add_argument("-Z", "--normalize-to", type=int, dest="normalize_to", default=DEFAULT_NORMALIZE_LIMIT,
                        help="median k-mer count from which -V lets a read be trimmed")
    parser.add_argument("-o", "--output", dest="single_output_file", metavar="optional_output_filename",
                        help="write every input's reads to this one file ('-': stdout)")
    parser.add_argument("-f", "--force", default=False, action="store_true",
                        help="go on past missing inputs and a full disk")
    parser.add_argument("-q", "--quiet", dest="quiet", default=False, action="store_true")
    KA.add_output_compression_type(parser)
    return parser


def write_record(record, fileobj):
    """FASTA, or FASTQ for a record with a quality (khmer/utils.py:120-135)."""
    if getattr(record, "quality", None) is not None:
        recstr = "@{}\n{}\n+\n{}\n".format(record.name, record.sequence, record.quality)
    else:
        recstr = ">{}\n{}\n".format(record.name, record.sequence)
    fileobj.write(recstr.encode("ascii"))


def filter_abund(argv=None):
    import khmer_amd
    from .trimming import trim_records
    args = filter_abund_parser().parse_args(argv)
    KA.configure_logging(args.quiet)

    infiles = args.input_filename
    if ("-" in infiles or "/dev/stdin" in infiles) and not args.single_output_file:
        KA.log_error("Accepting input from stdin; output filename must be provided with -o.")
        sys.exit(1)
    for filename in infiles:
        KA.check_input_files(filename, args.force)
    KA.check_space(infiles, args.force)

    KA.log_info("loading countgraph: {graph}", graph=args.input_graph)
    countgraph = khmer_amd.Countgraph.load(args.input_graph)
    ksize = countgraph.ksize()
    KA.log_info("K: {ksize}", ksize=ksize)

    def open_out(name):
        raw = sys.stdout.buffer if name == "-" else open(name, "wb")
        return raw, KA.get_file_writer(raw, args.gzip, args.bzip)

    def filter_batch(batch, outfp):
        for rec, _ in trim_records(countgraph, batch, args.cutoff, args.variable_coverage, args.normalize_to):
            if rec:
                write_record(rec, outfp)

    def close_out(raw, outfp):
        if outfp is not raw:
            outfp.close()        # the compressor's trailer
        if raw is not sys.stdout.buffer:
            raw.close()
        else:
            raw.flush()

    if args.single_output_file:
        outfile = args.single_output_file
        raw, outfp = open_out(outfile)
    for infile in infiles:
        KA.log_info("filtering {infile}", infile=infile)
        if not args.single_output_file:
            outfile = os.path.basename(infile) + ".abundfilt"
            raw, outfp = open_out(outfile)
        spool = None
        if infile in ("-", "/dev/stdin"):    # the parser wants a file it can reopen: spool the pipe
            spool = tempfile.NamedTemporaryFile(prefix="filter-abund-stdin-")
            shutil.copyfileobj(sys.stdin.buffer, spool)
            spool.flush()
        parser = khmer_amd.ReadParser(spool.name if spool else infile)
        batch = []
        for read in parser:
            if len(read.sequence) < ksize:   # broken_paired_reader(min_length=ksize, force_single=True)
                continue
            batch.append(read)
            if len(batch) >= FILTER_BATCH_READS:
                filter_batch(batch, outfp)
                batch = []
        filter_batch(batch, outfp)
        parser.close()
        if spool:
            spool.close()
        if not args.single_output_file:
            close_out(raw, outfp)
        KA.log_info("output in {outfile}", outfile=outfile)
    if args.single_output_file:
        close_out(raw, outfp)
    return 0


# ---------------------------------------------------------------------------
# normalize-by-median.py

DEFAULT_DESIRED_COVERAGE = 20
NORMALIZE_BATCH_READS = 1 << 16     # reads per device call of normalize_by_median

_NBM_EPILOG = """\
    Discard sequences based on whether or not their median k-mer abundance lies
    above a specified cutoff. Kept sequences will be placed in <fileN>.keep.

    By default, paired end reads will be considered together; if either read
    should be kept, both will be kept.  Unpaired reads are treated
    individually.  With -p/--paired proper pairing is required and the script
    exits on unpaired reads; --unpaired-reads names a file of orphan reads
    to be read after the paired ones.  --force_single ignores all pairing
    information.

    -s/--savegraph saves the k-mer countgraph after all sequences have been
    processed; -l/--loadgraph loads one before processing.  The files are those
    of load-into-counting.py.

    Example:

        normalize-by-median.py -k 17 -C 20 -p reads.pe.fq
    """


def normalize_by_median_parser():
    parser = KA.build_counting_args(descr="Do digital normalization (remove mostly redundant sequences)",
                                    epilog=KA.dedent(_NBM_EPILOG), citations=["diginorm"])
    parser.prog = "normalize-by-median.py"
    parser.add_argument("-q", "--quiet", dest="quiet", default=False, action="store_true")
    parser.add_argument("-C", "--cutoff", type=KA.check_argument_range(0, 256, "cutoff"),
                        default=DEFAULT_DESIRED_COVERAGE,
                        help="when the median k-mer coverage level is above this number the read is not kept.")
    parser.add_argument("-p", "--paired", action="store_true",
                        help="require that all sequences be properly paired")
    parser.add_argument("--force_single", dest="force_single", action="store_true",
                        help="treat all sequences as single-ended/unpaired")
    parser.add_argument("-u", "--unpaired-reads", metavar="unpaired_reads_filename",
                        help="include a file of unpaired reads to which -p/--paired does not apply.")
    parser.add_argument("-s", "--savegraph", metavar="filename", default=None,
                        help="save the k-mer countgraph to disk after all reads are loaded.")
    parser.add_argument("-R", "--report", metavar="report_filename",
                        help="write progress report to report_filename")
    parser.add_argument("--report-frequency", metavar="report_frequency", type=int, default=100000,
                        help="report progress every report_frequency reads")
    parser.add_argument("-f", "--force", dest="force", action="store_true",
                        help="continue past file reading errors")
    parser.add_argument("-o", "--output", metavar="filename", default=None, dest="single_output_file",
                        help="only output a single file with the specified filename; use a single dash \"-\" "
                             "to specify that output should go to STDOUT (the terminal)")
    parser.add_argument("input_filenames", metavar="input_sequence_filename", nargs="+",
                        help="Input FAST[AQ] sequence filename.")
    KA.add_loadgraph_args(parser)
    KA.add_output_compression_type(parser)
    return parser


class DiginormProgress(object):
    """The running total / kept counts of normalize-by-median.py and the
    points at which it reports them (scripts/normalize-by-median.py:72-152).
    The reference looks at the counts after every unit; here whole batches
    come back from the device, so advance() replays a batch's units from
    their keep flags and returns the (total, kept) pairs of every report due,
    the same ones the one-unit-at-a-time loop would give."""

    def __init__(self, report_frequency=100000):
        self.total = 0
        self.kept = 0
        self.report_frequency = report_frequency
        self.next_report_at = report_frequency
        self.last_report_at = report_frequency

    def advance(self, unit_sizes, unit_kept):
        due = []
        for size, kept in zip(unit_sizes, unit_kept):
            self.total += size
            if kept:
                self.kept += size
            if self.total >= self.next_report_at:
                self.next_report_at += self.report_frequency
                self.last_report_at = self.total
                due.append((self.total, self.kept))
        return due


def report_line(total, kept):
    """One line of the -R report (scripts/normalize-by-median.py:125-128)."""
    return "{total},{kept},{f_kept:.4}".format(total=total, kept=kept, f_kept=kept / float(total))


def _clean_input_reads(records):
    """khmer/utils.py:158-168: upper case, N -> A, as a plain attribute."""
    for record in records:
        record.cleaned = record.sequence.upper().replace("N", "A")
        yield record


class _NoReads(object):
    """Stands in for the parser of an empty input file."""

    def __iter__(self):
        return iter(())

    def close(self):
        pass


def normalize_by_median_args(argv=None):
    """Parsed options; -p with --force_single is refused (the reference stops
    on it with broken_paired_reader's ValueError at its first input)."""
    args = normalize_by_median_parser().parse_args(argv)
    if args.force_single and args.paired:
        KA.log_error("** ERROR: force_single and require_paired cannot both be set!")
        KA.log_error("** Exiting!")
        sys.exit(1)
    return args


def normalize_by_median(argv=None):
    import khmer_amd
    from .utils import broken_paired_reader
    args = normalize_by_median_args(argv)
    KA.configure_logging(args.quiet)
    KA.report_on_config(args)

    report_fp = open(args.report, "w") if args.report else None
    filenames = list(args.input_filenames)
    if not args.single_output_file:
        basenames = set()
        for name in filenames:
            base = os.path.basename(name)
            if base in basenames:
                KA.log_error("ERROR: Duplicate filename--Cannot handle this!")
                KA.log_error("** Exiting!")
                sys.exit(1)
            basenames.add(base)

    KA.check_valid_file_exists(filenames)
    KA.check_space(filenames, args.force)
    if args.savegraph is not None:
        KA.check_space_for_graph(args.savegraph, KA.calculate_graphsize(args, "countgraph"), args.force)

    if args.loadgraph:
        KA.log_info("loading k-mer countgraph from {graph}", graph=args.loadgraph)
        countgraph = khmer_amd.Countgraph.load(args.loadgraph)
    else:
        KA.log_info("making countgraph")
        countgraph = KA.create_countgraph(args)
    ksize = countgraph.ksize()

    progress = DiginormProgress(args.report_frequency)
    if report_fp:
        report_fp.write("total,kept,f_kept\n")

    files = [(name, args.paired) for name in filenames]
    if args.unpaired_reads:
        files.append((args.unpaired_reads, False))

    def open_out(name):
        raw = sys.stdout.buffer if name == "-" else open(name, "wb")
        return raw, KA.get_file_writer(raw, args.gzip, args.bzip)

    def close_out(raw, outfp):
        if outfp is not raw:
            outfp.close()        # the compressor's trailer
        if raw is not sys.stdout.buffer:
            raw.close()
        else:
            raw.flush()

    raw = outfp = None
    if args.single_output_file:
        raw, outfp = open_out(args.single_output_file)
    elif "-" in filenames or "/dev/stdin" in filenames:
        print("Accepting input from stdin; output filename must be provided with '-o'.", file=sys.stderr)
        sys.exit(1)

    def normalize_batch(units, filename):
        """One device call over the batch's units; writes the kept records."""
        if not units:
            return
        seqs, pairs = [], []
        for unit in units:
            for i, rec in enumerate(unit):
                seqs.append(rec.cleaned)
                pairs.append(i + 1 < len(unit))
        flags = countgraph.normalize_by_median_batch(seqs, args.cutoff, pairs=pairs)
        unit_kept, at = [], 0
        for unit in units:
            unit_kept.append(flags[at])
            if flags[at]:
                for rec in unit:
                    write_record(rec, outfp)
            at += len(unit)
        for total, kept in progress.advance([len(u) for u in units], unit_kept):
            KA.log_info("... kept {kept} of {tot} or {perc_kept:.1%} sofar", kept=kept, tot=total,
                        perc_kept=kept / float(total))
            KA.log_info("... in file {name}", name=filename)
            if report_fp:
                print(report_line(total, kept), file=report_fp)
                report_fp.flush()

    def normalize_file(filename, require_paired):
        reads_start = progress.total
        spool = None
        if filename in ("-", "/dev/stdin"):    # the parser wants a file it can reopen: spool the pipe
            spool = tempfile.NamedTemporaryFile(prefix="normalize-by-median-stdin-")
            shutil.copyfileobj(sys.stdin.buffer, spool)
            spool.flush()
        else:
            open(filename, "rb").close()       # a missing input fails here, with the system's message
        # an empty file is no error here: it is reported as SKIPPED below
        # (the parser itself refuses a file without sequences)
        empty = not spool and os.path.isfile(filename) and os.path.getsize(filename) == 0
        parser = _NoReads() if empty else khmer_amd.ReadParser(spool.name if spool else filename)
        units, nreads = [], 0
        try:
            reader = broken_paired_reader(_clean_input_reads(parser), min_length=ksize,
                                          force_single=args.force_single, require_paired=require_paired)
            while True:
                try:
                    _, is_pair, read1, read2 = next(reader)
                except StopIteration:
                    break
                except Exception:
                    # the units read before the error are normalized and written, as by
                    # the reference's one-unit-at-a-time loop
                    normalize_batch(units, filename)
                    raise
                units.append((read1, read2) if is_pair else (read1,))
                nreads += len(units[-1])
                if nreads >= NORMALIZE_BATCH_READS:
                    normalize_batch(units, filename)
                    units, nreads = [], 0
            normalize_batch(units, filename)
        finally:
            parser.close()
            if spool:
                spool.close()
        if progress.total == reads_start:
            KA.log_info("SKIPPED empty file {name}", name=filename)
        else:
            KA.log_info("DONE with {inp}; kept {kept} of {total} or {perc_kept:.1%}", inp=filename,
                        kept=progress.kept, total=progress.total,
                        perc_kept=progress.kept / float(progress.total))
        if report_fp and progress.total != progress.last_report_at:
            print(report_line(progress.total, progress.kept), file=report_fp)
            report_fp.flush()

    corrupt_files = []
    for filename, require_paired in files:
        if not args.single_output_file:
            output_name = os.path.basename(filename) + ".keep"
            raw, outfp = open_out(output_name)
        try:
            normalize_file(filename, require_paired)
            KA.log_info("output in {name}", name=KA.describe_file_handle(raw))
            if not args.single_output_file:
                close_out(raw, outfp)
        except (IOError, OSError, ValueError) as error:
            KA.log_error("** ERROR: {error}", error=str(error))
            KA.log_error("** Failed on {name}: ", name=filename)
            if not args.single_output_file:
                close_out(raw, outfp)
                os.remove(output_name)
            if not args.force:
                KA.log_error("** Exiting!")
                sys.exit(1)
            KA.log_error("*** Skipping error file, moving on...")
            corrupt_files.append(filename)
    if args.single_output_file:
        close_out(raw, outfp)

    KA.log_info("Total number of unique k-mers: {umers}", umers=countgraph.n_unique_kmers())
    if args.savegraph is not None:
        KA.log_info("...saving to {name}", name=args.savegraph)
        countgraph.save(args.savegraph)

    # for max_false_pos see Zhang et al., http://arxiv.org/abs/1309.2975
    fp_rate = khmer_amd.calc_expected_collisions(countgraph, False, max_false_pos=.8)
    KA.log_info("fp rate estimated to be {fpr:1.3f}", fpr=fp_rate)

    if args.force and corrupt_files:
        KA.log_error("** WARNING: Finished with errors!")
        KA.log_error("** I/O Errors occurred in the following files:")
        KA.log_error("\t" + " ".join(corrupt_files))
    if report_fp:
        report_fp.close()
    return 0


def run(fn):
    """Entry used by scripts/*.py: exit with fn's status."""
    sys.exit(fn())
