"""Table-sizing helpers (khmer/_oxli/utils.pyx:12-17 over
include/oxli/hashtable.hh:79-123), computed by libkhmer_hip.so, and the
pairing helpers of the read-filtering scripts (khmer/utils.py:48-118,
khmer/_oxli/parsing.pyx:150-156, 414-488), plain Python over any records with
`name`, `sequence` and an optional `quality`."""
import ctypes

from ._lib import lib, check


class UnpairedReadsError(ValueError):
    """ValueError that keeps the two records at fault
    (khmer/_oxli/parsing.pyx:150-156)."""

    def __init__(self, msg, r1, r2):
        r1_name = r1.name if r1 else "<no read>"
        r2_name = r2.name if r2 else "<no read>"
        super(UnpairedReadsError, self).__init__(msg + '\n"{0}"\n"{1}"'.format(r1_name, r2_name))
        self.read1 = r1
        self.read2 = r2


def _split_left_right(name):
    """A record name cut at its first blank or tab: (left, right), right
    empty when there is none (khmer/_oxli/parsing.pyx:414-433; the right part
    starts at the character after that first separator)."""
    for i, c in enumerate(name):
        if c in " \t" and i > 0:
            return name[:i], name[i + 1:]
    return name, ""


def check_is_pair(first, second):
    """True when the two records are the left and right read of one fragment
    (khmer/_oxli/parsing.pyx:436-488): 'name/1' + 'name/2', Casava 1.8
    'name 1:...' + 'name 2:...', or fastq-dump's 'accession name/1' +
    'accession name/2'.  ValueError when one is FASTA and the other FASTQ."""
    q1, q2 = getattr(first, "quality", None), getattr(second, "quality", None)
    if (q1 is None) != (q2 is None):
        raise ValueError("both records must be same type (FASTA or FASTQ)")
    lhs1, rhs1 = _split_left_right(first.name)
    lhs2, rhs2 = _split_left_right(second.name)
    if lhs1.endswith("/1") and lhs2.endswith("/2"):
        stem1, stem2 = lhs1.split("/", 1)[0], lhs2.split("/", 1)[0]
        return bool(stem1) and stem1 == stem2
    if lhs1 == lhs2 and rhs1.startswith("1:") and rhs2.startswith("2:"):
        return True
    if lhs1 == lhs2 and rhs1.endswith("/1") and rhs2.endswith("/2"):
        stem1, stem2 = rhs1.split("/", 1)[0], rhs2.split("/", 1)[0]
        return bool(stem1) and stem1 == stem2
    return False


def broken_paired_reader(records, min_length=None, force_single=False, require_paired=False):
    """Singletons and pairs from a stream of records that may be single-ended,
    interleaved, or interleaved with orphans (khmer/utils.py:48-118).  Yields
    (n, is_pair, read1, read2) with read2 None for a singleton; n counts the
    records yielded before this item.

    With min_length, reads below it are ignored: a short singleton is
    skipped, and a pair with a short read is not yielded as a pair (under
    require_paired both its reads are dropped, without an error; otherwise
    its second read stays in hand and goes on as a singleton candidate).
    require_paired raises UnpairedReadsError at the first orphan."""
    if force_single and require_paired:
        raise ValueError("force_single and require_paired cannot both be set!")

    def too_short(rec):
        return bool(min_length) and len(rec.sequence) < min_length

    num = 0
    held = None                       # the record waiting for its mate
    for record in records:
        if held is not None:
            if not force_single and check_is_pair(held, record):
                if too_short(held) or too_short(record):
                    if require_paired:
                        record = None
                else:
                    yield num, True, held, record
                    num += 2
                    record = None
            else:
                if require_paired:
                    raise UnpairedReadsError("Unpaired reads when require_paired is set!", held, record)
                if not too_short(held):
                    yield num, False, held, None
                    num += 1
        held = record
    if held is not None:
        if require_paired:
            raise UnpairedReadsError("Unpaired reads when require_paired is set!", held, None)
        if not too_short(held):
            yield num, False, held, None


def get_n_primes_near_x(n_primes, x):
    """The n largest primes strictly below x (x == 1 gives [1])."""
    n = int(n_primes)
    out = (ctypes.c_uint64 * max(n, 1))()
    found = ctypes.c_uint32()
    check(lib.kh_get_n_primes_near_x(n, int(x), out, ctypes.byref(found)))
    if found.value != n:
        raise RuntimeError("unable to find %d prime numbers < %d" % (n, int(x)))
    return [int(v) for v in out[:n]]


def is_prime(n):
    out = ctypes.c_int()
    check(lib.kh_is_prime(int(n), ctypes.byref(out)))
    return bool(out.value)
