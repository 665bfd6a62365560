"""Trimming reads where their k-mers become rare, the contract of
khmer/trimming.py:38-67.

`trim_record` keeps the reference's contract, `(record, did_trim)`:
`(None, True)` for a read whose trusted prefix is shorter than k,
`(record, False)` (the same object) for a read left as it is, and a new record
with sequence and quality cut otherwise.  Records are khmer_amd.parsing.Read
(there is no screed here).  `trim_records` is the same over a list of records
in one device pass: the median_at_least gate and the trim position of every
read come from one kh_trim_on_abundance call.
"""
from .parsing import Read


def _apply(countgraph, record, trim_at):
    seq = record.sequence
    # nothing of k bases or more is left: the read is dropped
    if trim_at < countgraph.ksize():
        return None, True
    # nothing to cut: the caller gets its own record back
    if trim_at == len(seq):
        return record, False
    if hasattr(record, "quality"):
        return Read(name=record.name, sequence=seq[:trim_at], quality=record.quality[:trim_at]), True
    return Read(name=record.name, sequence=seq[:trim_at]), True


def trim_records(countgraph, records, cutoff, variable_coverage=False, normalize_to=None):
    """trim_record over a list of records, one batch call; a list of
    (record or None, did_trim).  With variable_coverage only reads whose
    median k-mer count is at least normalize_to are trimmed (a failed gate is
    reported by the device as trim_at = len(sequence), i.e. unmodified)."""
    records = list(records)
    if not records:
        return []
    if variable_coverage and normalize_to is None:
        raise TypeError("variable_coverage needs normalize_to")
    seqs = [r.cleaned_seq for r in records]
    at = countgraph.trim_on_abundance_batch(seqs, cutoff, normalize_to=normalize_to if variable_coverage else None)
    for r, a in zip(records, at):
        if a is None:   # trim_on_abundance's error for this read
            raise ValueError("sequence length ({}) must >= the hashtable k-mer size ({})".format(
                len(r.sequence), countgraph.ksize()))
    return [_apply(countgraph, r, a) for r, a in zip(records, at)]


def trim_record(countgraph, record, cutoff, variable_coverage=False, normalize_to=None):
    return trim_records(countgraph, [record], cutoff, variable_coverage, normalize_to)[0]
