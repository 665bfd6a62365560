"""Table groups of the near-prime level 2 (k_scatter_n2, khmer_amd/csrc/
kh_nearprime.cuh) against the oracle: every table byte, n_unique_kmers,
n_occupied and the bigcount map, exactly.

A level-2 workgroup expands each level-1 record into the region records of
one group of tables only (two of four by default), so that two workgroups fit
a CU's LDS; KH_N2_TG=0 keeps one group of all the tables.  Every case runs
both kernels from the one library and both must equal the oracle (reference
semantics: Hashtable::consume_string -> ByteStorage::add, src/oxli/
hashtable.cc:280-294, include/oxli/storage.hh:571-624).

The geometry is the smallest that takes this path (tests/
test_gpu_nearprime.py): k = 19 into ~1e8-bin tables, 150 bp reads, device
passes of 9,000,000 k-mers.  With 300,000 uniform reads the last level-1
bucket holds r near P, so its bins wrap past p_i into regions 0 .. E (the
rho >= rt[i] branch of every group).  KH_NP_L1MAX=8 sends the same tables
through the three-level partition, whose level 2 is the same kernel over fine
buckets.  The skewed stream (reads of a 5000-base genome) overflows the fixed
capacities: destinations go dead in one group while the other group's live
on, and the pass comes out exact through the retry or the fallback."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x6e32   # a stream of its own (synth.batch / genomic_batch take the same seed)
K, X, L, BATCH = 19, 1e8, 150, 9000000

# name -> (reads, genome bases, tables)
STREAMS = {"uniform4": (300000, 0, 4), "uniform3": (300000, 0, 3), "uniform2": (300000, 0, 2),
           "skewed4": (200000, 5000, 4)}
# (stream, KH_NP_L1MAX or None)
CASES = [("uniform4", None), ("uniform3", None), ("uniform2", None), ("uniform4", 8), ("skewed4", None)]


def _bigcounts(g):
    from khmer_amd._lib import lib, check
    n = ctypes.c_uint64()
    check(lib.kh_graph_get_bigcounts(g._g, None, None, 0, ctypes.byref(n)))
    keys = (ctypes.c_uint64 * max(n.value, 1))()
    vals = (ctypes.c_uint16 * max(n.value, 1))()
    check(lib.kh_graph_get_bigcounts(g._g, keys, vals, n.value, ctypes.byref(n)))
    return dict(zip(keys[:n.value], vals[:n.value]))


def _kernels(g):
    from khmer_amd._lib import lib, check
    buf = ctypes.create_string_buffer(1 << 16)
    n = ctypes.c_size_t()
    check(lib.kh_graph_kernel_stats(g._g, buf, len(buf), ctypes.byref(n)))
    return {ln.split("\t")[0] for ln in buf.value.decode().splitlines() if ln}


def _make_stream(n, genome, tables):
    """The reads in device memory and what the oracle makes of them (once per stream)."""
    from khmer_amd._lib import lib, check, default_device
    from khmer_amd import synth
    from oracle import oracle as O
    import khmer_amd
    dev = default_device()
    words, koff = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.kh_device_malloc(dev, (n * L // 32 + 2) * 8, ctypes.byref(words)))
    check(lib.kh_device_malloc(dev, (n + 1) * 8, ctypes.byref(koff)))
    if genome:
        check(lib.kh_synth_genomic_device(dev, SEED, genome, 0, n, L, K, words, koff))
        seqs = synth.genomic_batch(0, n, L, genome, seed=SEED)[0]
    else:
        check(lib.kh_synth_packed_device(dev, SEED, 0, n, L, K, words, koff))
        seqs = synth.batch(0, n, L, seed=SEED)[0]
    sizes = khmer_amd.Countgraph(K, X, tables).hashsizes()
    o = O.Table(O.BYTE, K, sizes)
    o.set_use_bigcount(True)
    o.consume_batch(seqs, [i * L for i in range(n + 1)])
    want = {"tables": [o.table_bytes(i) for i in range(tables)], "n_unique": o.n_unique_kmers(),
            "n_occupied": o.n_occupied(), "bigcounts": o.bigcounts()}
    return dict(words=words, koff=koff, dev=dev, n=n, tables=tables, want=want)


@pytest.fixture(scope="module")
def streams():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _make_stream(*STREAMS[name])
        return cache[name]

    yield get
    from khmer_amd._lib import lib
    for s in cache.values():
        lib.kh_device_free(s["dev"], s["words"])
        lib.kh_device_free(s["dev"], s["koff"])


@pytest.mark.parametrize("groups", ["default", "one_group"])
@pytest.mark.parametrize("name,l1max", CASES,
                         ids=["%s%s" % (n, "_three_level" if m else "") for n, m in CASES])
def test_n2_groups_match_oracle(streams, name, l1max, groups, monkeypatch):
    import khmer_amd
    from khmer_amd._lib import lib, check
    s = streams(name)
    if groups == "one_group":
        monkeypatch.setenv("KH_N2_TG", "0")
    else:
        monkeypatch.delenv("KH_N2_TG", raising=False)
    if l1max:
        monkeypatch.setenv("KH_NP_L1MAX", str(l1max))
    g = khmer_amd.Countgraph(K, X, s["tables"])
    g.set_use_bigcount(True)
    check(lib.kh_graph_set_batch_kmers(g._g, BATCH))   # several device passes
    check(lib.kh_graph_set_profiling(g._g, 1))
    check(lib.kh_consume_packed_fixed_device(g._g, s["words"], s["n"], L))
    kernels = _kernels(g)
    assert "scatter_n2" in kernels, kernels
    assert ("scatter_n1b" in kernels) == bool(l1max), kernels
    want = s["want"]
    tabs = g.get_raw_tables()
    for i in range(s["tables"]):
        got = bytes(tabs[i])
        if got != want["tables"][i]:   # report without pytest's byte-wise diff of 1e8-byte strings
            bad = next(j for j in range(len(got)) if got[j] != want["tables"][i][j])
            pytest.fail("table %d differs first at bin %d (%d vs oracle %d)" % (i, bad, got[bad], want["tables"][i][bad]))
    assert g.n_unique_kmers() == want["n_unique"]
    assert g.n_occupied() == want["n_occupied"]
    assert _bigcounts(g) == want["bigcounts"]
