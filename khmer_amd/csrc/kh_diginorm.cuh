// kh_diginorm.cuh -- device kernels of digital normalization
// (scripts/normalize-by-median.py:155-179 over Hashtable::median_at_least,
// src/oxli/hashtable.cc:333-364).  Included by kh_engine.hip.
//
// A window of units (a read, or a pair) is decided against the table state T
// at the window's start.  Units that pass median_at_least under T are rejected
// for good (counts never decrease).  Every k-mer of the remaining candidate
// units becomes one record per table, keyed (table, bin, candidate index) and
// radix-sorted; a record's provisional count is T[bin] plus the number of
// records of *kept* candidates with a smaller index in its bin, which an
// exclusive scan of keep[unit(record)] over the sorted records gives as
// S[start of (bin, unit) run] - S[start of bin run].  keep is iterated to its
// fixed point (engine_diginorm); the system is triangular, so the prefix on
// which two successive iterates agree is the sequential answer.
//
// All indices inside a window are 32-bit: the host caps a window at 2^24
// records and 2^18 units.
#pragma once
#include "kh_query.cuh"

namespace kh {

// one read of a window: its k-mers are [k0, k0 + n) of the window's hashes
// (dst: [q0, q0 + n) of the compacted k-mers it is gathered into); unit = the
// index of its candidate unit
struct DnRead {
    uint32_t k0, n, q0, unit;
};

// the largest count a bin of this storage holds
__device__ __forceinline__ uint32_t dn_max_count(int kind) { return kind == BIT ? 1u : (kind == NIBBLE ? 15u : 255u); }

// in-table count of bin `bin` of table t (no bigcount: cutoffs here are <= the
// storage maximum, where the table bytes alone decide count >= cutoff)
__device__ __forceinline__ uint32_t dn_bin_count(const Params &P, const uint8_t *tab, int t, uint64_t bin) {
    if (P.kind == BIT) return (tab[P.tbyte[t] + (bin >> 3)] >> (bin & 7)) & 1;
    if (P.kind == NIBBLE) {
        const uint8_t byte = tab[P.tbyte[t] + (bin >> 1)];
        return (bin & 1) ? (byte & 0x0F) : (byte >> 4);
    }
    return tab[P.tbyte[t] + bin];
}

// Hashtable::median_at_least's threshold, as k_at_least computes it
__device__ __forceinline__ uint32_t dn_min_req(uint32_t n) { return (uint32_t)(0.5 + (double)((float)n / 2.0f)); }

// cheap reject, per k-mer: ge[j] = 1 when the k-mer's count under T is >= cutoff
__global__ void __launch_bounds__(256) k_dn_ge(Params P, const uint8_t *tab, const uint64_t *hashes, uint32_t nk,
                                               uint32_t cutoff, uint8_t *ge) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nk; j += gridDim.x * blockDim.x) {
        const uint64_t h = hashes[j];
        bool ok = true;
        for (int t = 0; t < P.n; t++) ok = ok && dn_bin_count(P, tab, t, mod_barrett(h, P.p[t], P.m[t])) >= cutoff;
        ge[j] = ok ? 1 : 0;
    }
}

// cheap reject, per unit (one wave each): cand[u] = 1 when some read of the
// unit fails median_at_least under T.  Unit u holds reads [uoff[u], uoff[u+1])
// of the batch; read r's k-mers are [koff[r], koff[r+1]) - kbase of the window.
__global__ void __launch_bounds__(256) k_dn_reject(const uint32_t *uoff, uint32_t nunits, const uint64_t *koff,
                                                   uint64_t kbase, const uint8_t *ge, uint8_t *cand) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t u = wave; u < nunits; u += nwaves) {
        bool fail = false;
        for (uint32_t r = uoff[u]; r < uoff[u + 1]; r++) {
            const uint32_t a = (uint32_t)(koff[r] - kbase), n = (uint32_t)(koff[r + 1] - koff[r]);
            uint32_t num = 0;
            for (uint32_t i0 = 0; i0 < n; i0 += 64) {
                const uint32_t i = i0 + lane;
                num += __popcll(__ballot(i < n && ge[a + i] != 0));
            }
            fail = fail || num < dn_min_req(n);
        }
        if (lane == 0) cand[u] = fail ? 1 : 0;
    }
}

// records of the candidate reads (one wave per read): record q*nt + t of
// compacted k-mer q and table t has the key (t, bin, candidate index)
__global__ void __launch_bounds__(256) k_dn_records(Params P, const uint64_t *hashes, const DnRead *reads,
                                                    uint32_t nreads, int ubits, int bbits, uint64_t *keys,
                                                    uint32_t *vals) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t r = wave; r < nreads; r += nwaves) {
        const DnRead rd = reads[r];
        for (uint32_t i = lane; i < rd.n; i += 64) {
            const uint64_t h = hashes[rd.k0 + i];
            const uint32_t rec = (rd.q0 + i) * (uint32_t)P.n;
            for (int t = 0; t < P.n; t++) {
                const uint64_t bin = mod_barrett(h, P.p[t], P.m[t]);
                keys[rec + t] = ((((uint64_t)t << bbits) | bin) << ubits) | rd.unit;
                vals[rec + t] = rec + t;
            }
        }
    }
}

// componentwise maximum of two packed (bin-run start, (bin, unit)-run start)
// pairs: the inclusive scan of the head positions gives every record its runs
struct DnMax2 {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
        const uint64_t ah = a >> 32, bh = b >> 32, al = a & 0xffffffffu, bl = b & 0xffffffffu;
        return ((ah > bh ? ah : bh) << 32) | (al > bl ? al : bl);
    }
};

// after the sort: where each record went (inv), the table count of its bin
// under T, and its head positions (i at the first record of a run, else 0)
__global__ void __launch_bounds__(256) k_dn_heads(Params P, const uint8_t *tab, const uint64_t *keys,
                                                  const uint32_t *vals, uint32_t nrec, int ubits, int bbits,
                                                  uint32_t *inv, uint8_t *base, uint64_t *heads) {
    const uint64_t bmask = (1ull << bbits) - 1;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nrec; i += gridDim.x * blockDim.x) {
        const uint64_t key = keys[i], prev = i ? keys[i - 1] : 0;
        inv[vals[i]] = i;
        const uint64_t tb = key >> ubits;
        base[i] = (uint8_t)dn_bin_count(P, tab, (int)(tb >> bbits), tb & bmask);
        const uint64_t hb = (i && tb != (prev >> ubits)) ? i : 0, hu = (i && key != prev) ? i : 0;
        heads[i] = (hb << 32) | hu;
    }
}

// keep flag of every sorted record's unit, the input of the scan
__global__ void __launch_bounds__(256) k_dn_kv(const uint64_t *keys, uint32_t nrec, uint32_t umask,
                                               const uint8_t *keep, uint32_t *kv) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nrec; i += gridDim.x * blockDim.x)
        kv[i] = keep[(uint32_t)keys[i] & umask];
}

// one fixed-point iteration, one wave per candidate unit: a k-mer counts when
// min(MAX, T[bin] + prefix) >= cutoff in every table, a read passes when
// num >= min_req, a unit is kept when any of its reads fails.  mismatch
// receives the first unit whose new flag differs from the old one.
__global__ void __launch_bounds__(256) k_dn_iter(int kind, int nt, const uint32_t *roff, const DnRead *reads,
                                                 uint32_t nunits, const uint32_t *inv, const uint8_t *base,
                                                 const uint64_t *runs, const uint32_t *S, uint32_t cutoff,
                                                 const uint8_t *keep, uint8_t *keep_new, uint32_t *mismatch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t mx = dn_max_count(kind);
    for (uint32_t u = wave; u < nunits; u += nwaves) {
        bool fail = false;
        for (uint32_t r = roff[u]; r < roff[u + 1]; r++) {
            const DnRead rd = reads[r];
            uint32_t num = 0;
            for (uint32_t i0 = 0; i0 < rd.n; i0 += 64) {
                const uint32_t i = i0 + lane;
                bool ok = i < rd.n;
                if (ok) {
                    const uint32_t rec = (rd.q0 + i) * (uint32_t)nt;
                    for (int t = 0; t < nt; t++) {
                        const uint32_t pos = inv[rec + t];
                        const uint64_t run = runs[pos];
                        const uint32_t prefix = S[(uint32_t)run] - S[(uint32_t)(run >> 32)];
                        const uint32_t c = min(mx, (uint32_t)base[pos] + prefix);
                        ok = ok && c >= cutoff;
                    }
                }
                num += __popcll(__ballot(ok));
            }
            fail = fail || num < dn_min_req(rd.n);
        }
        if (lane == 0) {
            const uint8_t kn = fail ? 1 : 0;
            keep_new[u] = kn;
            if (kn != keep[u]) atomicMin(mismatch, u);
        }
    }
}

// hashes of the kept reads, gathered in stream order for the consume pass
__global__ void __launch_bounds__(256) k_dn_gather(const uint64_t *hashes, const DnRead *reads, uint32_t nreads,
                                                   uint64_t *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t r = wave; r < nreads; r += nwaves) {
        const DnRead rd = reads[r];
        for (uint32_t i = lane; i < rd.n; i += 64) out[rd.q0 + i] = hashes[rd.k0 + i];
    }
}

}  // namespace kh
