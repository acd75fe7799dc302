// bmx_index_match_kernel.h -- kernels of the text index's matching statistics and seeds (bmx_index_match_device,
// bmx_index_seeds_device, include/bmx.h), over the query descriptor, comparator, loads, directory and bisection of
// bmx_index_kernel.h.
//
// index_match_kernel: one lane per blob byte b.  The lane finds its query q (index_query_of: b over pat_off), checks
// that q holds b, is at most INDEX_MAX_PATTERN bytes long and that every byte of the query's rest pat[b .. off[q+1]) is
// below 0x80, and then answers for that rest, which it treats as a query of its own that ends where query q ends:
//   1. the rest's insertion point x in the array, by the count kernel's first search (index_bound, inside the bucket
//      index_bucket gives for the rest's first two bytes, common-prefix lengths of both bounds carried along).  When
//      the search ends, the two lengths it carries are the common prefixes of the rest with sa[x - 1] and sa[x]; the
//      longer one is the longest match `len` (tests/match_oracle.py holds that to brute force; the virtual symbol
//      equals no query byte).
//   2. the interval of the prefix rest[0 .. len): it holds x - 1 or x.  The neighbour whose common prefix is shorter
//      than len is outside, so that bound is x with no further read; on the other side the lane gallops away from x
//      (1, 2, 4, .. entries) and bisects the last step, comparing against the prefix only.  An interval of c entries
//      costs about 2 log2 c probes, an occurrence that stands alone costs one.
// An empty two-byte bucket does not mean "no answer" here: the match is then 0 or 1 bytes long and the lane searches
// the rest's first byte plainly over the whole array.  Lane t < count also checks the offsets of query t, because a
// query without a byte has no lane of its own.
//
// Memory safety is the count kernel's: bytes only through index_load8, array entries only through index_entry, a lane
// that finds bad offsets or a byte >= 0x80 raises a status word and reads neither text nor array.
//
// Seeds (seed_flag, index_seed_fill_kernel, index_seed_off_kernel): the match kernel writes len, lo, cnt and the
// position inside the query for every blob byte into workspace; a position is a seed iff len >= min_len, it is the
// query's first or its predecessor's len is not larger, and cnt <= max_occ; rocPRIM's exclusive scan of that flag
// (computed on the fly) gives every seed its slot, the fill writes the seeds below `capacity`, and the scan's values
// at the query offsets are the offsets of the seeds per query.  No atomics: the list is the same in every run.
#pragma once
#include "bmx_index_kernel.h"

namespace bmx {

constexpr uint32_t INDEX_NO_QUERY = 0xffffffffu; // workspace qpos of a blob byte that no lane answered for

struct IndexMatchArgs {
    IndexQuery q;
    uint32_t *len;      // per blob byte
    uint32_t *lo, *cnt; // per blob byte; may be nullptr
    uint32_t *qpos;     // per blob byte: its position inside its query (seeds), or nullptr
};

__global__ __launch_bounds__(INDEX_BLOCK) void index_match_kernel(IndexMatchArgs a)
{
    const IndexQuery &q = a.q;
    const uint64_t t = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (t < q.count) {
        const uint64_t q0 = q.pat_off[t], q1 = q.pat_off[t + 1];
        if (q1 < q0 || q1 > q.pat_bytes || q1 == q0 || q1 - q0 > INDEX_MAX_PATTERN) q.status[0] = 1;
    }
    if (t >= q.pat_bytes || t < q.pat_off[0] || t >= q.pat_off[q.count]) return; // outside every query: left untouched

    const uint64_t qi = index_query_of(q.pat_off, q.count, t);
    const uint64_t o0 = q.pat_off[qi], o1 = q.pat_off[qi + 1];
    if (o0 > t || o1 <= t || o1 > q.pat_bytes || o1 - o0 > INDEX_MAX_PATTERN) { // (offsets that are not sorted end here)
        q.status[0] = 1;
        return;
    }
    uint32_t m = (uint32_t)(o1 - t); // the rest of the query: the match never runs into the next one
    if (!index_bytes_ok(q.pat, t, m, q.pat_bytes)) {
        q.status[1] = 1;
        return;
    }

    uint32_t lo0 = 0, hi0 = q.n, known = 0; // the interval that is searched; bytes every suffix in it shares with the rest
    if (index_bucket(q, t, m, lo0, hi0)) {
        // an empty bucket, the first two bytes occur nowhere: the match is 0 or 1 bytes long, and the first byte's plain
        // search over the whole array says which
        if (hi0 > lo0) known = 2;
        else lo0 = 0, hi0 = q.n, m = 1;
    }
    uint32_t x = lo0, lx = known, ly = known; // first suffix that is not below the rest
    index_bound<false>(q, t, m, x, hi0, lx, ly);
    // lx, ly: the bytes sa[x - 1] and sa[x] share with the rest (a bound that never moved has its neighbour outside
    // the bucket, or none, and keeps `known`, which the other one reaches at least)
    const uint32_t len = lx > ly ? lx : ly;
    uint32_t first = 0, end = 0;
    if (len > 0 && len == known) {
        first = lo0, end = hi0; // the two known bytes and no more: the bucket itself
    } else if (len > 0) {
        first = end = x;
        if (x > lo0 && lx == len) { // sa[x - 1] begins with the prefix: the first suffix that is not below it
            uint32_t f = lo0, b = x - 1u, lf = known, lb = len, step = 1; // the answer is in [f, b]; sa[b] is inside
            while (b - f >= step) {
                const uint32_t j = b - step;
                uint32_t l = lf < lb ? lf : lb;
                const int c = index_compare(q.text, q.n, index_entry(q.sa, j, q.n), q.pat, q.pat_bytes, t, len, l);
                if (c < 0) {
                    f = j + 1u, lf = l;
                    break;
                }
                b = j, lb = l, step <<= 1;
            }
            while (f < b) {
                const uint32_t mid = f + ((b - f) >> 1);
                uint32_t l = lf < lb ? lf : lb;
                const int c = index_compare(q.text, q.n, index_entry(q.sa, mid, q.n), q.pat, q.pat_bytes, t, len, l);
                if (c < 0) f = mid + 1u, lf = l;
                else b = mid, lb = l;
            }
            first = b;
        }
        if (x < hi0 && ly == len) { // sa[x] begins with the prefix: the first suffix above it
            uint32_t f = x, b = hi0, lf = len, lb = known, step = 1; // sa[f] is inside; the answer is in (f, b]
            while (b - f > step) {
                const uint32_t j = f + step;
                uint32_t l = lf < lb ? lf : lb;
                const int c = index_compare(q.text, q.n, index_entry(q.sa, j, q.n), q.pat, q.pat_bytes, t, len, l);
                if (c > 0) {
                    b = j, lb = l;
                    break;
                }
                f = j, lf = l, step <<= 1;
            }
            while (b - f > 1u) {
                const uint32_t mid = f + ((b - f) >> 1);
                uint32_t l = lf < lb ? lf : lb;
                const int c = index_compare(q.text, q.n, index_entry(q.sa, mid, q.n), q.pat, q.pat_bytes, t, len, l);
                if (c > 0) b = mid, lb = l;
                else f = mid, lf = l;
            }
            end = b;
        }
    }
    a.len[t] = len;
    if (a.lo) a.lo[t] = first;
    if (a.cnt) a.cnt[t] = end - first;
    if (a.qpos) a.qpos[t] = (uint32_t)(t - o0);
}

// 1 if blob byte b is a seed.  qpos arrives as INDEX_NO_QUERY everywhere and is written by the lanes that answered; a
// position behind a query's first has its predecessor in the same query.  b == bytes (the scan's last entry) is none.
struct IndexSeedFlag {
    const uint32_t *qpos, *len, *cnt;
    uint64_t bytes;
    uint32_t min_len, max_occ;
    __host__ __device__ uint32_t operator()(uint64_t b) const
    {
        if (b >= bytes) return 0u;
        const uint32_t i = qpos[b];
        if (i == INDEX_NO_QUERY) return 0u;
        const uint32_t l = len[b];
        if (l < min_len) return 0u;
        if (i != 0u && len[b - 1] > l) return 0u;
        if (max_occ != 0u && cnt[b] > max_occ) return 0u;
        return 1u;
    }
};

// slot[b]: the exclusive scan of the flags (bytes + 1 entries).  The seeds whose slots are below `capacity` are stored.
__global__ __launch_bounds__(INDEX_BLOCK) void index_seed_fill_kernel(IndexSeedFlag f, const uint32_t *slot, const uint32_t *lo,
                                                                      uint64_t capacity, uint32_t *out_qpos, uint32_t *out_len,
                                                                      uint32_t *out_lo, uint32_t *out_cnt)
{
    const uint64_t b = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (!f(b)) return;
    const uint32_t s = slot[b];
    if (s >= capacity) return;
    out_qpos[s] = f.qpos[b];
    out_len[s] = f.len[b];
    out_lo[s] = lo[b];
    out_cnt[s] = f.cnt[b];
}

// seed_off[q] = the seeds in front of query q (count + 1 entries), res[0] = the total.  (An offset past the blob, which
// the match kernel has reported, is kept inside the scan.)
__global__ __launch_bounds__(INDEX_BLOCK) void index_seed_off_kernel(const uint64_t *pat_off, uint64_t count, uint64_t bytes,
                                                                     const uint32_t *slot, uint64_t *seed_off, uint64_t *res)
{
    const uint64_t q = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (q > count) return;
    const uint64_t o = pat_off[q];
    const uint64_t s = slot[o < bytes ? o : bytes];
    seed_off[q] = s;
    if (q == count) res[0] = s;
}

} // namespace bmx
