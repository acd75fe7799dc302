// bmx_index_kernel.h -- kernels of the text index (bmx_index_*, include/bmx.h): batched pattern count and locate over a
// device-resident text and its suffix array.
//
// The order that is searched.  bmx_suffix_array keeps the reference's "past the end ranks as character 96" rule
// (sa_init_keys in bmx_sa.hip), so the array is NOT the plain lexicographic order outside lower-case text.  For every
// text that does not end in two or more bytes 96 it is the sorted order of these strings, one per suffix i:
//     text[i..n) compared as signed char,
//     then, if n - 1 - i is even, ONE virtual symbol strictly between byte 95 and byte 96 (equal to no pattern byte),
//     then "nothing", which is below everything.
// index_compare is that comparator against a pattern: a suffix that runs out before the pattern is never a match, it is
// LESS than the pattern unless it carries the virtual symbol and the pattern's next byte is below 96.  The suffixes
// that have the pattern as a prefix are then one interval [lo, lo + cnt) of the array: the true occurrences.
//
// index_count_kernel: one query per lane, two binary searches (index_bound: first suffix not below the pattern, first
// suffix above it) with the common-prefix lengths of both bounds carried along, so that a probe starts comparing at the
// smaller of the two (Manber and Myers); bytes are compared eight at a time as big-endian words with the sign bits
// flipped.  A query of two or more bytes starts inside the directory's bucket of its first two bytes (index_bucket).
// The match and map kernels (bmx_index_match_kernel.h, bmx_index_map_kernel.h) search with the same pieces: the query
// descriptor IndexQuery, index_bytes_ok, index_bucket, index_bound and index_query_of live here, once.  The path is a chain of
// dependent random reads (array entry, then text words): it is bound by latency and by the number of lanes in flight.
//
// Memory safety: a text or pattern byte is fetched as part of the aligned 8-byte word that holds it; no word is read
// that does not hold at least one byte of text[0..n) or of the pattern blob.  A lane whose offsets or bytes are
// invalid raises a status word and reads nothing of the text or the array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmx {

constexpr uint32_t INDEX_BLOCK = 256;       // lanes = queries per workgroup
constexpr uint32_t INDEX_MAX_PATTERN = 512; // == BMX_MAX_PATTERN
constexpr uint32_t INDEX_DIR_SIDE = 128;    // pattern bytes are < 0x80
constexpr uint32_t INDEX_DIR_ENTRIES = INDEX_DIR_SIDE * INDEX_DIR_SIDE;
// Fill: a segment of at most this many positions is copied by its own lane (64 such copies run side by side in a
// wave), a longer one by the whole wave, 64 consecutive entries per step.  Half a wave: below it the wave-wide copy
// would leave more than half of its lanes idle in its only step.
constexpr uint32_t INDEX_FILL_SHORT = 32;

// What every kernel of the index reads: the text and its array, the query blob and its offsets, the directory and the
// status words.  IndexArgs, IndexMatchArgs and IndexMapArgs begin with one and put their outputs behind it.
struct IndexQuery {
    const uint8_t *text;
    uint32_t n;
    const int32_t *sa;
    const uint8_t *pat;
    uint64_t pat_bytes;
    const uint64_t *pat_off;
    uint64_t count;
    const uint32_t *dir_lo, *dir_cnt; // the directory (INDEX_DIR_ENTRIES each), or nullptr: every search is plain
    uint64_t *status; // [0]: offsets or lengths out of range, [1]: a pattern byte >= 0x80
};

struct IndexArgs {
    IndexQuery q;
    uint32_t *lo; // may be nullptr
    uint32_t *cnt;
};

// base[at .. at + 8) as one big-endian word with every byte's sign bit flipped: unsigned order of two such words is
// the signed-char order of the byte strings.  at < len; bytes at and behind `len` come out as anything (the caller
// counts only valid ones).
__device__ __forceinline__ uint64_t index_load8(const uint8_t *base, uint64_t at, uint64_t len)
{
    const uintptr_t addr = (uintptr_t)base + at;
    const uintptr_t a = addr & ~(uintptr_t)7;
    const uintptr_t last = ((uintptr_t)base + len - 1) & ~(uintptr_t)7; // the word that holds the last byte
    const uint32_t sh = (uint32_t)(addr & 7u) * 8u;
    uint64_t w = *reinterpret_cast<const uint64_t *>(a);
    if (sh) {
        const uint64_t w1 = a < last ? *reinterpret_cast<const uint64_t *>(a + 8) : 0ull;
        w = (w >> sh) | (w1 << (64u - sh));
    }
    return __builtin_bswap64(w) ^ 0x8080808080808080ull;
}

// Pattern pat[poff .. poff + m) against the suffix that starts at p, in the order described above: -1 the suffix is
// below the pattern, 0 the pattern is a prefix of it, +1 it is above.  lcp: in, a number of leading bytes known to be
// equal; out, the number of leading bytes that are.
__device__ __forceinline__ int index_compare(const uint8_t *text, uint32_t n, uint32_t p, const uint8_t *pat,
                                             uint64_t pat_bytes, uint64_t poff, uint32_t m, uint32_t &lcp)
{
    const uint32_t len = n - p;
    const uint32_t lim = m < len ? m : len;
    uint32_t k = lcp < lim ? lcp : lim;
    while (k < lim) {
        const uint64_t tw = index_load8(text, (uint64_t)p + k, n);
        const uint64_t pw = index_load8(pat, poff + k, pat_bytes);
        const uint64_t x = tw ^ pw;
        const uint32_t valid = lim - k < 8u ? lim - k : 8u;
        const uint32_t same = x ? (uint32_t)__builtin_clzll(x) >> 3 : 8u;
        if (same < valid) {
            lcp = k + same;
            return tw < pw ? -1 : 1;
        }
        k += valid;
    }
    lcp = lim;
    if (lim == m) return 0;
    // the suffix ran out first: the virtual symbol (between 95 and 96) if n - 1 - p is even, "nothing" otherwise
    if (((len - 1u) & 1u) == 0u && pat[poff + len] < 96u) return 1;
    return -1;
}

// sa[j], kept inside the text whatever a caller's array holds (an array of another text gives wrong answers, not faults)
__device__ __forceinline__ uint32_t index_entry(const int32_t *sa, uint32_t j, uint32_t n)
{
    const uint32_t p = (uint32_t)sa[j];
    return p < n ? p : n - 1u;
}

// No byte of pat[at .. at + m) is 0x80 or above (flipped sign bits: such a byte shows as a clear top bit).
__device__ __forceinline__ bool index_bytes_ok(const uint8_t *pat, uint64_t at, uint32_t m, uint64_t pat_bytes)
{
    for (uint32_t k = 0; k < m; k += 8) {
        const uint32_t valid = m - k < 8u ? m - k : 8u;
        const uint64_t w = index_load8(pat, at + k, pat_bytes);
        if (~w & 0x8080808080808080ull & (~0ull << (8u * (8u - valid)))) return false;
    }
    return true;
}

// The directory's bucket [lo, hi) of the two bytes at pat[at]: every suffix in it shares them with the pattern.  false,
// and lo and hi as they were: there is no directory, or the pattern has one byte.  What an empty bucket means is the
// caller's to say.
__device__ __forceinline__ bool index_bucket(const IndexQuery &q, uint64_t at, uint32_t m, uint32_t &lo, uint32_t &hi)
{
    if (!q.dir_lo || m < 2) return false;
    const uint32_t b = (uint32_t)q.pat[at] * INDEX_DIR_SIDE + q.pat[at + 1];
    lo = q.dir_lo[b];
    hi = lo + q.dir_cnt[b];
    return true;
}

// Bisection of [x, y) for pat[at .. at + m): x becomes the first suffix that is not below the pattern, or with UPPER the
// first one above it.  lx, ly: in, bytes that the suffixes in front of x and from y on are known to share with the
// pattern; out, the bytes that sa[x - 1] and sa[x] share with it (a bound that never moved keeps what came in).  A probe
// starts comparing at the smaller of the two.
template <bool UPPER>
__device__ __forceinline__ void index_bound(const IndexQuery &q, uint64_t at, uint32_t m, uint32_t &x, uint32_t y, uint32_t &lx,
                                            uint32_t &ly)
{
    while (x < y) {
        const uint32_t mid = x + ((y - x) >> 1);
        uint32_t l = lx < ly ? lx : ly;
        const int c = index_compare(q.text, q.n, index_entry(q.sa, mid, q.n), q.pat, q.pat_bytes, at, m, l);
        if (UPPER ? c <= 0 : c < 0) x = mid + 1, lx = l;
        else y = mid, ly = l;
    }
}

// The last query that starts at or before blob byte b (count >= 1; offsets that are not sorted give some query, which
// the caller checks).
__device__ __forceinline__ uint64_t index_query_of(const uint64_t *pat_off, uint64_t count, uint64_t b)
{
    uint64_t q = 0, qe = count;
    while (qe - q > 1) {
        const uint64_t mid = q + ((qe - q) >> 1);
        if (pat_off[mid] <= b) q = mid;
        else qe = mid;
    }
    return q;
}

__global__ __launch_bounds__(INDEX_BLOCK) void index_count_kernel(IndexArgs a)
{
    const IndexQuery &q = a.q;
    const uint64_t i = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (i >= q.count) return;
    const uint64_t o0 = q.pat_off[i], o1 = q.pat_off[i + 1];
    if (o1 < o0 || o1 > q.pat_bytes || o1 == o0 || o1 - o0 > INDEX_MAX_PATTERN) {
        q.status[0] = 1;
        return;
    }
    const uint32_t m = (uint32_t)(o1 - o0);
    if (!index_bytes_ok(q.pat, o0, m, q.pat_bytes)) {
        q.status[1] = 1;
        return;
    }

    uint32_t lo = 0, hi = q.n; // the interval that is searched; `known` bytes every suffix in it shares with the pattern
    const uint32_t known = index_bucket(q, o0, m, lo, hi) ? 2u : 0u;
    uint32_t first = lo, end = hi;
    if (!(known == 2 && (m == 2 || lo == hi))) { // (an empty bucket's start is the pattern's insertion point as well)
        uint32_t x = lo, lx = known, ly = known;
        index_bound<false>(q, o0, m, x, hi, lx, ly);
        first = x;
        lx = known, ly = known;
        index_bound<true>(q, o0, m, x, hi, lx, ly);
        end = x;
    }
    if (a.lo) a.lo[i] = first;
    a.cnt[i] = end - first;
}

// Behind the exclusive scan of the counts (off: count + 1 entries): res[0] = the total, res[1] = the number of leading
// queries whose segments end at or below `capacity` (offsets do not decrease, so these are a prefix of the queries),
// res[2] = the positions they hold; seg[i] = off[i] in 32 bits for the segmented sort.  res[1], res[2] arrive zeroed.
__global__ __launch_bounds__(INDEX_BLOCK) void index_prefix_kernel(const uint64_t *off, uint64_t count, uint64_t capacity,
                                                                   uint32_t *seg, uint64_t *res)
{
    const uint64_t i = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (i > count) return;
    const uint64_t o = off[i];
    seg[i] = o > 0xffffffffull ? 0xffffffffu : (uint32_t)o;
    if (i == count) res[0] = o;
    if (i > 0 && o <= capacity && (i == count || off[i + 1] > capacity)) res[1] = i, res[2] = o; // one lane at most
}

// keys[off[i] .. off[i + 1)) = sa[lo[i] .. lo[i] + cnt[i]) for the first `stored_queries` queries.
__global__ __launch_bounds__(INDEX_BLOCK) void index_fill_kernel(const int32_t *sa, const uint32_t *lo, const uint32_t *cnt,
                                                                 const uint64_t *off, uint64_t stored_queries, uint32_t *keys)
{
    const uint64_t i = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    const bool own = i < stored_queries;
    const uint32_t c = own ? cnt[i] : 0u;
    const uint32_t l = own ? lo[i] : 0u;
    const uint32_t o = own ? (uint32_t)off[i] : 0u; // (the stored positions are fewer than 2^31: the host checks)
    if (c <= INDEX_FILL_SHORT)
        for (uint32_t j = 0; j < c; ++j) keys[o + j] = (uint32_t)sa[l + j];
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t todo = __ballot(c > INDEX_FILL_SHORT);
    while (todo) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t cc = __shfl(c, src), ll = __shfl(l, src), oo = __shfl(o, src);
        for (uint32_t j = lane; j < cc; j += 64u) keys[oo + j] = (uint32_t)sa[ll + j];
    }
}

__global__ __launch_bounds__(INDEX_BLOCK) void index_widen_kernel(const uint32_t *keys, uint64_t stored, uint64_t base_offset,
                                                                  uint64_t *pos)
{
    const uint64_t j = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (j < stored) pos[j] = base_offset + keys[j];
}

} // namespace bmx
