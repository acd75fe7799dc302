// bmx_index_map_kernel.h -- kernels of the text index's read mapping (bmx_index_map_device, include/bmx.h):
// every occurrence of every seed of a read becomes a candidate, and every candidate is verified by an approximate
// search of the whole read inside the window of the text that its diagonal allows.
//
// Candidates.  The match kernel (bmx_index_match_kernel.h) leaves qpos, len, lo, cnt per blob byte in workspace.
// IndexMapCount gives blob byte b the value cnt[b] if b is a seed (IndexSeedFlag) and 0 otherwise; rocPRIM's exclusive
// scan of it (64-bit, bytes + 1 entries) is `scan`: the candidates in front of blob byte b.  So the candidates of query q
// are [scan[off[q]], scan[off[q+1]]) and the total is scan[bytes].  index_map_fill_kernel: one lane per candidate c; the
// lane finds its blob byte by a binary search of c over scan (the last b with scan[b] <= c has a non-zero count), its
// query by index_query_of over the offsets, and writes (q, i, p = sa[lo[b] + c - scan[b]]).  No atomics: the
// list is in order of (query, seed, t) in every run.
//
// Verification (index_map_verify_kernel<W>): one candidate per lane.  d = p - i is the diagonal, the window is
// [w0, w1) = [max(0, d - k), min(n, d + m + k)).  The lane runs Myers' column step in its SEARCH form (row 0 free, as
// bmx_approx_kernel.h) over the window's bytes with the state in W 64-bit words: word b holds query rows 64b .. 64b+63,
// and the horizontal delta that leaves bit 63 of word b enters bit 0 of word b + 1 (Myers 1999, the block form; Hyyro's
// statement of the carries).  The score is read in the word and at the bit of row m - 1; the words above it compute
// on masked Eq bits and feed nothing back (carries only travel upwards), and a wave skips the words that none of its
// lanes needs.  dist = the minimum of the score over the window, end = the LAST position that attains it.
// Eq words: the query stays in registers, 64 bytes per word in the layout of ed_batch_eq32 (byte 8k + j of a 32-byte
// half in byte k of register j), and Eq is built per text byte with it (bmx_eq_kernel.h).  The query is loaded byte by
// byte: 64 W byte loads against (m + 2k) W steps of ~150 VALU each.
// Text: aligned 8-byte words of the window, upwards, one word ahead; a word that holds no byte of the window is not
// loaded.  Every lane takes the same number of 8-byte chunks (the host passes ceil((M + 2k) / 8) for the longest seeded
// query M); steps at or behind w1 only stop counting, so waves stay converged.
//
// Starts (index_map_start_kernel<W>): for a candidate that hit, Myers' GLOBAL step (row 0 costs 1, as ed_batch_step) of
// the REVERSED query against text[end], text[end - 1], ..: after L bytes the score is ED(query, text[end-L+1 .. end]).
// It keeps the first L that attains the minimum over L = 1 .. min(end - w0 + 1, m + k): the largest start.  The lane
// then writes the candidate's (start, end, dist) to the caller's lists if its slot is below `capacity`, and to workspace
// for the per-query pass.  Text: aligned 8-byte words downwards, none below the word that holds w0.
//
// Best (index_map_best_kernel): one lane per query over its candidates, the smallest (dist, end) among the hits.
//
// Memory safety: a candidate with q >= count, offsets that decrease or end past the blob, a query of 0 or more than
// 64 W bytes, i >= m or p >= n raises status[0] and reads neither query nor text.  Every loop bound is a function of
// the chunk count the host passes (m, k and the instance); nothing waits on another workgroup.
#pragma once
#include "bmx_eq_kernel.h"
#include "bmx_index_match_kernel.h"

namespace bmx {

constexpr uint32_t MAP_NO_HIT = 255u;
constexpr uint32_t MAP_NO_POS32 = 0xffffffffu; // workspace: no end / no start

// the candidates blob byte b stands for: its occurrences if it is a seed
struct IndexMapCount {
    IndexSeedFlag flag;
    __host__ __device__ uint64_t operator()(uint64_t b) const { return flag(b) ? (uint64_t)flag.cnt[b] : 0ull; }
};

// the length of query q if it has a candidate, else 0 (offsets past the blob are kept inside the scan)
struct IndexMapSeededLen {
    const uint64_t *pat_off, *scan;
    uint64_t bytes;
    __host__ __device__ uint64_t operator()(uint64_t q) const
    {
        uint64_t o0 = pat_off[q], o1 = pat_off[q + 1];
        o0 = o0 < bytes ? o0 : bytes, o1 = o1 < bytes ? o1 : bytes;
        return o1 > o0 && scan[o1] > scan[o0] ? o1 - o0 : 0ull;
    }
};

struct IndexMapMax {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

// cand_off[q] = the candidates in front of query q (count + 1 entries; cand_off may be nullptr), res[0] = the total.
__global__ __launch_bounds__(INDEX_BLOCK) void index_map_off_kernel(const uint64_t *pat_off, uint64_t count, uint64_t bytes,
                                                                    const uint64_t *scan, uint64_t *cand_off, uint64_t *res)
{
    const uint64_t q = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (q > count) return;
    const uint64_t o = pat_off[q];
    const uint64_t s = scan[o < bytes ? o : bytes];
    if (cand_off) cand_off[q] = s;
    if (q == count) res[0] = s;
}

// q.status has a second meaning here, behind the match kernel's (whose two words are then 0: it has raised none).
// [0]: a candidate that failed its checks, [1]: a start pass that disagrees with its verification.  The directory is not read.
struct IndexMapArgs {
    IndexQuery q;
    const uint64_t *scan;      // bytes + 1 entries
    const uint32_t *qpos, *lo; // per blob byte
    uint64_t total;            // candidates
    uint32_t k;
    uint32_t chunks;           // 8-byte chunks every lane walks (verify: ceil((M + 2k) / 8), starts: ceil((M + k) / 8))
    uint32_t *cq, *ci, *cp;    // per candidate: query, position in the query, text position of the seed's occurrence
    uint32_t *cend, *cstart, *cdist; // per candidate: text positions (MAP_NO_POS32) and distance (MAP_NO_HIT)
    uint64_t base_offset;
    uint64_t *out_start, *out_end; // the caller's lists, `capacity` entries
    uint8_t *out_dist;
    uint64_t capacity;
    uint64_t *best_start, *best_end; // per query
    uint8_t *best_dist;
};

__global__ __launch_bounds__(INDEX_BLOCK) void index_map_fill_kernel(IndexMapArgs a)
{
    const uint64_t c = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (c >= a.total) return;
    uint64_t x = 0, y = a.q.pat_bytes; // the last b in [0, bytes) with scan[b] <= c (scan[0] == 0, scan[bytes] == total > c)
    while (y - x > 1) {
        const uint64_t mid = x + ((y - x) >> 1);
        if (a.scan[mid] <= c) x = mid;
        else y = mid;
    }
    const uint64_t b = x;
    const uint64_t q = index_query_of(a.q.pat_off, a.q.count, b);
    const uint64_t j = (uint64_t)a.lo[b] + (c - a.scan[b]);
    a.cq[c] = (uint32_t)q;
    a.ci[c] = a.qpos[b];
    a.cp[c] = index_entry(a.q.sa, j < a.q.n ? (uint32_t)j : a.q.n - 1u, a.q.n);
}

// The query Q[0..m) into 16 W registers, in the layout ed_batch_eq32 reads: bit 64w + 32h + 8k + j of Eq belongs to
// byte k of register 16w + 8h + j.  REVERSED: bit x belongs to Q[m - 1 - x].  Bytes at and above m stay 0.
template <int W, bool REVERSED>
__device__ __forceinline__ void map_load_query(uint32_t *p, const uint8_t *Q, uint32_t m)
{
#pragma unroll
    for (int r = 0; r < 16 * W; ++r) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x = 32u * (uint32_t)(r >> 3) + 8u * (uint32_t)k + (uint32_t)(r & 7);
            if (x < m) v |= (uint32_t)Q[REVERSED ? m - 1u - x : x] << (8 * k);
        }
        p[r] = v;
    }
}

// One column of W words.  hp, hm: the horizontal delta that enters row 0 (search form 0, 0; global form 1, 0).
// lw, hb: word and bit of row m - 1, where the score is read.  words: the wave needs words 0 .. words - 1 (uniform).
template <int W>
__device__ __forceinline__ void map_column(uint64_t *pv, uint64_t *mv, uint32_t &score, const uint32_t *p, uint32_t c,
                                           const uint64_t *mask, uint64_t hp, uint32_t lw, uint32_t hb, uint32_t words)
{
    const uint32_t c4 = c * 0x01010101u;
    uint64_t hm = 0;
#pragma unroll
    for (int b = 0; b < W; ++b) {
        if ((uint32_t)b < words) {
            uint64_t eq = ed_batch_eq<uint64_t>(p + 16 * b, c4, mask[b]);
            const uint64_t xv = eq | mv[b];
            eq |= hm;
            const uint64_t xh = (((eq & pv[b]) + pv[b]) ^ pv[b]) | eq;
            uint64_t ph = mv[b] | ~(xh | pv[b]);
            uint64_t mh = pv[b] & xh;
            const uint32_t here = (uint32_t)b == lw ? 1u : 0u;
            score += here * ((uint32_t)((ph >> hb) & 1) - (uint32_t)((mh >> hb) & 1));
            const uint64_t op = ph >> 63, om = mh >> 63;
            ph = (ph << 1) | hp;
            mh = (mh << 1) | hm;
            pv[b] = mh | ~(xv | ph);
            mv[b] = ph & xv;
            hp = op, hm = om;
        }
    }
}

// what both passes need of a candidate; ok == false: nothing of it is read
struct MapCand {
    bool ok;
    uint32_t m, lw, hb;
    uint32_t w0, w1;
    const uint8_t *Q;
};

template <int W>
__device__ __forceinline__ MapCand map_candidate(const IndexMapArgs &a, uint64_t c)
{
    MapCand r = {false, 1u, 0u, 0u, 0u, 0u, nullptr};
    if (c >= a.total) return r;
    const uint64_t q = a.cq[c];
    const uint32_t i = a.ci[c], p = a.cp[c];
    bool ok = q < a.q.count;
    uint64_t o0 = 0, o1 = 0;
    if (ok) {
        o0 = a.q.pat_off[q], o1 = a.q.pat_off[q + 1];
        ok = o1 > o0 && o1 <= a.q.pat_bytes && o1 - o0 <= 64u * W && (uint64_t)i < o1 - o0 && p < a.q.n;
    }
    if (!ok) {
        a.q.status[0] = 1;
        return r;
    }
    r.ok = true;
    r.m = (uint32_t)(o1 - o0);
    r.lw = (r.m - 1u) >> 6;
    r.hb = (r.m - 1u) & 63u;
    const int64_t d = (int64_t)p - (int64_t)i;
    const int64_t lo = d - (int64_t)a.k, hi = d + (int64_t)r.m + (int64_t)a.k;
    r.w0 = lo > 0 ? (uint32_t)lo : 0u;
    r.w1 = hi < (int64_t)a.q.n ? (uint32_t)hi : a.q.n; // > w0: the window holds the seed's occurrence
    r.Q = a.q.pat + o0;
    return r;
}

template <int W>
__device__ __forceinline__ uint32_t map_wave_words(bool ok, uint32_t lw)
{
    uint32_t words = 0;
#pragma unroll
    for (int b = 0; b < W; ++b)
        if (__ballot(ok && lw >= (uint32_t)b)) words = b + 1;
    return words;
}

template <int W>
__device__ __forceinline__ void map_masks(uint64_t *mask, const MapCand &cd)
{
#pragma unroll
    for (int b = 0; b < W; ++b)
        mask[b] = !cd.ok || (uint32_t)b > cd.lw ? 0ull : (uint32_t)b < cd.lw || cd.hb == 63u ? ~0ull : (2ull << cd.hb) - 1ull;
}

template <int W>
__global__ __launch_bounds__(INDEX_BLOCK) void index_map_verify_kernel(const IndexMapArgs a)
{
    const uint64_t c = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    const MapCand cd = map_candidate<W>(a, c);
    const uint32_t words = map_wave_words<W>(cd.ok, cd.lw);
    if (words == 0) return; // (uniform: no lane of the wave has a candidate)

    uint32_t p[16 * W];
    map_load_query<W, false>(p, cd.Q, cd.ok ? cd.m : 0u);
    uint64_t mask[W], pv[W], mv[W];
    map_masks<W>(mask, cd);
#pragma unroll
    for (int b = 0; b < W; ++b) pv[b] = ~0ull, mv[b] = 0ull;
    uint32_t score = cd.m, best = 0xffffffffu, best_end = 0;

    // aligned 8-byte words of the window, from the word that holds w0 to the one that holds w1 - 1
    const uintptr_t t0 = (uintptr_t)a.q.text;
    const uint64_t *words8 = reinterpret_cast<const uint64_t *>(t0 & ~(uintptr_t)7);
    const uint64_t first = t0 & 7u;
    uint64_t wi = (first + cd.w0) >> 3;
    const uint64_t wlast = cd.ok ? (first + cd.w1 - 1u) >> 3 : 0;
    const uint32_t sh = (uint32_t)((first + cd.w0) & 7u) * 8u;
    uint64_t lo = cd.ok ? words8[wi] : 0ull;
    uint64_t hi = cd.ok && wi + 1 <= wlast ? words8[wi + 1] : 0ull;
    uint32_t pos = cd.w0;
    for (uint32_t ch = 0; ch < a.chunks; ++ch) {
        const uint64_t cur = sh ? (lo >> sh) | (hi << (64u - sh)) : lo; // text[pos .. pos + 8), the first in the low byte
        lo = hi;
        ++wi;
        hi = cd.ok && wi + 1 <= wlast ? words8[wi + 1] : 0ull; // one word ahead of its use
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            map_column<W>(pv, mv, score, p, (uint32_t)(cur >> (8 * t)) & 0xffu, mask, 0ull, cd.lw, cd.hb, words);
            if (pos < cd.w1 && score <= best) best = score, best_end = pos; // the last end that attains the minimum
            ++pos;
        }
    }
    if (!cd.ok) return;
    const bool hit = best <= a.k;
    a.cend[c] = hit ? best_end : MAP_NO_POS32;
    a.cdist[c] = hit ? best : MAP_NO_HIT;
}

template <int W>
__global__ __launch_bounds__(INDEX_BLOCK) void index_map_start_kernel(const IndexMapArgs a)
{
    const uint64_t c = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    MapCand cd = map_candidate<W>(a, c);
    const uint32_t end = cd.ok ? a.cend[c] : MAP_NO_POS32;
    const uint32_t dist = cd.ok ? a.cdist[c] : MAP_NO_HIT;
    const bool listed = c < a.total;
    cd.ok = cd.ok && dist != MAP_NO_HIT && end >= cd.w0 && end < cd.w1; // from here on: a hit to walk back from
    const uint32_t words = map_wave_words<W>(cd.ok, cd.lw);
    uint32_t best = 0xffffffffu, best_len = 0;
    if (words != 0) { // (uniform)
        uint32_t p[16 * W];
        map_load_query<W, true>(p, cd.Q, cd.ok ? cd.m : 0u);
        uint64_t mask[W], pv[W], mv[W];
        map_masks<W>(mask, cd);
#pragma unroll
        for (int b = 0; b < W; ++b) pv[b] = ~0ull, mv[b] = 0ull;
        uint32_t score = cd.m, len = 0;
        const uint32_t steps = cd.ok ? min(end - cd.w0 + 1u, cd.m + a.k) : 0u;

        const uintptr_t t0 = (uintptr_t)a.q.text;
        const uint64_t *words8 = reinterpret_cast<const uint64_t *>(t0 & ~(uintptr_t)7);
        const uint64_t first = t0 & 7u;
        int64_t wi = cd.ok ? (int64_t)((first + end) >> 3) : 0;
        const int64_t wfirst = (int64_t)((first + cd.w0) >> 3); // nothing below the word that holds w0 is loaded
        const uint32_t b = cd.ok ? (uint32_t)((first + end) & 7u) : 0u;
        uint64_t hi = cd.ok ? words8[wi] : 0ull; // text[end] is byte b of hi
        uint64_t lo = cd.ok && wi - 1 >= wfirst ? words8[wi - 1] : 0ull;
        for (uint32_t ch = 0; ch < a.chunks; ++ch) {
            // the next 8 bytes downwards, the first of them in the top byte
            const uint64_t cur = (hi << (8u * (7u - b))) | ((lo >> (8u * b)) >> 8);
            hi = lo;
            --wi;
            lo = cd.ok && wi - 1 >= wfirst ? words8[wi - 1] : 0ull; // one word ahead of its use
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                map_column<W>(pv, mv, score, p, (uint32_t)(cur >> (8 * (7 - t))) & 0xffu, mask, 1ull, cd.lw, cd.hb, words);
                ++len;
                if (len <= steps && score < best) best = score, best_len = len; // the first length that attains the minimum
            }
        }
    }
    if (!listed) return;
    uint32_t start = MAP_NO_POS32;
    if (cd.ok) {
        if (best != dist) a.q.status[1] = 1;
        start = end - (best_len - 1u);
    }
    a.cstart[c] = start;
    if (c < a.capacity) {
        a.out_start[c] = cd.ok ? a.base_offset + start : ~0ull;
        a.out_end[c] = cd.ok ? a.base_offset + end : ~0ull;
        a.out_dist[c] = (uint8_t)(cd.ok ? dist : MAP_NO_HIT);
    }
}

__global__ __launch_bounds__(INDEX_BLOCK) void index_map_best_kernel(const IndexMapArgs a)
{
    const uint64_t q = (uint64_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (q >= a.q.count) return;
    uint64_t c0 = 0, c1 = 0;
    if (a.total) { // (without a candidate the scan is not read: every query is unmapped)
        const uint64_t o0 = a.q.pat_off[q], o1 = a.q.pat_off[q + 1];
        c0 = a.scan[o0 < a.q.pat_bytes ? o0 : a.q.pat_bytes];
        c1 = a.scan[o1 < a.q.pat_bytes ? o1 : a.q.pat_bytes];
        if (c1 > a.total) c1 = a.total;
    }
    uint32_t bd = MAP_NO_HIT, be = MAP_NO_POS32, bs = MAP_NO_POS32;
    for (uint64_t c = c0; c < c1; ++c) {
        const uint32_t d = a.cdist[c], e = a.cend[c];
        if (d != MAP_NO_HIT && (d < bd || (d == bd && e < be))) bd = d, be = e, bs = a.cstart[c];
    }
    const bool hit = bd != MAP_NO_HIT && bs != MAP_NO_POS32;
    a.best_start[q] = hit ? a.base_offset + bs : ~0ull;
    a.best_end[q] = hit ? a.base_offset + be : ~0ull;
    a.best_dist[q] = (uint8_t)(hit ? bd : MAP_NO_HIT);
}

} // namespace bmx
