// bmx_myers_words.h -- Myers' bit-parallel column over several 64-bit words per lane, for patterns of 65 to 512 bytes
// (DESIGN.md s22): what the long approximate search (bmx_approx_long_kernel.h) and the long form of the starts pass
// (bmx_spans_kernel.h) share.  The pattern travels by value as a kernel argument, the workgroup builds its Peq table in
// LDS from it, and one column step runs the words in order, handing the horizontal deltas' top bits upwards.
//
// LDS layout.  tab[256][W] 64-bit words, stored as W / 2 pairs: row c holds, for byte value c, bit i of word b set iff
// pattern position 64 b + i holds c.  A lane fetches its byte's row with W / 2 reads of 128 bits.  2 KiB x W: 16 KiB at W = 8.
//
// Words.  A pattern of m positions needs words = ceil(m / 64) of them and takes the smallest instantiated W in {2, 4, 8}
// that covers it, so words > W / 2.  The column runs whole PAIRS of words: pairs below W / 4 + 1 unconditionally (every
// pattern of this W needs them), the rest while 2 * pair < words -- wave-uniform, from m.  A word above the pattern has an
// all-zero Peq and receives carries only; nothing flows downwards, so the extra word of an odd count is harmless.
//
// The three functions are __host__ __device__ so that tests/myers_words_check.hip can run them on the CPU against the plain
// edit table (tests/test_myers_words_cpu.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmx {

constexpr int MAX_APPROX_LONG_PATTERN = 512; // == BMX_MAX_APPROX_LONG_PATTERN

typedef uint64_t words_u64x2 __attribute__((ext_vector_type(2)));

// The pattern as a kernel argument (bytes at and above m are not read).
struct LongPattern {
    uint32_t w[MAX_APPROX_LONG_PATTERN / 4];
};

// The smallest instantiated word count that covers m positions (m > 64).
inline int words_for(int32_t m) { return m <= 128 ? 2 : m <= 256 ? 4 : 8; }

template <int W>
struct WordsColumn {
    uint64_t pv[W], mv[W];
    uint32_t score;
};

template <int W>
__host__ __device__ __forceinline__ void words_init(WordsColumn<W> &s, uint32_t m)
{
#pragma unroll
    for (int b = 0; b < W; ++b) s.pv[b] = ~0ull, s.mv[b] = 0;
    s.score = m;
}

// Lane tid of 256 builds row tid of the table from the pattern (uniform reads of the kernel argument).
template <int W>
__host__ __device__ __forceinline__ void words_fill(words_u64x2 *tab, const LongPattern &pat, uint32_t m, uint32_t tid)
{
    uint64_t *row = reinterpret_cast<uint64_t *>(tab) + (size_t)tid * W;
    for (uint32_t b = 0; b < (uint32_t)W; ++b) {
        uint64_t word = 0;
        for (uint32_t q = 0; q < 16; ++q) { // 16 dwords of four pattern bytes
            const uint32_t at = 64 * b + 4 * q;
            if (at >= m) break; // (uniform)
            const uint32_t v = pat.w[at >> 2];
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r)
                if (at + r < m && ((v >> (8 * r)) & 0xFFu) == tid) word |= 1ull << (4 * q + r);
        }
        row[b] = word;
    }
}

// One column: the text byte's row of the table, hp = the horizontal delta that enters row 0 (search form 0, global form
// 1).  lw, hb: word and bit of row m - 1, where the score is read; lw >= W / 2.  The word step is that of map_column
// (bmx_index_map_kernel.h): Hyyro's block form of Myers' recurrence.
template <int W>
__host__ __device__ __forceinline__ void words_column(WordsColumn<W> &s, const words_u64x2 *row, uint64_t hp, uint32_t lw,
                                                      uint32_t hb, uint32_t words)
{
    uint64_t hm = 0;
#pragma unroll
    for (int p = 0; p < W / 2; ++p) {
        if (p < W / 4 + 1 || 2u * (uint32_t)p < words) {
            const words_u64x2 e = row[p];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int b = 2 * p + h;
                uint64_t eq = e[h];
                const uint64_t xv = eq | s.mv[b];
                eq |= hm;
                const uint64_t xh = (((eq & s.pv[b]) + s.pv[b]) ^ s.pv[b]) | eq;
                uint64_t ph = s.mv[b] | ~(xh | s.pv[b]);
                uint64_t mh = s.pv[b] & xh;
                if (b >= W / 2 && (uint32_t)b == lw) // (uniform)
                    s.score += (uint32_t)((ph >> hb) & 1) - (uint32_t)((mh >> hb) & 1);
                const uint64_t op = ph >> 63, om = mh >> 63;
                ph = (ph << 1) | hp;
                mh = (mh << 1) | hm;
                s.pv[b] = mh | ~(xv | ph);
                s.mv[b] = ph & xv;
                hp = op, hm = om;
            }
        }
    }
}

} // namespace bmx
