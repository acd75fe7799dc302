// align_check.hip -- the alignment pieces of csrc/bmx_align_kernel.h (align_load_pattern, align_column,
// align_store_planes, align_traceback) run on the CPU: 64 "lanes" share one wave's column workspace in the
// kernel's layout, each runs the forward pass over its span and walks back, and every script is compared with the walk
// over the plain edit table written out below.  Every instance (a 32-bit word, 1, 2, 4 and 8 64-bit words), every length
// of {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512} the instance holds, one substitution, insertion
// and deletion at the first row, at the last row and at rows 63 and 64, random edits over 2, 4 and 95 symbols, a slot of
// exactly 2 dist + 1 words, and every 64-bit instance again with only the band |i - t| <= k stored (windows of one to
// four halves).  Built and run by tests/test_align_cpu.py; no device call is made.  Prints one line per
// failing pair and "bad = N"; exit status 1 if N != 0.
#define BMX_ALIGN_PIECES_ONLY
#include "bmx_align_kernel.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace bmx;

typedef std::vector<uint8_t> Bytes;

// the plain table and the canonical walk: diagonal, up (I), left (D), the first that keeps the value
static std::vector<uint32_t> table_walk(const Bytes &pat, const Bytes &span, uint32_t *dist)
{
    const size_t m = pat.size(), L = span.size(), w = L + 1;
    std::vector<int> D((m + 1) * w);
    for (size_t t = 0; t <= L; ++t) D[t] = (int)t;
    for (size_t i = 1; i <= m; ++i) {
        D[i * w] = (int)i;
        for (size_t t = 1; t <= L; ++t)
            D[i * w + t] = std::min({D[(i - 1) * w + t - 1] + (pat[i - 1] != span[t - 1]), D[(i - 1) * w + t] + 1, D[i * w + t - 1] + 1});
    }
    *dist = (uint32_t)D[m * w + L];
    std::vector<uint32_t> ops; // one per step, from the end
    size_t i = m, t = L;
    while (i > 0 || t > 0) {
        const int v = D[i * w + t];
        if (i > 0 && t > 0 && D[(i - 1) * w + t - 1] + (pat[i - 1] != span[t - 1]) == v) {
            ops.push_back(pat[i - 1] == span[t - 1] ? CIGAR_EQ : CIGAR_X), --i, --t;
        } else if (i > 0 && D[(i - 1) * w + t] + 1 == v) {
            ops.push_back(CIGAR_INS), --i;
        } else {
            ops.push_back(CIGAR_DEL), --t;
        }
    }
    std::reverse(ops.begin(), ops.end());
    std::vector<uint32_t> runs;
    for (uint32_t c : ops) {
        if (!runs.empty() && (runs.back() & 15u) == c) runs.back() += 16u;
        else runs.push_back(16u | c);
    }
    return runs;
}

static std::string text_of(const uint32_t *runs, size_t n)
{
    std::string s;
    for (size_t r = 0; r < n; ++r) s += std::to_string(runs[r] >> 4) + "MIDNSHP=X"[runs[r] & 15u];
    return s;
}

// one edit of `kind` (0 X, 1 I: the span loses a byte, 2 D: the span gains one) at pattern row `row`
static Bytes edited(const Bytes &pat, int kind, size_t row, int sigma)
{
    Bytes s = pat;
    row = std::min(row, pat.size() - 1);
    if (kind == 0) s[row] = (uint8_t)(' ' + (s[row] - ' ' + 1) % sigma);
    else if (kind == 1) s.erase(s.begin() + row);
    else s.insert(s.begin() + row, (uint8_t)(' ' + rand() % sigma));
    return s;
}

template <typename T, int W, bool BAND>
static int run_wave(uint32_t m, int sigma, unsigned seed)
{
    constexpr uint32_t BITS = 8 * (uint32_t)sizeof(T);
    constexpr int REGS = 2 * (int)sizeof(T) * W;
    srand(seed);
    std::vector<Bytes> pats(64), spans(64);
    size_t longest = 1;
    for (int lane = 0; lane < 64; ++lane) {
        Bytes &p = pats[lane];
        p.resize(m);
        for (auto &c : p) c = (uint8_t)(' ' + rand() % sigma);
        if (lane < 12) { // each kind of edit at the first row, the last row and rows 63 / 64
            const size_t rows[4] = {0, m - 1, 63, 64};
            spans[lane] = edited(p, lane % 3, rows[lane / 3], sigma);
        } else {
            Bytes s = p;
            for (int e = rand() % 9; e > 0 && !s.empty(); --e) s = edited(s, rand() % 3, rand() % s.size(), sigma);
            spans[lane] = s;
        }
        if (spans[lane].empty()) spans[lane] = Bytes(1, (uint8_t)' ');
        longest = std::max(longest, spans[lane].size());
    }
    const uint32_t C = 8 * (uint32_t)((longest + 7) / 8);
    // BAND: one k for the wave, the largest distance plus 0, 16, 32 or 48 (windows of one to four halves), as far as the
    // band is still what the kernel would store for it
    uint32_t k = 0;
    if (BAND) {
        for (int lane = 0; lane < 64; ++lane) {
            uint32_t d = 0;
            table_walk(pats[lane], spans[lane], &d);
            k = std::max(k, d);
        }
        uint32_t extra = 16 * (seed % 4);
        while (extra > 0 && !align_use_band(k + extra, 8, W)) extra -= 16;
        k += extra;
        if (!align_use_band(k, 8, W)) return 0;
    }
    const uint32_t halves = align_band_halves(k);
    typedef typename std::conditional<BAND, uint32_t, T>::type E;
    const size_t stride = align_stride<T, W, BAND>(halves);
    std::vector<E> cols((size_t)C * stride, (E)0x5a); // (a stale word must not matter)
    int bad = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const Bytes &pat = pats[lane], &span = spans[lane];
        const uint32_t L = (uint32_t)span.size();
        uint32_t want_dist = 0;
        const std::vector<uint32_t> want = table_walk(pat, span, &want_dist);

        uint32_t p[REGS];
        align_load_pattern<REGS>(p, pat.data(), m);
        const uint32_t lw = (m - 1) / BITS, hb = (m - 1) % BITS, words = lw + 1;
        T mask[W], pv[W], mv[W];
        for (int b = 0; b < W; ++b) {
            mask[b] = (uint32_t)b > lw ? (T)0 : (uint32_t)b < lw || hb == BITS - 1 ? (T)~(T)0 : (T)(((T)2 << hb) - 1);
            pv[b] = (T)~(T)0, mv[b] = 0;
        }
        uint32_t score = m;
        E *col = cols.data() + lane;
        for (uint32_t t = 0; t < L; ++t) {
            const AlignStore st = {col + (size_t)t * stride, halves, (int)t - (int)k};
            align_column<T, W, BAND>(pv, mv, score, p, span[t], mask, lw, hb, words, st);
        }
        bool ok = score == want_dist;
        const uint32_t slot_words = 2 * want_dist + 1;
        std::vector<uint32_t> slot(slot_words + 2, 0xdeadbeefu); // a guard word on either side
        const uint32_t n = align_traceback<T, W, BAND>(col, halves, k, m, L, score, slot.data() + 1, slot_words);
        ok = ok && n == want.size() && slot[0] == 0xdeadbeefu && slot[slot_words + 1] == 0xdeadbeefu &&
             std::equal(want.begin(), want.end(), slot.begin() + 1 + (slot_words - n));
        if (!ok) {
            printf("%d-bit x %d%s, m = %u, L = %u, sigma = %d, lane %d: dist %u (table %u), script %s (table %s)\n", (int)BITS, W, BAND ? " (band)" : "", m, L,
                   sigma, lane, score, want_dist, n <= slot_words ? text_of(slot.data() + 1 + (slot_words - n), n).c_str() : "?",
                   text_of(want.data(), want.size()).c_str());
            ++bad;
        }
    }
    return bad;
}

int main()
{
    int bad = 0, runs = 0;
    const uint32_t lengths[] = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512};
    for (int sigma : {2, 4, 95})
        for (uint32_t m : lengths) {
            if (m <= 32) bad += run_wave<uint32_t, 1, false>(m, sigma, m), ++runs;
            if (m <= 64) bad += run_wave<uint64_t, 1, false>(m, sigma, m + 1000), ++runs;
            if (m <= 128) bad += run_wave<uint64_t, 2, false>(m, sigma, m + 2000), ++runs;
            if (m <= 256) bad += run_wave<uint64_t, 4, false>(m, sigma, m + 3000), ++runs;
            bad += run_wave<uint64_t, 8, false>(m, sigma, m + 4000), ++runs;
            // ... and with only the band stored (one to four halves)
            if (m <= 64) bad += run_wave<uint64_t, 1, true>(m, sigma, m + 1000), ++runs;
            if (m <= 128) bad += run_wave<uint64_t, 2, true>(m, sigma, m + 2000), ++runs;
            if (m <= 256) bad += run_wave<uint64_t, 4, true>(m, sigma, m + 3000), ++runs;
            bad += run_wave<uint64_t, 8, true>(m, sigma, m + 4000), ++runs;
        }
    printf("runs = %d\nbad = %d\n", runs, bad);
    return bad != 0;
}
