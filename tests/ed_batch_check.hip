// ed_batch_check.hip -- the lane functions of csrc/bmx_ed_batch_kernel.h (ed_batch_load_pattern, ed_batch_walk with
// ed_batch_step, and ed_batch_eq of csrc/bmx_eq_kernel.h) run on the CPU, one "lane" at a time, against the plain
// two-row edit table written out below.  Both words (32 bits: m in 1..32, 64 bits: m in 1..64), both Eq sources (the
// pattern in registers, and a 256-word Peq built as the kernel builds it, with P = P_end = nullptr as the kernel passes
// them), 0..16 bytes of slack between the pattern's end and its blob's end, alphabets of 2, 4, 95 and 256 symbols, walked
// strings that are the pattern itself, the pattern a few edits apart, and unrelated strings of under 16 bytes and of every
// length modulo 16.  Every pattern lies at the end of a heap allocation of exactly lead + m + slack bytes and every walked
// string in one of exactly n bytes: built with -fsanitize=address,undefined (tests/test_ed_batch_cpu.py) a load that
// leaves either is an error, not a lucky pass.  The registers that ed_batch_load_pattern fills are compared byte by byte
// with the transposed layout AND with which chunks may come in one 16-byte load: a chunk that fits its blob holds the
// blob's bytes past the pattern too, a chunk that does not holds zeros there.  No device call is made.  Prints one line
// per failure (the first 20), "pairs = N" and "bad = N"; exit status 1 if bad != 0.
#define BMX_ED_BATCH_PIECES_ONLY
#include "bmx_ed_batch_kernel.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bmx;

typedef std::vector<uint8_t> Bytes;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) // 0 .. n - 1
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

static uint8_t symbol(int sigma)
{
    const uint32_t v = rnd((uint32_t)sigma);
    return sigma == 4 ? (uint8_t) "ACGT"[v] : sigma == 95 ? (uint8_t)(0x20 + v) : (uint8_t)v; // 256: half of them >= 0x80
}

static Bytes rand_string(size_t n, int sigma)
{
    Bytes s(n);
    for (auto &c : s) c = symbol(sigma);
    return s;
}

static Bytes edited(Bytes s, int k, int sigma)
{
    for (; k > 0; --k) {
        const uint32_t op = s.empty() ? 1 : rnd(3);
        if (op == 0) s[rnd((uint32_t)s.size())] = symbol(sigma);
        else if (op == 1) s.insert(s.begin() + rnd((uint32_t)s.size() + 1), symbol(sigma));
        else if (s.size() > 1) s.erase(s.begin() + rnd((uint32_t)s.size()));
    }
    return s;
}

// the plain table, two rows
static uint32_t table_distance(const uint8_t *a, size_t la, const uint8_t *b, size_t lb)
{
    std::vector<uint32_t> prev(lb + 1), cur(lb + 1);
    for (size_t j = 0; j <= lb; ++j) prev[j] = (uint32_t)j;
    for (size_t i = 1; i <= la; ++i) {
        cur[0] = (uint32_t)i;
        for (size_t j = 1; j <= lb; ++j) cur[j] = std::min({prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1});
        std::swap(prev, cur);
    }
    return prev[lb];
}

static int bad = 0, pairs = 0, loads = 0;
static bool seen_mod[2][16], seen_small[2][16], seen_n_eq_m[2][65];

static void fail(const char *what, int bits, uint32_t m, uint32_t slack, int sigma, uint32_t n, uint32_t got, uint32_t want)
{
    if (bad++ < 20) printf("%s: %d-bit, m = %u, slack = %u, sigma = %d, n = %u: got %u, want %u\n", what, bits, m, slack, sigma, n, got, want);
}

// ed_batch_load_pattern's registers: byte 8k + j of half h in byte k of register 8h + j.  Chunk c (16 bytes) is read at
// all only if 16c < m; in one load if it ends at or before `end` (then it holds the blob's bytes past the pattern too),
// else byte by byte below m (zeros past the pattern).
template <int ND>
static void check_load(const uint8_t *P, uint32_t m, const uint8_t *end, uint32_t slack, int sigma)
{
    uint32_t p[ND];
    ed_batch_load_pattern<ND>(p, P, m, end);
    ++loads;
    for (uint32_t t = 0; t < 4u * ND; ++t) {
        const uint32_t c = t / 16;
        uint8_t want = 0;
        if (t < m) want = P[t];
        else if (16 * c < m && P + 16 * c + 16 <= end) want = P[t];
        const uint32_t h = t / 32, k = (t % 32) / 8, j = t % 8;
        const uint8_t got = (uint8_t)(p[8 * h + j] >> (8 * k));
        if (got != want) {
            fail("pattern byte", ND * 4, m, slack, sigma, t, got, want);
            return;
        }
    }
}

template <typename W>
static void check_pair(const Bytes &pat, uint32_t slack, const Bytes &text, int sigma)
{
    constexpr int BITS = 8 * (int)sizeof(W), WI = sizeof(W) == 8;
    const uint32_t m = (uint32_t)pat.size(), n = (uint32_t)text.size(), lead = rnd(4);
    // the pattern's blob: `lead` bytes, the pattern, `slack` bytes of the same alphabet (never a free pass for a missing
    // mask: a slack byte can equal a text byte), in an allocation of exactly that size; the walked string in one of n bytes
    uint8_t *blob = (uint8_t *)malloc(lead + m + slack), *T = (uint8_t *)malloc(n);
    for (uint32_t i = 0; i < lead; ++i) blob[i] = symbol(sigma);
    memcpy(blob + lead, pat.data(), m);
    for (uint32_t i = 0; i < slack; ++i) blob[lead + m + i] = sigma == 2 ? (uint8_t)(1 + rnd(255)) : symbol(sigma);
    memcpy(T, text.data(), n);
    const uint8_t *P = blob + lead, *end = blob + lead + m + slack;
    const uint32_t want = table_distance(pat.data(), m, text.data(), n);

    check_load<sizeof(W) == 4 ? 8 : 16>(P, m, end, slack, sigma);
    const uint32_t in_regs = ed_batch_walk<W, false>(P, m, end, T, n, nullptr);
    if (in_regs != want) fail("Eq from registers", BITS, m, slack, sigma, n, in_regs, want);
    uint64_t peq[256]; // as the kernel: cleared, then bit tid of the word of query byte tid
    for (int i = 0; i < 256; ++i) peq[i] = 0;
    for (uint32_t tid = 0; tid < m; ++tid) peq[P[tid]] |= 1ull << tid;
    const uint32_t in_lds = ed_batch_walk<W, true>(nullptr, m, nullptr, T, n, peq);
    if (in_lds != want) fail("Eq from the Peq", BITS, m, slack, sigma, n, in_lds, want);
    pairs += 2;
    seen_mod[WI][n % 16] = true;
    if (n < 16) seen_small[WI][n] = true;
    if (n == m) seen_n_eq_m[WI][m] = true;
    free(blob);
    free(T);
}

template <typename W>
static void run_word()
{
    const uint32_t top = 8 * (uint32_t)sizeof(W);
    for (int sigma : {2, 4, 95, 256})
        for (uint32_t m = 1; m <= top; ++m)
            for (uint32_t slack = 0; slack <= 16; ++slack) {
                const Bytes pat = rand_string(m, sigma);
                check_pair<W>(pat, slack, pat, sigma);                                        // n = m, distance 0
                check_pair<W>(pat, slack, edited(pat, (int)rnd(9), sigma), sigma);            // a few edits apart
                check_pair<W>(pat, slack, rand_string(1 + (m + slack) % 15, sigma), sigma);   // unrelated, n < 16
                check_pair<W>(pat, slack, rand_string(16 + (3 * m + slack) % 80, sigma), sigma); // unrelated, every n mod 16
                check_pair<W>(pat, slack, edited(rand_string(m + rnd(40), sigma), 3, sigma), sigma); // unrelated, n around m
            }
}

int main()
{
    run_word<uint32_t>();
    run_word<uint64_t>();
    // what the loops above claim to cover
    for (int w = 0; w < 2; ++w) {
        for (int r = 0; r < 16; ++r)
            if (!seen_mod[w][r]) fail("no walked length with this n mod 16", 32 << w, 0, 0, 0, (uint32_t)r, 0, 1);
        for (int n = 1; n < 16; ++n)
            if (!seen_small[w][n]) fail("no walked length n < 16", 32 << w, 0, 0, 0, (uint32_t)n, 0, 1);
        for (int m = 1; m <= (32 << w); ++m)
            if (!seen_n_eq_m[w][m]) fail("no walked length n = m", 32 << w, (uint32_t)m, 0, 0, (uint32_t)m, 0, 1);
    }
    printf("pattern loads = %d\npairs = %d\nbad = %d\n", loads, pairs, bad);
    return bad != 0;
}
