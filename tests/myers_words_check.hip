// myers_words_check.hip -- the multi-word Myers column of csrc/bmx_myers_words.h (words_fill, words_init, words_column)
// run on the CPU against the plain edit table, column by column: the search form (zero enters row 0) and the global form
// (1 enters row 0), every word count, lengths at every word boundary, alphabets of 1 to 26 letters, one planted copy
// with a substitution.  Built and run by tests/test_myers_words_cpu.py; no device call is made.  Prints one line per
// mismatch (the first of a run) and "bad = N"; exit status 1 if N != 0.
#include "bmx_myers_words.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bmx;

template <int W>
static int run(int m, int n, int sigma, unsigned seed, bool global)
{
    srand(seed);
    std::vector<uint8_t> pat(m), text(n);
    for (auto &c : pat) c = 'a' + rand() % sigma;
    for (auto &c : text) c = 'a' + rand() % sigma;
    if (n > m) {
        memcpy(&text[(n - m) / 2], pat.data(), m);
        text[(n - m) / 2 + m / 2] ^= 1;
    }
    LongPattern lp;
    memset(&lp, 0, sizeof lp);
    memcpy(lp.w, pat.data(), m);
    std::vector<words_u64x2> tab(256 * W / 2);
    for (uint32_t tid = 0; tid < 256; ++tid) words_fill<W>(tab.data(), lp, m, tid);
    WordsColumn<W> s;
    words_init<W>(s, m);
    const uint32_t lw = (m - 1) >> 6, hb = (m - 1) & 63, words = lw + 1;
    std::vector<int> col(m + 1), next(m + 1);
    for (int i = 0; i <= m; ++i) col[i] = i;
    int bad = 0;
    for (int j = 0; j < n; ++j) {
        words_column<W>(s, tab.data() + (size_t)text[j] * (W / 2), global ? 1 : 0, lw, hb, words);
        next[0] = global ? j + 1 : 0;
        for (int i = 1; i <= m; ++i) next[i] = std::min({col[i - 1] + (pat[i - 1] != text[j]), col[i] + 1, next[i - 1] + 1});
        col.swap(next);
        if ((int)s.score != col[m]) {
            if (!bad) printf("W = %d, m = %d, sigma = %d, %s form, column %d: score %u, table %d\n", W, m, sigma,
                             global ? "global" : "search", j, s.score, col[m]);
            ++bad;
        }
    }
    return bad;
}

int main()
{
    int bad = 0, runs = 0;
    for (int global = 0; global < 2; ++global)
        for (int sigma : {1, 2, 4, 26}) {
            for (int m : {65, 66, 127, 128}) bad += run<2>(m, 700, sigma, m, global), ++runs;
            for (int m : {129, 191, 192, 193, 255, 256}) bad += run<4>(m, 900, sigma, m, global), ++runs;
            for (int m : {257, 320, 321, 383, 384, 385, 448, 449, 511, 512}) bad += run<8>(m, 1500, sigma, m, global), ++runs;
        }
    printf("runs = %d\nbad = %d\n", runs, bad);
    return bad != 0;
}
