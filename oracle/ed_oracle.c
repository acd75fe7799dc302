/*
 * ed_oracle.c -- TEST INFRASTRUCTURE ONLY (same rules as bm_oracle.c).
 *
 * CPU restatement of the reference's SECOND algorithm, Levenshtein distance:
 *   EditDistance-1/EditDistance-1/sequential.c:18-46   editDistDP (full int table)
 *   EditDistance-1/EditDistance-1/kernal.cl:5-56       one anti-diagonal per launch
 * Same recurrence -- equal characters take the diagonal, otherwise 1 + min of
 * diagonal, left, up -- kept in two rolling rows so that BASELINE config 5
 * (64k x 64k, a 17 GB table in the reference) fits.  Pinned to editDistDP itself
 * (oracle/_ref) up to 6000 x 6000 and to SURVEY.md's known answers ED-1 / ED-2.
 */
#include <stdint.h>
#include <stdlib.h>

/* rows follow `b` (kernal.cl: b[r-1]), columns follow `a` (a[c-1]) */
int64_t edo_edit_distance(const char *a, uint64_t la, const char *b, uint64_t lb)
{
    uint32_t *prev = (uint32_t *)malloc((la + 1) * sizeof(uint32_t));
    uint32_t *cur = (uint32_t *)malloc((la + 1) * sizeof(uint32_t));
    if (!prev || !cur) {
        free(prev);
        free(cur);
        return -1;
    }
    for (uint64_t c = 0; c <= la; ++c) prev[c] = (uint32_t)c; /* sequential.c:28-29 */
    for (uint64_t r = 1; r <= lb; ++r) {
        cur[0] = (uint32_t)r; /* :31-32 */
        const char br = b[r - 1];
        for (uint64_t c = 1; c <= la; ++c) {
            if (br == a[c - 1]) {
                cur[c] = prev[c - 1]; /* :33-34, kernal.cl:34-38 */
            } else {
                uint32_t mi = prev[c - 1]; /* :39-42, kernal.cl:40-53 */
                if (mi > cur[c - 1]) mi = cur[c - 1];
                if (mi > prev[c]) mi = prev[c];
                cur[c] = mi + 1;
            }
        }
        uint32_t *t = prev;
        prev = cur;
        cur = t;
    }
    int64_t d = prev[la];
    free(prev);
    free(cur);
    return d;
}

/*
 * The same recurrence with Ukkonen's cut-off: only the cells of a diagonal band are computed,
 *   -t <= c - r <= t + (la - lb)      (la >= lb; the strings are swapped otherwise),
 * everything outside counts as infinite.  A path of cost <= t leaves the main diagonal by at most t
 * insertions or deletions more than it needs to reach the last cell, so it stays inside the band: the
 * result is the distance whenever that is <= t.  Returns the distance if it is <= t, -2 ("more than t")
 * otherwise, -1 without memory.  About max(la, lb) * (2 t + |la - lb|) cells.  No bit tricks, nothing
 * shared with the GPU kernels: plain rows like edo_edit_distance above (whole rows of la + 2 cells are
 * allocated and preset, of which a row touches its band only: simple, and nothing next to the band's cells).
 * "Infinite" is 2^30 - 1: thresholds up to that are served, a larger one is refused with -2 like a
 * distance above it (the tests use strings of a few million characters).
 */
int64_t edo_edit_distance_within(const char *a, uint64_t la, const char *b, uint64_t lb, uint64_t t)
{
    const uint32_t INF = 0x3fffffffu; /* (+ 1 does not wrap) */
    if (la < lb) { /* the distance is symmetric */
        const char *ts = a;
        a = b;
        b = ts;
        uint64_t tl = la;
        la = lb;
        lb = tl;
    }
    const uint64_t diff = la - lb;
    if (diff > t || t >= INF) return -2;
    if (t > la) t = la; /* the distance is never more than max(la, lb) */
    uint32_t *prev = (uint32_t *)malloc((la + 2) * sizeof(uint32_t));
    uint32_t *cur = (uint32_t *)malloc((la + 2) * sizeof(uint32_t));
    if (!prev || !cur) {
        free(prev);
        free(cur);
        return -1;
    }
    for (uint64_t c = 0; c <= la + 1; ++c) prev[c] = cur[c] = INF;
    for (uint64_t c = 0; c <= la && c <= t + diff; ++c) prev[c] = (uint32_t)c; /* row 0 inside the band */
    for (uint64_t r = 1; r <= lb; ++r) {
        const uint64_t lo = r > t ? r - t : 0;                             /* first column of the band in this row */
        const uint64_t hi = r + t + diff < la ? r + t + diff : la;         /* last one */
        const char br = b[r - 1];
        uint64_t c = lo;
        if (lo == 0) {
            cur[0] = (uint32_t)r;
            c = 1;
        } else {
            cur[lo - 1] = INF; /* (held a cell of row r - 2) */
        }
        for (; c <= hi; ++c) {
            if (br == a[c - 1]) {
                cur[c] = prev[c - 1];
            } else {
                uint32_t mi = prev[c - 1];
                if (mi > cur[c - 1]) mi = cur[c - 1];
                if (mi > prev[c]) mi = prev[c]; /* (prev[hi] is outside row r - 1's band when hi moved: INF) */
                cur[c] = mi + 1;
            }
        }
        cur[hi + 1] = INF;
        uint32_t *sw = prev;
        prev = cur;
        cur = sw;
    }
    const int64_t d = prev[la];
    free(prev);
    free(cur);
    return d <= (int64_t)t ? d : -2;
}
