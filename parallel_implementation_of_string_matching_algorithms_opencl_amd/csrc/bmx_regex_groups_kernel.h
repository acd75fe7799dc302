// bmx_regex_groups_kernel.h -- the capture groups of every span of a list (bmx_regex_groups_device, include/bmx.h,
// DESIGN.md s34).  No counterpart in the reference.  One list entry per lane, two sweeps over its span text[s..e],
// L = e - s + 1 <= max_len <= 64 bytes:
//
// Backward.  The starts pass's recurrence (bmx_regex_kernel.h) on the REVERSED automaton, anchored at text[e]:
//     D = (first' at the first step | Follow'(D)) & B'[c]
// After the step of text[s + t], D holds -- in reversed numbering -- exactly the positions that consume text[s + t] and
// from which the rest of the span can still be consumed, ending in `last` at e: the set B_t of the model.  The lane
// stores it, turned back to forward numbering (one bit reversal), as word t of its COLUMN in LDS.  The column of lane l
// is col[t * BLOCK + l]: consecutive lanes read consecutive words, so neither the stores nor the loads conflict, whatever
// t each lane stands at.  The span matches iff B_0 meets `first`.
//
// Forward.  cur = START; at byte t the candidates are follow[cur] & B_t (never empty on a matching span).  One candidate:
// that is the step.  Several: the first entry of pref[cur] among them (pref sits in LDS, a row is 64 bytes).  The two
// tag words of the pair (cur, next) come from the context's device block (65 x 65 words of {open, close << 16}, read
// through the vector cache) and are applied with compare-selects over 16 statically indexed begin and 16 end registers:
// no array a lane indexes by a run-time value, hence no scratch.  The boundary behind the last byte goes to END.
//
// Text comes as in the starts pass: aligned 8-byte words, downwards from the one that holds text[e], one word ahead; a
// word below text[0]'s 16-byte line is never loaded, and a skipped or invalid entry reads no byte.
#pragma once

#include "bmx_regex_kernel.h"

namespace bmx {

constexpr int REGEX_GROUPS_BLOCK = 256;
constexpr int REGEX_GROUPS_MAX = 16;                 // == BMX_MAX_REGEX_GROUPS
constexpr uint32_t REGEX_GROUPS_ROWS = 65;           // positions and START / END
constexpr uint64_t REGEX_GROUPS_BAD_SPAN = 1, REGEX_GROUPS_TOO_LONG = 2, REGEX_GROUPS_NO_MATCH = 4; // status bits (ws[0])

// The device block of a call: what the forward walk reads.
struct RegexGroupsBlock {
    uint64_t follow[REGEX_GROUPS_ROWS];                  // forward numbering; row 64: first
    uint32_t pref[REGEX_GROUPS_ROWS * 16];               // 64 bytes per row, most preferred first, then 0xFF
    uint32_t tags[REGEX_GROUPS_ROWS * REGEX_GROUPS_ROWS]; // [from * 65 + to]: open | close << 16
};

struct RegexGroupsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *starts, *ends;
    uint64_t count;
    uint64_t *groups;      // count * (n_groups + 1) pairs
    uint64_t *ws;          // [0]: status bits
    const RegexGroupsBlock *block;
    uint32_t max_len, m;
    uint32_t n_groups, pad;
    RegexSets k;           // of the REVERSED automaton
    uint64_t peq[256];     // bit i set: byte belongs to position m - 1 - i (low word used when m <= 32)
};

__device__ __forceinline__ uint32_t regex_groups_unreverse(uint32_t d, uint32_t m) { return __brev(d) >> (32 - m); }
__device__ __forceinline__ uint64_t regex_groups_unreverse(uint64_t d, uint32_t m) { return __brevll(d) >> (64 - m); }

template <typename W>
__global__ __launch_bounds__(REGEX_GROUPS_BLOCK) void regex_groups_kernel(const RegexGroupsArgs a)
{
    constexpr uint32_t NB = sizeof(W); // bytes of the word: one T_b table each
    __shared__ W peq[256];
    __shared__ W tt[NB * 256];
    __shared__ W ffollow[REGEX_GROUPS_ROWS];
    __shared__ uint32_t pref[REGEX_GROUPS_ROWS * 16];
    extern __shared__ __align__(8) uint8_t col_bytes[]; // max_len words per lane
    W *col = reinterpret_cast<W *>(col_bytes);
    const uint32_t tid = threadIdx.x;
    peq[tid] = (W)a.peq[tid]; // REGEX_GROUPS_BLOCK == 256
#pragma unroll 1
    for (uint32_t b = 0; b < NB; ++b) tt[256 * b + tid] = (W)regex_table_entry(a.k.follow, b, tid);
    if (tid < REGEX_GROUPS_ROWS) ffollow[tid] = (W)a.block->follow[tid];
    for (uint32_t w = tid; w < REGEX_GROUPS_ROWS * 16; w += REGEX_GROUPS_BLOCK) pref[w] = a.block->pref[w];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * REGEX_GROUPS_BLOCK + tid;
    if (i >= a.count) return;

    const uint32_t pairs = a.n_groups + 1;
    uint64_t *out = a.groups + i * pairs * 2;
    const uint64_t s_abs = a.starts[i], e_abs = a.ends[i];
    const bool skipped = s_abs == ~0ull || e_abs == ~0ull || e_abs < s_abs;
    const uint64_t j = e_abs - a.base;
    uint64_t bad = 0;
    if (!skipped) {
        if (s_abs < a.base || j >= a.n) bad = REGEX_GROUPS_BAD_SPAN;
        else if (e_abs - s_abs >= a.max_len) bad = REGEX_GROUPS_TOO_LONG;
    }
    if (skipped || bad) { // no byte is read for this entry
        if (bad) atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)bad);
        for (uint32_t g = 0; g < 2 * pairs; ++g) out[g] = ~0ull;
        return;
    }
    const uint32_t len = (uint32_t)(e_abs - s_abs) + 1; // 1..max_len

    // ---- backward: B_t for t = len - 1 .. 0 into the column ----
    const uint64_t q0 = a.first + j;
    int64_t wi = (int64_t)(q0 >> 3); // index of the 8-byte word that holds text[e], counted from text16
    const uint32_t b0 = (uint32_t)(q0 & 7);
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = words[wi];                  // text[e] is byte b0 of hi
    uint64_t lo = wi > 0 ? words[wi - 1] : 0; // word 0 lies in text[0]'s line: nothing below it is loaded
    const W lin = (W)a.k.lin, nl = (W)a.k.nl;
    const uint32_t nl_bytes = a.k.nl_bytes;
    W d = 0, seed = (W)a.k.first; // anchored at text[e]: `first` enters the first step only
    uint32_t done = 0;
    const uint32_t chunks = (len + 7) / 8;
    for (uint32_t c = 0; c < chunks; ++c) {
        // the next 8 bytes downwards from text[e - 8c], the first of them in the top byte
        const uint64_t cur = (hi << (8 * (7 - b0))) | ((lo >> (8 * b0)) >> 8);
        hi = lo;
        --wi;
        lo = wi > 0 ? words[wi - 1] : 0; // one word ahead of its use
        W eq[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) eq[t] = peq[(uint32_t)(cur >> (8 * (7 - t))) & 0xFFu];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            W f = (W)((d & lin) << 1) | seed;
            seed = 0;
            const W x = d & nl;
#pragma unroll
            for (uint32_t q = 0; q < NB; ++q)
                if ((nl_bytes >> q) & 1u) f |= tt[256 * q + ((uint32_t)(x >> (8 * q)) & 0xFFu)];
            d = f & eq[t];
            if (done < len) col[(len - 1 - done) * REGEX_GROUPS_BLOCK + tid] = regex_groups_unreverse(d, a.m); // (below max_len rows)
            ++done;
        }
    }

    // ---- forward: the preferred path and its tags ----
    uint32_t gb[REGEX_GROUPS_MAX], ge[REGEX_GROUPS_MAX]; // offsets from s, 0..len; 0xFF: unset
#pragma unroll
    for (int g = 0; g < REGEX_GROUPS_MAX; ++g) gb[g] = ge[g] = 0xFFu;
    uint32_t cur = REGEX_GROUPS_ROWS - 1; // START
    bool match = true;
    for (uint32_t t = 0; t <= len; ++t) {
        uint32_t nxt = REGEX_GROUPS_ROWS - 1; // END behind the last byte
        if (t < len) {
            const W cand = ffollow[cur] & col[t * REGEX_GROUPS_BLOCK + tid];
            if (cand == 0) { // only at t == 0: B_0 does not meet `first`
                match = false;
                break;
            }
            nxt = sizeof(W) == 8 ? (uint32_t)__builtin_ctzll((uint64_t)cand) : (uint32_t)__builtin_ctz((uint32_t)cand);
            if ((cand & (cand - 1)) != 0) { // several candidates: the first of the row among them
                for (uint32_t r = 0; r < 64; ++r) {
                    const uint32_t q = (pref[cur * 16 + (r >> 2)] >> (8 * (r & 3))) & 0xFFu;
                    if (q >= 64u) break; // (a valid row lists every candidate before its 0xFF)
                    if ((cand >> q) & 1) {
                        nxt = q;
                        break;
                    }
                }
            }
        }
        const uint32_t tags = a.block->tags[cur * REGEX_GROUPS_ROWS + nxt];
        if (tags != 0) {
#pragma unroll
            for (int g = 0; g < REGEX_GROUPS_MAX; ++g) {
                gb[g] = (tags >> g) & 1u ? t : gb[g];
                ge[g] = (tags >> (16 + g)) & 1u ? t : ge[g];
            }
        }
        cur = nxt;
    }
    if (!match) {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_GROUPS_NO_MATCH);
        for (uint32_t g = 0; g < 2 * pairs; ++g) out[g] = ~0ull;
        return;
    }
    out[0] = s_abs;
    out[1] = e_abs + 1;
#pragma unroll
    for (int g = 0; g < REGEX_GROUPS_MAX; ++g) {
        if ((uint32_t)g < a.n_groups) {
            const bool set = gb[g] != 0xFFu && ge[g] != 0xFFu;
            out[2 * g + 2] = set ? s_abs + gb[g] : ~0ull;
            out[2 * g + 3] = set ? s_abs + ge[g] : ~0ull;
        }
    }
}

} // namespace bmx
