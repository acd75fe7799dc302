// bmx_ed_batch_kernel.h -- batched edit distance (bmx_edit_distance_batch_device): one string pair per lane.
//
// The recurrence is Myers' bit-parallel column update (J. ACM 46(3), 1999) in its GLOBAL form (Hyyro's statement of it):
// row 0 of the table is not free, so a 1 enters bit 0 of the shifted Ph, the score starts at the pattern length and the
// answer is the score after the last text byte.  bmx_approx_kernel.h holds the search form of the same step.  The
// reference's relative is the anti-diagonal DP of EditDistance-1/EditDistance-1/kernal.cl:5-56, set up again per pair
// by EditDistance-1.cpp:278-345.
//
// Geometry.  Lane i of the grid owns pair i.  It reads and checks its four offsets, answers the pairs
// that need no byte (an empty side, a length difference above the limit), lists the pairs the kernel does not cover
// (both sides over ED_BATCH_WORD bytes, or a longer side over ED_BATCH_LONG) for the host's pair-by-pair path, and
// otherwise makes the SHORTER string the bit vector and walks the longer one, 16 bytes per load.  A wave runs the
// 64-bit word only if one of its lanes has a bit vector of more than 32 bytes.
//
// Eq words, pairwise: built on the fly from the pattern, which stays in 8 (16) VGPRs with byte 8k + j of each half in
// byte k of register j (16-byte loads and a byte transpose, ed_batch_load_pattern).  XOR with the text byte replicated four times, an exact zero-byte test (no borrow between
// bytes) and a shift by 7 - j put the 32 flags of a half straight on their bit positions: 7 VALU per register and
// byte, no LDS, no table to clear between pairs.  The 16 Eq words of a chunk are computed before its 16 dependent
// steps (what bmx_approx_kernel.h does not do).
// Eq words, one against many (a_count == 1, query of 1..ED_BATCH_WORD bytes): ONE 256-word Peq in LDS, built by the
// workgroup from the query; a chunk's 16 words are gathered before its steps, and every lane walks its own b[i]
// whatever its length.
//
// BMX_ED_BATCH_PIECES_ONLY (tests/ed_batch_check.hip): a --cuda-host-only build gets the lane functions (ed_batch_step,
// ed_batch_load_pattern, ed_batch_walk) as host code, with host stand-ins for the two device builtins, and no kernel.
// Without the switch the macros below are the builtins and the qualifiers themselves: the device build is unchanged.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmx_eq_kernel.h"

#ifdef BMX_ED_BATCH_PIECES_ONLY
#define BMX_ED_BATCH_LANE static inline
// v_perm_b32(hi, lo, sel): byte i of the result is chosen by byte i of sel: 0..3 that byte of lo, 4..7 of hi, 8..11 the
// sign (bit 15 / 31) of lo / hi spread over the byte, 12 zero, 13 and above 0xff.
static inline uint32_t bmx_ed_batch_host_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 0xffu;
        uint32_t b;
        if (s < 8) b = (uint32_t)(src >> (8 * s)) & 0xffu;
        else if (s < 12) b = ((src >> (16 * (s - 8) + 15)) & 1) ? 0xffu : 0u;
        else b = s == 12 ? 0u : 0xffu;
        r |= b << (8 * i);
    }
    return r;
}
// v_bfe_u32: `width` bits of src from bit `offset` (both taken modulo 32)
static inline uint32_t bmx_ed_batch_host_ubfe(uint32_t src, uint32_t offset, uint32_t width)
{
    offset &= 31u, width &= 31u;
    return width == 0 ? 0u : (src >> offset) & (0xffffffffu >> (32u - width));
}
#define BMX_ED_BATCH_PERM(hi, lo, sel) bmx_ed_batch_host_perm(hi, lo, sel)
#define BMX_ED_BATCH_UBFE(src, offset, width) bmx_ed_batch_host_ubfe(src, offset, width)
#else
#define BMX_ED_BATCH_LANE __device__ __forceinline__
#define BMX_ED_BATCH_PERM(hi, lo, sel) __builtin_amdgcn_perm(hi, lo, sel)
#define BMX_ED_BATCH_UBFE(src, offset, width) __builtin_amdgcn_ubfe(src, offset, width)
#endif

namespace bmx {

constexpr int ED_BATCH_BLOCK = 256;          // lanes (pairs) per workgroup
constexpr uint32_t ED_BATCH_WORD = 64;       // == BMX_ED_BATCH_WORD
constexpr uint32_t ED_BATCH_LONG = 65536;    // == BMX_ED_BATCH_LONG: longest walk of a pairwise lane
constexpr uint32_t ED_BATCH_NO_LIMIT = 0xFFFFFFFFu;
constexpr int ED_BATCH_LIST_WORDS = 5;       // a listed pair: {index, a offset, a length, b offset, b length}

struct EdBatchArgs {
    const uint8_t *a, *b;
    const uint64_t *a_off, *b_off;
    uint64_t a_bytes, b_bytes, count;
    uint32_t one;   // a_count == 1: every pair takes a[0]
    uint32_t limit; // ED_BATCH_NO_LIMIT: none
    uint32_t *dist;
    uint64_t *ws;   // [0] set by a lane with bad offsets, [1] pairs for the pair-by-pair path
    uint64_t *list; // the first list_cap of them
    uint64_t list_cap;
};

typedef uint32_t ed_batch_u32x4 __attribute__((ext_vector_type(4)));

template <typename W>
struct EdBatchState {
    W pv, mv;
    uint32_t score;
};

template <typename W>
BMX_ED_BATCH_LANE void ed_batch_step(EdBatchState<W> &s, W eq, uint32_t hb)
{
    const W xv = eq | s.mv;
    const W xh = (((eq & s.pv) + s.pv) ^ s.pv) | eq;
    W ph = s.mv | ~(xh | s.pv);
    W mh = s.pv & xh;
    s.score += (uint32_t)((ph >> hb) & 1) - (uint32_t)((mh >> hb) & 1);
    ph = (ph << 1) | 1; // row 0 is not free: D[0][j] - D[0][j-1] = +1
    mh <<= 1;
    s.pv = mh | ~(xv | ph);
    s.mv = ph & xv;
}

// The pattern into its registers: byte 8k + j of a 32-byte half -> byte k of register j.  The bytes come in 16-byte loads
// at the pattern's own alignment (one to four global_load_dwordx4 per pair) and a 4 x 4 byte transpose (v_perm_b32, 16 per
// half) puts them in place.  A load may run past the pattern into the next string of the blob: those bytes only reach
// Eq bits at or above m, which the mask clears.  It never runs past the blob (`end`): a chunk that would end past
// `end` comes byte by byte, its bytes below m only.  That is any pattern whose last chunk starts fewer than 16 bytes before
// the blob's end (the blob's last pattern, and those before it that are as close), and only a pattern's LAST chunk: an
// earlier chunk holds 16 pattern bytes, all inside the blob.
template <int ND>
BMX_ED_BATCH_LANE void ed_batch_load_pattern(uint32_t *p, const uint8_t *P, uint32_t m, const uint8_t *end)
{
    uint32_t d[ND];
#pragma unroll
    for (int c = 0; c < ND / 4; ++c) {
        ed_batch_u32x4 v = {0u, 0u, 0u, 0u};
        if ((uint32_t)(16 * c) < m) {
            if (P + 16 * c + 16 <= end) {
                __builtin_memcpy(&v, P + 16 * c, 16);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((uint32_t)(16 * c + k) < m) v[k >> 2] |= (uint32_t)P[16 * c + k] << (8 * (k & 3));
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) d[4 * c + k] = v[k];
    }
#pragma unroll
    for (int h = 0; h < ND / 8; ++h) // a half: dwords d[8h .. 8h + 8)
#pragma unroll
        for (int q = 0; q < 2; ++q) { // registers 4q .. 4q + 3 take the bytes of dwords q, 2 + q, 4 + q, 6 + q
            const uint32_t x0 = d[8 * h + q], x1 = d[8 * h + 2 + q], x2 = d[8 * h + 4 + q], x3 = d[8 * h + 6 + q];
            // v_perm_b32(hi, lo, sel): selector byte 0..3 takes that byte of lo, 4..7 of hi
            const uint32_t t0 = BMX_ED_BATCH_PERM(x1, x0, 0x05010400u), t1 = BMX_ED_BATCH_PERM(x1, x0, 0x07030602u);
            const uint32_t u0 = BMX_ED_BATCH_PERM(x3, x2, 0x05010400u), u1 = BMX_ED_BATCH_PERM(x3, x2, 0x07030602u);
            p[8 * h + 4 * q + 0] = BMX_ED_BATCH_PERM(u0, t0, 0x05040100u);
            p[8 * h + 4 * q + 1] = BMX_ED_BATCH_PERM(u0, t0, 0x07060302u);
            p[8 * h + 4 * q + 2] = BMX_ED_BATCH_PERM(u1, t1, 0x05040100u);
            p[8 * h + 4 * q + 3] = BMX_ED_BATCH_PERM(u1, t1, 0x07060302u);
        }
}

// One lane: the distance of P[0..m) and T[0..n), 1 <= m <= bits of W, n >= 1.  SHARED: Eq from the workgroup's Peq (built
// from P), else from P in registers (P_end: the end of P's blob).  Reads T[0..n) only: full 16-byte chunks of T, then its
// last bytes singly.
template <typename W, bool SHARED>
BMX_ED_BATCH_LANE uint32_t ed_batch_walk(const uint8_t *P, uint32_t m, const uint8_t *P_end, const uint8_t *T, uint32_t n,
                                         const uint64_t *peq)
{
    constexpr int ND = sizeof(W) == 4 ? 8 : 16;
    uint32_t p[ND];
    if (!SHARED) ed_batch_load_pattern<ND>(p, P, m, P_end);
    const W mask = m >= 8 * sizeof(W) ? ~(W)0 : (((W)1 << m) - 1);
    const uint32_t hb = m - 1;
    EdBatchState<W> s;
    s.pv = ~(W)0;
    s.mv = 0;
    s.score = m;
    uint32_t pos = 0;
    for (; pos + 16 <= n; pos += 16) {
        ed_batch_u32x4 v;
        __builtin_memcpy(&v, T + pos, 16);
        W eq[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { // all of the chunk's Eq words first
            if (SHARED) {
                eq[i] = (W)peq[BMX_ED_BATCH_UBFE(v[i >> 2], 8 * (i & 3), 8)];
            } else {
                const uint32_t c4 = BMX_ED_BATCH_PERM(v[i >> 2], v[i >> 2], 0x01010101u * (uint32_t)(i & 3));
                eq[i] = ed_batch_eq<W>(p, c4, mask);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) ed_batch_step<W>(s, eq[i], hb);
    }
    for (; pos < n; ++pos) {
        const uint32_t c = T[pos];
        const W eq = SHARED ? (W)peq[c] : ed_batch_eq<W>(p, c * 0x01010101u, mask);
        ed_batch_step<W>(s, eq, hb);
    }
    return s.score;
}

#ifndef BMX_ED_BATCH_PIECES_ONLY // (tests/ed_batch_check.hip builds for the host alone: the pieces above, no kernel)

__global__ __launch_bounds__(ED_BATCH_BLOCK) void ed_batch_kernel(const EdBatchArgs a)
{
    __shared__ uint64_t peq[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * ED_BATCH_BLOCK + tid;

    // one against many: the query's offsets are the same two words for every lane
    uint64_t q0 = 0, q1 = 0;
    bool q_ok = true, shared = false;
    if (a.one) {
        q0 = a.a_off[0];
        q1 = a.a_off[1];
        q_ok = q1 >= q0 && q1 <= a.a_bytes && q1 - q0 < (1ull << 31);
        shared = q_ok && q1 - q0 >= 1 && q1 - q0 <= ED_BATCH_WORD;
        if (shared) { // (uniform over the grid)
            peq[tid] = 0; // ED_BATCH_BLOCK == 256
            __syncthreads();
            if (tid < (uint32_t)(q1 - q0)) atomicOr((unsigned long long *)&peq[a.a[q0 + tid]], 1ull << tid);
            __syncthreads();
        }
    }

    bool walk = false;
    const uint8_t *P = nullptr, *P_end = nullptr, *T = nullptr;
    uint32_t m = 0, n = 0;
    if (i < a.count) {
        const uint64_t b0 = a.b_off[i], b1 = a.b_off[i + 1];
        const uint64_t a0 = a.one ? q0 : a.a_off[i], a1 = a.one ? q1 : a.a_off[i + 1];
        const bool ok = q_ok && a1 >= a0 && a1 <= a.a_bytes && a1 - a0 < (1ull << 31) && b1 >= b0 && b1 <= a.b_bytes &&
                        b1 - b0 < (1ull << 31);
        if (!ok) { // no string byte is read; the call returns BMX_ERR_ARG
            atomicOr((unsigned long long *)&a.ws[0], 1ull);
        } else {
            const uint32_t la = (uint32_t)(a1 - a0), lb = (uint32_t)(b1 - b0);
            const uint32_t lo = min(la, lb), hi = max(la, lb);
            if (a.limit != ED_BATCH_NO_LIMIT && hi - lo > a.limit) {
                a.dist[i] = a.limit + 1; // the distance is at least the length difference
            } else if (lo == 0) {
                a.dist[i] = hi; // (<= limit here)
            } else if (shared) {
                walk = true;
                m = la;
                T = a.b + b0;
                n = lb;
            } else if (lo > ED_BATCH_WORD || hi > ED_BATCH_LONG) {
                const uint64_t slot = atomicAdd((unsigned long long *)&a.ws[1], 1ull);
                if (slot < a.list_cap) {
                    uint64_t *e = a.list + slot * ED_BATCH_LIST_WORDS;
                    e[0] = i, e[1] = a0, e[2] = la, e[3] = b0, e[4] = lb;
                }
            } else {
                walk = true;
                const bool a_short = la <= lb; // the distance is symmetric
                P = a_short ? a.a + a0 : a.b + b0;
                P_end = a_short ? a.a + a.a_bytes : a.b + a.b_bytes;
                T = a_short ? a.b + b0 : a.a + a0;
                m = lo;
                n = hi;
            }
        }
    }
    const bool wide = __ballot(walk && m > 32) != 0; // per wave
    if (walk) {
        uint32_t d;
        if (shared)
            d = wide ? ed_batch_walk<uint64_t, true>(P, m, P_end, T, n, peq) : ed_batch_walk<uint32_t, true>(P, m, P_end, T, n, peq);
        else
            d = wide ? ed_batch_walk<uint64_t, false>(P, m, P_end, T, n, peq) : ed_batch_walk<uint32_t, false>(P, m, P_end, T, n, peq);
        a.dist[i] = a.limit != ED_BATCH_NO_LIMIT ? min(d, a.limit + 1) : d;
    }
}

// The pair-by-pair path's answers, to their places: dist[list[j].index] = vals[j].
__global__ void ed_batch_scatter_kernel(const uint64_t *list, const uint32_t *vals, uint64_t n, uint32_t *dist)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dist[list[j * ED_BATCH_LIST_WORDS]] = vals[j];
}

#endif // BMX_ED_BATCH_PIECES_ONLY

} // namespace bmx
