// bmx_regex_long_kernel.h -- regular-expression search for automata of up to 128 positions (bmx_search_regex_long_device,
// bmx_regex_long_starts_device): bmx_regex_kernel.h's recurrence on a state of four dwords per lane.  Every END j of the
// view at which some text[s..j] matches is reported once, ascending.  No counterpart in the reference.
//
//     D = (first | Follow(D)) & B[c]            end j is a hit iff (D & last) != 0
//     Follow(D) = ((D & lin) << 1 over 128 bits) | OR over the bytes b of the 16 with nl != 0 there:  T_b[ byte b of (D & nl) ]
// Position i is bit (i & 31) of dword (i >> 5).  The shift carries from dword to dword with v_alignbit_b32, the test "does
// any lane of the wave stand on an irregular position" stands in front of the table reads, and which bytes have a table
// is a scalar branch, all as in the 64-bit step.
//
// What differs is where the tables live.  B is 256 x 16 bytes and follow[] 128 x 16 bytes, more than kernel arguments
// hold: the host writes both into a block of REGEX_LONG_BLOCK entries in device memory (B first, follow[] behind it) and
// the kernel gets the four sets, nl_bytes and a pointer to the block by value.  The workgroup copies B into LDS and builds
// the T_b tables behind it, 256 entries of 16 bytes each (one ds_read_b128 per read), COMPACTED: the table of byte b sits
// in slot popcount(nl_bytes below b), a scalar.  The kernel is instantiated for NT = 0, 7, 12 and 16 table slots, so an
// expression with three irregular bytes does not pay the LDS of sixteen; the host picks the smallest NT that holds the
// expression's tables.  The steps are where the workgroups per CU change: the frame's 17 KiB, B and NT tables of 4 KiB
// make 49 KiB at NT = 7 (three workgroups in the CU's 160 KiB, which is also what the registers allow), 69 KiB at 12
// (two) and 85 KiB at 16 (one).
//
// The walk is bmx_classes_kernel.h's (whole 128-byte lines per lane) with this state; a chunk gathers its B words eight at
// a time (sixteen of four dwords would be 64 registers) in front of their steps, and the head chunk of an unaligned view
// steps the bytes in front of the view with an empty B word.
//
// Starts (regex_long_starts_kernel): one list entry per lane, the REVERSED automaton against text[j], text[j - 1], ...
// for at most max_len bytes, `first` entering at the first step only, exactly as regex_starts_kernel; the same block and
// the same compacted tables.
#pragma once

#include "bmx_classes_kernel.h"

namespace bmx {

constexpr int MAX_REGEX_LONG_POSITIONS = 128; // == BMX_MAX_REGEX_LONG_POSITIONS
constexpr int REGEX_LONG_BLOCK = 256 + MAX_REGEX_LONG_POSITIONS; // entries of 16 bytes: B[256], then follow[128]
constexpr int REGEX_LONG_STARTS_BLOCK = 256;
constexpr uint64_t REGEX_LONG_BAD_END = 1, REGEX_LONG_BAD_START = 2; // status bits of the starts kernel (ws[0])

// The sets of the automaton, bit (i & 31) of component (i >> 5) = position i, and where its tables are.
struct RegexLongSets {
    tile_u32x4 first, last, lin, nl;
    uint32_t nl_bytes; // bit b: byte b of nl is non-zero (at most NT of them)
    uint32_t pad;
    const tile_u32x4 *block; // device memory: B[c] for c < 256, then follow[i] for i < 128
};

struct RegexLongState {
    tile_u32x4 d;
};

// byte b (0..15) of the 128-bit word x
__device__ __forceinline__ uint32_t regex_long_byte(tile_u32x4 x, uint32_t b)
{
    return __builtin_amdgcn_ubfe(x[b >> 2], 8 * (b & 3), 8);
}

// (l << 1) over 128 bits
__device__ __forceinline__ tile_u32x4 regex_long_shift1(tile_u32x4 l)
{
    tile_u32x4 f;
    f[0] = l[0] << 1;
    f[1] = __builtin_amdgcn_alignbit(l[1], l[0], 31);
    f[2] = __builtin_amdgcn_alignbit(l[2], l[1], 31);
    f[3] = __builtin_amdgcn_alignbit(l[3], l[2], 31);
    return f;
}

// Workgroup of 256 lanes: B into tab[0..256), behind it the compacted T_b tables, lane tid entry tid of each.  entry v of
// T_b: the OR of follow[8b + t] over the bits t of v.
template <int NT>
__device__ __forceinline__ void regex_long_fill(tile_u32x4 *tab, const RegexLongSets &k, uint32_t tid)
{
    tab[tid] = k.block[tid];
    if (NT > 0) {
        const tile_u32x4 *follow = k.block + 256;
        uint32_t slot = 0;
#pragma unroll 1
        for (uint32_t b = 0; b < 16; ++b) {
            if (!((k.nl_bytes >> b) & 1u)) continue; // (no table: never read)
            if (slot >= (uint32_t)NT) break;         // (the host never asks for more than NT)
            tile_u32x4 f = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t t = 0; t < 8; ++t)
                if ((tid >> t) & 1u) f |= follow[8 * b + t];
            tab[256 + 256 * slot + tid] = f;
            ++slot;
        }
    }
}

// Follow(D) | seed, with tt the compacted tables
template <int NT>
__device__ __forceinline__ tile_u32x4 regex_long_follow(const RegexLongSets &k, const tile_u32x4 *tt, tile_u32x4 d, tile_u32x4 seed,
                                                        bool wave_test)
{
    tile_u32x4 f = regex_long_shift1(d & k.lin) | seed;
    if (NT > 0) {
        const tile_u32x4 x = d & k.nl;
        // (search: some lane of the wave stands on an irregular position; starts: every lane reads)
        if (!wave_test || __builtin_amdgcn_ballot_w64((x[0] | x[1] | x[2] | x[3]) != 0) != 0) {
            uint32_t slot = 0;
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) {
                if ((k.nl_bytes >> b) & 1u) { // (the same for every lane of the grid)
                    f |= tt[256 * slot + regex_long_byte(x, b)];
                    ++slot;
                }
            }
        }
    }
    return f;
}

// One text byte on its B word.  Returns D & last, folded into one word.
template <int NT>
__device__ __forceinline__ uint32_t regex_long_step(const RegexLongSets &k, const tile_u32x4 *tt, RegexLongState &s, tile_u32x4 bw)
{
    s.d = regex_long_follow<NT>(k, tt, s.d, k.first, true) & bw;
    const tile_u32x4 h = s.d & k.last;
    return h[0] | h[1] | h[2] | h[3];
}

// One 16-byte chunk: two rounds of gather eight B words, then their eight steps.  Returns the hit bits, bit i = byte i.
template <int NT>
__device__ __forceinline__ uint32_t regex_long_chunk(const tile_u32x4 *tab, const RegexLongSets &k, RegexLongState &s, tile_u32x4 v)
{
    const tile_u32x4 *tt = tab + 256;
    uint32_t hits = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        tile_u32x4 bw[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) bw[i] = tab[regex_long_byte(v, 8 * half + i)];
#pragma unroll
        for (int i = 0; i < 8; ++i) hits |= (regex_long_step<NT>(k, tt, s, bw[i]) != 0 ? 1u : 0u) << (8 * half + i);
    }
    return hits;
}

// The chunk that holds view byte 0 when the view does not begin on a 16-byte line: its first `skip` bytes lie in front of
// the view and are stepped with an empty B word, which leaves D = 0.  One chunk per call, so a plain loop.
template <int NT>
__device__ __forceinline__ uint32_t regex_long_chunk_head(const tile_u32x4 *tab, const RegexLongSets &k, RegexLongState &s, tile_u32x4 v,
                                                          uint32_t skip)
{
    const tile_u32x4 *tt = tab + 256;
    uint32_t hits = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t byte = v[0] & 0xFFu;
        v[0] = __builtin_amdgcn_alignbit(v[1], v[0], 8);
        v[1] = __builtin_amdgcn_alignbit(v[2], v[1], 8);
        v[2] = __builtin_amdgcn_alignbit(v[3], v[2], 8);
        v[3] >>= 8;
        tile_u32x4 bw = tab[byte];
        if (i < skip) bw = tile_u32x4{0, 0, 0, 0};
        hits |= (regex_long_step<NT>(k, tt, s, bw) != 0 ? 1u : 0u) << i;
    }
    return hits;
}

// The step for the shared walk: the head chunk where bytes lie in front of the view, the unrolled one everywhere else.
template <int NT>
struct RegexLongStep {
    const RegexLongSets &k;
    __device__ __forceinline__ explicit RegexLongStep(const RegexLongSets &sets) : k(sets) {}
    __device__ __forceinline__ uint32_t chunk(const tile_u32x4 *tab, RegexLongState &s, tile_u32x4 v, uint32_t skip) const
    {
        return skip != 0 ? regex_long_chunk_head<NT>(tab, k, s, v, skip) : regex_long_chunk<NT>(tab, k, s, v);
    }
};

// The frame's policy: B, then NT table slots, all of 16-byte entries; TileArgs::peq is not used.
template <int NT>
struct RegexLongPolicy {
    typedef tile_u32x4 Elem;
    static constexpr bool FILL_TAKES_X = true;
    static constexpr int TAB = 256 + 256 * NT;
    static __device__ __forceinline__ void fill(tile_u32x4 *tab, const TileArgs &, uint32_t tid, const RegexLongSets &k)
    {
        regex_long_fill<NT>(tab, k, tid); // TILE_BLOCK == 256
    }
    template <int PASS>
    static __device__ __forceinline__ uint32_t walk(const TileArgs &a, const tile_u32x4 *tab, uint64_t lo, uint64_t hi, uint64_t tile0,
                                                    uint64_t *stage, uint32_t *stage_n, uint64_t base, const RegexLongSets &k)
    {
        return shift_and_walk_state<RegexLongState, PASS>(a, RegexLongStep<NT>(k), tab, lo, hi, tile0, stage, stage_n, base);
    }
    static __device__ __forceinline__ uint32_t ordinal(uint64_t e) { return (uint32_t)(e >> 32); }
    static __device__ __forceinline__ void also(const TileArgs &, uint64_t, uint64_t) {}
};

struct RegexLongStartsArgs {
    const uint8_t *text16; // the 16-byte line that holds text[0]
    uint64_t first;        // text[0] is text16[first]
    uint64_t n, base;
    const uint64_t *ends;
    uint64_t count;
    uint64_t *starts;
    uint64_t *ws;          // [0]: status bits
    uint32_t max_len, chunks; // chunks = ceil(max_len / 8)
    uint32_t longest, pad;
    RegexLongSets k;       // of the REVERSED automaton (its block: bit i of B[c] says that c belongs to position m - 1 - i)
};

template <int NT>
__global__ __launch_bounds__(REGEX_LONG_STARTS_BLOCK) void regex_long_starts_kernel(const RegexLongStartsArgs a)
{
    __shared__ tile_u32x4 tab[256 + 256 * NT];
    const uint32_t tid = threadIdx.x;
    regex_long_fill<NT>(tab, a.k, tid); // REGEX_LONG_STARTS_BLOCK == 256
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * REGEX_LONG_STARTS_BLOCK + tid;
    if (i >= a.count) return;

    const uint64_t e = a.ends[i];
    const uint64_t j = e - a.base;
    const bool valid = e >= a.base && j < a.n;
    uint32_t steps = 0, b = 0;
    int64_t wi = -1; // index of the 8-byte word that holds text[j], counted from text16
    if (valid) {
        steps = (uint32_t)min(j + 1, (uint64_t)a.max_len); // the window is clipped at text[0]
        const uint64_t q = a.first + j;
        wi = (int64_t)(q >> 3);
        b = (uint32_t)(q & 7);
    } else {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_LONG_BAD_END); // no byte is read for this entry
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(a.text16);
    uint64_t hi = valid ? words[wi] : 0;               // text[j] is byte b of hi
    uint64_t lo = valid && wi > 0 ? words[wi - 1] : 0; // word 0 lies in text[0]'s line: nothing below it is loaded

    const tile_u32x4 *tt = tab + 256;
    tile_u32x4 d = {0, 0, 0, 0}, seed = a.k.first; // anchored at text[j]: `first` enters the first step only
    uint32_t first_len = 0, last_len = 0, len = 0;
    for (uint32_t c = 0; c < a.chunks; ++c) {
        // the next 8 bytes downwards from text[j - 8c], the first of them in the top byte
        const uint64_t cur = (hi << (8 * (7 - b))) | ((lo >> (8 * b)) >> 8);
        hi = lo;
        --wi;
        lo = valid && wi > 0 ? words[wi - 1] : 0; // one word ahead of its use
        tile_u32x4 eq[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) eq[t] = tab[(uint32_t)(cur >> (8 * (7 - t))) & 0xFFu];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            d = regex_long_follow<NT>(a.k, tt, d, seed, false) & eq[t];
            seed = tile_u32x4{0, 0, 0, 0};
            ++len;
            const tile_u32x4 h = d & a.k.last;
            if (len <= steps && (h[0] | h[1] | h[2] | h[3]) != 0) { // text[j - len + 1 .. j] matches
                if (first_len == 0) first_len = len;
                last_len = len;
            }
        }
    }
    if (!valid) return;
    if (first_len == 0) {
        atomicOr((unsigned long long *)&a.ws[0], (unsigned long long)REGEX_LONG_BAD_START);
        a.starts[i] = e;
        return;
    }
    a.starts[i] = e - ((a.longest ? last_len : first_len) - 1);
}

} // namespace bmx
