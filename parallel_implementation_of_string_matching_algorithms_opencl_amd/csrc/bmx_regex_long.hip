// bmx_regex_long.hip -- host side of the regular-expression search for automata of up to 128 positions
// (bmx_search_regex_long_device, bmx_regex_long_starts_device, include/bmx.h): builds the Shift-And table of the classes
// and follow[] into a pinned staging block of the state, the sets of the recurrence (lin, nl, the bytes of the word that
// hold an irregular position) beside it, copies the block to the state's device buffer on the caller's stream in front of
// the launch, picks the kernel by the number of follow tables (0, up to 7, up to 12, up to 16) and the lane piece, and
// launches bmx_regex_long_kernel.h's policy through the tile frame (bmx_tile_frame.h); for the starts it builds the same
// for the reversed automaton and launches one lane per list entry.  A call returns only after synchronising the stream, so
// one staging block and one device block serve both passes.  The argument checks and the context are the shim's
// (bmx_shim.hip); everything here runs on a valid context with a valid automaton.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_regex_long_kernel.h"

static_assert(bmx::MAX_REGEX_LONG_POSITIONS == BMX_MAX_REGEX_LONG_POSITIONS, "header and kernel disagree");
static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::RegexLongSets) <= 4096 && sizeof(bmx::RegexLongStartsArgs) <= 4096, "kernel arguments");
static_assert(sizeof(bmx_set128) == sizeof(bmx::tile_u32x4), "one entry of the block");

namespace {

constexpr const char *WHERE = "bmx_search_regex_long_device";
constexpr const char *WHERE_STARTS = "bmx_regex_long_starts_device";
constexpr size_t BLOCK_BYTES = (size_t)bmx::REGEX_LONG_BLOCK * sizeof(bmx_set128);

struct RegexLongState {
    bmx::TileState tile; // (first: bmx_tile_frame.h)
    uint64_t *d_ws = nullptr; // the starts pass: its status word ...
    uint64_t *h_ws = nullptr; // ... and the pinned copy of it
    bmx_set128 *h_block = nullptr; // B[256] and follow[128] of the call's automaton, pinned: valid until the call's last synchronise
    void *d_block = nullptr;       // ... and where the kernels read them
};
static_assert(offsetof(RegexLongState, tile) == 0, "tile_state, ordered_set_seq");

int block_ready(const char *where, RegexLongState *st, char *err, size_t errlen)
{
    if (!st->h_block) BMX_HIP(where, hipHostMalloc(reinterpret_cast<void **>(&st->h_block), BLOCK_BYTES, hipHostMallocDefault));
    if (!st->d_block) BMX_HIP(where, hipMalloc(&st->d_block, BLOCK_BYTES));
    return BMX_OK;
}

bmx::tile_u32x4 dwords(bmx_set128 s)
{
    bmx::tile_u32x4 v;
    for (int q = 0; q < 4; ++q) v[q] = (uint32_t)(s >> (32 * q));
    return v;
}

// The block (B, follow) and the sets of m positions as the kernels want them; *slot: the kernel's table class.
bmx::RegexLongSets regex_long_sets(int32_t m, bmx_set128 first, bmx_set128 last, const bmx_set128 *follow, const uint8_t *classes,
                                   bmx_set128 *h_block, const void *d_block, int *slot)
{
    std::memset(h_block, 0, BLOCK_BYTES);
    for (int32_t i = 0; i < m; ++i) {
        const uint8_t *cls = classes + (size_t)i * BMX_CLASS_BYTES;
        for (uint32_t c = 0; c < 256; ++c)
            if ((cls[c >> 3] >> (c & 7)) & 1u) h_block[c] |= (bmx_set128)1 << i; // bit i: the byte is in class i
        h_block[256 + i] = follow[i];
    }
    bmx_set128 lin, nl;
    bmx_regex_lin_nl_t<bmx_set128>(m, follow, &lin, &nl);
    bmx::RegexLongSets k;
    std::memset(&k, 0, sizeof k);
    k.first = dwords(first);
    k.last = dwords(last);
    k.lin = dwords(lin);
    k.nl = dwords(nl);
    for (uint32_t b = 0; b < 16; ++b)
        if ((uint32_t)(nl >> (8 * b)) & 0xFFu) k.nl_bytes |= 1u << b;
    k.block = static_cast<const bmx::tile_u32x4 *>(d_block);
    const int tables = __builtin_popcount(k.nl_bytes);
    *slot = tables == 0 ? 0 : tables <= 7 ? 1 : tables <= 12 ? 2 : 3; // (NT = 0, 7, 12, 16: bmx_regex_long_kernel.h)
    return k;
}

} // namespace

void bmx_internal_regex_long_free(void *state_v)
{
    RegexLongState *st = static_cast<RegexLongState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    if (st->d_block) (void)hipFree(st->d_block);
    if (st->h_block) (void)hipHostFree(st->h_block);
    delete st;
}

float bmx_internal_regex_long_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_regex_long(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                            const bmx_regex_long *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, hipStream_t stream,
                            char *err, size_t errlen)
{
    RegexLongState *st = bmx::tile_state<RegexLongState>(state_v, n_matches);
    if (lead >= n) return BMX_OK; // no end is owned (before anything is put on `stream`)
    bmx_regex_long_sets s;
    bmx_regex_long_load(re, &s);
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths_t<bmx_set128>(s.m, s.first, s.last, s.follow, &min_len, &max_len); // (the struct's fields are not read)
    if (max_len == 0) return BMX_OK; // no path from first to last: nothing can match
    const int rc = block_ready(WHERE, st, err, errlen);
    if (rc != BMX_OK) return rc;
    int slot = 0;
    const bmx::RegexLongSets k = regex_long_sets(s.m, s.first, s.last, s.follow, re->classes, st->h_block, st->d_block, &slot);
    BMX_HIP(WHERE, hipMemcpyAsync(st->d_block, st->h_block, BLOCK_BYTES, hipMemcpyHostToDevice, stream));
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexLongSets);
    static const Kernel kernels[4] = {
        bmx::tile_kernel<bmx::RegexLongPolicy<0>, bmx::RegexLongSets>, bmx::tile_kernel<bmx::RegexLongPolicy<7>, bmx::RegexLongSets>,
        bmx::tile_kernel<bmx::RegexLongPolicy<12>, bmx::RegexLongSets>, bmx::tile_kernel<bmx::RegexLongPolicy<16>, bmx::RegexLongSets>};
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a); // (peq stays empty: the table travels in the block)
    a.m = (uint32_t)s.m;
    a.warm = (uint32_t)max_len - 1;
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n - lead, max_len, resident); };
    const int lrc = bmx::tile_launch(&st->tile, WHERE, kernels[slot], slot, num_cu, a, d_text, n, lead, base_offset, piece, d_ends,
                                     capacity, n_matches, stream, err, errlen, k);
    if (lrc == BMX_ERR_HIP) (void)hipStreamSynchronize(stream); // (a launch that never got to its own wait: the copy may still read the block)
    return lrc;
}

// count >= 1: d_starts[i] for d_ends[i]; a lane walks max_len bytes of the reversed automaton.
int bmx_internal_regex_long_starts(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex_long *re,
                                   const uint64_t *d_ends, uint64_t count, uint32_t flags, uint64_t *d_starts, hipStream_t stream,
                                   char *err, size_t errlen)
{
    if (!*state_v) *state_v = new RegexLongState();
    RegexLongState *st = static_cast<RegexLongState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::REGEX_LONG_STARTS_BLOCK - 1) / bmx::REGEX_LONG_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_regex_long_starts_device: more than 2^31 workgroups of list entries in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_STARTS, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_STARTS, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    const int rc = block_ready(WHERE_STARTS, st, err, errlen);
    if (rc != BMX_OK) return rc;
    BMX_HIP(WHERE_STARTS, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call

    bmx_regex_long_sets s;
    bmx_regex_long_load(re, &s);
    const int32_t m = s.m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths_t<bmx_set128>(m, s.first, s.last, s.follow, &min_len, &max_len);
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::RegexLongStartsArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.n = n;
    a.base = base_offset;
    a.ends = d_ends;
    a.count = count;
    a.starts = d_starts;
    a.ws = st->d_ws;
    a.max_len = (uint32_t)max_len; // (0: no entry can be an end of a match, and every valid one raises the status word)
    a.chunks = (uint32_t)(max_len + 7) / 8;
    a.longest = (flags & BMX_REGEX_LONGEST) ? 1u : 0u;
    // the REVERSED automaton: bit i stands for position m - 1 - i, first and last swap, follow is transposed
    bmx_regex_long_sets rev;
    uint8_t rev_classes[BMX_MAX_REGEX_LONG_POSITIONS * BMX_CLASS_BYTES];
    rev.m = m;
    bmx_regex_reverse_t<bmx_set128>(m, s.first, s.last, s.follow, re->classes, &rev.first, &rev.last, rev.follow, rev_classes);
    int slot = 0;
    a.k = regex_long_sets(m, rev.first, rev.last, rev.follow, rev_classes, st->h_block, st->d_block, &slot);
    BMX_HIP(WHERE_STARTS, hipMemcpyAsync(st->d_block, st->h_block, BLOCK_BYTES, hipMemcpyHostToDevice, stream));
    typedef void (*Kernel)(const bmx::RegexLongStartsArgs);
    static const Kernel kernels[4] = {bmx::regex_long_starts_kernel<0>, bmx::regex_long_starts_kernel<7>, bmx::regex_long_starts_kernel<12>,
                                      bmx::regex_long_starts_kernel<16>};
    hipLaunchKernelGGL(kernels[slot], dim3((uint32_t)n_blocks), dim3(bmx::REGEX_LONG_STARTS_BLOCK), 0, stream, a);
    BMX_HIP(WHERE_STARTS, hipGetLastError());
    BMX_HIP(WHERE_STARTS, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_STARTS, hipStreamSynchronize(stream));

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "bmx_regex_long_starts_device: %s%s", bad & bmx::REGEX_LONG_BAD_END ? "an end outside the view; " : "",
                 bad & bmx::REGEX_LONG_BAD_START ? "an end at which no match of this expression ends; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}
