// bmx_regex.hip -- host side of the regular-expression search (bmx_search_regex_device, bmx_regex_starts_device,
// include/bmx.h): builds the Shift-And table of the classes and the sets of the recurrence (lin, nl, the bytes of the
// word that hold an irregular position) from the automaton, picks the word width, the kernel with or without the follow
// tables and the lane piece, and launches bmx_regex_kernel.h's policy through the tile frame (bmx_tile_frame.h: state,
// geometry, the ordered-output call around the launch); for the starts it builds the same for the reversed automaton
// and launches one lane per list entry.  Behind them the mirror image (bmx_search_regex_begins_device,
// bmx_regex_ends_device; bmx_regex_begins_kernel.h): the reversed automaton through the tile frame in start coordinates,
// with a state of its own, and the automaton as given, one lane per start of a list.  The argument checks and the context are the shim's (bmx_shim.hip); everything
// here runs on a valid context with a valid automaton.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_regex_begins_kernel.h"
#include "bmx_regex_kernel.h"

static_assert(bmx::MAX_REGEX_POSITIONS == BMX_MAX_REGEX_POSITIONS, "header and kernel disagree");
static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::RegexSets) <= 4096 && sizeof(bmx::RegexStartsArgs) <= 4096, "kernel arguments");
static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::RegexSets) + 8 <= 4096 && sizeof(bmx::RegexEndsArgs) <= 4096, "kernel arguments");

namespace {

constexpr const char *WHERE = "bmx_search_regex_device";
constexpr const char *WHERE_STARTS = "bmx_regex_starts_device";

struct RegexState {
    bmx::TileState tile; // (first: bmx_tile_frame.h)
    uint64_t *d_ws = nullptr; // the starts pass: its status word ...
    uint64_t *h_ws = nullptr; // ... and the pinned copy of it
};
static_assert(offsetof(RegexState, tile) == 0, "tile_state, ordered_set_seq");

// first, last and follow[0..m) as the kernel wants them: lin = the positions whose only successor is the next one, nl =
// the other positions with a successor, and which bytes of the word nl touches
bmx::RegexSets regex_sets(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow)
{
    bmx::RegexSets k;
    std::memset(&k, 0, sizeof k);
    k.first = first;
    k.last = last;
    for (int32_t i = 0; i < m; ++i) {
        k.follow[i] = follow[i];
        if (follow[i] == 0) continue;
        if (i < 63 && follow[i] == (1ull << (i + 1))) k.lin |= 1ull << i;
        else k.nl |= 1ull << i;
    }
    for (uint32_t b = 0; b < 8; ++b)
        if ((k.nl >> (8 * b)) & 0xFFu) k.nl_bytes |= 1u << b;
    return k;
}

} // namespace

void bmx_internal_regex_free(void *state_v)
{
    RegexState *st = static_cast<RegexState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    delete st;
}

float bmx_internal_regex_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_regex(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                       const bmx_regex *re, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, hipStream_t stream,
                       char *err, size_t errlen)
{
    RegexState *st = bmx::tile_state<RegexState>(state_v, n_matches);
    if (lead >= n) return BMX_OK; // no end is owned (before anything is put on `stream`)
    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len); // (the struct's fields are not read)
    if (max_len == 0) return BMX_OK; // no path from first to last: nothing can match
    const bmx::RegexSets k = regex_sets(m, re->first, re->last, re->follow);
    const bool wide = m > 32, nl = k.nl != 0;
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexSets);
    static const Kernel kernels[4] = {
        bmx::tile_kernel<bmx::RegexPolicy<false, false>, bmx::RegexSets>, bmx::tile_kernel<bmx::RegexPolicy<true, false>, bmx::RegexSets>,
        bmx::tile_kernel<bmx::RegexPolicy<false, true>, bmx::RegexSets>, bmx::tile_kernel<bmx::RegexPolicy<true, true>, bmx::RegexSets>};
    const int slot = (wide ? 1 : 0) + (nl ? 2 : 0);
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    a.warm = (uint32_t)max_len - 1;
    bmx::tile_class_table(re->classes, m, 0, false, a.peq); // bit i: the byte is in class i
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n - lead, max_len, resident); };
    return bmx::tile_launch(&st->tile, WHERE, kernels[slot], slot, num_cu, a, d_text, n, lead, base_offset, piece, d_ends, capacity,
                            n_matches, stream, err, errlen, k);
}

// count >= 1: d_starts[i] for d_ends[i].  window == 0: the automaton is acyclic and a lane walks max_len bytes; else it
// walks `window` bytes of an automaton that may have a cycle (the transposed follow[] goes into the same tables).
// bad_out != NULL: the status bits go there and only an end outside the view is an error here (the caller decides about
// the ends without a match).
int bmx_internal_regex_starts(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                              const uint64_t *d_ends, uint64_t count, uint32_t window, uint32_t flags, uint64_t *d_starts,
                              uint64_t *bad_out, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new RegexState();
    RegexState *st = static_cast<RegexState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::REGEX_STARTS_BLOCK - 1) / bmx::REGEX_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_regex_starts_device: more than 2^31 workgroups of list entries in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_STARTS, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_STARTS, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    BMX_HIP(WHERE_STARTS, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call

    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    if (window == 0) bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len);
    else max_len = (int32_t)window;
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::RegexStartsArgs a;
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
    bmx_regex rev;
    (void)bmx_regex_reverse(re, &rev); // (valid: the shim's check)
    a.k = regex_sets(m, rev.first, rev.last, rev.follow);
    bmx::tile_class_table(rev.classes, m, 0, false, a.peq);
    void (*kernel)(const bmx::RegexStartsArgs) = m > 32 ? bmx::regex_starts_kernel<uint64_t> : bmx::regex_starts_kernel<uint32_t>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::REGEX_STARTS_BLOCK), 0, stream, a);
    BMX_HIP(WHERE_STARTS, hipGetLastError());
    BMX_HIP(WHERE_STARTS, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_STARTS, hipStreamSynchronize(stream));

    uint64_t bad = st->h_ws[0];
    if (bad_out) {
        *bad_out = bad;
        bad &= bmx::REGEX_BAD_END;
    }
    if (bad != 0) {
        snprintf(err, errlen, "bmx_regex_starts_device: %s%s", bad & bmx::REGEX_BAD_END ? "an end outside the view; " : "",
                 bad & bmx::REGEX_BAD_START ? "an end at which no match of this expression ends; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}

// ---- the mirror image: every start, and the end of every start of a list (bmx_regex_begins_kernel.h) ----

namespace {

constexpr const char *WHERE_BEGINS = "bmx_search_regex_begins_device";
constexpr const char *WHERE_ENDS = "bmx_regex_ends_device";

struct RegexBeginsState {
    bmx::TileState tile; // (first: bmx_tile_frame.h)
    uint64_t *d_ws = nullptr; // the ends pass: its status word ...
    uint64_t *h_ws = nullptr; // ... and the pinned copy of it
};
static_assert(offsetof(RegexBeginsState, tile) == 0, "tile_state, ordered_set_seq");

} // namespace

void bmx_internal_regex_begins_free(void *state_v)
{
    RegexBeginsState *st = static_cast<RegexBeginsState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    delete st;
}

float bmx_internal_regex_begins_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

// The frame in START coordinates: the owned starts are [0, n - tail), the frame's "ends" with lead = 0; the kernel gets the
// reversed automaton and, as a further argument, where the view ends.
int bmx_internal_regex_begins(void **state_v, int num_cu, int piece_shift, const void *d_text, uint64_t n, uint64_t tail,
                              uint64_t base_offset, const bmx_regex *re, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches,
                              hipStream_t stream, char *err, size_t errlen)
{
    RegexBeginsState *st = bmx::tile_state<RegexBeginsState>(state_v, n_matches);
    if (tail >= n) return BMX_OK; // no start is owned (before anything is put on `stream`)
    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len); // (the struct's fields are not read)
    if (max_len == 0) return BMX_OK; // no path from first to last: nothing can match
    bmx_regex rev;
    (void)bmx_regex_reverse(re, &rev); // (valid: the shim's check)
    const bmx::RegexSets k = regex_sets(m, rev.first, rev.last, rev.follow);
    const bool wide = m > 32, nl = k.nl != 0;
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexSets, const uint64_t);
    static const Kernel kernels[4] = {bmx::tile_kernel<bmx::RegexBeginsPolicy<false, false>, bmx::RegexSets, uint64_t>,
                                      bmx::tile_kernel<bmx::RegexBeginsPolicy<true, false>, bmx::RegexSets, uint64_t>,
                                      bmx::tile_kernel<bmx::RegexBeginsPolicy<false, true>, bmx::RegexSets, uint64_t>,
                                      bmx::tile_kernel<bmx::RegexBeginsPolicy<true, true>, bmx::RegexSets, uint64_t>};
    const int slot = (wide ? 1 : 0) + (nl ? 2 : 0);
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    a.warm = (uint32_t)max_len - 1;
    bmx::tile_class_table(rev.classes, m, 0, false, a.peq); // bit i: the byte is in class m - 1 - i
    const uint64_t view_hi = n + (reinterpret_cast<uint64_t>(d_text) & 15ull); // one past the view's last byte, aligned coordinates
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n - tail, max_len, resident); };
#ifdef BMX_EXPERIMENTS
    struct Restore { // the session's own piece knob reaches below the shared one's range
        uint32_t &slot, saved;
        ~Restore() { slot = saved; }
    } restore{st->tile.oo.force_piece_shift, st->tile.oo.force_piece_shift};
    if (piece_shift) st->tile.oo.force_piece_shift = (uint32_t)piece_shift;
#else
    (void)piece_shift;
#endif
    return bmx::tile_launch(&st->tile, WHERE_BEGINS, kernels[slot], slot, num_cu, a, d_text, n - tail, 0, base_offset, piece, d_starts,
                            capacity, n_matches, stream, err, errlen, k, view_hi);
}

// count >= 1: d_ends[i] for d_starts[i], one lane per entry over the automaton as given.
int bmx_internal_regex_ends(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                            const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit, uint32_t flags, uint64_t *d_ends,
                            hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new RegexBeginsState();
    RegexBeginsState *st = static_cast<RegexBeginsState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::REGEX_STARTS_BLOCK - 1) / bmx::REGEX_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_regex_ends_device: more than 2^31 workgroups of list entries in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_ENDS, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_ENDS, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    BMX_HIP(WHERE_ENDS, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call

    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len);
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::RegexEndsArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.n = n;
    a.base = base_offset;
    a.starts = d_starts;
    a.limit = d_limit;
    a.count = count;
    a.ends = d_ends;
    a.ws = st->d_ws;
    a.max_len = (uint32_t)max_len; // (0: no entry can be a start of a match)
    a.chunks = (uint32_t)(max_len + 7) / 8;
    a.longest = (flags & BMX_REGEX_LONGEST) ? 1u : 0u;
    a.k = regex_sets(m, re->first, re->last, re->follow);
    bmx::tile_class_table(re->classes, m, 0, false, a.peq);
    void (*kernel)(const bmx::RegexEndsArgs) = m > 32 ? bmx::regex_ends_kernel<uint64_t> : bmx::regex_ends_kernel<uint32_t>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::REGEX_STARTS_BLOCK), 0, stream, a);
    BMX_HIP(WHERE_ENDS, hipGetLastError());
    BMX_HIP(WHERE_ENDS, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_ENDS, hipStreamSynchronize(stream));

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "bmx_regex_ends_device: %s%s", bad & bmx::REGEX_ENDS_BAD_START ? "a start outside the view; " : "",
                 bad & bmx::REGEX_ENDS_NO_MATCH ? "a start at which no match of this expression begins; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}
