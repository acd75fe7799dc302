// bmx_regex_star_begins.hip -- host side of the begins search for automata with a cycle and of its ends pass
// (bmx_search_regex_star_begins_device, bmx_regex_star_ends_device, include/bmx.h): masks the automaton
// down to the positions a match can use, reverses it, builds the sets and tables as bmx_regex_star.hip does, picks the piece
// and the warm-up by the same rules, launches the downward pair-warm-up policy through the tile frame in START coordinates
// and, if that call ends tainted (or the experiments knob says so), the exact slow path over pieces numbered from the top
// of the view: bounds, columns, the forward search's scan and sweep through bmx_regex_star.hip's launchers, and the tile
// kernel again from the swept states.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_regex_star_begins_kernel.h"

static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::RegexStarBeginsX) + sizeof(bmx::RegexSets) + 64 <= 4096, "kernel arguments");
static_assert(sizeof(bmx::RegexEndsArgs) + 8 <= 4096, "kernel arguments");
static_assert(bmx::REGEX_STAR_BLOCK == bmx::TILE_BLOCK, "RegexPolicy::fill: one table entry per lane");

namespace {

constexpr const char *WHERE = "bmx_search_regex_star_begins_device";
constexpr const char *WHERE_ENDS = "bmx_regex_star_ends_device";

struct StarBeginsState {
    bmx::TileState tile; // (first: bmx_tile_frame.h)
    uint64_t *h_words = nullptr;     // pinned: [0] the taint word, [1] the slow path's column total
    uint64_t *h_words_dev = nullptr;
    unsigned long long *d_taint_n = nullptr;
    // the slow path's workspace, made on its first use: five words per piece (e, u, offsets, base, entry) ...
    uint64_t *d_pieces = nullptr;
    uint64_t pieces_cap = 0;
    uint64_t *d_cols = nullptr; // ... the columns ...
    uint64_t cols_cap = 0;
    void *d_scan = nullptr; // ... and the scan's
    size_t scan_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // slow path: start, after R1, after the sweep, after R2
    float last_ms = -1.0f;
    uint64_t last[10] = {0}; // as bmx_regex_star.hip's: what the last call did (libbmx_exp.so reads it)
    uint64_t *d_ws = nullptr; // the ends pass: its status word and clipped count ...
    uint64_t *h_ws = nullptr; // ... and the pinned copy of them
};
static_assert(offsetof(StarBeginsState, tile) == 0, "tile_state, ordered_set_seq");

// (bmx_regex_star.hip's: self-loops and back edges are irregular)
bmx::RegexSets star_sets(int32_t m, uint64_t first, uint64_t last, const uint64_t *follow)
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

// `re` with everything but its useful positions taken out of first, last and follow[]; false: nothing can match.
bool masked_automaton(const bmx_regex *re, bmx_regex *out, uint64_t *useful_out)
{
    int32_t min_len = 0, max_len = 0;
    uint64_t useful = 0;
    bmx_regex_star_lengths(re->m, re->first, re->last, re->follow, &min_len, &max_len, &useful); // (the struct's fields are not read)
    if (max_len == 0) return false;
    *out = *re;
    out->first &= useful;
    out->last &= useful;
    for (int32_t i = 0; i < BMX_MAX_REGEX_POSITIONS; ++i) out->follow[i] = i < re->m && ((useful >> i) & 1u) ? re->follow[i] & useful : 0;
    *useful_out = useful;
    return true;
}

template <bool ENTRY>
void (*star_begins_tile_kernel(int slot))(const bmx::TileArgs, const bmx::RegexStarBeginsX)
{
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexStarBeginsX);
    static const Kernel kernels[4] = {bmx::tile_kernel<bmx::RegexStarBeginsPolicy<false, false, ENTRY>, bmx::RegexStarBeginsX>,
                                      bmx::tile_kernel<bmx::RegexStarBeginsPolicy<true, false, ENTRY>, bmx::RegexStarBeginsX>,
                                      bmx::tile_kernel<bmx::RegexStarBeginsPolicy<false, true, ENTRY>, bmx::RegexStarBeginsX>,
                                      bmx::tile_kernel<bmx::RegexStarBeginsPolicy<true, true, ENTRY>, bmx::RegexStarBeginsX>};
    return kernels[slot];
}

float elapsed_us(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? 1000.0f * ms : 0.0f;
}

// The exact list by R1, the sweep and R2.  `a` is the argument block as the first launch left it (geometry and table).
int slow_path(StarBeginsState *st, int slot, int num_cu, bmx::TileArgs a, bmx::RegexStarBeginsX x, const void *d_text, uint64_t n_starts,
              uint64_t base_offset, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err,
              size_t errlen)
{
    const uint32_t ps = a.p_shift;
    const uint64_t n_pieces = ((x.view_hi - 1) >> ps) + 1; // down to aligned piece 0, from the piece of the view's last byte
    const uint32_t blocks = (uint32_t)((n_pieces + bmx::REGEX_STAR_BLOCK - 1) / bmx::REGEX_STAR_BLOCK); // n < 2^40, ps >= 4
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(WHERE, hipEventCreate(&e));
    if (n_pieces + 1 > st->pieces_cap) {
        if (st->d_pieces) (void)hipFree(st->d_pieces);
        st->d_pieces = nullptr, st->pieces_cap = 0;
        BMX_HIP(WHERE, hipMalloc(&st->d_pieces, 5 * (n_pieces + 1) * sizeof(uint64_t)));
        st->pieces_cap = n_pieces + 1;
    }
    uint64_t *d_e = st->d_pieces, *d_u = d_e + st->pieces_cap, *d_off = d_u + st->pieces_cap, *d_base = d_off + st->pieces_cap,
             *d_entry = d_base + st->pieces_cap;

    BMX_HIP(WHERE, hipEventRecord(st->ev[0], stream));
    const bool wide = slot & 1, nl = slot & 2;
#define BMX_STAR_PICK(kernel) (wide ? (nl ? bmx::kernel<true, true> : bmx::kernel<true, false>) : (nl ? bmx::kernel<false, true> : bmx::kernel<false, false>))
    hipLaunchKernelGGL(BMX_STAR_PICK(star_begins_bounds_kernel), dim3(blocks), dim3(bmx::REGEX_STAR_BLOCK), 0, stream, a, x, n_pieces, d_e, d_u);
    BMX_HIP(WHERE, hipGetLastError());

    int orc = bmx_internal_regex_star_offsets(WHERE, &st->d_scan, &st->scan_cap, d_u, n_pieces, d_off, &st->h_words[1], stream, err, errlen);
    if (orc != BMX_OK) return orc;
    const uint64_t n_cols = st->h_words[1];
    if (n_cols > st->cols_cap) {
        if (st->d_cols) (void)hipFree(st->d_cols);
        st->d_cols = nullptr, st->cols_cap = 0;
        BMX_HIP(WHERE, hipMalloc(&st->d_cols, n_cols * sizeof(uint64_t)));
        st->cols_cap = n_cols;
    }
    if (n_pieces > 1) {
        bmx::RegexSets k0 = x.k;
        k0.first = 0;
        const uint32_t run_blocks = (uint32_t)((n_pieces - 1 + bmx::REGEX_STAR_BLOCK - 1) / bmx::REGEX_STAR_BLOCK);
        hipLaunchKernelGGL(BMX_STAR_PICK(star_begins_columns_kernel), dim3(run_blocks), dim3(bmx::REGEX_STAR_BLOCK), 0, stream, a, x, k0,
                           n_pieces - 1, d_e, d_u, d_off, d_base, st->d_cols);
        BMX_HIP(WHERE, hipGetLastError());
    }
#undef BMX_STAR_PICK
    BMX_HIP(WHERE, hipEventRecord(st->ev[1], stream));
    orc = bmx_internal_regex_star_sweep(WHERE, n_pieces, d_e, d_u, d_off, d_base, st->d_cols, d_entry, stream, err, errlen);
    if (orc != BMX_OK) return orc;
    BMX_HIP(WHERE, hipEventRecord(st->ev[2], stream));

    x.entry = d_entry;
    bmx::TileArgs a2;
    std::memset(&a2, 0, sizeof a2);
    a2.m = a.m;
    std::memcpy(a2.peq, a.peq, sizeof a2.peq);
    const auto piece = [&](uint64_t) { return ps; };
    const int rc = bmx::tile_launch(&st->tile, WHERE, star_begins_tile_kernel<true>(slot), slot, num_cu, a2, d_text, n_starts, 0, base_offset,
                                    piece, d_starts, capacity, n_matches, stream, err, errlen, x);
    if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) return rc;
    BMX_HIP(WHERE, hipEventRecord(st->ev[3], stream));
    BMX_HIP(WHERE, hipEventSynchronize(st->ev[3]));
    st->last[4] = n_pieces, st->last[5] = n_cols;
    st->last[7] = (uint64_t)elapsed_us(st->ev[0], st->ev[1]);
    st->last[8] = (uint64_t)elapsed_us(st->ev[1], st->ev[2]);
    st->last[9] = (uint64_t)(1000.0f * st->tile.oo.last_ms);
    st->last_ms += 1e-3f * elapsed_us(st->ev[0], st->ev[3]);
    return rc;
}

} // namespace

void bmx_internal_regex_star_begins_free(void *state_v)
{
    StarBeginsState *st = static_cast<StarBeginsState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->h_words) (void)hipHostFree(st->h_words);
    if (st->d_taint_n) (void)hipFree(st->d_taint_n);
    if (st->d_pieces) (void)hipFree(st->d_pieces);
    if (st->d_cols) (void)hipFree(st->d_cols);
    if (st->d_scan) (void)hipFree(st->d_scan);
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_regex_star_begins_ms(const void *state_v)
{
    return state_v ? static_cast<const StarBeginsState *>(state_v)->last_ms : -1.0f;
}

void bmx_internal_regex_star_begins_last(const void *state_v, uint64_t out10[10])
{
    const StarBeginsState *st = static_cast<const StarBeginsState *>(state_v);
    for (int i = 0; i < 10; ++i) out10[i] = st ? st->last[i] : 0;
}

int bmx_internal_regex_star_begins(void **state_v, int num_cu, const bmx_regex_star_knobs *knobs, const void *d_text, uint64_t n,
                                   uint64_t tail, uint64_t base_offset, const bmx_regex *re, uint64_t *d_starts, uint64_t capacity,
                                   uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    StarBeginsState *st = bmx::tile_state<StarBeginsState>(state_v, n_matches);
    st->last_ms = 0.0f;
    std::memset(st->last, 0, sizeof st->last);
    if (tail >= n) return BMX_OK; // no start is owned (before anything is put on `stream`)
    const int32_t m = re->m;
    // Only the positions a match can use take part, then the mirror image of what is left.
    bmx_regex rev;
    uint64_t useful = 0;
    if (!masked_automaton(re, &rev, &useful)) return BMX_OK; // no path from first to last: nothing can match
    if (bmx_regex_reverse(&rev, &rev) != BMX_OK) return BMX_ERR_ARG; // (valid by the shim's check: does not happen)
    bmx::RegexStarBeginsX x;
    std::memset(&x, 0, sizeof x);
    x.k = star_sets(m, rev.first, rev.last, rev.follow);
    for (uint64_t u = useful; u != 0; u &= u - 1) x.all |= 1ull << (m - 1 - __builtin_ctzll(u));
    x.view_hi = n + (reinterpret_cast<uint64_t>(d_text) & 15ull);
    const bool wide = m > 32, nl = x.k.nl != 0;
    const int slot = (wide ? 1 : 0) + (nl ? 2 : 0);

    if (!st->h_words) {
        BMX_HIP(WHERE, hipHostMalloc(&st->h_words, 2 * sizeof(uint64_t), hipHostMallocMapped));
        BMX_HIP(WHERE, hipHostGetDevicePointer((void **)&st->h_words_dev, st->h_words, 0));
    }
    if (!st->d_taint_n) BMX_HIP(WHERE, hipMalloc(&st->d_taint_n, sizeof(unsigned long long)));
    BMX_HIP(WHERE, hipMemsetAsync(st->d_taint_n, 0, sizeof(unsigned long long), stream));
    st->h_words[0] = st->h_words[1] = 0;
    x.taint = st->h_words_dev;
    x.taint_n = st->d_taint_n;

    int &bpc = st->tile.blocks_per_cu[slot]; // (as tile_launch would: the piece below needs it first)
    if (bpc == 0) {
        BMX_HIP(WHERE, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, star_begins_tile_kernel<false>(slot), bmx::TILE_BLOCK, 0));
        bpc = std::max(1, std::min(bpc, 8));
    }
    uint32_t ps = bmx_internal_regex_star_piece_shift(n - tail, (uint64_t)num_cu * (uint64_t)bpc * bmx::TILE_BLOCK);
    bool force_slow = false;
#ifdef BMX_EXPERIMENTS
    struct Restore { // the session's own piece knob reaches below the shared one's range
        uint32_t &slot, saved;
        ~Restore() { slot = saved; }
    } restore{st->tile.oo.force_piece_shift, st->tile.oo.force_piece_shift};
    if (knobs->piece_shift) st->tile.oo.force_piece_shift = (uint32_t)knobs->piece_shift;
    if (st->tile.oo.force_piece_shift) ps = st->tile.oo.force_piece_shift;
    force_slow = knobs->force_slow;
#endif
    x.warm = bmx_internal_regex_star_warm(ps);
#ifdef BMX_EXPERIMENTS
    if (knobs->warm) x.warm = (uint32_t)knobs->warm;
#else
    (void)knobs;
#endif

    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    bmx::tile_class_table(rev.classes, m, 0, false, a.peq); // bit i: the byte is in class m - 1 - i
    for (uint64_t &w : a.peq) w &= x.all;
    const auto piece = [&](uint64_t) { return ps; };
    int rc = bmx::tile_launch(&st->tile, WHERE, star_begins_tile_kernel<false>(slot), slot, num_cu, a, d_text, n - tail, 0, base_offset, piece,
                              d_starts, capacity, n_matches, stream, err, errlen, x);
    st->last_ms = st->tile.oo.last_ms;
    st->last[2] = ps, st->last[3] = x.warm, st->last[6] = (uint64_t)(1000.0f * st->tile.oo.last_ms);
    if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) return rc;
    const bool tainted = *(volatile uint64_t *)&st->h_words[0] != 0;
#ifdef BMX_EXPERIMENTS
    {
        unsigned long long waves = 0;
        BMX_HIP(WHERE, hipMemcpyAsync(&waves, st->d_taint_n, sizeof waves, hipMemcpyDeviceToHost, stream));
        BMX_HIP(WHERE, hipStreamSynchronize(stream));
        st->last[0] = waves;
    }
#endif
    if (!tainted && !force_slow) return rc;
    st->last[1] = 1;
    if (n_matches) *n_matches = 0;
    return slow_path(st, slot, num_cu, a, x, d_text, n - tail, base_offset, d_starts, capacity, n_matches, stream, err, errlen);
}

// count >= 1: d_ends[i] for d_starts[i], one lane per entry over the automaton as given (masked to its useful positions, so
// that a state that can no longer reach `last` is empty), at most `window` bytes upwards.  *bad_out: the status bits (only
// a start outside the view is an error here); *clipped_out: the entries the window cut short.
int bmx_internal_regex_star_ends(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                 const uint64_t *d_starts, uint64_t count, const uint64_t *d_limit, uint32_t window, uint32_t flags,
                                 bool early_exit, uint64_t *d_ends, uint64_t *bad_out, uint64_t *clipped_out, hipStream_t stream,
                                 char *err, size_t errlen)
{
    if (!*state_v) *state_v = new StarBeginsState();
    StarBeginsState *st = static_cast<StarBeginsState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::REGEX_STARTS_BLOCK - 1) / bmx::REGEX_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_regex_star_ends_device: more than 2^31 workgroups of list entries in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_ENDS, hipMalloc(&st->d_ws, 2 * sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_ENDS, hipHostMalloc(&st->h_ws, 2 * sizeof(uint64_t), hipHostMallocDefault));
    BMX_HIP(WHERE_ENDS, hipMemsetAsync(st->d_ws, 0, 2 * sizeof(uint64_t), stream)); // status and count start clean in every call

    const int32_t m = re->m;
    bmx_regex fwd;
    uint64_t useful = 0;
    if (!masked_automaton(re, &fwd, &useful)) std::memset(&fwd, 0, sizeof fwd), fwd.m = m, useful = 0; // nothing matches anywhere
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
    a.max_len = window;
    a.chunks = (window + 7) / 8;
    a.longest = (flags & BMX_REGEX_LONGEST) ? 1u : 0u;
    a.k = star_sets(m, fwd.first, fwd.last, fwd.follow);
    bmx::tile_class_table(re->classes, m, 0, false, a.peq);
    for (uint64_t &w : a.peq) w &= useful;
    void (*kernel)(const bmx::RegexEndsArgs, const uint32_t) = m > 32 ? bmx::regex_star_ends_kernel<uint64_t> : bmx::regex_star_ends_kernel<uint32_t>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::REGEX_STARTS_BLOCK), 0, stream, a, early_exit ? 1u : 0u);
    BMX_HIP(WHERE_ENDS, hipGetLastError());
    BMX_HIP(WHERE_ENDS, hipMemcpyAsync(st->h_ws, st->d_ws, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_ENDS, hipStreamSynchronize(stream));
    *bad_out = st->h_ws[0];
    *clipped_out = st->h_ws[1];
    if (st->h_ws[0] & bmx::REGEX_STAR_ENDS_BAD_START) {
        snprintf(err, errlen, "bmx_regex_star_ends_device: a start outside the view");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}
