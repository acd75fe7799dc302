// bmx_regex_star.hip -- host side of the regular-expression search with unbounded repetition
// (bmx_search_regex_star_device, bmx_regex_star_starts_device, include/bmx.h): masks the automaton down to
// the positions a match can use, builds the sets and tables as bmx_regex.hip does, picks the piece and the warm-up,
// launches the pair-warm-up policy through the tile frame and, if that call ends tainted (or the experiments knob says
// so), the exact slow path: bounds, scan, columns, sweep, and the tile kernel again from the swept states.  The starts
// are bmx_regex.hip's pass with the window in place of max_len, and a fix-up for the ends without a match that short.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_regex_star_kernel.h"

static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::RegexStarX) + sizeof(bmx::RegexSets) + 64 <= 4096, "kernel arguments");
static_assert(bmx::REGEX_STAR_BLOCK == bmx::TILE_BLOCK, "RegexPolicy::fill: one table entry per lane");

namespace {

constexpr const char *WHERE = "bmx_search_regex_star_device";
constexpr const char *WHERE_STARTS = "bmx_regex_star_starts_device";
constexpr uint32_t MIN_PIECE_SHIFT = 8, MAX_PIECE_SHIFT = 12;

struct StarState {
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
    // what the last call did (libbmx_exp.so reads it): tainted waves of the first launch, slow path taken, piece shift,
    // warm-up bytes, pieces, columns, and microseconds of the first launch, R1, the sweep and R2
    uint64_t last[10] = {0};
};
static_assert(offsetof(StarState, tile) == 0, "tile_state, ordered_set_seq");

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
        else k.nl |= 1ull << i; // (self-loops and back edges are irregular)
    }
    for (uint32_t b = 0; b < 8; ++b)
        if ((k.nl >> (8 * b)) & 0xFFu) k.nl_bytes |= 1u << b;
    return k;
}

template <bool ENTRY>
void (*star_tile_kernel(int slot))(const bmx::TileArgs, const bmx::RegexStarX)
{
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexStarX);
    static const Kernel kernels[4] = {bmx::tile_kernel<bmx::RegexStarPolicy<false, false, ENTRY>, bmx::RegexStarX>,
                                      bmx::tile_kernel<bmx::RegexStarPolicy<true, false, ENTRY>, bmx::RegexStarX>,
                                      bmx::tile_kernel<bmx::RegexStarPolicy<false, true, ENTRY>, bmx::RegexStarX>,
                                      bmx::tile_kernel<bmx::RegexStarPolicy<true, true, ENTRY>, bmx::RegexStarX>};
    return kernels[slot];
}

float elapsed_us(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? 1000.0f * ms : 0.0f;
}

} // namespace

// What the slow path has between its own kernels, for this file and for bmx_regex_star_begins.hip, whose pieces are numbered
// from the top of the view and are otherwise the same.  The column offsets: the exclusive scan of popcount(u[l]) over
// [0, n_pieces] into d_off (the scan's temporary storage grows in *d_scan / *scan_cap), the total into the pinned *h_total
// once `stream` is synchronised.
int bmx_internal_regex_star_offsets(const char *where, void **d_scan, size_t *scan_cap, const uint64_t *d_u, uint64_t n_pieces,
                                    uint64_t *d_off, uint64_t *h_total, hipStream_t stream, char *err, size_t errlen)
{
    auto counts = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), bmx::RegexStarColumns{d_u, n_pieces});
    size_t scan_bytes = 0;
    BMX_HIP(where, rocprim::exclusive_scan(nullptr, scan_bytes, counts, d_off, uint64_t(0), (size_t)n_pieces + 1, rocprim::plus<uint64_t>(), stream));
    if (scan_bytes > *scan_cap) {
        if (*d_scan) (void)hipFree(*d_scan);
        *d_scan = nullptr, *scan_cap = 0;
        BMX_HIP(where, hipMalloc(d_scan, scan_bytes));
        *scan_cap = scan_bytes;
    }
    BMX_HIP(where, rocprim::exclusive_scan(*d_scan, scan_bytes, counts, d_off, uint64_t(0), (size_t)n_pieces + 1, rocprim::plus<uint64_t>(), stream));
    BMX_HIP(where, hipMemcpyAsync(h_total, d_off + n_pieces, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(where, hipStreamSynchronize(stream));
    return BMX_OK;
}

// ... and star_sweep_kernel over the pieces [0, n_pieces)
int bmx_internal_regex_star_sweep(const char *where, uint64_t n_pieces, const uint64_t *d_e, const uint64_t *d_u, const uint64_t *d_off,
                                  const uint64_t *d_base, const uint64_t *d_cols, uint64_t *d_entry, hipStream_t stream, char *err,
                                  size_t errlen)
{
    const uint32_t blocks = (uint32_t)((n_pieces + bmx::REGEX_STAR_BLOCK - 1) / bmx::REGEX_STAR_BLOCK);
    hipLaunchKernelGGL(bmx::star_sweep_kernel, dim3(blocks), dim3(bmx::REGEX_STAR_BLOCK), 0, stream, n_pieces, d_e, d_u, d_off, d_base, d_cols,
                       d_entry);
    BMX_HIP(where, hipGetLastError());
    return BMX_OK;
}

namespace {

// The exact list by R1, the sweep and R2.  `a` is the argument block as the first launch left it (geometry and table).
int slow_path(StarState *st, int slot, int num_cu, bmx::TileArgs a, bmx::RegexStarX x, const void *d_text, uint64_t n, uint64_t lead,
              uint64_t base_offset, uint64_t *d_ends, uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err,
              size_t errlen)
{
    const uint32_t ps = a.p_shift;
    const uint64_t n_pieces = ((a.own_hi - 1) >> ps) + 1; // from aligned piece 0: what lies in front of `lead` counts too
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
    hipLaunchKernelGGL(BMX_STAR_PICK(star_bounds_kernel), dim3(blocks), dim3(bmx::REGEX_STAR_BLOCK), 0, stream, a, x, n_pieces, d_e, d_u);
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
        hipLaunchKernelGGL(BMX_STAR_PICK(star_columns_kernel), dim3(run_blocks), dim3(bmx::REGEX_STAR_BLOCK), 0, stream, a, x, k0,
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
    const int rc = bmx::tile_launch(&st->tile, WHERE, star_tile_kernel<true>(slot), slot, num_cu, a2, d_text, n, lead, base_offset, piece,
                                    d_ends, capacity, n_matches, stream, err, errlen, x);
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

void bmx_internal_regex_star_free(void *state_v)
{
    StarState *st = static_cast<StarState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->h_words) (void)hipHostFree(st->h_words);
    if (st->d_taint_n) (void)hipFree(st->d_taint_n);
    if (st->d_pieces) (void)hipFree(st->d_pieces);
    if (st->d_cols) (void)hipFree(st->d_cols);
    if (st->d_scan) (void)hipFree(st->d_scan);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_regex_star_ms(const void *state_v) { return state_v ? static_cast<const StarState *>(state_v)->last_ms : -1.0f; }

void bmx_internal_regex_star_last(const void *state_v, uint64_t out10[10])
{
    const StarState *st = static_cast<const StarState *>(state_v);
    for (int i = 0; i < 10; ++i) out10[i] = st ? st->last[i] : 0;
}

uint32_t bmx_internal_regex_star_piece_shift(uint64_t n, uint64_t resident_lanes)
{
    const uint64_t per = (n + resident_lanes - 1) / std::max<uint64_t>(resident_lanes, 1);
    return std::min<uint32_t>(std::max<uint32_t>(bmx::ceil_log2(per), MIN_PIECE_SHIFT), MAX_PIECE_SHIFT);
}

// a sixteenth of the piece, at least 64 bytes
uint32_t bmx_internal_regex_star_warm(uint32_t piece_shift) { return std::max<uint32_t>(64u, (1u << piece_shift) >> 4); }

int bmx_internal_regex_star(void **state_v, int num_cu, const bmx_regex_star_knobs *knobs, const void *d_text, uint64_t n,
                            uint64_t lead, uint64_t base_offset, const bmx_regex *re, uint64_t *d_ends, uint64_t capacity,
                            uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    StarState *st = bmx::tile_state<StarState>(state_v, n_matches);
    st->last_ms = 0.0f;
    std::memset(st->last, 0, sizeof st->last);
    if (lead >= n) return BMX_OK; // no end is owned (before anything is put on `stream`)
    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    uint64_t useful = 0;
    bmx_regex_star_lengths(m, re->first, re->last, re->follow, &min_len, &max_len, &useful); // (the struct's fields are not read)
    if (max_len == 0) return BMX_OK; // no path from first to last: nothing can match
    // Only the positions a match can use take part: one that cannot reach `last` reports nothing, and left in it could keep
    // the two bounds apart for ever.
    uint64_t follow[BMX_MAX_REGEX_POSITIONS] = {0};
    for (int32_t i = 0; i < m; ++i)
        if ((useful >> i) & 1u) follow[i] = re->follow[i] & useful;
    bmx::RegexStarX x;
    std::memset(&x, 0, sizeof x);
    x.k = star_sets(m, re->first & useful, re->last & useful, follow);
    x.all = useful;
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
        BMX_HIP(WHERE, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, star_tile_kernel<false>(slot), bmx::TILE_BLOCK, 0));
        bpc = std::max(1, std::min(bpc, 8));
    }
    uint32_t ps = bmx_internal_regex_star_piece_shift(n - lead, (uint64_t)num_cu * (uint64_t)bpc * bmx::TILE_BLOCK);
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
    bmx::tile_class_table(re->classes, m, 0, false, a.peq); // bit i: the byte is in class i
    for (uint64_t &w : a.peq) w &= useful;
    const auto piece = [&](uint64_t) { return ps; };
    int rc = bmx::tile_launch(&st->tile, WHERE, star_tile_kernel<false>(slot), slot, num_cu, a, d_text, n, lead, base_offset, piece, d_ends,
                              capacity, n_matches, stream, err, errlen, x);
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
    return slow_path(st, slot, num_cu, a, x, d_text, n, lead, base_offset, d_ends, capacity, n_matches, stream, err, errlen);
}

// The fix-up behind bmx_internal_regex_starts for the ends without a match within the window (their start was stored as
// the end itself): UINT64_MAX unless the end's byte alone matches.
int bmx_internal_regex_star_starts_fix(const void *d_text, uint64_t base_offset, const bmx_regex *re, const uint64_t *d_ends,
                                       uint64_t count, uint64_t *d_starts, hipStream_t stream, char *err, size_t errlen)
{
    bmx::RegexStarFixArgs f;
    std::memset(&f, 0, sizeof f);
    f.text = static_cast<const uint8_t *>(d_text);
    f.base = base_offset;
    f.ends = d_ends;
    f.count = count;
    f.starts = d_starts;
    for (uint64_t both = re->first & re->last; both != 0; both &= both - 1) {
        const uint8_t *cls = re->classes + (size_t)__builtin_ctzll(both) * BMX_CLASS_BYTES;
        for (uint32_t c = 0; c < 256; ++c)
            if ((cls[c >> 3] >> (c & 7)) & 1u) f.one[c >> 6] |= 1ull << (c & 63);
    }
    const uint64_t blocks = (count + bmx::REGEX_STAR_BLOCK - 1) / bmx::REGEX_STAR_BLOCK; // (the starts pass checked the range)
    hipLaunchKernelGGL(bmx::star_starts_fix_kernel, dim3((uint32_t)blocks), dim3(bmx::REGEX_STAR_BLOCK), 0, stream, f);
    BMX_HIP(WHERE_STARTS, hipGetLastError());
    BMX_HIP(WHERE_STARTS, hipStreamSynchronize(stream));
    return BMX_OK;
}
