// bmx_scan.hip -- the exact search of the C ABI (include/bmx.h): the Boyer-Moore scan over a resident text.  The table
// of scan-kernel variants and the choice among them, the LDS arithmetic, the enqueue / finish pair with the ordering
// kernel and the fill pass behind it, the several-patterns pass, and the state all of that keeps between calls.  The
// state hangs off the context (ctx->scan), like every other feature's; the entry points of the exact search are
// defined here, where their code is -- the shim (bmx_shim.hip) holds the context and knows no variant.
#include "bmx.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmx_internal.h"
#include "bmx_scan_kernel.h"

#include "bmx_order_kernels.h"
#ifdef BMX_EXPERIMENTS
#include "bmx_scan_ring_kernel.h"
#include "bmx_scan_wave_kernel.h"
#endif

static_assert(bmx::MAX_PATTERN == BMX_MAX_PATTERN, "header and kernel disagree");
static_assert(bmx::MAX_MULTI == BMX_MAX_MULTI, "header and kernel disagree");

namespace {

// the text bmx_last_error() returns on this thread (the shim's buffer)
void set_err(const char *fmt, ...)
{
    size_t len = 0;
    char *buf = bmx_internal_error_buffer(&len);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, len, fmt, ap);
    va_end(ap);
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return BMX_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

// Scan-kernel variants.  kind 0 = workgroup-tile kernel (bmx_scan_kernel.h): `block`
// threads share a tile of block*seg window starts, two tile buffers, one barrier
// per tile.  kind 1 = wave-stream kernel (bmx_scan_wave_kernel.h): every wave owns
// pieces of 64*seg window starts and `nbuf` private buffers, no barrier.
// kernel_short is the walker used for m < 4 (kind 0 only differs).
struct Variant {
    int kind;
    int block;
    int seg;
    int nbuf;
    int loaders; // kind 0: waves that issue all of the DMA (< 0: the last ones); they walk `segi` window starts per lane (0: none)
    int segi;
    bool stamps; // diagnostic build that writes s_memtime sums (bmx_scan_stamps)
    bool qgram;  // 4-gram walker: shift table in LDS
    int canon_minm; // > 0: the walker skips with a filter of its own (4-gram table, quad-SAD) and therefore needs the
                    // canonical shift tables and a pattern of at least this length; 0: any tables, any m
    void (*kernel)(const bmx::ScanArgs); // nullptr: this slot is not built into this library
    void (*kernel_short)(const bmx::ScanArgs);
    // the fill pass of this geometry for dense results (m >= 4 / m < 4); nullptr: the kernel appends dense tiles the
    // direct way (global atomics) and bmx_search_device_finish sorts
    void (*fill)(const bmx::ScanArgs);
    void (*fill_short)(const bmx::ScanArgs);
    void (*fill_count)(const bmx::ScanArgs); // the fill pass's first launch (tile counts)
    void (*fill_count_short)(const bmx::ScanArgs);
    bool steal = false; // the main kernel hands its last tiles out by ticket (scan_kernel MODE 12): the ordering kernel checks the tile count
    bool steal_short = false; // ... the short-pattern kernel does
};

// The slot numbers are stable (tools/ and the notes in DESIGN.md refer to them), but the PRODUCT library
// (libbmx.so) only contains the kernels the automatic choice can pick plus their parity-tested alternates;
// every other slot -- schedules that lost (ring, wave streams, loader waves, other geometries) and the
// timing-only builds whose match lists are NOT valid (DMA only, walkers only, one walking wave) -- exists
// only in libbmx_exp.so, the same sources compiled with -DBMX_EXPERIMENTS for tools/ (BMX_LIB=exp).
// bmx_set_variant() refuses a slot that is not built: no caller of the shipped C ABI can select a kernel
// that returns a wrong match list (tests/test_gpu_parity.py::test_product_library_accepts_only_its_variants).
#define BMX_ABSENT {0, 0, 0, 0, 0, 0, false, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}
#define BMX_TILE(B, S, AUX, MODE, W) BMX_TILE_L(B, S, AUX, MODE, W, 0)
#define BMX_TILE_L(B, S, AUX, MODE, W, L) BMX_TILE_LS(B, S, AUX, MODE, W, L, 0)
#define BMX_TILE_LS(B, S, AUX, MODE, W, L, SI) BMX_TILE_G(B, S, AUX, MODE, W, L, SI, 0)
#define BMX_TILE_G(B, S, AUX, MODE, W, L, SI, G) \
    {0, B, S, 2, L, SI, (MODE) == 5 || (MODE) == 8, (W) == 3 || (W) == 10, \
     (W) == 7 || (W) == 8 ? 1 : ((W) == 3 || (W) == 9 ? 4 : ((W) == 10 ? 8 : 0)), \
     bmx::scan_kernel<B, S, AUX, MODE, W, L, SI, G>, bmx::scan_kernel<B, S, AUX, MODE, 6, L, SI, G>, nullptr, nullptr, nullptr, nullptr}
// a product geometry: with the fill pass for dense results (byte-wise walker / short-pattern walker on the same tiles)
#define BMX_TILE_F(B, S, AUX, W) \
    {0, B, S, 2, 0, 0, false, (W) == 3 || (W) == 10, (W) == 3 ? 4 : ((W) == 10 ? 8 : 0), bmx::scan_kernel<B, S, AUX, 0, W>, \
     bmx::scan_kernel<B, S, AUX, 0, 6>, bmx::scan_kernel<B, S, AUX, 9, 0>, bmx::scan_kernel<B, S, AUX, 9, 6>, \
     bmx::scan_kernel<B, S, AUX, 10, 0>, bmx::scan_kernel<B, S, AUX, 10, 6>}
// ... and with static shares + a stolen tail (scan_kernel MODE 12); short patterns and the fill pass as in BMX_TILE_F
#define BMX_TILE_S(B, S, AUX, W) \
    {0, B, S, 2, 0, 0, false, (W) == 3 || (W) == 10, (W) == 7 || (W) == 8 ? 1 : ((W) == 3 ? 4 : ((W) == 10 ? 8 : 0)), bmx::scan_kernel<B, S, AUX, 12, W>, \
     bmx::scan_kernel<B, S, AUX, 0, 6>, bmx::scan_kernel<B, S, AUX, 9, 0>, bmx::scan_kernel<B, S, AUX, 9, 6>, \
     bmx::scan_kernel<B, S, AUX, 10, 0>, bmx::scan_kernel<B, S, AUX, 10, 6>, true}
// ... and the short-pattern kernel with a stolen tail as well
#define BMX_TILE_SS(B, S, AUX, W) \
    {0, B, S, 2, 0, 0, false, (W) == 3 || (W) == 10, (W) == 7 || (W) == 8 ? 1 : ((W) == 3 ? 4 : ((W) == 10 ? 8 : 0)), bmx::scan_kernel<B, S, AUX, 12, W>, \
     bmx::scan_kernel<B, S, AUX, 12, 6>, bmx::scan_kernel<B, S, AUX, 9, 0>, bmx::scan_kernel<B, S, AUX, 9, 6>, \
     bmx::scan_kernel<B, S, AUX, 10, 0>, bmx::scan_kernel<B, S, AUX, 10, 6>, true, true}
// a product geometry with clock stamps (MODE 5: per tile phase, MODE 8: two stamps around the loop): everything the
// product kernel does, the per-tile counts of short patterns included
#define BMX_TILE_FM(B, S, AUX, MODE, W) \
    {0, B, S, 2, 0, 0, true, (W) == 3 || (W) == 10, (W) == 3 ? 4 : ((W) == 10 ? 8 : 0), bmx::scan_kernel<B, S, AUX, MODE, W>, \
     bmx::scan_kernel<B, S, AUX, MODE, 6>, bmx::scan_kernel<B, S, AUX, 9, 0>, bmx::scan_kernel<B, S, AUX, 9, 6>, \
     bmx::scan_kernel<B, S, AUX, 10, 0>, bmx::scan_kernel<B, S, AUX, 10, 6>}
#define BMX_TILE_W32(B, S, AUX, MODE, W) /* 32 waves per CU: the 80-SGPR build */ \
    {0, B, S, 2, 0, 0, (MODE) == 5, (W) == 3, (W) == 3 ? 4 : 0, bmx::scan_kernel_w32<B, S, AUX, MODE, W, 0>, bmx::scan_kernel_w32<B, S, AUX, (MODE) == 12 ? 0 : (MODE), 6, 0>, \
     (MODE) == 0 || (MODE) == 12 ? bmx::scan_kernel<B, S, AUX, 9, 0> : nullptr, (MODE) == 0 || (MODE) == 12 ? bmx::scan_kernel<B, S, AUX, 9, 6> : nullptr, \
     (MODE) == 0 || (MODE) == 12 ? bmx::scan_kernel<B, S, AUX, 10, 0> : nullptr, (MODE) == 0 || (MODE) == 12 ? bmx::scan_kernel<B, S, AUX, 10, 6> : nullptr, (MODE) == 12}
#define BMX_RING(B, S, AUX, SKIP, MODE) BMX_RING_P(B, S, AUX, (SKIP) ? 2 : 0, MODE, 0)
#define BMX_RING_P(B, S, AUX, W, MODE, P) \
    {2, B, S, 3, 0, 0, (MODE) == 5, (W) == 10, (W) == 10 ? 8 : 0, bmx::scan_ring_kernel<B, S, AUX, W, MODE, P>, bmx::scan_ring_kernel<B, S, AUX, 0, MODE, P>, nullptr, nullptr, nullptr, nullptr}
#define BMX_WAVE(WV, S, AUX, MODE, D, NB)                                                      \
    {1, (WV) * 64, S, NB, 0, 0, false, false, 0, bmx::scan_wave_kernel<WV, S, AUX, MODE, D, NB>, bmx::scan_wave_kernel<WV, S, AUX, MODE, D, NB>, nullptr, nullptr, nullptr, nullptr}
constexpr int N_VARIANTS = 90; // slots of the kernel table (built into this library or not)
struct VariantTable {
    Variant v[N_VARIANTS];
    VariantTable()
    {
        for (Variant &x : v) x = Variant BMX_ABSENT;
#define SLOT(I, ...) v[I] = Variant __VA_ARGS__
#include "bmx_variants_product.inc"
#ifdef BMX_EXPERIMENTS
#include "bmx_variants_exp.inc"
#endif
#undef SLOT
    }
};
const VariantTable g_table;
const Variant *const g_variants = g_table.v;

constexpr uint32_t LDS_PER_CU = 160 * 1024;


// What the exact search keeps between calls: one per context (ctx->scan), made by bmx_ctx_create and freed by
// bmx_ctx_destroy.
struct ScanState {
    int variant = 0;
    bool auto_walker = true; // until bmx_set_variant(): the walker by the pattern and the text's alphabet (pick_variant)
    int blocks_per_cu = 0; // 0 = as many as LDS and the 32-wave limit admit
    // distinct byte values of the texts seen last (sampled by order_kernel behind every search), by device pointer and length
    static constexpr int N_SAMPLED = 16;
    struct { const void *ptr; uint64_t n; int sigma; } sampled[N_SAMPLED] = {};
    unsigned sampled_next = 0;
    const void *last_text = nullptr; // the text of the search whose status is awaited (its order_kernel samples it again)
    uint64_t last_text_n = 0;
    struct { // the most recent scan launch
        int variant = 0;         // what it ran (bmx_scan_geometry reports it)
        bmx::ScanArgs args;      // its arguments (the fill pass re-runs its geometry)
        int grid = 0;
        int32_t m = 0;
        bool short_pat = false;  // ... was for a short pattern (short_pattern(): its fill pass tests every position, nothing is walked)
        bool counted = false;    // ... and its scan kernel left the per-tile / per-wave match counts the fill pass starts from
        bool fillable = false;
    } last;
    unsigned long long *d_count = nullptr; // live match counter; re-armed by order_kernel
    uint32_t *d_tile_count = nullptr;      // matches per tile of the last scan (dense results: input of the fill pass)
    uint64_t *d_tile_base = nullptr;       // their exclusive scan
    uint32_t *d_wave_count = nullptr;      // 1-3-byte patterns: matches per wave piece of every tile (block / 64 words per tile)
    uint64_t tile_cap = 0;                 // tiles the three arrays have room for
    int multi_attr[2] = {0, 0};            // dynamic-LDS limit set for the two multi-pattern kernels on this device
    uint8_t *d_multi = nullptr;            // bmx_search_device_multi: the patterns' tables (one blob) in HBM ...
    uint8_t *h_multi = nullptr;            // ... and the pinned host buffer they are copied from (truly asynchronous; no wait for a pageable copy)
    void *d_sort_scratch = nullptr;        // second key array + rocPRIM's temporary storage of the large sort (grown on demand, kept)
    size_t sort_scratch_bytes = 0;
    uint32_t *d_bucket_cnt = nullptr;      // ORDER_BUCKETS, re-armed by order_kernel
    uint64_t *d_bucket_store = nullptr;    // ORDER_BUCKETS x ORDER_BUCKET_CAP
    uint32_t *d_overflow = nullptr;
    uint64_t *d_status = nullptr;          // {count, needs_sort} of the last search
    uint64_t *h_status = nullptr;          // pinned, device-visible: {count, needs_sort, seq} written by order_kernel
    uint64_t *h_status_dev = nullptr;      // device address of h_status
    uint64_t seq = 0;                      // sequence number of the last enqueue
    unsigned long long *d_stamps = nullptr; // diagnostic builds only (bmx_scan_stamps)
    uint64_t stamp_words = 0;
    bool armed = false;                    // counters known to be zero
    int order_overlap = 0;                 // bmx_set_order_overlap
    hipStream_t order_stream = nullptr;    // ... the context's own stream for the ordering kernel
    hipEvent_t ev_order = nullptr;         // ... recorded behind it
    bool order_forked = false;             // the last enqueue's ordering kernel went there and _finish has not been called yet
    bool last_sorted = false;              // the last finish had to sort (the order kernel could not order the list)
    static constexpr int EV_RING = 64;     // event pairs around the last EV_RING scan kernels
    hipEvent_t ev0[EV_RING] = {}, ev1[EV_RING] = {};
    uint64_t n_timed = 0;                  // scan kernels launched with events so far
    bool timed = false;
    int lds_attr_set[N_VARIANTS] = {};
    int lds_attr_set_short[N_VARIANTS] = {};
};

ScanState *scan_of(const bmx_ctx *ctx) { return static_cast<ScanState *>(ctx->scan); }

} // namespace

// Eager, in this order: the counter, the bucket counts, the bucket store, the overflow words, the status words, the mapped
// pinned block, the event pairs -- a first search allocates nothing but what its own path grows.  *state is set even when
// a step fails (bmx_internal_scan_free takes a half-made one).
hipError_t bmx_internal_scan_create(void **state)
{
    ScanState *s = new ScanState();
    *state = s;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc(&s->d_count, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc(&s->d_bucket_cnt, bmx::ORDER_BUCKETS * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMalloc(&s->d_bucket_store, (size_t)bmx::ORDER_BUCKETS * bmx::ORDER_BUCKET_CAP * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&s->d_overflow, 8 * sizeof(uint32_t)); // {bucket overflow, scan error, dense, ticket counter, tiles walked (stolen-tail kernels), -, -, -}
    if (e == hipSuccess) e = hipMalloc(&s->d_status, 4 * sizeof(uint64_t));
    // [0..3] {count, needs_sort, seq, scan error}; [6]: order_kernel's text sample; [8..16]: where each pattern's list begins (multi-pattern pass)
    if (e == hipSuccess) e = hipHostMalloc(&s->h_status, 32 * sizeof(uint64_t), hipHostMallocMapped);
    if (e == hipSuccess) {
        std::memset(s->h_status, 0, 32 * sizeof(uint64_t));
        e = hipHostGetDevicePointer((void **)&s->h_status_dev, s->h_status, 0);
    }
    for (int i = 0; i < ScanState::EV_RING && e == hipSuccess; ++i) {
        e = hipEventCreate(&s->ev0[i]);
        if (e == hipSuccess) e = hipEventCreate(&s->ev1[i]);
    }
    return e;
}

void bmx_internal_scan_free(void *state)
{
    ScanState *s = static_cast<ScanState *>(state);
    if (!s) return;
    if (s->d_count) (void)hipFree(s->d_count);
    if (s->d_multi) (void)hipFree(s->d_multi);
    if (s->h_multi) (void)hipHostFree(s->h_multi);
    if (s->d_tile_count) (void)hipFree(s->d_tile_count);
    if (s->d_tile_base) (void)hipFree(s->d_tile_base);
    if (s->d_wave_count) (void)hipFree(s->d_wave_count);
    if (s->d_bucket_cnt) (void)hipFree(s->d_bucket_cnt);
    if (s->d_bucket_store) (void)hipFree(s->d_bucket_store);
    if (s->d_overflow) (void)hipFree(s->d_overflow);
    if (s->d_status) (void)hipFree(s->d_status);
    if (s->d_stamps) (void)hipFree(s->d_stamps);
    if (s->d_sort_scratch) (void)hipFree(s->d_sort_scratch);
    if (s->ev_order) (void)hipEventDestroy(s->ev_order);
    if (s->order_stream) (void)hipStreamDestroy(s->order_stream);
    if (s->h_status) (void)hipHostFree(s->h_status);
    for (int i = 0; i < ScanState::EV_RING; ++i) {
        if (s->ev0[i]) (void)hipEventDestroy(s->ev0[i]);
        if (s->ev1[i]) (void)hipEventDestroy(s->ev1[i]);
    }
    delete s;
}

namespace {

uint64_t unit_bytes(const Variant &v)
{
    const int nl = v.loaders < 0 ? -v.loaders : v.loaders;
    return v.kind != 1 ? 64ull * (uint64_t)(nl * v.segi + (v.block / 64 - nl) * v.seg) : 64ull * v.seg;
}

// LDS of one workgroup with two buffers of `cap` parked matches of 8 bytes (bmx_scan_common.h report_hit).
uint32_t lds_bytes_with(const Variant &v, int32_t m, uint32_t cap)
{
    const uint32_t halo16 = ((uint32_t)(m - 1) + 15u) & ~15u;
    const uint32_t waves = (uint32_t)v.block / 64u;
    const uint32_t tables = 256 * 2 + (((uint32_t)m + 7u) & ~7u) * 2 + (((uint32_t)m + 15u) & ~15u) + 256 +
                            (v.qgram ? bmx::QGRAM_TABLE : 0u) + 256u + (cap ? 2u * cap * 8u + 32u : 0u);
    if (v.kind != 1) return (uint32_t)v.nbuf * ((uint32_t)unit_bytes(v) + halo16) + tables;
    return waves * v.nbuf * (64u * v.seg + halo16) + tables;
}

// Matches a workgroup may park in LDS per tile: workgroup-tile kernels only, and only as many as leave the
// number of workgroups per CU alone (variant 2 lives on its second workgroup) and fit at all.
uint32_t stage_cap_for(const Variant &v, int32_t m)
{
    if (v.kind != 0) return 0;
    const uint32_t bare = lds_bytes_with(v, m, 0);
    if (bare > LDS_PER_CU) return 0;
    for (uint32_t cap = 1024; cap >= 64; cap /= 2) {
        const uint32_t with = lds_bytes_with(v, m, cap);
        if (with <= LDS_PER_CU && LDS_PER_CU / with == LDS_PER_CU / bare) return cap;
    }
    return 0;
}

uint32_t lds_bytes_for(const Variant &v, int32_t m) { return lds_bytes_with(v, m, stage_cap_for(v, m)); }

int blocks_per_cu_for(const ScanState *s, const Variant &v, int32_t m)
{
    int by_lds = (int)(LDS_PER_CU / lds_bytes_for(v, m));
    int by_waves = 2048 / v.block;
    int b = std::max(1, std::min(by_lds, by_waves));
    if (s->blocks_per_cu > 0) b = std::min(b, s->blocks_per_cu);
    return b;
}

// Default kernel choice.  On small alphabets (DNA: 4 symbols) almost every window ends in a character of the
// pattern and the reference's one-character bad-symbol rule shifts by a few bytes: the walkers, not HBM, bound
// the scan (4 GiB ACGT, m = 64: 1.2 TB/s byte-wise walker, 2.0 skip loop, 2.3 skip loop + two workgroups per
// CU = variant 2).  The q-gram walkers apply the same rule to the window's last four / eight characters
// (walk_lane_qgram, walk_lane_qgram8): 5.7 TB/s with four, 6.4 with eight (whose lanes stay in step: hardly any
// 8-gram of the text occurs in the pattern); they need the canonical shift tables (below).
constexpr int VARIANT_QGRAM4 = 54;   // 4-gram walker, 76 KiB tiles
constexpr int VARIANT_QGRAM8 = 53;   // 8-gram walker, 76 KiB tiles
constexpr int VARIANT_SKIP_STEAL = 82;     // skip loop on 36 KiB tiles, two workgroups per CU, static shares + a stolen tail
constexpr int VARIANT_BIG_TILE_STEAL = 79; // ... with a stolen tail: the shorter the walk, the more a launch waits for its slowest workgroup
constexpr int VARIANT_SAD = 87;      // quad-SAD skip loop on the last 4 pattern bytes, 76 KiB tiles, stolen tail
constexpr int VARIANT_SAD8 = 88;     // ... on the last 8 (m >= 8)
constexpr int VARIANT_BIG_TILE = 29; // 76 KiB tiles: +2 % on large alphabets, but room for 512 parked matches per tile only

// `canonical`: the shift tables in use are the ones bmx_build_tables makes (always so when the caller
// passes none).  The q-gram walkers skip with a table of their own and only leave a verified window with
// the caller's shifts, so with tables that shift FURTHER than the canonical ones (unsafe ones: the
// reference kernel would miss matches) they would not reproduce the reference kernel's list.
// The walker and geometry for one search.  `sigma` = distinct byte values in samples of the TEXT (0: unknown).
// Measured, 2 GiB, TB/s (tools/variant_sweep.py):
//   printable text (sigma 95), byte-wise on 76 KiB tiles / skip loop on 36 KiB tiles with two workgroups per CU /
//   8-gram: m = 4: 3.6 / 4.4 / -, m = 6: 4.5 / 5.2 / - (4-gram: 3.9), m = 9: 5.4 / 6.0 / 2.6, m = 10: 5.5 / 6.0 / 3.4,
//   m = 12: 5.8 / 5.9 / 4.6, m = 16: 6.7 / - / 6.4;
//   ACGT, skip loop / 4-gram / 8-gram: m = 8: 2.1 / 2.3 / 1.6, m = 9: 2.4 / 2.6 / 2.7, m = 10: 2.3 / 3.0 / 3.7, m = 16: 2.3 / 4.1 / 6.4.
// The q-gram rules pay on small alphabets only, and whether the alphabet is small is a property of the text: the
// pattern's own distinct symbols (all there was to go by until round 2's second half) say "small" for every short
// English word -- `Tennessee` ran the 8-gram walker at 2.6 TB/s on English text.
// Patterns that are not walked at all (ShortTile, bmx_scan_common.h): with m <= 4 the shift tables cannot skip anything worth
// two dependent LDS reads per window, and one v_mqsad_u32_u8 tests four window starts against up to four pattern bytes
// (a reference byte of 0 is left out of the sums: a pattern of four bytes with a zero byte goes to the walkers).
bool short_pattern(const char *pat, int32_t m)
{
    if (m <= 3) return true;
    return m == 4 && pat[0] != 0 && pat[1] != 0 && pat[2] != 0 && pat[3] != 0;
}

// Distinct byte values of a pattern: what stands in for the text's alphabet until the text has been sampled (text_sigma).
int distinct_symbols(const char *pat, int32_t m)
{
    bool seen[256] = {};
    int distinct = 0;
    for (int i = 0; i < m; ++i)
        if (!seen[(unsigned char)pat[i]]) {
            seen[(unsigned char)pat[i]] = true;
            ++distinct;
        }
    return distinct;
}

// *sparse (short patterns only): matches are expected to be rare -- fewer than 64 per 76 KiB tile on a text that is uniform
// over `sigma` symbols -- so the kernel takes 76 KiB tiles (room for 512 parked matches) and looks for ANY match in a
// chunk before it works out which (ShortTile::mask).  A text that is not uniform (English: `is` is in one position of
// 150) only costs this choice what a dense result costs anyway: its tiles are counted and the fill pass writes the list.
int pick_variant(const ScanState *s, const char *pat, int32_t m, bool canonical, int sigma, bool *sparse, bool *use_short_kernel)
{
    *sparse = false;
    const bool is_short = short_pattern(pat, m);
    *use_short_kernel = is_short;
    const int distinct = distinct_symbols(pat, m);
    auto fits = [&](int vi) { return lds_bytes_for(g_variants[vi], m) <= LDS_PER_CU; };
    if (is_short) {
        double per_tile = 77824.0;
        for (int i = 0; i < m; ++i) per_tile /= (double)(sigma > 0 ? sigma : distinct);
        *sparse = per_tile < 64.0;
    }
    if (!s->auto_walker) { // an explicitly chosen variant
        const Variant &v = g_variants[s->variant];
        if (v.canon_minm && (!canonical || m < v.canon_minm)) return !is_short ? 2 : 0;
        if (v.canon_minm > 1 && is_short) return 0; // (a q-gram kernel's LDS budget has no room for the short-pattern kernel's parking buffer)
        if (v.canon_minm == 1) *use_short_kernel = false; // the quad-SAD skip loop takes any m
        return lds_bytes_for(v, m) <= LDS_PER_CU ? s->variant : 0; // buffers + halo do not fit at this m -> default
    }
    // Whether the text's alphabet is large is only known from the second search on a text on (text_sigma); until then the
    // pattern's own symbols have to do, and a word of five or more distinct letters is taken for text over a large alphabet
    // (DNA and binary patterns have at most four; round 2 asked for more than eight and sent every short English word to
    // the q-gram walkers on its first search).
    const bool large_alphabet = sigma > 0 ? sigma > 8 : distinct > 4;
    // (Whether it is also spread like random text no longer decides anything for the longer patterns, see below.)  Prose shows ~45 distinct bytes in the sample, printable-95 text all 95.  On
    // English-LIKE text (Zipf words over 27 symbols, tools/english_like.py) n-grams repeat, the quad-SAD skip loop stops where
    // the text shows the pattern's last four bytes, and frequent short words cost it twice what they cost the others (1 GiB,
    // ms, quad-SAD / skip loop on 36 KiB tiles / byte-wise: `esh` 0.62 / 0.43 / 0.31 (short-pattern kernel), ` esh ` 0.95 /
    // 0.52 / 0.95, a word of 6: 0.32 / 0.29 / 0.41, of 8: 0.22 / 0.23 / 0.29, of 10 + blank: 0.25 / 0.29 / 0.42, a rare one
    // of 12: 0.20 / 0.22 / 0.28): there it only took over from m = 8
    if (is_short) {
        // m = 2, 3, 4 with rare matches: the quad-SAD skip loop (4 GiB printable text, steady protocol, ms: m = 3: 0.61 against
        // 0.75 for the short-pattern kernel, m = 4: 0.60 against 0.72; m = 2 -- one position in 9,000 stops it -- since its stops
        // are verified out of registers and reported per lane: 0.70 against 0.77, before: 0.96); m = 1 and dense results: the
        // short-pattern kernel
        if (*sparse && canonical && m >= 2 && sigma > 64 && fits(VARIANT_SAD)) {
            *use_short_kernel = false;
            return VARIANT_SAD;
        }
        // everything else: the short-pattern kernel.  76 KiB tiles unless more than one position in eight matches (1 GiB,
        // whole search incl. the fill pass, ms, 68 / 76 KiB tiles: printable text, m = 1: 0.83 / 0.71; ACGT, m = 2: 0.80 /
        // 0.75, m = 3: 0.83 / 0.69, m = 4: 0.76 / 0.70; but ACGT, m = 1 -- 268 M matches -- 1.02 / 1.31: the fill pass of the
        // smaller tiles lays 512 matches out per turn, that of the larger ones 128)
        double density = 1.0;
        for (int i = 0; i < m; ++i) density /= (double)(sigma > 0 ? sigma : distinct);
        return density <= 0.125 && fits(VARIANT_BIG_TILE) ? VARIANT_BIG_TILE : 0;
    }
    if (large_alphabet) { // sparse by nature (9^-4 and less)
        // The quad-SAD skip loop (walk_lane_sad): no dependent LDS chain, ~1,500 cycles of walk per tile whatever m is, and
        // with the parking ledger its matches cost it nothing in the loop: 4 GiB printable text, steady protocol, one match
        // per MiB, ms: m = 16: 0.620 against 0.645-0.660 byte-wise (bench.py: 0.622 against 0.651), m = 64: 0.620 against
        // 0.646, m = 4..12: 0.605-0.61 against 0.63-0.93 for the skip loop on 36 KiB tiles.  It needs the canonical tables.
        // On English-LIKE text it took over from m = 8 only while a stop cost its wave ~2,000 cycles; with stops verified out of
        // registers (verify_quarter) it wins from m = 5 on (1 GiB, ms, quad-SAD / skip loop on 36 KiB tiles: ` esh ` 0.40 / 0.52,
        // a word of 6: 0.25 / 0.29, of 8: 0.18 / 0.23, two words of 16: 0.22 / 0.23): every pattern that is not "short".
        if (canonical && fits(VARIANT_SAD)) return VARIANT_SAD;
        // short patterns: long walks, 32 waves per CU hide them better (4 GiB printable text, ms, byte-wise 76 KiB / skip loop
        // 36 KiB / the latter with a stolen tail: m = 8: - / 0.742 / 0.750, m = 10: 0.768 / 0.726 / 0.690, m = 12: 0.727 / 0.752 /
        // 0.697, m = 13: 0.703 / 0.775 / 0.714, m = 15: 0.685 / 0.766 / 0.715)
        if (sigma > 0 && m <= 8 && distinct > 1) return 2;
        if (sigma > 0 && m <= 12 && distinct > 1) return VARIANT_SKIP_STEAL;
        // (4 GiB printable text, byte-wise walker, ms without / with the stolen tail: m = 16: 0.651 / 0.653, m = 24: 0.643 / 0.640,
        // m = 32: 0.648 / 0.633, m = 64: 0.668 / 0.643)
        if (m >= 28 && fits(VARIANT_BIG_TILE_STEAL)) return VARIANT_BIG_TILE_STEAL;
        return fits(VARIANT_BIG_TILE) ? VARIANT_BIG_TILE : 0;
    }
    // sigma^m small = matches every few bytes on a text over the pattern's alphabet (binary, m = 6: one position
    // in 64): what matters then is room to park them, and the default geometry has four times variant 2's
    double expect = 1.0;
    for (int i = 0; i < m && expect < 1e6; ++i) expect *= distinct;
    if (expect < 128.0) return 0;
    // DNA-like texts (4..8 symbols), m = 8..15: the quad-SAD skip loop on the pattern's last EIGHT bytes.  An 8-gram of such a
    // text equals the pattern's last one once in 65,536 positions (one stop per tile), and the loop's cost does not depend on m,
    // while the 8-gram WALKER shifts by m - 7 per window: 4 GiB ACGT, steady protocol, ms, walkers (4-gram at m = 8) / this: m = 8:
    // 1.79 / 0.70, m = 9: 1.56 / 0.70, m = 10: 1.15 / 0.69, m = 12: 0.86 / 0.69, m = 14: 0.74 / 0.69, m = 16: 0.684 / 0.688, m = 20:
    // 0.63 / 0.69, m >= 24: 0.61 / 0.69 (profiles/r03_acgt_sweep.jsonl).  Fewer than 4 symbols: every other window would stop.
    // (m = 5..7: the same loop with the whole pattern as its reference, every stop a match)
    if (canonical && m >= 5 && m < 16 && (sigma > 0 ? sigma : distinct) >= 4 && fits(VARIANT_SAD8)) return VARIANT_SAD8;
    if (canonical && m >= 9 && fits(VARIANT_QGRAM8)) return VARIANT_QGRAM8;
    if (canonical && m >= 6 && fits(VARIANT_QGRAM4)) return VARIANT_QGRAM4;
    return 2;
}

// Distinct byte values of the text at (d_text, n), as far as this context knows them: the ordering kernel of EVERY search
// samples 4 x 256 bytes of the text it has just scanned (free: four loads per thread of four waves) and
// bmx_search_device_finish files the count here.  0 = not seen yet: the first search on a text goes by the pattern's own
// symbols and is corrected one search later -- an enqueue never waits for the device (round 2 sampled a new text on the
// spot: one kernel and one stream synchronisation inside bmx_search_device_enqueue).
int text_sigma(const bmx_ctx *ctx, const void *d_text, uint64_t n)
{
    const ScanState *s = scan_of(ctx);
    if (n == 0 || !ctx->scan_knobs.text_sample) return 0;
    for (const auto &e : s->sampled)
        if (e.ptr == d_text && e.n == n) return e.sigma;
    return 0;
}

void remember_sigma(ScanState *s, const void *d_text, uint64_t n, int sigma)
{
    if (sigma <= 0 || d_text == nullptr) return;
    for (auto &e : s->sampled)
        if (e.ptr == d_text && e.n == n) {
            e.sigma = sigma; // the text as it is NOW (a caller may put another text at the same address: one search late, not wrong for ever)
            return;
        }
    auto &slot = s->sampled[s->sampled_next++ % ScanState::N_SAMPLED];
    slot.ptr = d_text, slot.n = n, slot.sigma = sigma;
}

// Convert the caller's int32 tables (or build them) into the kernel-argument layout.
int fill_tables(bmx::ScanTables &tab, const char *pat, int32_t m, const int32_t *good, const int32_t *bad,
                bool *canonical)
{
    std::vector<int32_t> own_good(m);
    int32_t own_bad[BMX_BAD_TABLE_SIZE];
    int rc = bmx_build_tables(pat, m, own_bad, own_good.data());
    if (rc != BMX_OK) return rc;
    *canonical = true;
    if (!good || !bad) {
        good = own_good.data();
        bad = own_bad;
    } else { // the caller's tables (like the reference passes its own): are they the canonical ones?
        for (int c = 0; c < BMX_BAD_TABLE_SIZE && *canonical; ++c) *canonical = bad[c] == own_bad[c];
        for (int k = 1; k < m && *canonical; ++k) *canonical = good[k] == own_good[k]; // good[0] is never read
    }
    // kernel1.cl:28 clamps (bad - k) to >= 1, and k == 0 uses bad as is
    for (int i = 0; i < m; ++i) // the kernels index 128-entry tables with pattern characters
        if ((unsigned char)pat[i] >= BMX_BAD_TABLE_SIZE) return BMX_ERR_DOMAIN;
    for (int c = 0; c < BMX_BAD_TABLE_SIZE; ++c) tab.bad[c] = (uint16_t)std::min(std::max(bad[c], 1), 65535);
    for (int k = 0; k < m; ++k) tab.good[k] = (uint16_t)std::min(std::max(good[k], 0), 65535);
    std::memcpy(tab.pat, pat, (size_t)m);
    return BMX_OK;
}

// First use, or a previous enqueue failed half way: zero the device counters (otherwise order_kernel has re-armed them).
int arm_counters(ScanState *s, hipStream_t stream)
{
    HIPCHK(hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), stream));
    HIPCHK(hipMemsetAsync(s->d_bucket_cnt, 0, bmx::ORDER_BUCKETS * sizeof(uint32_t), stream));
    HIPCHK(hipMemsetAsync(s->d_overflow, 0, 8 * sizeof(uint32_t), stream));
    return BMX_OK;
}

// Room for n_tiles tiles in the three per-tile arrays of the fill pass (grown on demand, kept).
int grow_tile_arrays(ScanState *s, uint64_t n_tiles)
{
    if (s->tile_cap >= n_tiles) return BMX_OK;
    if (s->d_tile_count) (void)hipFree(s->d_tile_count);
    if (s->d_tile_base) (void)hipFree(s->d_tile_base);
    if (s->d_wave_count) (void)hipFree(s->d_wave_count);
    s->d_tile_count = nullptr, s->d_tile_base = nullptr, s->d_wave_count = nullptr, s->tile_cap = 0;
    HIPCHK(hipMalloc(&s->d_tile_count, n_tiles * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&s->d_tile_base, n_tiles * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&s->d_wave_count, n_tiles * 16 * sizeof(uint32_t))); // (1024-thread workgroups)
    s->tile_cap = n_tiles;
    return BMX_OK;
}

// What the single and the several-patterns launch have in common: the text from its 16-byte boundary on, cut into tiles
// of `tile` bytes, n_starts window starts of which the caller owns, a pattern (the longest one) of m bytes, the list and
// the position buckets; no per-tile counts, no stamps.  The callers set the tables, stage_cap, the bucket shift and the
// multi-pattern fields.
void fill_geometry(bmx::ScanArgs &a, const ScanState *s, const void *d_text, uint64_t n, uint64_t n_starts, uint64_t base_offset,
                   uint64_t tile, int32_t m, uint64_t *out, uint64_t capacity)
{
    const uintptr_t addr = (uintptr_t)d_text;
    const uint64_t mis = addr & 15u;
    a.text16 = (const uint8_t *)(addr - mis);
    a.first = mis;
    a.own_end = mis + n_starts;
    a.data_end = mis + n;
    a.out_bias = base_offset - mis;
    a.tile_begin = 0; // mis < 16 <= tile
    a.tile_end = (a.own_end + tile - 1) / tile;
    a.out = out;
    a.cap = capacity;
    a.count = s->d_count;
    a.bucket_cnt = s->d_bucket_cnt;
    a.bucket_store = s->d_bucket_store;
    a.bucket_overflow = s->d_overflow;
    a.tile_count = nullptr;
    a.wave_count = nullptr;
    a.dense_enabled = 0;
    a.tile_base = nullptr;
    a.stamps = nullptr;
    a.m = (uint32_t)m;
    a.halo16 = ((uint32_t)(m - 1) + 15u) & ~15u;
}

} // namespace

extern "C" {

int bmx_set_order_overlap(bmx_ctx *ctx, int on)
{
    if (!ctx) return BMX_ERR_ARG;
    scan_of(ctx)->order_overlap = on != 0;
    return BMX_OK;
}

int bmx_set_variant(bmx_ctx *ctx, int variant, int blocks_per_cu)
{
    if (!ctx || variant < -1 || variant >= N_VARIANTS || blocks_per_cu < 0) return BMX_ERR_ARG;
    if (variant >= 0 && g_variants[variant].kernel == nullptr) { // a slot of libbmx_exp.so only
        set_err("bmx_set_variant: variant %d is not part of this library (experiments: libbmx_exp.so)", variant);
        return BMX_ERR_ARG;
    }
    ScanState *s = scan_of(ctx);
    if (variant == -1) { // back to the automatic choice (pick_variant)
        s->variant = 0;
        s->auto_walker = true;
        s->blocks_per_cu = blocks_per_cu;
        return BMX_OK;
    }
    s->variant = variant;
    s->auto_walker = false;
    s->blocks_per_cu = blocks_per_cu;
    return BMX_OK;
}

int bmx_variant_count(void) { return N_VARIANTS; }

int bmx_scan_geometry(bmx_ctx *ctx, int32_t m, uint64_t out[6])
{
    if (!ctx || !out || m < 1 || m > BMX_MAX_PATTERN) return BMX_ERR_ARG;
    const ScanState *s = scan_of(ctx);
    const Variant &v = g_variants[s->auto_walker ? s->last.variant : s->variant];
    out[0] = (uint64_t)blocks_per_cu_for(s, v, m) * ctx->num_cu;
    out[1] = v.block;
    out[2] = unit_bytes(v);
    out[3] = lds_bytes_for(v, m);
    out[4] = v.seg;
    out[5] = v.kind;
    return BMX_OK;
}

int bmx_last_search_sorted(bmx_ctx *ctx) { return ctx && scan_of(ctx)->last_sorted ? 1 : 0; }
int bmx_last_variant(bmx_ctx *ctx) { return ctx ? scan_of(ctx)->last.variant : -1; }

int bmx_stream_wait_last_scan(bmx_ctx *ctx, void *stream_v)
{
    if (!ctx) return BMX_ERR_ARG;
    const ScanState *s = scan_of(ctx);
    if (s->n_timed == 0) return BMX_OK; // nothing enqueued yet
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream_v, s->ev1[(s->n_timed - 1) % ScanState::EV_RING], 0));
    return BMX_OK;
}

float bmx_last_scan_ms(bmx_ctx *ctx)
{
    float ms = -1.0f;
    if (!ctx || !scan_of(ctx)->timed || bmx_scan_ms_history(ctx, &ms, 1) != 1) return -1.0f;
    return ms;
}

int bmx_scan_ms_history(bmx_ctx *ctx, float *ms_out, int32_t max_n)
{
    if (!ctx || !ms_out || max_n < 0) return BMX_ERR_ARG;
    const ScanState *s = scan_of(ctx);
    const uint64_t have = std::min<uint64_t>(s->n_timed, ScanState::EV_RING);
    const int n = (int)std::min<uint64_t>(have, (uint64_t)max_n);
    for (int i = 0; i < n; ++i) { // ms_out[0] = most recent
        const int slot = (int)((s->n_timed - 1 - i) % ScanState::EV_RING);
        if (hipEventSynchronize(s->ev1[slot]) != hipSuccess) return BMX_ERR_HIP;
        if (hipEventElapsedTime(&ms_out[i], s->ev0[slot], s->ev1[slot]) != hipSuccess) return BMX_ERR_HIP;
    }
    return n;
}

int bmx_search_device_enqueue(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own,
                              uint64_t base_offset, const char *pat, int32_t m, const int32_t *good,
                              const int32_t *bad, uint64_t *d_match_positions, uint64_t capacity,
                              void *stream_v)
{
    if (!ctx || !pat || m < 1 || m > BMX_MAX_PATTERN) return BMX_ERR_ARG;
    if (capacity > 0 && !d_match_positions) return BMX_ERR_ARG;
    if (n > 0 && !d_text) return BMX_ERR_ARG;
    ScanState *s = scan_of(ctx);
    hipStream_t stream = (hipStream_t)stream_v;
    HIPCHK(hipSetDevice(ctx->device));
    s->timed = false;
    if (s->order_forked) { // (a second search on this context without _finish in between: behind the first one's ordering kernel)
        HIPCHK(hipStreamWaitEvent(stream, s->ev_order, 0));
        s->order_forked = false;
    }
    if (!s->armed) {
        const int rc = arm_counters(s, stream);
        if (rc != BMX_OK) return rc;
    }
    s->armed = false;

    // windows that fit: starts 0 .. n-m; of those the caller owns [0, n_own)
    const uint64_t n_starts = n < (uint64_t)m ? 0 : std::min<uint64_t>(n - (uint64_t)m + 1, n_own);
    uint64_t *out = capacity ? d_match_positions : nullptr;
    uint32_t expect_tiles = 0; // stolen-tail kernels: the tiles the workgroups must have walked between them (order_kernel checks)

    if (n_starts > 0) {
        bmx::ScanArgs a;
        bool canonical = true;
        int rc = fill_tables(a.tab, pat, m, good, bad, &canonical);
        if (rc != BMX_OK) {
            s->armed = true; // nothing was launched
            return rc;
        }
        bool sparse = false, is_short = false; // is_short: the launch is the short-pattern kernel (ShortTile), which leaves per-tile counts
        const int vi = pick_variant(s, pat, m, canonical, text_sigma(ctx, d_text, n), &sparse, &is_short);
        s->last.variant = vi;
        const Variant &v = g_variants[vi];
        fill_geometry(a, s, d_text, n, n_starts, base_offset, unit_bytes(v), m, out, capacity);
        a.multi = nullptr;
        a.multi_bytes = a.K = a.bucket_stride = a.multi_qmask = 0;
        a.bucket_shift = 0;
        a.stage_cap = stage_cap_for(v, m);
        while (((n_starts - 1) >> a.bucket_shift) >= (uint64_t)bmx::ORDER_BUCKETS) ++a.bucket_shift;

        const uint32_t lds = lds_bytes_for(v, m);
        if (lds > LDS_PER_CU) {
            set_err("LDS need %u exceeds %u", lds, LDS_PER_CU);
            s->armed = true;
            return BMX_ERR_ARG;
        }
        auto kernel = !is_short ? v.kernel : v.kernel_short;
        int &attr = !is_short ? s->lds_attr_set[vi] : s->lds_attr_set_short[vi];
        if (attr < (int)lds) {
            HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr = (int)lds;
        }
        uint64_t nblocks = a.tile_end - a.tile_begin; // kind 0: one tile per workgroup at a time
        if (v.kind == 1) nblocks = (nblocks + v.block / 64 - 1) / (v.block / 64); // one piece per wave
        // (order overlap: one CU stays free for the ordering kernel of the search before -- the scan is HBM-bound, 255 CUs read as fast)
        const uint64_t max_grid = (uint64_t)blocks_per_cu_for(s, v, m) * (ctx->num_cu - (s->order_overlap && ctx->num_cu > 8 ? 1 : 0));
        uint32_t grid = (uint32_t)std::min<uint64_t>(nblocks, max_grid);
        if (ctx->scan_knobs.max_grid > 0) grid = std::min<uint32_t>(grid, (uint32_t)ctx->scan_knobs.max_grid); // (libbmx_exp.so only)

        // dense results: the scan counts per tile, bmx_search_device_finish runs the fill pass of this geometry
        auto fill = !short_pattern(pat, m) ? v.fill : v.fill_short;
        if (ctx->scan_knobs.no_dense) fill = nullptr; // (libbmx_exp.so only: A/B runs)
        s->last.fillable = false;
        if (fill != nullptr && a.stage_cap != 0) a.dense_enabled = 1u | (is_short && sparse ? 2u : 0u); // (count-only calls too: dense tiles are just counted)
        if (fill != nullptr && a.stage_cap != 0 && out != nullptr) {
            rc = grow_tile_arrays(s, a.tile_end - a.tile_begin);
            if (rc != BMX_OK) return rc;
            s->last.fillable = true;
            // the short-pattern scan leaves the counts itself -- unless matches are expected to be rare: then it spares itself the
            // per-tile bookkeeping, and the fill pass, should the result be dense after all, counts in a launch of its own
            if (is_short && !sparse) a.tile_count = s->d_tile_count, a.wave_count = s->d_wave_count;
        }
        const int slot = (int)(s->n_timed % ScanState::EV_RING);
        if (v.stamps) { // diagnostic build: room for 8 words per wave
            const uint64_t words = (uint64_t)grid * (v.block / 64) * 8;
            if (s->stamp_words < words) {
                if (s->d_stamps) HIPCHK(hipFree(s->d_stamps));
                HIPCHK(hipMalloc(&s->d_stamps, words * sizeof(unsigned long long)));
                s->stamp_words = words;
            }
            HIPCHK(hipMemsetAsync(s->d_stamps, 0, words * sizeof(unsigned long long), stream));
            a.stamps = s->d_stamps;
        }
        // (the two timing events ride on the kernel's own dispatch packet -- hipExtLaunchKernel -- instead of a barrier packet in
        // front of it and one behind: the command processor spent ~12 us per search on those)
        hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(v.block), lds, stream, s->ev0[slot], s->ev1[slot], 0, a);
        HIPCHK(hipGetLastError());
        if (is_short ? v.steal_short : v.steal) expect_tiles = (uint32_t)(a.tile_end - a.tile_begin);
        s->n_timed++;
        s->timed = true;
        s->last.args = a;
        s->last.grid = (int)grid;
        s->last.m = m;
        s->last.short_pat = short_pattern(pat, m); // (the fill pass of a short pattern is ShortTile's, whatever kernel scanned)
        s->last.counted = is_short && !sparse;
    } else {
        s->last.fillable = false;
    }

    // ascending list from the position buckets, {count, needs_sort} for the host, counters re-armed
    // bmx_set_order_overlap: the ordering kernel runs on a stream of the context's own behind the scan's stop event, so that the
    // caller's stream holds nothing but scans -- the next search's scan (another context, same stream) starts right behind this
    // one instead of behind this one's ordering kernel.  Not inside a graph capture (the fork would become part of the graph).
    hipStream_t order_stream = stream;
    bool forked = false;
    if (s->order_overlap && s->timed) { // (timed: a scan was launched just now, its stop event is the one to wait for)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cap);
        if (cap == hipStreamCaptureStatusNone) {
            if (!s->order_stream) HIPCHK(hipStreamCreateWithFlags(&s->order_stream, hipStreamNonBlocking));
            if (!s->ev_order) HIPCHK(hipEventCreateWithFlags(&s->ev_order, hipEventDisableTiming));
            HIPCHK(hipStreamWaitEvent(s->order_stream, s->ev1[(s->n_timed - 1) % ScanState::EV_RING], 0));
            order_stream = s->order_stream;
            forked = true;
        }
    }
    hipLaunchKernelGGL(bmx::order_kernel, dim3(1), dim3(bmx::ORDER_THREADS), 0, order_stream, out, capacity, s->d_count,
                       s->d_bucket_cnt, s->d_bucket_store, s->d_overflow, s->d_status, s->h_status_dev,
                       ++s->seq, (uint64_t *)nullptr, 1u, ctx->scan_knobs.text_sample ? (const uint8_t *)d_text : nullptr, n,
                       expect_tiles);
    s->last_text = d_text, s->last_text_n = n;
    HIPCHK(hipGetLastError());
    if (forked) HIPCHK(hipEventRecord(s->ev_order, s->order_stream));
    s->order_forked = forked;
    s->armed = true;
    return BMX_OK;
}

int bmx_search_device_finish(bmx_ctx *ctx, uint64_t *d_match_positions, uint64_t capacity,
                             uint64_t *n_matches, void *stream_v)
{
    if (!ctx) return BMX_ERR_ARG;
    ScanState *s = scan_of(ctx);
    hipStream_t stream = (hipStream_t)stream_v;
    HIPCHK(hipSetDevice(ctx->device));
    // order_kernel stores {count, needs_sort} and then the sequence number straight into
    // pinned host memory: poll for it instead of paying a D2H copy plus a stream
    // synchronisation (~25 us) per search.  The stream is queried now and then so that
    // a failed launch cannot hang the caller.
    {
        const uint64_t want = s->seq;
        uint64_t spins = 0;
        while (__atomic_load_n(&s->h_status[2], __ATOMIC_ACQUIRE) != want) {
            if ((++spins & 0xFFFF) == 0) {
                hipError_t q = hipStreamQuery(s->order_forked ? s->order_stream : stream);
                if (q != hipSuccess && q != hipErrorNotReady) {
                    set_err("scan failed: %s", hipGetErrorString(q));
                    s->armed = false;
                    return BMX_ERR_HIP;
                }
                if (q == hipSuccess && __atomic_load_n(&s->h_status[2], __ATOMIC_ACQUIRE) != want) {
                    set_err("bmx_search_device_finish: nothing enqueued on this stream");
                    return BMX_ERR_ARG;
                }
            }
            __builtin_ia32_pause();
        }
    }
    s->order_forked = false; // (the ordering kernel is done: whatever follows on `stream` sees its list)
    const uint64_t total = s->h_status[0];
    const bool needs_sort = s->h_status[1] == 1;
    remember_sigma(s, s->last_text, s->last_text_n, (int)s->h_status[6]);
    if (s->h_status[3] != 0) { // finish_parked (bmx_scan_common.h): matches were dropped, the list is not the answer
        if (s->h_status[3] & 2)
            set_err("scan kernel: the workgroups did not walk every tile exactly once between them (stolen tail); result discarded");
        else
            set_err("scan kernel: a workgroup waited longer than its bound for a slot reservation; result discarded");
        if (n_matches) *n_matches = 0;
        return BMX_ERR_HIP;
    }
    s->last_sorted = needs_sort;
    if (n_matches) *n_matches = total;
    const uint64_t stored = std::min(total, capacity);
    // A complete but unordered list (clustered matches overflowed the position buckets) can be sorted or written
    // anew by the fill pass; the fill pass costs a second read of the text (~n / 4 TB/s), the radix sort ~0.1 ms +
    // 65 ns per thousand matches (16.8 M matches: 1.1 ms).
    // (Only for patterns of 1-3 bytes, whose fill pass tests every position from registers: the byte-wise walker
    // of the longer ones, run twice over a small alphabet, is slower than the sort -- 1 GiB ACGT, m = 4: 3.3 vs 1.9 ms.)
    const bool fill_instead_of_sort = needs_sort && s->last.fillable && s->last.short_pat && d_match_positions && capacity > 0 &&
                                      (double)(s->last.args.data_end) / 4.0e9 < 0.1 + (double)stored * 6.5e-8;
    if ((s->h_status[1] == 2 || fill_instead_of_sort) && d_match_positions && capacity > 0) {
        // Dense result: some tile held more matches than its workgroup can park in LDS.  The scan has counted every
        // tile's matches; their exclusive scan says where each tile's matches go, and the fill pass -- the same
        // geometry, every tile walked twice: count per lane, scan over the workgroup, write -- puts them there in
        // ascending order.  The text is read a second time; nothing is sorted, no atomic is issued.
        if (!s->last.fillable) {
            set_err("bmx_search_device_finish: dense result without a fill pass");
            return BMX_ERR_HIP;
        }
        const Variant &v = g_variants[s->last.variant];
        auto fill = !s->last.short_pat ? v.fill : v.fill_short;
        bmx::ScanArgs a = s->last.args;
        const uint64_t n_tiles = a.tile_end - a.tile_begin;
        auto fill_count = !s->last.short_pat ? v.fill_count : v.fill_count_short;
        a.out = d_match_positions;
        a.cap = capacity;
        a.stage_cap = 0;
        a.tile_base = s->d_tile_base;
        a.tile_count = s->d_tile_count;
        a.dense_enabled = 0;
        // (m = 1..3: 1 KiB per wave in the parking area's place, where the fill pass lays a round's matches out in slot order)
        const uint32_t lds = lds_bytes_with(v, s->last.m, s->last.short_pat ? (v.seg > 68 ? 256u : 1024u) : 0u); // (ShortTile::BATCH x 4)
        HIPCHK(hipFuncSetAttribute((const void *)fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (!s->last.counted) { // (the short-pattern kernel has left the counts already)
            a.wave_count = s->d_wave_count;
            HIPCHK(hipFuncSetAttribute((const void *)fill_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(fill_count, dim3(s->last.grid), dim3(v.block), lds, stream, a);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(bmx::tile_scan_kernel, dim3(1), dim3(bmx::ORDER_THREADS), 0, stream, s->d_tile_count, n_tiles,
                           s->d_tile_base);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(fill, dim3(s->last.grid), dim3(v.block), lds, stream, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        s->last_sorted = false;
        return total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    }
    if (needs_sort && stored > 1 && d_match_positions) {
        // a position bucket overflowed (clustered / dense matches): order the complete unordered list
        if (stored <= (uint64_t)bmx::SMALL_SORT_MAX) {
            hipLaunchKernelGGL(bmx::small_sort_kernel, dim3(1), dim3(bmx::SMALL_SORT_THREADS),
                               bmx::SMALL_SORT_MAX * sizeof(uint64_t), stream, d_match_positions, (uint32_t)stored);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(stream));
        } else {
            // (positions are below base offset + text length)
            const uint64_t top = s->last.args.out_bias + s->last.args.own_end; // (aligned coordinate + bias = reported offset)
            unsigned bits = 1;
            while (bits < 64 && (top >> bits) != 0) ++bits;
            size_t errlen = 0;
            char *err = bmx_internal_error_buffer(&errlen);
            int rc = bmx_internal_radix_sort(d_match_positions, stored, bits, &s->d_sort_scratch, &s->sort_scratch_bytes, stream, err, errlen);
            if (rc != BMX_OK) return rc;
        }
    }
    return total > capacity ? BMX_ERR_CAPACITY : BMX_OK; // (count-only calls too: capacity 0 holds none of a non-empty list)
}

int bmx_search_device(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                      const char *pat, int32_t m, const int32_t *good, const int32_t *bad,
                      uint64_t *d_match_positions, uint64_t capacity, uint64_t *n_matches, void *stream)
{
    int rc = bmx_search_device_enqueue(ctx, d_text, n, n_own, base_offset, pat, m, good, bad,
                                       d_match_positions, capacity, stream);
    if (rc != BMX_OK) return rc;
    return bmx_search_device_finish(ctx, d_match_positions, capacity, n_matches, stream);
}

// ---- several patterns in one pass ----------------------------------------
namespace {
constexpr uint32_t MULTI_BLOB_MAX = bmx::MAX_MULTI * (512 + 2 * ((BMX_MAX_PATTERN + 7) & ~7) + BMX_MAX_PATTERN + 32);
// (static tile shares + a stolen tail, scan_kernel MODE 12, like the single-pattern kernels: round 3)
const auto g_multi_kernel = bmx::scan_kernel<1024, 68, 2, 12, 20>;
const Variant g_multi_variant = {0, 1024, 68, 2, 0, 0, false, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
// the same pass with the 8-gram rule for the patterns over small alphabets (one 4 KiB shift table each in LDS: 52 KiB tiles)
const auto g_multi_kernel_q = bmx::scan_kernel<1024, 52, 2, 12, 21>;
const Variant g_multi_variant_q = {0, 1024, 52, 2, 0, 0, false, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
} // namespace

int bmx_search_device_multi(bmx_ctx *ctx, const void *d_text, uint64_t n, uint64_t n_own, uint64_t base_offset,
                            const char *const *pats, const int32_t *ms, int32_t K, uint64_t *d_match_positions,
                            uint64_t capacity, uint64_t *n_matches, uint64_t *first, void *stream_v)
{
    if (!ctx || !pats || !ms || !n_matches || !first || K < 1 || K > BMX_MAX_MULTI) return BMX_ERR_ARG;
    if ((capacity > 0 && !d_match_positions) || (n > 0 && !d_text)) return BMX_ERR_ARG;
    int32_t m_max = 0;
    for (int k = 0; k < K; ++k) {
        if (!pats[k] || ms[k] < 1 || ms[k] > BMX_MAX_PATTERN) return BMX_ERR_ARG;
        m_max = std::max(m_max, ms[k]);
        n_matches[k] = first[k] = 0;
    }
    ScanState *s = scan_of(ctx);
    hipStream_t stream = (hipStream_t)stream_v;
    HIPCHK(hipSetDevice(ctx->device));
    // the exact way, pattern by pattern: what the one-pass result must equal, and what it falls back to
    auto one_by_one = [&]() -> int {
        uint64_t at = 0, total = 0;
        for (int k = 0; k < K; ++k) {
            uint64_t got = 0;
            const uint64_t room = capacity > at ? capacity - at : 0;
            const int rc = bmx_search_device(ctx, d_text, n, n_own, base_offset, pats[k], ms[k], nullptr, nullptr,
                                             room ? d_match_positions + at : nullptr, room, &got, stream);
            if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) return rc;
            first[k] = at;
            n_matches[k] = got;
            total += got;
            at += std::min(got, room);
        }
        return total > capacity ? BMX_ERR_CAPACITY : BMX_OK;
    };
    if (K == 1 || capacity == 0) return one_by_one();

    // tables of every pattern (BoyreMoore.cpp:150-190 each), laid out as the kernel keeps them in LDS
    std::vector<uint8_t> blob;
    bmx::ScanArgs a;
    uint64_t n_starts_max = 0;
    uint32_t qmask = 0, many_symbols = 0, sadmask = 0; // sadmask: bit k = quad-SAD walk for pattern k, bit 8 + k = ... on its last eight bytes
    int distinct_of[BMX_MAX_MULTI] = {};
    const uint64_t mis = (uintptr_t)d_text & 15u; // (the kernels count from the text's 16-byte boundary: fill_geometry)
    for (int k = 0; k < K; ++k) {
        const int32_t m = ms[k];
        int32_t bad[BMX_BAD_TABLE_SIZE];
        std::vector<int32_t> good(m);
        const int rc = bmx_build_tables(pats[k], m, bad, good.data());
        if (rc != BMX_OK) return rc;
        const size_t off = blob.size();
        blob.resize(off + 512 + (((size_t)2 * m + 15) & ~(size_t)15) + (((size_t)m + 15) & ~(size_t)15), 0);
        uint16_t *b16 = reinterpret_cast<uint16_t *>(blob.data() + off);
        for (int c = 0; c < 256; ++c) b16[c] = (uint16_t)(c < BMX_BAD_TABLE_SIZE ? std::max(bad[c], 1) : m);
        uint16_t *g16 = b16 + 256;
        for (int i = 0; i < m; ++i) g16[i] = (uint16_t)std::max(good[i], 0);
        std::memcpy(blob.data() + off + 512 + (((size_t)2 * m + 15) & ~(size_t)15), pats[k], (size_t)m);
        a.multi_off[k] = (uint16_t)off;
        a.multi_m[k] = (uint16_t)m;
        // the 8-gram rule for this pattern?  As pick_variant decides for a single search: few distinct symbols, m >= 9
        const int distinct = distinct_of[k] = distinct_symbols(pats[k], m);
        if (m >= 9 && distinct >= 2 && distinct <= 8) qmask |= 1u << k;
        if (distinct > 4) many_symbols |= 1u << k;
        const uint64_t n_starts = n < (uint64_t)m ? 0 : std::min<uint64_t>(n - (uint64_t)m + 1, n_own);
        a.multi_own_end[k] = mis + n_starts;
        n_starts_max = std::max(n_starts_max, n_starts);
    }
    for (int k = K; k < BMX_MAX_MULTI; ++k) a.multi_off[k] = a.multi_m[k] = 0, a.multi_own_end[k] = 0;
    if (n_starts_max == 0) return BMX_OK;
    if (!s->d_multi) HIPCHK(hipMalloc(&s->d_multi, MULTI_BLOB_MAX));
    if (!s->h_multi) HIPCHK(hipHostMalloc(&s->h_multi, MULTI_BLOB_MAX, hipHostMallocDefault));
    // (through pinned memory the copy is asynchronous and nothing waits for it here; the buffer is free again when this call
    // returns -- it ends with the wait for the search's status word, which the kernels behind the copy write)
    std::memcpy(s->h_multi, blob.data(), blob.size());
    HIPCHK(hipMemcpyAsync(s->d_multi, s->h_multi, blob.size(), hipMemcpyHostToDevice, stream));

    s->timed = false;
    if (!s->armed) {
        const int rc = arm_counters(s, stream);
        if (rc != BMX_OK) return rc;
    }
    s->armed = false;
    if (ctx->scan_knobs.multi_no_qgram) qmask = 0; // (libbmx_exp.so only: A/B runs)
    {   // which walker per pattern, by the TEXT's alphabet as far as it is known (pick_variant's rule): large and spread like
        // random text -> the quad-SAD skip loop; prose-like -> quad-SAD from m = 8; small -> the 8-gram rule from m = 9
        const int sigma = text_sigma(ctx, d_text, n);
        if (sigma > 8) qmask = 0;
        for (int k = 0; k < K; ++k) {
            const bool large = sigma > 0 ? sigma > 8 : ((many_symbols >> k) & 1u) != 0;
            const bool uniform_like = sigma > 0 ? sigma > 64 : ((many_symbols >> k) & 1u) != 0;
            if (large && (uniform_like || ms[k] >= 8) && !ctx->scan_knobs.multi_no_qgram) sadmask |= 1u << k;
            // DNA-like text (4..8 symbols), m = 8..15: the quad-SAD loop on the last eight bytes (pick_variant's rule)
            const int s_eff = sigma > 0 ? sigma : distinct_of[k];
            if (!large && s_eff >= 4 && ms[k] >= 8 && ms[k] < 16 && !ctx->scan_knobs.multi_no_qgram) sadmask |= 0x101u << k;
        }
        qmask &= ~sadmask;
    }
    const uint32_t q_bytes = (uint32_t)__builtin_popcount(qmask) * bmx::QGRAM_TABLE;
    // LDS of one workgroup without the parking area: two tiles with their halo, every pattern's tables, the shift tables of the
    // 8-gram rule, and the single-pattern block
    auto lds_without_parking = [&](const Variant &geometry, uint32_t shift_tables) {
        const uint32_t halo = ((uint32_t)(m_max - 1) + 15u) & ~15u;
        return 2u * ((uint32_t)unit_bytes(geometry) + halo) + (uint32_t)blob.size() + shift_tables + 512 +
               ((((uint32_t)m_max + 7u) & ~7u) * 2) + (((uint32_t)m_max + 15u) & ~15u) + 256 + 256;
    };
    // (the tables of long patterns can leave no room for the shift tables beside two 52 KiB tiles: byte-wise then)
    if (lds_without_parking(g_multi_variant_q, q_bytes) + 2 * 64 * 8 + 32 > LDS_PER_CU) qmask = 0;
    const bool with_q = qmask != 0;
    const Variant &v = with_q ? g_multi_variant_q : g_multi_variant;
    const auto kernel = with_q ? g_multi_kernel_q : g_multi_kernel;
    bool canonical = true;
    int rc = fill_tables(a.tab, pats[0], ms[0], nullptr, nullptr, &canonical); // (unused by the multi walk; keeps the block defined)
    if (rc != BMX_OK) {
        s->armed = true;
        return rc;
    }
    // (dense_enabled stays 0: dense tiles take the direct path, raise the overflow flag and send the call the exact way)
    fill_geometry(a, s, d_text, n, n_starts_max, base_offset, unit_bytes(v), m_max, d_match_positions, capacity);
    a.multi = s->d_multi;
    a.multi_bytes = (uint32_t)blob.size();
    a.multi_qmask = qmask | (sadmask << 8);
    a.K = (uint32_t)K;
    uint32_t kp2 = 1;
    while ((int)kp2 < K) kp2 <<= 1;
    a.bucket_stride = (uint32_t)bmx::ORDER_BUCKETS / kp2;
    a.bucket_shift = 0;
    while (((n_starts_max - 1) >> a.bucket_shift) >= (uint64_t)a.bucket_stride) ++a.bucket_shift;
    const uint32_t lds_fixed = lds_without_parking(v, with_q ? q_bytes : 0u);
    a.stage_cap = 0;
    for (uint32_t cap = 512; cap >= 64 && a.stage_cap == 0; cap /= 2)
        if (lds_fixed + 2 * cap * 8 + 32 <= LDS_PER_CU) a.stage_cap = cap;
    const uint32_t lds = lds_fixed + (a.stage_cap ? 2 * a.stage_cap * 8 + 32 : 0);
    if (lds > LDS_PER_CU) {
        s->armed = true;
        return one_by_one();
    }
    if (s->multi_attr[with_q] < (int)lds) { // (per context = per device: a function attribute is the device's)
        HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        s->multi_attr[with_q] = (int)lds;
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(a.tile_end - a.tile_begin, (uint64_t)ctx->num_cu);
    const int slot = (int)(s->n_timed % ScanState::EV_RING);
    HIPCHK(hipEventRecord(s->ev0[slot], stream));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(v.block), lds, stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev1[slot], stream));
    s->n_timed++;
    s->timed = true;
    s->last.fillable = false;
    hipLaunchKernelGGL(bmx::order_kernel, dim3(1), dim3(bmx::ORDER_THREADS), 0, stream, d_match_positions, capacity, s->d_count,
                       s->d_bucket_cnt, s->d_bucket_store, s->d_overflow, s->d_status, s->h_status_dev, ++s->seq,
                       s->h_status_dev + 8, a.bucket_stride / 8u, (const uint8_t *)d_text, n, (uint32_t)(a.tile_end - a.tile_begin));
    s->last_text = d_text, s->last_text_n = n;
    HIPCHK(hipGetLastError());
    s->armed = true;
    uint64_t total = 0;
    rc = bmx_search_device_finish(ctx, nullptr, 0, &total, stream); // waits for the status word; no list handling here
    if (rc != BMX_OK && rc != BMX_ERR_CAPACITY) return rc;
    if (s->h_status[1] != 0 || total > capacity) return one_by_one(); // unordered / dense / too many: the exact way
    // where each pattern's list begins: written by the ordering kernel into the pinned status block in front of the sequence
    // number the wait above has seen (no copy, no stream synchronisation)
    const uint64_t *h_first = s->h_status + 8;
    for (int k = 0; k < K; ++k) {
        first[k] = h_first[k];
        n_matches[k] = (k + 1 < (int)kp2 ? h_first[k + 1] : total) - h_first[k];
    }
    return BMX_OK;
}

int bmx_count_to_device(bmx_ctx *ctx, uint64_t *d_dst, void *stream_v)
{
    if (!ctx || !d_dst) return BMX_ERR_ARG;
    const ScanState *s = scan_of(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    // bmx_set_order_overlap: the count (and the list) come from the ordering kernel on the context's own stream, which `stream`
    // is not ordered behind -- the copy, and with it the exchange the caller puts behind it, wait for that kernel
    if (s->order_forked) HIPCHK(hipStreamWaitEvent((hipStream_t)stream_v, s->ev_order, 0));
    HIPCHK(hipMemcpyAsync(d_dst, s->d_status + 2, sizeof(uint64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream_v));
    return BMX_OK;
}

int bmx_scan_stamps(bmx_ctx *ctx, uint64_t *out, uint64_t max_words)
{
    if (!ctx || !out) return BMX_ERR_ARG;
    const ScanState *s = scan_of(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t n = std::min(max_words, s->stamp_words);
    if (n) HIPCHK(hipMemcpy(out, s->d_stamps, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return (int)std::min<uint64_t>(n, 0x7fffffff);
}

} // extern "C"
