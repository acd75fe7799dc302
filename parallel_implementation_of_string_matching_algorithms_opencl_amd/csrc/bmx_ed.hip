// bmx_ed.hip -- host side of the single-pair edit distance (bmx_edit_distance_device, include/bmx.h): the
// schedule table, the band pipeline (one launch, bmx_ed_bits3_kernel.h by default) and the tile schedule it falls back
// to.  Keeps the band pipeline's workspace, the last device time and its own event pair between calls.  The argument
// checks, the empty strings and the context are the shim's (bmx_shim.hip); everything here runs on a valid context's
// device with two non-empty strings.  Compiled twice, as the shim is: the kernels carry BMX_EXPERIMENTS code (stamps).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_ed_band_kernel.h"
#include "bmx_ed_bits3_kernel.h"
#include "bmx_ed_kernel.h"
#ifdef BMX_EXPERIMENTS
#include "bmx_ed_bits_kernel.h"
#include "bmx_ed_bits2_kernel.h"
#endif

namespace {

struct EdVariant {
    int c, r;                              // tile schedules: 64*c columns x r rows per wave
    void (*kernel)(const bmx::EdArgs);     // one tile diagonal per launch, from the top-left corner (nullptr: this slot is
                                           // not built into this library)
    void (*dual)(const bmx::EdArgs);       // a forward and a mirrored tile diagonal per launch (nullptr: none)
    int band_c;                            // band pipeline: 64*band_c columns per wave
    void (*band)(const bmx::EdBandArgs);   // the whole table in one launch: pipeline of column bands, both directions
    void (*band16)(const bmx::EdBandArgs); // same with 16-row hand-over groups (libbmx_exp.so: knob ed_group)
    uint32_t band_lds = 0;                 // dynamic LDS of the band kernel (the bit-parallel band's Eq table)
    int band_lag = 180;                    // rows a band trails its predecessor by (measured; places the cut rows)
    int band_threads = 64;                 // threads of a band's workgroup (256: a main wave and its helpers)
};

// The slot numbers are stable (tools/ and DESIGN.md section 7 refer to them), and the scan kernels' rule holds
// (bmx_shim.hip): the PRODUCT library only contains what the library's choice runs -- schedule 13, slot 0 as its alias,
// and their 4 x 256 tiles behind +16 / +32; every schedule that lost exists in libbmx_exp.so alone, and
// bmx_internal_ed_variant_ok refuses a slot that is not built.  Schedule 13 won at every shape; DESIGN.md section 7 has
// the history of the step model that used to choose among the bands.
#ifdef BMX_EXPERIMENTS
#define BMX_ED_EXP(...) __VA_ARGS__ // a row of libbmx_exp.so alone
#define BMX_ED_EXP_KERNEL(...) __VA_ARGS__
#else
#define BMX_ED_EXP(...) {0, 0, nullptr, nullptr, 0, nullptr, nullptr}
#define BMX_ED_EXP_KERNEL(...) nullptr
#endif
#define BMX_ED(C_, R_, BC_)                                                                                                \
    BMX_ED_EXP({C_, R_, bmx::ed_tile_kernel<C_, R_, true>, bmx::ed_dual_kernel<C_, R_>, BC_, bmx::ed_band_kernel<BC_, 32>, \
                bmx::ed_band_kernel<BC_, 16>})
// the bit-parallel band with a helper wave per band that talks to the neighbouring bands (bmx_ed_bits3_kernel.h): groups
// of 32 / 16 steps; tiles (fallback, +16, +32) of 256 rows x 256 columns
#define BMX_ED_BITS3                                                                                              \
    {4, 256, bmx::ed_tile_kernel<4, 256, true>, bmx::ed_dual_kernel<4, 256>, 32, bmx::ed_bits3_kernel<32, 2>,    \
     BMX_ED_EXP_KERNEL(bmx::ed_bits3_kernel<16, 2>), bmx::ed_bits3_lds(32, 2), 310, 256}
const EdVariant g_ed_variants[] = {
    BMX_ED_BITS3,      // 0: the library's choice = 13
    BMX_ED(4, 128, 4), // 1
    BMX_ED(8, 256, 8), // 2
    BMX_ED(4, 384, 5), // 3
    BMX_ED(6, 256, 6), // 4: bands of 384 columns (the default before the bit-parallel bands)
    // 5: the first version (ds_bpermute shuffle, predicated steps)
    BMX_ED_EXP({4, 256, bmx::ed_tile_kernel<4, 256, false>, nullptr, 0, nullptr, nullptr}),
    BMX_ED(4, 512, 7), // 6
    BMX_ED(3, 256, 3), // 7
    // 8: the bit-parallel band (bmx_ed_bits_kernel.h): 2048 columns per wave, 32 per lane as two words of differences
    BMX_ED_EXP({4, 256, bmx::ed_tile_kernel<4, 256, true>, bmx::ed_dual_kernel<4, 256>, 32, bmx::ed_bits_kernel<32, 1>,
                bmx::ed_bits_kernel<16, 1>, bmx::ED_BITS_LDS, 190}),
    // 9: ... two rows per step (a window entry = two rows); 10: four.  Measured at 64k x 64k (profiles/r03_ed_*.jsonl), ms at the
    // best assumed lag: one row 2.80-2.97 (lag 180-200), two rows 2.58 (350-400), four 2.67 (800): a step is ~40 / 57 / 90
    // instructions at ~5.5 cycles each for a lone wave (the recurrence is one dependent chain), so rows per step only
    // amortise the ~17 instructions around it
    BMX_ED_EXP({4, 256, bmx::ed_tile_kernel<4, 256, true>, bmx::ed_dual_kernel<4, 256>, 32, bmx::ed_bits_kernel<32, 2>,
                bmx::ed_bits_kernel<16, 2>, bmx::ED_BITS_LDS, 380}),
    BMX_ED_EXP({4, 256, bmx::ed_tile_kernel<4, 256, true>, bmx::ed_dual_kernel<4, 256>, 32, bmx::ed_bits_kernel<32, 4>,
                bmx::ed_bits_kernel<16, 4>, bmx::ED_BITS_LDS, 800}),
    // 11, 12: the bit-parallel band with the hand-over, the edge collector and the row windows out of the step
    // (bmx_ed_bits2_kernel.h): two rows / one row per step
    BMX_ED_EXP({4, 256, bmx::ed_tile_kernel<4, 256, true>, bmx::ed_dual_kernel<4, 256>, 32, bmx::ed_bits2_kernel<32, 2>,
                bmx::ed_bits2_kernel<16, 2>, bmx::ed_bits2_lds(32, 2), 380}),
    BMX_ED_EXP({4, 256, bmx::ed_tile_kernel<4, 256, true>, bmx::ed_dual_kernel<4, 256>, 32, bmx::ed_bits2_kernel<32, 1>,
                bmx::ed_bits2_kernel<16, 1>, bmx::ed_bits2_lds(32, 1), 190}),
    BMX_ED_BITS3, // 13
};
#ifdef BMX_EXPERIMENTS
void (*const g_ed_step_experiments[])(const bmx::EdBandArgs) = {
    bmx::ed_bits3_kernel<32, 2, 0>,  bmx::ed_bits3_kernel<32, 2, 1>,  bmx::ed_bits3_kernel<32, 2, 2>,  bmx::ed_bits3_kernel<32, 2, 4>,
    bmx::ed_bits3_kernel<32, 2, 8>,  bmx::ed_bits3_kernel<32, 2, 16>, bmx::ed_bits3_kernel<32, 2, 3>,  bmx::ed_bits3_kernel<32, 2, 11>,
    bmx::ed_bits3_kernel<32, 2, 27>,
};
#endif
constexpr int N_ED_VARIANTS = sizeof(g_ed_variants) / sizeof(g_ed_variants[0]);
constexpr int ED_ONE_DIRECTION = 16; // flag on the variant number: tiles, from the top-left corner only
constexpr int ED_TILES = 32;         // flag: tiles from both corners (one launch per pair of tile diagonals)
constexpr int ED_FLAGS = ED_ONE_DIRECTION | ED_TILES;
constexpr uint64_t ED_BAND_WS_LIMIT = 16ull << 30; // bytes of right-column storage the band pipeline may take
constexpr uint64_t ED_BAND_WS_KEEP = 1ull << 30;   // workspaces up to this size stay in the state between calls
constexpr int ED_STAMP_WORDS = 24 + 64 * 4; // cycle counts of one band of a band-pipeline run + a hand-over's timeline

struct EdHost {
    void *ws = nullptr; // band pipeline workspace, kept between calls while it is small
    uint64_t ws_bytes = 0;
    uint64_t ws_shape[3] = {0, 0, 0}; // (la, lb, W) of the call that last used it: same layout, stale tags only
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // around the kernels of a call
    float last_ms = -1.0f;
#ifdef BMX_EXPERIMENTS
    uint64_t stamps[ED_STAMP_WORDS] = {}; // of the last band-pipeline run (bmx_exp_ed_stamps)
#endif
};

// Band pipeline (bmx_ed_band_kernel.h).  Returns BMX_OK with *used = false if it does not apply
// (workspace too large / allocation refused): the caller then takes the tile schedule.
int ed_band_run(EdHost *st, const bmx_ed_knobs *knobs, const EdVariant &v, const void *d_a, uint64_t la, const void *d_b, uint64_t lb,
                hipStream_t stream, uint32_t *h_result, bool *used, char *err, size_t errlen)
{
    *used = false;
    const uint32_t W = 64u * v.band_c;
    const uint32_t bands = (uint32_t)((la + W - 1) / W);
    // [right columns: 2 x (bands + 1) x (lb + 1) entries of 8 B | cut rows: 2 x bands x (W + 1) | cut | err | result]
    const uint64_t rc_entries = 2ull * (bands + 1) * (lb + 1), stair_words = 2ull * bands * (W + 1);
    const uint64_t stamp_at = (rc_entries * sizeof(uint64_t) + (stair_words + bands + 2) * sizeof(uint32_t) + 7) / 8 * 8;
    const uint64_t bytes = stamp_at + ED_STAMP_WORDS * sizeof(uint64_t);
    if (bytes > ED_BAND_WS_LIMIT || la + lb >= (1ull << 31)) return BMX_OK; // (the kernel's F = D - r - c is an int32)
    // Workspace: kept in the state between calls while it is small (a fresh hipMalloc + hipFree per
    // call costs 0.3 ms next to a 4 ms kernel).  Entries are valid only with this call's tag; tags are
    // unique per process, so a workspace reused for the same shape needs no clearing -- a new allocation
    // (or another shape) is zeroed first.
    static std::atomic<uint32_t> g_tag{0};
    uint32_t tag = ++g_tag;
    bool fresh = false;
    uint64_t *ws = nullptr;
    if (st->ws && st->ws_bytes >= bytes && tag != 0) {
        ws = (uint64_t *)st->ws;
        // another shape lays the regions out differently: what was a cut row or a result word may now
        // be read as an entry, so the storage is cleared like a new one
        fresh = st->ws_shape[0] != la || st->ws_shape[1] != lb || st->ws_shape[2] != W;
    } else {
        if (st->ws) (void)hipFree(st->ws);
        st->ws = nullptr;
        st->ws_bytes = 0;
        if (hipMalloc(&ws, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return BMX_OK;
        }
        fresh = true;
        if (tag == 0) tag = ++g_tag; // 2^32 calls later: start over on zeroed storage
        if (bytes <= ED_BAND_WS_KEEP) {
            st->ws = ws;
            st->ws_bytes = bytes;
        }
    }
    const bool keep = st->ws == (void *)ws;
    if (keep) {
        st->ws_shape[0] = la;
        st->ws_shape[1] = lb;
        st->ws_shape[2] = W;
    }
    bmx::EdBandArgs a = {};
    a.a = (const uint8_t *)d_a;
    a.b = (const uint8_t *)d_b;
    a.la = (uint32_t)la;
    a.lb = (uint32_t)lb;
    a.bands = bands;
    a.rc[0] = ws;
    a.rc[1] = ws + rc_entries / 2;
    uint32_t *tail = (uint32_t *)(ws + rc_entries);
    a.stair_row[0] = tail;
    a.stair_row[1] = tail + stair_words / 2;
    uint32_t *d_cut = tail + stair_words;
    a.cut = d_cut;
    a.err = d_cut + bands;
    uint32_t *d_result = a.err + 1;
    a.tag = tag;
    a.lag = knobs->lag >= 0 ? knobs->lag : v.band_lag;
#ifdef BMX_EXPERIMENTS
    a.stamps = (uint64_t *)((char *)ws + stamp_at);
    a.stamp_block = knobs->stamp_block >= 0 ? (uint32_t)knobs->stamp_block : bands / 2;
    (void)hipMemsetAsync(a.stamps, 0, ED_STAMP_WORDS * sizeof(uint64_t), stream);
#endif
    // generous: 10 s + 100x the time the tile schedule would need (100 MHz ticks)
    a.timeout_ticks = 1000000000ull + (uint64_t)((double)la * (double)lb / 2.0e9 * 100.0);
    hipError_t e = hipEventRecord(st->ev0, stream);
    if (e == hipSuccess && fresh) e = hipMemsetAsync(ws, 0, rc_entries * sizeof(uint64_t), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bmx::ed_band_init_kernel, dim3(64), dim3(256), 0, stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        auto kern = knobs->group == 16 && v.band16 ? v.band16 : v.band;
#ifdef BMX_EXPERIMENTS
        if (knobs->step_x > 0 && v.band_threads == 256 && knobs->step_x < (int)(sizeof g_ed_step_experiments / sizeof g_ed_step_experiments[0]))
            kern = g_ed_step_experiments[knobs->step_x];
#endif
        if (v.band_lds > 64 * 1024) e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.band_lds);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(kern, dim3(2 * bands), dim3(v.band_threads), v.band_lds, stream, a);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bmx::ed_band_meet_kernel, dim3(bands), dim3(256), 0, stream, a, W, (int32_t *)d_result);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(st->ev1, stream);
    uint32_t h_tail[2] = {0, 0}; // err, result
    if (e == hipSuccess) e = hipMemcpyAsync(h_tail, a.err, sizeof h_tail, hipMemcpyDeviceToHost, stream);
#ifdef BMX_EXPERIMENTS
    if (e == hipSuccess) e = hipMemcpyAsync(st->stamps, a.stamps, sizeof st->stamps, hipMemcpyDeviceToHost, stream);
#endif
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) (void)hipEventElapsedTime(&st->last_ms, st->ev0, st->ev1);
    if (!keep) (void)hipFree(ws);
    if (e != hipSuccess) {
        snprintf(err, errlen, "bmx_edit_distance_device (band pipeline): %s", hipGetErrorString(e));
        return BMX_ERR_HIP;
    }
    if (h_tail[0] != 0) {
        snprintf(err, errlen, "bmx_edit_distance_device: a column band waited longer than the time limit for its neighbour");
        return BMX_ERR_HIP;
    }
    *h_result = (uint32_t)((int64_t)(int32_t)h_tail[1] + (int64_t)la + (int64_t)lb); // min(F_fwd + F_mir) + la + lb
    *used = true;
    return BMX_OK;
}
} // namespace

bool bmx_internal_ed_variant_ok(int variant)
{
    return variant >= 0 && (variant & ~ED_FLAGS) < N_ED_VARIANTS && g_ed_variants[variant & ~ED_FLAGS].kernel != nullptr;
}

void bmx_internal_ed_free(void *state_v)
{
    EdHost *st = static_cast<EdHost *>(state_v);
    if (!st) return;
    if (st->ws) (void)hipFree(st->ws);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    delete st;
}

float bmx_internal_ed_ms(const void *state_v)
{
    const EdHost *st = static_cast<const EdHost *>(state_v);
    return st ? st->last_ms : -1.0f;
}

void bmx_internal_ed_no_kernel(void *state_v)
{
    if (state_v) static_cast<EdHost *>(state_v)->last_ms = -1.0f;
}

#ifdef BMX_EXPERIMENTS
int bmx_internal_ed_stamps(const void *state_v, uint64_t *out280)
{
    const EdHost *st = static_cast<const EdHost *>(state_v);
    for (int i = 0; i < ED_STAMP_WORDS; ++i) out280[i] = st ? st->stamps[i] : 0;
    return BMX_OK;
}
#endif

// la >= 1, lb >= 1, both below 2^31; knobs->variant is one bmx_internal_ed_variant_ok accepts.
int bmx_internal_ed(void **state_v, const bmx_ed_knobs *knobs, const void *d_a, uint64_t la, const void *d_b, uint64_t lb,
                    uint64_t *distance, hipStream_t stream, char *err, size_t errlen)
{
    constexpr const char *WHERE = "bmx_edit_distance_device";
    if (!*state_v) *state_v = new EdHost();
    EdHost *st = static_cast<EdHost *>(*state_v);
    st->last_ms = -1.0f;
    if (!st->ev0) BMX_HIP(WHERE, hipEventCreate(&st->ev0));
    if (!st->ev1) BMX_HIP(WHERE, hipEventCreate(&st->ev1));
    const EdVariant &v = g_ed_variants[knobs->variant & ~ED_FLAGS];
    if (v.band && !(knobs->variant & ED_FLAGS)) {
        // The distance is symmetric and the pipeline is not: a row costs a step of every band, a column only its
        // share of one more band's lag (0.5 vs lag / (128 C) = 0.23 steps per character).  So the longer string
        // provides the columns.
        if (lb > la) {
            std::swap(d_a, d_b);
            std::swap(la, lb);
        }
        uint32_t h = 0;
        bool used = false;
        const int rc = ed_band_run(st, knobs, v, d_a, la, d_b, lb, stream, &h, &used, err, errlen);
        if (rc != BMX_OK) return rc;
        if (used) {
            *distance = h;
            return BMX_OK;
        }
    }
    const uint32_t W = 64u * v.c, R = (uint32_t)v.r;
    bmx::EdArgs a = {};
    a.a = (const uint8_t *)d_a;
    a.b = (const uint8_t *)d_b;
    a.la = (uint32_t)la;
    a.lb = (uint32_t)lb;
    a.tile_cols = (a.la + W - 1) / W;
    a.tile_rows = (a.lb + R - 1) / R;
    const uint32_t ndiag = a.tile_rows + a.tile_cols - 1;
    // Two-ended schedule: forward tile diagonals 0..K, mirrored ones for the rest, pairwise in one
    // launch; worth it as soon as there are three diagonals.
    const bool two_ended = v.dual && !(knobs->variant & ED_ONE_DIRECTION) && ndiag >= 3;
    const uint64_t n_srow = (uint64_t)a.tile_cols * (W + 1), n_scol = (uint64_t)a.tile_rows * (R + 1);
    // [3 x (la+1) bottom rows | lb+1 right column] per direction | staircase F/G rows, F/G columns | result
    const uint64_t per_dir = 3 * (la + 1) + (lb + 1);
    const uint64_t words = (two_ended ? 2 * per_dir + 2 * n_srow + 2 * n_scol : per_dir) + 1;
    uint32_t *ws = nullptr;
    BMX_HIP(WHERE, hipMalloc(&ws, words * sizeof(uint32_t)));
    a.bottom = ws;
    a.rightcol = ws + 3 * (la + 1);
    a.result = ws + words - 1;
    hipError_t e = hipEventRecord(st->ev0, stream);
    auto blocks_on = [&](uint32_t d) { // tiles on (logical) tile diagonal d
        const uint32_t i_lo = d >= a.tile_cols ? d - (a.tile_cols - 1) : 0;
        return std::min(d, a.tile_rows - 1) - i_lo + 1;
    };
    if (!two_ended) {
        for (uint32_t d = 0; d < ndiag && e == hipSuccess; ++d) {
            a.diag = d;
            hipLaunchKernelGGL(v.kernel, dim3(blocks_on(d)), dim3(64), 0, stream, a);
            e = hipGetLastError();
        }
    } else {
        a.bottom_m = ws + per_dir;
        a.rightcol_m = a.bottom_m + 3 * (la + 1);
        uint32_t *stair = ws + 2 * per_dir;
        a.stair_row[0] = stair;
        a.stair_row[1] = stair + n_srow;
        a.stair_col[0] = stair + 2 * n_srow;
        a.stair_col[1] = stair + 2 * n_srow + n_scol;
        if (e == hipSuccess) // 0xFF.. = bmx::ED_NONE: edges only one direction reaches never pair up
            e = hipMemsetAsync(stair, 0xFF, (2 * n_srow + 2 * n_scol) * sizeof(uint32_t), stream);
        const uint32_t K = (ndiag - 2) / 2;     // forward: diagonals 0..K
        const uint32_t last_m = ndiag - 2 - K;  // mirrored: its own diagonals 0..last_m (= table diagonals ndiag-1 .. K+1)
        for (uint32_t t = 0; t <= std::max(K, last_m) && e == hipSuccess; ++t) {
            const uint32_t nf = t <= K ? blocks_on(t) : 0, nm = t <= last_m ? blocks_on(t) : 0;
            a.diag = a.diag_m = t;
            a.n_fwd = nf;
            a.stair_fwd = t == K;
            a.stair_m = t == last_m;
            hipLaunchKernelGGL(v.dual, dim3(nf + nm), dim3(64), 0, stream, a);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(bmx::ed_meet_kernel, dim3(1), dim3(1024), 0, stream, a.stair_row[0], a.stair_row[1],
                               (uint32_t)n_srow, a.stair_col[0], a.stair_col[1], (uint32_t)n_scol, a.result);
            e = hipGetLastError();
        }
    }
    uint32_t h_result = 0;
    if (e == hipSuccess) e = hipEventRecord(st->ev1, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_result, a.result, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) (void)hipEventElapsedTime(&st->last_ms, st->ev0, st->ev1);
    (void)hipFree(ws);
    if (e != hipSuccess) {
        snprintf(err, errlen, "bmx_edit_distance_device: %s", hipGetErrorString(e));
        return BMX_ERR_HIP;
    }
    *distance = h_result;
    return BMX_OK;
}
