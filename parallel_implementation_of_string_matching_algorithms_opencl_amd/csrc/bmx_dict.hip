// bmx_dict.hip -- host side of the dictionary search (bmx_dict_*, include/bmx.h): builds a dictionary's tables in plain
// C++ (the LDS bitmaps, the exact-prefix table, the id order, the pattern blob) and uploads them once; launches
// bmx_dict_kernel.h once per search inside an ordered-output call (bmx_ordered_out.h: status words, ticket, pinned result
// words, the wait for the stream).  The argument checks are the shim's (bmx_shim.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "bmx.h"
#include "bmx_dict_kernel.h"
#include "bmx_internal.h"

static_assert(bmx::DICT_MAX == BMX_MAX_DICT, "header and kernel disagree");
static_assert(bmx::DICT_ROUND == 1 << 13, "tile_shift assumes 8 KiB rounds");
static_assert(sizeof(bmx::DictArgs) <= 4096, "kernel arguments");
#ifdef BMX_EXPERIMENTS
static_assert(6 + bmx::DICT_MAX_ROUNDS_SHIFT == bmx::ORDERED_DICT_MAX_PIECE_SHIFT, "what the knob tile_piece_shift accepts");
#endif

struct bmx_dict {
    const void *owner = nullptr; // the context it was built for
    int device = 0;
    int32_t K = 0, max_m = 0;
    uint32_t classes = 0, table_mask = 0;
    uint32_t *d_bitmaps = nullptr;
    uint4 *d_table = nullptr;
    uint32_t *d_ids = nullptr;
    uint2 *d_pats = nullptr;
    uint8_t *d_blob = nullptr;
};

namespace {

struct DictState {
    bmx::OrderedOut oo; // (first: bmx_ordered_out.h)
    unsigned long long *d_cand = nullptr; // candidates of the last call
    bool launched = false;
    int blocks_per_cu = 0;
};
static_assert(offsetof(DictState, oo) == 0, "ordered_set_seq");

void set_bit(std::vector<uint32_t> &bm, uint32_t base, uint32_t word, uint32_t bit)
{
    bm[base + word] |= 1u << (bit & 31u);
}

void free_dict(bmx_dict *d)
{
    if (!d) return;
    if (d->d_bitmaps) (void)hipFree(d->d_bitmaps);
    if (d->d_table) (void)hipFree(d->d_table);
    if (d->d_ids) (void)hipFree(d->d_ids);
    if (d->d_pats) (void)hipFree(d->d_pats);
    if (d->d_blob) (void)hipFree(d->d_blob);
    delete d;
}

} // namespace

// The patterns' prefix key as the exact-prefix table stores it (bytes < 0x80 assumed: the shim checked them).
static uint32_t prefix_key(const char *p, int32_t m)
{
    const int c = std::min<int32_t>(m, 4);
    uint32_t k = 0;
    for (int j = 0; j < c; ++j) k |= (uint32_t)(uint8_t)p[j] << (8 * j);
    return c == 4 ? k : (k | (0xffffffffu << (8 * c)));
}

int bmx_internal_dict_create(const void *owner, int device, const char *const *pats, const int32_t *ms, int32_t K,
                             bmx_dict **out, char *err, size_t errlen)
{
    const char *where = "bmx_dict_create";
    std::vector<uint32_t> bm(bmx::DICT_BM_WORDS, 0u);
    std::map<uint32_t, std::vector<uint32_t>> groups; // prefix key -> ids, ascending
    std::vector<uint2> pl(K);
    std::vector<uint8_t> blob;
    uint32_t classes = 0;
    int32_t max_m = 0;
    for (int32_t i = 0; i < K; ++i) {
        const char *p = pats[i];
        const int32_t m = ms[i];
        const int c = std::min<int32_t>(m, 4);
        classes |= 1u << (c - 1);
        max_m = std::max(max_m, m);
        uint32_t k = 0;
        for (int j = 0; j < c; ++j) k |= (uint32_t)(uint8_t)p[j] << (8 * j);
        if (c == 1) {
            set_bit(bm, bmx::DICT_BM1, k >> 5, k);
        } else if (c == 2) {
            const uint32_t x = (k & 0x7fu) | ((k >> 1) & 0x3f80u);
            set_bit(bm, bmx::DICT_BM2, x >> 5, x);
        } else if (c == 3) {
            const uint32_t f1 = bmx::dict_fold1(k), f2 = bmx::dict_fold2(k);
            set_bit(bm, bmx::DICT_BM3, bmx::dict_h3a_word(f1), f1);
            set_bit(bm, bmx::DICT_BM3, bmx::dict_h3b_word(f2), f2);
        } else {
            const uint32_t f1 = bmx::dict_fold1(k), f2 = bmx::dict_fold2(k);
            set_bit(bm, bmx::DICT_BM4, bmx::dict_h4a_word(f1), f1);
            set_bit(bm, bmx::DICT_BM4, bmx::dict_h4b_word(f2), f2);
        }
        groups[prefix_key(p, m)].push_back((uint32_t)i);
        pl[i] = make_uint2((uint32_t)blob.size(), (uint32_t)m);
        blob.insert(blob.end(), p, p + m);
    }
    // exact-prefix table: open addressing, linear probing, at most half full
    const uint32_t bits = std::max<uint32_t>(bmx::ceil_log2(2 * groups.size()), 4);
    const uint32_t size = 1u << bits;
    std::vector<uint4> table(size, make_uint4(bmx::DICT_EMPTY, 0, 0, 0));
    std::vector<uint32_t> ids;
    ids.reserve(K);
    for (const auto &g : groups) {
        uint32_t s = bmx::dict_slot(g.first) & (size - 1);
        while (table[s].x != bmx::DICT_EMPTY) s = (s + 1) & (size - 1);
        table[s] = make_uint4(g.first, (uint32_t)ids.size(), (uint32_t)g.second.size(), 0);
        ids.insert(ids.end(), g.second.begin(), g.second.end());
    }

    bmx_dict *d = new bmx_dict();
    d->owner = owner;
    d->device = device;
    d->K = K;
    d->max_m = max_m;
    d->classes = classes;
    d->table_mask = size - 1;
    auto upload = [&](void **dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(dst, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = upload((void **)&d->d_bitmaps, bm.data(), bm.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = upload((void **)&d->d_table, table.data(), table.size() * sizeof(uint4));
    if (e == hipSuccess) e = upload((void **)&d->d_ids, ids.data(), ids.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = upload((void **)&d->d_pats, pl.data(), pl.size() * sizeof(uint2));
    if (e == hipSuccess) e = upload((void **)&d->d_blob, blob.data(), blob.size());
    if (e != hipSuccess) {
        snprintf(err, errlen, "%s: upload of the tables failed: %s", where, hipGetErrorString(e));
        free_dict(d);
        return BMX_ERR_HIP;
    }
    *out = d;
    return BMX_OK;
}

void bmx_internal_dict_destroy(bmx_dict *d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    free_dict(d);
}

const void *bmx_internal_dict_owner(const bmx_dict *d) { return d->owner; }

void bmx_internal_dict_state_free(void *state_v)
{
    DictState *st = static_cast<DictState *>(state_v);
    if (!st) return;
    st->oo.free();
    if (st->d_cand) (void)hipFree(st->d_cand);
    delete st;
}

float bmx_internal_dict_ms(const void *state_v)
{
    const DictState *st = static_cast<const DictState *>(state_v);
    return st ? st->oo.last_ms : -1.0f;
}

// Positions of the last search that passed the LDS filters and were looked up in the exact-prefix table.
int64_t bmx_internal_dict_candidates(const void *state_v)
{
    const DictState *st = static_cast<const DictState *>(state_v);
    if (!st) return -1;
    if (!st->launched) return 0; // (a search of nothing: no kernel, and on a new context no counter yet)
    if (!st->d_cand) return -1;
    unsigned long long v = 0;
    if (hipMemcpy(&v, st->d_cand, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

int bmx_internal_dict_search(void **state_v, int num_cu, const bmx_dict *d, const void *d_text, uint64_t n, uint64_t n_own,
                             uint64_t base_offset, uint64_t *d_pos, uint32_t *d_pid, uint64_t capacity,
                             uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    const char *where = "bmx_dict_search_device";
    if (!*state_v) *state_v = new DictState();
    DictState *st = static_cast<DictState *>(*state_v);
    if (n_matches) *n_matches = 0;
    st->oo.last_ms = 0.0f;
    st->launched = false;
    const uint64_t own = std::min(n_own, n);
    if (own == 0) return BMX_OK; // no start to report (before anything is put on `stream`)
    if (!st->d_cand) BMX_HIP(where, hipMalloc(&st->d_cand, sizeof(unsigned long long)));
    if (st->blocks_per_cu == 0) {
        BMX_HIP(where, hipOccupancyMaxActiveBlocksPerMultiprocessor(&st->blocks_per_cu, bmx::dict_kernel, bmx::DICT_BLOCK, 0));
        st->blocks_per_cu = std::max(1, std::min(st->blocks_per_cu, 4));
    }

    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::DictArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.own_hi = own + a.first;
    a.vend = n + a.first;
    a.out_bias = base_offset - a.first;
    // tiles of 2^rs rounds: about eight tiles per resident workgroup, at most 256 KiB
    const uint64_t resident = (uint64_t)num_cu * (uint64_t)st->blocks_per_cu;
    const uint64_t rounds = (a.own_hi + bmx::DICT_ROUND - 1) / bmx::DICT_ROUND;
    const uint64_t per = rounds / std::max<uint64_t>(8 * resident, 1);
    uint32_t rs = std::min<uint32_t>(per ? 63 - __builtin_clzll(per) : 0, bmx::DICT_MAX_ROUNDS_SHIFT);
#ifdef BMX_EXPERIMENTS
    if (st->oo.force_piece_shift) rs = st->oo.force_piece_shift - 6; // libbmx_exp.so's knob "tile_piece_shift" (6..11 here)
#endif
    const uint32_t tile_shift = rs + 13;
    a.tile_begin = a.first >> tile_shift; // == 0
    a.n_tiles = ((a.own_hi + (1ull << tile_shift) - 1) >> tile_shift) - a.tile_begin;
    a.out = capacity ? d_pos : nullptr;
    a.pid = capacity ? d_pid : nullptr;
    a.cap = capacity;
    a.bitmaps = d->d_bitmaps;
    a.table = d->d_table;
    a.ids = d->d_ids;
    a.pats = d->d_pats;
    a.blob = d->d_blob;
    a.table_mask = d->table_mask;
    a.classes = d->classes;
    a.rounds_shift = rs;

    a.cand = st->d_cand;

    BMX_HIP(where, hipMemsetAsync(st->d_cand, 0, sizeof(unsigned long long), stream));
    int rc = st->oo.begin(where, stream, a, err, errlen);
    if (rc != BMX_OK) return rc;
    uint64_t grid = std::min<uint64_t>(a.n_tiles, resident);
#ifdef BMX_EXPERIMENTS
    if (st->oo.force_max_grid) grid = std::min<uint64_t>(grid, st->oo.force_max_grid); // ... "tile_max_grid"
    st->oo.last_piece_shift = rs + 6, st->oo.last_grid = grid, st->oo.last_tiles = a.n_tiles; // (bmx_exp_last_launch)
#endif
    hipLaunchKernelGGL(bmx::dict_kernel, dim3((uint32_t)grid), dim3(bmx::DICT_BLOCK), 0, stream, a);
    st->launched = true;
    return st->oo.finish(where, grid, a.n_tiles, stream, capacity, n_matches, err, errlen);
}
