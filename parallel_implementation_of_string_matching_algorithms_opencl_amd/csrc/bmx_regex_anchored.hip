// bmx_regex_anchored.hip -- host side of the anchored regular-expression search (bmx_search_regex_anchored_device,
// bmx_regex_anchored_starts_device, bmx_search_regex_anchored_begins_device, bmx_regex_anchored_ends_device,
// include/bmx.h): what bmx_regex.hip builds for the plain search, with max_len in place of max_len - 1 as
// the warm-up, and the two gate tables E and A (bmx_regex_anchored_kernel.h) from struct bmx_regex_anchors.  The tables
// are too large for kernel arguments: the state owns a device buffer for them and a pinned copy, written on the host
// and sent on the call's stream in front of the launch (every entry returns after synchronising its stream, so the
// pinned copy is free again when the next call fills it).  The argument checks and the context are the shim's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_regex_anchored_kernel.h"

static_assert(sizeof(bmx::TileArgs) + sizeof(bmx::RegexSets) + sizeof(bmx::RegexGate) + 8 <= 4096, "kernel arguments");
static_assert(sizeof(bmx::RegexAnchoredStartsArgs) <= 4096 && sizeof(bmx::RegexAnchoredEndsArgs) <= 4096, "kernel arguments");

namespace {

constexpr const char *WHERE = "bmx_search_regex_anchored_device";
constexpr const char *WHERE_STARTS = "bmx_regex_anchored_starts_device";
constexpr const char *WHERE_BEGINS = "bmx_search_regex_anchored_begins_device";
constexpr const char *WHERE_ENDS = "bmx_regex_anchored_ends_device";
constexpr size_t GATE_BYTES = bmx::REGEX_GATE_WORDS * sizeof(uint64_t);

// the forward search with its starts pass, and the begins search with its ends pass: one of these each
struct AnchoredState {
    bmx::TileState tile; // (first: bmx_tile_frame.h)
    uint64_t *d_ws = nullptr;   // the post-pass: its status word ...
    uint64_t *h_ws = nullptr;   // ... and the pinned copy of it
    uint64_t *d_gate = nullptr; // the gate tables: {E, A, A_rev, E_rev}, 256 words each ...
    uint64_t *h_gate = nullptr; // ... and the pinned copy they are sent from
};
static_assert(offsetof(AnchoredState, tile) == 0, "tile_state, ordered_set_seq");

// (as bmx_regex.hip's; first and last are not in the anchored step, they stay for the post-passes' seed)
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

// The four tables into the pinned copy and from there to the device, on `stream`.
int send_gate(AnchoredState *st, const char *where, const bmx_regex *re, const bmx_regex_anchors *an, hipStream_t stream, char *err,
              size_t errlen)
{
    if (!st->d_gate) BMX_HIP(where, hipMalloc(&st->d_gate, GATE_BYTES));
    if (!st->h_gate) BMX_HIP(where, hipHostMalloc(&st->h_gate, GATE_BYTES, hipHostMallocDefault));
    uint64_t *e = st->h_gate, *a = e + 256, *a_rev = e + 512, *e_rev = e + 768;
    std::memset(st->h_gate, 0, GATE_BYTES);
    const int32_t m = re->m;
    for (int32_t i = 0; i < m; ++i) {
        const uint8_t *before = an->before + (size_t)i * BMX_CLASS_BYTES, *after = an->after + (size_t)i * BMX_CLASS_BYTES;
        for (uint32_t c = 0; c < 256; ++c) {
            if (((re->first >> i) & 1u) && ((before[c >> 3] >> (c & 7)) & 1u)) e[c] |= 1ull << i, e_rev[c] |= 1ull << (m - 1 - i);
            if (((re->last >> i) & 1u) && ((after[c >> 3] >> (c & 7)) & 1u)) a[c] |= 1ull << i, a_rev[c] |= 1ull << (m - 1 - i);
        }
    }
    BMX_HIP(where, hipMemcpyAsync(st->d_gate, st->h_gate, GATE_BYTES, hipMemcpyHostToDevice, stream));
    return BMX_OK;
}

void state_free(void *state_v)
{
    AnchoredState *st = static_cast<AnchoredState *>(state_v);
    if (!st) return;
    st->tile.oo.free();
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    if (st->d_gate) (void)hipFree(st->d_gate);
    if (st->h_gate) (void)hipHostFree(st->h_gate);
    delete st;
}

} // namespace

void bmx_internal_regex_anchored_free(void *state_v) { state_free(state_v); }
void bmx_internal_regex_anchored_begins_free(void *state_v) { state_free(state_v); }
float bmx_internal_regex_anchored_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }
float bmx_internal_regex_anchored_begins_ms(const void *state_v) { return bmx::tile_last_ms(state_v); }

int bmx_internal_regex_anchored(void **state_v, int num_cu, const void *d_text, uint64_t n, uint64_t lead, uint64_t base_offset,
                                const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left, uint32_t right, uint64_t *d_ends,
                                uint64_t capacity, uint64_t *n_matches, hipStream_t stream, char *err, size_t errlen)
{
    AnchoredState *st = bmx::tile_state<AnchoredState>(state_v, n_matches);
    if (lead >= n) return BMX_OK; // no end is owned (before anything is put on `stream`)
    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len); // (the struct's fields are not read)
    if (max_len == 0) return BMX_OK; // no path from first to last: nothing can match
    const bmx::RegexSets k = regex_sets(m, re->first, re->last, re->follow);
    const bool wide = m > 32, nl = k.nl != 0;
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexSets, const bmx::RegexGate);
    static const Kernel kernels[4] = {bmx::tile_kernel<bmx::RegexAnchoredPolicy<false, false>, bmx::RegexSets, bmx::RegexGate>,
                                      bmx::tile_kernel<bmx::RegexAnchoredPolicy<true, false>, bmx::RegexSets, bmx::RegexGate>,
                                      bmx::tile_kernel<bmx::RegexAnchoredPolicy<false, true>, bmx::RegexSets, bmx::RegexGate>,
                                      bmx::tile_kernel<bmx::RegexAnchoredPolicy<true, true>, bmx::RegexSets, bmx::RegexGate>};
    const int slot = (wide ? 1 : 0) + (nl ? 2 : 0);
    const int rc = send_gate(st, WHERE, re, an, stream, err, errlen);
    if (rc != BMX_OK) return rc;
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    a.warm = (uint32_t)max_len; // one byte more than the plain search: the look-behind of a lane's first byte
    bmx::tile_class_table(re->classes, m, 0, false, a.peq); // bit i: the byte is in class i
    const bmx::RegexGate g = {st->d_gate, left, right};
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n - lead, max_len + 1, resident); };
    return bmx::tile_launch(&st->tile, WHERE, kernels[slot], slot, num_cu, a, d_text, n, lead, base_offset, piece, d_ends, capacity,
                            n_matches, stream, err, errlen, k, g);
}

// count >= 1: d_starts[i] for d_ends[i], one lane per entry over the reversed automaton
int bmx_internal_regex_anchored_starts(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                       const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_ends,
                                       uint64_t count, uint32_t flags, uint64_t *d_starts, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new AnchoredState();
    AnchoredState *st = static_cast<AnchoredState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::REGEX_STARTS_BLOCK - 1) / bmx::REGEX_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "%s: more than 2^31 workgroups of list entries in one call", WHERE_STARTS);
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_STARTS, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_STARTS, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    BMX_HIP(WHERE_STARTS, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call
    const int rc = send_gate(st, WHERE_STARTS, re, an, stream, err, errlen);
    if (rc != BMX_OK) return rc;

    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len);
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::RegexAnchoredStartsArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.n = n;
    a.base = base_offset;
    a.ends = d_ends;
    a.count = count;
    a.starts = d_starts;
    a.ws = st->d_ws;
    a.gate = st->d_gate + 512; // {A_rev, E_rev}
    a.max_len = (uint32_t)max_len; // (0: no entry can be an end of a match, and every valid one raises the status word)
    a.chunks = (uint32_t)(max_len + 1 + 7) / 8;
    a.longest = (flags & BMX_REGEX_LONGEST) ? 1u : 0u;
    a.left = left;
    a.right = right;
    bmx_regex rev; // bit i stands for position m - 1 - i, first and last swap, follow is transposed
    (void)bmx_regex_reverse(re, &rev); // (valid: the shim's check)
    a.k = regex_sets(m, rev.first, rev.last, rev.follow);
    bmx::tile_class_table(rev.classes, m, 0, false, a.peq);
    void (*kernel)(const bmx::RegexAnchoredStartsArgs) =
        m > 32 ? bmx::regex_anchored_starts_kernel<uint64_t> : bmx::regex_anchored_starts_kernel<uint32_t>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::REGEX_STARTS_BLOCK), 0, stream, a);
    BMX_HIP(WHERE_STARTS, hipGetLastError());
    BMX_HIP(WHERE_STARTS, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_STARTS, hipStreamSynchronize(stream));

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "%s: %s%s", WHERE_STARTS, bad & bmx::REGEX_BAD_END ? "an end outside the view; " : "",
                 bad & bmx::REGEX_BAD_START ? "an end at which no anchored match of this expression ends; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}

// The frame in START coordinates, as bmx_internal_regex_begins: the reversed automaton, {A_rev, E_rev} as the gate.
int bmx_internal_regex_anchored_begins(void **state_v, int num_cu, int piece_shift, const void *d_text, uint64_t n, uint64_t tail,
                                       uint64_t base_offset, const bmx_regex *re, const bmx_regex_anchors *an, uint32_t left,
                                       uint32_t right, uint64_t *d_starts, uint64_t capacity, uint64_t *n_matches, hipStream_t stream,
                                       char *err, size_t errlen)
{
    AnchoredState *st = bmx::tile_state<AnchoredState>(state_v, n_matches);
    if (tail >= n) return BMX_OK; // no start is owned (before anything is put on `stream`)
    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len); // (the struct's fields are not read)
    if (max_len == 0) return BMX_OK; // no path from first to last: nothing can match
    bmx_regex rev;
    (void)bmx_regex_reverse(re, &rev); // (valid: the shim's check)
    const bmx::RegexSets k = regex_sets(m, rev.first, rev.last, rev.follow);
    const bool wide = m > 32, nl = k.nl != 0;
    typedef void (*Kernel)(const bmx::TileArgs, const bmx::RegexSets, const bmx::RegexGate, const uint64_t);
    static const Kernel kernels[4] = {bmx::tile_kernel<bmx::RegexAnchoredBeginsPolicy<false, false>, bmx::RegexSets, bmx::RegexGate, uint64_t>,
                                      bmx::tile_kernel<bmx::RegexAnchoredBeginsPolicy<true, false>, bmx::RegexSets, bmx::RegexGate, uint64_t>,
                                      bmx::tile_kernel<bmx::RegexAnchoredBeginsPolicy<false, true>, bmx::RegexSets, bmx::RegexGate, uint64_t>,
                                      bmx::tile_kernel<bmx::RegexAnchoredBeginsPolicy<true, true>, bmx::RegexSets, bmx::RegexGate, uint64_t>};
    const int slot = (wide ? 1 : 0) + (nl ? 2 : 0);
    const int rc = send_gate(st, WHERE_BEGINS, re, an, stream, err, errlen);
    if (rc != BMX_OK) return rc;
    bmx::TileArgs a;
    std::memset(&a, 0, sizeof a);
    a.m = (uint32_t)m;
    a.warm = (uint32_t)max_len;
    bmx::tile_class_table(rev.classes, m, 0, false, a.peq); // bit i: the byte is in class m - 1 - i
    const bmx::RegexGate g = {st->d_gate + 512, left, right};
    const uint64_t view_hi = n + (reinterpret_cast<uint64_t>(d_text) & 15ull); // one past the view's last byte, aligned coordinates
    const auto piece = [&](uint64_t resident) { return bmx_internal_classes_piece_shift(n - tail, max_len + 1, resident); };
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
                            capacity, n_matches, stream, err, errlen, k, g, view_hi);
}

// count >= 1: d_ends[i] for d_starts[i], one lane per entry over the automaton as given.
int bmx_internal_regex_anchored_ends(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                                     const bmx_regex_anchors *an, uint32_t left, uint32_t right, const uint64_t *d_starts,
                                     uint64_t count, const uint64_t *d_limit, uint32_t flags, uint64_t *d_ends, hipStream_t stream,
                                     char *err, size_t errlen)
{
    if (!*state_v) *state_v = new AnchoredState();
    AnchoredState *st = static_cast<AnchoredState *>(*state_v);
    const uint64_t n_blocks = (count + bmx::REGEX_STARTS_BLOCK - 1) / bmx::REGEX_STARTS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "%s: more than 2^31 workgroups of list entries in one call", WHERE_ENDS);
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE_ENDS, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE_ENDS, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    BMX_HIP(WHERE_ENDS, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call
    const int rc = send_gate(st, WHERE_ENDS, re, an, stream, err, errlen);
    if (rc != BMX_OK) return rc;

    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len);
    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::RegexAnchoredEndsArgs a;
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
    a.gate = st->d_gate; // {E, A}
    a.max_len = (uint32_t)max_len; // (0: no entry can be a start of a match)
    a.chunks = (uint32_t)(max_len + 1 + 7) / 8;
    a.longest = (flags & BMX_REGEX_LONGEST) ? 1u : 0u;
    a.left = left;
    a.right = right;
    a.k = regex_sets(m, re->first, re->last, re->follow);
    bmx::tile_class_table(re->classes, m, 0, false, a.peq);
    void (*kernel)(const bmx::RegexAnchoredEndsArgs) =
        m > 32 ? bmx::regex_anchored_ends_kernel<uint64_t> : bmx::regex_anchored_ends_kernel<uint32_t>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::REGEX_STARTS_BLOCK), 0, stream, a);
    BMX_HIP(WHERE_ENDS, hipGetLastError());
    BMX_HIP(WHERE_ENDS, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE_ENDS, hipStreamSynchronize(stream));

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "%s: %s%s", WHERE_ENDS, bad & bmx::REGEX_ENDS_BAD_START ? "a start outside the view; " : "",
                 bad & bmx::REGEX_ENDS_NO_MATCH ? "a start at which no anchored match of this expression begins; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}
