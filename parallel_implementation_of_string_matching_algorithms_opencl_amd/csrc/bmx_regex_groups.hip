// bmx_regex_groups.hip -- host side of the capture groups pass (bmx_regex_groups_device, include/bmx.h):
// per context a status word with its pinned copy, a pinned staging block and a device block for the tables of the forward
// walk (follow[] in forward numbering, pref, the tag words), two events.  A call builds the reversed automaton's sets and
// class table as the starts pass does (bmx_regex.hip), fills the staging block, copies it on the caller's stream in front
// of the launch, sizes the dynamic LDS by the automaton's max_len (one column word per byte and lane) and launches
// bmx_regex_groups_kernel.h's kernel, one lane per list entry.  The call returns only after synchronising the stream, so
// one staging block serves every call.  The argument checks and the context are the shim's (bmx_shim.hip).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "bmx.h"
#include "bmx_internal.h"
#include "bmx_regex_groups_kernel.h"
#include "bmx_tile_frame.h"

static_assert(bmx::REGEX_GROUPS_MAX == BMX_MAX_REGEX_GROUPS && bmx::REGEX_GROUPS_ROWS == BMX_MAX_REGEX_POSITIONS + 1, "header and kernel disagree");
static_assert(BMX_REGEX_START == BMX_MAX_REGEX_POSITIONS && BMX_REGEX_END == BMX_MAX_REGEX_POSITIONS, "the rows of the tables");
static_assert(sizeof(bmx::RegexGroupsArgs) <= 4096, "kernel arguments");

namespace {

constexpr const char *WHERE = "bmx_regex_groups_device";

struct RegexGroupsState {
    uint64_t *d_ws = nullptr; // the status word ...
    uint64_t *h_ws = nullptr; // ... and the pinned copy of it
    bmx::RegexGroupsBlock *h_block = nullptr; // the call's tables, pinned: valid until the call's synchronise
    bmx::RegexGroupsBlock *d_block = nullptr; // ... and where the kernel reads them
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t lds_attr[2] = {0, 0}; // the dynamic LDS each kernel may take so far
    float last_ms = -1.0f;
};

// as bmx_regex.hip's: lin = the positions whose only successor is the next one, nl = the others with a successor
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

void bmx_internal_regex_groups_free(void *state_v)
{
    RegexGroupsState *st = static_cast<RegexGroupsState *>(state_v);
    if (!st) return;
    if (st->d_ws) (void)hipFree(st->d_ws);
    if (st->h_ws) (void)hipHostFree(st->h_ws);
    if (st->d_block) (void)hipFree(st->d_block);
    if (st->h_block) (void)hipHostFree(st->h_block);
    for (hipEvent_t e : st->ev)
        if (e) (void)hipEventDestroy(e);
    delete st;
}

float bmx_internal_regex_groups_ms(const void *state_v) { return state_v ? static_cast<const RegexGroupsState *>(state_v)->last_ms : -1.0f; }

// count >= 1, a valid pair (re, gr): the (begin, end) pairs of groups 0..n_groups of every entry
int bmx_internal_regex_groups(void **state_v, const void *d_text, uint64_t n, uint64_t base_offset, const bmx_regex *re,
                              const bmx_regex_groups *gr, const uint64_t *d_starts, const uint64_t *d_ends, uint64_t count,
                              uint64_t *d_groups, hipStream_t stream, char *err, size_t errlen)
{
    if (!*state_v) *state_v = new RegexGroupsState();
    RegexGroupsState *st = static_cast<RegexGroupsState *>(*state_v);
    st->last_ms = -1.0f;
    const uint64_t n_blocks = (count + bmx::REGEX_GROUPS_BLOCK - 1) / bmx::REGEX_GROUPS_BLOCK;
    if (n_blocks > 0x7fffffffull) {
        snprintf(err, errlen, "bmx_regex_groups_device: more than 2^31 workgroups of list entries in one call");
        return BMX_ERR_ARG;
    }
    if (!st->d_ws) BMX_HIP(WHERE, hipMalloc(&st->d_ws, sizeof(uint64_t)));
    if (!st->h_ws) BMX_HIP(WHERE, hipHostMalloc(&st->h_ws, sizeof(uint64_t), hipHostMallocDefault));
    if (!st->h_block) BMX_HIP(WHERE, hipHostMalloc(reinterpret_cast<void **>(&st->h_block), sizeof(bmx::RegexGroupsBlock), hipHostMallocDefault));
    if (!st->d_block) BMX_HIP(WHERE, hipMalloc(reinterpret_cast<void **>(&st->d_block), sizeof(bmx::RegexGroupsBlock)));
    for (hipEvent_t &e : st->ev)
        if (!e) BMX_HIP(WHERE, hipEventCreate(&e));
    BMX_HIP(WHERE, hipMemsetAsync(st->d_ws, 0, sizeof(uint64_t), stream)); // the status word starts clean in every call

    const int32_t m = re->m;
    int32_t min_len = 0, max_len = 0;
    bmx_regex_lengths(m, re->first, re->last, re->follow, &min_len, &max_len); // (the struct's fields are not read)

    // the tables of the forward walk
    bmx::RegexGroupsBlock *blk = st->h_block;
    std::memset(blk, 0, sizeof *blk);
    for (int32_t p = 0; p < m; ++p) blk->follow[p] = re->follow[p];
    blk->follow[BMX_REGEX_START] = re->first;
    std::memcpy(blk->pref, gr->pref, sizeof gr->pref);
    for (uint32_t from = 0; from < bmx::REGEX_GROUPS_ROWS; ++from)
        for (uint32_t to = 0; to < bmx::REGEX_GROUPS_ROWS; ++to)
            blk->tags[from * bmx::REGEX_GROUPS_ROWS + to] = (uint32_t)gr->open[from][to] | ((uint32_t)gr->close[from][to] << 16);
    BMX_HIP(WHERE, hipMemcpyAsync(st->d_block, st->h_block, sizeof *blk, hipMemcpyHostToDevice, stream));

    const uint64_t addr = reinterpret_cast<uint64_t>(d_text);
    bmx::RegexGroupsArgs a;
    std::memset(&a, 0, sizeof a);
    a.text16 = reinterpret_cast<const uint8_t *>(addr & ~15ull);
    a.first = addr & 15ull;
    a.n = n;
    a.base = base_offset;
    a.starts = d_starts;
    a.ends = d_ends;
    a.count = count;
    a.groups = d_groups;
    a.ws = st->d_ws;
    a.block = st->d_block;
    a.max_len = (uint32_t)max_len; // (0: no span can match, and every entry that is not skipped raises the status word)
    a.m = (uint32_t)m;
    a.n_groups = (uint32_t)gr->n_groups;
    // the REVERSED automaton: bit i stands for position m - 1 - i, first and last swap, follow is transposed
    bmx_regex rev;
    (void)bmx_regex_reverse(re, &rev); // (valid: the shim's check)
    a.k = regex_sets(m, rev.first, rev.last, rev.follow);
    bmx::tile_class_table(rev.classes, m, 0, false, a.peq);

    const bool wide = m > 32;
    void (*kernel)(const bmx::RegexGroupsArgs) = wide ? bmx::regex_groups_kernel<uint64_t> : bmx::regex_groups_kernel<uint32_t>;
    const size_t lds = (size_t)max_len * bmx::REGEX_GROUPS_BLOCK * (wide ? 8 : 4); // the columns: at most 128 KiB
    if (lds > st->lds_attr[wide]) {
        BMX_HIP(WHERE, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        st->lds_attr[wide] = lds;
    }
    BMX_HIP(WHERE, hipEventRecord(st->ev[0], stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_blocks), dim3(bmx::REGEX_GROUPS_BLOCK), lds, stream, a);
    BMX_HIP(WHERE, hipGetLastError());
    BMX_HIP(WHERE, hipEventRecord(st->ev[1], stream));
    BMX_HIP(WHERE, hipMemcpyAsync(st->h_ws, st->d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(WHERE, hipStreamSynchronize(stream));
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, st->ev[0], st->ev[1]) == hipSuccess) st->last_ms = ms;

    const uint64_t bad = st->h_ws[0];
    if (bad != 0) {
        snprintf(err, errlen, "bmx_regex_groups_device: %s%s%s", bad & bmx::REGEX_GROUPS_BAD_SPAN ? "a span outside the view; " : "",
                 bad & bmx::REGEX_GROUPS_TOO_LONG ? "a span longer than the expression's longest match; " : "",
                 bad & bmx::REGEX_GROUPS_NO_MATCH ? "a span that is no match of this expression; " : "");
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}
