// index_entries_check.cpp -- the host side of the text index's entries under AddressSanitizer and UBSan, on a machine
// WITHOUT a GPU: every argument-error path of the five host-buffer entries (bmx_index_count/locate/match/seeds/map) and of
// the five device entries with ctx = NULL, then the host-buffer entries with valid arguments, which fail at the context
// and must free what they took.  Prints one line per call, "label rc last-error": two builds of the library answer alike
// iff their outputs are equal, and the sanitizers' exit code says whether anything leaked or was misused.
//
// A stand-alone program, not a test and never loaded into Python.  Build it with the sources of the library and the host
// side instrumented (from parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc, every .hip and .cpp but
// bmx_main.cpp):
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//           <sources> ../../tools/index_entries_check.cpp -o index_entries_check -ldl -pthread
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bmx.h"

static void say(const char *label, int rc) { printf("%-44s %3d  %s\n", label, rc, bmx_last_error()); }

int main()
{
    const char text[] = "abracadabra abracadabra";
    const uint64_t n = sizeof text - 1;
    const uint8_t blob[] = "abracadzz";
    const uint8_t high[] = {'a', 'b', 0x80, 'c', 'a', 'd', 'z', 'z', 'z'};
    const uint64_t good[] = {0, 4, 7, 9}, falls[] = {0, 7, 4, 9}, past[] = {0, 4, 7, 10}, empty[] = {0, 4, 4, 9};
    std::vector<uint8_t> long_blob(BMX_MAX_PATTERN + 1, 'a');
    const uint64_t long_off[] = {0, BMX_MAX_PATTERN + 1};
    uint32_t u32[4][64];
    uint64_t u64[5][64], total = 77;
    uint8_t u8[2][64];
    void *const dev = u64; // a non-NULL "device" pointer: no entry reaches a HIP call with ctx = NULL
    bmx_index *const no_ix = nullptr;

    // one call of each entry; what an entry does not take is ignored
    struct Args {
        const char *text;
        uint64_t n;
        const void *pat;
        uint64_t pat_bytes;
        const uint64_t *off;
        uint64_t count;
        uint32_t min_len, max_occ;
        int32_t k;
        bool out, lists; // the outputs every call needs / the lists behind `capacity`
        uint64_t capacity;
    };
    const Args ok = {text, n, blob, 9, good, 3, 3, 4, 1, true, true, 32};
    auto host = [&](int e, const Args &a) {
        total = 77;
        switch (e) {
        case 0: return bmx_index_count(nullptr, a.text, a.n, a.pat, a.pat_bytes, a.off, a.count, a.out ? u32[0] : nullptr);
        case 1:
            return bmx_index_locate(nullptr, a.text, a.n, a.pat, a.pat_bytes, a.off, a.count, a.out ? u64[0] : nullptr,
                                    a.lists ? u64[1] : nullptr, a.capacity, &total);
        case 2:
            return bmx_index_match(nullptr, a.text, a.n, a.pat, a.pat_bytes, a.off, a.count, a.out ? u32[0] : nullptr, u32[1],
                                   u32[2]);
        case 3:
            return bmx_index_seeds(nullptr, a.text, a.n, a.pat, a.pat_bytes, a.off, a.count, a.min_len, a.max_occ,
                                   a.out ? u64[0] : nullptr, u32[0], u32[1], u32[2], a.lists ? u32[3] : nullptr, a.capacity, &total);
        default:
            return bmx_index_map(nullptr, a.text, a.n, a.pat, a.pat_bytes, a.off, a.count, a.min_len, a.max_occ, a.k, u64[0], u64[1],
                                 a.out ? u8[0] : nullptr, u64[2], u64[3], u64[4], a.lists ? u8[1] : nullptr, a.capacity, &total);
        }
    };
    auto device = [&](int e, const Args &a) {
        total = 77;
        switch (e) {
        case 0:
            return bmx_index_count_device(nullptr, no_ix, a.pat, a.pat_bytes, a.off, a.count, nullptr, a.out ? u32[0] : nullptr,
                                          nullptr);
        case 1:
            return bmx_index_locate_device(nullptr, no_ix, a.pat, a.pat_bytes, a.off, a.count, 0, a.out ? u64[0] : nullptr,
                                           a.lists ? u64[1] : nullptr, a.capacity, &total, nullptr);
        case 2:
            return bmx_index_match_device(nullptr, no_ix, a.pat, a.pat_bytes, a.off, a.count, a.out ? u32[0] : nullptr, nullptr,
                                          nullptr, nullptr);
        case 3:
            return bmx_index_seeds_device(nullptr, no_ix, a.pat, a.pat_bytes, a.off, a.count, a.min_len, a.max_occ,
                                          a.out ? u64[0] : nullptr, u32[0], u32[1], u32[2], a.lists ? u32[3] : nullptr, a.capacity,
                                          &total, nullptr);
        default:
            return bmx_index_map_device(nullptr, no_ix, a.pat, a.pat_bytes, a.off, a.count, a.min_len, a.max_occ, a.k, 0, u64[0],
                                        u64[1], a.out ? u8[0] : nullptr, nullptr, u64[3], u64[4], a.lists ? u8[1] : nullptr,
                                        a.capacity, &total, nullptr);
        }
    };

    struct Case {
        const char *what;
        Args a;
    };
    auto with = [&](auto change) {
        Args a = ok;
        change(a);
        return a;
    };
    const std::vector<Case> cases = {
        {"no text", with([](Args &a) { a.text = nullptr; })},
        {"n == 0", with([](Args &a) { a.n = 0; })},
        {"n == 2^31", with([](Args &a) { a.n = 1ull << 31; })},
        {"no blob", with([](Args &a) { a.pat = nullptr; })},
        {"no offsets", with([](Args &a) { a.off = nullptr; })},
        {"no output", with([](Args &a) { a.out = false; })},
        {"no list behind a capacity", with([](Args &a) { a.lists = false; })},
        {"no list, capacity 0", with([](Args &a) { a.lists = false, a.capacity = 0; })},
        {"min_len == 0", with([](Args &a) { a.min_len = 0; })},
        {"max_occ == 0", with([](Args &a) { a.max_occ = 0; })},
        {"k < 0", with([](Args &a) { a.k = -1; })},
        {"k above the limit", with([](Args &a) { a.k = BMX_MAP_MAX_K + 1; })},
        {"count == 0", with([](Args &a) { a.count = 0; })},
        {"count == 0, nothing else", with([](Args &a) { a.count = 0, a.pat = nullptr, a.off = nullptr, a.out = a.lists = false; })},
        {"an offset that decreases", with([&](Args &a) { a.off = falls; })},
        {"an end past the blob", with([&](Args &a) { a.off = past; })},
        {"a query of no byte", with([&](Args &a) { a.off = empty; })},
        {"a query above the limit",
         with([&](Args &a) { a.pat = long_blob.data(), a.pat_bytes = long_blob.size(), a.off = long_off, a.count = 1; })},
        {"a byte >= 0x80", with([&](Args &a) { a.pat = high; })},
        {"valid", ok},
    };
    const char *names[5] = {"count", "locate", "match", "seeds", "map"};
    char label[96];
    for (int e = 0; e < 5; ++e)
        for (const Case &c : cases) {
            snprintf(label, sizeof label, "bmx_index_%s: %s", names[e], c.what);
            const int rc = host(e, c.a);
            say(label, rc);
            if (e != 0 && e != 2) printf("%-44s total %llu\n", "", (unsigned long long)total);
        }
    for (int e = 0; e < 5; ++e)
        for (const Case &c : cases) {
            if (!c.a.text || c.a.n != n) continue; // the device entries take no text
            Args a = c.a;
            a.pat = a.pat ? dev : nullptr; // (a device entry does not read its queries on the host)
            snprintf(label, sizeof label, "bmx_index_%s_device: %s", names[e], c.what);
            say(label, device(e, a));
        }
    bmx_index *ix = reinterpret_cast<bmx_index *>(dev);
    say("bmx_index_create_device: no context", bmx_index_create_device(nullptr, dev, n, nullptr, nullptr, &ix));
    return 0;
}
