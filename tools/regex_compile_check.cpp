// regex_compile_check.cpp -- bmx_compile_regex under AddressSanitizer and UBSan, on a machine WITHOUT a GPU: a table of
// tests/test_regex_cpu.py's kind (each expression with its expected return code, position count and shortest / longest
// match), then 200,000 random byte strings as expressions under each flag combination.  Every expression sits in a heap
// buffer of exactly its length and the automaton in a heap buffer of exactly sizeof(bmx_regex), so a read or a write one
// byte past either is reported.  A successful compile must give a valid automaton (1 <= m <= 64, first and last non-zero
// and inside m, follow upward only and inside m, nothing set behind position m - 1) with 1 <= min_len <= max_len <= m;
// a failed one must leave *out untouched.
//
// A stand-alone program, not a test and never loaded into Python.  Build it with the two compilers' sources instrumented
// (from parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc):
//     g++ -O1 -g -std=c++17 -I../../include -I. -fsanitize=address,undefined -fno-sanitize-recover=all \
//         bmx_regex_compile.cpp bmx_classes_compile.cpp ../../tools/regex_compile_check.cpp -o regex_compile_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>

#include "bmx.h"

// the library's shim keeps the text of bmx_last_error; here it only has to be a string that can be read to its end
static std::string g_last_error;
void bmx_internal_set_error(const char *text) { g_last_error = text; }

namespace {

struct Result {
    int rc;
    bmx_regex re;
    bool untouched;
};

Result compile(const void *expr, uint64_t len, uint32_t flags)
{
    std::unique_ptr<char[]> e(new char[len ? len : 1]); // exactly the expression: nothing behind it is readable
    std::memcpy(e.get(), expr, len);
    std::unique_ptr<bmx_regex> out(new bmx_regex);
    std::memset(out.get(), 0xA5, sizeof(bmx_regex));
    Result r;
    r.rc = bmx_compile_regex(e.get(), len, flags, out.get());
    r.re = *out;
    r.untouched = true;
    const uint8_t *raw = reinterpret_cast<const uint8_t *>(out.get());
    for (size_t i = 0; i < sizeof(bmx_regex) && r.untouched; ++i) r.untouched = raw[i] == 0xA5;
    return r;
}

bool sane(const Result &r)
{
    if (r.rc != BMX_OK) return r.rc == BMX_ERR_ARG && r.untouched && g_last_error.rfind("bmx_compile_regex: ", 0) == 0;
    const bmx_regex &a = r.re;
    if (a.m < 1 || a.m > BMX_MAX_REGEX_POSITIONS || a.first == 0 || a.last == 0) return false;
    const uint64_t all = a.m == 64 ? ~0ull : (1ull << a.m) - 1;
    if ((a.first | a.last) & ~all) return false;
    for (int i = 0; i < BMX_MAX_REGEX_POSITIONS; ++i) {
        const uint64_t above = i >= 63 ? 0 : ~0ull << (i + 1);
        if (a.follow[i] & ~(i < a.m ? all & above : 0)) return false;
    }
    for (int i = a.m * BMX_CLASS_BYTES; i < BMX_MAX_REGEX_POSITIONS * BMX_CLASS_BYTES; ++i)
        if (a.classes[i] != 0) return false;
    return 1 <= a.min_len && a.min_len <= a.max_len && a.max_len <= a.m;
}

struct Case {
    const char *expr;
    uint32_t flags;
    int rc;
    int32_t m, min_len, max_len;
};

const uint32_t I = BMX_CLASS_ICASE, U = BMX_CLASS_IUPAC;
const Case TABLE[] = {
    {"a", 0, BMX_OK, 1, 1, 1},
    {"abc", 0, BMX_OK, 3, 3, 3},
    {"a|b", 0, BMX_OK, 2, 1, 1},
    {"(a|)b", 0, BMX_OK, 2, 1, 2},
    {"(ab){2,3}", 0, BMX_OK, 6, 4, 6},
    {"(a|bc)d", 0, BMX_OK, 4, 2, 3},
    {"a(b|c)?d", 0, BMX_OK, 4, 2, 3},
    {"(a?b?){2}c", 0, BMX_OK, 5, 1, 5},
    {"()a(){3}", 0, BMX_OK, 1, 1, 1},
    {"\\(\\)\\|\\?\\{\\*\\+", 0, BMX_OK, 7, 7, 7},
    {"[()|?{*+]{2}", 0, BMX_OK, 2, 2, 2},
    {"aB|c", I, BMX_OK, 3, 1, 2},
    {"AC(N|R{2})T", U, BMX_OK, 6, 4, 5},
    {"(r|Y)n", I | U, BMX_OK, 3, 2, 2},
    {"x{64}", 0, BMX_OK, 64, 64, 64},
    {"(a|b){1,32}", 0, BMX_OK, 64, 1, 32},
    {"ATG([ACGT]{3}){2,4}(TAA|TAG|TGA)", 0, BMX_OK, 24, 12, 18},
    {"(ERROR|FATAL|PANIC): [0-9]{2,4}", 0, BMX_OK, 21, 9, 11},
    {"([0-9]{1,3}\\.){3}[0-9]{1,3}", 0, BMX_OK, 15, 7, 15},
    {"(RGD|KGD)x{2,5}[ST]", 0, BMX_OK, 12, 6, 9},
    {"((((((((((((((((((((((((((((((((a))))))))))))))))))))))))))))))))", 0, BMX_OK, 1, 1, 1},
    {"(((((((((((((((((((((((((((((((((a)))))))))))))))))))))))))))))))))", 0, BMX_ERR_ARG, 0, 0, 0},
    {"", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a*", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a)+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{2,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(", 0, BMX_ERR_ARG, 0, 0, 0},
    {")", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a))", 0, BMX_ERR_ARG, 0, 0, 0},
    {"((a)", 0, BMX_ERR_ARG, 0, 0, 0},
    {"?a", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(?:a)", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a??", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a){2}{3}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{0}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{3,2}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{2,3", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{65}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(ab){33}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{99999999999999999999}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"((){999}){999}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"()", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a?", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a|", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a?b?){2}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"[abc", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a|[b)", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a\\", 0, BMX_ERR_ARG, 0, 0, 0},
    {"[\\x4", 0, BMX_ERR_ARG, 0, 0, 0},
    {"abc", 4, BMX_ERR_ARG, 0, 0, 0},
};

} // namespace

int main()
{
    int bad = 0;
    for (const Case &c : TABLE) {
        const Result r = compile(c.expr, std::strlen(c.expr), c.flags);
        const bool ok = sane(r) && r.rc == c.rc &&
                        (r.rc != BMX_OK || (r.re.m == c.m && r.re.min_len == c.min_len && r.re.max_len == c.max_len));
        if (!ok) {
            printf("TABLE %-44s flags %u: rc %d m %d lengths %d..%d\n", c.expr, c.flags, r.rc, r.re.m, r.re.min_len, r.re.max_len);
            ++bad;
        }
    }
    // random expressions: bytes drawn mostly from the grammar's own alphabet, now and then any byte value
    static const char alphabet[] = "ab]^-[\\.xN?{},0123*+()|()|AC";
    std::mt19937_64 rng(0x2E6E0C0DEull);
    uint64_t compiled[4] = {0, 0, 0, 0};
    for (uint32_t flags = 0; flags < 4; ++flags) {
        for (int i = 0; i < 200000; ++i) {
            uint8_t e[40];
            const uint64_t len = rng() % (sizeof e + 1);
            for (uint64_t j = 0; j < len; ++j) e[j] = rng() % 8 ? (uint8_t)alphabet[rng() % (sizeof alphabet - 1)] : (uint8_t)rng();
            const uint32_t f = flags | (rng() % 16 ? 0u : 4u << (rng() % 8)); // now and then an unknown bit
            const Result r = compile(e, len, f);
            compiled[flags] += r.rc == BMX_OK;
            if (!sane(r) || (r.rc == BMX_OK && f != flags)) {
                printf("RANDOM case %d flags %u: rc %d m %d untouched %d\n", i, f, r.rc, r.re.m, (int)r.untouched);
                ++bad;
            }
        }
    }
    // NULL arguments
    bmx_regex out;
    bad += bmx_compile_regex(nullptr, 0, 0, &out) != BMX_ERR_ARG;
    bad += bmx_compile_regex("a", 1, 0, nullptr) != BMX_ERR_ARG;
    printf("%zu table cases, 4 x 200000 random expressions (%llu, %llu, %llu, %llu compiled), %d failures\n",
           sizeof TABLE / sizeof TABLE[0], (unsigned long long)compiled[0], (unsigned long long)compiled[1],
           (unsigned long long)compiled[2], (unsigned long long)compiled[3], bad);
    return bad != 0;
}
