// gaps_compile_check.cpp -- bmx_compile_gaps under AddressSanitizer and UBSan, on a machine WITHOUT a GPU: the table of
// tests/test_gaps_cpu.py's kind (each expression with its expected return code, position count and optional mask), then
// 200,000 random byte strings as expressions in both syntaxes and under every flag.  Every expression sits in a heap
// buffer of exactly its length and the outputs in heap buffers of exactly 64 classes, so a read or a write one byte past
// either is reported.  A successful compile must give 1 <= m <= 64, no optional bit at or above m and a mandatory
// position; a failed one must leave the outputs untouched.
//
// A stand-alone program, not a test and never loaded into Python.  Build it with the two compilers' sources instrumented
// (from parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc):
//     g++ -O1 -g -std=c++17 -I../../include -fsanitize=address,undefined -fno-sanitize-recover=all \
//         bmx_gaps_compile.cpp bmx_classes_compile.cpp ../../tools/gaps_compile_check.cpp -o gaps_compile_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

#include "bmx.h"

namespace {

struct Result {
    int rc;
    int32_t m;
    uint64_t optional;
    bool untouched;
};

Result compile(const void *expr, uint64_t len, uint32_t flags)
{
    std::unique_ptr<char[]> e(new char[len ? len : 1]); // exactly the expression: nothing behind it is readable
    std::memcpy(e.get(), expr, len);
    std::unique_ptr<uint8_t[]> classes(new uint8_t[BMX_MAX_GAPS_PATTERN * BMX_CLASS_BYTES]);
    std::memset(classes.get(), 0xA5, BMX_MAX_GAPS_PATTERN * BMX_CLASS_BYTES);
    std::unique_ptr<uint64_t> optional(new uint64_t(0xDEAD));
    std::unique_ptr<int32_t> m(new int32_t(-7));
    Result r;
    r.rc = bmx_compile_gaps(e.get(), len, flags, classes.get(), optional.get(), m.get());
    r.m = *m;
    r.optional = *optional;
    r.untouched = *m == -7 && *optional == 0xDEAD;
    for (int i = 0; i < BMX_MAX_GAPS_PATTERN * BMX_CLASS_BYTES && r.untouched; ++i) r.untouched = classes[i] == 0xA5;
    return r;
}

bool sane(const Result &r)
{
    if (r.rc != BMX_OK) return r.rc == BMX_ERR_ARG && r.untouched;
    if (r.m < 1 || r.m > BMX_MAX_GAPS_PATTERN) return false;
    const uint64_t all = r.m == 64 ? ~0ull : (1ull << r.m) - 1;
    return (r.optional & ~all) == 0 && r.optional != all;
}

struct Case {
    const char *expr;
    uint32_t flags;
    int rc;
    int32_t m;
    uint64_t optional;
};

const uint32_t P = BMX_GAPS_PROSITE, I = BMX_CLASS_ICASE, U = BMX_CLASS_IUPAC;
const Case TABLE[] = {
    {"abc", 0, BMX_OK, 3, 0},
    {"colou?r", 0, BMX_OK, 6, 1u << 4},
    {"a{1,3}b", 0, BMX_OK, 4, 6},
    {"a.{0,2}b", 0, BMX_OK, 4, 6},
    {"a?b?c", 0, BMX_OK, 3, 3},
    {"[a-c]{2,3}[^x]?y", 0, BMX_OK, 5, 12},
    {"\\?\\{\\*\\+", 0, BMX_OK, 4, 0},
    {"[?{*+]{2}", 0, BMX_OK, 2, 0},
    {"x{64}", 0, BMX_OK, 64, 0},
    {"a{1,64}", 0, BMX_OK, 64, ~1ull},
    {"a.{0,62}b", 0, BMX_OK, 64, (~0ull >> 2) << 1},
    {"aB?", I, BMX_OK, 2, 2},
    {"ACN{1,3}GT", U, BMX_OK, 7, 24},
    {"C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H", P, BMX_OK, 25, (3ull << 3) | (3ull << 22)},
    {"A-x-{PG}(2)-[ST](0,1)-B.", P, BMX_OK, 6, 16},
    {"a-[bc]-{d}", P | I, BMX_OK, 3, 0},
    {"", 0, BMX_ERR_ARG, 0, 0},
    {"a*", 0, BMX_ERR_ARG, 0, 0},
    {"a+", 0, BMX_ERR_ARG, 0, 0},
    {"a{2,}", 0, BMX_ERR_ARG, 0, 0},
    {"?a", 0, BMX_ERR_ARG, 0, 0},
    {"a??", 0, BMX_ERR_ARG, 0, 0},
    {"a{2}{3}", 0, BMX_ERR_ARG, 0, 0},
    {"a{0}", 0, BMX_ERR_ARG, 0, 0},
    {"a{3,2}", 0, BMX_ERR_ARG, 0, 0},
    {"a{", 0, BMX_ERR_ARG, 0, 0},
    {"a{2,3", 0, BMX_ERR_ARG, 0, 0},
    {"a{65}", 0, BMX_ERR_ARG, 0, 0},
    {"a{99999999999999999999}", 0, BMX_ERR_ARG, 0, 0},
    {"a?", 0, BMX_ERR_ARG, 0, 0},
    {".{0,64}", 0, BMX_ERR_ARG, 0, 0},
    {"[abc", 0, BMX_ERR_ARG, 0, 0},
    {"a\\", 0, BMX_ERR_ARG, 0, 0},
    {"[\\x4", 0, BMX_ERR_ARG, 0, 0},
    {"[a-\\", 0, BMX_ERR_ARG, 0, 0},
    {"<A-x", P, BMX_ERR_ARG, 0, 0},
    {"A-x>", P, BMX_ERR_ARG, 0, 0},
    {"A-[BC", P, BMX_ERR_ARG, 0, 0},
    {"A-x(2", P, BMX_ERR_ARG, 0, 0},
    {"A-", P, BMX_ERR_ARG, 0, 0},
    {"A-x", P | U, BMX_ERR_ARG, 0, 0},
    {"abc", 8, BMX_ERR_ARG, 0, 0},
};

} // namespace

int main()
{
    int bad = 0;
    for (const Case &c : TABLE) {
        const Result r = compile(c.expr, std::strlen(c.expr), c.flags);
        const bool ok = sane(r) && r.rc == c.rc && (r.rc != BMX_OK || (r.m == c.m && r.optional == c.optional));
        if (!ok) {
            printf("TABLE %-44s flags %u: rc %d m %d optional %llx\n", c.expr, c.flags, r.rc, r.m, (unsigned long long)r.optional);
            ++bad;
        }
    }
    // random expressions: bytes drawn mostly from the grammar's own alphabet, now and then any byte value
    static const char alphabet[] = "ab]^-[\\.xN?{},0123*+()<>AC";
    std::mt19937_64 rng(0x6A95C0DEull);
    uint64_t compiled = 0;
    for (int i = 0; i < 200000; ++i) {
        uint8_t e[40];
        const uint64_t len = rng() % (sizeof e + 1);
        for (uint64_t j = 0; j < len; ++j) e[j] = rng() % 8 ? (uint8_t)alphabet[rng() % (sizeof alphabet - 1)] : (uint8_t)rng();
        const uint32_t flags = (uint32_t)(rng() % 8) | (rng() % 16 ? 0u : 8u); // now and then an unknown bit
        const Result r = compile(e, len, flags);
        compiled += r.rc == BMX_OK;
        if (!sane(r)) {
            printf("RANDOM case %d flags %u: rc %d m %d optional %llx untouched %d\n", i, flags, r.rc, r.m,
                   (unsigned long long)r.optional, (int)r.untouched);
            ++bad;
        }
    }
    // NULL arguments
    uint8_t classes[BMX_MAX_GAPS_PATTERN * BMX_CLASS_BYTES];
    uint64_t optional = 0;
    int32_t m = 0;
    bad += bmx_compile_gaps(nullptr, 0, 0, classes, &optional, &m) != BMX_ERR_ARG;
    bad += bmx_compile_gaps("a", 1, 0, nullptr, &optional, &m) != BMX_ERR_ARG;
    bad += bmx_compile_gaps("a", 1, 0, classes, nullptr, &m) != BMX_ERR_ARG;
    bad += bmx_compile_gaps("a", 1, 0, classes, &optional, nullptr) != BMX_ERR_ARG;
    printf("%zu table cases, 200000 random expressions (%llu compiled), %d failures\n", sizeof TABLE / sizeof TABLE[0],
           (unsigned long long)compiled, bad);
    return bad != 0;
}
