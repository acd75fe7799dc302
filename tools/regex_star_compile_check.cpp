// regex_star_compile_check.cpp -- bmx_compile_regex_star under AddressSanitizer and UBSan, on a machine WITHOUT a GPU,
// after regex_compile_check.cpp: a table (each expression with its expected return code, position count and shortest /
// longest match, BMX_REGEX_UNBOUNDED where there is a cycle), then 200,000 random byte strings as expressions under each
// flag combination.  Every expression sits in a heap buffer of exactly its length and the automaton in a heap buffer of
// exactly sizeof(bmx_regex), so a read or a write one byte past either is reported.  A successful compile must give an
// automaton that is valid for the entries that take a cycle (1 <= m <= 64, first and last non-zero and inside m, follow
// inside m, nothing set behind position m - 1) with 1 <= min_len and max_len either unbounded or in [min_len, m]; where
// bmx_compile_regex takes the expression too, it must give the same bytes; a failed compile must leave *out untouched.
//
// A stand-alone program, not a test and never loaded into Python.  Build it with the two compilers' sources instrumented
// (from parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc):
//     g++ -O1 -g -std=c++17 -I../../include -I. -fsanitize=address,undefined -fno-sanitize-recover=all \
//         bmx_regex_compile.cpp bmx_classes_compile.cpp ../../tools/regex_star_compile_check.cpp -o regex_star_compile_check
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

Result compile(const void *expr, uint64_t len, uint32_t flags, bool star = true)
{
    std::unique_ptr<char[]> e(new char[len ? len : 1]); // exactly the expression: nothing behind it is readable
    std::memcpy(e.get(), expr, len);
    std::unique_ptr<bmx_regex> out(new bmx_regex);
    std::memset(out.get(), 0xA5, sizeof(bmx_regex));
    Result r;
    r.rc = star ? bmx_compile_regex_star(e.get(), len, flags, out.get()) : bmx_compile_regex(e.get(), len, flags, out.get());
    r.re = *out;
    r.untouched = true;
    const uint8_t *raw = reinterpret_cast<const uint8_t *>(out.get());
    for (size_t i = 0; i < sizeof(bmx_regex) && r.untouched; ++i) r.untouched = raw[i] == 0xA5;
    return r;
}

bool sane(const Result &r)
{
    if (r.rc != BMX_OK) return r.rc == BMX_ERR_ARG && r.untouched && g_last_error.rfind("bmx_compile_regex_star: ", 0) == 0;
    const bmx_regex &a = r.re;
    if (a.m < 1 || a.m > BMX_MAX_REGEX_POSITIONS || a.first == 0 || a.last == 0) return false;
    const uint64_t all = a.m == 64 ? ~0ull : (1ull << a.m) - 1;
    if ((a.first | a.last) & ~all) return false;
    for (int i = 0; i < BMX_MAX_REGEX_POSITIONS; ++i)
        if (a.follow[i] & ~(i < a.m ? all : 0)) return false;
    for (int i = a.m * BMX_CLASS_BYTES; i < BMX_MAX_REGEX_POSITIONS * BMX_CLASS_BYTES; ++i)
        if (a.classes[i] != 0) return false;
    if (a.min_len < 1) return false;
    return a.max_len == BMX_REGEX_UNBOUNDED || (a.min_len <= a.max_len && a.max_len <= a.m);
}

struct Case {
    const char *expr;
    uint32_t flags;
    int rc;
    int32_t m, min_len, max_len;
};

const uint32_t I = BMX_CLASS_ICASE, U = BMX_CLASS_IUPAC;
const int32_t INF = BMX_REGEX_UNBOUNDED;
const Case TABLE[] = {
    {"a+", 0, BMX_OK, 1, 1, INF},
    {"a*b", 0, BMX_OK, 2, 1, INF},
    {"ab*", 0, BMX_OK, 2, 1, INF},
    {"a{2,}", 0, BMX_OK, 2, 2, INF},
    {"a{0,}b", 0, BMX_OK, 2, 1, INF},
    {"a{64,}", 0, BMX_OK, 64, 64, INF},
    {"(ab)+", 0, BMX_OK, 2, 2, INF},
    {"(ab){2,}", 0, BMX_OK, 4, 4, INF},
    {"((ab)+c)*d", 0, BMX_OK, 4, 1, INF},
    {"(a?b)+", 0, BMX_OK, 2, 1, INF},
    {"()a+(){3}", 0, BMX_OK, 1, 1, INF},
    {"aB+", I, BMX_OK, 2, 2, INF},
    {"AN+T", U, BMX_OK, 3, 3, INF},
    {"x{63}y+", 0, BMX_OK, 64, 64, INF},
    {"(x{32})+", 0, BMX_OK, 32, 32, INF},
    {"ERROR.*timeout", 0, BMX_OK, 13, 12, INF},
    {"[0-9]+\\.[0-9]+", 0, BMX_OK, 3, 3, INF},
    {"ATG([ACGT]{3})+(TAA|TAG|TGA)", 0, BMX_OK, 15, 9, INF},
    {"[A-Za-z_][A-Za-z0-9_]*\\(", 0, BMX_OK, 3, 2, INF},
    {"abc", 0, BMX_OK, 3, 3, 3},
    {"(ab){2,3}", 0, BMX_OK, 6, 4, 6},
    {"(ERROR|FATAL|PANIC): [0-9]{2,4}", 0, BMX_OK, 21, 9, 11},
    {"((((((((((((((((((((((((((((((((a+))))))))))))))))))))))))))))))))", 0, BMX_OK, 1, 1, INF},
    {"(((((((((((((((((((((((((((((((((a+)))))))))))))))))))))))))))))))))", 0, BMX_ERR_ARG, 0, 0, 0},
    {"", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a*", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(ab)*", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a+)?", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{0,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"*", 0, BMX_ERR_ARG, 0, 0, 0},
    {"+a", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a**", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a+?", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a?+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{2,}{3}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{2,", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{65,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{64}b+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(ab){33,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{99999999999999999999,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"((){999,}){999,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"()+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"[abc+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a+\\", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a+", 4, BMX_ERR_ARG, 0, 0, 0},
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
    static const char alphabet[] = "ab]^-[\\.xN?{},0123*+()|()|AC*+";
    std::mt19937_64 rng(0x57A20C0DEull);
    uint64_t compiled[4] = {0, 0, 0, 0}, cyclic = 0, same = 0;
    for (uint32_t flags = 0; flags < 4; ++flags) {
        for (int i = 0; i < 200000; ++i) {
            uint8_t e[40];
            const uint64_t len = rng() % (sizeof e + 1);
            for (uint64_t j = 0; j < len; ++j) e[j] = rng() % 8 ? (uint8_t)alphabet[rng() % (sizeof alphabet - 1)] : (uint8_t)rng();
            const uint32_t f = flags | (rng() % 16 ? 0u : 4u << (rng() % 8)); // now and then an unknown bit
            const Result r = compile(e, len, f);
            compiled[flags] += r.rc == BMX_OK;
            bool ok = sane(r) && !(r.rc == BMX_OK && f != flags);
            if (ok && r.rc == BMX_OK) {
                cyclic += r.re.max_len == BMX_REGEX_UNBOUNDED;
                const Result old = compile(e, len, f, false);
                if (old.rc == BMX_OK) { // a star-free expression: byte for byte
                    ok = std::memcmp(&old.re, &r.re, sizeof(bmx_regex)) == 0;
                    ++same;
                } // (refused there for spelling * + or {a,}, even around an empty group, where nothing loops)
            }
            if (!ok) {
                printf("RANDOM case %d flags %u: rc %d m %d untouched %d\n", i, f, r.rc, r.re.m, (int)r.untouched);
                ++bad;
            }
        }
    }
    // NULL arguments
    bmx_regex out;
    bad += bmx_compile_regex_star(nullptr, 0, 0, &out) != BMX_ERR_ARG;
    bad += bmx_compile_regex_star("a", 1, 0, nullptr) != BMX_ERR_ARG;
    printf("%zu table cases, 4 x 200000 random expressions (%llu, %llu, %llu, %llu compiled, %llu with a cycle, %llu equal to "
           "bmx_compile_regex's), %d failures\n",
           sizeof TABLE / sizeof TABLE[0], (unsigned long long)compiled[0], (unsigned long long)compiled[1],
           (unsigned long long)compiled[2], (unsigned long long)compiled[3], (unsigned long long)cyclic, (unsigned long long)same, bad);
    return bad != 0;
}
