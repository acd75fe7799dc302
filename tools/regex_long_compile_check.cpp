// regex_long_compile_check.cpp -- bmx_compile_regex_long and bmx_regex_long_widen under AddressSanitizer and UBSan, on a
// machine WITHOUT a GPU: a table of expressions around 64, 65, 127, 128 and 129 positions (each with its expected return
// code, position count and shortest / longest match), then 200,000 random byte strings as expressions under each flag
// combination, half of them with a counted repeat behind them that reaches past 64 and past 128 positions.  Every
// expression sits in a heap buffer of exactly its length and the automaton in a heap buffer of exactly
// sizeof(bmx_regex_long), so a read or a write one byte past either is reported.  A successful compile must give a valid
// automaton (1 <= m <= 128, first and last non-empty and inside m, follow upward only and inside m, nothing set behind
// position m - 1, pad 0) with 1 <= min_len <= max_len <= m, and where bmx_compile_regex takes the expression too, the
// widened output of that entry byte for byte; a failed one must leave *out untouched.
//
// A stand-alone program, not a test and never loaded into Python.  Build it with the two compilers' sources instrumented
// (from parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc):
//     g++ -O1 -g -std=c++17 -I../../include -I. -fsanitize=address,undefined -fno-sanitize-recover=all \
//         bmx_regex_compile.cpp bmx_classes_compile.cpp ../../tools/regex_long_compile_check.cpp -o regex_long_compile_check
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

typedef unsigned __int128 Set;

struct Result {
    int rc;
    bmx_regex_long re;
    bool untouched;
};

Result compile(const void *expr, uint64_t len, uint32_t flags)
{
    std::unique_ptr<char[]> e(new char[len ? len : 1]); // exactly the expression: nothing behind it is readable
    std::memcpy(e.get(), expr, len);
    std::unique_ptr<bmx_regex_long> out(new bmx_regex_long);
    std::memset(out.get(), 0xA5, sizeof(bmx_regex_long));
    Result r;
    r.rc = bmx_compile_regex_long(e.get(), len, flags, out.get());
    r.re = *out;
    r.untouched = true;
    const uint8_t *raw = reinterpret_cast<const uint8_t *>(out.get());
    for (size_t i = 0; i < sizeof(bmx_regex_long) && r.untouched; ++i) r.untouched = raw[i] == 0xA5;
    if (r.rc == BMX_OK) { // against the 64-position entry through the widening, each in a buffer of its own size
        std::unique_ptr<bmx_regex> small(new bmx_regex);
        std::unique_ptr<bmx_regex_long> wide(new bmx_regex_long);
        if (bmx_compile_regex(e.get(), len, flags, small.get()) == BMX_OK) {
            if (r.re.m > BMX_MAX_REGEX_POSITIONS || bmx_regex_long_widen(small.get(), wide.get()) != BMX_OK ||
                std::memcmp(wide.get(), out.get(), sizeof(bmx_regex_long)) != 0)
                r.rc = -100; // the two entries disagree
        } else if (r.re.m <= BMX_MAX_REGEX_POSITIONS) {
            r.rc = -101; // the short entry refuses what fits it
        }
    }
    return r;
}

Set load(const uint64_t w[2]) { return (Set)w[0] | ((Set)w[1] << 64); }

bool sane(const Result &r)
{
    if (r.rc != BMX_OK) return r.rc == BMX_ERR_ARG && r.untouched && g_last_error.rfind("bmx_compile_regex_long: ", 0) == 0;
    const bmx_regex_long &a = r.re;
    if (a.m < 1 || a.m > BMX_MAX_REGEX_LONG_POSITIONS || a.pad != 0) return false;
    const Set first = load(a.first), last = load(a.last);
    if (first == 0 || last == 0) return false;
    const Set all = a.m == 128 ? ~(Set)0 : ((Set)1 << a.m) - 1;
    if ((first | last) & ~all) return false;
    for (int i = 0; i < BMX_MAX_REGEX_LONG_POSITIONS; ++i) {
        const Set above = i >= 127 ? (Set)0 : ~(Set)0 << (i + 1);
        if (load(a.follow[i]) & ~(i < a.m ? all & above : (Set)0)) return false;
    }
    for (int i = a.m * BMX_CLASS_BYTES; i < BMX_MAX_REGEX_LONG_POSITIONS * BMX_CLASS_BYTES; ++i)
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
    {"(a|bc)d", 0, BMX_OK, 4, 2, 3},
    {"(r|Y)n", I | U, BMX_OK, 3, 2, 2},
    {"x{63}", 0, BMX_OK, 63, 63, 63},
    {"x{64}", 0, BMX_OK, 64, 64, 64},
    {"x{65}", 0, BMX_OK, 65, 65, 65},
    {"x{63}y?", 0, BMX_OK, 64, 63, 64},
    {"x{64}y?", 0, BMX_OK, 65, 64, 65},
    {"(a|b){1,32}", 0, BMX_OK, 64, 1, 32},
    {"(a|b){1,33}", 0, BMX_OK, 66, 1, 33},
    {"(ab){32}", 0, BMX_OK, 64, 64, 64},
    {"(ab){33}", 0, BMX_OK, 66, 66, 66},
    {"x{127}", 0, BMX_OK, 127, 127, 127},
    {"x{128}", 0, BMX_OK, 128, 128, 128},
    {"x{129}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"x{127}y?", 0, BMX_OK, 128, 127, 128},
    {"x{128}y?", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(ab){64}", 0, BMX_OK, 128, 128, 128},
    {"(ab){65}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a|b){1,64}", 0, BMX_OK, 128, 1, 64},
    {"(a|b){1,65}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(abc|de){1,25}f", 0, BMX_OK, 126, 3, 76},
    {"(x{64}){2}", 0, BMX_OK, 128, 128, 128},
    {"(x{64}){3}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(x{43}){0,3}y", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(x{42}){0,3}y", 0, BMX_OK, 127, 1, 127},
    {"a.{0,100}b", 0, BMX_OK, 102, 2, 102},
    {"ATG([ACGT]{3}){2,38}(TAA|TAG|TGA)", 0, BMX_OK, 126, 12, 120},
    {"ATG([ACGT]{3}){2,40}(TAA|TAG|TGA)", 0, BMX_ERR_ARG, 0, 0, 0},
    {"C.{2,4}C.{20,40}[LIVMFYWC].{8,16}H.{3,5}H", 0, BMX_OK, 70, 38, 70},
    {"(ERROR|FATAL|PANIC|WARNING|CRITICAL|EXCEPTION|TIMEOUT|REFUSED|DENIED|ABORTED): [0-9]{2,4}", 0, BMX_OK, 72, 9, 15},
    {"(ERROR|FATAL|PANIC|WARNING|CRITICAL|EXCEPTION|TIMEOUT|REFUSED|DENIED|ABORTED): [0-9]{2,4}", I, BMX_OK, 72, 9, 15},
    {"((((((((((((((((((((((((((((((((a{128}))))))))))))))))))))))))))))))))", 0, BMX_OK, 128, 128, 128},
    {"(((((((((((((((((((((((((((((((((a)))))))))))))))))))))))))))))))))", 0, BMX_ERR_ARG, 0, 0, 0},
    {"", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a*", 0, BMX_ERR_ARG, 0, 0, 0},
    {"(a)+", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{2,}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{99999999999999999999}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"((){999}){999}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a{999}", 0, BMX_ERR_ARG, 0, 0, 0},
    {"a?", 0, BMX_ERR_ARG, 0, 0, 0},
    {"[abc", 0, BMX_ERR_ARG, 0, 0, 0},
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
    // random expressions: bytes drawn mostly from the grammar's own alphabet, now and then any byte value; every other
    // one in a group with a count of 20..149 behind it
    static const char alphabet[] = "ab]^-[\\.xN?{},0123*+()|()|AC";
    std::mt19937_64 rng(0x331C0C0DEull);
    uint64_t compiled[4] = {0, 0, 0, 0}, wide[4] = {0, 0, 0, 0};
    for (uint32_t flags = 0; flags < 4; ++flags) {
        for (int i = 0; i < 200000; ++i) {
            uint8_t e[48];
            uint64_t len = rng() % 41;
            for (uint64_t j = 0; j < len; ++j) e[j] = rng() % 8 ? (uint8_t)alphabet[rng() % (sizeof alphabet - 1)] : (uint8_t)rng();
            if (i & 1) {
                char tail[8];
                const int t = snprintf(tail, sizeof tail, "{%d}", (int)(20 + rng() % 130));
                std::memcpy(e + len, tail, (size_t)t);
                len += (uint64_t)t;
            }
            const uint32_t f = flags | (rng() % 16 ? 0u : 4u << (rng() % 8)); // now and then an unknown bit
            const Result r = compile(e, len, f);
            compiled[flags] += r.rc == BMX_OK;
            wide[flags] += r.rc == BMX_OK && r.re.m > BMX_MAX_REGEX_POSITIONS;
            if (!sane(r) || (r.rc == BMX_OK && f != flags)) {
                printf("RANDOM case %d flags %u: rc %d m %d untouched %d\n", i, f, r.rc, r.re.m, (int)r.untouched);
                ++bad;
            }
        }
    }
    // NULL arguments
    std::unique_ptr<bmx_regex_long> out(new bmx_regex_long);
    std::unique_ptr<bmx_regex> small(new bmx_regex);
    bad += bmx_compile_regex_long(nullptr, 0, 0, out.get()) != BMX_ERR_ARG;
    bad += bmx_compile_regex_long("a", 1, 0, nullptr) != BMX_ERR_ARG;
    bad += bmx_regex_long_widen(nullptr, out.get()) != BMX_ERR_ARG;
    bad += bmx_compile_regex("ab", 2, 0, small.get()) != BMX_OK;
    bad += bmx_regex_long_widen(small.get(), nullptr) != BMX_ERR_ARG;
    small->follow[1] = 1; // downward
    bad += bmx_regex_long_widen(small.get(), out.get()) != BMX_ERR_ARG;
    printf("%zu table cases, 4 x 200000 random expressions (%llu, %llu, %llu, %llu compiled; %llu, %llu, %llu, %llu of them past 64 "
           "positions), %d failures\n",
           sizeof TABLE / sizeof TABLE[0], (unsigned long long)compiled[0], (unsigned long long)compiled[1],
           (unsigned long long)compiled[2], (unsigned long long)compiled[3], (unsigned long long)wide[0], (unsigned long long)wide[1],
           (unsigned long long)wide[2], (unsigned long long)wide[3], bad);
    return bad != 0;
}
