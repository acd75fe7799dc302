// regex_groups_compile_check.cpp -- bmx_compile_regex_groups, bmx_regex_groups_valid and bmx_compile_template under
// AddressSanitizer and UBSan, on a machine WITHOUT a GPU: the fixed expressions of the capture model, the refused ones,
// 200,000 random strings over the bytes of the grammar as expressions, and the accepted and refused template forms plus
// 200,000 random templates.  Every expression and template sits in a heap buffer of exactly its length and every output
// in a heap buffer of exactly its size, so a read or a write one byte past either is reported.  A successful compile must
// give a pair that bmx_regex_groups_valid accepts and the automaton of bmx_compile_regex for the expression with every (?:
// written as (; a failed one must leave both outputs untouched.
//
// A stand-alone program, not a test and never loaded into Python.  Build it with the two compilers' sources instrumented
// (from parallel_implementation_of_string_matching_algorithms_opencl_amd/csrc):
//     g++ -O1 -g -std=c++17 -I../../include -I. -fsanitize=address,undefined -fno-sanitize-recover=all \
//         bmx_regex_compile.cpp bmx_classes_compile.cpp ../../tools/regex_groups_compile_check.cpp -o regex_groups_compile_check
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

int failures = 0;
void fail(const char *what, const std::string &expr)
{
    std::printf("FAIL %s: %s\n", what, expr.c_str());
    ++failures;
}

template <typename T>
bool untouched(const T *p)
{
    const uint8_t *raw = reinterpret_cast<const uint8_t *>(p);
    for (size_t i = 0; i < sizeof(T); ++i)
        if (raw[i] != 0xA5) return false;
    return true;
}

// BMX_OK or BMX_ERR_ARG, checked both ways
int compile(const std::string &expr, uint32_t flags = 0)
{
    std::unique_ptr<char[]> e(new char[expr.size() ? expr.size() : 1]); // exactly the expression
    std::memcpy(e.get(), expr.data(), expr.size());
    std::unique_ptr<bmx_regex> re(new bmx_regex);
    std::unique_ptr<bmx_regex_groups> gr(new bmx_regex_groups);
    std::memset(re.get(), 0xA5, sizeof(bmx_regex));
    std::memset(gr.get(), 0xA5, sizeof(bmx_regex_groups));
    const int rc = bmx_compile_regex_groups(e.get(), expr.size(), flags, re.get(), gr.get());
    if (rc != BMX_OK) {
        if (rc != BMX_ERR_ARG || !untouched(re.get()) || !untouched(gr.get())) fail("a refusal that touched its outputs", expr);
        if (g_last_error.rfind("bmx_compile_regex_groups: ", 0) != 0) fail("the error text's prefix", expr);
        return rc;
    }
    if (!bmx_regex_groups_valid(re.get(), gr.get())) fail("a compiled pair that is not valid", expr);
    std::string plain;
    for (size_t i = 0; i < expr.size(); ++i) { // every (?: as ( -- outside sets and escapes only, which the alphabet below keeps apart
        plain += expr[i];
        if (expr[i] == '(' && i + 2 < expr.size() && expr[i + 1] == '?' && expr[i + 2] == ':') i += 2;
    }
    std::unique_ptr<bmx_regex> ref(new bmx_regex);
    if (bmx_compile_regex(plain.data(), plain.size(), flags, ref.get()) != BMX_OK || std::memcmp(ref.get(), re.get(), sizeof(bmx_regex)) != 0)
        fail("an automaton that is not bmx_compile_regex's", expr);
    return rc;
}

int compile_template(const std::string &tmpl, int32_t n_groups)
{
    std::unique_ptr<char[]> t(new char[tmpl.size() ? tmpl.size() : 1]);
    std::memcpy(t.get(), tmpl.data(), tmpl.size());
    std::unique_ptr<bmx_template> out(new bmx_template);
    std::unique_ptr<uint8_t[]> lits(new uint8_t[tmpl.size() ? tmpl.size() : 1]); // room for len bytes, no more
    std::memset(out.get(), 0xA5, sizeof(bmx_template));
    const int rc = bmx_compile_template(t.get(), tmpl.size(), n_groups, out.get(), lits.get());
    if (rc != BMX_OK) {
        if (rc != BMX_ERR_ARG || !untouched(out.get())) fail("a refused template that touched its output", tmpl);
        return rc;
    }
    uint32_t at = 0;
    bool ok = out->n_refs >= 0 && out->n_refs <= BMX_MAX_TEMPLATE_REFS && out->lit_bytes <= tmpl.size();
    for (int32_t r = 0; ok && r <= out->n_refs; ++r) {
        ok = out->lit_off[r] == at && (r == out->n_refs || (out->ref[r] >= 0 && out->ref[r] <= n_groups));
        at += out->lit_len[r];
    }
    if (!ok || at != out->lit_bytes) fail("a template whose literals do not tile its bytes", tmpl);
    return rc;
}

} // namespace

int main()
{
    const char *fixed[] = {"(a|ab)(c|bcd)(d?)", "((a?)b){2}", "(a?|[bc])([bc]?)c", "((a)|b){2}", "(a)?b", "(a?)b", "()a", "(a|)b",
                           "(a?)?b", "(a|b?)c", "((a|b)(c)?){1,3}", "(?:(a)|(b)|(c)){2}", "([0-9]{4})-([0-9]{2})-([0-9]{2})",
                           "(ERROR|FATAL): ([0-9]{2,4})", "((((a))))", "(a)(?:)(b)", "x(|a|ab)(b?)y", "(?:a){64}", "(a){64}",
                           "(a)(b)(c)(d)(e)(f)(g)(h)(i)(j)(k)(l)(m)(n)(o)(p)"};
    for (const char *e : fixed)
        if (compile(e) != BMX_OK) fail("a fixed expression was refused", e);
    std::string wide;
    for (int i = 0; i < 16; ++i) wide += i % 2 ? "(a[bc]?c|.)" : "([ab](?:c|a)a?)";
    if (compile(wide) != BMX_OK) fail("the 64-position / 16-group expression was refused", wide);
    const char *refused[] = {"(a?){2}b", "((a)|b?){1,3}c", "(){3}a", "(?:(a)?){2}b", "(a|){2}b", "(?a)", "(?=a)b", "(?P<x>a)", "(?", "(",
                             "(a)(b)(c)(d)(e)(f)(g)(h)(i)(j)(k)(l)(m)(n)(o)(p)(q)", "a*", "(a", "a)", "(a?)", "", "?a", "(a){2,1}", "[a",
                             "(?:a){65}", "(a){65}", "(?:", "(?:)", "()"};
    for (const char *e : refused)
        if (compile(e) == BMX_OK) fail("a refused expression was accepted", e);
    if (bmx_compile_regex_groups("(a)", 3, 0, nullptr, nullptr) != BMX_ERR_ARG) fail("NULL outputs", "(a)");

    std::mt19937_64 rng(0x6709);
    const std::string alphabet = "ab.()()()|?{}12,:[]\\-^c";
    uint64_t accepted = 0;
    for (int it = 0; it < 200000; ++it) {
        std::string e;
        const int len = 1 + (int)(rng() % 24);
        for (int i = 0; i < len; ++i) e += alphabet[rng() % alphabet.size()];
        if (e.find("[") != std::string::npos || e.find("\\") != std::string::npos) { // (?: inside a set or behind \ is no group
            std::unique_ptr<bmx_regex> re(new bmx_regex);
            std::unique_ptr<bmx_regex_groups> gr(new bmx_regex_groups);
            std::unique_ptr<char[]> buf(new char[e.size()]);
            std::memcpy(buf.get(), e.data(), e.size());
            if (bmx_compile_regex_groups(buf.get(), e.size(), (uint32_t)(rng() % 4), re.get(), gr.get()) == BMX_OK) {
                ++accepted;
                if (!bmx_regex_groups_valid(re.get(), gr.get())) fail("a compiled pair that is not valid", e);
            }
            continue;
        }
        accepted += compile(e, (uint32_t)(rng() % 4)) == BMX_OK;
    }

    const struct { const char *t; int32_t g; int rc; } templates[] = {
        {"", 0, BMX_OK}, {"plain", 0, BMX_OK}, {"\\1", 1, BMX_OK}, {"\\3.\\2.\\1", 3, BMX_OK}, {"\\1\\2", 2, BMX_OK}, {"a\\\\b", 0, BMX_OK},
        {"<\\g<0>>", 0, BMX_OK}, {"\\g<16>\\g<1>0", 16, BMX_OK}, {"\\g<01>", 1, BMX_OK}, {"\\9", 9, BMX_OK},
        {"\\", 1, BMX_ERR_ARG}, {"a\\", 1, BMX_ERR_ARG}, {"\\0", 1, BMX_ERR_ARG}, {"\\n", 1, BMX_ERR_ARG}, {"\\2", 1, BMX_ERR_ARG},
        {"\\g<2>", 1, BMX_ERR_ARG}, {"\\g<17>", 16, BMX_ERR_ARG}, {"\\g<1", 1, BMX_ERR_ARG}, {"\\g<", 1, BMX_ERR_ARG}, {"\\g", 1, BMX_ERR_ARG},
        {"\\g<>", 1, BMX_ERR_ARG}, {"\\g<a>", 1, BMX_ERR_ARG}, {"\\g<123>", 16, BMX_ERR_ARG}, {"\\10", 16, BMX_ERR_ARG}, {"x", -1, BMX_ERR_ARG},
        {"x", 17, BMX_ERR_ARG}};
    for (const auto &c : templates)
        if (compile_template(c.t, c.g) != c.rc) fail("a template's return code", c.t);
    std::string refs32, refs33;
    for (int i = 0; i < 33; ++i) (i < 32 ? refs32 : refs33) += "\\1";
    refs33 = refs32 + refs33;
    if (compile_template(refs32, 1) != BMX_OK || compile_template(refs33, 1) != BMX_ERR_ARG) fail("32 and 33 references", "\\1 ...");
    if (compile_template(std::string(BMX_MAX_REPLACEMENT, 'x'), 0) != BMX_OK || compile_template(std::string(BMX_MAX_REPLACEMENT + 1, 'x'), 0) != BMX_ERR_ARG)
        fail("the longest template", "x ...");
    const std::string talpha = "ab\\\\\\g<>0129";
    uint64_t taccepted = 0;
    for (int it = 0; it < 200000; ++it) {
        std::string t;
        const int len = (int)(rng() % 20);
        for (int i = 0; i < len; ++i) t += talpha[rng() % talpha.size()];
        taccepted += compile_template(t, (int32_t)(rng() % 17)) == BMX_OK;
    }
    std::printf("regex_groups_compile_check: %llu random expressions and %llu random templates accepted, %d failure(s)\n",
                (unsigned long long)accepted, (unsigned long long)taccepted, failures);
    return failures ? 1 : 0;
}
