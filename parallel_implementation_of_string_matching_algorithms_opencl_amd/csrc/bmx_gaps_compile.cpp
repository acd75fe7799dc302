// bmx_gaps_compile.cpp -- bmx_compile_gaps (include/bmx.h): a gapped pattern expression to one 256-bit set per position
// and the mask of the optional positions (pure C++, no GPU).  No counterpart in the reference.
//
// Default syntax: the elements of bmx_compile_classes (. [...] [^...] \xHH \c, literals; BMX_CLASS_ICASE, BMX_CLASS_IUPAC),
// each optionally followed by ONE quantifier ? {a} {a,b} (decimal, 0 <= a <= b, b >= 1).  An element with {a,b} becomes a
// mandatory copies followed by b - a optional ones.  This file only finds where an element ends and reads the quantifier:
// the element itself goes through bmx_compile_classes, so the two grammars cannot drift apart.
// BMX_GAPS_PROSITE: elements separated by -, x = any byte, [ABC] a set, {ABC} a negated set, any other byte itself,
// (n) or (a,b) behind an element its repetition, one trailing . ignored.  A set is handed to bmx_compile_classes as a
// set of \xHH items, which also gives it BMX_CLASS_ICASE.
#include "bmx.h"

#include <cstring>
#include <string>

namespace {

constexpr uint64_t NPOS = ~0ull;

// Behind a backslash at e[p - 1]: one past the escape, or NPOS where the expression ends first.
uint64_t skip_escape(const uint8_t *e, uint64_t len, uint64_t p)
{
    if (p >= len) return NPOS;
    if (e[p] != 'x') return p + 1;
    return len - (p + 1) < 2 ? NPOS : p + 3;
}

// One past the element that begins at e[at] (at < len), by the rules of bmx_compile_classes; NPOS where it has no end.
uint64_t element_end(const uint8_t *e, uint64_t len, uint64_t at)
{
    const unsigned c = e[at];
    if (c == '\\') return skip_escape(e, len, at + 1);
    if (c != '[') return at + 1;
    uint64_t p = at + 1;
    if (p < len && e[p] == '^') ++p;
    bool first = true;
    while (p < len) {
        unsigned x = e[p++];
        if (x == ']' && !first) return p;
        first = false;
        if (x == '\\' && (p = skip_escape(e, len, p)) == NPOS) return NPOS;
        if (p + 1 < len && e[p] == '-' && e[p + 1] != ']') { // a range
            ++p;
            x = e[p++];
            if (x == '\\' && (p = skip_escape(e, len, p)) == NPOS) return NPOS;
        }
    }
    return NPOS;
}

// A decimal number at e[at]: at least one digit, values above 999 saturate (any such count is out of range anyway).
bool number(const uint8_t *e, uint64_t len, uint64_t &at, int &value)
{
    if (at >= len || e[at] < '0' || e[at] > '9') return false;
    value = 0;
    for (; at < len && e[at] >= '0' && e[at] <= '9'; ++at) value = value > 99 ? 999 : 10 * value + (int)(e[at] - '0');
    return true;
}

// The counts between `open` (already read) and `close`: n or a,b with 0 <= a <= b and b >= 1.
bool counts(const uint8_t *e, uint64_t len, uint64_t &at, unsigned close, int &a, int &b)
{
    if (!number(e, len, at, a)) return false;
    b = a;
    if (at < len && e[at] == ',') {
        ++at;
        if (!number(e, len, at, b)) return false;
    }
    if (at >= len || e[at] != close) return false;
    ++at;
    return b >= 1 && a <= b;
}

struct Pattern {
    uint8_t classes[BMX_MAX_GAPS_PATTERN * BMX_CLASS_BYTES];
    uint64_t optional = 0;
    int32_t m = 0;

    // a mandatory copies of cls, then b - a optional ones
    bool add(const uint8_t *cls, int a, int b)
    {
        if (b > BMX_MAX_GAPS_PATTERN - m) return false;
        for (int i = 0; i < b; ++i, ++m) {
            std::memcpy(classes + (size_t)m * BMX_CLASS_BYTES, cls, BMX_CLASS_BYTES);
            if (i >= a) optional |= 1ull << m;
        }
        return true;
    }
};

// one element of the class grammar -> its class
bool one_class(const uint8_t *e, uint64_t len, uint32_t flags, uint8_t *cls /* BMX_MAX_CLASS_PATTERN classes */)
{
    int32_t m1 = 0;
    return bmx_compile_classes(reinterpret_cast<const char *>(e), len, flags, cls, &m1) == BMX_OK && m1 == 1;
}

bool compile_default(const uint8_t *e, uint64_t len, uint32_t flags, Pattern &out)
{
    uint8_t cls[BMX_MAX_CLASS_PATTERN * BMX_CLASS_BYTES];
    uint64_t at = 0;
    while (at < len) {
        const unsigned c = e[at];
        if (c == '?' || c == '{' || c == '*' || c == '+') return false; // no element in front, or unbounded repetition
        const uint64_t end = element_end(e, len, at);
        if (end == NPOS || !one_class(e + at, end - at, flags, cls)) return false;
        at = end;
        int a = 1, b = 1;
        if (at < len && e[at] == '?') {
            a = 0;
            ++at;
        } else if (at < len && e[at] == '{') {
            ++at;
            if (!counts(e, len, at, '}', a, b)) return false;
        }
        if (!out.add(cls, a, b)) return false;
    }
    return true;
}

bool compile_prosite(const uint8_t *e, uint64_t len, uint32_t flags, Pattern &out)
{
    uint8_t cls[BMX_MAX_CLASS_PATTERN * BMX_CLASS_BYTES];
    if (len > 0 && e[len - 1] == '.') --len;
    uint64_t at = 0;
    static const char hex[] = "0123456789abcdef";
    for (;;) {
        if (at >= len) return false; // an element is due: an empty pattern, or one that ends in -
        const unsigned c = e[at++];
        std::string expr;
        if (c == 'x') {
            expr = ".";
        } else if (c == '[' || c == '{') {
            const unsigned close = c == '[' ? ']' : '}';
            expr = c == '[' ? "[" : "[^";
            uint64_t items = 0;
            for (; at < len && e[at] != close; ++at, ++items) {
                if (e[at] == '<' || e[at] == '>') return false; // anchors are out of scope
                expr += {'\\', 'x', hex[e[at] >> 4], hex[e[at] & 15]};
            }
            if (at >= len || items == 0) return false;
            ++at;
            expr += ']';
        } else if (std::strchr("-]}()<>.,", (int)c) != nullptr && c != 0) {
            return false;
        } else {
            expr = {'\\', 'x', hex[c >> 4], hex[c & 15]};
        }
        if (!one_class(reinterpret_cast<const uint8_t *>(expr.data()), expr.size(), flags, cls)) return false;
        int a = 1, b = 1;
        if (at < len && e[at] == '(') {
            ++at;
            if (!counts(e, len, at, ')', a, b)) return false;
        }
        if (!out.add(cls, a, b)) return false;
        if (at == len) return true;
        if (e[at++] != '-') return false;
    }
}

} // namespace

extern "C" int bmx_compile_gaps(const char *expr, uint64_t expr_len, uint32_t flags, uint8_t *classes, uint64_t *optional,
                                int32_t *m_out)
{
    if (!expr || !classes || !optional || !m_out) return BMX_ERR_ARG;
    if (flags & ~(BMX_CLASS_ICASE | BMX_CLASS_IUPAC | BMX_GAPS_PROSITE)) return BMX_ERR_ARG; // an unknown flag bit
    if ((flags & BMX_GAPS_PROSITE) && (flags & BMX_CLASS_IUPAC)) return BMX_ERR_ARG;
    const uint8_t *e = reinterpret_cast<const uint8_t *>(expr);
    Pattern p;
    const uint32_t class_flags = flags & (BMX_CLASS_ICASE | BMX_CLASS_IUPAC);
    const bool ok = (flags & BMX_GAPS_PROSITE) ? compile_prosite(e, expr_len, class_flags, p) : compile_default(e, expr_len, class_flags, p);
    if (!ok || p.m == 0) return BMX_ERR_ARG;
    const uint64_t all = p.m == 64 ? ~0ull : (1ull << p.m) - 1;
    if (p.optional == all) return BMX_ERR_ARG; // it would match the empty string
    std::memcpy(classes, p.classes, (size_t)p.m * BMX_CLASS_BYTES);
    *optional = p.optional;
    *m_out = p.m;
    return BMX_OK;
}
