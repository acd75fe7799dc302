// bmx_classes_compile.cpp -- bmx_compile_classes (include/bmx.h): a fixed-length class expression to one 256-bit set
// per position (pure C++, no GPU).  No counterpart in the reference.
//
// Grammar: one element of the expression is one class.
//   .            every byte value
//   [...]        a set: items and inclusive ranges x-y (x <= y); a leading ^ negates; ] directly after [ or [^ is a
//                literal; a - that is not between two items (first, or right before the closing ]) is a literal
//   \xHH         the byte with that hexadecimal value (inside sets too)
//   \c           the byte c as a literal (inside sets too)
//   any other    itself
// No repetition, alternation or anchors.  BMX_CLASS_ICASE gives every ASCII letter of a class its other case, before a
// set's negation.  BMX_CLASS_IUPAC reads the upper-case letters R Y S W K M B D H V N outside sets and escapes as
// their nucleotide sets over ACGT.
#include "bmx.h"

#include <cstring>

namespace {

struct ByteSet {
    uint8_t bits[BMX_CLASS_BYTES];
    void clear() { std::memset(bits, 0, sizeof bits); }
    void add(unsigned b) { bits[b >> 3] |= (uint8_t)(1u << (b & 7)); }
    bool has(unsigned b) const { return (bits[b >> 3] >> (b & 7)) & 1u; }
    void fold_case()
    {
        for (unsigned c = 'a'; c <= 'z'; ++c) {
            const unsigned u = c - 'a' + 'A';
            if (has(c)) add(u);
            else if (has(u)) add(c);
        }
    }
    void negate()
    {
        for (auto &b : bits) b = (uint8_t)~b;
    }
};

int hex_value(unsigned c)
{
    if (c >= '0' && c <= '9') return (int)(c - '0');
    if (c >= 'a' && c <= 'f') return (int)(c - 'a' + 10);
    if (c >= 'A' && c <= 'F') return (int)(c - 'A' + 10);
    return -1;
}

// The escape whose backslash is at e[at - 1]: the byte it stands for, or -1 (dangling, bad hex).  Advances at.
int escape(const uint8_t *e, uint64_t len, uint64_t &at)
{
    if (at >= len) return -1;
    const unsigned c = e[at++];
    if (c != 'x') return (int)c;
    if (len - at < 2) return -1;
    const int h = hex_value(e[at]), l = hex_value(e[at + 1]);
    if (h < 0 || l < 0) return -1;
    at += 2;
    return 16 * h + l;
}

const char *iupac(unsigned c)
{
    switch (c) {
    case 'R': return "AG";
    case 'Y': return "CT";
    case 'S': return "CG";
    case 'W': return "AT";
    case 'K': return "GT";
    case 'M': return "AC";
    case 'B': return "CGT";
    case 'D': return "AGT";
    case 'H': return "ACT";
    case 'V': return "ACG";
    case 'N': return "ACGT";
    default: return nullptr;
    }
}

} // namespace

extern "C" int bmx_compile_classes(const char *expr, uint64_t expr_len, uint32_t flags, uint8_t *classes, int32_t *m_out)
{
    if (!expr || !classes || !m_out) return BMX_ERR_ARG;
    const uint8_t *e = reinterpret_cast<const uint8_t *>(expr);
    static_assert(sizeof(ByteSet) == BMX_CLASS_BYTES, "one class is 32 bytes");
    ByteSet sets[BMX_MAX_CLASS_PATTERN];
    int32_t m = 0;
    uint64_t at = 0;
    while (at < expr_len) {
        if (m == BMX_MAX_CLASS_PATTERN) return BMX_ERR_ARG;
        ByteSet &s = sets[m];
        s.clear();
        bool negated = false;
        const unsigned c = e[at++];
        if (c == '.') {
            s.negate();
        } else if (c == '\\') {
            const int b = escape(e, expr_len, at);
            if (b < 0) return BMX_ERR_ARG;
            s.add((unsigned)b);
        } else if (c == '[') {
            if (at < expr_len && e[at] == '^') negated = true, ++at;
            bool first = true, closed = false;
            while (at < expr_len) {
                int x = e[at++];
                if (x == ']' && !first) {
                    closed = true;
                    break;
                }
                first = false;
                if (x == '\\' && (x = escape(e, expr_len, at)) < 0) return BMX_ERR_ARG;
                int y = x;
                if (at + 1 < expr_len && e[at] == '-' && e[at + 1] != ']') { // a range
                    ++at;
                    y = e[at++];
                    if (y == '\\' && (y = escape(e, expr_len, at)) < 0) return BMX_ERR_ARG;
                    if (y < x) return BMX_ERR_ARG;
                }
                for (int b = x; b <= y; ++b) s.add((unsigned)b);
            }
            if (!closed) return BMX_ERR_ARG;
        } else {
            const char *bases = (flags & BMX_CLASS_IUPAC) ? iupac(c) : nullptr;
            if (bases)
                for (; *bases; ++bases) s.add((unsigned char)*bases);
            else
                s.add(c);
        }
        if (flags & BMX_CLASS_ICASE) s.fold_case();
        if (negated) s.negate();
        ++m;
    }
    if (m == 0) return BMX_ERR_ARG;
    std::memcpy(classes, sets, (size_t)m * BMX_CLASS_BYTES);
    *m_out = m;
    return BMX_OK;
}
