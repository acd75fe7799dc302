// bmx_regex_compile.cpp -- bmx_compile_regex and bmx_compile_regex_star (include/bmx.h): a regular expression to its
// Glushkov (position) automaton, struct bmx_regex (pure C++, no GPU).  No counterpart in the reference.  One parser
// behind a switch (Compiler::star): the first entry takes the star-free expressions, the second also * + {a,}.
//
//     alt    := concat ('|' concat)*        an empty alternative is allowed: (a|) is a?
//     concat := repeat*
//     repeat := atom quant?                 quant := '?' | '{a}' | '{a,b}'   decimal, 0 <= a <= b, b >= 1
//                                           (star: also '*' | '+' | '{a,}')
//     atom   := element | '(' alt ')'
// An element is exactly one element of bmx_compile_classes; this file only finds where it ends and hands it over, as
// bmx_gaps_compile.cpp does, so the grammars cannot drift apart.  The expression is first parsed into a tree (every
// syntax error is found there, once), then the tree is expanded: X{a,b} is a copies of X followed by b - a optional
// ones, positions are numbered left to right as they are made, and first, last, follow and nullability come from the
// standard recursion (Glushkov 1961; Berry and Sethi 1986).  follow[] only ever points upward: a concatenation links the
// last positions of what stands left to the first positions of what stands right of it, and nothing else makes a link.
// A subtree without an element is the empty string whatever its counts say, so it is never expanded more than once and
// every other expansion step makes a position: the work is bounded by the 64 positions, not by the counts.
// With the switch: X+ links every last position of X to the first positions of X (the one rule that makes follow[] point
// downward or at itself), X* is (X+)? and X{a,} is a - 1 copies of X followed by X+ (a == 0: X*).
#include "bmx.h"

#include <cstdio>
#include <cstring>
#include <vector>

#include "bmx_regex_sets.h"

void bmx_internal_set_error(const char *text); // bmx_shim.hip: the text bmx_last_error() returns on this thread

namespace {

constexpr uint64_t NPOS = ~0ull;
constexpr int MAX_DEPTH = 32;
constexpr int UNBOUNDED = -1;

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

enum Kind { ELEM, CAT, ALT, REP };
struct Node {
    Kind kind;
    int a = 1, b = 1;          // REP (b == UNBOUNDED: no upper count)
    bool has_element = false;  // some element stands below it
    std::vector<int> kids;     // CAT, ALT: any number; REP: one
    uint8_t cls[BMX_CLASS_BYTES]; // ELEM
};

struct Frag {
    bool nullable;
    uint64_t first, last;
};

struct Compiler {
    const uint8_t *e;
    uint64_t len;
    uint32_t flags;
    bool star = false; // the grammar of bmx_compile_regex_star
    uint64_t at = 0;
    const char *why = nullptr;
    std::vector<Node> nodes;
    bmx_regex re;

    bool fail(const char *text)
    {
        if (!why) why = text;
        return false;
    }
    int make(Kind k)
    {
        nodes.emplace_back();
        nodes.back().kind = k;
        return (int)nodes.size() - 1;
    }

    // the counts behind '{' (already read): n or a,b with 0 <= a <= b and b >= 1
    bool counts(int &a, int &b)
    {
        if (!number(e, len, at, a)) return fail("a malformed {...}");
        b = a;
        if (at < len && e[at] == ',') {
            ++at;
            if (at < len && e[at] == '}') {
                if (!star) return fail("{a,}: unbounded repetition is out of scope");
                ++at;
                b = UNBOUNDED;
                return true;
            }
            if (!number(e, len, at, b)) return fail("a malformed {...}");
        }
        if (at >= len || e[at] != '}') return fail("a malformed or unterminated {...}");
        ++at;
        if (b < 1 || a > b) return fail("{a,b} needs 0 <= a <= b and b >= 1");
        return true;
    }

    bool parse_repeat(int depth, int &out)
    {
        const unsigned c = e[at];
        if (!star && (c == '*' || c == '+')) return fail("* and +: unbounded repetition is out of scope");
        if (c == '?' || c == '{' || c == '*' || c == '+') return fail("a quantifier with nothing in front of it");
        int atom;
        if (c == '(') {
            if (depth + 1 > MAX_DEPTH) return fail("groups nested deeper than 32");
            ++at;
            if (!parse_alt(depth + 1, atom)) return false;
            if (at >= len || e[at] != ')') return fail("an unbalanced (");
            ++at;
        } else {
            const uint64_t end = element_end(e, len, at);
            uint8_t cls[BMX_MAX_CLASS_PATTERN * BMX_CLASS_BYTES];
            int32_t m1 = 0;
            if (end == NPOS || bmx_compile_classes(reinterpret_cast<const char *>(e + at), end - at, flags, cls, &m1) != BMX_OK || m1 != 1)
                return fail("a bad element (an unterminated set, a reversed range, a dangling \\ or bad hex)");
            atom = make(ELEM);
            nodes[atom].has_element = true;
            std::memcpy(nodes[atom].cls, cls, BMX_CLASS_BYTES);
            at = end;
        }
        out = atom;
        if (at >= len) return true;
        int a = 1, b = 1;
        if (e[at] == '?') {
            a = 0;
            ++at;
        } else if (e[at] == '{') {
            ++at;
            if (!counts(a, b)) return false;
        } else if (e[at] == '*' || e[at] == '+') {
            if (!star) return fail("* and +: unbounded repetition is out of scope");
            a = e[at] == '*' ? 0 : 1;
            b = UNBOUNDED;
            ++at;
        } else {
            return true;
        }
        if (at < len && (e[at] == '?' || e[at] == '{')) return fail("a quantifier right after another quantifier");
        if (at < len && (e[at] == '*' || e[at] == '+'))
            return fail(star ? "a quantifier right after another quantifier" : "* and +: unbounded repetition is out of scope");
        out = make(REP);
        nodes[out].a = a, nodes[out].b = b;
        nodes[out].has_element = nodes[atom].has_element;
        nodes[out].kids.push_back(atom);
        return true;
    }

    bool parse_alt(int depth, int &out)
    {
        const int alt = make(ALT);
        for (;;) {
            const int cat = make(CAT);
            while (at < len && e[at] != '|' && e[at] != ')') {
                int r;
                if (!parse_repeat(depth, r)) return false;
                nodes[cat].kids.push_back(r);
                nodes[cat].has_element |= nodes[r].has_element;
            }
            nodes[alt].kids.push_back(cat);
            nodes[alt].has_element |= nodes[cat].has_element;
            if (at >= len || e[at] != '|') break;
            ++at;
        }
        out = alt;
        return true;
    }

    static Frag cat(Frag f, const Frag &g, uint64_t *follow)
    {
        for (uint64_t l = f.last; l != 0; l &= l - 1) follow[__builtin_ctzll(l)] |= g.first;
        Frag r;
        r.first = f.first | (f.nullable ? g.first : 0);
        r.last = g.last | (g.nullable ? f.last : 0);
        r.nullable = f.nullable && g.nullable;
        return r;
    }

    bool expand(int id, Frag &out)
    {
        const Frag empty = {true, 0, 0};
        out = empty;
        if (!nodes[id].has_element) return true; // the empty string, whatever its counts
        switch (nodes[id].kind) {
        case ELEM: {
            if (re.m >= BMX_MAX_REGEX_POSITIONS) return fail("more than 64 positions after expansion");
            std::memcpy(re.classes + (size_t)re.m * BMX_CLASS_BYTES, nodes[id].cls, BMX_CLASS_BYTES);
            out.nullable = false;
            out.first = out.last = 1ull << re.m;
            ++re.m;
            return true;
        }
        case CAT:
            for (size_t i = 0; i < nodes[id].kids.size(); ++i) {
                Frag g;
                if (!expand(nodes[id].kids[i], g)) return false;
                out = cat(out, g, re.follow);
            }
            return true;
        case ALT: {
            Frag r = {false, 0, 0};
            for (size_t i = 0; i < nodes[id].kids.size(); ++i) {
                Frag g;
                if (!expand(nodes[id].kids[i], g)) return false;
                r.nullable |= g.nullable, r.first |= g.first, r.last |= g.last;
            }
            out = r;
            return true;
        }
        case REP:
            if (nodes[id].b == UNBOUNDED) { // X{a,}: max(a, 1) copies, the last one looped; a == 0 makes that one optional
                const int copies = nodes[id].a > 1 ? nodes[id].a : 1;
                for (int i = 0; i < copies; ++i) {
                    Frag g;
                    if (!expand(nodes[id].kids[0], g)) return false;
                    if (i == copies - 1) {
                        for (uint64_t l = g.last; l != 0; l &= l - 1) re.follow[__builtin_ctzll(l)] |= g.first;
                        if (nodes[id].a == 0) g.nullable = true;
                    }
                    out = cat(out, g, re.follow);
                }
                return true;
            }
            for (int i = 0; i < nodes[id].b; ++i) { // (every copy makes a position, so 65 copies at the most)
                Frag g;
                if (!expand(nodes[id].kids[0], g)) return false;
                if (i >= nodes[id].a) g.nullable = true;
                out = cat(out, g, re.follow);
            }
            return true;
        }
        return false;
    }
};

} // namespace

namespace {

int compile(const char *where, bool star, const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out)
{
    char text[160];
    if (!expr || !out) {
        snprintf(text, sizeof text, "%s: a NULL argument", where);
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    if (flags & ~(BMX_CLASS_ICASE | BMX_CLASS_IUPAC)) {
        snprintf(text, sizeof text, "%s: an unknown flag bit", where);
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    Compiler c;
    c.e = reinterpret_cast<const uint8_t *>(expr);
    c.len = expr_len;
    c.flags = flags;
    c.star = star;
    std::memset(&c.re, 0, sizeof c.re);
    int root = 0;
    Frag f = {true, 0, 0};
    bool ok = c.parse_alt(0, root);
    if (ok && c.at < c.len) ok = c.fail("an unbalanced )");
    if (ok) ok = c.expand(root, f);
    if (ok && c.re.m == 0) ok = c.fail("zero positions");
    if (ok && f.nullable) ok = c.fail("the expression matches the empty string");
    if (!ok) {
        snprintf(text, sizeof text, "%s: %s", where, c.why ? c.why : "a bad expression");
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    c.re.first = f.first;
    c.re.last = f.last;
    if (star) bmx_regex_star_lengths(c.re.m, c.re.first, c.re.last, c.re.follow, &c.re.min_len, &c.re.max_len, nullptr);
    else bmx_regex_lengths(c.re.m, c.re.first, c.re.last, c.re.follow, &c.re.min_len, &c.re.max_len);
    *out = c.re;
    return BMX_OK;
}

} // namespace

extern "C" int bmx_compile_regex(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out)
{
    return compile("bmx_compile_regex", false, expr, expr_len, flags, out);
}

extern "C" int bmx_compile_regex_star(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out)
{
    return compile("bmx_compile_regex_star", true, expr, expr_len, flags, out);
}
