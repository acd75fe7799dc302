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
// every other expansion step makes a position: the work is bounded by the entry's 64 or 128 positions, not by the counts.
// With the switch: X+ links every last position of X to the first positions of X (the one rule that makes follow[] point
// downward or at itself), X* is (X+)? and X{a,} is a - 1 copies of X followed by X+ (a == 0: X*).
// bmx_compile_regex_anchored is the star-free grammar behind a second switch (Compiler::anchored): ^ $ \b \B \< \> parse
// as zero-width atoms, the expansion carries a relation between the byte before and the byte after a boundary where the
// plain one carries a bit (aexpand), and resolve() turns the relations into struct bmx_regex_anchors, splitting a position
// whose condition depends on its own byte and deciding every assertion between two positions from their classes
// (DESIGN.md s32).  The two plain entries never see an assertion: without the switch ^ and $ are literals.
// bmx_compile_regex_long is the star-free grammar with the limit at 128 positions (Compiler::limit): the expansion always
// works on sets of 128 bits (Set, bmx_regex_sets.h) and each entry stores them into its own struct at the end, so for an
// expression of at most 64 positions the long entry's low words are the short entry's sets.
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

// ---- assertions (bmx_compile_regex_anchored) ----
// Every assertion is a relation between the byte before and the byte after a boundary, and every one of them sees a byte
// only as one of three categories: the line break, a word byte (W = [A-Za-z0-9_]), any other.  A relation is therefore a set
// of (category before, category after) pairs: bit 3 * before + after of nine.  Relations at one boundary intersect,
// alternatives unite, and whether a relation holds between two classes is a question about the categories they touch.
enum Cat { CAT_NL = 0, CAT_WORD = 1, CAT_OTHER = 2 };
constexpr int REL_FULL = 0x1FF;
constexpr int REL_BOL = 0x007;      // before is the line break
constexpr int REL_EOL = 0x049;      // after is the line break
constexpr int REL_WB = 0x0AA;       // exactly one side is a word byte
constexpr int REL_NWB = REL_FULL & ~REL_WB;
constexpr int REL_WSTART = 0x082;   // before is no word byte, after is one
constexpr int REL_WEND = 0x028;     // before is a word byte, after is none
constexpr int REL_BEFORE_NOT_WORD = 0x1C7, REL_AFTER_NOT_WORD = 0x16D;

int cat_of(unsigned c)
{
    if (c == '\n') return CAT_NL;
    return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_' ? CAT_WORD : CAT_OTHER;
}

// The relation of the assertion at e[at], 0 where none stands there.  ^ and $ take one byte, the others two.
int assertion_at(const uint8_t *e, uint64_t len, uint64_t at)
{
    if (e[at] == '^') return REL_BOL;
    if (e[at] == '$') return REL_EOL;
    if (e[at] != '\\' || at + 1 >= len) return 0;
    switch (e[at + 1]) {
    case 'b': return REL_WB;
    case 'B': return REL_NWB;
    case '<': return REL_WSTART;
    case '>': return REL_WEND;
    }
    return 0;
}

// What an expression with assertions expands to: as Frag, with a relation where Frag has a bit.  eps: the relation under
// which it matches the empty string (0 where it cannot); nullable: whether it does once assertions are ignored.
// first[p] relates the byte before the match to position p's byte, last[p] position p's byte to the byte after.
struct AFrag {
    bool nullable;
    uint16_t eps;
    uint16_t first[BMX_MAX_REGEX_POSITIONS], last[BMX_MAX_REGEX_POSITIONS];
};

enum Kind { ELEM, CAT, ALT, REP, ASSERT, GROUP };
struct Node {
    Kind kind;
    int a = 1, b = 1;          // REP (b == UNBOUNDED: no upper count); ASSERT: a is its relation (below); GROUP: a is its number
    bool has_element = false;  // some element stands below it
    bool has_group = false;    // a capturing group stands below it, or it is one (bmx_compile_regex_groups)
    std::vector<int> kids;     // CAT, ALT: any number; REP, GROUP: one
    uint8_t cls[BMX_CLASS_BYTES]; // ELEM
};

// The compiler's own automaton: sets of 128 bits whatever the entry's limit, turned into the entry's struct at the end.
typedef bmx_set128 Set;
struct Automaton {
    int32_t m;
    Set follow[BMX_MAX_REGEX_LONG_POSITIONS];
    uint8_t classes[BMX_MAX_REGEX_LONG_POSITIONS * BMX_CLASS_BYTES];
};

struct Frag {
    bool nullable;
    Set first, last;
};

struct Compiler {
    const uint8_t *e;
    uint64_t len;
    uint32_t flags;
    bool star = false; // the grammar of bmx_compile_regex_star
    bool anchored = false; // the grammar of bmx_compile_regex_anchored: ^ $ \b \B \< \> are zero-width atoms
    bool groups = false; // the grammar of bmx_compile_regex_groups: ( captures, (?: does not
    int n_groups = 0;
    uint64_t at = 0;
    const char *why = nullptr;
    bool has_assertion = false;
    std::vector<Node> nodes;
    int limit = BMX_MAX_REGEX_POSITIONS; // positions after expansion (bmx_compile_regex_long: 128)
    Automaton re;

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
        if (anchored) {
            const int rel = assertion_at(e, len, at);
            if (rel != 0) {
                at += c == '\\' ? 2 : 1;
                if (at < len && (e[at] == '?' || e[at] == '{' || e[at] == '*' || e[at] == '+')) return fail("a quantifier on an assertion");
                out = make(ASSERT);
                nodes[out].a = rel;
                has_assertion = true;
                return true;
            }
        }
        int atom;
        if (c == '(') {
            if (depth + 1 > MAX_DEPTH) return fail("groups nested deeper than 32");
            ++at;
            int number = 0; // of a capturing group, by its '(' (0: it does not capture)
            if (groups) {
                if (at < len && e[at] == '?') {
                    if (at + 1 >= len || e[at + 1] != ':') return fail("(? followed by anything but : (only (?: is known)");
                    at += 2;
                } else {
                    if (n_groups == BMX_MAX_REGEX_GROUPS) return fail("more than 16 capturing groups");
                    number = ++n_groups;
                }
            }
            if (!parse_alt(depth + 1, atom)) return false;
            if (at >= len || e[at] != ')') return fail("an unbalanced (");
            ++at;
            if (number) {
                const int inner = atom;
                atom = make(GROUP);
                nodes[atom].a = number;
                nodes[atom].has_element = nodes[inner].has_element;
                nodes[atom].has_group = true;
                nodes[atom].kids.push_back(inner);
            }
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
        nodes[out].has_group = nodes[atom].has_group;
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
                nodes[cat].has_group |= nodes[r].has_group;
            }
            nodes[alt].kids.push_back(cat);
            nodes[alt].has_element |= nodes[cat].has_element;
            nodes[alt].has_group |= nodes[cat].has_group;
            if (at >= len || e[at] != '|') break;
            ++at;
        }
        out = alt;
        return true;
    }

    static Frag cat(Frag f, const Frag &g, Set *follow)
    {
        for (Set l = f.last; l != 0; l &= l - 1) follow[bmx_set_low_bit(l)] |= g.first;
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
        case ASSERT: return true; // (has no element: not reached; the anchored grammar expands with aexpand)
        case GROUP: return expand(nodes[id].kids[0], out); // (the automaton does not see it: bmx_compile_regex_groups' tables do)
        case ELEM: {
            if (re.m >= limit)
                return fail(limit == BMX_MAX_REGEX_POSITIONS ? "more than 64 positions after expansion" : "more than 128 positions after expansion");
            std::memcpy(re.classes + (size_t)re.m * BMX_CLASS_BYTES, nodes[id].cls, BMX_CLASS_BYTES);
            out.nullable = false;
            out.first = out.last = (Set)1 << re.m;
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
                        for (Set l = g.last; l != 0; l &= l - 1) re.follow[bmx_set_low_bit(l)] |= g.first;
                        if (nodes[id].a == 0) g.nullable = true;
                    }
                    out = cat(out, g, re.follow);
                }
                return true;
            }
            for (int i = 0; i < nodes[id].b; ++i) { // (every copy makes a position, so limit + 1 copies at the most)
                Frag g;
                if (!expand(nodes[id].kids[0], g)) return false;
                if (i >= nodes[id].a) g.nullable = true;
                out = cat(out, g, re.follow);
            }
            return true;
        }
        return false;
    }

    // ---- the same expansion with relations (anchored) ----
    uint16_t edge[BMX_MAX_REGEX_POSITIONS][BMX_MAX_REGEX_POSITIONS]; // [l][r]: the relation under which r may follow l (0: never)

    AFrag acat(const AFrag &f, const AFrag &g)
    {
        AFrag r;
        for (int l = 0; l < re.m; ++l) {
            if (!f.last[l]) continue;
            for (int p = 0; p < re.m; ++p) edge[l][p] |= f.last[l] & g.first[p]; // both speak of the same boundary
        }
        for (int p = 0; p < BMX_MAX_REGEX_POSITIONS; ++p) {
            r.first[p] = f.first[p] | (g.first[p] & f.eps);
            r.last[p] = g.last[p] | (f.last[p] & g.eps);
        }
        r.eps = f.eps & g.eps;
        r.nullable = f.nullable && g.nullable;
        return r;
    }

    bool aexpand(int id, AFrag &out)
    {
        std::memset(&out, 0, sizeof out);
        out.nullable = true, out.eps = REL_FULL;
        switch (nodes[id].kind) {
        case GROUP: return false; // (bmx_compile_regex_groups only, which is not anchored)
        case ASSERT:
            out.eps = (uint16_t)nodes[id].a;
            return true;
        case ELEM:
            if (re.m >= BMX_MAX_REGEX_POSITIONS) return fail("more than 64 positions after expansion");
            std::memcpy(re.classes + (size_t)re.m * BMX_CLASS_BYTES, nodes[id].cls, BMX_CLASS_BYTES);
            out.nullable = false, out.eps = 0;
            out.first[re.m] = out.last[re.m] = REL_FULL;
            ++re.m;
            return true;
        case CAT:
            for (size_t i = 0; i < nodes[id].kids.size(); ++i) {
                AFrag g;
                if (!aexpand(nodes[id].kids[i], g)) return false;
                out = acat(out, g);
            }
            return true;
        case ALT: {
            AFrag r;
            std::memset(&r, 0, sizeof r);
            for (size_t i = 0; i < nodes[id].kids.size(); ++i) {
                AFrag g;
                if (!aexpand(nodes[id].kids[i], g)) return false;
                r.nullable |= g.nullable, r.eps |= g.eps;
                for (int p = 0; p < BMX_MAX_REGEX_POSITIONS; ++p) r.first[p] |= g.first[p], r.last[p] |= g.last[p];
            }
            out = r;
            return true;
        }
        case REP: {
            // a subtree without an element makes no position: one copy says all (X{a,b} of assertions alone is X, or empty)
            const int copies = nodes[id].has_element ? nodes[id].b : 1;
            for (int i = 0; i < copies; ++i) {
                AFrag g;
                if (!aexpand(nodes[id].kids[0], g)) return false;
                if (i >= nodes[id].a) g.nullable = true, g.eps = REL_FULL;
                out = acat(out, g);
            }
            return true;
        }
        }
        return false;
    }

    // ---- bmx_compile_regex_groups: the refusal rule, then pref / open / close from the expanded tree ----
    bool can_be_empty(int id) const
    {
        const Node &n = nodes[id];
        switch (n.kind) {
        case ELEM: return false;
        case ASSERT: return true;
        case GROUP: return can_be_empty(n.kids[0]);
        case REP: return n.a == 0 || can_be_empty(n.kids[0]);
        case CAT:
            for (int k : n.kids)
                if (!can_be_empty(k)) return false;
            return true;
        case ALT:
            for (int k : n.kids)
                if (can_be_empty(k)) return true;
            return false;
        }
        return false;
    }

    // No repeat with b >= 2 whose body can match the empty string and holds a capturing group: engines disagree there.
    bool repeats_capture_exactly(int id)
    {
        const Node &n = nodes[id];
        if (n.kind == REP && n.b >= 2 && n.has_group && can_be_empty(n.kids[0]))
            return fail("a repeat of two or more whose body can match the empty string and holds a capturing group");
        for (int k : n.kids)
            if (!repeats_capture_exactly(k)) return false;
        return true;
    }

    // The expanded tree as states with ordered epsilon moves: a state either consumes (pos >= 0, then `next`) or has moves
    // in the order a backtracking matcher tries them.  A move may carry tags.
    struct Move {
        int to;
        uint16_t open, close;
    };
    struct State {
        int pos = -1, next = -1;
        std::vector<Move> moves;
    };
    std::vector<State> states;
    int n_pos = 0;

    int state()
    {
        states.emplace_back();
        return (int)states.size() - 1;
    }
    void move(int from, int to, uint16_t open = 0, uint16_t close = 0) { states[from].moves.push_back({to, open, close}); }

    // Node id behind state `in`; returns the state behind it.  Positions are numbered as expand() numbers them: left to
    // right, copy by copy.  A subtree without an element still threads its groups: () and (a|) fire their tags.
    int thread(int id, int in)
    {
        const Node &n = nodes[id];
        if (!n.has_element && !n.has_group) return in; // the empty string, and no tag
        switch (n.kind) {
        case ASSERT: return in;
        case ELEM: {
            const int c = state(), out = state();
            states[c].pos = n_pos++;
            states[c].next = out;
            move(in, c);
            return out;
        }
        case GROUP: {
            const uint16_t bit = (uint16_t)(1u << (n.a - 1));
            const int kin = state();
            move(in, kin, bit, 0);
            const int kout = thread(n.kids[0], kin), out = state();
            move(kout, out, 0, bit);
            return out;
        }
        case CAT:
            for (int k : n.kids) in = thread(k, in);
            return in;
        case ALT: {
            const int out = state();
            for (int k : n.kids) { // left to right
                const int kin = state();
                move(in, kin);
                move(thread(k, kin), out);
            }
            return out;
        }
        case REP: {
            const int copies = n.has_element ? n.b : 1; // (without an element and with a group: b == 1, or it was refused)
            for (int i = 0; i < copies; ++i) {
                if (i < n.a) {
                    in = thread(n.kids[0], in);
                    continue;
                }
                const int kin = state(), after = state();
                move(in, kin); // an optional copy before its skip
                move(thread(n.kids[0], kin), after);
                move(in, after);
                in = after;
            }
            return in;
        }
        }
        return in;
    }

    // depth first from the state behind `row`: the first path to a consuming position, or to the end, gives the pair's
    // rank and tags.  All tags of one boundary fire at the same text offset, so their order among themselves is immaterial.
    void walk(int s, uint16_t open, uint16_t close, int row, int final_state, std::vector<char> &seen, int &rank, bmx_regex_groups &g) const
    {
        if (seen[s]) return;
        seen[s] = 1;
        const int q = states[s].pos >= 0 ? states[s].pos : s == final_state ? BMX_REGEX_END : -1;
        if (q >= 0) {
            if (q != BMX_REGEX_END) g.pref[row][rank++] = (uint8_t)q;
            g.open[row][q] = open;
            g.close[row][q] = close;
            return;
        }
        for (const Move &mv : states[s].moves) walk(mv.to, (uint16_t)(open | mv.open), (uint16_t)(close | mv.close), row, final_state, seen, rank, g);
    }

    void tables(int root, bmx_regex_groups &g)
    {
        states.clear();
        n_pos = 0;
        const int start = state();
        const int final_state = thread(root, start);
        std::memset(&g, 0, sizeof g);
        std::memset(g.pref, 0xFF, sizeof g.pref);
        g.n_groups = n_groups;
        int behind[BMX_MAX_REGEX_POSITIONS + 1];
        for (int &b : behind) b = -1;
        behind[BMX_REGEX_START] = start;
        for (const State &st : states)
            if (st.pos >= 0) behind[st.pos] = st.next;
        for (int row = 0; row <= BMX_MAX_REGEX_POSITIONS; ++row) {
            if (behind[row] < 0) continue;
            std::vector<char> seen(states.size(), 0);
            int rank = 0;
            walk(behind[row], 0, 0, row, final_state, seen, rank, g);
        }
    }
};

// bit k: the class holds a byte of category k
int class_cats(const uint8_t *cls)
{
    int cats = 0;
    for (unsigned c = 0; c < 256; ++c)
        if ((cls[c >> 3] >> (c & 7)) & 1u) cats |= 1 << cat_of(c);
    return cats;
}

// the class of all bytes whose category is in `cats`
void cats_class(int cats, uint8_t *cls)
{
    std::memset(cls, 0, BMX_CLASS_BYTES);
    for (unsigned c = 0; c < 256; ++c)
        if ((cats >> cat_of(c)) & 1) cls[c >> 3] |= (uint8_t)(1u << (c & 7));
}

// From the expansion with relations to plain data: the automaton and the two classes per position.  A first position
// whose admissible bytes before it depend on the category of its own byte (\b in front of [a-z.]) is split by category
// into copies that stand side by side, and so is a last position; then every relation on an edge is decided from the
// two classes, or the expression is refused.  Returns NULL, or why not.
const char *resolve(const Compiler &c, const AFrag &f, uint32_t flags, bmx_regex *re_out, bmx_regex_anchors *an_out)
{
    const int m = c.re.m;
    uint16_t F[BMX_MAX_REGEX_POSITIONS], L[BMX_MAX_REGEX_POSITIONS];
    for (int p = 0; p < m; ++p) {
        F[p] = f.first[p], L[p] = f.last[p];
        if (flags & BMX_REGEX_WORD) F[p] &= REL_BEFORE_NOT_WORD, L[p] &= REL_AFTER_NOT_WORD;
        if (flags & BMX_REGEX_LINE) F[p] &= REL_BOL, L[p] &= REL_EOL;
    }
    struct Copy {
        int of, cats, before, after; // the position it copies; the categories it keeps; categories admitted before / after it
    };
    std::vector<Copy> copies;
    int begin[BMX_MAX_REGEX_POSITIONS + 1];
    for (int p = 0; p < m; ++p) {
        begin[p] = (int)copies.size();
        const int cats = class_cats(c.re.classes + (size_t)p * BMX_CLASS_BYTES);
        int before[3], after[3];
        for (int b = 0; b < 3; ++b) {
            before[b] = after[b] = 0;
            for (int a = 0; a < 3; ++a) {
                if ((F[p] >> (3 * a + b)) & 1) before[b] |= 1 << a;
                if ((L[p] >> (3 * b + a)) & 1) after[b] |= 1 << a;
            }
        }
        if (cats == 0) { // an empty class consumes nothing: kept as one position, for the numbering
            copies.push_back({p, 0, before[0] & before[1] & before[2], after[0] & after[1] & after[2]});
            continue;
        }
        for (int b = 0; b < 3; ++b) { // categories with the same answers on both sides stay together
            if (!((cats >> b) & 1)) continue;
            size_t q = begin[p];
            while (q < copies.size() && (copies[q].before != before[b] || copies[q].after != after[b])) ++q;
            if (q == copies.size()) copies.push_back({p, 0, before[b], after[b]});
            copies[q].cats |= 1 << b;
        }
    }
    begin[m] = (int)copies.size();
    const int m2 = (int)copies.size();
    if (m2 > BMX_MAX_REGEX_POSITIONS) return "more than 64 positions after splitting";

    bmx_regex re;
    bmx_regex_anchors an;
    std::memset(&re, 0, sizeof re);
    std::memset(&an, 0xFF, sizeof an); // a full class: no condition
    re.m = m2;
    for (int q = 0; q < m2; ++q) {
        const Copy &k = copies[q];
        uint8_t keep[BMX_CLASS_BYTES];
        cats_class(k.cats, keep);
        for (int t = 0; t < BMX_CLASS_BYTES; ++t)
            re.classes[(size_t)q * BMX_CLASS_BYTES + t] = c.re.classes[(size_t)k.of * BMX_CLASS_BYTES + t] & keep[t];
        // (a copy that admits no byte on a side stays in the set with an empty class: it begins or ends no match)
        if (f.first[k.of]) re.first |= 1ull << q, cats_class(k.before, an.before + (size_t)q * BMX_CLASS_BYTES);
        if (f.last[k.of]) re.last |= 1ull << q, cats_class(k.after, an.after + (size_t)q * BMX_CLASS_BYTES);
    }
    for (int l = 0; l < m; ++l) {
        for (int r = l + 1; r < m; ++r) {
            const int rel = c.edge[l][r];
            if (rel == 0) continue;
            for (int ql = begin[l]; ql < begin[l + 1]; ++ql) {
                for (int qr = begin[r]; qr < begin[r + 1]; ++qr) {
                    int holds = 0, pairs = 0;
                    for (int a = 0; a < 3; ++a)
                        for (int b = 0; b < 3; ++b)
                            if (((copies[ql].cats >> a) & 1) && ((copies[qr].cats >> b) & 1)) ++pairs, holds += (rel >> (3 * a + b)) & 1;
                    if (rel != REL_FULL && holds != 0 && holds != pairs)
                        return "an assertion between two positions whose classes do not decide it";
                    if (rel == REL_FULL || holds != 0) re.follow[ql] |= 1ull << qr;
                }
            }
        }
    }
    if (re.first != 0 && re.last != 0) bmx_regex_lengths(re.m, re.first, re.last, re.follow, &re.min_len, &re.max_len);
    if (re.max_len == 0) return "the assertions leave no possible match";
    *re_out = re;
    *an_out = an;
    return nullptr;
}

} // namespace

namespace {

// The plain grammar (star: with * + {a,}) up to `limit` positions: c.re and f on BMX_OK, else the error text is set.
int compile(const char *where, bool star, int limit, const char *expr, uint64_t expr_len, uint32_t flags, bool have_out, Compiler &c,
            Frag &f, bool groups = false, int *root_out = nullptr)
{
    char text[160];
    if (!expr || !have_out) {
        snprintf(text, sizeof text, "%s: a NULL argument", where);
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    if (flags & ~(BMX_CLASS_ICASE | BMX_CLASS_IUPAC)) {
        snprintf(text, sizeof text, "%s: an unknown flag bit", where);
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    c.e = reinterpret_cast<const uint8_t *>(expr);
    c.len = expr_len;
    c.flags = flags;
    c.star = star;
    c.groups = groups;
    c.limit = limit;
    std::memset(&c.re, 0, sizeof c.re);
    int root = 0;
    f = {true, 0, 0};
    bool ok = c.parse_alt(0, root);
    if (ok && c.at < c.len) ok = c.fail("an unbalanced )");
    if (ok) ok = c.expand(root, f);
    if (ok && c.re.m == 0) ok = c.fail("zero positions");
    if (ok && f.nullable) ok = c.fail("the expression matches the empty string");
    if (ok && groups) ok = c.repeats_capture_exactly(root);
    if (root_out) *root_out = root;
    if (!ok) {
        snprintf(text, sizeof text, "%s: %s", where, c.why ? c.why : "a bad expression");
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}

// the compiler's automaton of at most 64 positions as struct bmx_regex: the low word of every set is the whole set
bmx_regex store(const Compiler &c, const Frag &f, bool star)
{
    bmx_regex re;
    std::memset(&re, 0, sizeof re);
    re.m = c.re.m;
    re.first = (uint64_t)f.first;
    re.last = (uint64_t)f.last;
    for (int32_t i = 0; i < re.m; ++i) re.follow[i] = (uint64_t)c.re.follow[i];
    std::memcpy(re.classes, c.re.classes, sizeof re.classes);
    if (star) bmx_regex_star_lengths(re.m, re.first, re.last, re.follow, &re.min_len, &re.max_len, nullptr);
    else bmx_regex_lengths(re.m, re.first, re.last, re.follow, &re.min_len, &re.max_len);
    return re;
}

// ... into struct bmx_regex
int compile(const char *where, bool star, const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out)
{
    Compiler c;
    Frag f;
    const int rc = compile(where, star, BMX_MAX_REGEX_POSITIONS, expr, expr_len, flags, out != nullptr, c, f);
    if (rc != BMX_OK) return rc;
    *out = store(c, f, star);
    return BMX_OK;
}

} // namespace

// The star-free grammar with capturing groups: the same automaton, and the capture model from the tree beside it.
extern "C" int bmx_compile_regex_groups(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *re, bmx_regex_groups *gr)
{
    Compiler c;
    Frag f;
    int root = 0;
    const int rc = compile("bmx_compile_regex_groups", false, BMX_MAX_REGEX_POSITIONS, expr, expr_len, flags, re != nullptr && gr != nullptr,
                           c, f, true, &root);
    if (rc != BMX_OK) return rc;
    bmx_regex_groups g;
    c.tables(root, g);
    *re = store(c, f, false);
    *gr = g;
    return BMX_OK;
}

extern "C" int bmx_regex_groups_valid(const bmx_regex *re, const bmx_regex_groups *gr)
{
    if (!re || !gr || !bmx_regex_sets_ok(re->m, re->first, re->last, re->follow)) return 0;
    if (gr->n_groups < 0 || gr->n_groups > BMX_MAX_REGEX_GROUPS) return 0;
    const uint32_t known = (1u << gr->n_groups) - 1u;
    for (int row = 0; row <= BMX_MAX_REGEX_POSITIONS; ++row) {
        const bool live = row == BMX_REGEX_START || row < re->m;
        const uint64_t set = !live ? 0 : row == BMX_REGEX_START ? re->first : re->follow[row];
        uint64_t seen = 0;
        int k = 0;
        for (; k < BMX_MAX_REGEX_POSITIONS && gr->pref[row][k] != 0xFF; ++k) { // a permutation of the set ...
            const unsigned q = gr->pref[row][k];
            if (q >= (unsigned)BMX_MAX_REGEX_POSITIONS || !((set >> q) & 1) || ((seen >> q) & 1)) return 0;
            seen |= 1ull << q;
        }
        if (seen != set) return 0;
        for (; k < BMX_MAX_REGEX_POSITIONS; ++k) // ... and nothing behind it
            if (gr->pref[row][k] != 0xFF) return 0;
        for (int col = 0; col <= BMX_MAX_REGEX_POSITIONS; ++col) {
            const uint32_t tags = (uint32_t)gr->open[row][col] | gr->close[row][col];
            if (tags == 0) continue;
            const bool pair = col < BMX_MAX_REGEX_POSITIONS ? ((set >> col) & 1) != 0
                                                            : row != BMX_REGEX_START && live && ((re->last >> row) & 1) != 0;
            if (!pair || (tags & ~known)) return 0;
        }
    }
    return 1;
}

// A replacement template into its references and the literals between them.
extern "C" int bmx_compile_template(const void *tmpl, uint64_t len, int32_t n_groups, bmx_template *out, void *lits)
{
    const char *why = nullptr;
    bmx_template t;
    std::memset(&t, 0, sizeof t);
    std::vector<uint8_t> bytes;
    if (!out || (len > 0 && (!tmpl || !lits))) why = "a NULL argument";
    else if (len > BMX_MAX_REPLACEMENT) why = "a template longer than 65536 bytes";
    else if (n_groups < 0 || n_groups > BMX_MAX_REGEX_GROUPS) why = "n_groups outside 0..16";
    const uint8_t *p = static_cast<const uint8_t *>(tmpl);
    size_t lit0 = 0; // where the current literal begins in `bytes`
    for (uint64_t i = 0; !why && i < len;) {
        if (p[i] != '\\') {
            bytes.push_back(p[i++]);
            continue;
        }
        const unsigned c = i + 1 < len ? p[i + 1] : 0x100u;
        int ref = -1;
        if (c == '\\') {
            bytes.push_back('\\');
            i += 2;
            continue;
        } else if (c >= '1' && c <= '9') {
            if (i + 2 < len && p[i + 2] >= '0' && p[i + 2] <= '9') why = "a digit right behind \\1..\\9 (engines read two digits there: write \\g<N>)";
            ref = (int)(c - '0');
            i += 2;
        } else if (c == 'g' && i + 2 < len && p[i + 2] == '<') {
            uint64_t j = i + 3;
            int digits = 0;
            for (ref = 0; j < len && p[j] >= '0' && p[j] <= '9' && digits < 3; ++j, ++digits) ref = 10 * ref + (int)(p[j] - '0');
            if (digits < 1 || digits > 2 || j >= len || p[j] != '>') why = "\\g without <one or two digits>";
            i = j + 1;
        } else {
            why = c == 0x100u ? "a dangling backslash" : "an escape that is none of \\1..\\9, \\g<N>, \\\\";
        }
        if (why) break;
        if (ref > n_groups) why = "a reference to a group the expression does not have";
        else if (t.n_refs == BMX_MAX_TEMPLATE_REFS) why = "more than 32 references";
        if (why) break;
        t.ref[t.n_refs] = ref;
        t.lit_off[t.n_refs] = (uint32_t)lit0;
        t.lit_len[t.n_refs] = (uint32_t)(bytes.size() - lit0);
        lit0 = bytes.size();
        ++t.n_refs;
    }
    if (why) {
        char text[192];
        snprintf(text, sizeof text, "bmx_compile_template: %s", why);
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    t.lit_off[t.n_refs] = (uint32_t)lit0;
    t.lit_len[t.n_refs] = (uint32_t)(bytes.size() - lit0);
    t.lit_bytes = (uint32_t)bytes.size();
    *out = t;
    if (!bytes.empty()) std::memcpy(lits, bytes.data(), bytes.size());
    return BMX_OK;
}

extern "C" int bmx_compile_regex(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out)
{
    return compile("bmx_compile_regex", false, expr, expr_len, flags, out);
}

// The star-free grammar with the zero-width atoms: the same parser, the expansion with relations, then resolve().
extern "C" int bmx_compile_regex_anchored(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *re, bmx_regex_anchors *an)
{
    const char *where = "bmx_compile_regex_anchored";
    char text[192];
    const char *why = nullptr;
    Compiler c;
    AFrag f;
    if (!expr || !re || !an) why = "a NULL argument";
    else if (flags & ~(BMX_CLASS_ICASE | BMX_CLASS_IUPAC | BMX_REGEX_WORD | BMX_REGEX_LINE)) why = "an unknown flag bit";
    if (!why) {
        c.e = reinterpret_cast<const uint8_t *>(expr);
        c.len = expr_len;
        c.flags = flags & (BMX_CLASS_ICASE | BMX_CLASS_IUPAC);
        c.anchored = true;
        std::memset(&c.re, 0, sizeof c.re);
        std::memset(c.edge, 0, sizeof c.edge);
        int root = 0;
        bool ok = c.parse_alt(0, root);
        if (ok && c.at < c.len) ok = c.fail("an unbalanced )");
        if (ok) ok = c.aexpand(root, f);
        if (ok && c.re.m == 0) ok = c.fail("zero positions");
        if (ok && f.nullable) ok = c.fail("the expression matches the empty string once its assertions are ignored");
        if (!ok) why = c.why ? c.why : "a bad expression";
    }
    if (!why) why = resolve(c, f, flags, re, an);
    if (why) {
        snprintf(text, sizeof text, "%s: %s", where, why);
        bmx_internal_set_error(text);
        return BMX_ERR_ARG;
    }
    return BMX_OK;
}

extern "C" int bmx_compile_regex_star(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex *out)
{
    return compile("bmx_compile_regex_star", true, expr, expr_len, flags, out);
}

// The star-free grammar up to 128 positions, into the struct with two-word sets.
extern "C" int bmx_compile_regex_long(const char *expr, uint64_t expr_len, uint32_t flags, bmx_regex_long *out)
{
    Compiler c;
    Frag f;
    const int rc = compile("bmx_compile_regex_long", false, BMX_MAX_REGEX_LONG_POSITIONS, expr, expr_len, flags, out != nullptr, c, f);
    if (rc != BMX_OK) return rc;
    bmx_regex_long re;
    std::memset(&re, 0, sizeof re);
    re.m = c.re.m;
    bmx_set128_store(f.first, re.first);
    bmx_set128_store(f.last, re.last);
    for (int32_t i = 0; i < re.m; ++i) bmx_set128_store(c.re.follow[i], re.follow[i]);
    std::memcpy(re.classes, c.re.classes, sizeof re.classes);
    bmx_regex_lengths_t<Set>(re.m, f.first, f.last, c.re.follow, &re.min_len, &re.max_len);
    *out = re;
    return BMX_OK;
}

// The automaton of a struct bmx_regex in the wide struct: the low words are its sets, the high words are empty.
extern "C" int bmx_regex_long_widen(const bmx_regex *in, bmx_regex_long *out)
{
    if (!in || !out || !bmx_regex_sets_ok(in->m, in->first, in->last, in->follow)) {
        bmx_internal_set_error("bmx_regex_long_widen: a NULL argument or an automaton that is not valid");
        return BMX_ERR_ARG;
    }
    bmx_regex_long re;
    std::memset(&re, 0, sizeof re);
    re.m = in->m;
    re.first[0] = in->first;
    re.last[0] = in->last;
    for (int32_t i = 0; i < in->m; ++i) re.follow[i][0] = in->follow[i];
    std::memcpy(re.classes, in->classes, sizeof in->classes);
    bmx_regex_lengths(in->m, in->first, in->last, in->follow, &re.min_len, &re.max_len);
    *out = re;
    return BMX_OK;
}
