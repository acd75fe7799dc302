"""CPU suite of the capture model (bmx_compile_regex_groups, bmx_regex_groups_valid, bmx_compile_template): the library's
tables against tests/regex_groups_oracle.py (written from the header's description) for a fixed list and for random
expressions; the automaton byte for byte against bmx_compile_regex; every refusal; the oracle's walker over the LIBRARY's
tables against Python's ``re.fullmatch(...).regs`` on every matching span of every short text over {a, b, c}; the
argument errors of the device entries before any HIP call (ctx = NULL); every accepted and refused template form."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import regex_groups_oracle as go
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

FIXED = ["(a|ab)(c|bcd)(d?)", "((a?)b){2}", "(a?|[bc])([bc]?)c", "((a)|b){2}", "(a)?b", "(a?)b", "()a", "(a|)b", "a(?:b|c)(d)",
         "(a?)?b", "(a|b?)c", "((a|b)(c)?){1,3}", "(?:(a)|(b)|(c)){2}", "([0-9]{4})-([0-9]{2})-([0-9]{2})",
         "(ERROR|FATAL): ([0-9]{2,4})", "(..)(..)", "(a){0,2}(?:b(c)){1,2}", "((((a))))", "(a)(?:)(b)", "x(|a|ab)(b?)y"]
WIDE, WIDE_PIECES = go.WIDE, go.WIDE_PIECES
REFUSED = {
    "(a?){2}b": "a repeat of two or more", "((a)|b?){1,3}c": "a repeat of two or more", "(){3}a": "a repeat of two or more",
    "(?:(a)?){2}b": "a repeat of two or more", "(a|){2}b": "a repeat of two or more",
    "(?a)": "(? followed by", "(?=a)b": "(? followed by", "(?P<x>a)": "(? followed by", "(?": "(? followed by",
    "(a)" * 17: "more than 16 capturing groups",
    "a*": "unbounded", "(a": "unbalanced", "a)": "unbalanced", "(a?)": "empty string", "": "zero positions", "?a": "quantifier",
    "(a){2,1}": "0 <= a <= b", "[a": "bad element", "(?:a){65}": "more than 64 positions",
}


def lib_tables(expr, flags=0):
    re_, gr = host.compile_regex_groups(expr, flags)
    return re_, gr, (gr.n_groups, gr.pref_array(), gr.open_array(), gr.close_array())


def same_tables(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_struct_layout_and_constants(built):
    G = host.RegexGroups
    assert (G.n_groups.offset, G.pref.offset, G.open.offset, G.close.offset, C.sizeof(G)) == (0, 4, 4164, 12614, 21064)
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    define = lambda name: int(re.search(rf"#define {name}\s+(\d+)", src).group(1))
    assert define("BMX_MAX_REGEX_GROUPS") == host.MAX_REGEX_GROUPS == go.MAX_GROUPS == 16
    assert define("BMX_REGEX_START") == define("BMX_REGEX_END") == host.REGEX_START == host.REGEX_END == go.START == 64
    assert define("BMX_MAX_TEMPLATE_REFS") == host.MAX_TEMPLATE_REFS == 32 and define("BMX_EXPAND_EXTRACT") == host.EXPAND_EXTRACT == 1


@pytest.mark.parametrize("expr", FIXED + [WIDE])
def test_tables_equal_the_oracle_fixed(built, expr):
    re_, gr, got = lib_tables(expr)
    assert same_tables(got, go.tables(expr)), expr
    assert bytes(re_) == bytes(host.compile_regex(expr.replace("(?:", "("))), "the automaton is bmx_compile_regex's"
    assert host.lib().bmx_regex_groups_valid(C.byref(re_), C.byref(gr)) == 1


def test_wide_expression_has_64_positions_and_16_groups(built):
    re_, gr, _ = lib_tables(WIDE)
    assert re_.m == 64 and gr.n_groups == 16


def test_preference_is_not_the_position_index(built):
    _, gr, _ = lib_tables("(a?|[bc])([bc]?)c")  # positions: a=0 [bc]=1 [bc]=2 c=3
    assert gr.pref_array()[host.REGEX_START, :4].tolist() == [0, 2, 3, 1]


@pytest.mark.parametrize("expr", sorted(REFUSED))
def test_refusals_leave_the_outputs_untouched(built, expr):
    re_, gr = host.Regex(), host.RegexGroups()
    C.memset(C.byref(re_), 0xA5, C.sizeof(re_))
    C.memset(C.byref(gr), 0x5A, C.sizeof(gr))
    before = bytes(re_), bytes(gr)
    e = expr.encode()
    assert host.lib().bmx_compile_regex_groups(e, len(e), 0, C.byref(re_), C.byref(gr)) == host.ERR_ARG
    text = host.lib().bmx_last_error().decode()
    assert text.startswith("bmx_compile_regex_groups: ") and REFUSED[expr] in text, text
    assert (bytes(re_), bytes(gr)) == before
    # (?: stays an error in every other compile entry
    if expr.startswith("(?"):
        with pytest.raises(host.BmxError):
            host.compile_regex(expr)


def test_non_capturing_group_is_an_error_elsewhere(built):
    for compile_ in (host.compile_regex, host.compile_regex_star, host.compile_regex_long, host.compile_regex_anchored):
        with pytest.raises(host.BmxError):
            compile_("(?:a)b")
    host.compile_regex_groups("(?:a)b")


def test_null_arguments_and_flags(built):
    L = host.lib()
    re_, gr = host.Regex(), host.RegexGroups()
    assert L.bmx_compile_regex_groups(b"(a)", 3, 0, None, C.byref(gr)) == host.ERR_ARG
    assert L.bmx_compile_regex_groups(b"(a)", 3, 0, C.byref(re_), None) == host.ERR_ARG
    assert L.bmx_compile_regex_groups(None, 0, 0, C.byref(re_), C.byref(gr)) == host.ERR_ARG
    assert L.bmx_compile_regex_groups(b"(a)", 3, 64, C.byref(re_), C.byref(gr)) == host.ERR_ARG
    a, ga = host.compile_regex_groups("(a)b", host.CLASS_ICASE)
    assert bytes(a) == bytes(host.compile_regex("(a)b", host.CLASS_ICASE)) and ga.n_groups == 1


FIXED_REGS = [
    ("(a|ab)(c|bcd)(d?)", b"abcd", ((0, 4), (0, 1), (1, 4), (4, 4))),
    ("((a?)b){2}", b"abb", ((0, 3), (2, 3), (2, 2))),
    ("(a?|[bc])([bc]?)c", b"bc", ((0, 2), (0, 0), (0, 1))),
    ("((a)|b){2}", b"ab", ((0, 2), (1, 2), (0, 1))),
    ("(a)?b", b"b", ((0, 1), (-1, -1))),
    ("(a?)b", b"b", ((0, 1), (0, 0))),
]


@pytest.mark.parametrize("expr,text,want", FIXED_REGS)
def test_fixed_cases(built, expr, text, want):
    re_, gr = host.compile_regex_groups(expr)
    got = go.walk(go.Model.from_library(re_, gr), text, 0, len(text) - 1)
    assert got == want == go.py_regs(expr, text, 0, len(text) - 1)


def test_wide_expression_against_re(built):
    re_, gr = host.compile_regex_groups(WIDE)
    model = go.Model.from_library(re_, gr)
    rng = np.random.default_rng(64)
    for _ in range(40):
        text = "".join(WIDE_PIECES[i % 2][int(rng.integers(0, 6))] for i in range(16)).encode()
        want = go.py_regs(WIDE, text, 0, len(text) - 1)
        assert want is not None and go.walk(model, text, 0, len(text) - 1) == want


def test_walker_over_library_tables_equals_re_on_every_span(built):
    """Random expressions over {a, b, c}; every text of 1..6 bytes is tried as a whole span, so no matching span of these
    texts is left out.  At least 20,000 matching spans."""
    rng = np.random.default_rng(20260)
    texts = [bytes(t) for n in range(1, 7) for t in itertools.product(b"abc", repeat=n)]
    spans = accepted = 0
    while spans < 20000:
        expr = go.random_expr(rng)
        try:
            want_tables = go.tables(expr)
        except go.Refused:
            with pytest.raises(host.BmxError):
                host.compile_regex_groups(expr)
            continue
        re_, gr, got = lib_tables(expr)
        assert same_tables(got, want_tables), expr
        assert bytes(re_) == bytes(host.compile_regex(expr.replace("(?:", "("))), expr
        accepted += 1
        model = go.Model.from_library(re_, gr)
        pattern = re.compile(expr.encode(), re.DOTALL)
        for text in texts:
            if not re_.min_len <= len(text) <= re_.max_len:
                assert pattern.fullmatch(text) is None
                continue
            mt = pattern.fullmatch(text)
            got_regs = go.walk(model, text, 0, len(text) - 1)
            assert got_regs == (None if mt is None else tuple(mt.regs)), (expr, text)
            spans += mt is not None
    assert accepted >= 100


def test_walker_inside_a_longer_text(built):
    expr, text = "(a|ab)(c|bcd)(d?)", b"xxabcdyy"
    re_, gr = host.compile_regex_groups(expr)
    assert go.walk(go.Model.from_library(re_, gr), text, 2, 5) == go.py_regs(expr, text, 2, 5) == ((2, 6), (2, 3), (3, 6), (6, 6))
    assert go.walk(go.Model.from_library(re_, gr), text, 1, 5) is None


def test_validity_check(built):
    L = host.lib()
    re_, gr = host.compile_regex_groups("(a|b)(c?)d")
    ok = lambda g: L.bmx_regex_groups_valid(C.byref(re_), C.byref(g))
    assert ok(gr) == 1 and L.bmx_regex_groups_valid(None, C.byref(gr)) == 0 and L.bmx_regex_groups_valid(C.byref(re_), None) == 0

    def changed(edit):
        g = host.RegexGroups.from_buffer_copy(bytes(gr))
        edit(g)
        return g

    def set_(table, i, j, v):
        def edit(g):
            getattr(g, table)[i][j] = v
        return edit

    assert ok(changed(lambda g: setattr(g, "n_groups", 17))) == 0
    assert ok(changed(lambda g: setattr(g, "n_groups", -1))) == 0
    assert ok(changed(set_("pref", 64, 0, 1))) == 0      # START lists position 1 twice
    assert ok(changed(set_("pref", 64, 1, 0xFF))) == 0   # ... or leaves one out
    assert ok(changed(set_("pref", 64, 2, 3))) == 0      # ... or lists one that is not in `first`
    assert ok(changed(set_("pref", 10, 0, 0))) == 0      # a row of no position
    assert ok(changed(set_("open", 0, 2, 4))) == 0       # a tag bit at or above n_groups
    assert ok(changed(set_("open", 0, 1, 1))) == 0       # a tag on a pair outside follow
    assert ok(changed(set_("close", 0, 64, 1))) == 0     # ... on (p, END) with p not in last
    assert ok(changed(set_("close", 64, 64, 1))) == 0    # ... on (START, END)
    assert ok(changed(set_("open", 0, 2, 3))) == 1       # inside follow and below n_groups: valid
    bad_re = host.Regex.from_buffer_copy(bytes(re_))
    bad_re.follow[1] = 1
    assert L.bmx_regex_groups_valid(C.byref(bad_re), C.byref(gr)) == 0


def test_device_entries_refuse_bad_arguments_before_any_hip_call(built):
    L = host.lib()
    re_, gr = host.compile_regex_groups("(a)b")
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    args = lambda r, g, s, e, c, o, n=4: (None, p, n, 0, r, g, s, e, c, o, None)
    R, G = C.byref(re_), C.byref(gr)
    assert L.bmx_regex_groups_device(*args(R, G, None, None, 0, None)) == host.OK       # count == 0 launches nothing
    assert L.bmx_regex_groups_device(*args(R, G, p, p, 1, p)) == host.ERR_ARG           # no context
    assert L.bmx_regex_groups_device(*args(None, G, p, p, 1, p)) == host.ERR_ARG
    assert L.bmx_regex_groups_device(*args(R, None, p, p, 1, p)) == host.ERR_ARG
    assert L.bmx_regex_groups_device(*args(R, G, None, p, 1, p)) == host.ERR_ARG
    assert L.bmx_regex_groups_device(*args(R, G, p, p, 1, None)) == host.ERR_ARG
    assert L.bmx_regex_groups_device(*args(R, G, p, p, 0, None, n=1 << 40)) == host.ERR_ARG
    bad = host.RegexGroups.from_buffer_copy(bytes(gr))
    bad.pref[64][0] = 1
    assert L.bmx_regex_groups_device(*args(R, C.byref(bad), None, None, 0, None)) == host.ERR_ARG
    total = C.c_uint64(7)
    ex = lambda tmpl, flags=0, groups=p, count=1, out=None, cap=0, off=None, ng=1, n=4: L.bmx_expand_device(
        None, p, n, 0, groups, ng, count, tmpl, len(tmpl), flags, out, cap, off, C.byref(total), None)
    assert ex(b"\\1") == host.ERR_ARG                           # no context
    assert ex(b"\\2") == host.ERR_ARG and "bmx_compile_template" in L.bmx_last_error().decode()
    assert ex(b"x", flags=2) == host.ERR_ARG and ex(b"x", flags=1) == host.ERR_ARG  # an unknown flag; EXTRACT without offsets
    assert ex(b"x", groups=None) == host.ERR_ARG and ex(b"x", ng=17) == host.ERR_ARG and ex(b"x", n=1 << 40) == host.ERR_ARG
    assert ex(b"x", out=p, cap=8) == host.ERR_ARG               # the output overlaps the text
    assert ex(b"x", count=0) == host.OK and total.value == 4    # no match, counting only: the text's length


ACCEPTED_TEMPLATES = [
    (b"", 0, [], [b""]), (b"plain", 0, [], [b"plain"]), (b"\\1", 1, [1], [b"", b""]), (b"\\3.\\2.\\1", 3, [3, 2, 1], [b"", b".", b".", b""]),
    (b"\\1\\2", 2, [1, 2], [b"", b"", b""]), (b"a\\\\b", 0, [], [b"a\\b"]), (b"\\\\1", 1, [], [b"\\1"]), (b"<\\g<0>>", 0, [0], [b"<", b">"]),
    (b"\\g<16>\\g<1>0", 16, [16, 1], [b"", b"", b"0"]), (b"\\g<01>x", 1, [1], [b"", b"x"]), (b"\\9", 9, [9], [b"", b""]),
    (b"\\1" * 32, 1, [1] * 32, [b""] * 33), (b"\x00\xff\\1\n", 1, [1], [b"\x00\xff", b"\n"]),
]
REFUSED_TEMPLATES = [(b"\\", 1), (b"a\\", 1), (b"\\0", 1), (b"\\n", 1), (b"\\2", 1), (b"\\g<2>", 1), (b"\\g<17>", 16), (b"\\g<1", 1),
                     (b"\\g<>", 1), (b"\\g1", 1), (b"\\g<a>", 1), (b"\\g<123>", 16), (b"\\10", 16), (b"\\1" * 33, 1), (b"\\x41", 1),
                     (b"x" * (host.MAX_REPLACEMENT + 1), 0), (b"x", -1), (b"x", 17)]


@pytest.mark.parametrize("tmpl,n_groups,refs,lits", ACCEPTED_TEMPLATES)
def test_template_accepted(built, tmpl, n_groups, refs, lits):
    t, blob = host.compile_template(tmpl, n_groups)
    assert t.n_refs == len(refs) and list(t.ref[: t.n_refs]) == refs
    got = [blob[t.lit_off[r]: t.lit_off[r] + t.lit_len[r]] for r in range(t.n_refs + 1)]
    assert got == lits and t.lit_bytes == sum(map(len, lits)) == len(blob)
    # the subset on which Python's template syntax agrees: expand on a match that has all groups
    mt = re.fullmatch(b"".join(b"(%c)" % (97 + i) for i in range(n_groups)) or b"", bytes(range(97, 97 + n_groups)))
    want = mt.expand(tmpl)
    parts = [lits[r] + (mt.group(refs[r]) if r < len(refs) else b"") for r in range(len(lits))]
    assert b"".join(parts) == want


@pytest.mark.parametrize("tmpl,n_groups", REFUSED_TEMPLATES)
def test_template_refused(built, tmpl, n_groups):
    out = host.Template()
    C.memset(C.byref(out), 0x77, C.sizeof(out))
    before = bytes(out)
    lits = C.create_string_buffer(len(tmpl) + 1)
    assert host.lib().bmx_compile_template(tmpl, len(tmpl), n_groups, C.byref(out), lits) == host.ERR_ARG
    assert host.lib().bmx_last_error().decode().startswith("bmx_compile_template: ")
    assert bytes(out) == before and lits.raw == bytes(len(tmpl) + 1)
    assert host.lib().bmx_compile_template(b"x", 1, 0, None, lits) == host.ERR_ARG


def test_package_exports(built):
    import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

    for name in ("compile_regex_groups", "compile_template", "search_regex_groups", "RegexGroups", "Template", "MAX_REGEX_GROUPS",
                 "MAX_TEMPLATE_REFS", "EXPAND_EXTRACT"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("regex_groups_device", "search_regex_groups", "expand_device", "last_regex_groups_ms"):
        assert callable(getattr(host.Context, name))
    for kw in ({"merge": True}, {"longest": True}):
        with pytest.raises(ValueError):
            host.Context._selected_groups_device(None, None, "(a)", None, kw.get("merge", False), kw.get("longest"), 0, False)
