"""CPU suite for the anchored regular-expression search (bmx_compile_regex_anchored and the argument checks of the
bmx_*regex_anchored* entries): the compiler's output run through the oracle's automaton matcher against Python's ``re``
with re.MULTILINE on generated texts, the expressions it must refuse with both outputs untouched, a random family that it
has no reason to refuse, the identity with bmx_compile_regex, the symbols, and the argument errors that return before any
HIP call.  No compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import regex_anchored_oracle as ao
import regex_oracle as ro
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg
from test_regex_cpu import ERRORS as PLAIN_ERRORS

WORD, LINE = host.REGEX_WORD, host.REGEX_LINE

# (expression, flags, alphabet of the generated texts, a few planted strings)
MUST_COMPILE = [
    ("^ERROR", 0, b"ERO \n", [b"ERROR", b"\nERROR", b" ERROR"]),
    ("timeout$", 0, b"timeou \n", [b"timeout", b"timeout\n", b"timeout "]),
    ("^(ERROR|FATAL|PANIC): [0-9]{2,4}$", 0, b"ER: 12\n", [b"ERROR: 12", b"\nFATAL: 1234\n", b"PANIC: 12345", b"ERROR: 123\n"]),
    (r"\bcat\b", 0, b"cat_ .\n", [b"cat", b" cat.", b"_cat", b"cat\n", b"\ncat"]),
    (r"\<[A-Z][a-z]{1,8}\>", 0, b"Ab_ .\n", [b"Abb", b" Abbb.", b"AAb", b"\nAb\n"]),
    ("^a?b", 0, b"ab \n", [b"ab", b"\nb", b"aab"]),
    ("^a|b$", 0, b"ab \n", [b"a", b"b\n", b"\na", b"ab"]),
    (r"x\By", 0, b"xy_ .\n", [b"xy", b"x y"]),
    (r"foo\b bar", 0, b"fo bar\n", [b"foo bar", b"foo  bar"]),
    (r"\b[a-z.]x", 0, b"ax._ \n", [b"ax", b".x", b" .x", b"a.x", b"_ax"]),
    (r"[a-z.]{1,3}\b", 0, b"ab._ \n", [b"ab.", b"a. ", b".a_", b"..."]),
    ("(a|ab)(c|bcd)", WORD, b"abcd_ \n", [b"abcd", b" ac ", b"abc", b"_abcd", b"\nabcd\n"]),
    ("(a|ab)(c|bcd)", LINE, b"abcd_ \n", [b"abcd", b"\nac\n", b"\nabc", b"abcd\n", b"\nabcd\n"]),
    (r"(^|\b)a(y|$)", 0, b"axy \n", [b"a", b"xay", b" a\n"]),
    (r"(\<a|b\>)c?", 0, b"abc_ \n", [b"ac", b"b c", b"bc"]),
]
MUST_REFUSE = ["^*", r"\b?", "${2}", "^", "^$", r"\b", r"[a-z.]\b[a-z.]", r"a\bb", "(^)+", r"a\<{2}", r"^\>a", "a$b", "x^y"]


def _compile_raw(expr, flags):
    """(rc, re, an, both untouched?) through the C ABI, with a sentinel pattern in both outputs."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    re_, an = host.Regex(), host.RegexAnchors()
    C.memset(C.byref(re_), 0xA5, C.sizeof(re_))
    C.memset(C.byref(an), 0xA5, C.sizeof(an))
    rc = host.lib().bmx_compile_regex_anchored(e, len(e), flags, C.byref(re_), C.byref(an))
    untouched = bytes(re_) == b"\xa5" * C.sizeof(re_) and bytes(an) == b"\xa5" * C.sizeof(an)
    return rc, re_, an, untouched


def _texts(rng, alphabet, planted, count=6, max_len=96):
    """Texts of at most 96 bytes over the alphabet with the planted strings at offset 0, at the end, after two line breaks
    and in front of a trailing line break, and pure noise."""
    alphabet = np.frombuffer(alphabet, np.uint8)
    out = [b"", b"\n", b"\n\n"]
    for p in planted:
        out += [p, p + b"\n", b"\n\n" + p, p + p, b" " + p + b" " + p]
    for _ in range(count):
        body = rng.choice(alphabet, int(rng.integers(1, max_len))).tobytes()
        p = planted[int(rng.integers(0, len(planted)))]
        at = int(rng.integers(0, len(body)))
        out += [body, (p + body)[:max_len], (body + p)[-max_len:], (body[:at] + b"\n\n" + p + body[at:])[:max_len],
                (body + p + b"\n")[-max_len:]]
    return out


def _check_against_re(expr, flags, a, text, left=10, right=10):
    want = ao.matches_re(text, expr, flags, left, right)
    assert ao.simulate(text, a, left, right) == want, (expr, flags, text, left, right)
    ends, short, long_, starts, e_short, e_long = ao.lists_of(want)
    for longest, s_want in ((False, short), (True, long_)):
        e, s = ao.spans_numpy(text, a, left, right, longest)
        assert (e.tolist(), s.tolist()) == (ends, s_want), (expr, flags, text, longest)
    for longest, e_want in ((False, e_short), (True, e_long)):
        s, e = ao.begins_numpy(text, a, left, right, longest)
        assert (s.tolist(), e.tolist()) == (starts, e_want), (expr, flags, text, longest)
    return len(want)


@pytest.mark.parametrize("case", range(len(MUST_COMPILE)))
def test_must_compile_and_agree_with_re(built, case):
    expr, flags, alphabet, planted = MUST_COMPILE[case]
    rng = np.random.default_rng(0xA7C0 + case)
    re_, an = host.compile_regex_anchored(expr, flags)
    a = ao.from_lib(re_, an)
    assert 1 <= re_.min_len <= re_.max_len <= re_.m <= 64
    found = 0
    for text in _texts(rng, alphabet, planted):
        assert len(text) <= 96
        found += _check_against_re(expr, flags, a, text)
    assert found > 0, expr
    # the neighbour bytes: a line break, a word byte, another byte on either side
    for left in (10, ord("a"), ord(" ")):
        for right in (10, ord("a"), ord(" ")):
            for p in planted[:2]:
                _check_against_re(expr, flags, a, p, left, right)


def test_a_split_keeps_the_numbering_upward_and_the_classes_pure(built):
    re_, an = host.compile_regex_anchored(r"\b[a-z.]x")
    assert re_.m == 3 and re_.first == 0b011 and re_.last == 0b100  # [a-z], [.], x
    assert list(re_.follow)[:3] == [0b100, 0b100, 0]
    a = ao.from_lib(re_, an)
    assert a.rx.member[0].sum() == 26 and a.rx.member[1].sum() == 1 and a.rx.member[1][ord(".")]
    assert np.array_equal(a.before[0], ~ao.W) and np.array_equal(a.before[1], ao.W)
    assert a.after[2].all()
    re_, an = host.compile_regex_anchored(r"[a-z.]{1,3}\b")
    a = ao.from_lib(re_, an)
    assert re_.m == 6
    for i in range(6):
        assert (re_.last >> i) & 1
        word = bool(a.rx.member[i][ord("a")])
        assert a.rx.member[i].sum() == (26 if word else 1)
        assert np.array_equal(a.after[i], ~ao.W if word else ao.W)
        assert all(j > i for j in ro.bits(re_.follow[i]))
    # ^a?b: the gate stands on the way in through `first`, not on the edge a -> b
    re_, an = host.compile_regex_anchored("^a?b")
    a = ao.from_lib(re_, an)
    assert re_.m == 2 and re_.first == 0b11 and re_.follow[0] == 0b10
    assert a.before[0].sum() == 1 and a.before[0][10] and a.before[1].sum() == 1 and a.before[1][10]


@pytest.mark.parametrize("expr", MUST_REFUSE)
def test_must_refuse_with_the_outputs_untouched(built, expr):
    rc, _, _, untouched = _compile_raw(expr, 0)
    assert rc == host.ERR_ARG and untouched, expr
    assert host.lib().bmx_last_error().decode().startswith("bmx_compile_regex_anchored: "), expr


def test_every_error_of_the_plain_compiler(built):
    n = 0
    for expr, flags in PLAIN_ERRORS:
        if flags in (WORD, LINE):
            continue  # flag bits of this entry
        rc, _, _, untouched = _compile_raw(expr, flags)
        assert rc == host.ERR_ARG and untouched, (expr, flags)
        n += 1
    assert n >= 50
    rc, _, _, untouched = _compile_raw("abc", 16)
    assert rc == host.ERR_ARG and untouched
    L = host.lib()
    re_, an = host.Regex(), host.RegexAnchors()
    assert L.bmx_compile_regex_anchored(None, 0, 0, C.byref(re_), C.byref(an)) == host.ERR_ARG
    assert L.bmx_compile_regex_anchored(b"a", 1, 0, None, C.byref(an)) == host.ERR_ARG
    assert L.bmx_compile_regex_anchored(b"a", 1, 0, C.byref(re_), None) == host.ERR_ARG
    assert host.compile_regex_anchored(r"\^\$")[0].m == 2  # escaped: literals
    assert host.compile_regex_anchored(r"[$^\b]x")[0].m == 2  # inside a set: members
    with pytest.raises(host.BmxError) as e:
        host.compile_regex_anchored("x" * 32 + r"[a-z.]{32}\b")  # 64 positions, 65 once the last one is split
    assert host.compile_regex_anchored("x" * 32 + r"[a-z.]{31}\b")[0].m == 64
    assert e.value.rc == host.ERR_ARG


PREFIX = ["", "", "^", r"\b", r"\B", r"\<"]
SUFFIX = ["", "", "$", r"\b", r"\B", r"\>"]


def _random_anchored(rng, symbols):
    """regex_oracle.random_regex, each top-level alternative with an assertion in front of it and behind it, or none."""
    while True:
        expr, _ = ro.random_regex(rng, symbols, 8)
        alts, depth, at = [], 0, 0
        for i, ch in enumerate(expr):  # (every byte of the expression is spelt \xHH, so ( ) | [ ] are syntax)
            if ch == "[":
                depth += 100
            elif ch == "]":
                depth -= 100
            elif ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
            elif ch == "|" and depth == 0:
                alts.append(expr[at:i])
                at = i + 1
        alts.append(expr[at:])
        if all(alts):
            pre = [PREFIX[int(rng.integers(0, 6))] for _ in alts]
            suf = [SUFFIX[int(rng.integers(0, 6))] for _ in alts]
            return "|".join(p + alt + s for p, alt, s in zip(pre, alts, suf)), sum(map(bool, pre + suf))


def test_random_family_is_never_refused_and_agrees_with_re(built):
    rng = np.random.default_rng(0xA7C1)
    symbols = np.frombuffer(b"ab_ .\n", np.uint8)
    refused, matched, anchored = [], 0, 0
    for case in range(250):
        expr, n_assertions = _random_anchored(rng, symbols)
        rc, re_, an, _ = _compile_raw(expr, 0)
        if rc != host.OK:
            refused.append((expr, host.lib().bmx_last_error().decode()))
            continue
        anchored += n_assertions > 0
        a = ao.from_lib(re_, an)
        for _ in range(2):
            text = rng.choice(symbols, int(rng.integers(0, 40))).tobytes()
            matched += _check_against_re(expr, 0, a, text) > 0
    assert not refused, refused  # a refusal is a failure: this family gives the compiler no reason
    assert matched >= 100 and anchored >= 150, (matched, anchored)


def test_identity_without_assertions(built):
    rng = np.random.default_rng(0xA7C2)
    symbols = np.arange(97, 101)
    exprs = ["(ERROR|FATAL|PANIC): [0-9]{2,4}", "a", "x{64}", "(a?b?){2}c", r"\^\$", "[^\\x00-\\xff]a|b"]
    exprs += [ro.random_regex(rng, symbols, 20)[0] for _ in range(100)]
    for expr in exprs:
        for flags in (0, host.CLASS_ICASE):
            rc, re_, an, _ = _compile_raw(expr, flags)
            assert rc == host.OK, expr
            assert bytes(re_) == bytes(host.compile_regex(expr, flags)), expr
            assert bytes(an) == b"\xff" * C.sizeof(an), expr


def test_symbols_constants_and_struct_layout(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    names = ("bmx_compile_regex_anchored", "bmx_search_regex_anchored_device", "bmx_regex_anchored_starts_device",
             "bmx_search_regex_anchored_begins_device", "bmx_regex_anchored_ends_device", "bmx_search_regex_anchored",
             "bmx_search_regex_anchored_spans", "bmx_search_regex_anchored_begins", "bmx_search_regex_anchored_begins_spans",
             "bmx_last_regex_anchored_ms", "bmx_last_regex_anchored_begins_ms")
    for name in names:
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("compile_regex_anchored", "search_regex_anchored", "RegexAnchors", "REGEX_WORD", "REGEX_LINE"):
        assert getattr(pkg, name) is getattr(host, name)
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert int(re.search(r"#define BMX_REGEX_WORD (\d+)u", src).group(1)) == WORD == ao.WORD == 4
    assert int(re.search(r"#define BMX_REGEX_LINE (\d+)u", src).group(1)) == LINE == ao.LINE == 8
    A = host.RegexAnchors
    assert (A.before.offset, A.after.offset, C.sizeof(A)) == (0, 2048, 4096)
    assert bytes(A.full()) == b"\xff" * 4096


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    r, an = host.compile_regex_anchored(r"^(a|bc)d\b")
    p, q = C.byref(r), C.byref(an)
    bad = host.compile_regex("(a|bc)d")
    bad.follow[3] = 1
    b = C.byref(bad)
    for fn in (L.bmx_search_regex_anchored, L.bmx_search_regex_anchored_begins):
        assert fn(None, text, len(text), None, q, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), p, None, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), b, q, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), p, q, None, 8, C.byref(total)) == host.ERR_ARG  # a capacity needs room
        assert fn(None, None, len(text), p, q, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, 1 << 40, p, q, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, 0, p, q, out, 8, C.byref(total)) == host.OK and total.value == 0
    for fn in (L.bmx_search_regex_anchored_spans, L.bmx_search_regex_anchored_begins_spans):
        assert fn(None, text, len(text), None, q, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), p, None, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), b, q, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), p, q, 0, None, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), p, q, 0, out, None, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, None, len(text), p, q, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
        assert fn(None, text, len(text), p, q, 2, out, out, 8, C.byref(total)) == host.ERR_ARG  # an unknown flag bit
        assert fn(None, text, 1 << 40, p, q, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    for dev in (L.bmx_search_regex_anchored_device, L.bmx_search_regex_anchored_begins_device):
        assert dev(None, None, 10, 0, 0, None, q, 10, 10, None, 0, C.byref(total), None) == host.ERR_ARG
        assert dev(None, None, 10, 0, 0, p, None, 10, 10, None, 0, C.byref(total), None) == host.ERR_ARG
        assert dev(None, None, 10, 0, 0, b, q, 10, 10, None, 0, C.byref(total), None) == host.ERR_ARG
        assert dev(None, None, 10, 11, 0, p, q, 10, 10, None, 0, C.byref(total), None) == host.ERR_ARG  # lead / tail > n
        assert dev(None, None, 1 << 40, 0, 0, p, q, 10, 10, None, 0, C.byref(total), None) == host.ERR_ARG
        assert dev(None, None, 10, 0, 0, p, q, 256, 10, None, 0, C.byref(total), None) == host.ERR_ARG  # left is a byte
        assert dev(None, None, 10, 0, 0, p, q, 10, 256, None, 0, C.byref(total), None) == host.ERR_ARG  # right is a byte
        assert dev(None, None, 10, 0, 0, p, q, 10, 10, None, 8, C.byref(total), None) == host.ERR_ARG  # capacity, no list
        assert dev(None, None, 10, 0, 0, p, q, 10, 10, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    st = L.bmx_regex_anchored_starts_device
    assert st(None, None, 10, 0, None, q, 10, 10, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, None, 10, 10, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, b, q, 10, 10, out, 0, 0, out, None) == host.ERR_ARG  # even with count == 0
    assert st(None, None, 10, 0, p, q, 10, 10, out, 8, 2, out, None) == host.ERR_ARG  # an unknown flag bit
    assert st(None, None, 1 << 40, 0, p, q, 10, 10, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, q, 300, 10, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, q, 10, 300, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, q, 10, 10, None, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, q, 10, 10, out, 8, 0, None, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, q, 10, 10, out, 8, host.REGEX_LONGEST, out, None) == host.ERR_ARG  # no context
    assert st(None, None, 10, 0, p, q, 10, 10, None, 0, 0, None, None) == host.OK  # count == 0: nothing to do
    en = L.bmx_regex_anchored_ends_device
    assert en(None, None, 10, 0, None, q, 10, 10, out, 8, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, None, 10, 10, out, 8, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, b, q, 10, 10, out, 0, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, q, 10, 10, out, 8, None, 2, out, None) == host.ERR_ARG
    assert en(None, None, 1 << 40, 0, p, q, 10, 10, out, 8, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, q, 256, 10, out, 8, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, q, 10, 256, out, 8, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, q, 10, 10, None, 8, None, 0, out, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, q, 10, 10, out, 8, None, 0, None, None) == host.ERR_ARG
    assert en(None, None, 10, 0, p, q, 10, 10, out, 8, None, 0, out, None) == host.ERR_ARG  # no context
    assert en(None, None, 10, 0, p, q, 10, 10, None, 0, None, 0, None, None) == host.OK
    assert L.bmx_last_regex_anchored_ms(None) < 0 and L.bmx_last_regex_anchored_begins_ms(None) < 0
