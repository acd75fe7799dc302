"""GPU suite of the capture groups pass and the template expansion (bmx_regex_groups_device, bmx_search_regex_groups,
bmx_expand_device, bmx_expand, kind "regex_groups" of sub / findall) against tests/regex_groups_oracle.py and Python's
``re``: list lengths around the wave and the workgroup, spans of one byte and of the full column of 64, the 64-position /
16-group expression, a view at an odd address with a base offset and spans on its first and last byte, skipped entries,
the three errors of the status word, a random differential, a caller's non-blocking stream; the expansion against
``re.sub`` / ``Match.expand`` for every shape of piece (empty literal, empty group, unset group, adjacent matches, a
match on the first and on the last byte, more than one tile of output), its capacity rules and its list check; sub and
findall end to end."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import regex_groups_oracle as go
import stream_cases as sc
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def text_dev(text: bytes, front: int = 0):
    """The text on the device, `front` bytes into its allocation (an odd address for an odd `front`)."""
    import torch

    buf = torch.zeros(front + len(text) + 64, dtype=torch.uint8, device="cuda")
    buf[front:front + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return buf[front:front + len(text)]


def regs_of(expr, text: bytes, spans, base: int = 0) -> np.ndarray:
    """[count, G + 1, 2] by Python's re: fullmatch on every span (s, e inclusive; -1 rows for a skipped one)."""
    pattern = re.compile(expr.encode() if isinstance(expr, str) else expr, re.DOTALL)
    out = np.full((len(spans), pattern.groups + 1, 2), -1, np.int64)
    for i, (s, e) in enumerate(spans):
        if s < 0 or e < s:
            continue
        mt = pattern.fullmatch(text, s, e + 1)
        assert mt is not None, (expr, s, e)
        r = np.asarray(mt.regs, np.int64)
        out[i] = np.where(r >= 0, r + base, -1)
    return out


def all_spans(expr, text: bytes):
    """Every (s, e) with text[s..e] a match, by brute force over Python's re (short texts only)."""
    pattern = re.compile(expr.encode(), re.DOTALL)
    return [(s, e) for e in range(len(text)) for s in range(max(0, e - 63), e + 1) if pattern.fullmatch(text, s, e + 1)]


def groups_dev(ctx, d_text, pair, spans, **kw) -> np.ndarray:
    s = dev(np.asarray([a for a, _ in spans], np.int64))
    e = dev(np.asarray([b for _, b in spans], np.int64))
    return ctx.regex_groups_device(d_text, pair, s, e, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def abcd():
    rng = np.random.default_rng(0xABCD)
    text = rng.choice(np.frombuffer(b"abcd", np.uint8), 6000, p=[0.35, 0.3, 0.2, 0.15]).tobytes()
    expr = "(a|ab)(c|bcd)(d?)"
    spans = all_spans(expr, text)
    assert len(spans) >= 257
    return expr, text, spans


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_list_lengths_around_the_wave_and_the_workgroup(ctx, abcd, count):
    expr, text, spans = abcd
    pair = host.compile_regex_groups(expr)
    got = groups_dev(ctx, text_dev(text), pair, spans[:count])
    assert got.shape == (count, 4, 2) and np.array_equal(got, regs_of(expr, text, spans[:count]))
    model = go.Model.from_library(*pair)
    for i in (0, count - 1):
        assert tuple(map(tuple, got[i])) == go.walk(model, text, *spans[i])
    assert ctx.last_regex_groups_ms() >= 0.0


def test_spans_of_one_byte_and_of_the_full_column(ctx):
    rng = np.random.default_rng(64)
    text = rng.choice(np.frombuffer(b"ab", np.uint8), 400).tobytes()
    d_text = text_dev(text)
    one = "(a)|(b)"
    spans = [(i, i) for i in range(len(text))]
    assert np.array_equal(groups_dev(ctx, d_text, one, spans), regs_of(one, text, spans))
    full = "([ab])([ab]{62})([ab])"  # 64 positions, every span 64 bytes: the whole column of a lane
    re_, gr = host.compile_regex_groups(full)
    assert (re_.m, re_.min_len, re_.max_len) == (64, 64, 64)
    spans = [(i, i + 63) for i in range(len(text) - 63)]
    assert np.array_equal(groups_dev(ctx, d_text, (re_, gr), spans), regs_of(full, text, spans))
    # 34 positions, spans of 4..34 bytes along many paths: the preferred one is the backtracking matcher's
    opt = "(a?)(b?)" + "(?:a?b?)" * 14 + "([ab]{4})"
    spans = [(i, i + n - 1) for i in range(0, 300, 7) for n in (4, 5, 11, 17) if re.fullmatch(opt.encode(), text[i:i + n])]
    assert len(spans) >= 20
    assert np.array_equal(groups_dev(ctx, d_text, opt, spans), regs_of(opt, text, spans))


def test_the_64_position_16_group_expression(ctx):
    rng = np.random.default_rng(16)
    parts = [go.wide_text(rng) for _ in range(300)]
    text = b"#".join(parts)
    spans, at = [], 0
    for p in parts:
        spans.append((at, at + len(p) - 1))
        at += len(p) + 1
    pair = host.compile_regex_groups(go.WIDE)
    assert pair[0].m == 64 and pair[1].n_groups == 16
    got = groups_dev(ctx, text_dev(text), pair, spans)
    assert got.shape == (300, 17, 2) and np.array_equal(got, regs_of(go.WIDE, text, spans))


def test_view_edges_odd_address_base_offset_and_skipped_entries(ctx, abcd):
    expr = "(a|ab)(c|bcd)(d?)"
    text = b"abcd" + abcd[1][:500] + b"xacd"  # a match on the view's first byte and one on its last
    n, base = len(text), 1000003
    inner = all_spans(expr, text)
    assert inner[0][0] == 0 and inner[-1][1] == n - 1
    for front in (1, 7, 16):
        d_text = text_dev(text, front)
        spans = [(s + base, e + base) for s, e in inner]
        # skipped: a start or an end of -1, an end below its start
        spans[3:3] = [(-1, 5 + base), (5 + base, -1), (-1, -1), (9 + base, 8 + base)]
        got = groups_dev(ctx, d_text, expr, spans, base_offset=base)
        want = regs_of(expr, text, [(s - base, e - base) if s >= 0 and e >= s else (-1, -1) for s, e in spans], base)
        assert np.array_equal(got, want), front
        assert (got[3:7] == -1).all()


def test_status_word_errors(ctx, abcd):
    expr, text, spans = abcd
    d_text = text_dev(text[:200])
    good = [sp for sp in spans if sp[1] < 200][:10]
    groups_dev(ctx, d_text, expr, good)
    never = next((s, s) for s in range(200) if (s, s) not in spans)
    for bad, what in ((never, "no match"), ((198, 201), "outside the view"), ((10, 10 + 64), "longer than"),
                      ((10, 17), "longer than")):
        with pytest.raises(host.BmxError) as err:
            groups_dev(ctx, d_text, expr, good[:5] + [bad] + good[5:])
        assert err.value.rc == host.ERR_ARG and what in str(err.value), (bad, str(err.value))
    with pytest.raises(host.BmxError):  # below the view's base
        groups_dev(ctx, d_text, expr, [(5, 8)], base_offset=6)
    assert np.array_equal(groups_dev(ctx, d_text, expr, good), regs_of(expr, text, good))  # the word starts clean again
    empty = ctx.regex_groups_device(d_text, expr, dev(np.zeros(0, np.int64)), dev(np.zeros(0, np.int64)))
    assert tuple(empty.shape) == (0, 4, 2)


def test_random_differential_through_the_host_entry(ctx):
    """About 200 random expressions: every match end of a random text with its shortest and with its longest start
    (bmx_search_regex_groups), the groups against re.fullmatch and against the oracle's walker."""
    rng = np.random.default_rng(200)
    done = spans_seen = 0
    while done < 200:
        expr = go.random_expr(rng)
        try:
            pair = host.compile_regex_groups(expr)
        except host.BmxError:
            continue
        done += 1
        text = rng.choice(np.frombuffer(b"abc", np.uint8), 160).tobytes()
        model = go.Model.from_library(*pair)
        for posix in (False, True):
            starts, ends, groups = ctx.search_regex_groups(text, pair, posix=posix)
            spans = list(zip(starts.astype(np.int64).tolist(), ends.astype(np.int64).tolist()))
            assert np.array_equal(groups, regs_of(expr, text, spans)), (expr, posix)
            for i in range(0, len(spans), 9):
                assert tuple(map(tuple, groups[i])) == go.walk(model, text, *spans[i]), (expr, spans[i])
            spans_seen += len(spans)
    assert spans_seen >= 5000


@functools.lru_cache(maxsize=None)
def delay_scratch():
    import torch

    return torch.zeros(2 * sc.DELAY_BYTES, dtype=torch.uint8, device="cuda")


def behind_a_pending_copy(buf, real, what):
    """On a fresh non-blocking stream: a long delay, then the copy of `real` over `buf` (which holds a decoy); returns the
    stream with the copy still outstanding (asserted)."""
    import torch

    s = torch.cuda.Stream()
    scratch = delay_scratch()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i in range(sc.DELAY_COPIES):
            a, b = (0, sc.DELAY_BYTES) if i & 1 else (sc.DELAY_BYTES, 0)
            scratch[a:a + sc.DELAY_BYTES].copy_(scratch[b:b + sc.DELAY_BYTES], non_blocking=True)
        buf.copy_(real, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
    assert not pending.query(), f"{what}: the producer had finished before the call"
    return s


def test_both_entries_on_a_callers_stream_behind_a_pending_copy(ctx, abcd):
    import torch

    expr, text, spans = abcd
    spans = spans[:300]
    real = dev(np.asarray([s for s, _ in spans], np.int64))
    ends = dev(np.asarray([e for _, e in spans], np.int64))
    starts = torch.full_like(real, -1)  # the decoy: every entry skipped
    d_text = text_dev(text)
    stream = behind_a_pending_copy(starts, real, "groups")
    got = ctx.regex_groups_device(d_text, expr, starts, ends, stream=stream)
    want = regs_of(expr, text, spans)
    assert np.array_equal(got.cpu().numpy(), want)
    # the expansion reads the groups that the pending copy brings
    disjoint = [i for i in range(len(spans)) if i == 0 or spans[i][0] > max(e for _, e in spans[:i])]
    g_real = dev(want[disjoint])
    g = torch.full_like(g_real, -1)
    stream = behind_a_pending_copy(g, g_real, "expand")
    out, n_out = ctx.expand_device(d_text, g, "<\\2|\\1>", stream=stream)
    assert out.cpu().numpy().tobytes() == expand_want(text, want[disjoint], b"<\\2|\\1>")[0]


# ---- the expansion ----

def expand_want(text: bytes, groups: np.ndarray, tmpl: bytes):
    """(the text with every match replaced, the expansions) from the group table alone (view coordinates): what re.sub
    and Match.expand do with a template of this subset."""
    t, lits = host.compile_template(tmpl, groups.shape[1] - 1)
    lit = [lits[t.lit_off[r]:t.lit_off[r] + t.lit_len[r]] for r in range(t.n_refs + 1)]
    out, column, at = [], [], 0
    for g in groups:
        x = b""
        for r in range(t.n_refs):
            b, e = g[t.ref[r]]
            x += lit[r] + (text[b:e] if b >= 0 else b"")
        x += lit[t.n_refs]
        out += [text[at:g[0][0]], x]
        column.append(x)
        at = g[0][1]
    return b"".join(out) + text[at:], column


def finditer_groups(expr: bytes, text: bytes) -> np.ndarray:
    pattern = re.compile(expr, re.DOTALL)
    return np.asarray([mt.regs for mt in pattern.finditer(text)], np.int64).reshape(-1, pattern.groups + 1, 2)


DATE = rb"([0-9]{4})-([0-9]{2})-([0-9]{2})"


@pytest.fixture(scope="module")
def dates():
    """About 48 KiB (three tiles of output): dates among filler, some adjacent, one on the first and one on the last byte."""
    rng = np.random.default_rng(2026)
    parts = [b"2026-10-21"]
    for i in range(2400):
        parts.append(rng.choice(np.frombuffer(b"abc xyz,.\n", np.uint8), int(rng.integers(0, 24))).tobytes())
        for _ in range(1 + (i % 5 == 0)):  # adjacent matches
            parts.append(b"%04d-%02d-%02d" % (int(rng.integers(0, 10000)), int(rng.integers(1, 13)), int(rng.integers(1, 29))))
    text = b"".join(parts)
    assert re.match(DATE, text) and re.search(DATE + b"$", text) and len(text) > 40000
    return text


@pytest.mark.parametrize("tmpl", [rb"\3.\2.\1", rb"\1\2", rb"\2\2\g<0>\\", b"", b"--", rb"[\g<0>]", rb"\1" * 32, rb"x\3"])
def test_expand_dates_against_re_sub_and_expand(ctx, dates, tmpl):
    groups = finditer_groups(DATE, dates)
    d_text, g = text_dev(dates, 3), dev(groups)
    out, n_out = ctx.expand_device(d_text, g, tmpl)
    want = re.sub(DATE, tmpl, dates)
    assert n_out == len(want) and out.cpu().numpy().tobytes() == want
    blob, off = ctx.expand_device(d_text, g, tmpl, extract=True)
    column = [mt.expand(tmpl) for mt in re.finditer(DATE, dates)]
    assert blob.cpu().numpy().tobytes() == b"".join(column)
    assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(x) for x in column])]))
    assert expand_want(dates, groups, tmpl) == (want, column)


def test_a_template_without_a_reference_gives_replace_devices_bytes(ctx, dates):
    groups = finditer_groups(DATE, dates)
    d_text = text_dev(dates)
    for lit in (b"", b"#", b"<redacted date>"):
        a, na = ctx.expand_device(d_text, dev(groups), lit)
        b, nb = ctx.replace_device(d_text, dev(groups[:, 0, 0]), dev(groups[:, 0, 1] - 1), lit)
        assert na == nb and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("expr,tmpl", [(rb"(a)?b", rb"[\1]"), (rb"(a?)b", rb"[\1]"), (rb"(a)?(b)?c", rb"\2\1"), (rb"(a|(b))(c?)", rb"\3\2\1\3"),
                                       (rb"()(a)()", rb"\1\2\3x\1")])
def test_unset_and_empty_groups(ctx, expr, tmpl):
    rng = np.random.default_rng(len(expr))
    text = rng.choice(np.frombuffer(b"abc", np.uint8), 3000).tobytes()
    groups = finditer_groups(expr, text)
    assert (groups[:, 1:, 0] == -1).any() or (groups[:, 1:, 0] == groups[:, 1:, 1]).any()
    d_text = text_dev(text, 1)
    out, _ = ctx.expand_device(d_text, dev(groups), tmpl)
    assert out.cpu().numpy().tobytes() == re.sub(expr, tmpl, text)
    blob, off = ctx.expand_device(d_text, dev(groups), tmpl, extract=True)
    column = [mt.expand(tmpl) for mt in re.finditer(expr, text)]
    assert blob.cpu().numpy().tobytes() == b"".join(column) and off.cpu().numpy()[-1] == len(blob)


@pytest.mark.parametrize("count", [1, 257])
def test_extract_offsets_base_offset_and_output_alignment(ctx, dates, count):
    import torch

    base = 777
    groups = finditer_groups(DATE, dates)[:count]
    d_text = text_dev(dates, 5)
    want, column = expand_want(dates, groups, rb"\3/\2")
    for front in (0, 1, 15):
        buf = torch.zeros(len(dates) + 64, dtype=torch.uint8, device="cuda")
        out, n_out = ctx.expand_device(d_text, dev(groups + base), rb"\3/\2", base_offset=base, out=buf[front:])
        assert n_out == len(want) and out.cpu().numpy().tobytes() == want
        blob, off = ctx.expand_device(d_text, dev(groups + base), rb"\3/\2", extract=True, base_offset=base, out=buf[front:])
        assert blob.cpu().numpy().tobytes() == b"".join(column) and off.numel() == count + 1
        assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(x) for x in column])]))


def test_capacity_rules_and_the_list_check(ctx, dates):
    import torch

    L = ctx._L
    groups = finditer_groups(DATE, dates)[:40]
    tmpl = rb"\3.\2.\1!"
    want, column = expand_want(dates, groups, tmpl)
    d_text, g = text_dev(dates), dev(groups)
    total = C.c_uint64(0)
    off = torch.zeros(41, dtype=torch.int64, device="cuda")
    out = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda")
    call = lambda flags, cap, gg=g: L.bmx_expand_device(ctx._h, d_text.data_ptr(), len(dates), 0, gg.data_ptr(), 3, gg.shape[0], tmpl, len(tmpl),
                                                        flags, out.data_ptr() if cap else None, cap, off.data_ptr() if flags else None,
                                                        C.byref(total), None)
    assert call(0, 0) == host.OK and total.value == len(want)                     # capacity 0 counts
    assert call(0, 100) == host.ERR_CAPACITY and total.value == len(want)         # the lowest 100 bytes
    assert out[:100].cpu().numpy().tobytes() == want[:100] and int(out[100]) == 0
    assert call(0, len(want)) == host.OK and out[:len(want)].cpu().numpy().tobytes() == want
    assert call(1, 0) == host.OK and total.value == sum(map(len, column))         # the offsets always come, all of them
    assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(x) for x in column])]))
    assert call(1, 7) == host.ERR_CAPACITY and out[:7].cpu().numpy().tobytes() == b"".join(column)[:7]
    for bad in (groups[::-1].copy(), np.concatenate([groups[:3], groups[2:]]), groups - 1 - groups[0, 0, 0]):  # descending; twice; below the view
        assert call(0, 0, dev(bad)) == host.ERR_ARG
    unset = groups.copy()
    unset[5, 0] = -1
    outside = groups.copy()
    outside[7, 2, 1] = outside[7, 0, 1] + 1  # a group that reaches past its match
    for bad in (unset, outside):
        with pytest.raises(host.BmxError) as err:
            ctx.expand_device(d_text, dev(bad), tmpl)
        assert err.value.rc == host.ERR_ARG
    past = groups.copy()
    past[-1, 0, 1] = len(dates) + 1
    assert call(0, 0, dev(past)) == host.ERR_ARG
    # no match at all: the text itself, or the single offset 0
    none = torch.zeros((0, 4, 2), dtype=torch.int64, device="cuda")
    same, n_same = ctx.expand_device(d_text, none, tmpl)
    assert n_same == len(dates) and same.cpu().numpy().tobytes() == dates
    blob, off0 = ctx.expand_device(d_text, none, tmpl, extract=True)
    assert blob.numel() == 0 and off0.cpu().numpy().tolist() == [0]


def test_host_buffer_entry(ctx, dates):
    L = ctx._L
    groups = np.ascontiguousarray(finditer_groups(DATE, dates)[:100]).view(np.uint64)
    tmpl = rb"\2/\3/\1"
    want, column = expand_want(dates, groups.view(np.int64), tmpl)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    total = C.c_uint64(0)
    out = np.zeros(len(want), np.uint8)
    assert L.bmx_expand(ctx._h, dates, len(dates), ptr(groups), 3, 100, tmpl, len(tmpl), 0, ptr(out), out.size, None, C.byref(total)) == host.OK
    assert total.value == len(want) and out.tobytes() == want
    off = np.zeros(101, np.uint64)
    assert L.bmx_expand(ctx._h, dates, len(dates), ptr(groups), 3, 100, tmpl, len(tmpl), 1, ptr(out), 50, ptr(off), C.byref(total)) == host.ERR_CAPACITY
    assert total.value == sum(map(len, column)) and out[:50].tobytes() == b"".join(column)[:50] and off[-1] == total.value


# ---- end to end ----

def test_sub_and_findall_on_dates(ctx, dates):
    expr = DATE.decode()
    assert host.sub(dates, expr, r"\3.\2.\1", kind="regex_groups") == re.sub(DATE, rb"\3.\2.\1", dates)
    assert host.sub(dates, expr, r"\3.\2.\1", kind="regex_groups", posix=True) == re.sub(DATE, rb"\3.\2.\1", dates)
    assert host.findall(dates, expr, kind="regex_groups") == re.findall(DATE, dates)
    one = rb"[0-9]{4}-([0-9]{2})-[0-9]{2}"
    assert host.findall(dates, one.decode(), kind="regex_groups") == re.findall(one, dates)   # one group: strings
    none = rb"[0-9]{4}-(?:[0-9]{2})-[0-9]{2}"
    assert host.findall(dates, none.decode(), kind="regex_groups") == re.findall(none, dates)  # no group: the matches
    assert host.sub(b"2026-10-21", r"(..)(..)", r"\2\1", kind="regex_groups") == re.sub(rb"(..)(..)", rb"\2\1", b"2026-10-21")


def test_sub_and_findall_posix_on_log_lines(ctx):
    rng = np.random.default_rng(404)
    lines = []
    for i in range(3000):
        level = [b"ERROR", b"FATAL", b"INFO", b"WARN"][int(rng.integers(0, 4))]
        lines.append(b"%s: %d %s" % (level, int(rng.integers(10, 10000)), [b"disk", b"net;", b"(cpu)"][i % 3]))
    text = b"\n".join(lines) + b"\n"
    expr = rb"(ERROR|FATAL): ([0-9]{2,4})"
    assert host.findall(text, expr.decode(), kind="regex_groups", posix=True) == re.findall(expr, text)
    assert host.sub(text, expr.decode(), r"\2=\1", kind="regex_groups", posix=True) == re.sub(expr, rb"\2=\1", text)
    assert host.findall(text, expr.decode(), kind="regex_groups", posix=True, rows=True) == re.findall(expr, text)
    starts, ends, groups = host.search_regex_groups(text, expr.decode(), posix=True)
    first = re.search(expr, text)
    i = int(np.flatnonzero(ends == first.end() - 1)[0])
    assert tuple(map(tuple, groups[i])) == first.regs and starts[i] == first.start()


def test_rows_keep_matches_that_cross_a_line_break_out(ctx):
    rng = np.random.default_rng(10)
    words = [b"abxcd", b"ab\ncd", b"ab cd", b"zz", b"\n", b"cdab", b"ab"]
    text = b"".join(words[int(rng.integers(0, len(words)))] for _ in range(4000))
    expr, tmpl = rb"(ab)(.)(cd)", rb"\3\2\1"
    assert b"ab\ncd" in text
    assert host.sub(text, expr.decode(), tmpl.decode(), kind="regex_groups") == re.sub(expr, tmpl, text, flags=re.DOTALL)
    assert host.sub(text, expr.decode(), tmpl.decode(), kind="regex_groups", rows=True) == re.sub(expr, tmpl, text)
    assert host.findall(text, expr.decode(), kind="regex_groups", rows=True) == re.findall(expr, text)
    for kw in ({"merge": True}, {"longest": True}):
        with pytest.raises(ValueError):
            host.sub(text, expr.decode(), tmpl.decode(), kind="regex_groups", **kw)


def test_the_driver(ctx, dates, tmp_path):
    import os
    import subprocess

    from conftest import ROOT

    text = dates[:6000] + b"\n"
    path = tmp_path / "dates.txt"
    path.write_bytes(text)
    exe = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")

    def cli(*args, code=0):
        out = subprocess.run([exe, "--text", str(path)] + list(args), capture_output=True, timeout=120)
        assert out.returncode == code, out.stderr
        return out.stdout

    expr = DATE.decode()
    assert cli("--regex-groups", expr, "--replace", r"\3.\2.\1") == re.sub(DATE, rb"\3.\2.\1", text)
    assert cli("--regex-groups", expr, "--replace", r"\3.\2.\1", "--posix", "--lines") == re.sub(DATE, rb"\3.\2.\1", text)
    column = [mt.expand(rb"\2/\1") for mt in re.finditer(DATE, text)]
    assert cli("--regex-groups", expr, "--only-matching", "--template", r"\2/\1", "--max-print", "100000") == b"".join(x + b"\n" for x in column)
    whole = [mt.group(0) for mt in re.finditer(DATE, text)]
    assert cli("--regex-groups", expr, "--only-matching", "--max-print", "100000") == b"".join(x + b"\n" for x in whole)
    lines = cli("--regex-groups", expr, "--spans", "--max-print", "3").decode().splitlines()
    first = re.search(DATE, text)
    assert lines[0].split("\t") == [str(first.start()), str(first.end() - 1)] + ["%d,%d" % first.span(g) for g in (1, 2, 3)]
    assert lines[3].startswith("matches with groups: %d " % len(whole))
    cli("--regex-groups", expr, code=2)
    cli("--regex-groups", expr, "--replace", "x", "--merge", code=2)
    cli("--regex", expr, "--only-matching", "--template", "x", code=2)
    cli("--regex-groups", "(a?){2}b", "--replace", "x", code=1)
    cli("--regex-groups", expr, "--replace", r"\4", code=1)
