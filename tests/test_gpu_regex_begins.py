"""GPU suite of the begins search (bmx_search_regex_begins_device), the ends pass (bmx_regex_ends_device) and the
leftmost-longest route of sub / findall (posix=True), against regex_begins_oracle.py: begins_numpy everywhere,
begins_brute where the text has 64 bytes or fewer, posix_matches end to end.

The geometry case forces lanes of 16 starts through libbmx_exp.so's "regex_begins_piece_shift" (the shared
"tile_piece_shift" begins at 6, which the same test sets as well) with "tile_max_grid" = 2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import regex_begins_oracle as bo
import regex_oracle as ro
import subst_oracle as so
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

LOG = "(ERROR|FATAL|PANIC): [0-9]{2,4}"
ORF = "GATTACAGATTACAGATTAC" + "ATG([ACGT]{3}){2,4}(TAA|TAG|TGA)"
CLS40 = "[AC][CG][GT][AT]" * 10
LITERAL = "needle in the hay"


def _dev(data, first: int = 0, behind: bytes = b""):
    """A view at alignment ``first`` (mod 16) of a device buffer that goes on with ``behind``."""
    import torch

    data = bytes(data)
    buf = torch.from_numpy(np.frombuffer(b"\x00" * first + data + behind + b"\x00" * 16, np.uint8).copy()).cuda()
    view = buf[first:first + len(data)]
    assert len(data) == 0 or view.data_ptr() % 16 == first % 16
    return view


def _begins(ctx, d_text, rx, **kw):
    re_ = rx if isinstance(rx, host.Regex) else bo.struct_of(rx)
    n = kw.get("n", d_text.numel())
    cap = kw.pop("capacity", max(n, 1))
    starts, total = ctx.search_regex_begins_device(d_text, re_, capacity=cap, **kw)
    return starts.cpu().numpy().astype(np.int64), total


def _check(ctx, text, expr_or_rx, first=0, behind=b"", what=None):
    """Begins search and both ends passes on one text against the oracles."""
    rx = ro.parse(expr_or_rx) if isinstance(expr_or_rx, str) else expr_or_rx
    text = bytes(text)
    want_s, want_short, want_long = bo.begins_numpy(text, rx)
    if len(text) <= 64 and isinstance(expr_or_rx, str):
        assert bo.begins_brute(text, expr_or_rx) == (want_s.tolist(), want_short.tolist(), want_long.tolist()), what
    d_text = _dev(text, first, behind)
    got, total = _begins(ctx, d_text, rx)
    assert total == want_s.size and np.array_equal(got, want_s), (what, total, want_s.size)
    if total:
        import torch

        d_s = torch.from_numpy(want_s).cuda()
        re_ = bo.struct_of(rx)
        assert np.array_equal(ctx.regex_ends_device(d_text, re_, d_s).cpu().numpy(), want_short), what
        assert np.array_equal(ctx.regex_ends_device(d_text, re_, d_s, longest=True).cpu().numpy(), want_long), what
    return want_s


def _random_pairs(count, seed, max_len=40, max_m=10):
    rng = np.random.default_rng(seed)
    for case in range(count):
        symbols = np.arange(97, 97 + (2 if case % 2 else 4))
        text = rng.choice(symbols, int(rng.integers(1, max_len + 1))).astype(np.uint8).tobytes()
        expr, rx = ro.random_regex(rng, symbols, max_m)
        yield text, expr, rx


# ---- the begins search -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 4097])
def test_view_sizes(ctx, n):
    rng = np.random.default_rng(n)
    hits = 0
    for case in range(8):
        symbols = np.arange(97, 99 + case % 2)
        expr, rx = ro.random_regex(rng, symbols, 10)
        text = rng.choice(symbols, n).astype(np.uint8).tobytes()
        hits += _check(ctx, text, expr, what=(n, expr)).size
    assert hits > 0


def test_every_alignment_and_every_length_mod_16(ctx):
    """All 16 alignments of d_text x all 16 values of n mod 16, each view cut out of one long text of the same alphabet:
    the bytes behind the view would complete matches, and the chunk of the view's last byte is where this kernel is new."""
    rng = np.random.default_rng(0xA116)
    symbols = np.arange(97, 99)
    back = rng.choice(symbols, 256).astype(np.uint8).tobytes()
    cases = [ro.random_regex(rng, symbols, 10) for _ in range(3)] + [("ab{1,3}a", ro.parse("ab{1,3}a"))]
    cut = 0
    for first in range(16):
        for r in range(16):
            n = 32 + r + 16 * (first % 3)
            for expr, rx in cases:
                want = _check(ctx, back[:n], expr, first=first, behind=back[n:], what=(first, n, expr))
                cut += int((bo.begins_numpy(back[:n + rx.max_len], rx)[0] < n).sum()) > want.size  # a start the cut took away
    assert cut > 50


def test_a_match_cut_by_the_view_end_is_absent(ctx):
    text = b"xx ERROR: 12 yy ERROR: 1"
    for first in range(16):
        for keep, want in ((len(text), [3]), (len(text) - 1, [3]), (12, [3]), (11, [])):
            # ERROR: 1 | 2 follows behind the view; [3] with keep == 12: the match ends exactly on n - 1
            d_text = _dev(text[:keep], first, behind=text[keep:] + b"234 ")
            got, total = _begins(ctx, d_text, host.compile_regex(LOG))
            assert got.tolist() == want and total == len(want), (first, keep)
    d_text = _dev(text + b"2", 7)
    assert _begins(ctx, d_text, host.compile_regex(LOG))[0].tolist() == [3, 16]


def _planted(rng, n, alphabet, rx, count):
    text = rng.choice(np.frombuffer(alphabet, np.uint8), n).astype(np.uint8)
    for at in rng.integers(0, n - 80, count):
        ro.plant_path(rng, text, rx, int(at))
    ro.plant_path(rng, text, rx, 0)
    return text


@pytest.mark.parametrize("expr,alphabet,wide,irregular", [(LITERAL, b"abcdefgh ", False, False), (LOG, b"ERORFATL: 0123 ", False, True),
                                                          (ORF, b"ACGT", True, True), (CLS40, b"ACGT", True, False)],
                         ids=["m<=32 regular", "m<=32 irregular", "m>32 irregular", "m>32 regular"])
def test_the_four_kernels(ctx, expr, alphabet, wide, irregular):
    rx = ro.parse(expr)
    rev = ro.reverse(rx)
    assert (rx.m > 32) == wide and (ro.split(rev)[1] != 0) == irregular  # which kernel the host picks
    if expr == ORF:
        assert rx.max_len == 38 and ro.parse(ORF[20:]).max_len == 18
    rng = np.random.default_rng(rx.m)
    text = _planted(rng, 20011, alphabet, rx, 150)
    for first in (0, 9):
        want = _check(ctx, text.tobytes(), rx, first=first, what=expr)
        assert want.size >= 100 and want[0] == 0


def test_lane_tile_and_ownership_boundaries(exp_ctx):
    """Lanes of 16 starts, tiles of 4 KiB, two workgroups over five tiles: a max_len-byte match that begins at the last and
    at the first start of a lane, of a tile and of the view's ownership."""
    rx = ro.parse("(k|lm)n{8}o")
    L = rx.max_len
    assert L == 11
    first = 5
    n = 4 * 4096 + 300
    tail = L - 1
    text = np.full(n, ord("z"), np.uint8)
    match = np.frombuffer(b"lmnnnnnnnno", np.uint8)
    T = 4096
    at = [0,                          # the view's first start
          T - first - 1,              # the last start of tile 0 (of its lane 255)
          T - first + 16 * 40,        # the first start of a lane
          T - first + 16 * 60 - 1,    # the last start of a lane
          2 * T - first,              # the first start of a tile
          3 * T - first - 1,          # the last start of a tile
          3 * T - first + 16,
          n - L]                      # the last start the view owns with tail = max_len - 1 (the match ends on n - 1)
    for a in at:
        text[a:a + L] = match
    want_s, _, _ = bo.begins_numpy(text.tobytes(), rx)
    assert want_s.tolist() == at
    d_text = _dev(text.tobytes(), first)
    re_ = bo.struct_of(rx)
    exp_ctx.set_knob("regex_begins_piece_shift", 4)
    got, total = _begins(exp_ctx, d_text, re_)  # (the shared knobs reach a session that exists)
    assert np.array_equal(got, want_s)
    exp_ctx.set_knob("tile_max_grid", 2)
    for t in (0, tail):
        got, total = _begins(exp_ctx, d_text, re_, tail=t)
        assert total == want_s.size and np.array_equal(got, want_s), t
        shift, grid, tiles = exp_ctx.last_launch("regex_begins")
        assert (shift, grid) == (4, 2) and tiles == 5 and tiles > 2 * grid - 1  # more than one tile per workgroup
    got, total = _begins(exp_ctx, d_text, re_, tail=tail + 1)  # the last match's start is no longer owned
    assert np.array_equal(got, want_s[:-1])
    exp_ctx.set_knob("regex_begins_piece_shift", 0)
    exp_ctx.set_knob("tile_piece_shift", 6)  # the shared knob applies too
    got, total = _begins(exp_ctx, d_text, re_)
    assert np.array_equal(got, want_s) and exp_ctx.last_launch("regex_begins")[:2] == (6, 2)


@pytest.fixture(scope="module")
def dense():
    n = 1 << 16
    flat = np.full(n, ord("a"), np.uint8)
    gaps = flat.copy()
    gaps[::97] = ord("b")
    return flat, gaps


def test_dense_tiles_write_downwards(ctx, dense):
    flat, gaps = dense
    re_ = host.compile_regex("a{1,3}")
    for first in (0, 3):
        got, total = _begins(ctx, _dev(flat.tobytes(), first), re_)
        assert total == flat.size and np.array_equal(got, np.arange(flat.size))
        want = np.nonzero(gaps == ord("a"))[0]
        got, total = _begins(ctx, _dev(gaps.tobytes(), first), re_)
        assert total == want.size and np.array_equal(got, want)
    re_ = host.compile_regex("aaab")  # lanes with one hit beside lanes with none, in the same text
    want = np.nonzero(gaps == ord("b"))[0][1:] - 3
    got, total = _begins(ctx, _dev(gaps.tobytes(), 11), re_)
    assert np.array_equal(got, want)


def test_capacity(ctx, dense):
    import torch

    flat, gaps = dense
    want = np.nonzero(gaps == ord("a"))[0]
    re_ = host.compile_regex("a{1,3}")
    d_text = _dev(gaps.tobytes(), 2)
    L = ctx._L
    total = C.c_uint64(0)

    def raw(out, cap):
        rc = L.bmx_search_regex_begins_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0, C.byref(re_),
                                              C.c_void_p(out.data_ptr()) if out is not None else None, cap, C.byref(total), None)
        return rc, int(total.value)

    assert raw(None, 0) == (host.ERR_CAPACITY, want.size)  # count only
    out = torch.full((want.size + 8,), -1, dtype=torch.int64, device="cuda")
    assert raw(out, want.size) == (host.OK, want.size)  # exact
    assert np.array_equal(out[:want.size].cpu().numpy(), want) and bool((out[want.size:] == -1).all())
    for cap in (want.size - 1, 1, 2049):  # one short; one entry of a dense tile; inside the second tile
        out.fill_(-1)
        assert raw(out, cap) == (host.ERR_CAPACITY, want.size), cap
        assert np.array_equal(out[:cap].cpu().numpy(), want[:cap]) and bool((out[cap:] == -1).all()), cap  # the lowest
    sparse = _dev(b"zzzz" * 2000 + b"aaz", 1)  # a parked tile
    out.fill_(-1)
    d_text = sparse
    assert raw(out, 1) == (host.ERR_CAPACITY, 2) and out[:2].cpu().tolist() == [8000, -1]
    assert raw(out, 2) == (host.OK, 2) and out[:3].cpu().tolist() == [8000, 8001, -1]


@pytest.mark.parametrize("shards", [3, 7])
def test_shards_concatenate(ctx, shards):
    rx = ro.parse(LOG)
    rng = np.random.default_rng(shards)
    n = 70001
    text = _planted(rng, n, b"ERORFATL: 0123 ", rx, 900)
    want, _, _ = bo.begins_numpy(text.tobytes(), rx)
    re_ = bo.struct_of(rx)
    d_text = _dev(text.tobytes(), 6)
    cuts = [n * i // shards for i in range(shards + 1)]
    for base in (0, (1 << 40) - n):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            tail = min(rx.max_len - 1, n - hi)  # clipped at the text's end
            got, total = _begins(ctx, d_text[lo:hi + tail], re_, tail=tail, base_offset=base + lo)
            assert total == got.size
            parts.append(got)
        assert np.array_equal(np.concatenate(parts), want + base), base
    got, total = _begins(ctx, d_text[:100], re_, tail=100)  # tail == n: no start is owned
    assert total == 0 and got.size == 0


def test_identities_against_the_forward_search(ctx):
    import torch

    rng = np.random.default_rng(0x1DE)
    some = 0
    for case in range(12):
        symbols = np.arange(97, 99 + case % 3)
        expr, rx = ro.random_regex(rng, symbols, 12)
        text = rng.choice(symbols, 5000).astype(np.uint8)
        re_ = host.compile_regex(expr)
        d_text = torch.from_numpy(text).cuda()
        n = text.size
        begins, total = ctx.search_regex_begins_device(d_text, re_, capacity=n)
        assert total == begins.numel()
        ends, t2 = ctx.search_regex_device(d_text, re_, capacity=n)
        have = set(begins.cpu().tolist())
        for longest in (False, True):  # (a) every start of either starts pass is in the list
            s = ctx.regex_starts_device(d_text, re_, ends, longest=longest) if t2 else ends
            assert set(s.cpu().tolist()) <= have, (expr, longest)
        flipped = torch.flip(d_text, [0]).contiguous()  # (b) the forward search of the reversed automaton on the flipped text
        rev_ends, t3 = ctx.search_regex_device(flipped, host.reverse_regex(re_), capacity=n)
        assert t3 == total and torch.equal(torch.flip((n - 1) - rev_ends, [0]), begins), expr
        assert np.array_equal(begins.cpu().numpy(), bo.begins_numpy(text.tobytes(), rx)[0]), expr
        some += total
    assert some > 5000


def test_text_beyond_4GiB(ctx):
    """2^32 + 4,097 bytes of ACGT (allocated and filled as in test_gpu_tile_geometry.py): matches that begin at 2^32 - 1
    (it ends at 2^32) and at 2^32, one in front, one in the last 16 bytes that ends on the last byte.  Exactly the planted
    starts are reported, with their ends; the oracle runs on the windows around the plants."""
    import torch

    B = 1 << 32
    n = B + 4097
    rx = ro.parse("a(b|cd){0,2}a")
    d_text = torch.empty(n, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    ctx.gen_text(d_text, 0, 0x5EED4B17, kind=1)
    for at, p in ((5, b"acdba"), (B - 2, b"aaaba"), (n - 5, b"abcda")):
        d_text[at:at + len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(d_text.device)
    want_s, want_short, want_long = [], [], []
    for lo, hi in ((0, 64), (B - 64, B + 64), (n - 64, n)):
        s_, short, long_ = bo.begins_numpy(d_text[lo:hi].cpu().numpy().tobytes(), rx)
        want_s += (s_ + lo).tolist()
        want_short += (short + lo).tolist()
        want_long += (long_ + lo).tolist()
    assert want_s == [5, B - 2, B - 1, B, n - 5] and want_long == [9, B - 1, B, B + 2, n - 1] and want_short[2] == B
    re_ = bo.struct_of(rx)
    out = torch.full((64,), -1, dtype=torch.int64, device=d_text.device)
    starts, total = ctx.search_regex_begins_device(d_text, re_, out=out)
    assert total == len(want_s) and starts.cpu().tolist() == want_s and bool((out[total:] == -1).all())
    assert ctx.regex_ends_device(d_text, re_, starts, longest=True).cpu().tolist() == want_long
    assert ctx.regex_ends_device(d_text, re_, starts).cpu().tolist() == want_short
    del d_text
    torch.cuda.empty_cache()


def test_on_a_callers_stream_behind_a_pending_copy(ctx):
    """The view holds a decoy; a long row of copies and then the copy of the real text are enqueued on a non-blocking
    stream; the search is called while that copy is outstanding and must see the real text."""
    import torch

    rx = ro.parse(LOG)
    rng = np.random.default_rng(77)
    real = _planted(rng, 1 << 20, b"ERORFATL: 0123 ", rx, 500)
    decoy = _planted(rng, 1 << 20, b"ERORFATL: 0123 ", rx, 400)
    want, _, want_long = bo.begins_numpy(real.tobytes(), rx)
    assert not np.array_equal(want, bo.begins_numpy(decoy.tobytes(), rx)[0])
    re_ = bo.struct_of(rx)
    buf = torch.from_numpy(decoy.copy()).cuda()
    d_real = torch.from_numpy(real.copy()).cuda()
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(2 << 28, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i in range(64):
            a, b = (0, 1 << 28) if i & 1 else (1 << 28, 0)
            scratch[a:a + (1 << 28)].copy_(scratch[b:b + (1 << 28)], non_blocking=True)
        buf.copy_(d_real, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
        assert not pending.query(), "the delay is too short: the producer had finished before the call"
        starts, total = ctx.search_regex_begins_device(buf, re_, out=out, stream=s)
        ends = ctx.regex_ends_device(buf, re_, starts, longest=True, stream=s)
    assert total == want.size and np.array_equal(starts.cpu().numpy(), want) and bool((out[total:] == -1).all())
    assert np.array_equal(ends.cpu().numpy(), want_long)


# ---- the ends pass -----------------------------------------------------------------------------------------------------

def test_ends_on_random_pairs(ctx):
    seen = clipped = 0
    for i, (text, expr, rx) in enumerate(_random_pairs(100, 0xE2D5)):
        want = _check(ctx, text, expr, first=i % 16, behind=text, what=(text, expr))  # (also: matches clipped by the view's end)
        seen += want.size
        full_s, _, full_l = bo.begins_numpy(text + text, rx)
        clipped += list(zip(full_s[full_s < len(text)].tolist(), full_l[full_s < len(text)].tolist())) != \
            list(zip(want.tolist(), bo.begins_numpy(text, rx)[2].tolist()))
    assert seen > 500 and clipped > 5


def test_ends_word_alignment_and_the_last_word(ctx):
    import torch

    rx = ro.parse("a(b|cd){1,3}e")
    re_ = bo.struct_of(rx)
    for first in range(16):
        for s in range(8):  # every s mod 8, for every alignment of the view
            text = b"z" * s + b"acdbcde" + b"z" * (first % 3)
            d_text = _dev(text, first, behind=b"bcde")
            starts = torch.tensor([s], dtype=torch.int64, device="cuda")
            assert ctx.regex_ends_device(d_text, re_, starts, longest=True).cpu().tolist() == [s + 6]
            assert ctx.regex_ends_device(d_text, re_, starts).cpu().tolist() == [s + 6]
            text = b"z" * s + b"abe"  # a start in the view's last 8-byte word, the match ends on the last byte
            d_text = _dev(text, first, behind=b"bcde")
            for base in (0, 1 << 33):
                starts = torch.tensor([base + s], dtype=torch.int64, device="cuda")
                got = ctx.regex_ends_device(d_text, re_, starts, longest=True, base_offset=base)
                assert got.cpu().tolist() == [base + s + 2]


def test_ends_errors_and_limits(ctx):
    import torch

    re_ = host.compile_regex("a.{0,3}b")
    text = b"a1b3b\nab a"
    d_text = _dev(text, 3, behind=b"bbbb")
    t = lambda *v: torch.tensor(list(v), dtype=torch.int64, device="cuda")
    assert ctx.regex_ends_device(d_text, re_, t()).numel() == 0  # count == 0
    assert ctx.regex_ends_device(d_text, re_, t(0, 6)).cpu().tolist() == [2, 7]
    assert ctx.regex_ends_device(d_text, re_, t(0, 6), longest=True).cpu().tolist() == [4, 7]
    for bad in (t(0, len(text)), t(-1, 0), t(1 << 40)):  # a start outside the view
        with pytest.raises(host.BmxError) as e:
            ctx.regex_ends_device(d_text, re_, bad)
        assert e.value.rc == host.ERR_ARG
    assert ctx.regex_ends_device(d_text, re_, t(1, 7), base_offset=1).cpu().tolist() == [3, 8]
    with pytest.raises(host.BmxError) as e:
        ctx.regex_ends_device(d_text, re_, t(1, 4), base_offset=1)  # 4 - 1 = 3: nothing begins at '3'
    assert e.value.rc == host.ERR_ARG
    for none in (t(1), t(9), t(0, 9)):  # a start from which nothing begins (9: the b lies behind the view)
        with pytest.raises(host.BmxError) as e:
            ctx.regex_ends_device(d_text, re_, none)
        assert e.value.rc == host.ERR_ARG
        lim = torch.full_like(none, len(text) - 1)
        got = ctx.regex_ends_device(d_text, re_, none, limit=lim, longest=True).cpu().tolist()
        assert got == [4 if s == 0 else -1 for s in none.cpu().tolist()]
    starts = t(0, 0, 0, 0, 6, 6, 0)
    limit = t(4, 3, 2, 1, 7, 6, 0)  # cuts the longest match to the shorter one; leaves none
    assert ctx.regex_ends_device(d_text, re_, starts, longest=True, limit=limit).cpu().tolist() == [4, 2, 2, -1, 7, -1, -1]
    assert ctx.regex_ends_device(d_text, re_, starts, limit=limit).cpu().tolist() == [2, 2, 2, -1, 7, -1, -1]
    assert ctx.regex_ends_device(d_text, re_, t(100, 106), limit=t(103, 50), base_offset=100, longest=True).cpu().tolist() == [102, -1]
    L = ctx._L
    out = torch.empty(4, dtype=torch.int64, device="cuda")
    assert L.bmx_regex_ends_device(ctx._h, None, 10, 0, C.byref(re_), C.c_void_p(out.data_ptr()), 0, None, 0, None, None) == host.OK


# ---- end to end --------------------------------------------------------------------------------------------------------

def _log(lines=2000):
    rng = np.random.default_rng(2000)
    words = [b"ERROR: ", b"FATAL: ", b"INFO: ", b"ERROR:", b"WARN "]
    out = []
    for _ in range(lines):
        w = words[int(rng.integers(0, len(words)))]
        out.append(w + bytes(rng.integers(48, 58, int(rng.integers(0, 7))).astype(np.uint8)) + b" at " +
                   bytes(rng.integers(97, 123, int(rng.integers(0, 9))).astype(np.uint8)))
    return b"\n".join(out) + b"\n"


@pytest.mark.parametrize("expr,text", [("[0-9]{1,8}", b"a1 22 x333333333333 4444\n5"), ("(a|ab)(c|bcd)", b"abcd abc abcdabcd"),
                                       ("ab|b", b"ab cab bab abb"), ("colou?r", b"color colour colouur colourcolor"),
                                       ("(ERROR|FATAL): [0-9]{2,4}", None)],
                         ids=["digit runs", "abcd", "ab|b", "colou?r", "log"])
def test_findall_and_sub_posix(ctx, expr, text):
    text = _log() if text is None else text
    want = bo.posix_matches(text, expr) if len(text) < 1000 else None
    if want is None:  # the log: the sequential definition from the oracle's list of (start, longest end), which the CPU suite ties to it
        s, _, e = bo.begins_numpy(text, ro.parse(expr))
        ws, we, _ = so.select(so.spans_of(starts=s.astype(np.uint64), ends=e.astype(np.uint64)))
        want = list(zip(ws.tolist(), we.tolist()))
        assert len(want) > 300
    assert host.findall(text, expr, posix=True) == [text[s:e + 1] for s, e in want]
    assert host.sub(text, expr, b"<>", posix=True) == so.replace(text, [s for s, _ in want], [e for _, e in want], b"<>")
    if expr == "[0-9]{1,8}":
        assert host.findall(text, expr, posix=True) == [b"1", b"22", b"33333333", b"3333", b"4444", b"5"]
        assert host.findall(text, expr) == [bytes([c]) for c in text if 48 <= c < 58]  # leftmost-shortest: single digits
    if expr == "(a|ab)(c|bcd)":
        assert host.findall(text, expr, posix=True)[0] == b"abcd"


def test_posix_per_line(ctx):
    expr = "a.{0,3}b"
    text = b"a1\nxb a1b\nab\n" + b"axb\nb\n" + b"ab\nb a\nb axxb\n"
    assert host.findall(text, expr, posix=True)[0] == b"a1\nxb"  # across the line break without rows
    want = bo.posix_matches(text, expr, bo.row_end(text))
    assert want != bo.posix_matches(text, expr) and (13, 15) in want  # axb: the longest from 13 would be axb\nb
    assert host.findall(text, expr, posix=True, rows=True) == [text[s:e + 1] for s, e in want]
    assert host.sub(text, expr, b"-", posix=True, rows=True) == bo.posix_replace(text, expr, b"-", bo.row_end(text))
    log = _log(300)
    want = bo.posix_matches(log, "[0-9]{2,3}.{0,6}[a-z]", bo.row_end(log))
    assert len(want) > 100
    assert host.findall(log, "[0-9]{2,3}.{0,6}[a-z]", posix=True, rows=True) == [log[s:e + 1] for s, e in want]


@pytest.mark.parametrize("expr", ["ERROR: [0-9]{3}", "[0-9]{1,8}"])
def test_without_posix_nothing_changes(ctx, expr):
    import torch

    text = _log(500)
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    s, e = ctx.search_regex_spans(text, expr)
    ws, we, _ = so.select(so.spans_of(s, e))
    assert ws.size > 50
    for kw in ({}, {"posix": False}):
        out, n_out = ctx.sub_device(d_text, expr, b"<>", kind="regex", **kw)
        assert out.cpu().numpy().tobytes() == so.replace(text, ws, we, b"<>")
        blob, off = ctx.findall_device(d_text, expr, kind="regex", **kw)
        want_blob, want_off = so.extract(text, ws, we)
        assert blob.cpu().numpy().tobytes() == want_blob and np.array_equal(off.cpu().numpy().astype(np.uint64), want_off)


def test_host_buffer_forms(ctx):
    text = _log(200)
    expr = "(ERROR|FATAL): [0-9]{2,4}"
    s, short, long_ = bo.begins_numpy(text, ro.parse(expr))
    assert np.array_equal(host.search_regex_begins(text, expr).astype(np.int64), s)
    gs, ge = host.search_regex_begins(text, expr, spans=True)
    assert np.array_equal(gs.astype(np.int64), s) and np.array_equal(ge.astype(np.int64), short)
    gs, ge = ctx.search_regex_begins_spans(text, expr, longest=True)
    assert np.array_equal(gs.astype(np.int64), s) and np.array_equal(ge.astype(np.int64), long_)
    with pytest.raises(host.BmxError) as e:
        ctx.search_regex_begins(text, expr, capacity=3)
    assert e.value.rc == host.ERR_CAPACITY
    assert ctx.last_regex_begins_ms() > 0


def _cli(path, args):
    exe = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")
    out = subprocess.run([exe, "--text", str(path)] + args, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout, out.stderr.decode()


def test_cli(tmp_path):
    text = b"a1 22 x333333333333 4444\n5 a12b\nb66\n"
    path = tmp_path / "t.txt"
    path.write_bytes(text)
    out, err = _cli(path, ["--regex", "[0-9]{1,8}", "--only-matching", "--posix"])
    assert out.split(b"\n")[:-1] == [b"1", b"22", b"33333333", b"3333", b"4444", b"5", b"12", b"66"]
    out, err = _cli(path, ["--regex", "[0-9]{1,8}", "--replace", "N", "--posix"])
    assert out == b"aN N xNN N\nN aNb\nbN\n"
    want = bo.posix_matches(text, "a.{1,4}b", bo.row_end(text))
    assert want == [(27, 30)] and bo.posix_matches(text, "a.{1,4}b") == [(27, 32)]
    out, err = _cli(path, ["--regex", "a.{1,4}b", "--only-matching", "--posix", "--lines"])
    assert out == b"a12b\n"
    out, err = _cli(path, ["--regex", "a.{1,4}b", "--only-matching", "--posix"])
    assert out == b"a12b\nb\n"
    starts, short, long_ = bo.begins_brute(text, "[0-9]{1,8}")
    out, err = _cli(path, ["--regex", "[0-9]{1,8}", "--begins", "--positions", "--max-print", "1000"])
    assert [int(l.split(b":")[1]) for l in out.split(b"\n") if l.startswith(b"Start at")] == starts
    assert f"regex match starts: {len(starts)}".encode() in out
    out, err = _cli(path, ["--regex", "[0-9]{1,8}", "--begins", "--spans", "--longest", "--positions", "--max-print", "1000"])
    assert [tuple(map(int, l.split(b":")[1].split())) for l in out.split(b"\n") if l.startswith(b"Match at")] == list(zip(starts, long_))
    exe = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")
    for bad in (["--regex", "a", "--posix"], ["--regex", "a", "--posix", "--merge", "--only-matching"],
                ["--gaps", "a", "--posix", "--only-matching"], ["--regex", "a", "--begins", "--longest"]):
        assert subprocess.run([exe, "--text", str(path)] + bad, capture_output=True, timeout=60).returncode == 2
