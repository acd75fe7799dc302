"""CPU suite of the row-wise results (bmx_rows_*): the numpy oracle against bytes.split bookkeeping on hand-written texts
and, end to end, against Python's ``re`` per line; every argument error of the three device entries and of bmx_rows_split
with ctx = NULL, which has to come back as BMX_ERR_ARG before any HIP call and touch no output."""
import ctypes as C
import re

import numpy as np
import pytest

import regex_oracle as rx
import rows_oracle as ro
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

NONE = int(ro.NONE)


def by_split(text: bytes, d: int):
    """The rows as bytes.split sees them: the pieces, each but an unterminated last one with its delimiter back on."""
    parts = text.split(bytes([d]))
    rows = [p + bytes([d]) for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return off


@pytest.mark.parametrize("text,d,want", [
    (b"", 10, [0]),
    (b"\n", 10, [0, 1]),
    (b"a", 10, [0, 1]),
    (b"a\n", 10, [0, 2]),
    (b"a\nb", 10, [0, 2, 3]),
    (b"\n\n", 10, [0, 1, 2]),
    (b"x\xffyz\xff\xff", 0xFF, [0, 2, 5, 6]),
])
def test_split_oracle_on_hand_written_texts(text, d, want):
    off = ro.split(text, d)
    assert off.tolist() == want == by_split(text, d)
    rows = off.size - 1
    assert rows == text.count(bytes([d])) + (len(text) > 0 and text[-1] != d)
    assert ro.split(text, d, base_offset=1000).tolist() == [w + 1000 for w in want]


def test_row_of_and_matching_oracle_by_hand():
    off = np.array([10, 13, 13, 20], np.uint64)  # rows [10,13) [13,13) [13,20)
    s = np.array([10, 12, 12, 13, 19, 9, 19, NONE, 15], np.uint64)
    e = np.array([12, 12, 13, 13, 19, 10, 20, 15, 14], np.uint64)
    ids = ro.row_of(off, s, e)
    assert ids.tolist() == [0, 0, NONE, 2, 2, NONE, NONE, NONE, NONE]
    hit, cnt = ro.matching(ids, 3)
    assert hit.tolist() == [0, 2] and cnt.tolist() == [2, 2]
    assert ro.matching(ids, 3, invert=True)[0].tolist() == [1]
    assert ro.matching(np.zeros(0, np.uint64), 2, invert=True)[0].tolist() == [0, 1]


def test_line_set_equals_re_per_line():
    expr = "(ERROR|FATAL): [0-9]{2,4}"
    text, plants = ro.log_text(np.random.default_rng(2000), 2000, 120)
    assert len(plants) > 100
    lines = text.split(b"\n")[:-1]
    assert len(lines) == 2000
    off = ro.split(text, 10)
    assert off.size == 2001
    ends, starts = rx.starts_numpy(text, rx.parse(expr))
    ids = ro.row_of(off, starts, ends)
    assert not (ids == ro.NONE).any()  # no class of the expression holds the newline
    hit, cnt = ro.matching(ids, 2000)
    pat = re.compile(expr.encode())
    want = [i for i, ln in enumerate(lines) if pat.search(ln)]
    assert want and hit.tolist() == want
    assert int(cnt.sum()) == ends.size
    inv, none = ro.matching(ids, 2000, invert=True)
    assert none is None and inv.tolist() == sorted(set(range(2000)) - set(want))


def test_a_dot_that_spans_a_newline_has_no_row():
    text = b"ab\ncd\n"
    ends, starts = rx.starts_numpy(text, rx.parse("b.c"))
    assert ends.tolist() == [3] and starts.tolist() == [1]
    assert ro.row_of(ro.split(text, 10), starts, ends).tolist() == [NONE]
    ends, starts = rx.starts_numpy(text, rx.parse("b."))  # the delimiter as the last byte stays inside the row
    assert ro.row_of(ro.split(text, 10), starts, ends).tolist() == [0]


# ---- argument errors: before any HIP call, with ctx = NULL ------------------------------------------------------------

P = C.c_void_p(0x1000)  # a pointer that is not NULL and must never be read


def test_split_device_argument_errors(built):
    L = host.lib()
    rows, longest = C.c_uint64(77), C.c_uint64(78)
    tail = (C.byref(rows), C.byref(longest), None)
    assert L.bmx_rows_split_device(None, None, 5, 0, 10, P, 8, *tail) == host.ERR_ARG  # NULL text
    assert L.bmx_rows_split_device(None, P, 1 << 40, 0, 10, P, 8, *tail) == host.ERR_ARG  # n too large
    assert L.bmx_rows_split_device(None, P, 5, 0, 10, None, 8, *tail) == host.ERR_ARG  # capacity without a buffer
    assert L.bmx_rows_split_device(None, P, 5, 0, 10, P, 8, *tail) == host.ERR_ARG  # valid, but no context
    assert L.bmx_rows_split_device(None, None, 0, 0, 10, None, 0, *tail) == host.ERR_ARG  # ... not even for an empty text
    assert (rows.value, longest.value) == (77, 78)
    assert L.bmx_last_rows_ms(None) < 0


def test_rows_of_device_argument_errors(built):
    L = host.lib()
    assert L.bmx_rows_of_device(None, None, 3, P, P, 0, 4, P, None) == host.ERR_ARG  # NULL offsets
    assert L.bmx_rows_of_device(None, P, 3, P, P, 0, 4, None, None) == host.ERR_ARG  # NULL output
    assert L.bmx_rows_of_device(None, P, 3, None, None, 4, 4, P, None) == host.ERR_ARG  # no list
    assert L.bmx_rows_of_device(None, P, 3, P, P, 4, 4, P, None) == host.ERR_ARG  # both lists and a length
    assert L.bmx_rows_of_device(None, P, 3, P, None, 0, 4, P, None) == host.ERR_ARG  # starts alone, no length
    assert L.bmx_rows_of_device(None, P, 3, None, P, 0, 4, P, None) == host.ERR_ARG  # ends alone, no length
    for starts, ends, ln in ((P, P, 0), (P, None, 4), (None, P, 4)):  # the three valid forms, but no context
        assert L.bmx_rows_of_device(None, P, 3, starts, ends, ln, 4, P, None) == host.ERR_ARG
    assert L.bmx_rows_of_device(None, None, 3, None, None, 0, 0, None, None) == host.OK  # count == 0: nothing to do


def test_rows_matching_device_argument_errors(built):
    L = host.lib()
    n_out = C.c_uint64(77)
    assert L.bmx_rows_matching_device(None, P, 4, 3, 2, P, None, 8, C.byref(n_out), None) == host.ERR_ARG  # unknown flag
    assert L.bmx_rows_matching_device(None, P, 4, 3, host.ROWS_INVERT, P, P, 8, C.byref(n_out), None) == host.ERR_ARG  # counts of no entries
    assert L.bmx_rows_matching_device(None, None, 4, 3, 0, P, None, 8, C.byref(n_out), None) == host.ERR_ARG  # NULL list
    assert L.bmx_rows_matching_device(None, P, 4, 3, 0, None, None, 8, C.byref(n_out), None) == host.ERR_ARG  # capacity without a buffer
    assert L.bmx_rows_matching_device(None, P, 4, 3, 0, P, P, 8, C.byref(n_out), None) == host.ERR_ARG  # valid, but no context
    assert n_out.value == 77


def test_rows_split_host_argument_errors(built):
    L = host.lib()
    rows, longest = C.c_uint64(77), C.c_uint64(78)
    off = (C.c_uint64 * 4)(9, 9, 9, 9)
    buf = C.create_string_buffer(b"a\nb")
    t = C.cast(buf, C.c_void_p)
    assert L.bmx_rows_split(None, None, 3, 10, off, 4, C.byref(rows), C.byref(longest)) == host.ERR_ARG  # NULL text
    assert L.bmx_rows_split(None, t, 1 << 40, 10, off, 4, C.byref(rows), C.byref(longest)) == host.ERR_ARG  # n too large
    assert L.bmx_rows_split(None, t, 3, 10, None, 4, C.byref(rows), C.byref(longest)) == host.ERR_ARG  # capacity without a buffer
    assert (rows.value, longest.value, list(off)) == (77, 78, [9, 9, 9, 9])
    # an empty text is answered without a device: no row, the single entry off[0]
    assert L.bmx_rows_split(None, None, 0, 10, off, 4, C.byref(rows), C.byref(longest)) == host.OK
    assert (rows.value, longest.value, list(off)) == (0, 0, [0, 9, 9, 9])
    o, lg = host.rows_split(b"")
    assert o.tolist() == [0] and lg == 0


def test_rows_of_and_matching_host_argument_errors(built):
    """The host-buffer forms make the device entries' checks, before a context is made."""
    L = host.lib()
    row = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert L.bmx_rows_of(None, None, 3, P, P, 0, 4, row) == host.ERR_ARG
    assert L.bmx_rows_of(None, P, 3, P, P, 4, 4, row) == host.ERR_ARG
    assert L.bmx_rows_of(None, P, 3, P, None, 0, 4, row) == host.ERR_ARG
    assert L.bmx_rows_of(None, P, 3, None, None, 4, 4, row) == host.ERR_ARG
    assert L.bmx_rows_of(None, P, 3, P, P, 0, 4, None) == host.ERR_ARG
    assert L.bmx_rows_of(None, None, 3, None, None, 0, 0, None) == host.OK
    n_out = C.c_uint64(77)
    assert L.bmx_rows_matching(None, P, 4, 3, 2, row, None, 4, C.byref(n_out)) == host.ERR_ARG
    assert L.bmx_rows_matching(None, P, 4, 3, host.ROWS_INVERT, row, row, 4, C.byref(n_out)) == host.ERR_ARG
    assert L.bmx_rows_matching(None, None, 4, 3, 0, row, None, 4, C.byref(n_out)) == host.ERR_ARG
    assert L.bmx_rows_matching(None, P, 4, 3, 0, None, None, 4, C.byref(n_out)) == host.ERR_ARG
    assert (n_out.value, list(row)) == (77, [9, 9, 9, 9])
