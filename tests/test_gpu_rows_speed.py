"""The row-wise results against the route a caller took before them, measured in the same run, best of 3 after a warm-up;
no absolute times.  1 GiB of printable-95 text with about 2^23 newlines at seeded random positions and ``ERROR: 123``
planted 2^16 times.

Split: bmx_last_rows_ms of the split (offsets and longest row) against bmx_last_classes_ms of the one-position class
search for the newline on the same text, which is what gave the line breaks before -- not charging the arithmetic that
turns that list into offsets.
Row of every match + matching rows: 2^22 synthetic ascending spans through Rows.of and Rows.matching against
torch.searchsorted(off, ends, right=True), the two comparisons and torch.unique_consecutive(return_counts=True), each side
between one pair of events.

Each new stage may take at most (1 + SPREAD) times the old route, SPREAD being the 4 % box-to-box spread the README states
for one kernel: not being slower is the condition.  The measured values are in DESIGN.md s28.

Measured on the MI355X: the split takes 0.453 ms against 0.747 ms (ratio 0.61; 0.383 against 0.765 on another box).
Rows.of + Rows.matching take 0.266-0.274 ms against 0.304-0.312 ms for the torch route (ratio 0.87-0.88; the row kernel
0.095 ms against 0.28 ms for searchsorted and the comparisons, the matching rows 0.098 ms over three tile passes against
0.045 ms for unique_consecutive, each of the two calls waiting for the stream once)."""
import numpy as np
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

SPREAD = 0.04


@pytest.fixture(scope="module")
def big(ctx):
    """The text, once for the module."""
    import torch

    n = 1 << 30
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x20B5, 0)
    rng = np.random.default_rng(0x20B5)
    ctx.plant(d_text, 0, b"ERROR: 123", np.sort(rng.choice(n // 16 - 1, 1 << 16, replace=False).astype(np.uint64)) * np.uint64(16))
    g = torch.Generator(device="cuda")
    g.manual_seed(0x20B5)
    d_text[torch.randint(0, n, (1 << 23,), generator=g, device="cuda")] = 10
    yield d_text
    del d_text
    torch.cuda.empty_cache()


def test_split_is_not_slower_than_the_class_search_for_the_newline(ctx, big):
    import torch

    d_text = big
    room = (1 << 23) + 64
    out_r = torch.empty(room, dtype=torch.int64, device="cuda")
    out_c = torch.empty(room, dtype=torch.int64, device="cuda")
    newline = host.compile_classes("\\x0a")
    assert newline.shape[0] == 1
    ctx.rows_split_device(d_text, out=out_r)  # warm-up
    ctx.search_classes_device(d_text, newline, out=out_c)
    t_rows, t_cls = [], []
    for _ in range(3):
        rows = ctx.rows_split_device(d_text, out=out_r)
        t_rows.append(ctx.last_rows_ms())
        starts, total = ctx.search_classes_device(d_text, newline, out=out_c)
        t_cls.append(ctx.last_classes_ms())
    assert total == starts.numel() and (1 << 22) < total <= (1 << 23)
    assert rows.count == total + int(d_text[-1].item() != 10)
    assert torch.equal(rows.offsets[1:total + 1], starts + 1) and rows.offsets[0].item() == 0 and rows.offsets[-1].item() == d_text.numel()
    assert rows.longest == int((rows.offsets[1:] - rows.offsets[:-1]).max().item())
    r, c = min(t_rows), min(t_cls)
    print(f"ROWS split {r:.3f} ms, class search for the newline {c:.3f} ms, ratio {r / c:.3f} ({rows.count} rows, longest {rows.longest})")
    assert r <= (1.0 + SPREAD) * c, (r, c)


def test_row_of_and_matching_are_not_slower_than_searchsorted_and_unique(ctx, big):
    import torch

    d_text = big
    rows = ctx.rows_split_device(d_text)
    off, n_rows = rows.offsets, rows.count
    g = torch.Generator(device="cuda")
    g.manual_seed(22)
    starts = torch.sort(torch.randint(0, d_text.numel() - 10, (1 << 22,), generator=g, device="cuda")).values
    ends = starts + 9
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def ours():
        ids = rows.of(starts=starts, length=10)
        return ids, rows.matching(ids)

    def theirs():
        r = torch.searchsorted(off, ends, right=True) - 1
        ok = (r >= 0) & (r < n_rows)
        ok &= starts >= off[r.clamp(0, n_rows - 1)]
        return r, ok, torch.unique_consecutive(r[ok], return_counts=True)

    ours(), theirs()  # warm-up
    t_new, t_old = [], []
    for _ in range(3):
        ev[0].record()
        ids, (hit, cnt) = ours()
        ev[1].record()
        ev[2].record()
        r, ok, (hit_t, cnt_t) = theirs()
        ev[3].record()
        torch.cuda.synchronize()
        t_new.append(ev[0].elapsed_time(ev[1]))
        t_old.append(ev[2].elapsed_time(ev[3]))
    assert torch.equal(torch.where(ok, r, torch.full_like(r, -1)), ids)
    assert torch.equal(hit, hit_t) and torch.equal(cnt, cnt_t) and hit.numel() > (1 << 20)
    a, b = min(t_new), min(t_old)
    print(f"ROWS of + matching {a:.3f} ms, searchsorted + comparisons + unique_consecutive {b:.3f} ms, ratio {a / b:.3f} "
          f"({hit.numel()} rows hit by {int(ok.sum().item())} of {starts.numel()} spans)")
    assert a <= (1.0 + SPREAD) * b, (a, b)
