"""GPU suite: every device entry point of include/bmx.h on a caller's NON-BLOCKING stream.

host.py passes torch's current stream to the library; under pytest that is the null stream, on which everything
serialises and a kernel, copy or memset issued on the wrong stream cannot show.  Here the current stream is a
torch.cuda.Stream() -- created non-blocking, so without implicit ordering against the null stream (asserted through
hipStreamGetFlags) -- and

(a) the input is still being produced on that stream when the entry point is called: the device buffer holds a DECOY,
    the stream holds a long delay and then the copy of the real input, and the answer must be the real input's
    (tests/stream_cases.py; tests/test_stream_cases_cpu.py proves that the decoy's answer differs);
(b) the output is consumed on the stream, without synchronising first;
(c) the null stream is busy while a NEW context makes its first call on the side stream (the first call allocates and
    clears the look-back words and the ticket counter of the approximate and the dictionary search);
(d) one context goes through every algorithm over two side streams and the null stream, with shapes that grow,
    shrink and repeat;
(e) two host threads do (d) at once, each with its own context, streams and answers.

`not pending.query()` right before a call is part of every test of (a) and (c): if the producer is no longer
outstanding the test FAILS ("delay too short"), it never passes for that reason.  The measured host gaps and the
delay's duration are printed (pytest -s) and recorded beside DELAY_COPIES in tests/stream_cases.py.
"""
import ctypes as C
import functools
import threading
import time

import numpy as np
import pytest

import stream_cases as sc
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host, shard, corpus

pytestmark = pytest.mark.gpu

HIP_STREAM_NON_BLOCKING = 0x01  # hipStreamNonBlocking


# ---- the shared rig ------------------------------------------------------------------------------------------------------

def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), through ctypes."""
    import torch  # noqa: F401  (loads it)

    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
    assert paths, "the HIP runtime is not loaded"
    return C.CDLL(paths[0])


def _stream_flags(stream) -> int:
    hip = _hip_runtime()
    hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    hip.hipStreamGetFlags.restype = C.c_int
    flags = C.c_uint(0xFFFF)
    rc = hip.hipStreamGetFlags(C.c_void_p(stream.cuda_stream), C.byref(flags))
    assert rc == 0, f"hipStreamGetFlags: {rc}"
    return int(flags.value)


@functools.lru_cache(maxsize=None)
def _scratch():
    import torch

    return torch.zeros(2 * sc.DELAY_BYTES, dtype=torch.uint8, device="cuda:0")


def side_stream():
    """A torch side stream, checked to be non-blocking (asserted, not skipped)."""
    import torch

    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    assert _stream_flags(s) & HIP_STREAM_NON_BLOCKING, "torch.cuda.Stream() is not a non-blocking stream"
    return s


def null_stream():
    import torch

    s = torch.cuda.default_stream()
    assert s.cuda_stream == 0
    return s


def delay(stream):
    """sc.DELAY_COPIES device-to-device copies of sc.DELAY_BYTES on `stream`: what keeps a producer behind it outstanding
    while the host gets to the library call."""
    import torch

    buf, half = _scratch(), sc.DELAY_BYTES
    with torch.cuda.stream(stream):
        for i in range(sc.DELAY_COPIES):
            a, b = (0, half) if i & 1 else (half, 0)
            buf[a:a + half].copy_(buf[b:b + half], non_blocking=True)


GAPS_MS = []  # host time between pending.record() and the call of the host.py wrapper, every call site of this run


class Pending:
    """An event behind the producer; assert_outstanding() comes right before the library call."""

    def __init__(self, stream):
        import torch

        self.ev = torch.cuda.Event()
        self.ev.record(stream)
        self.t0 = time.perf_counter()

    def assert_outstanding(self, what):
        done = self.ev.query()
        GAPS_MS.append((time.perf_counter() - self.t0) * 1e3)
        print(f"\nSTREAMS host gap pending.record -> {what}: {GAPS_MS[-1]:.3f} ms (worst so far {max(GAPS_MS):.3f} ms)")
        assert not done, f"{what}: delay too short -- the producer had finished before the call (gap {GAPS_MS[-1]:.3f} ms)"


class Loaded:
    """A case on the device: `buf` (what the entry point is given) holds the decoy or the real input, `real` a copy of the
    real operands to produce from, and the output buffers."""

    def __init__(self, case, port, start_with: str = "decoy"):
        import torch

        self.case = case
        self.want = case.want(port)
        dev = torch.device("cuda", 0)
        self.real = [torch.from_numpy(np.array(a)).to(dev) for a in case.real]
        self.buf = [torch.from_numpy(np.array(a)).to(dev) for a in case.operands(start_with)]
        room = max(sum(w.size for w in self.want), 1) + 64
        self.out = torch.full((room,), -1, dtype=torch.int64, device=dev)
        self.aux = {"approx": torch.uint8, "dict": torch.int32}.get(case.kind)
        if self.aux is not None:
            self.aux = torch.zeros(room, dtype=self.aux, device=dev)
        self.dictionary = None

    def produce(self):
        """The copy of the real input over the buffer, on torch's current stream."""
        for b, r in zip(self.buf, self.real):
            b.copy_(r, non_blocking=True)


def call(ctx, L):
    """The case's entry point through host.py on torch's current stream; the result on the host in the layout of
    StreamCase.want().  A return code other than BMX_OK raises (host.BmxError carries it) or fails the assertion."""
    c = L.case
    if c.kind == "scan":
        pos, total = ctx.search_device(L.buf[0], c.pat, out=L.out)
        assert total == pos.numel(), ("BMX_ERR_CAPACITY", total)
        res = [pos]
    elif c.kind == "multi":
        res = ctx.search_device_multi(L.buf[0], c.patterns, out=L.out)
    elif c.kind == "approx":
        ends, dist, total = ctx.search_approx_device(L.buf[0], c.pat, c.k, out=L.out, dist_out=L.aux)
        assert total == ends.numel(), ("BMX_ERR_CAPACITY", total)
        res = [ends, dist]
    elif c.kind == "dict":
        if L.dictionary is None or L.dictionary._ctx is not ctx:
            L.dictionary = ctx.dictionary(c.patterns)
        pos, pid, total = L.dictionary.search_device(L.buf[0], out=L.out, pid_out=L.aux)
        assert total == pos.numel(), ("BMX_ERR_CAPACITY", total)
        res = [pos, pid]
    elif c.kind == "regex_star":
        ends, total = ctx.search_regex_star_device(L.buf[0], c.expr, out=L.out)
        assert total == ends.numel(), ("BMX_ERR_CAPACITY", total)
        res = [ends]
    elif c.kind == "ed":
        return [np.array([ctx.edit_distance_device(L.buf[0], L.buf[1])], np.int64)]
    else:
        assert c.kind == "sa"
        res = [ctx.suffix_array_device(L.buf[0])]
    return [r.cpu().numpy().astype(np.int64) for r in res]


def check(got, L, what):
    want = L.want
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, (what, i, g.size, w.size)
        assert np.array_equal(g, w), (what, i)


@functools.lru_cache(maxsize=None)
def _entry_cases():
    return sc.entry_point_cases()


ENTRY_NAMES = ["search_device", "search_device_multi", "search_approx_device m<=32", "search_approx_device m>32",
               "Dictionary.search_device", "edit_distance_device", "suffix_array_device"]


def test_rig_side_stream_is_non_blocking_and_the_delay_lasts(ctx):
    """The stream flag, and the delay's own duration from a pair of events (printed; recorded in stream_cases.py)."""
    import torch

    s = side_stream()
    assert _stream_flags(s) & HIP_STREAM_NON_BLOCKING
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    delay(s)
    e1.record(s)
    assert not e1.query(), "the delay is over before the host has finished enqueuing it"
    s.synchronize()
    print(f"\nSTREAMS delay: {sc.DELAY_COPIES} copies of {sc.DELAY_BYTES >> 20} MiB take {e0.elapsed_time(e1):.2f} ms")


# ---- (a) input still being produced on the caller's stream ----------------------------------------------------------------

@pytest.mark.parametrize("which", range(7), ids=ENTRY_NAMES)
def test_input_still_being_produced_on_the_stream(which, ctx, port):
    import torch

    L = Loaded(_entry_cases()[which], port, start_with="decoy")
    if L.case.kind == "dict":
        L.dictionary = ctx.dictionary(L.case.patterns)  # (built with blocking copies: before anything is enqueued)
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s)
        L.produce()
        pending = Pending(s)
        pending.assert_outstanding(ENTRY_NAMES[which])
        got = call(ctx, L)
    check(got, L, ENTRY_NAMES[which])


def test_input_still_being_produced_prepare_enqueue_finish(ctx, port):
    import torch

    L = Loaded(_entry_cases()[0], port, start_with="decoy")
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        q = ctx.prepare(L.buf[0], L.case.pat, L.out, tables=host.build_tables(L.case.pat))  # binds the stream
        delay(s)
        L.produce()
        pending = Pending(s)
        pending.assert_outstanding("enqueue")
        q.enqueue()
        total = q.finish()
        got = [L.out[:total].cpu().numpy()]
    check(got, L, "prepare/enqueue/finish")


def test_input_still_being_generated_on_the_stream(ctx, port):
    """bmx_gen_text_device as the producer: the search is called while the generator kernel is outstanding behind the
    delay.  bmx_plant_device then plants on the same stream (it synchronises that stream itself) and the planted
    pattern is searched."""
    import torch

    raw, planted = sc.gen_case()
    spec = sc.GEN_SPEC
    L = Loaded(raw, port, start_with="decoy")
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s)
        ctx.gen_text(L.buf[0], 0, spec.seed, spec.kind)
        pending = Pending(s)
        pending.assert_outstanding("gen_text")
        check(call(ctx, L), L, "generated text")
        for layer in spec.plant_layers():
            ctx.plant(L.buf[0], 0, spec.pattern(), layer)
        L.case, L.want = planted, planted.want(port)
        check(call(ctx, L), L, "generated and planted text")
        assert np.array_equal(L.buf[0].cpu().numpy(), planted.real[0])


@pytest.mark.parametrize("which", [0, 1], ids=["real tainted, decoy untainted", "real untainted, decoy tainted"])
def test_regex_star_input_still_being_produced_on_the_stream(which, exp_ctx, port):
    """bmx_search_regex_star_device while the copy of the real text is outstanding.  Real tainted: the slow path's own
    memset, kernels, scan, copy and events must all wait behind the caller's stream; a first launch that read the decoy
    would not even be tainted.  Real untainted: a first launch that read the decoy would take the slow path."""
    import torch

    L = Loaded(sc.regex_star_cases()[which], port, start_with="decoy")
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s)
        L.produce()
        pending = Pending(s)
        pending.assert_outstanding("search_regex_star_device")
        got = call(exp_ctx, L)
    check(got, L, L.case.name)
    last = exp_ctx.regex_star_last()
    assert last["slow"] == int(which == 0) and (last["tainted"] > 0) == (which == 0), last
    assert bool((L.out[L.want[0].size:] == -1).all())


# ---- (b) output consumed on the stream -------------------------------------------------------------------------------------

def test_output_of_the_regex_star_slow_path_consumed_on_the_stream(exp_ctx, port):
    """One tainted call on the side stream behind the delay; a clone enqueued right behind it, with no synchronisation
    by the caller in between, sees the slow path's list."""
    import torch

    L = Loaded(sc.regex_star_cases()[0], port, start_with="real")
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s)
        ends, total = exp_ctx.search_regex_star_device(L.buf[0], L.case.expr, out=L.out)
        taken = L.out[:total].clone()
    s.synchronize()
    check([taken.cpu().numpy()], L, "clone behind search_regex_star_device")
    assert exp_ctx.regex_star_last()["slow"] == 1


def test_output_of_search_device_consumed_on_the_stream(ctx, port):
    """search_device polls a status word, it does not synchronise the stream: a clone enqueued right behind it sees the
    list."""
    import torch

    L = Loaded(_entry_cases()[0], port, start_with="real")
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s)
        pos, total = ctx.search_device(L.buf[0], L.case.pat, out=L.out)
        taken = L.out[:total].clone()
    s.synchronize()
    check([taken.cpu().numpy()], L, "clone behind search_device")


@pytest.mark.parametrize("overlap", [False, True], ids=["order on the stream", "order overlap"])
def test_eight_shard_slot_merge_entirely_on_the_stream(overlap, ctx, port):
    """test_eight_shard_slot_merge_in_one_process under a side stream: enqueue -> count_to_device -> finish per shard, then
    merge_gathered, and only then a synchronisation of the stream.  With bmx_set_order_overlap the ordering kernel runs
    on the context's own stream: count_to_device must still publish that kernel's count and list."""
    import torch

    world, slot = 8, 8192
    n = 40 * (1 << 20) + 4321
    per = shard.shard_bounds(n, world, 0)[1]
    spec = corpus.CorpusSpec("merge8s", n, 16, 0, 0x5EED0004, 1 << 17, per, -1)
    h_text = spec.host_text()
    want = port.search(h_text, spec.pattern())
    dev = torch.device("cuda", 0)
    d_all = torch.from_numpy(h_text).to(dev)
    gathered = torch.zeros(world * (slot + 1), dtype=torch.int64, device=dev)
    merged = torch.zeros(world * slot, dtype=torch.int64, device=dev)
    totals = torch.zeros(3, dtype=torch.int64).pin_memory()
    tables = host.build_tables(spec.pattern())
    s = side_stream()
    torch.cuda.synchronize()
    with host.Context(0) as c:
        c.set_order_overlap(overlap)
        with torch.cuda.stream(s):
            delay(s)
            for r in range(world):
                start, length, n_own = shard.shard_extent(n, spec.m, world, r)
                buf = gathered[r * (slot + 1):(r + 1) * (slot + 1)]
                q = c.prepare(d_all[start:start + length], spec.pattern(), buf[1:], n=length, n_own=n_own, base_offset=start,
                              tables=tables)
                q.enqueue()
                c.count_to_device(buf)
                if r == world - 1:  # the last shard's slot goes into the merge without the host having waited for it
                    c.merge_gathered(gathered, world, slot + 1, merged, totals, 7)
                q.finish()
            taken = merged[:want.size].clone()
        s.synchronize()
        counts = gathered[::slot + 1].cpu().numpy()
    assert int(totals[2]) == 7 and int(totals[0]) == want.size, (totals.tolist(), want.size, counts.tolist())
    assert np.array_equal(taken.cpu().numpy().astype(np.uint64), want)


# ---- (c) null stream busy, fresh context ------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(1, 7), ids=ENTRY_NAMES[1:])
def test_first_call_of_a_fresh_context_on_a_side_stream_while_the_null_stream_is_busy(which, ctx, port):
    """The first approximate / dictionary search of a context allocates and clears its look-back words and its ticket
    counter, the others their workspaces; all of it must be ordered in front of the kernels on the caller's stream,
    whatever the null stream is doing.  A second call follows after the null stream has drained."""
    import torch

    L = Loaded(_entry_cases()[which], port, start_with="real")
    s = side_stream()
    c = None
    if L.case.kind == "dict":  # bmx_dict_create uploads with blocking copies, which would drain the null stream: the
        c = host.Context(0)    # context and its dictionary exist before the delay; the SEARCH is the first one
        L.dictionary = c.dictionary(L.case.patterns)
    torch.cuda.synchronize()
    delay(null_stream())
    busy = Pending(null_stream())
    if c is None:
        c = host.Context(0)
    try:
        with torch.cuda.stream(s):
            busy.assert_outstanding(ENTRY_NAMES[which] + " (null stream)")
            got = call(c, L)
            print(f"\nSTREAMS {ENTRY_NAMES[which]}: null stream still busy after the first call: {not busy.ev.query()}")
        check(got, L, "first call")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            check(call(c, L), L, "second call")
    finally:
        if L.dictionary is not None:
            L.dictionary.close()
        c.close()


# ---- (d) one context across streams, (e) two host threads ---------------------------------------------------------------------

class SequenceRun:
    """sc.SEQUENCE on one context: everything loaded (real inputs) and every dictionary built before the first call."""

    def __init__(self, seed, port):
        self.ctx = host.Context(0)
        self.loaded = {k: Loaded(c, port, start_with="real") for k, c in sc.sequence_cases(seed).items()}
        for L in self.loaded.values():
            if L.case.kind == "dict":
                L.dictionary = self.ctx.dictionary(L.case.patterns)
        self.streams = {"A": side_stream(), "B": side_stream(), "0": null_stream()}
        self.error = None
        self.done = 0

    def run(self):
        import torch

        try:
            for key, where in sc.SEQUENCE:
                with torch.cuda.stream(self.streams[where]):
                    check(call(self.ctx, self.loaded[key]), self.loaded[key], (key, where))
                self.done += 1
        except BaseException as e:  # (reported by the test's own thread)
            self.error = e

    def close(self):
        for L in self.loaded.values():
            if L.dictionary is not None:
                L.dictionary.close()
        self.ctx.close()


def test_one_context_across_two_side_streams_and_the_null_stream(ctx, port):
    import torch

    seq = SequenceRun(0xA11CE, port)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seq.run()
    print(f"\nSTREAMS sequence of {len(sc.SEQUENCE)} calls on one thread: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    if seq.error is not None:
        raise seq.error
    assert seq.done == len(sc.SEQUENCE)
    seq.close()


def test_two_host_threads_each_with_its_own_context_and_streams(ctx, port):
    """Per-context state, the pinned words, the ticket counters and the thread-local error text are not shared: two
    threads run the sequence at once (ctypes releases the GIL during the calls), each against its own answers.  A
    thread that has not finished within the timeout is a failure, and nothing else is started on the GPU after it."""
    import torch

    seqs = [SequenceRun(0xA11CE, port), SequenceRun(0xB0B, port)]
    torch.cuda.synchronize()
    threads = [threading.Thread(target=q.run, daemon=True) for q in seqs]
    for t in threads:
        t.start()
    deadline = time.monotonic() + sc.JOIN_TIMEOUT_S
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not stuck, f"threads {stuck} did not finish within {sc.JOIN_TIMEOUT_S:.2f} s ({[q.done for q in seqs]} calls done)"
    for i, q in enumerate(seqs):
        if q.error is not None:
            raise AssertionError(f"thread {i} after {q.done} calls") from q.error
        assert q.done == len(sc.SEQUENCE)
    for q in seqs:
        q.close()


# ---- the wrap of the status words' 22-bit tag ----------------------------------------------------------------------------

WRAP_N = 128 << 10  # 8 tiles of the approximate, class-pattern, k-mismatch, gapped and regex search, 16 of the dictionary search
WRAP_PATTERN = b"ACG"
WRAP_LONG = b"GATTACAGATTACCAGGATCCAAGCTTGCATGCCTGCAGGTCGACTCTAGAGGATCCCCGGGTAC"  # 65 bytes: tiles of 128 KiB
assert len(WRAP_LONG) == 65 and WRAP_LONG[30:31] == b"T"


def _wrap_search(c, kind):
    """text -> None: one search of `kind` on context c, its whole list compared with the Python oracle."""
    import torch

    import classes_oracle as co
    from approx_oracle import approx_ends
    from dict_oracle import dict_matches

    def dev(text):
        return torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(f"cuda:{c.device}")

    def same(got, want, what):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (kind, what)

    if kind == "approx":
        def search(text):
            want_e, want_d = approx_ends(text, WRAP_PATTERN, 1)
            e, d, total = c.search_approx_device(dev(text), WRAP_PATTERN, 1, capacity=len(text))
            assert total == want_e.size > 1000
            same(e, want_e, "ends"), same(d, want_d, "distances")
        return search, lambda: None
    if kind == "classes":
        member = co.singletons(WRAP_PATTERN)

        def search(text):
            want = co.class_starts(text, member)
            pos, total = c.search_classes_device(dev(text), co.pack(member), capacity=len(text))
            assert total == want.size > 1000
            same(pos, want, "starts")
        return search, lambda: None
    if kind == "approx_long":
        def search(text):
            # four tiles: the text four times over with copies of the pattern, half of them with byte 30 replaced, at
            # places drawn from the text itself, so that the tiles' counts and prefixes differ from search to search
            import zlib

            rng = np.random.default_rng(zlib.crc32(text))
            big = bytearray(text * 4)
            at = int(rng.integers(0, 300))
            while at + len(WRAP_LONG) <= len(big):
                big[at:at + len(WRAP_LONG)] = WRAP_LONG if rng.integers(0, 2) else WRAP_LONG[:30] + b"A" + WRAP_LONG[31:]
                at += len(WRAP_LONG) + int(rng.integers(100, 600))
            big = bytes(big)
            want_e, want_d = approx_ends(big, WRAP_LONG, 1)
            e, d, total = c.search_approx_device(dev(big), WRAP_LONG, 1, capacity=len(text))
            assert total == want_e.size > 1000 and set(want_d.tolist()) == {0, 1}
            same(e, want_e, "ends"), same(d, want_d, "distances")
        return search, lambda: None
    if kind == "hamming":
        import hamming_oracle as ho

        member = co.singletons(WRAP_PATTERN)

        def search(text):
            want_s, want_d = ho.hamming_starts(text, member, 1)
            pos, d, total = c.search_hamming_device(dev(text), co.pack(member), 1, out=torch.empty(len(text), dtype=torch.int64, device=f"cuda:{c.device}"))
            assert total == want_s.size > 1000
            same(pos, want_s, "starts"), same(d, want_d, "distances")
        return search, lambda: None
    if kind == "gaps":
        import gaps_oracle as go

        member, optional = go.parse("AC?G")

        def search(text):
            want = go.gap_ends(text, member, optional)
            e, total = c.search_gaps_device(dev(text), (co.pack(member), optional), capacity=len(text))
            assert total == want.size > 1000
            same(e, want, "ends")
        return search, lambda: None
    if kind == "regex":
        import regex_oracle as ro
        from test_gpu_regex import _struct

        rx = ro.parse("A(C|GT)G")

        def search(text):
            want = ro.ends_numpy(text, rx)
            e, total = c.search_regex_device(dev(text), _struct(rx), capacity=len(text))
            assert total == want.size > 1000
            same(e, want, "ends")
        return search, lambda: None
    if kind in ("regex_star", "regex_star_slow"):
        import regex_star_oracle as so
        from test_gpu_regex import _struct

        # fast: the loop C+ dies in every warm-up of a random ACGT text (the model says so for these texts).  slow: an N
        # in place 7 and N.*ACG -- no lane's lower bound has the `.`, every upper bound keeps it: the call takes two
        # sequence numbers, the first launch's and R2's
        slow = kind == "regex_star_slow"
        rx = so.parse("N.*ACG" if slow else "AC+G")

        def search(text):
            text = text * 4  # eight tiles of 64 KiB: a star piece is 2^8 ends at the least
            if slow:
                text = text[:7] + b"N" + text[8:]
            want = so.ends_numpy(text, rx)
            waves = so.fast_taint(text, rx, 0, 0, 8, 64, walk=False).waves
            assert (waves > 0) == slow
            e, total = c.search_regex_star_device(dev(text), _struct(rx), capacity=len(text))
            assert total == want.size > 1000
            same(e, want, "ends")
            last = c.regex_star_last()
            assert last["slow"] == int(slow) and last["tainted"] == waves and last["piece_shift"] == 8, last
        return search, lambda: None
    assert kind == "dict"
    d = c.dictionary([WRAP_PATTERN])

    def search(text):
        want_p, want_i = dict_matches(text, [WRAP_PATTERN])
        pos, pid, total = d.search_device(dev(text), capacity=len(text))
        assert total == want_p.size > 1000
        same(pos, want_p, "positions"), same(pid, want_i, "pattern ids")
    return search, d.close


@pytest.mark.parametrize("kind", ["approx", "classes", "dict", "approx_long", "hamming", "gaps", "regex", "regex_star", "regex_star_slow"])
def test_tag_wrap_clears_the_status_words(exp_ctx, kind):
    """The status words of an ordered-output session carry the call's sequence number mod 2^22 and are cleared only when
    that tag wraps.  The first search leaves a tag-1 prefix in every word; "ordered_seq" then puts the next call on the
    wrap, so it takes tag 1 again: without the clear its tiles would read the first search's prefixes as their
    predecessors' (a wrong list, or BMX_ERR_HIP from the bounded wait -- never a hang).  A tainted call of the star search
    takes two sequence numbers: from 2^22 - 1 the wrap falls on its first launch, from 2^22 - 2 on R2, whose tiles would
    then read what the searches before left under the tags 1 and 2."""
    rng = np.random.default_rng(0x7A6)
    texts = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, WRAP_N)].tobytes() for _ in range(3)]
    search, close = _wrap_search(exp_ctx, kind)
    try:
        search(texts[0])
        with pytest.raises(host.BmxError):  # (BMX_ERR_ARG, as for an unknown name)
            exp_ctx.set_knob("ordered_seq", -1)
        for seq in ((1 << 22) - 1,) + (((1 << 22) - 2,) if kind == "regex_star_slow" else ()):
            exp_ctx.set_knob("ordered_seq", seq)
            search(texts[1])
            search(texts[2])
    finally:
        close()
