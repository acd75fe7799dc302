"""CPU suite for tests/stream_cases.py: for every case of the stream-ordering tests (tests/test_gpu_streams.py) the
oracle's answer for the DECOY differs from its answer for the REAL input -- a kernel that read the buffer before the
caller's stream had produced it cannot pass -- and the window oracles of the two large cases equal the oracle on the
whole text.  No call into the library is made here."""
import numpy as np

import stream_cases as sc
from approx_oracle import approx_ends
from dict_oracle import dict_matches


def _differs(case, port):
    real, decoy = case.want(port, "real"), case.want(port, "decoy")
    assert all(r.shape == d.shape for r, d in zip(case.real, case.decoy)), case.name
    assert not any(np.array_equal(r, d) for r, d in zip(case.real, case.decoy)), case.name
    assert not sc.same(real, decoy), case.name
    assert sum(a.size for a in real) > 0, case.name  # the real answer is not the empty list a cleared buffer gives
    return real, decoy


def test_entry_point_cases_decoy_answers_differ(port):
    cases = sc.entry_point_cases()
    assert [c.kind for c in cases] == ["scan", "multi", "approx", "approx", "dict", "ed", "sa"]
    assert [len(c.pat) > 32 for c in cases if c.kind == "approx"] == [False, True]  # both word widths
    for case in cases:
        real, decoy = _differs(case, port)
        if case.kind == "multi":  # every pattern's list differs, not only one
            assert all(r.size > 0 and not np.array_equal(r, d) for r, d in zip(real, decoy))
        if case.kind == "approx":  # ends of several distances
            assert len(set(real[1].tolist())) > 1
        if case.kind == "dict":  # several patterns at work
            assert len(set(real[1].tolist())) > 20


def test_edit_distance_one_stale_operand_changes_the_distance(port):
    for case in (sc.ed_case(0x57A), sc.ed_case(0x57A, 3000, 2500)):
        (a, b), (a2, b2) = case.real, case.decoy
        want = int(case.want(port)[0][0])
        assert port.edit_distance(a, b2) != want and port.edit_distance(a2, b) != want
        # the decoy's b is a's head with at most 300 substitutions; two unrelated strings are much further apart
        assert int(case.want(port, "decoy")[0][0]) <= (a.size - b.size) + 300 < want


def test_generated_corpus_cases(port):
    raw, planted = sc.gen_case()
    real, _ = _differs(raw, port)
    assert real[0].size > 100
    real, decoy = _differs(planted, port)
    assert real[0].size >= sc.GEN_SPEC.n >> 14 and decoy[0].size == 0  # the planted pattern is not in the unplanted text


def test_sequence_cases_decoy_answers_differ_for_both_threads(port):
    streams = {}
    for key, s in sc.SEQUENCE:
        streams.setdefault(key.split("_")[0].rstrip("0123456789"), set()).add(s)
    assert all(len(v) >= 2 for v in streams.values()), streams  # every algorithm on more than one stream
    answers = []
    for seed in (0xA11CE, 0xB0B):
        cases = sc.sequence_cases(seed)
        assert {k for k, _ in sc.SEQUENCE} == set(cases)
        for case in cases.values():
            _differs(case, port)
        answers.append({k: c.want(port) for k, c in cases.items()})
    # the two threads have answers of their own: a result that landed in the other context's buffers shows
    for key in answers[0]:
        if key != "scan_dense":  # (one byte all through: the same for both)
            assert not sc.same(answers[0][key], answers[1][key]), key


def test_regex_star_cases_differ_and_taint_as_claimed(port):
    """The star search's two cases: the decoy's answer differs, and at the rule's geometry for this size (pieces of 2^8
    ends, a warm-up of 64 bytes, an aligned buffer) the model of the first launch taints the one text in (nearly) every
    wave and the other in none."""
    import regex_star_oracle as so

    cases = sc.regex_star_cases()
    assert [c.kind for c in cases] == ["regex_star", "regex_star"]
    rx = so.parse(sc.STAR_EXPR)
    waves = []
    for case in cases:
        real, decoy = _differs(case, port)
        assert real[0].size > 5000 and decoy[0].size > 5000
        waves.append(so.fast_taint(case.real[0].tobytes(), rx, 0, 0, 8, 64, walk=False).waves)
    n_waves = -(-sc.STAR_N // (64 << 8))
    assert waves[0] >= n_waves - 1 and waves[1] == 0, (waves, n_waves)
    assert np.array_equal(cases[0].real[0], cases[1].decoy[0]) and np.array_equal(cases[0].decoy[0], cases[1].real[0])
    assert 5 * (256 << 8) > sc.STAR_N > 4 * (256 << 8)  # five tiles: the slow path's kernels run several workgroups' worth of pieces


def test_large_cases_windows_hold_every_hit():
    a = sc.approx_big_case(0xA11CE)
    for which, text in (("real", a.real[0]), ("decoy", a.decoy[0])):
        e, d = approx_ends(text.tobytes(), a.pat, a.k)
        got = a.want(None, which)
        assert np.array_equal(got[0], e) and np.array_equal(got[1], d)
    assert lc_tiles(a.real[0].size, 16384) > 1024
    b = sc.dict_big_case(0xA11CE)
    for which, text in (("real", b.real[0]), ("decoy", b.decoy[0])):
        p, i = dict_matches(text.tobytes(), b.patterns)
        got = b.want(None, which)
        assert np.array_equal(got[0], p) and np.array_equal(got[1], i)
    assert lc_tiles(b.real[0].size, 8192) > 1024


def lc_tiles(n: int, tile: int) -> int:
    return (n + tile - 1) // tile
