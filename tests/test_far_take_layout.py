"""The layout arithmetic of tests/far_take.py in Python integers (no device): every island inside the take, the three
line-crossing islands astride their lines, a byte offset truncated to 32 bits landing on OTHER signal, the control windows short
and aligned, and J31 feeding converter outputs on both sides of index 2^31."""
import numpy as np
import pytest

import far_take as FT
import resample_ref as R

UNITS = (1, 2, 147, 160, 256, 375, 512, 1024, 3000, 4410, 4800, 384000)  # 384 000 = lcm(375, 1024): the circular-window STFT plans'


def test_the_limit_and_the_image():
    assert FT.N_MAX == 2147418111 and FT.N_MAX % 2 == 1
    assert FT.IMAGE == 2 ** 31 - 1                      # the trailing pad ends exactly on the last int32 index
    assert 4 * FT.IMAGE == 8 * FT.GIB - 4
    from melonix_amd import _capi
    assert FT.PAD == _capi.MX_AUDIO_PAD


def test_islands_lie_inside_the_take_and_apart():
    spans = sorted(FT.span(name) for name in FT.STARTS)
    assert spans[0][0] >= 0 and spans[-1][1] <= FT.N_MAX
    assert FT.span("END")[1] == FT.N_MAX and FT.span("START") == (65536, 327680)
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert lo - hi >= 2 * FT.MARGIN + max(UNITS)  # no control window reaches a neighbour, whatever the unit
    for name in FT.STARTS:
        assert FT.span(name)[1] - FT.span(name)[0] == FT.ISLAND == 262144


@pytest.mark.parametrize("name", sorted(FT.LINES))
def test_line_crossing_islands_straddle_their_lines(name):
    lo, hi = FT.byte_span(name)
    line = FT.LINES[name]
    assert lo < line < hi and line - lo == hi - line == 2 * FT.ISLAND  # half of the island either side
    assert (line // 4 - FT.PAD) in range(*FT.span(name))


def test_b6g_is_four_gib_above_b2g():
    assert FT.byte_span("B6G")[0] - FT.byte_span("B2G")[0] == 4 * FT.GIB
    assert FT.STARTS["B6G"] - FT.STARTS["B2G"] == 2 ** 30


def test_j31_is_astride_the_sample_output_2_31_reads():
    lo, hi = FT.span("J31")
    assert lo < FT.J31_SAMPLE < hi and FT.J31_SAMPLE == 1973000601


def _wrapped(lo, hi):
    """Byte offsets [lo, hi) at or above 4 GiB, truncated to 32 bits -> [lo', hi') (empty where nothing wraps)"""
    lo = max(lo, 4 * FT.GIB)
    return (lo % 2 ** 32, lo % 2 ** 32 + (hi - lo)) if lo < hi else (0, 0)


def test_a_truncated_byte_offset_lands_on_other_signal():
    # from B6G: exactly B2G, sample for sample (the half below 6 GiB included: 6 GiB - x wraps to 2 GiB - x)
    lo, hi = FT.byte_span("B6G")
    assert (lo % 2 ** 32, lo % 2 ** 32 + (hi - lo)) == FT.byte_span("B2G")
    # from B4G: the half at and above 4 GiB lands on the leading pad and the take's first samples, START among them
    lo, hi = _wrapped(*FT.byte_span("B4G"))
    assert lo == 0 and hi == 2 * FT.ISLAND
    s_lo, s_hi = FT.byte_span("START")
    assert lo < s_lo < hi and hi - s_lo >= 4 * 32768   # 32 768 samples of START under the island's last 32 768
    assert 4 * FT.PAD < s_lo                            # the leading pad and the zeros before START under the rest: not B4G's bytes
    # from END: its last 65 536 samples and the whole trailing pad land inside B4G
    e_lo, e_hi = FT.byte_span("END")
    tail = (e_hi - 4 * 65536, e_hi + 4 * FT.PAD)
    assert tail[1] == 4 * FT.IMAGE
    lo, hi = _wrapped(*tail)
    b_lo, b_hi = FT.byte_span("B4G")
    assert b_lo <= lo and hi <= b_hi
    lo, hi = _wrapped(e_lo, e_hi)
    assert lo < b_lo < hi                               # (its first samples land on the zeros below B4G)
    for name, other in FT.ALIASES.items():
        assert not np.array_equal(FT.samples(name), FT.samples(other))


def test_no_two_islands_share_bytes():
    names = list(FT.STARTS)
    for i, a in enumerate(names):
        wa = FT.samples(a)
        assert wa.dtype == np.float32 and len(wa) == FT.ISLAND and np.abs(wa).max() > 0.4
        for b in names[i + 1:]:
            assert (wa != FT.samples(b)).mean() > 0.99, (a, b)


@pytest.mark.parametrize("unit", UNITS)
def test_windows_are_aligned_and_short(unit):
    for name in FT.STARTS:
        q, end = FT.window_span(name, unit)
        lo, hi = FT.span(name)
        assert q % unit == 0 and 0 <= q <= max(lo - FT.MARGIN, 0) and (q == 0 or lo - FT.MARGIN - q < unit)
        assert end == min(hi + FT.MARGIN, FT.N_MAX) and end - q <= FT.ISLAND + 2 * FT.MARGIN + unit <= 800000
    assert FT.window_span("END", unit)[1] == FT.N_MAX   # the control ends where the far take ends


def test_a_window_holds_the_island_between_zeros():
    for name, unit in (("B4G", 375), ("END", 4800), ("START", 256)):
        q, w = FT.window(name, unit)
        lo, hi = FT.span(name)
        assert len(w) == FT.window_span(name, unit)[1] - q
        assert np.array_equal(w[lo - q:hi - q], FT.samples(name)) and not w[:lo - q].any() and not w[hi - q:].any()


def test_j31_maps_to_outputs_on_both_sides_of_2_31():
    p = R.plan(44100, 48000)
    assert (p["L"], p["M"]) == (160, 147)
    lo, hi = FT.span("J31")
    for j in (2 ** 31 - 2048, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 2047):
        i, _ = R.index_map(j, p)
        assert lo + p["half"] <= i < hi - p["half"], j  # the whole window of taps inside the island
    assert R.index_map(2 ** 31, p)[0] == FT.J31_SAMPLE
    m = R.length(FT.N_MAX, p)
    assert m == 2337325836 and m > 2 ** 31             # what mx_audio_resample of the far take would have to allocate
    assert R.index_map(m - 1, p)[0] <= FT.N_MAX - 1 and R.index_map(m - 4096, p)[0] >= FT.span("END")[0] + p["half"]
