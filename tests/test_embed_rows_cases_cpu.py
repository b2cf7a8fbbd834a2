"""The lists of tests/embed_rows_cases.py have the properties that make them reach every branch of the three list forms: proved here
with numpy (a stable argsort and counts), so a case that stops reaching its branch fails without a GPU."""
import numpy as np
import pytest

import embed_rows_cases as ec

CHUNK = ec.CHUNK


def _segments(keys, pad):
    """(id, first, end) of every segment of real keys in a sorted key list"""
    out = []
    p = 0
    while p < keys.size and keys[p] != pad:
        e = p
        while e < keys.size and keys[e] == keys[p]:
            e += 1
        out.append((int(keys[p]), p, e))
        p = e
    return out


def _chunks_spanned(first, end):
    return (end - 1) // CHUNK - first // CHUNK + 1


def _shapes(keys, pad):
    segs = _segments(keys, pad)
    return {
        "three_chunks": [s for s in segs if _chunks_spanned(s[1], s[2]) >= 3],
        "one_boundary": [s for s in segs if _chunks_spanned(s[1], s[2]) == 2],
        "inside_4_rem": [s for s in segs if _chunks_spanned(s[1], s[2]) == 1 and s[2] - s[1] >= 5 and (s[2] - s[1]) % 4],
        "singletons": [s for s in segs if s[2] - s[1] == 1],
        "ends_at_n": [s for s in segs if s[2] == keys.size],
    }


@pytest.mark.parametrize("second", [False, True])
def test_short_list_reaches_every_branch_of_the_scan(second):
    ids = ec.short_ids(second=second)
    T, B = ids.shape
    assert (T, B) == (25, 8) and ids.size == 200 and ids.size < 3072
    flat = ids.reshape(-1)
    count = lambda i, mask=None: int(((flat == i) & (True if mask is None else mask)).sum())
    # without lengths: 37 positions -> quarters of 10, 10, 10, 7: none empty, a full trip of the 8-wide unroll and a remainder
    assert count(ec.SHORT_MANY) == 37
    per = -(-37 // 4)
    assert per > 8 and per % 8 and 37 - 3 * per > 0
    assert count(ec.SHORT_TWICE) == 2 and count(ec.SHORT_THRICE) == 3          # quarters of 1: two, then one, of them empty
    assert count(60 if second else ec.SHORT_ONCE) == 1
    assert int((flat < 0).sum()) == 1 and int((flat >= ec.SMALL_V).sum()) == 1 and int((flat == ec.SMALL_V).sum()) == 1
    # ragged: the id occurs at padding and at other positions, and still fills four quarters with a full trip and a remainder
    lengths = np.array(ec.SHORT_LENGTHS)
    assert lengths.size == B and lengths.max() == T and lengths.min() < T and len(set(ec.SHORT_LENGTHS)) > 2
    live = ec.live_mask(ids, lengths)
    k = count(ec.SHORT_MANY, live)
    assert 0 < k < 37 and count(ec.SHORT_MANY, ~live) == 37 - k
    per = -(-k // 4)
    assert per > 8 and per % 8 and k - 3 * per > 0
    # the first position of the id is not position 0 and the list spans several 32-bit mask words
    assert np.flatnonzero(flat == ec.SHORT_MANY)[-1] // 32 > np.flatnonzero(flat == ec.SHORT_MANY)[0] // 32
    # both widths: two dimension groups with a tail, and less than one wave
    assert ec.WIDE_D > 256 and (ec.WIDE_D - 256) % 64 == 44 and ec.NARROW_D < 64
    if second:
        first = ec.short_ids()
        a, b = set(ec.touched_rows(first, lengths, ec.SMALL_V)), set(ec.touched_rows(ids, lengths, ec.SMALL_V))
        assert a - b and b - a and a & b                                         # the catch-up meets stale and current rows


@pytest.mark.parametrize("negatives", [False, True])
def test_segment_list_reaches_every_branch_of_the_two_levels(negatives):
    ids = ec.segment_ids(negatives)
    assert ids.size == 203 and ids.size % CHUNK
    keys, order, pad = ec.sorted_keys(ids)
    assert not np.array_equal(order, np.arange(ids.size))                        # the list is not sorted already
    sh = _shapes(keys, pad)
    assert [s[0] for s in sh["three_chunks"]] == [3]
    assert [s[0] for s in sh["one_boundary"]] == [50] and sh["one_boundary"][0][1] < 192 < sh["one_boundary"][0][2]
    assert 7 in [s[0] for s in sh["inside_4_rem"]]
    assert len(sh["singletons"]) == 20
    if negatives:
        assert int((ids < 0).sum()) == ec.SEG_NEGATIVE and len(set(ids[ids < 0])) == ec.SEG_NEGATIVE
        assert int((keys == pad).sum()) == ec.SEG_NEGATIVE and not sh["ends_at_n"]
        assert sh["one_boundary"][0][2] == 203 - ec.SEG_NEGATIVE
    else:
        assert (ids >= 0).all() and [s[0] for s in sh["ends_at_n"]] == [50]
    assert ec.SEG_D > 64 and ec.SEG_D % 64


@pytest.mark.parametrize("V", [ec.SMALL_V, ec.LARGE_V])
def test_long_list_keeps_the_shapes_among_its_live_positions(V):
    ids = ec.long_ids(V)
    lengths = ec.long_lengths()
    T, B = ids.shape
    assert (T, B) == (50, 64) and ids.size == 3200 and 3072 <= ids.size <= 4096  # at the threshold: the first lengths that sort
    assert lengths.size == B and lengths.max() == T and lengths.min() < T and len(set(lengths.tolist())) > 8
    scale = V // ec.SMALL_V
    keys, order, pad = ec.sorted_keys(ids, lengths, V)
    assert pad == V
    sh = _shapes(keys, pad)
    assert 3 * scale in [s[0] for s in sh["three_chunks"]]
    assert 20 * scale in [s[0] for s in sh["one_boundary"]]
    assert 7 * scale in [s[0] for s in sh["inside_4_rem"]]
    assert len(sh["singletons"]) == 6
    live = ec.live_mask(ids, lengths)
    flat = ids.reshape(-1)
    assert int((flat[live] >= V).sum()) == 1                                     # refused by the row count, not by its sign
    assert int((flat < 0).sum()) == 1
    assert int((keys == pad).sum()) == int((~live).sum()) + 1 > 1000             # padding, the negative id, the id == V
    for i in (3, 7, 30):                                                         # ids at padding positions occur at live ones too
        assert ((flat == i * scale) & ~live).any() and ((flat == i * scale) & live).any()
    real = keys[keys != pad]
    assert real.max() < V and (int(real.max()).bit_length() > 8) == (V == ec.LARGE_V)
    assert (V - 1).bit_length() <= 8 if V == ec.SMALL_V else 8 < V.bit_length() <= 16          # one key pass, two key passes
    # the plain scatter's list names table rows only and has the same segments
    inside = ec.in_table(ids, V)
    assert inside.max() == V - 1 and (inside[inside != ids] == V - 1).all()


def test_values_are_exact_and_their_sums_round():
    x = ec.values((40, 9), 3)
    assert x.dtype == np.float32 and x.shape == (40, 9) and np.array_equal(x, ec.values((40, 9), 3))
    assert not np.array_equal(x, ec.values((40, 9), 4))
    assert (np.abs(x) >= 2.0 ** -5).all() and (np.abs(x) < 4.0).all() and (x < 0).any() and (x > 0).any()
    col = x[:, 0].astype(np.float64)
    fwd = np.float32(0)
    for v in x[:, 0]:
        fwd = np.float32(fwd + v)
    assert float(fwd) != float(col.sum())                                        # fp32 sums of these round: their order matters
    P, M, V = ec.table(5, 7, 1)
    assert (V > 0).all() and (np.abs(M) < 2.0 ** -4).all()
