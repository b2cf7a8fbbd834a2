"""The id lists and inputs of tests/golden/gen_embed_rows_bits.py: the smallest lists that reach every branch of the three list forms
of the embedding-rows code (short: one workgroup per position; sort: stable radix sort + two-level list-order sums; the presorted form
runs the same two levels).  Literals plus exact integer formulas of the element index, so nothing large is stored; numpy only.
tests/test_embed_rows_cases_cpu.py proves, without a GPU, that every list has the properties claimed here.

Positions are p = t * B + b; with `lengths`, position p is padding when t >= lengths[b]."""
import numpy as np

CHUNK = 64                       # the sorted list is cut into runs at multiples of this (level 1), level 2 adds a segment's runs
SMALL_V, LARGE_V = 120, 20000    # table rows; the sort walks one 8-bit key pass for the first and two for the second
WIDE_D, NARROW_D = 300, 7        # 300: two dimension groups of the short form, the second with a tail of 44; 7: less than a wave
SEG_D = 70                       # the segment sum's width: a lane's second trip has a tail of 6

# ---- short form: n = 200 (T = 25, B = 8)
SHORT_T, SHORT_B = 25, 8
SHORT_LENGTHS = (25, 17, 9, 25, 3, 21, 12, 25)
SHORT_MANY = 5                   # the id that occurs 37 times: 33 times in the full columns 0, 3, 7 and 4 times at padding positions
SHORT_ONCE, SHORT_TWICE, SHORT_THRICE = 100, 101, 102


def short_ids(V=SMALL_V, second=False):
    """(T, B) int64.  second: another list over other rows as well (the deferred case catches it up)"""
    T, B = SHORT_T, SHORT_B
    p = np.arange(T * B, dtype=np.int64)
    ids = 10 + (p * 7 + p // B) % 8 + (20 if second else 0)           # eight filler ids, about 19 positions each
    ids = ids.reshape(T, B)
    for k in range(33):
        ids[(2 * k) % 25, (0, 3, 7)[k % 3]] = SHORT_MANY
    for t, b in ((24, 4), (20, 2), (24, 1), (23, 6)):                   # t >= SHORT_LENGTHS[b]
        ids[t, b] = SHORT_MANY
    ids[1, 0] = SHORT_ONCE
    ids[3, 3] = ids[5, 5] = SHORT_TWICE
    ids[7, 7] = ids[9, 0] = ids[11, 3] = SHORT_THRICE
    ids[13, 0] = -1
    ids[15, 3] = V                                                      # the first id that is no table row
    if second:
        ids[ids == SHORT_ONCE] = 60
    return np.ascontiguousarray(ids)


# ---- sort form, n = 203: the sorted list as (id, count) in ascending id order
#   id 3   [0, 150)    three chunks: level 2 adds three partials
#   id 7   [150, 155)  inside one chunk, a trip of four and a remainder of one
#   10..29 [155, 175)  singletons
#   id 40  [175, 185)  inside one chunk
#   id 50  [185, 203)  crosses the boundary at 192 and ends at n
SEG_N = 203
SEG_COUNTS = ((3, 150), (7, 5)) + tuple((i, 1) for i in range(10, 30)) + ((40, 10), (50, 18))
SEG_NEGATIVE = 6                 # in the second list the last six positions of id 50 (list order) hold -1, -2, ...: [185, 197), pads behind


def segment_ids(negatives):
    """(203,) int64: SEG_COUNTS spread over the list by a fixed permutation"""
    srt = np.concatenate([np.full(c, i, dtype=np.int64) for i, c in SEG_COUNTS])
    assert srt.size == SEG_N
    ids = np.empty(SEG_N, dtype=np.int64)
    ids[(np.arange(SEG_N) * 89 + 17) % SEG_N] = srt
    if negatives:
        where = np.flatnonzero(ids == 50)[-SEG_NEGATIVE:]
        ids[where] = -1 - np.arange(SEG_NEGATIVE)
    return ids


# ---- sort form, n = 3200 (T = 50, B = 64), ragged: the same shapes among the non-padding positions
LONG_T, LONG_B = 50, 64
LONG_COUNTS = ((3, 150), (7, 5)) + tuple((i, 1) for i in range(8, 14)) + ((20, 40),)       # [0,150) [150,155) [155,161) [161,201)
LONG_FILL = tuple(range(30, 40))                                                           # the rest, in equal shares


def long_lengths():
    b = np.arange(LONG_B)
    return np.where(b % 4 == 0, LONG_T, 5 + (b * 11) % 46).astype(np.int32)


def long_ids(V):
    """(T, B) int64 for a table of V rows: the ids of LONG_COUNTS / LONG_FILL times V // 120, so the large table's ids need two key
    bytes; one negative id and one id == V among the non-padding positions; padding positions repeat ids that also occur elsewhere"""
    T, B = LONG_T, LONG_B
    scale = V // SMALL_V
    lengths = long_lengths()
    p = np.arange(T * B)
    live = np.flatnonzero((p // B) < lengths[p % B])
    m = live.size
    head = np.concatenate([np.full(c, i, dtype=np.int64) for i, c in LONG_COUNTS])
    rest = m - head.size - 2
    fill = np.repeat(np.array(LONG_FILL, dtype=np.int64), -(-rest // len(LONG_FILL)))[:rest]
    srt = np.concatenate([head, fill]) * scale
    srt = np.concatenate([srt, np.array([-1, V], dtype=np.int64)])
    assert srt.size == m
    ids = (np.array((3, 30, 7), dtype=np.int64) * scale)[p % 3]             # padding positions
    mult = 1237
    assert np.gcd(mult, m) == 1
    ids[live[(np.arange(m) * mult + 5) % m]] = srt
    return np.ascontiguousarray(ids.reshape(T, B))


def in_table(ids, V):
    """the list for the plain scatter-add, which has no row count to refuse an id by: ids >= V become V - 1"""
    return np.where(ids >= V, V - 1, ids)


# ---- what the kernels make of a list (numpy)
def live_mask(ids, lengths=None):
    """False at padding positions and negative ids"""
    flat = ids.reshape(-1)
    ok = flat >= 0
    if lengths is not None:
        B = len(lengths)
        p = np.arange(flat.size)
        ok &= (p // B) < np.asarray(lengths)[p % B]
    return ok


def sorted_keys(ids, lengths=None, V=None):
    """(keys, positions) of the stable sort: padding, negative ids and ids >= V (V given) take the pad key and go last"""
    flat = ids.reshape(-1)
    pad = np.int64(V if V is not None else 0xFFFFFFFF)
    ok = live_mask(ids, lengths) & (flat < pad)
    keys = np.where(ok, flat, pad)
    order = np.argsort(keys, kind="stable")
    return keys[order], order, pad


def touched_rows(ids, lengths=None, V=None):
    flat = ids.reshape(-1)
    ok = live_mask(ids, lengths)
    if V is not None:
        ok &= flat < V
    return np.unique(flat[ok])


# ---- values: exact integer formulas of the element index (the same bits from any numpy)
def _hash(i, mul, add):
    return ((i * np.uint64(mul) + np.uint64(add)) % np.uint64(4294967296)) >> np.uint64(7)


def values(shape, salt, lo_exp=-5, span=7, signed=True):
    """fp32 of full 24-bit mantissas, |x| in [2^lo_exp, 2^(lo_exp + span)): sums of them round, so the order of a sum shows in its bits"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    mant = (_hash(i, 2654435761, 2 * salt + 1) % np.uint64(1 << 23) + np.uint64(1 << 23)).astype(np.float32)      # exact: < 2^24
    expo = lo_exp - 23 + (_hash(i, 2246822519, 3 * salt + 2) % np.uint64(span)).astype(np.int64)
    x = np.ldexp(mant, expo.astype(np.int32)).astype(np.float32)
    if signed:
        x = np.where(_hash(i, 3266489917, 5 * salt + 3) % np.uint64(2) == 0, x, -x)
    return np.ascontiguousarray(x.reshape(shape), dtype=np.float32)


def table(V, D, salt):
    """P, M, V of a table: weights in +-[2^-5, 4), first moments in +-[2^-9, 2^-4), second moments in [2^-16, 2^-8)"""
    return (values((V, D), salt), values((V, D), salt + 1, lo_exp=-9, span=5), values((V, D), salt + 2, lo_exp=-16, span=8, signed=False))


def grad_rows(n, D, salt):
    """gradient rows in +-[2^-5, 4): scaled by 0.05 a single row stays under the clamp at 1, elements of a long segment's sum reach it"""
    return values((n, D), salt)
