"""numpy model of the split-operand dense scans (csrc/rr_dense_x3.hip, rr_dense_x3w.hip, rr_x3.h): the truncating three-way
split, the query planes rr_split_queries writes (bit for bit), the kept-term sum in float64, the stored layouts, and the
"defects" a test must be able to tell from the promised arithmetic.  tests/test_x3_model.py checks the model and the input
families on the CPU; tests/test_gpu_x3_scan_kernels.py compares the kernels with it one launch at a time.

The arithmetic (DESIGN.md "K1a'"): x = x1 + x2 + x3 with x1 = the top 16 bits of x, x2 = the top 16 bits of x - x1,
x3 = x - x1 - x2, every subtraction exact in fp32; a product of two such terms is exact in fp32; a score is the fp32
accumulation of a1q1 + a1q2 + a2q1 + a2q2 + a1q3 + a3q1 over the 384 dims (fp32 rows), of a q1 + a q2 + a q3 (bf16 rows:
the stored element is one term).  The model sums the kept terms in float64: what is left to the kernel is the roundings of
its fp32 accumulator.
"""
import numpy as np

DIM = 384
ORDER_NATURAL, ORDER_PAIR64, ORDER_WIDE_BF16 = 0, 1, 2       # RR_X3_ORDER_* (rr_x3.h)
KEPT_F32 = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1))  # (row term, query term)
KEPT_BF16 = ((1, 1), (1, 2), (1, 3))                         # the row is its own single term
SC_SENTINEL = np.uint32(0x7FC5A5A5)                          # RR_DEBUG_SC_SENTINEL
KEY_SENTINEL = np.uint32(0xFFC00001)                         # RR_DEBUG_KEY_SENTINEL
PLANE_SENTINEL = np.uint16(0x5A5A)
NEG_INF_BITS = np.uint32(0xFF800000)
NQS = (5, 16, 17, 32, 33, 64)                                # both ends of each kernel's range


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def bits(x):
    return f32(x).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def trunc16(x):
    """The top 16 bits of an fp32 number: its bf16 truncation."""
    return from_bits(bits(x) & np.uint32(0xFFFF0000))


def split3(x):
    """rr_x3_split<false> / rr_split_queries: three fp32 numbers, computed in fp32 as the kernels compute them."""
    x = f32(x)
    with np.errstate(invalid="ignore", over="ignore"):
        x1 = trunc16(x)
        r1 = (x - x1).astype(np.float32)
        x2 = trunc16(r1)
        x3 = (r1 - x2).astype(np.float32)
    return x1, x2, x3


def split3_stored(x):
    """The three terms as the MFMAs see them: only the top 16 bits of each are kept (`>> 16` into the query planes, the
    byte permute of rr_pack_hi for the rows).  That cuts nothing of x1 and x2, and of x3 only when it is an fp32
    subnormal, |x| < 2^-110."""
    return tuple(trunc16(t) for t in split3(x))


def split2(x):
    """Defect: a two-term split (x1 + x2, the third term lost)."""
    x1, x2, _ = split3_stored(x)
    return x1, x2, np.zeros_like(x1)


def round_to_bf16(x):
    """Round to nearest even onto bf16, as a bf16 index stores fp32 rows (finite values and infinities)."""
    u = bits(x).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return from_bits(r)


def slots_of(nq, fallback=False):
    """Query slots of the launch that serves nq queries: 16 rr_scan_mfma_x3, 32 rr_scan_x3w<1>, 64 rr_scan_x3w<2>; the
    fallback launches (mode 2) are rr_scan_x3w at any count."""
    return 16 if (nq <= 16 and not fallback) else 32 if nq <= 32 else 64


def order_of(slots, bf16):
    if slots == 16:
        return ORDER_NATURAL if bf16 else ORDER_PAIR64
    return ORDER_WIDE_BF16 if bf16 else ORDER_NATURAL


def plane_src(order):
    """Position i of a plane holds dim plane_src(order)[i] (rr_split_queries)."""
    i = np.arange(DIM)
    e = i & 31
    if order == ORDER_PAIR64:
        kg, j = e >> 3, e & 7
        return (i & ~31) + np.where(j < 4, 4 * kg + j, 16 + 4 * kg + (j - 4))
    if order == ORDER_WIDE_BF16:
        v, h, j = e >> 4, (e >> 3) & 1, e & 7
        return (i & ~31) + 16 * h + 8 * v + j
    return i


def planes(Q, slots, order):
    """planes[3][slots][384] uint16 as rr_split_queries leaves them for the queries Q (zero rows fill the slots)."""
    Qp = np.zeros((slots, DIM), dtype=np.float32)
    Qp[:len(Q)] = Q
    src = plane_src(order)
    return np.stack([(bits(t[:, src]) >> 16).astype(np.uint16) for t in split3(Qp)])


def kept_sum(A, Q, bf16_rows, drop=None, two_term=False):
    """float64 [nq][n]: the sum of the kept partial products, every product exact.  A: the STORED rows as fp32 values.
    drop = (i, j): that kept term left out; two_term: both operands split in two.  Non-finite elements give NaN as in the
    kernels (inf - inf in the split, inf * 0 with a zero query term)."""
    sp = split2 if two_term else split3_stored
    qt = [t.astype(np.float64) for t in sp(Q)]
    at = [f32(A).astype(np.float64)] * 3 if bf16_rows else [t.astype(np.float64) for t in sp(A)]
    out = np.zeros((len(Q), len(A)))
    with np.errstate(invalid="ignore", over="ignore"):
        for (i, j) in (KEPT_BF16 if bf16_rows else KEPT_F32):
            if drop == (i, j):
                continue
            out = out + qt[j - 1] @ at[i - 1].T
    return out


def defects(bf16_rows):
    """name -> kwargs of kept_sum for every defect the one-product cases must catch."""
    d = {f"no a{i}q{j}": dict(drop=(i, j)) for (i, j) in (KEPT_BF16 if bf16_rows else KEPT_F32)}
    d["two-term split"] = dict(two_term=True)
    return d


def canon(s, n_rows=None):
    """rr_x3_canon on float32 scores: NaN -> -inf."""
    s = f32(s).copy()
    s[np.isnan(s)] = -np.inf
    return s


def f2key(f):
    u = bits(f)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ---- layouts (rr_dense.h).  QN = query slots, every index in 4-byte words.
def decode_sims(words, n_pad, QN):
    """Stored scores [row / 16][QN][16] -> [QN][n_pad] (uint32 bits)."""
    return np.ascontiguousarray(words[:QN * n_pad].reshape(n_pad // 16, QN, 16).transpose(1, 0, 2)).reshape(QN, n_pad)


def decode_mtile_max(words, n_tiles, QN, mm_pairs):
    """M-tile maxima of the normal scan -> [QN][4 n_tiles] (one per 16 rows): [tile][QN][4] (rr_scan_mfma_x3) or
    [32-row tile][QN][2] (rr_scan_x3w, mm_pairs = 1)."""
    per = 2 if mm_pairs else 4
    w = words[:4 * n_tiles * QN].reshape(4 * n_tiles // per, QN, per)
    return np.ascontiguousarray(w.transpose(1, 0, 2)).reshape(QN, 4 * n_tiles)


def decode_tile_max(words, n_tiles, QN):
    """Tile maxima of the stored pass [tile][QN] -> [QN][n_tiles]."""
    return np.ascontiguousarray(words[:n_tiles * QN].reshape(n_tiles, QN).T)


def decode_keys(words, n_waves, QN):
    """Group keys [wave][QN] -> [QN][n_waves]."""
    return np.ascontiguousarray(words[:n_waves * QN].reshape(n_waves, QN).T)


def maxima_of(scores, n_tiles, tiles_per_wave, n_waves):
    """From stored scores [QN][n_pad] (float32, canonical): the 16-row maxima, the 64-row maxima and the group keys."""
    QN = scores.shape[0]
    m16 = scores.reshape(QN, 4 * n_tiles, 16).max(axis=2)
    m64 = scores.reshape(QN, n_tiles, 64).max(axis=2)
    keys = np.empty((QN, n_waves), dtype=np.uint32)
    for w in range(n_waves):
        keys[:, w] = f2key(m64[:, w * tiles_per_wave:min((w + 1) * tiles_per_wave, n_tiles)].max(axis=1))
    return m16, m64, keys


# ---- input families
def mantissas(rng, shape):
    """fp32 numbers in [1, 2) whose three 8-bit fields all carry weight: the top bit of the second and of the third field
    (the 9th and 17th significant bit) is set, so x2 >= 2^-9 x and x3 >= 2^-17 x; everything else is random."""
    m = rng.integers(0, 1 << 23, size=shape, dtype=np.uint32) | np.uint32(1 << 15) | np.uint32(1 << 7)
    return from_bits(np.uint32(0x3F800000) | m)


def signs(rng, shape):
    return rng.choice(np.float32([-1.0, 1.0]), size=shape)


def pow2(rng, shape, lo, hi):
    return np.ldexp(np.float32(1.0), rng.integers(lo, hi + 1, size=shape)).astype(np.float32)


ONEHOT_ROWS = DIM + 83       # every dim once and 83 twice: ragged last 16-, 32- and 64-row tile


def one_hot(values):
    """Row k = values[k] at dim k mod 384, zero elsewhere."""
    A = np.zeros((len(values), DIM), dtype=np.float32)
    A[np.arange(len(values)), np.arange(len(values)) % DIM] = values
    return A


def fill_i(nq, seed):
    """Rows +-2^e, queries full mantissas: score = +-2^e q_k, exact (pins a1q1, a1q2, a1q3 and the k order)."""
    rng = np.random.default_rng(seed)
    v = signs(rng, ONEHOT_ROWS) * pow2(rng, ONEHOT_ROWS, -20, 20)
    Q = signs(rng, (nq, DIM)) * mantissas(rng, (nq, DIM)) * pow2(rng, (nq, DIM), -20, 20)
    return one_hot(v), f32(Q)


def fill_ii(nq, seed):
    """Rows full mantissas (fp32 storage), queries +-2^e at every dim: the mirror product (pins a2q1, a3q1)."""
    rng = np.random.default_rng(seed)
    v = signs(rng, ONEHOT_ROWS) * mantissas(rng, ONEHOT_ROWS) * pow2(rng, ONEHOT_ROWS, -20, 20)
    Q = signs(rng, (nq, DIM)) * pow2(rng, (nq, DIM), -20, 20)
    return one_hot(f32(v)), f32(Q)


def fill_iii(nq, seed):
    """Rows and queries 1 + 2^-9: score = 1 + 2^-8 + 2^-18 (pins a2q2) on fp32 rows."""
    v = np.full(ONEHOT_ROWS, 1 + 2.0 ** -9, dtype=np.float32)
    return one_hot(v), np.full((nq, DIM), 1 + 2.0 ** -9, dtype=np.float32)


def fill_b(nq, seed):
    """One product per output, full mantissas on both sides, exponents uniform over +-40."""
    rng = np.random.default_rng(seed)
    v = signs(rng, ONEHOT_ROWS) * mantissas(rng, ONEHOT_ROWS) * pow2(rng, ONEHOT_ROWS, -40, 40)
    Q = signs(rng, (nq, DIM)) * mantissas(rng, (nq, DIM)) * pow2(rng, (nq, DIM), -40, 40)
    return one_hot(f32(v)), f32(Q)


# Case b's bar, relative to |a_k q_k|.  Dropped terms: with a, q in [1, 2) the fields are a2 <= 2^-7 - 2^-15,
# a3 <= 2^-15 - 2^-23 (same for q), so a2q3 + a3q2 + a3q3 <= 2 * 2^-22 (1 - 2^-8)^2 + 2^-30 < 2^-21 a q.  Accumulator: the six
# exact partial products enter one fp32 accumulator, each addition rounds to nearest (<= 2^-24 of a partial sum that is
# no larger than a q (1 + 2^-7)): 6 * 2^-24 * (1 + 2^-7).  bf16 rows drop nothing; the same bar is kept for them.
ONE_PRODUCT_BAR = 2.0 ** -21 + 6 * 2.0 ** -24 * (1 + 2.0 ** -7)


def unit_rows(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, DIM))
    return f32(A / np.linalg.norm(A, axis=1, keepdims=True))


def dense_queries(nq, seed):
    rng = np.random.default_rng(seed + 7919)
    Q = rng.standard_normal((nq, DIM))
    Q = np.where(np.abs(Q) < 0.01, 0.01, Q)                 # (the cancelling rows divide by the entries)
    return f32(Q / np.linalg.norm(Q, axis=1, keepdims=True))


def dense_rows(kind, n, Q, seed):
    """The data sets of the float64 comparison: unit rows; "wide": per-row scale 10^U(-12, 12) with a tenth of the entries
    at 10^U(-9, -4) of the row's scale; "cancelling": row r built against query r mod nq so that sum a_k q_k ~ 0 at
    sum |a_k q_k| = 1."""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        return unit_rows(n, seed)
    if kind == "wide":
        A = rng.standard_normal((n, DIM)) * 10.0 ** rng.uniform(-12, 12, size=(n, 1))
        small = rng.random((n, DIM)) < 0.1
        return f32(np.where(small, A * 10.0 ** rng.uniform(-9, -4, size=(n, DIM)), A))
    assert kind == "cancelling"
    s = np.tile(np.float64([1.0, -1.0]), DIM // 2)
    A = np.empty((n, DIM))
    for r in range(n):
        A[r] = rng.permutation(s) / (DIM * Q[r % len(Q)].astype(np.float64))
    return f32(A)


DENSE_KINDS = ("unit", "wide", "cancelling")
DENSE_SHAPES = (64, 65, 79, 80, 127, 129, 1000)


def rel_error(got, A, Q):
    """max |got - float64| / sum |a_k q_k| over all (query, row) pairs; A = the stored rows."""
    A64, Q64 = f32(A).astype(np.float64), f32(Q).astype(np.float64)
    ref, mag = Q64 @ A64.T, np.abs(Q64) @ np.abs(A64).T
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / mag).max())


def f32_matvec(A, Q):
    """The yardstick: numpy's float32 product on the same data."""
    return f32(Q) @ f32(A).T


# ---- case d: maxima and groups
MAXIMA_ROWS = 2000 + 13      # 32 tiles of 64 (the last one ragged: 29 rows, its last M-tile 13 rows)


def maxima_matrix(seed=5):
    """Unit rows; see maxima_plants for what is planted on top."""
    return unit_rows(MAXIMA_ROWS, seed)


def maxima_plants(A, Q, tiles_per_wave):
    """Plants, for query 0 .. 3, a copy of the (unit) query scaled by 2 -- a score of about 2, above every other -- into:
    query 0: the first M-tile of group 1's run; query 1: the last M-tile of group 0's run; query 2: the ragged last M-tile;
    query 3: two M-tiles of one group (a tie between two M-tiles, the same row bits).  Returns the planted rows."""
    A = A.copy()
    C = tiles_per_wave
    rows = {0: [C * 64 + 3], 1: [C * 64 - 1], 2: [MAXIMA_ROWS - 1], 3: [5, 16 + 9]}
    for q, rr in rows.items():
        for r in rr:
            A[r] = 2 * Q[q]
    return A, rows


# ---- case e: rescoring lists
def rescore_lists(n_rows, nq, cap=24):
    """mtiles[nq][cap], count, fb: query 0 the ragged last M-tile first, then both halves of 32-row tiles; query 1 repeats;
    query 2 count = 0; query 3 fb = 1; query 4 a full list; the rest one M-tile each."""
    n_mt = (n_rows + 15) // 16
    mt = np.full((nq, cap), 0xFFFFFFFF, dtype=np.uint32)     # (unlisted slots: never read)
    count = np.zeros(nq, dtype=np.int32)
    fb = np.zeros(nq, dtype=np.int32)
    lists = {0: [n_mt - 1, 0, 1, 2, 3, n_mt - 2, 5], 1: [4, 4, 4, n_mt - 1, n_mt - 1, 7, 4], 2: [], 3: [1, 2, 3],
             4: [(3 * i + 1) % n_mt for i in range(cap)]}
    for q in range(nq):
        l = lists.get(q, [(q * 5) % n_mt])
        mt[q, :len(l)] = l
        count[q] = len(l)
    fb[3] = 1
    return mt, count, fb


def rescore_expected(stored_bits, n_rows, mt, count, fb):
    """sc[nq][cap][16] uint32: the stored scores (bits, [QN][n_pad]) of the listed M-tiles' rows, -inf past n_rows, the
    sentinel for unlisted slots and flagged queries."""
    nq, cap = mt.shape
    exp = np.full((nq, cap, 16), SC_SENTINEL, dtype=np.uint32)
    for q in range(nq):
        if fb[q]:
            continue
        for s in range(count[q]):
            r0 = int(mt[q, s]) * 16
            for i in range(16):
                exp[q, s, i] = stored_bits[q, r0 + i] if r0 + i < n_rows else NEG_INF_BITS
    return exp


# ---- case f: non-finite rows
NONFINITE_ROWS = 1000 + 13


def nonfinite_matrix(kinds=("nan", "+inf", "-inf", "+-inf", "overflow"), n=NONFINITE_ROWS, seed=11):
    """Unit rows with, in full tiles and in the ragged last one: a NaN element; a +inf element; a -inf element; +inf and -inf
    in one row; a finite element (+-3e38 at dim 0) whose product with the queries' element 0 (nonfinite_queries) overflows.  Returns the matrix and {kind: rows}."""
    A = unit_rows(n, seed)
    where = {"nan": [7, 300, n - 2], "+inf": [20, 64 * 5 + 63, n - 1], "-inf": [33, 500, n - 4], "+-inf": [70, n - 6],
             "overflow": [100, 640, n - 8]}
    rows = {}
    for k in kinds:
        rows[k] = where[k]
        for i, r in enumerate(where[k]):
            d = (37 * r + 11 * i) % DIM
            if k == "nan":
                A[r, d] = np.nan
            elif k == "+inf":
                A[r, d] = np.inf
            elif k == "-inf":
                A[r, d] = -np.inf
            elif k == "+-inf":
                A[r, d], A[r, (d + 5) % DIM] = np.inf, -np.inf
            else:
                A[r, 0] = 3.0e38 if i % 2 == 0 else -3.0e38
    return A, rows


def nonfinite_queries(nq, seed=2):
    """Unit queries with element 0 raised to 1.5: times the +-3e38 of the overflow rows that is beyond fp32."""
    Q = dense_queries(nq, seed)
    Q[:, 0] = 1.5
    return Q
