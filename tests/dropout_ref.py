"""NumPy restatement of the dropout mask contract (include/vtx_dropout.h, vtx_dropout_rows), written from the contract alone:
Philox4x32-10 on uint64 arrays, the keep mask of a launch, and the float32 value with one rounding on the store."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or ints) holding 32-bit words, key: two 32-bit ints -> four uint64 arrays of 32-bit words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                      # 32 x 32 bits: fits uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def threshold(p):
    """floor(p * 2^32) in Python integers (p is a binary fraction: the product is exact)."""
    from fractions import Fraction
    return int(Fraction(float(p)) * (1 << 32))


def keep_scale(p):
    return np.float32(0) if float(p) == 1.0 else np.float32(1) / np.float32(1 - float(p))


def words(seed, site, e0, rows, D):
    """The 32-bit word of every element (m, c) of a rows x D launch, as uint64 [rows, D]."""
    e = np.uint64(e0) + np.arange(rows * D, dtype=np.uint64)
    q = np.unique(e >> np.uint64(2))
    out = philox4x32_10((q & MASK32, q >> np.uint64(32), np.full(q.shape, site, np.uint64), np.zeros(q.shape, np.uint64)),
                        (seed & 0xFFFFFFFF, seed >> 32))
    table = np.stack(out, axis=1)                      # [counters, 4]
    idx = ((e >> np.uint64(2)) - q[0]).astype(np.int64)
    return table[idx, (e & np.uint64(3)).astype(np.int64)].reshape(rows, D)


def keep_mask(seed, site, e0, rows, D, p):
    """bool [rows, D]: True where the element is kept (dropped iff word < floor(p * 2^32))."""
    return words(seed, site, e0, rows, D) >= np.uint64(threshold(p))


def to_bf16_bits(x32):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even (no NaN in the tests' data)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
    return (u >> np.uint64(16)).astype(np.uint16)


def bf16_round(x32):
    return (to_bf16_bits(x32).astype(np.uint32) << np.uint32(16)).view(np.float32)


def apply(x, seed, site, p, e0=0, pre=None, s=None, post=None, bf16=False):
    """x [rows, D] float32 (for bf16: values that are bf16 numbers).  pre [rows, D] float32 (already gathered per row), s [rows]
    float32, post [rows, D] float32, all optional.  t = x [+ pre]; t = kept ? t * scale : +0; t = t * s; t = t + post -- each
    a float32 operation -- then the store's rounding."""
    x = np.asarray(x, dtype=np.float32)
    rows, D = x.shape
    keep = keep_mask(seed, site, e0, rows, D, p)
    t = x if pre is None else (x + np.asarray(pre, np.float32)).astype(np.float32)
    t = np.where(keep, (t * keep_scale(p)).astype(np.float32), np.float32(0))
    if s is not None:
        t = (t * np.asarray(s, np.float32)[:, None]).astype(np.float32)
    if post is not None:
        t = (t + np.asarray(post, np.float32)).astype(np.float32)
    return bf16_round(t) if bf16 else t
