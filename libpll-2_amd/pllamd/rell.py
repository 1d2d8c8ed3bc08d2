"""The replicate weights of pll_gpu_draw_replicate_weights / pll_gpu_quartet_rell_loglikelihoods, restated in integer
arithmetic. THIS FILE IS THE SPECIFICATION: the device equals it bit for bit.

The partition has pattern weights p[0..sites), total = sum p (0 < total < 2^32), cdf[n] = p[0] + ... + p[n]. Replicate b
(an absolute number) is `total` draws; draw j of replicate b

  1. takes the 64-bit word x(seed, b, j): Philox-4x32-10 with key (seed & 0xFFFFFFFF, seed >> 32) over the counter
     (j >> 1, 0, b, TAG) gives four 32-bit words o[0..3]; an even j takes x = o[1] * 2^32 + o[0], an odd j
     x = o[3] * 2^32 + o[2];
  2. forms r = floor(x * total / 2^64), the high half of the 64 x 64-bit product;
  3. increments w_b[n] for the first n with cdf[n] > r.

Nothing is carried from draw to draw: row b is a function of (seed, b, p) and of nothing else. A pattern of weight 0 is
never drawn, every row adds up to `total`, and pattern n is drawn with probability p[n] / total up to total / 2^64.

numpy uint64 holds every intermediate: a 32 x 32-bit product fits, and x * total is formed from the two halves of x
(total < 2^32), so no step relies on wrap-around other than the stated masks."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # Philox-4x32 round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # ... and key increments (Weyl sequence)
TAG = 0x52454C4C                 # "RELL": the counter's domain word, so that other uses of the seed draw other streams
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or scalars) of 32-bit values, key: two ints; the four output words as uint64 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def draw_words(seed, b, total):
    """x(seed, b, j) for j = 0 .. total - 1, as (high, low) 32-bit halves in uint64 arrays"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    j = np.arange(total, dtype=np.uint64)
    o = philox4x32_10((j >> np.uint64(1), 0, int(b) & 0xFFFFFFFF, TAG), (seed & 0xFFFFFFFF, seed >> 32))
    odd = (j & np.uint64(1)).astype(bool)
    return np.where(odd, o[3], o[1]), np.where(odd, o[2], o[0])


def scaled(high, low, total):
    """floor((high * 2^32 + low) * total / 2^64) for total < 2^32"""
    t = np.uint64(total)
    return (high * t + ((low * t) >> S32)) >> S32


def replicate_weights(pattern_weights, seed, first, replicates):
    """rows [first, first + replicates) of the definition: uint32 [replicates][sites]"""
    p = np.ascontiguousarray(pattern_weights, dtype=np.uint32).reshape(-1)
    cdf = np.cumsum(p.astype(np.uint64), dtype=np.uint64)
    total = int(cdf[-1]) if len(cdf) else 0
    if not 0 < total < 2 ** 32:
        raise ValueError("the pattern weights must add up to a value in [1, 2^32)")
    out = np.zeros((int(replicates), len(p)), dtype=np.uint32)
    for k in range(int(replicates)):
        high, low = draw_words(seed, int(first) + k, total)
        r = scaled(high, low, total)
        n = np.searchsorted(cdf, r, side="right")  # the first n with cdf[n] > r
        out[k] = np.bincount(n, minlength=len(p)).astype(np.uint32)
    return out


def replicate_weights_slow(pattern_weights, seed, first, replicates):
    """the same in Python ints, draw by draw, with a linear search - what replicate_weights is tested against"""
    p = [int(x) for x in pattern_weights]
    total = sum(p)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros((int(replicates), len(p)), dtype=np.uint32)
    for k in range(int(replicates)):
        for j in range(total):
            c = [j >> 1, 0, (int(first) + k) & 0xFFFFFFFF, TAG]
            k0, k1 = seed & 0xFFFFFFFF, seed >> 32
            for _ in range(10):
                p0, p1 = M0 * c[0], M1 * c[2]
                c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
                k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
            x = (c[3] << 32 | c[2]) if j & 1 else (c[1] << 32 | c[0])
            r = (x * total) >> 64
            acc, n = 0, 0
            while True:
                acc += p[n]
                if acc > r:
                    break
                n += 1
            out[k, n] += 1
    return out
