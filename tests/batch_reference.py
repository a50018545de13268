"""The batch statistics restated in numpy (include/neutral_hip.h: neutral_hip_batch_fold,
neutral_hip_batch_statistics): one numpy operation per step of the header's definition, so that the
GPU's results can be held to it bit for bit.  numpy rounds every elementwise f64 operation once and
never contracts a product with a sum.

The two sums of the statistics and the fold's sum are sums of many doubles, whose bits depend on the
order.  The library's order is fixed (neutral_comb.hip: comb_reduce_tiles_kernel, level upon level),
and tile_sum() restates it: eight consecutive entries per lane, the 64 lanes of a wave by an
inclusive shuffle scan, the four waves one after the other, the tiles' sums the same way one level
up.
"""
from collections import namedtuple

import numpy as np

MAX_LEN = 2 ** 30
BLOCK, ITEMS, WAVE = 256, 8, 64  # neutral_kernels.h: kCombBlock, kCombItems; a wave of gfx950
TILE = BLOCK * ITEMS

Statistics = namedtuple("Statistics", "estimate relerr stats")


def _tile_sums(v):
    """one level: the sum of every tile of TILE entries, in the kernel's order"""
    tiles = -(-len(v) // TILE)
    a = np.zeros(tiles * TILE, dtype=np.float64)
    a[:len(v)] = v  # (beyond the end: the identity, 0.0)
    a = a.reshape(tiles, BLOCK, ITEMS)
    lane = np.zeros((tiles, BLOCK), dtype=np.float64)
    for i in range(ITEMS):
        lane = lane + a[:, :, i]
    w = lane.reshape(tiles, BLOCK // WAVE, WAVE)
    d = 1
    while d < WAVE:  # wave_inclusive: lane i takes lane i - d
        nxt = w.copy()
        nxt[:, :, d:] = w[:, :, :-d] + w[:, :, d:]
        w = nxt
        d *= 2
    total = np.zeros(tiles, dtype=np.float64)
    for wave in range(BLOCK // WAVE):
        total = total + w[:, wave, WAVE - 1]
    return total


def tile_sum(values) -> float:
    """the sum of `values` in the order of the library's reduce<SumF64>"""
    v = _tile_sums(np.ascontiguousarray(values, dtype=np.float64).ravel())
    while len(v) > 1:
        v = _tile_sums(v)
    return float(v[0])


def fold(x, k, moments):
    """-> (moments after batch k, stats), or None where the library refuses.  moments: 2 * len values,
    means then M2; ignored (may be None) for k == 1.  The input is not written to."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    n = len(x)
    if n < 1 or n > MAX_LEN or k < 1 or not np.all(np.isfinite(x)):
        return None
    if k == 1:
        mean, m2 = x.copy(), np.zeros(n, dtype=np.float64)
    else:
        old = np.asarray(moments, dtype=np.float64)
        assert old.shape == (2 * n,)
        mean0, m20 = old[:n], old[n:]
        d = x - mean0
        step = d / np.float64(k)
        mean = mean0 + step
        d2 = x - mean
        product = d * d2
        m2 = m20 + product
    return np.concatenate([mean, m2]), dict(sum=tile_sum(x), nonzero=int(np.count_nonzero(x)))


def statistics(moments, nbatches, scale):
    """-> Statistics(estimate, relerr, stats), or None where the library refuses"""
    m = np.ascontiguousarray(moments, dtype=np.float64).ravel()
    n = len(m) // 2
    if n < 1 or n > MAX_LEN or len(m) != 2 * n or nbatches < 2 or not (np.isfinite(scale) and scale > 0.0):
        return None
    mean, m2 = m[:n], m[n:]
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(m2)) and np.all(m2 >= 0.0)):
        return None
    b = np.float64(nbatches)
    estimate = np.float64(scale) * mean
    var = m2 / (b - np.float64(1.0))
    se = np.sqrt(var / b)
    scored = mean != 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        relerr = np.where(scored, se / np.abs(mean), 0.0)
    count = int(scored.sum())
    relerr_sum = tile_sum(relerr)  # (an entry that is not scored adds 0.0)
    stats = dict(scored=count,
                 within_10pc=int((scored & (relerr <= 0.1)).sum()),
                 within_5pc=int((scored & (relerr <= 0.05)).sum()),
                 max_relerr=float(relerr.max()),
                 mean_relerr=float(np.float64(relerr_sum) / np.float64(count)) if count else 0.0,
                 estimate_sum=tile_sum(estimate))
    return Statistics(estimate, relerr, stats)


def run(batches, scale=None):
    """fold after fold over a list of arrays, then the statistics: -> (moments, fold stats, Statistics)"""
    moments, folds = None, []
    for k, x in enumerate(batches, 1):
        moments, s = fold(x, k, moments)
        folds.append(s)
    return moments, folds, statistics(moments, len(batches), float(len(batches)) if scale is None else scale)


def total_of(sums):
    """(mean, standard error) of a few host numbers: neutral_amd.interface.welford_total's formulas"""
    mean = m2 = 0.0
    for k, v in enumerate(sums, 1):
        d = v - mean
        mean = mean + d / k
        m2 = m2 + d * (v - mean)
    n = len(sums)
    return mean, float(np.sqrt(m2 / (n - 1) / n))
