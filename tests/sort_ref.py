"""Integer references for the radix-sort kernels and for what the hand-out orders are made from (tests/test_gpu_sort.py,
tests/test_gpu_hand_out_order.py).  numpy only; everything compares exactly.

  sort_reference    mirt_probe_sort: the stable argsort of the keys (mode 0) or of their low bytes (mode 1), and the whole keys in
                    that order
  SIZES, key_sets   the sizes and key sets both modes are run on
  cost_key          shade_common.h's cost_key restated: 255 for 0 steps, else 255 - 4 e - frac, e = floor(log2 s), frac the two bits
                    below the leading one (0 for e < 2)
  class_bounds      the smallest step count of a key's class and that of the next class
  cost_bin          render.hip's cost_bin restated: 1023 - cost / 8, costs of 8192 and more in bin 0
  chunk_order_faults  what an output of order_kernel must satisfy, as a list of faults
"""
import numpy as np

TILE = 2048      # keys per workgroup of a sort pass (build_plan.h, SORT_TILE); row_scan_kernel gives each of its 256 threads ceil(tiles / 256) tiles
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097, TILE * 256, TILE * 256 + 1, TILE * 513 + 5]
MIN_KEY = 255 - 4 * 31 - 3
SORT_BINS = 1024


def sort_reference(keys, mode):
    """(keys_out, vals_out) of mirt_probe_sort."""
    assert keys.dtype == np.uint32 and mode in (0, 1)
    order = np.argsort(keys if mode == 0 else keys & np.uint32(255), kind="stable")
    return keys[order], order.astype(np.uint32)


def key_sets(n, mode, seed=950):
    """[(name, uint32 [n])]: the key sets of one size."""
    rng = np.random.default_rng([seed, n, mode])
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)      # noqa: E731
    i = np.arange(n, dtype=np.uint64)
    four = u32([0x10203040, 0x10203041, 0xF0203040, 0x1020F0C1])      # (two of them share a low byte: mode 1 must keep their frame order)
    sets = [("all 0", np.zeros(n, np.uint32)),
            ("all 0xffffffff", np.full(n, 0xFFFFFFFF, np.uint32)),      # (the value a padding lane carries)
            ("alternating", u32(np.where(i % 2 == 0, 0xA5A5A5A5, 0x5A5A5A5A))),
            ("descending", u32(n - 1 - i)),
            ("random 32 bits", u32(rng.integers(0, 1 << 32, n, dtype=np.uint64))),
            ("four values", four[rng.integers(0, 4, n)])]
    for b in range(4):
        rest = np.uint64(0x3C5A96E1 & ~(0xFF << (8 * b)))
        sets.append((f"random byte {b}", u32(rest | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * b)))))
    if mode == 1:
        classes = np.array([0, 4, 8, 9, 40, 127], np.uint64)
        sets.append(("cost classes", u32((np.uint64(255) - classes[rng.integers(0, len(classes), n)]) | (rng.integers(0, 1 << 24, n, dtype=np.uint64) << np.uint64(8)))))
    return sets


def cost_key(steps):
    s = np.asarray(steps, dtype=np.uint64)
    assert (s < (1 << 32)).all()
    e = np.frexp(s.astype(np.float64))[1].astype(np.int64) - 1      # floor(log2 s); -1 for s = 0 (exact: s < 2^53)
    shift = np.where(e >= 2, e - 2, 0).astype(np.uint64)
    frac = np.where(e >= 2, (s >> shift) & np.uint64(3), 0).astype(np.int64)
    return np.where(s == 0, 255, 255 - 4 * e - frac).astype(np.uint32)


def key_is_valid(keys):
    """A key cost_key can return: 255 (0 or 1 step), 251 (2 or 3), or 255 - 4 e - frac with 2 <= e <= 31."""
    c = 255 - np.asarray(keys, dtype=np.int64)
    return (c >= 0) & (c <= 255 - MIN_KEY) & ((c >= 8) | (c % 4 == 0))


def class_bounds(keys):
    """(lo, hi) int64: the step counts s with cost_key(s) == key are lo <= s < hi."""
    assert key_is_valid(keys).all()
    c = 255 - np.asarray(keys, dtype=np.int64)
    e, f = c // 4, c % 4
    sh = np.maximum(e - 2, 0)
    lo = np.where(e == 0, 0, np.where(e == 1, 2, (4 + f) << sh))
    hi = np.where(e == 0, 2, np.where(e == 1, 4, (5 + f) << sh))
    return lo, hi


def cost_bin(cost):
    b = np.asarray(cost, dtype=np.int64) >> 3
    return np.where(b < SORT_BINS, SORT_BINS - 1 - b, 0)


def chunk_order_faults(cost, order):
    """order_kernel over `cost`: a permutation; bins non-decreasing; every maximal run of equal bins inside one thread's slice
    [t per, min(n, (t + 1) per)), per = ceil(n / 1024), comes out as consecutive ascending indices.  The order between runs of one
    bin is the order of LDS atomics and is not looked at."""
    n = len(cost)
    order = np.asarray(order, dtype=np.int64)
    if not np.array_equal(np.sort(order), np.arange(n)):
        return ["not a permutation of 0..n-1"]
    faults = []
    bins = cost_bin(cost)
    if (np.diff(bins[order]) < 0).any():
        faults.append(f"bins decrease at output position {int(np.flatnonzero(np.diff(bins[order]) < 0)[0])}")
    per = (n + SORT_BINS - 1) // SORT_BINS
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    i = np.arange(n - 1)
    same_run = (bins[1:] == bins[:-1]) & (i // per == (i + 1) // per)
    torn = same_run & (pos[1:] != pos[:-1] + 1)
    if torn.any():
        faults.append(f"the run through chunk {int(np.flatnonzero(torn)[0])} is torn or out of order")
    return faults
