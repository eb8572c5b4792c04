"""tests/sort_ref.py held to what it claims, without a GPU: the key sets reach the digits and boundaries they are there for, the
restated cost key and its class bounds agree with a brute-force count, and chunk_order_faults accepts a right order and names a
wrong one."""
import numpy as np

import sort_ref as R


def test_the_key_sets_are_what_they_claim():
    n = R.TILE * 256 + 1
    for mode in (0, 1):
        sets = dict(R.key_sets(n, mode))
        assert all(k.dtype == np.uint32 and k.shape == (n,) and k.flags["C_CONTIGUOUS"] for k in sets.values())
        assert len(sets) == 10 + mode
        assert len(np.unique(sets["random 32 bits"] >> 24)) == 256      # digits 64..255 in the top pass
        assert len(np.unique(sets["four values"])) == 4 and len(np.unique(sets["four values"] & 255)) == 3
        assert np.array_equal(sets["descending"], np.arange(n - 1, -1, -1, dtype=np.uint32))
        assert set(np.unique(sets["alternating"])) == {0xA5A5A5A5, 0x5A5A5A5A} and (sets["alternating"][1:] != sets["alternating"][:-1]).all()
        for b in range(4):
            k = sets[f"random byte {b}"]
            assert len(np.unique((k >> (8 * b)) & 255)) == 256 and len(np.unique(k & ~np.uint32(0xFF << (8 * b)))) == 1
    assert len(np.unique(sets["cost classes"] & 255)) == 6 and len(np.unique(sets["cost classes"] >> 8)) > 1000
    assert R.key_is_valid(sets["cost classes"] & 255).all()
    # row_scan_kernel's tiles per thread at the three large sizes
    assert [(-(-s // R.TILE) + 255) // 256 for s in R.SIZES[-3:]] == [1, 2, 3] and R.SIZES[-1] % R.TILE == 5


def test_the_reference_sort_is_stable_and_carries_the_whole_key():
    keys = np.array([0x0201, 0x0100, 0x0301, 0x0000, 0x0101], np.uint32)
    k0, v0 = R.sort_reference(keys, 0)
    assert v0.tolist() == [3, 1, 4, 0, 2] and k0.tolist() == [0x0000, 0x0100, 0x0101, 0x0201, 0x0301]
    k1, v1 = R.sort_reference(keys, 1)
    assert v1.tolist() == [1, 3, 0, 2, 4] and k1.tolist() == [0x0100, 0x0000, 0x0201, 0x0301, 0x0101]


def test_the_cost_key_and_its_class_bounds():
    s = np.arange(0, 1 << 16, dtype=np.uint64)
    k = R.cost_key(s)
    assert k[:9].tolist() == [255, 255, 251, 251, 247, 246, 245, 244, 243]
    assert (np.diff(k.astype(np.int64)) <= 0).all() and R.key_is_valid(k).all()
    lo, hi = R.class_bounds(k)
    assert ((lo <= s) & (s < hi)).all()
    for key in np.unique(k)[1:]:      # (the most expensive class seen is cut off by the range of s)
        members = s[k == key]
        l, h = R.class_bounds(np.array([key]))
        assert (int(members[0]), int(members[-1]) + 1) == (int(l[0]), int(h[0])), key
    assert R.cost_key([0xFFFFFFFF, 1 << 31, (1 << 31) - 1]).tolist() == [R.MIN_KEY, 255 - 124, 255 - 120 - 3] and R.MIN_KEY == 128
    assert not R.key_is_valid([254, 253, 252, 250, 249, 248, 127, 256]).any() and R.key_is_valid([255, 251, 247, 246, 128]).all()
    assert [int(x[0]) for x in R.class_bounds(np.array([R.MIN_KEY]))] == [7 << 29, 1 << 32]


def test_the_chunk_order_check_accepts_a_right_order_and_names_a_wrong_one():
    rng = np.random.default_rng(5)
    cost = rng.integers(0, 9000, 5000).astype(np.uint32)
    assert R.cost_bin([0, 7, 8, 8191, 8192, 0xFFFFFFFF]).tolist() == [1023, 1023, 1022, 0, 0, 0]
    right = np.argsort(R.cost_bin(cost), kind="stable")
    assert R.chunk_order_faults(cost, right) == []
    # the runs of one bin in another order are as good: the slices' runs of the most frequent bin, last slice first
    b = R.cost_bin(cost)
    per = -(-len(cost) // R.SORT_BINS)
    slices = [np.arange(t * per, min(len(cost), (t + 1) * per)) for t in range(R.SORT_BINS)]
    other = np.concatenate([np.concatenate([s[b[s] == v] for s in reversed(slices)]) for v in np.unique(b)])
    assert not np.array_equal(other, right) and R.chunk_order_faults(cost, other) == []
    assert R.chunk_order_faults(cost, right[::-1]) != [] and "bins decrease" in R.chunk_order_faults(cost, right[::-1])[0]
    assert R.chunk_order_faults(cost, np.zeros(5000, np.int64)) == ["not a permutation of 0..n-1"]
    flat = np.zeros(5000, np.uint32)
    swapped = np.arange(5000)
    swapped[[10, 11]] = [11, 10]      # chunks 10 and 11 lie in one slice (per = 5) and one bin
    assert R.chunk_order_faults(flat, np.arange(5000)) == [] and "torn" in R.chunk_order_faults(flat, swapped)[0]
