"""The radix-sort kernels on keys of the test's choosing, against numpy's stable argsort (tests/sort_ref.py).  Exact.

mirt_probe_sort runs radix_pass_kernel<false>, row_scan_kernel and radix_pass_kernel<true> through the functions the product calls:
mode 0 the four passes of a build (the values are the positions 0..n-1), mode 1 the one pass over the low byte that orders a frame's
samples by cost class.  In both modes the output is the stable argsort -- of the whole key, or of its low byte -- and the whole key
travels with it.  Sizes (sort_ref.SIZES): one key, a pair, around a wave (64), a block of threads (256), the 512 keys one wave owns
and a tile (2048), a third workgroup with one key, and around 256 tiles: 256 tiles keep every thread of row_scan_kernel busy with one
tile, 257 give every other thread two and one thread a single one, 513 and a partly filled last tile give three.  Key sets
(sort_ref.key_sets): all equal (0, and 0xffffffff, which padding lanes carry too), two values alternating, descending, random over
all 32 bits (digits 64..255 in the top pass, which 30-bit Morton codes never show), random over four values (long equal runs across
every boundary: stability is the whole answer), random in one byte with the others constant, and for mode 1 cost classes under
arbitrary high bytes."""
import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import sort_ref as R

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else (int(d[0]), int(got[d[0]]), int(want[d[0]]), int(d.size))


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("mode", [0, 1])
def test_the_sort_is_the_stable_argsort(mode, n):
    for name, keys in R.key_sets(n, mode):
        before = keys.copy()
        keys_out, vals_out = api.probe_sort(mode, keys)
        want_keys, want_vals = R.sort_reference(keys, mode)
        assert np.array_equal(keys, before), name
        assert np.array_equal(vals_out, want_vals), (name, "vals_out: first difference (index, got, want, how many)", _first_difference(vals_out, want_vals))
        assert np.array_equal(keys_out, want_keys), (name, "keys_out: first difference (index, got, want, how many)", _first_difference(keys_out, want_keys))


def test_bad_arguments_are_errors():
    k = np.arange(4, dtype=np.uint32)
    a, b = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    for args in ((0, 0, 0, k.ctypes.data, a.ctypes.data, b.ctypes.data), (0, 0, -1, k.ctypes.data, a.ctypes.data, b.ctypes.data),
                 (0, 2, 4, k.ctypes.data, a.ctypes.data, b.ctypes.data), (0, -1, 4, k.ctypes.data, a.ctypes.data, b.ctypes.data),
                 (0, 0, 4, None, a.ctypes.data, b.ctypes.data), (0, 1, 4, k.ctypes.data, None, b.ctypes.data), (0, 1, 4, k.ctypes.data, a.ctypes.data, None)):
        assert m.lib().mirt_probe_sort(*args) == 3, args
        assert "mirt_probe_sort: bad argument" in m.lib().mirt_last_error().decode()
