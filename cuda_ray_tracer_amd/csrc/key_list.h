// A lane's sorted list of its CAP smallest 64-bit keys, in registers (multihit.hip, closest_multi.hip, overlap.hip; DESIGN.md sections 6p, 6s, 6w).
// A key holds a non-negative float's bits in its high word, so that one unsigned compare is the whole order.  Every index is a
// compile-time constant once the loops are unrolled: a runtime index would move the list to scratch.
#ifndef MIRT_KEY_LIST_H
#define MIRT_KEY_LIST_H

namespace mirt {

constexpr unsigned long long KEY_NONE = ~0ull;      // above every key: a distance's bits stay below +inf's

// The contact key (closest_multi.hip, overlap.hip): a non-negative distance's bits high, kind << 30 | id low, so that one unsigned
// compare is the (dist, kind, id) order of mirt_contacts.h.  The low word's id part -- at closest_multi.hip's capacity 1 a sphere's
// unit -- stays below 2^28 (REF_OFFMASK).
constexpr unsigned KEY_ID = 0x3fffffffu;
__device__ __forceinline__ unsigned long long contact_key(float dist, unsigned kind, unsigned id)
{
  return ((unsigned long long)__float_as_uint(dist) << 32) | (kind << 30) | id;
}

template <int CAP>
struct KeyList {
  unsigned long long key[CAP > 0 ? CAP : 1];
  __device__ __forceinline__ void clear()
  {
#pragma unroll
    for (int j = 0; j < CAP; ++j) key[j] = KEY_NONE;
  }
  __device__ __forceinline__ void insert(unsigned long long x)
  {
    if (CAP == 0 || !(x < key[CAP > 0 ? CAP - 1 : 0])) return;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      const bool below = x < key[j];
      const unsigned long long lo = below ? x : key[j];
      x = below ? key[j] : x;
      key[j] = lo;
    }
  }
  // ... with the caller's order: less(a, b) must be a strict total order on the keys that agrees with < wherever it does not look
  // beyond the keys themselves (KEY_NONE above everything)
  template <class Less>
  __device__ __forceinline__ void insert(unsigned long long x, Less less)
  {
    if (CAP == 0 || !less(x, key[CAP > 0 ? CAP - 1 : 0])) return;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      const bool below = less(x, key[j]);
      const unsigned long long lo = below ? x : key[j];
      x = below ? key[j] : x;
      key[j] = lo;
    }
  }
  // the smallest key; the others move up by one
  __device__ __forceinline__ unsigned long long pop_front()
  {
    const unsigned long long first = key[0];
#pragma unroll
    for (int j = 0; j + 1 < CAP; ++j) key[j] = key[j + 1];
    key[CAP > 0 ? CAP - 1 : 0] = KEY_NONE;
    return first;
  }
};

} // namespace mirt

#endif
