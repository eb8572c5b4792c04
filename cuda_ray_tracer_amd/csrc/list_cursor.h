// The bounded write rule of the list fills (overlap_list.hip, query_lists.hip; DESIGN.md sections 6x, 6z): the part of a row's
// segment of the caller's offsets that a fill may write.  One copy, inlined into its callers.
#ifndef MIRT_LIST_CURSOR_H
#define MIRT_LIST_CURSOR_H

#include "device_common.h"

namespace mirt {

// Row i's segment is [offsets[i], min(offsets[i + 1], capacity)): `room` entries from index `beg` on -- none if the segment begins
// below 0, at or beyond the capacity or after its own end, and beg is then 0.  (A row admits fewer than 2^32 candidates, so a
// longer segment's room may stop there.)  Read once per row; a fill stores only while there is room, so offsets from other counts
// truncate a row and never move a store outside [0, capacity).
struct ListRoom { long long beg; uint32_t room; };
MIRT_DEV ListRoom list_room(const long long* offsets, long long capacity, long long i)
{
  const long long beg = offsets[i], lim = offsets[i + 1];
  const long long end = lim < capacity ? lim : capacity;
  ListRoom r;
  r.room = (beg >= 0 && beg < end) ? (uint32_t)(end - beg > 0xffffffffll ? 0xffffffffll : end - beg) : 0u;
  r.beg = r.room ? beg : 0;
  return r;
}

} // namespace mirt

#endif
