// bdl_claim_ring.hpp — which {claim, done} counter pair a dynamic-order launch
// gets (include/bdl_order.h).  Host only and plain C++ (no HIP): bdl_api.hip
// calls it under its lock, tests/test_claim_ring_host.py builds it into a
// stand-alone program.
//
// Why a launch may use slot s: the pair must be zero when the launch starts,
// and the last workgroup of the previous launch on s zeroes it.  Launches of
// one stream run in order, so a slot only ever used by one stream is zero
// again before that stream's next launch starts.  Hence a slot is bound to the
// first stream that takes it, for good; nothing is known about the progress of
// another stream, so a slot bound elsewhere is never taken.  A stream binds at
// most BDL_CLAIM_SLOTS_PER_STREAM slots (so that BDL_CLAIM_SLOTS /
// BDL_CLAIM_SLOTS_PER_STREAM streams get the dynamic order) and walks them as
// a ring.  No slot: the launch runs the grid-stride order.
#pragma once
#include <stdint.h>

#include "bdl_order.h"

namespace bdl {

struct ClaimRing {
  uintptr_t owner[BDL_CLAIM_SLOTS];
  bool bound[BDL_CLAIM_SLOTS];
  int cursor;
};

// The slot of the next launch on `stream`, or -1: the launch runs order 1.
// capturing: the stream is being captured (a captured launch may replay any
// number of times, in any graph); redirect: the launch rewrites a graph node.
inline int claim_ring_next(ClaimRing& ring, uintptr_t stream, bool capturing, bool redirect) {
  if (capturing || redirect) return -1;
  int owned = 0;
  for (int i = 0; i < BDL_CLAIM_SLOTS; ++i) owned += ring.bound[i] && ring.owner[i] == stream;
  for (int k = 0; k < BDL_CLAIM_SLOTS; ++k) {
    const int s = (ring.cursor + k) % BDL_CLAIM_SLOTS;
    if (ring.bound[s] ? ring.owner[s] != stream : owned >= BDL_CLAIM_SLOTS_PER_STREAM) continue;
    ring.bound[s] = true;
    ring.owner[s] = stream;
    ring.cursor = (s + 1) % BDL_CLAIM_SLOTS;
    return s;
  }
  return -1;
}

}  // namespace bdl
