// ysb_window.h -- the rules of the per-workgroup LDS window of (campaign, bucket) counters and
// of the ring's automatic base, as pure functions.  No HIP here: the device side that applies
// them (LdsWindow, commit_ring_base) is ysb_ring_add.h's, the parked views' host model
// (ysb_parked.h) uses the ring rule, and tests/native/window_logic.cpp runs all of it on the CPU.
//
// The window: WL (a power of two) consecutive buckets per campaign, counted with LDS atomics and
// flushed to the ring when the window moves.  A view outside it is counted into the ring at
// once; one ahead of it -- or any view while there is no window yet -- also asks for a move
// (the largest such bucket of a tile wins), which the next tile carries out.  A view behind the
// window never moves it: late events must not drag it backwards.
#pragma once
#include "ysb_common.h"

namespace ysb {

// the base of the window re-centred on the requested bucket: the request sits at rel WL / 2 - 1,
// half the window lies ahead of it
YSB_HD i64 window_base_for(i64 req, u32 WL) { return req - (i64)(WL / 2) + 1; }
// the window (if there is one) holds the bucket at rel = bucket - base
YSB_HD bool window_holds(bool set, i64 rel, u32 WL) { return set && rel >= 0 && rel < (i64)WL; }
// a view at rel that the window does not hold asks for a move
YSB_HD bool window_asks_move(bool set, i64 rel, u32 WL) { return !set || rel >= (i64)WL; }

// The base of a ring of ring_w buckets fixed by the smallest bucket first seen: an eighth of the
// ring stays behind it, room for out-of-order and late events.
YSB_HD i64 ring_base_for(i64 min_bucket, u32 ring_w) { return min_bucket - (i64)(ring_w / 8); }

}  // namespace ysb
