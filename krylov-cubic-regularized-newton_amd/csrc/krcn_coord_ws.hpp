// krcn_coord_ws.hpp — the workspace of the coordinate calls (krcn_coord.hip),
// shared with the one-call SSCN step (krcn_sscn.hip), which runs the same
// kernels over the same buffers and stages its selection through the same ring.
//
// The workspace serves selections of up to cap columns (cap = k rounded up to
// a multiple of 64; grown when k grows).
//   device  delta (cap doubles) | cols (cap int32) | result (cap x cap doubles)
//           = cap (12 + 8 cap) bytes, one block of the handle's owner table
//   pinned  the result's host mirror | kCoordSlots staging slots (delta | cols)
// Staging: a call copies cols_host / delta_host into the next slot of the ring
// (a host memcpy, so the caller may overwrite its arrays once the call
// returns), enqueues one H2D copy from that slot and records the slot's event
// behind it; a slot is refilled only after its event has completed, so a copy
// still in flight never reads a slot the next call is writing.  The device
// side needs no ring: copies and kernels of one handle share one stream.
#pragma once
#include "krcn_internal.hpp"

constexpr int kCoordSlots = 4;
struct CoordWs {
  int cap = 0;
  char* dev = nullptr;
  double* delta = nullptr;
  int* cols = nullptr;
  double* res = nullptr;
  char* pin = nullptr;
  double* res_host = nullptr;
  char* slot[kCoordSlots] = {};
  hipEvent_t ev[kCoordSlots] = {};
  bool busy[kCoordSlots] = {};
  int next = 0;
};

constexpr size_t kCoordSlotPerCol = 12;   // bytes of a staging slot per column: a double and an int32
inline size_t coord_slot_bytes(int cap) { return size_t(cap) * kCoordSlotPerCol; }
inline bool coord_empty(const krcn_csr* h) { return h->n == 0 || h->nnz == 0; }

// The workspace for selections of k columns (krcn_coord.hip).
krcn_status coord_reserve(krcn_csr* h, int k, hipStream_t s);
// `bytes` from the host to `dst` on the device through the next ring slot;
// more than coord_slot_bytes(cap) is refused (KRCN_ERR_INVALID) before any copy.
krcn_status coord_stage_bytes(krcn_csr* h, const void* src, size_t bytes, void* dst, hipStream_t s);
