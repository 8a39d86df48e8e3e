// handoff.h -- what one launch of the multi-launch solve leaves for the next one, owned by type: a region of per-workgroup
// partial sums that remembers the grid of the launch that wrote it, and the two-slot state record.  Host-side bookkeeping
// only: a handle's launches go to one stream, so the order of these calls is the order the kernels run in (the just-in-time
// feed's early-exit launches included).  Includes nothing from HIP (tests/cxx/test_handoff.cpp builds it with the host
// compiler); host.h turns a refusal into DPGO_ERR_STATE.
#pragma once

namespace dpgo_host {

// One region of Cap per-workgroup entries.  A kernel stores one entry per workgroup; the next kernel's prologue sums
// count() of them, so the count travels with the region instead of being recomputed by every reader.
template <int Cap>
struct PartialRegion {
  double* base = nullptr;
  int written = 0;  // workgroups of the launch that last wrote the region; 0: none since the handle was created
  // for the launch that writes the region on `grid` workgroups; NULL (and nothing recorded) for a grid outside 1 .. Cap
  double* out(int grid) {
    if (grid < 1 || grid > Cap) return nullptr;
    written = grid;
    return base;
  }
  // for the launch that sums the region.  A launch that really reads it asks is_written() first; one that receives the
  // pointer without reading it (the tCG update with first = 1) does not.
  const double* in() const { return base; }
  int count() const { return written; }
  bool is_written() const { return written > 0; }
};

// The state record's two slots: a kernel reads in() and writes out(), advance() makes what it wrote the current record.
template <class State>
struct StateSlots {
  State* base = nullptr;  // two records
  int cur = 0, holds = 0;
  const State* in() const { return base + cur; }
  State* out() const { return base + (cur ^ 1); }
  State* slot(int i) const { return base + i; }
  void advance() {
    if (!holds) cur ^= 1;
  }
  // slot 0 becomes the current record; returns it (k_rtr_begin and the one-launch solve's commit kernel write it)
  State* rewind() {
    cur = 0;
    return base;
  }
  // while a Hold lives advance() does nothing: the kernel probes launch again and again from the record they pushed
  struct Hold {
    StateSlots& s;
    explicit Hold(StateSlots& slots) : s(slots) { ++s.holds; }
    ~Hold() { --s.holds; }
    Hold(const Hold&) = delete;
    Hold& operator=(const Hold&) = delete;
  };
};

}  // namespace dpgo_host
