// The partial-sum regions and the state slots of the multi-launch solve (dpgo_amd/csrc/handoff.h), with the host compiler and
// no library: a region hands its reader the grid of the launch that last wrote it, and the slots advance, rewind and hold.
#include "handoff.h"

#include <cstdio>

using namespace dpgo_host;

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("handoff: line %d: %s\n", __LINE__, #cond);         \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

int main() {
  constexpr int kCap = 1024;
  double mem[8] = {};
  {  // a region: the recorded count comes back, a second writer replaces it, grids outside 1 .. kCap are refused
    PartialRegion<kCap> R;
    R.base = mem;
    EXPECT(!R.is_written() && R.count() == 0);  // a checked read of a never-written region is refused ...
    EXPECT(R.in() == mem);                      // ... an unchecked one gets the pointer
    EXPECT(R.out(157) == mem && R.is_written() && R.count() == 157 && R.in() == mem);
    EXPECT(R.out(3) == mem && R.count() == 3);
    EXPECT(R.out(0) == nullptr && R.count() == 3);  // (a refused writer records nothing)
    EXPECT(R.out(-1) == nullptr && R.count() == 3);
    EXPECT(R.out(kCap + 1) == nullptr && R.count() == 3);
    EXPECT(R.out(kCap) == mem && R.count() == kCap);
    EXPECT(R.out(1) == mem && R.count() == 1);
    PartialRegion<kCap> other;  // regions do not share their counts
    other.base = mem + 4;
    EXPECT(!other.is_written() && other.out(7) == mem + 4 && R.count() == 1 && other.count() == 7);
  }
  {  // the slots
    int rec[2] = {10, 11};
    StateSlots<int> S;
    S.base = rec;
    EXPECT(S.in() == rec && S.out() == rec + 1 && S.slot(0) == rec && S.slot(1) == rec + 1);
    S.advance();
    EXPECT(S.in() == rec + 1 && S.out() == rec);
    S.advance();
    EXPECT(S.in() == rec && S.out() == rec + 1);
    S.advance();
    EXPECT(S.rewind() == rec && S.in() == rec && S.out() == rec + 1);
    EXPECT(S.rewind() == rec && S.in() == rec);  // (from slot 0 too)
    S.advance();  // hold on slot 1: advance() does nothing until the last hold is released
    {
      StateSlots<int>::Hold h(S);
      S.advance();
      EXPECT(S.in() == rec + 1 && S.out() == rec);
      {
        StateSlots<int>::Hold inner(S);
        S.advance();
      }
      S.advance();
      EXPECT(S.in() == rec + 1);
    }
    EXPECT(S.in() == rec + 1);  // (the release itself moves nothing)
    S.advance();
    EXPECT(S.in() == rec && S.out() == rec + 1);
    {  // a rewind under a hold still takes effect: it names a slot, it does not flip
      S.advance();
      StateSlots<int>::Hold h(S);
      EXPECT(S.rewind() == rec && S.in() == rec);
    }
  }
  if (failures) return 1;
  std::printf("handoff: ok\n");
  return 0;
}
