// scour_counts.cpp — the counter behind mt_engine.h's FMT_SCOUR_NOTE in a -DFMT_SCOUR_COUNT build of the host
// emulation (tools/scour_counts.py). One call per leaf-block scour that reached the serial pass; the
// emulation runs documents one after another on the calling thread, so plain counters do.
#include <stdint.h>
#include <string.h>

namespace {
// [sibling][what]: calls, no change, no change and predicted (no E neighbours, no drops), drops only,
// drops only and predicted (no E neighbours), merges (with or without drops), wrongly predicted
uint64_t g[2][7];
}

extern "C" {

void fmtScourNote(int sibling, int pairs, int drops, uint32_t mergeMask, uint32_t dropMask) {
  uint64_t* c = g[sibling ? 1 : 0];
  c[0]++;
  if ((mergeMask | dropMask) == 0) {
    c[1]++;
    if (!pairs && !drops) c[2]++;
  } else if (mergeMask == 0) {
    c[3]++;
    if (!pairs) c[4]++;
  } else {
    c[5]++;
  }
  // what the fast paths would have got wrong (must stay 0): a merge without E neighbours, or drop
  // ballots that disagree with the serial pass
  if ((mergeMask != 0 && !pairs) || ((dropMask != 0) != (drops != 0))) c[6]++;
}

void scour_counts_read(uint64_t* out) { memcpy(out, g, sizeof g); }
void scour_counts_reset() { memset(g, 0, sizeof g); }

}  // extern "C"
