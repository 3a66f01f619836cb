// scour_counts.cpp — the counter behind mt_engine.h's FMT_SCOUR_NOTE in a -DFMT_SCOUR_COUNT build of the host
// emulation (tools/scour_counts.py). One call per leaf-block scour that reached the serial pass; the
// emulation runs documents one after another on the calling thread, so plain counters do.
#include <stdint.h>
#include <string.h>

namespace {
// [sibling][what]: calls, no change, no change and predicted (no E neighbours, no drops), drops only,
// drops only and predicted (no E neighbours), merges (with or without drops), wrongly predicted
uint64_t g[2][7];
// per packParent (fmtPackNote): packParents, children, children with leaves, leaves in the span, children that
// only drop, children that merge, packParents in which no child changes, ... in which exactly one does, text
// units moved by the siblings' separate moves, text units one move from the first dropped offset would take,
// sibling moves, packParents with a move, leaves left
uint64_t pk[13];
bool inPack;
int chg, firstC0;
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
  if (sibling && inPack) {
    pk[2]++;
    if ((mergeMask | dropMask) != 0) {
      chg++;
      pk[mergeMask == 0 ? 4 : 5]++;
    }
  }
}

void fmtPackNote(int what, int a, int b) {
  if (what == 0) {  // start: a children holding b leaves
    inPack = true;
    chg = 0;
    firstC0 = -1;
    pk[0]++;
    pk[1] += static_cast<uint64_t>(a);
    pk[3] += static_cast<uint64_t>(b);
  } else if (what == 1) {  // a sibling's text move: units [a, b) are rewritten
    pk[8] += static_cast<uint64_t>(b - a);
    pk[10]++;
    if (firstC0 < 0) firstC0 = a;
  } else {  // end: a text units and b leaves are left
    if (chg == 0) pk[6]++;
    if (chg == 1) pk[7]++;
    if (firstC0 >= 0) {
      pk[9] += static_cast<uint64_t>(a - firstC0);
      pk[11]++;
    }
    pk[12] += static_cast<uint64_t>(b);
    inPack = false;
  }
}

void pack_counts_read(uint64_t* out) { memcpy(out, pk, sizeof pk); }

void scour_counts_read(uint64_t* out) { memcpy(out, g, sizeof g); }
void scour_counts_reset() {
  memset(g, 0, sizeof g);
  memset(pk, 0, sizeof pk);
  inPack = false;
}

}  // extern "C"
