// range_plan_san.cpp — a stand-alone program over fluidframework_amd/csrc/range_plan.h, meant to be built
// with -fsanitize=address,undefined (tests/test_range_host.py does). It runs the three host steps of the
// bulk range read (views, the cut into items, the offsets) around a plain restatement of the device passes,
// over randomised documents (hidden leaves, Markers, removers, failed and empty documents), ranges that
// overlap, repeat, descend, end on tile bases and run past the end, every refusal and malformed offsets, at
// tile sizes around the chunk of 64 leaves, and compares hits and text with a straight restatement of
// fmt_range.h over the whole document.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../fluidframework_amd/csrc/range_plan.h"

namespace {

struct Doc {
  fmt_mt_doc_result h{};
  std::vector<fmt_mt_leaf> leaves;
  std::vector<uint16_t> chars;
};

uint32_t unitsOf(const fmt_mt_leaf& L) { return (L.pad & FMT_MT_LEAF_MARKER) != 0 ? 1u : L.len; }

bool visible(const fmt_mt_leaf& L, int32_t refSeq, int32_t client) {
  if (refSeq == FMT_MT_VIEW_LOCAL) return L.rm_seq == FMT_NOT_REMOVED;
  const bool inserted = L.ins_seq <= refSeq || L.ins_client == client;
  const bool removed = L.rm_seq <= refSeq || ((L.rm_clients >> (static_cast<uint32_t>(client) & 63u)) & 1ull) != 0;
  return inserted && !removed;
}

// The units of positions [lo, hi) of leaves [first, first + n) in the view, appended to out; returns the
// positions the leaves hold.
uint64_t walk(const Doc& D, uint32_t first, uint32_t n, int32_t refSeq, int32_t client, uint64_t lo, uint64_t hi,
              uint16_t placeholder, std::vector<uint16_t>* out) {
  uint64_t at = 0;
  for (uint32_t i = first; i < first + n; i++) {
    const fmt_mt_leaf& L = D.leaves[i];
    if (!visible(L, refSeq, client)) continue;
    const uint32_t u = unitsOf(L);
    for (uint32_t k = 0; k < u; k++, at++) {
      if (at < lo || at >= hi || out == nullptr) continue;
      if ((L.pad & FMT_MT_LEAF_MARKER) != 0) {
        if (placeholder != 0) out->push_back(placeholder);
      } else {
        out->push_back(D.chars[L.char_off + k]);
      }
    }
  }
  return at;
}

int fail(const char* what, unsigned tile, unsigned round) {
  std::printf("FAILED: %s (tile %u, round %u)\n", what, tile, round);
  return 1;
}

Doc makeDoc(std::mt19937& rng, uint32_t nLeaves, bool failed) {
  Doc D;
  for (uint32_t i = 0; i < nLeaves; i++) {
    fmt_mt_leaf L{};
    const unsigned kind = rng() % 10;
    L.ins_seq = 1 + static_cast<int32_t>(rng() % 80);
    L.ins_client = static_cast<int16_t>(rng() % 6);
    L.rm_seq = FMT_NOT_REMOVED;
    L.props = 0xFFFF;
    L.len = kind == 9 ? 70 + rng() % 200 : 1 + rng() % 4;
    if (kind < 3) {
      L.rm_seq = 20 + static_cast<int32_t>(rng() % 70);
      L.rm_clients = 1ull << (rng() % 6);
    }
    if (kind == 3) {
      L.pad = FMT_MT_LEAF_MARKER;
      L.len = 1;
    }
    L.char_off = static_cast<uint32_t>(D.chars.size());
    for (uint32_t k = 0; k < L.len; k++) D.chars.push_back(static_cast<uint16_t>(0x100 * (i % 200) + k));
    D.leaves.push_back(L);
  }
  D.h.status = failed ? FMT_E_DATA : FMT_OK;
  D.h.n_leaves = nLeaves;
  D.h.n_chars = static_cast<uint32_t>(D.chars.size());
  D.h.min_seq = 10;
  D.h.cur_seq = 100;
  return D;
}

int round(unsigned tile, unsigned r, uint16_t placeholder) {
  std::mt19937 rng(tile * 7919u + r * 31u + placeholder);
  const uint32_t sizes[] = {0, 1, 2, 7, 63, 64, 65, 130, 200};
  std::vector<Doc> docs;
  const uint32_t nDocs = 1 + rng() % 6;
  for (uint32_t d = 0; d < nDocs; d++) docs.push_back(makeDoc(rng, sizes[rng() % 9], rng() % 10 == 0));
  const bool obliterates = rng() % 8 == 0;
  std::vector<fmt_mt_doc_result> hdrs;
  for (const Doc& D : docs) hdrs.push_back(D.h);
  const int32_t refs[] = {FMT_MT_VIEW_LOCAL, 100, 65, 30, 10, 9, 101};
  const int32_t clients[] = {0, 1, 5, 40, 63, 64, -1};
  std::vector<uint64_t> offs(1, 0);
  std::vector<fmt_mt_range_query> q;
  for (const Doc& D : docs) {
    const uint32_t nq = rng() % 24;
    for (uint32_t i = 0; i < nq; i++) {
      fmt_mt_range_query x{};
      x.ref_seq = refs[rng() % 7];
      x.client = clients[rng() % 7];
      const uint64_t len = D.h.status == FMT_OK && x.client >= 0 && x.client < 64
                               ? walk(D, 0, D.h.n_leaves, x.ref_seq, x.client, 0, 0, 0, nullptr) : 5;
      x.start = static_cast<uint32_t>(rng() % (len + 2));
      x.end = static_cast<uint32_t>(rng() % (len + 2));
      if (rng() % 3 != 0 && x.start > x.end) std::swap(x.start, x.end);
      if (rng() % 5 == 0) x.end = FMT_MT_RANGE_TO_END;
      if (rng() % 7 == 0) x.start = 0;
      q.push_back(x);
      if (rng() % 6 == 0) q.push_back(x);  // (a repeated range)
    }
    offs.push_back(q.size());
  }
  const uint64_t nq = q.size();

  // the definition over whole documents
  std::vector<fmt_mt_range_hit> want(nq);
  std::vector<uint16_t> wantText;
  for (uint32_t d = 0; d < nDocs; d++) {
    for (uint64_t i = offs[d]; i < offs[d + 1]; i++) {
      fmt_mt_range_hit& w = want[i];
      w = fmt_mt_range_hit{};
      fmt_mt_pos_query pq{0u, q[i].ref_seq, q[i].client, 0u};
      w.status = fmt_plan::posQueryStatus(hdrs[d], obliterates, pq);
      if (w.status != FMT_OK) continue;
      const uint64_t len = walk(docs[d], 0, hdrs[d].n_leaves, q[i].ref_seq, q[i].client, 0, 0, 0, nullptr);
      const uint64_t start = q[i].start, end = q[i].end == FMT_MT_RANGE_TO_END ? len : q[i].end;
      if (start > end || end > len) {
        w.status = FMT_E_DATA;
        continue;
      }
      w.text_off = wantText.size();
      walk(docs[d], 0, hdrs[d].n_leaves, q[i].ref_seq, q[i].client, start, end, placeholder, &wantText);
      w.units = static_cast<uint32_t>(wantText.size() - w.text_off);
      w.span = static_cast<uint32_t>(end - start);
    }
  }

  // the plan around the restated passes
  fmt_plan::TextPlan T;
  fmt_plan::planTextTiles(hdrs.data(), nDocs, tile, T);
  fmt_plan::RangePlan P;
  std::vector<fmt_mt_range_hit> hits(nq + 1);
  if (fmt_plan::planRangeViews(hdrs.data(), nDocs, obliterates, T, offs.data(), q.data(), nq, hits.data(), P) != FMT_OK)
    return fail("planRangeViews refused well-formed offsets", tile, r);
  std::vector<fmt_plan::PosTileUnits> tu(P.views.items.size() + 1);
  for (size_t k = 0; k < P.views.items.size(); k++) {
    const fmt_plan::PosItem& it = P.views.items[k];
    tu[k].view = walk(docs[it.doc], it.firstLeaf, it.nLeaves, it.refSeq, it.client, 0, 0, 0, nullptr);
    tu[k].local = walk(docs[it.doc], it.firstLeaf, it.nLeaves, FMT_MT_VIEW_LOCAL, 0, 0, 0, 0, nullptr);
  }
  if (fmt_plan::cutRanges(P, T, tu.data(), q.data(), nq, hits.data()) != FMT_OK) return fail("cutRanges", tile, r);
  std::vector<uint64_t> iu(P.items.size() + 1);
  std::vector<std::vector<uint16_t>> itemText(P.items.size());
  for (size_t k = 0; k < P.items.size(); k++) {
    const fmt_plan::RangeItem& it = P.items[k];
    if (it.lo >= it.hi) return fail("an empty item", tile, r);
    walk(docs[it.doc], it.firstLeaf, it.nLeaves, it.refSeq, it.client, it.lo, it.hi, placeholder, &itemText[k]);
    iu[k] = itemText[k].size();
  }
  const uint64_t total = fmt_plan::rangeOffsets(P, placeholder == 0 ? iu.data() : nullptr, nq, hits.data());
  if (total != wantText.size()) return fail("total", tile, r);
  std::vector<uint16_t> text(total, 0xDEAD);
  std::vector<uint8_t> wrote(total, 0);
  for (size_t k = 0; k < P.items.size(); k++)
    for (size_t j = 0; j < itemText[k].size(); j++) {
      const uint64_t at = P.itemBase[k] + j;
      if (at >= total || wrote[at]) return fail("a unit outside the text or written twice", tile, r);
      text[at] = itemText[k][j];
      wrote[at] = 1;
    }
  if (text != wantText) return fail("text", tile, r);
  if (nq && std::memcmp(hits.data(), want.data(), nq * sizeof(fmt_mt_range_hit)) != 0) return fail("hits", tile, r);

  // malformed offsets: refused, nothing written
  if (nDocs >= 1 && nq >= 1) {
    std::vector<fmt_mt_range_hit> guard(nq, fmt_mt_range_hit{7, 7, 7, 7, 7}), before = guard;
    std::vector<uint64_t> bad = offs;
    bad[nDocs] += 1;
    if (fmt_plan::planRangeViews(hdrs.data(), nDocs, obliterates, T, bad.data(), q.data(), nq, guard.data(), P) != FMT_E_USAGE)
      return fail("offsets past n_queries accepted", tile, r);
    bad = offs;
    bad[0] = 1;
    if (fmt_plan::planRangeViews(hdrs.data(), nDocs, obliterates, T, bad.data(), q.data(), nq, guard.data(), P) != FMT_E_USAGE)
      return fail("offsets not from 0 accepted", tile, r);
    if (nDocs >= 2) {
      bad = offs;
      bad[1] = nq + 1;
      if (fmt_plan::planRangeViews(hdrs.data(), nDocs, obliterates, T, bad.data(), q.data(), nq, guard.data(), P) != FMT_E_USAGE)
        return fail("descending offsets accepted", tile, r);
    }
    if (fmt_plan::planRangeViews(hdrs.data(), nDocs, obliterates, T, nullptr, q.data(), nq, guard.data(), P) != FMT_E_USAGE)
      return fail("null offsets accepted", tile, r);
    if (std::memcmp(guard.data(), before.data(), nq * sizeof(fmt_mt_range_hit)) != 0) return fail("a refused call wrote hits", tile, r);
  }
  return 0;
}

}  // namespace

int main() {
  static_assert(sizeof(fmt_mt_range_query) == 16 && sizeof(fmt_mt_range_hit) == 24 && sizeof(fmt_plan::RangeItem) == 32, "layouts");
  const unsigned tiles[] = {1, 2, 3, 63, 64, 65, 1024};
  unsigned rounds = 0;
  for (unsigned tile : tiles)
    for (unsigned r = 0; r < 40; r++, rounds++)
      if (round(tile, r, r % 2 ? 0xFFFC : 0)) return 1;
  std::printf("ok: %u rounds\n", rounds);
  return 0;
}
