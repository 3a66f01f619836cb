// map_sum_plan_san.cpp — a stand-alone program over fluidframework_amd/csrc/map_sum_plan.h, meant to
// be built with -fsanitize=address,undefined (tests/test_map_summary_host.py does). It runs the tables,
// the ordering, the blob scan and the threaded formatter over directed documents (key classification,
// undefined values, the 8191 / 8192 and 16384 / 16385 edges, the dropped contribution, interleaved
// blob numbers, empty documents, ids outside the tables) and over randomised ones, and compares them
// with a straight restatement of SharedMap.summarizeCore that builds member lists and std::strings.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../fluidframework_amd/csrc/map_sum_plan.h"

namespace {

struct Doc {
  std::vector<fmt_map_entry> entries;  // birth order
};

std::string quoted(const std::string& s) { return "\"" + s + "\""; }  // (the keys here need no escapes)

bool isIndex(const std::string& k, uint64_t* v) {
  if (k.empty() || k.size() > 10 || (k.size() > 1 && k[0] == '0')) return false;
  uint64_t x = 0;
  for (char c : k) {
    if (c < '0' || c > '9') return false;
    x = x * 10 + static_cast<uint64_t>(c - '0');
  }
  *v = x;
  return x < 4294967295ull;
}

size_t units(const std::string& s) {
  size_t n = 0;
  for (unsigned char c : s)
    if ((c & 0xC0) != 0x80) n += c >= 0xF0 ? 2 : 1;
  return n;
}

// The reference's rule, restated with explicit lists (map.ts:190-240 as oracle/map.cpp reads it).
std::pair<std::string, std::vector<std::string>> reference(const Doc& doc, const std::vector<std::string>& keys,
                                                           const std::vector<std::string>& values) {
  std::vector<std::pair<uint64_t, size_t>> idx;
  std::vector<size_t> order, rest;
  for (size_t i = 0; i < doc.entries.size(); i++) {
    uint64_t v;
    if (isIndex(keys[doc.entries[i].key], &v)) idx.emplace_back(v, i);
    else rest.push_back(i);
  }
  std::sort(idx.begin(), idx.end());
  for (auto& p : idx) order.push_back(p.second);
  order.insert(order.end(), rest.begin(), rest.end());
  auto member = [&](size_t i) {
    const fmt_map_entry& e = doc.entries[i];
    std::string m = quoted(keys[e.key]) + ":{\"type\":\"Plain\"";
    if (e.value != FMT_MAP_VALUE_UNDEFINED) m += ",\"value\":" + values[e.value];
    return m + "}";
  };
  auto object = [&](const std::vector<size_t>& members) {
    std::string j = "{";
    for (size_t k = 0; k < members.size(); k++) j += (k ? "," : "") + member(members[k]);
    return j + "}";
  };
  std::vector<std::string> blobs;
  std::vector<size_t> open;
  size_t size = 0;
  for (size_t i : order) {
    const fmt_map_entry& e = doc.entries[i];
    const bool undef = e.value == FMT_MAP_VALUE_UNDEFINED;
    const size_t len = undef ? 0 : units(values[e.value]);
    if (!undef && len >= 8192) {
      blobs.push_back(object({i}));
      continue;
    }
    size += 26 + len;
    if (size > 16384) {
      blobs.push_back(object(open));
      open.clear();
      size = 0;
    }
    open.push_back(i);
  }
  std::string h = "{\"blobs\":[";
  for (size_t b = 0; b < blobs.size(); b++) h += (b ? ",\"blob" : "\"blob") + std::to_string(b) + "\"";
  return {h + "],\"content\":" + object(open) + "}", blobs};
}

int failures = 0;

void check(bool ok, const char* what, size_t doc) {
  if (ok) return;
  std::printf("FAILED: %s (document %zu)\n", what, doc);
  failures++;
}

void run(const std::vector<Doc>& docs, const std::vector<std::string>& keys, const std::vector<std::string>& values,
         uint32_t nKeysGiven, uint32_t nValuesGiven, uint32_t nt) {
  std::vector<std::string> qk;
  for (const auto& k : keys) qk.push_back(quoted(k));
  std::vector<const char*> kp, vp;
  for (uint32_t i = 0; i < nKeysGiven; i++) kp.push_back(qk[i].c_str());
  for (uint32_t i = 0; i < nValuesGiven; i++) vp.push_back(values[i].c_str());
  const uint32_t nd = static_cast<uint32_t>(docs.size());
  std::vector<uint32_t> counts(nd);
  std::vector<uint64_t> at(nd + 1, 0);
  std::vector<fmt_map_entry> birth;
  for (uint32_t d = 0; d < nd; d++) {
    counts[d] = static_cast<uint32_t>(docs[d].entries.size());
    at[d + 1] = at[d] + counts[d];
    birth.insert(birth.end(), docs[d].entries.begin(), docs[d].entries.end());
  }
  fmt_plan::MapSumTables T;
  fmt_plan::mapSumBuildTables(kp.data(), nKeysGiven, vp.data(), nValuesGiven, nt, T);
  std::vector<fmt_map_entry> ordered(birth.size());
  std::vector<uint32_t> tags(birth.size()), nBlobs(nd);
  std::vector<int32_t> status(nd, FMT_OK);
  const uint32_t done = fmt_plan::mapSumOrderDocs(birth.data(), at.data(), ordered.data(), tags.data(), nBlobs.data(),
                                                  counts.data(), at.data(), nd, T, nt, [](uint32_t) { return true; });
  check(done == nd, "every document ordered", 0);
  for (uint32_t d = 0; d < nd; d++)
    if (!fmt_plan::mapSumInTables(ordered.data() + at[d], counts[d], nKeysGiven, nValuesGiven)) status[d] = FMT_E_USAGE;
  fmt_plan::MapSumBlobs B;
  fmt_plan::mapSumFormat(ordered.data(), tags.data(), nBlobs.data(), counts.data(), at.data(), status.data(), nd, kp.data(),
                         vp.data(), T, nt, B);
  for (uint32_t d = 0; d < nd; d++) {
    bool inTables = true;
    for (const auto& e : docs[d].entries)
      inTables = inTables && e.key < nKeysGiven && (e.value == FMT_MAP_VALUE_UNDEFINED || e.value < nValuesGiven);
    check((status[d] == FMT_OK) == inTables, "status", d);
    const uint64_t pieces = B.pieceAt[d + 1] - B.pieceAt[d];
    if (!inTables) {
      check(pieces == 0, "a refused document has no pieces", d);
      continue;
    }
    const auto want = reference(docs[d], keys, values);
    check(pieces == 1 + want.second.size() && nBlobs[d] == want.second.size(), "number of blobs", d);
    if (pieces != 1 + want.second.size()) continue;
    const char* base = B.buf[B.docThread[d]].data() + B.docAt[d];
    uint64_t from = 0;
    for (uint64_t k = 0; k < pieces; k++) {
      const uint64_t to = B.ends[B.pieceAt[d] + k];
      const std::string got(base + from, to - from);
      check(got == (k ? want.second[k - 1] : want.first), k ? "blob" : "header", d);
      from = to;
    }
  }
}

}  // namespace

int main() {
  // key ranks and value units
  struct {
    const char* key;
    uint32_t rank;
  } ranks[] = {{"0", 0}, {"7", 7}, {"10", 10}, {"4294967294", 4294967294u}, {"4294967295", 0xFFFFFFFFu}, {"01", 0xFFFFFFFFu},
               {"-1", 0xFFFFFFFFu}, {"1.5", 0xFFFFFFFFu}, {"", 0xFFFFFFFFu}, {"1e3", 0xFFFFFFFFu}, {" 1", 0xFFFFFFFFu},
               {"12345678901", 0xFFFFFFFFu}, {"99999999999999999999", 0xFFFFFFFFu}};
  for (const auto& r : ranks) {
    const std::string q = quoted(r.key);
    check(fmt_plan::mapKeyRank(q.c_str(), q.size()) == r.rank, r.key, 0);
  }
  check(fmt_plan::mapKeyRank("7", 1) == fmt_plan::kMapSumNotIndex && fmt_plan::mapKeyRank("\"7", 2) == fmt_plan::kMapSumNotIndex,
        "unquoted text is no index key", 0);
  check(fmt_plan::mapValueUnits("\"\xF0\x9F\x98\x80\xC3\xA9\"", 8) == 5, "a 4-byte sequence is two units", 0);

  auto text = [](size_t n, char c) { return "\"" + std::string(n - 2, c) + "\""; };
  std::vector<std::string> keys = {"zeta", "10", "4294967295", "7", "01", "4294967294", "-1", "0", "1.5", "", "1e3", " 1",
                                   "12345678901", "e1", "e2", "e3", "e4", "e0", "4", "S1", "S2", "a", "b", "c", "d", "e", "f"};
  std::vector<std::string> values = {"1", "null", text(8191, 'x'), text(8192, 'y'), text(8166, 'a'), text(8167, 'b'),
                                     text(8000, 'c'), text(400, 'd'), text(9000, 'e')};
  std::string pairs = "\"";
  for (int i = 0; i < 4095; i++) pairs += "\xF0\x9F\x98\x80";
  values.push_back(pairs + "\"");  // 9: 8192 units, 16382 bytes
  const uint32_t U = FMT_MAP_VALUE_UNDEFINED;
  std::vector<Doc> docs;
  auto doc = [&](std::vector<std::pair<uint32_t, uint32_t>> kv) {
    Doc d;
    uint32_t seq = 1;
    for (auto& p : kv) d.entries.push_back({p.first, p.second, seq++});
    docs.push_back(d);
  };
  doc({{0, 0}, {1, 1}, {2, 0}, {3, 1}, {4, 0}, {5, 1}, {6, 0}, {7, U}, {8, 0}, {9, 1}, {10, U}, {11, 0}, {12, 1}});  // keys
  doc({{21, 2}, {22, 3}, {3, 0}});                                        // 8191 stays, 8192 is its own blob
  doc({{21, 9}, {22, 2}});                                                // non-BMP 8192 units
  doc({{21, 4}, {22, 4}});                                                // exactly 16384
  doc({{21, 4}, {22, 5}});                                                // 16385
  doc({{13, 6}, {14, 6}, {15, 6}, {16, 6}, {17, 7}, {18, 6}});            // the dropped contribution
  doc({{21, 6}, {19, 3}, {22, 6}, {23, 6}, {20, 8}, {24, 6}, {25, 6}, {26, 6}});  // interleaved blob numbers
  doc({});
  doc({{21, 6}, {22, 6}, {23, 6}, {24, 6}, {25, 6}, {26, 6}, {13, 6}, {14, 6}, {15, 6}, {16, 6}, {1, 6}, {3, 6}});  // many flushes
  const uint32_t nk = static_cast<uint32_t>(keys.size()), nv = static_cast<uint32_t>(values.size());
  for (uint32_t nt : {1u, 3u, 16u}) run(docs, keys, values, nk, nv, nt);
  // ids outside the tables: the documents that name the last key / the last value fail alone
  run(docs, keys, values, nk - 1, nv, 2);
  run(docs, keys, values, nk, nv - 1, 2);
  run(docs, keys, values, 0, 0, 2);

  // randomised: 0..80 entries, values drawn so that most documents flush
  std::mt19937 rng(7);
  std::vector<std::string> rk, rv;
  for (int i = 0; i < 200; i++) rk.push_back(i % 2 ? std::to_string(rng() % 3000) + (i % 10 == 1 ? "x" : "") : "k" + std::to_string(i));
  for (size_t n : {2, 3, 17, 40, 200, 700, 1500, 3000, 8191, 8192, 9000}) rv.push_back(text(n, 'r'));
  std::vector<Doc> rdocs;
  for (int d = 0; d < 300; d++) {
    Doc D;
    const uint32_t n = rng() % 81;
    for (uint32_t i = 0; i < n; i++)
      D.entries.push_back({static_cast<uint32_t>(rng() % rk.size()), rng() % 20 == 0 ? U : static_cast<uint32_t>(rng() % rv.size()), i + 1});
    rdocs.push_back(D);
  }
  for (uint32_t nt : {1u, 7u})
    run(rdocs, rk, rv, static_cast<uint32_t>(rk.size()), static_cast<uint32_t>(rv.size()), nt);
  if (failures) return 1;
  std::printf("ok: %zu directed and %zu randomised documents\n", docs.size(), rdocs.size());
  return 0;
}
