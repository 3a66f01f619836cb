// map_sum_plan.h — the host-only half of fmt_map_summarize (include/fmt_map_summary.h): everything the
// bulk SharedMap summaries do without a device. SharedMap.summarizeCore (map.ts:176-246) over one
// document's sequenced entries in birth order (fmt_map_entry, the sparse path's output):
//
//   tables    keyRank[k]: the array-index value of JSON-quoted key k, or kMapSumNotIndex; valUnits[v]:
//             the UTF-16 length of value text v (what `value.length` of the serialized value is)
//   order     the JS object order of the entries (mapKernel.ts:545-551): index keys ascending by
//             value, then the rest in birth order; sort key (keyRank << 32) | ordinal
//   scan      the blob split (map.ts:190-240), one tag per ordered entry: the blob it lands in, or
//             kMapSumContent for the header's "content"
//   format    the header and the blobs of every document, string concatenation only
//
// map_summary.hip restates order and scan for documents of at most kMapSumDeviceMax live entries; the
// functions here are what its arrays are compared against (fmt_internal_map_summary_format) and what
// orders the documents beyond that limit. No HIP include, no fmt_ctx.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fmt.h"

namespace fmt_plan {

constexpr uint32_t kMapSumNotIndex = 0xFFFFFFFFu;  // keyRank of a key that is not an array index
constexpr uint32_t kMapSumContent = 0xFFFFFFFFu;   // tag of an entry that stays in the header
constexpr uint32_t kMapSumSeparate = 8 * 1024;     // MinValueSizeSeparateSnapshotBlob (map.ts:190)
constexpr uint32_t kMapSumMaxBlob = 16 * 1024;     // MaxSnapshotBlobSize (map.ts:194)
constexpr uint32_t kMapSumMember = 26;             // "Plain".length + 21 (map.ts:222)
constexpr uint32_t kMapSumDeviceMax = 2048;        // live entries per document the device tier orders

// The array-index value of a JSON-quoted key ('"' + 1..10 digits + '"', no leading zero unless "0",
// value <= 2^32 - 2; such a key holds no escapes), or kMapSumNotIndex.
inline uint32_t mapKeyRank(const char* q, size_t len) {
  if (len < 3 || len > 12 || q[0] != '"' || q[len - 1] != '"') return kMapSumNotIndex;
  if (len > 3 && q[1] == '0') return kMapSumNotIndex;
  uint64_t v = 0;
  for (size_t i = 1; i + 1 < len; i++) {
    if (q[i] < '0' || q[i] > '9') return kMapSumNotIndex;
    v = v * 10 + static_cast<uint64_t>(q[i] - '0');
  }
  return v <= 4294967294ull ? static_cast<uint32_t>(v) : kMapSumNotIndex;
}

// String.prototype.length of a UTF-8 text: one unit per lead byte, two for a 4-byte sequence.
inline uint32_t mapValueUnits(const char* s, size_t len) {
  uint64_t n = 0;
  for (size_t i = 0; i < len; i++) {
    const unsigned char c = static_cast<unsigned char>(s[i]);
    if ((c & 0xC0) == 0x80) continue;
    n += c >= 0xF0 ? 2 : 1;
  }
  return n < 0xFFFFFFFFull ? static_cast<uint32_t>(n) : 0xFFFFFFFFu;
}

// f(t) on nt host threads (the calling thread runs t = 0).
template <class F>
inline void mapSumThreads(uint32_t nt, F f) {
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < nt; t++) pool.emplace_back([&f, t] { f(t); });
  f(0u);
  for (auto& th : pool) th.join();
}

struct MapSumTables {
  std::vector<uint32_t> keyRank, valUnits;  // what the device reads
  std::vector<uint32_t> keyLen, valLen;     // bytes, for the formatter
};

inline void mapSumBuildTables(const char* const* keys, uint32_t nKeys, const char* const* values, uint32_t nValues,
                              uint32_t nt, MapSumTables& T) {
  T.keyRank.resize(nKeys);
  T.keyLen.resize(nKeys);
  T.valUnits.resize(nValues);
  T.valLen.resize(nValues);
  mapSumThreads(nt, [&](uint32_t t) {
    for (uint32_t k = t; k < nKeys; k += nt) {
      const size_t len = std::strlen(keys[k]);
      T.keyLen[k] = static_cast<uint32_t>(len);
      T.keyRank[k] = mapKeyRank(keys[k], len);
    }
    for (uint32_t v = t; v < nValues; v += nt) {
      const size_t len = std::strlen(values[v]);
      T.valLen[v] = static_cast<uint32_t>(len);
      T.valUnits[v] = mapValueUnits(values[v], len);
    }
  });
}

// Every live entry names a key and a value of the tables (FMT_E_USAGE for the document otherwise).
inline bool mapSumInTables(const fmt_map_entry* e, uint32_t n, uint32_t nKeys, uint32_t nValues) {
  for (uint32_t i = 0; i < n; i++)
    if (e[i].key >= nKeys || (e[i].value != FMT_MAP_VALUE_UNDEFINED && e[i].value >= nValues)) return false;
  return true;
}

// One document's entries, birth order -> summary order (in != out). A key id outside the table sorts
// as a plain key, as on the device; the document is refused by mapSumInTables anyway.
inline void mapSumOrder(const fmt_map_entry* in, uint32_t n, const uint32_t* keyRank, uint32_t nKeys, fmt_map_entry* out,
                        std::vector<uint64_t>& scratch) {
  scratch.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t r = in[i].key < nKeys ? keyRank[in[i].key] : kMapSumNotIndex;
    scratch[i] = (static_cast<uint64_t>(r) << 32) | i;
  }
  std::sort(scratch.begin(), scratch.end());
  for (uint32_t i = 0; i < n; i++) out[i] = in[scratch[i] & 0xFFFFFFFFull];
}

// The blob split over one document's entries in summary order: tags[i] and the number of blobs.
// A defined value of >= kMapSumSeparate units is its own blob at once. Any other entry adds
// kMapSumMember + its units to the running size; when that exceeds kMapSumMaxBlob the members
// collected before this entry become the next blob, the size restarts at 0 (the overflowing entry's
// own contribution is not carried over, map.ts:226-232) and the entry opens the new member list.
inline uint32_t mapSumScan(const fmt_map_entry* e, uint32_t n, const uint32_t* valUnits, uint32_t nValues, uint32_t* tags) {
  uint32_t blobs = 0, running = 0, pending = 0;  // pending: first entry of the open member list
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t v = e[i].value;
    const bool undef = v == FMT_MAP_VALUE_UNDEFINED;
    const uint32_t units = undef || v >= nValues ? 0u : valUnits[v];
    if (!undef && units >= kMapSumSeparate) {
      tags[i] = blobs++;
      continue;
    }
    running += kMapSumMember + units;
    if (running > kMapSumMaxBlob) {
      for (uint32_t j = pending; j < i; j++)
        if (tags[j] == kMapSumContent) tags[j] = blobs;
      blobs++;
      running = 0;
      pending = i;
    }
    tags[i] = kMapSumContent;
  }
  return blobs;
}

// ------------------------------------------------------------------------------------ formatter
// Every document's header and blobs. Thread t formats a contiguous range of documents into buf[t],
// sized beforehand from the key and value byte lengths; document d's pieces (header, blob0, ...) lie
// back to back from docAt[d] in buf[docThread[d]], piece k ending at ends[pieceAt[d] + k] (relative to
// docAt[d]); pieceAt[d + 1] - pieceAt[d] - 1 blobs.
struct MapSumBlobs {
  std::vector<std::string> buf;
  std::vector<uint32_t> docThread;
  std::vector<uint64_t> docAt, pieceAt, ends;
  uint64_t bytes = 0;
};

namespace mapsum_detail {

constexpr char kMemberHead[] = ":{\"type\":\"Plain\"";  // after the quoted key
constexpr char kMemberValue[] = ",\"value\":";
constexpr size_t kMemberHeadLen = sizeof kMemberHead - 1, kMemberValueLen = sizeof kMemberValue - 1;

inline uint32_t decimalDigits(uint32_t x) {
  uint32_t n = 1;
  while (x >= 10) {
    x /= 10;
    n++;
  }
  return n;
}

inline char* put(char* p, const char* s, size_t n) {
  std::memcpy(p, s, n);
  return p + n;
}

// Bytes of one member without its separating comma: "key":{"type":"Plain","value":V}
inline uint64_t memberBytes(const fmt_map_entry& e, const MapSumTables& T) {
  return T.keyLen[e.key] + kMemberHeadLen + (e.value == FMT_MAP_VALUE_UNDEFINED ? 0 : kMemberValueLen + T.valLen[e.value]) + 1;
}

// Piece sizes of one document: size[0] the header, size[1 + k] blob k.
inline void pieceBytes(const fmt_map_entry* e, const uint32_t* tags, uint32_t n, uint32_t nBlobs, const MapSumTables& T,
                       std::vector<uint64_t>& size, std::vector<uint32_t>& members) {
  size.assign(1ull + nBlobs, 0);
  members.assign(1ull + nBlobs, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t p = tags[i] == kMapSumContent ? 0u : 1u + tags[i];
    size[p] += memberBytes(e[i], T) + (members[p]++ ? 1 : 0);
  }
  // {"blobs":["blob0",...],"content":{...}}
  uint64_t names = 0;
  for (uint32_t b = 0; b < nBlobs; b++) names += 6 + decimalDigits(b) + (b ? 1 : 0);
  size[0] += 10 + names + 13 + 2;
  for (uint32_t b = 0; b < nBlobs; b++) size[1 + b] += 2;
}

}  // namespace mapsum_detail

// entries / tags: every document's ordered entries and tags, document d's at at[d] .. at[d] + counts[d].
// status[d] != FMT_OK: the document gets no pieces (pieceAt[d + 1] == pieceAt[d]).
inline void mapSumFormat(const fmt_map_entry* entries, const uint32_t* tags, const uint32_t* nBlobs, const uint32_t* counts,
                         const uint64_t* at, const int32_t* status, uint32_t nDocs, const char* const* keys,
                         const char* const* values, const MapSumTables& T, uint32_t nt, MapSumBlobs& B) {
  using namespace mapsum_detail;
  B.buf.assign(nt, std::string());
  B.docThread.assign(nDocs, 0);
  B.docAt.assign(nDocs, 0);
  B.pieceAt.assign(nDocs + 1ull, 0);
  for (uint32_t d = 0; d < nDocs; d++) B.pieceAt[d + 1] = B.pieceAt[d] + (status[d] == FMT_OK ? 1ull + nBlobs[d] : 0ull);
  B.ends.assign(B.pieceAt[nDocs], 0);
  // contiguous document ranges of about equal entries + documents
  std::vector<uint32_t> first(nt + 1ull, nDocs);
  {
    const uint64_t total = at[nDocs] + nDocs;
    uint32_t d = 0;
    for (uint32_t t = 0; t < nt; t++) {
      first[t] = d;
      const uint64_t goal = total / nt * (t + 1ull);
      while (d < nDocs && at[d] + d < goal) d++;
    }
  }
  std::vector<uint64_t> bytes(nt, 0);
  mapSumThreads(nt, [&](uint32_t t) {
    std::vector<uint64_t> size, cursor;
    std::vector<uint32_t> members;
    uint64_t need = 0;
    for (uint32_t d = first[t]; d < first[t + 1]; d++) {
      if (status[d] != FMT_OK) continue;
      pieceBytes(entries + at[d], tags + at[d], counts[d], nBlobs[d], T, size, members);
      B.docThread[d] = t;
      B.docAt[d] = need;
      uint64_t end = 0;
      for (size_t p = 0; p < size.size(); p++) B.ends[B.pieceAt[d] + p] = end += size[p];
      need += end;
    }
    std::string& out = B.buf[t];
    out.resize(need);
    bytes[t] = need;
    for (uint32_t d = first[t]; d < first[t + 1]; d++) {
      if (status[d] != FMT_OK) continue;
      const uint32_t nb = nBlobs[d];
      char* const base = &out[0] + B.docAt[d];
      const uint64_t* ends = &B.ends[B.pieceAt[d]];
      // piece openings; cursor[p]: where piece p's next member goes
      cursor.assign(1ull + nb, 0);
      members.assign(1ull + nb, 0);
      char* p = put(base, "{\"blobs\":[", 10);
      for (uint32_t b = 0; b < nb; b++) {
        if (b) *p++ = ',';
        p = put(p, "\"blob", 5);
        char digits[10];
        uint32_t nd = 0;
        for (uint32_t x = b; nd == 0 || x; x /= 10) digits[nd++] = static_cast<char>('0' + x % 10);
        while (nd) *p++ = digits[--nd];
        *p++ = '"';
      }
      p = put(p, "],\"content\":{", 13);
      cursor[0] = static_cast<uint64_t>(p - base);
      for (uint32_t b = 0; b < nb; b++) {
        base[ends[b]] = '{';
        cursor[1 + b] = ends[b] + 1;
      }
      const fmt_map_entry* e = entries + at[d];
      const uint32_t* tg = tags + at[d];
      for (uint32_t i = 0; i < counts[d]; i++) {
        const uint32_t piece = tg[i] == kMapSumContent ? 0u : 1u + tg[i];
        char* q = base + cursor[piece];
        if (members[piece]++) *q++ = ',';
        q = put(q, keys[e[i].key], T.keyLen[e[i].key]);
        q = put(q, kMemberHead, kMemberHeadLen);
        if (e[i].value != FMT_MAP_VALUE_UNDEFINED) {
          q = put(q, kMemberValue, kMemberValueLen);
          q = put(q, values[e[i].value], T.valLen[e[i].value]);
        }
        *q++ = '}';
        cursor[piece] = static_cast<uint64_t>(q - base);
      }
      base[cursor[0]] = '}';
      base[cursor[0] + 1] = '}';
      for (uint32_t b = 0; b < nb; b++) base[cursor[1 + b]] = '}';
    }
  });
  B.bytes = 0;
  for (uint64_t x : bytes) B.bytes += x;
}

// Host ordering and scan of the documents `pick` selects (d -> bool), on nt threads: birth[birthAt[d] ..]
// -> ordered[at[d] ..], tags, nBlobs[d]. Returns how many documents it ordered.
template <class Pick>
inline uint32_t mapSumOrderDocs(const fmt_map_entry* birth, const uint64_t* birthAt, fmt_map_entry* ordered, uint32_t* tags, uint32_t* nBlobs,
                                const uint32_t* counts, const uint64_t* at, uint32_t nDocs, const MapSumTables& T, uint32_t nt,
                                Pick pick) {
  std::vector<uint32_t> docs;
  for (uint32_t d = 0; d < nDocs; d++)
    if (pick(d)) docs.push_back(d);
  const uint32_t nKeys = static_cast<uint32_t>(T.keyRank.size()), nValues = static_cast<uint32_t>(T.valUnits.size());
  mapSumThreads(nt, [&](uint32_t t) {
    std::vector<uint64_t> scratch;
    // (blocks of documents per thread: neighbours share cache lines of nBlobs)
    const size_t per = (docs.size() + nt - 1) / nt, lo = std::min(docs.size(), per * t), hi = std::min(docs.size(), lo + per);
    for (size_t i = lo; i < hi; i++) {
      const uint32_t d = docs[i];
      mapSumOrder(birth + birthAt[d], counts[d], T.keyRank.data(), nKeys, ordered + at[d], scratch);
      nBlobs[d] = mapSumScan(ordered + at[d], counts[d], T.valUnits.data(), nValues, tags + at[d]);
    }
  });
  return static_cast<uint32_t>(docs.size());
}

}  // namespace fmt_plan
