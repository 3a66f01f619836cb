// map_summary.hip — the device half of fmt_map_summarize (include/fmt_map_summary.h): every
// document's sparse entries (birth order, map_sparse.hip / map_sparse_large.hip) put into JS object
// order and split into summary blobs (map.ts:176-246). The host half, and the plain C++ both kernels
// are compared against, is map_sum_plan.h.
//
// Ordering: an entry's sort key is (keyRank[key] << 32) | ordinal. keyRank is the key's array-index
// value, or 0xFFFFFFFF for any other key, so index keys come first by value and the rest keep their
// birth order; ordinals make the keys distinct.
//   mapSummarySmallKernel  one wave per document of at most 64 live entries, one entry per lane: a
//                          lane's position is the number of smaller keys (a readlane loop over the
//                          live lanes), the entries move there by ds_permute. Longer documents are
//                          listed for
//   mapSummaryLargeKernel  one workgroup per listed document of at most kMsMax entries: a bitonic
//                          sort of the 64-bit keys in LDS, then wave 0 runs the scan tile by tile.
//                          A document beyond kMsMax is copied as it is (the host orders it).
// Blob assignment (msScanTile): 64 ordered entries per step. An entry whose defined value has >= 8192
// units is its own blob; the others add 26 + units to a running size, and when that exceeds 16384 the
// members before the entry are flushed as a blob and the size restarts at 0. Across a wave this is a
// prefix sum with a moving base: each round finds the first lane past base + 16384 by ballot and moves
// the base to that lane's inclusive sum (a round closes at least two entries: a contribution is at
// most 8217). Blob indices count separate and flushed blobs in order of occurrence, a flush at lane f
// before entry f.
// The results go to a second entry buffer and a tag buffer with the replay's per-document layout
// (the replay's own entries are only read); mapSummaryPackKernel packs them for one copy to the host.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "kernels.h"

namespace fmt_kernels {

constexpr int kMsWaves = 4;
constexpr uint32_t kMsMax = 2048;  // map_sum_plan.h kMapSumDeviceMax
constexpr uint32_t kMsContent = 0xFFFFFFFFu, kMsNotIndex = 0xFFFFFFFFu;
constexpr uint32_t kMsSeparate = 8192, kMsMaxBlob = 16384, kMsMember = 26;

__device__ __forceinline__ uint32_t msLane(uint32_t v, int k) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), k));
}
__device__ __forceinline__ uint64_t msBelow(int lane) { return (1ull << lane) - 1; }  // lanes < lane (lane <= 63)

__device__ __forceinline__ int msCtz(uint64_t m) { return __builtin_ctzll(m); }
__device__ __forceinline__ uint32_t msUni(uint32_t x) {
  return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)));
}
// LDS this wave's other lanes wrote, before it is read
__device__ __forceinline__ void msWaveSync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// Inclusive wave64 prefix sum, all lanes active: Kogge-Stone inside 16-lane rows (row_shr), then row
// broadcasts (row_bcast:15 to rows 1 and 3, row_bcast:31 to rows 2 and 3), as wave.h waveInclusiveSum.
template <int Ctrl, int RowMask = 0xF>
__device__ __forceinline__ uint32_t msDpp(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), Ctrl, RowMask, 0xF, false));
}
__device__ __forceinline__ uint32_t msInclusiveSum(uint32_t v) {
  v += msDpp<0x111>(v);
  v += msDpp<0x112>(v);
  v += msDpp<0x114>(v);
  v += msDpp<0x118>(v);
  v += msDpp<0x142, 0xA>(v);
  v += msDpp<0x143, 0xC>(v);
  return v;
}

struct MsScan {  // wave-uniform, carried from tile to tile
  uint32_t running, blobs;
};

// Whether the entry is a blob of its own, and what it adds to the running size otherwise.
__device__ __forceinline__ bool msSeparate(uint32_t value, const uint32_t* __restrict__ valUnits, uint32_t nValues,
                                           uint32_t* contrib) {
  const bool undef = value == FMT_MAP_VALUE_UNDEFINED;
  const uint32_t units = undef || value >= nValues ? 0u : valUnits[value];
  *contrib = kMsMember + units;
  return !undef && units >= kMsSeparate;
}

// One tile of 64 entries in summary order, called by all 64 lanes. Returns the lane's tag; a member
// after the tile's last flush gets kMsContent (a later tile's first flush may still claim it).
// *flushOut: the lanes a flush happens before; *firstBlob: the index of the tile's first flushed blob.
__device__ __forceinline__ uint32_t msScanTile(bool valid, bool sep, uint32_t contrib, MsScan& st, uint64_t* flushOut,
                                               uint32_t* firstBlob) {
  const int lane = static_cast<int>(__lane_id());
  const bool member = valid && !sep;
  const uint32_t S = msInclusiveSum(member ? contrib : 0u);
  uint32_t base = 0u - st.running;  // running size after lane l: S_l - base (mod 2^32)
  uint64_t live = ~0ull, flush = 0;
  for (;;) {
    const uint64_t over = __ballot(member && S - base > kMsMaxBlob) & live;
    if (over == 0) break;
    const int f = msCtz(over);
    flush |= 1ull << f;
    base = msLane(S, f);  // the size restarts at 0 after entry f
    live = f == 63 ? 0ull : ~0ull << (f + 1);
  }
  st.running = msLane(S, 63) - base;
  const uint64_t ev = __ballot(sep && valid) | flush;  // blobs in order of occurrence
  uint32_t tag = kMsContent;
  if (valid && sep) {
    tag = st.blobs + static_cast<uint32_t>(__popcll(ev & msBelow(lane)));
  } else if (valid) {
    const uint64_t later = flush & ~msBelow(lane) & ~(1ull << lane);  // a flush at this lane closes the entries before it
    if (later != 0) tag = st.blobs + static_cast<uint32_t>(__popcll(ev & msBelow(msCtz(later))));
  }
  *flushOut = flush;
  *firstBlob = flush != 0 ? st.blobs + static_cast<uint32_t>(__popcll(ev & msBelow(msCtz(flush)))) : 0u;
  st.blobs += static_cast<uint32_t>(__popcll(ev));
  return tag;
}

__global__ __launch_bounds__(64 * kMsWaves) void mapSummarySmallKernel(
    const fmt_map_entry* __restrict__ in, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
    uint32_t nDocs, const uint32_t* __restrict__ keyRank, uint32_t nKeys, const uint32_t* __restrict__ valUnits,
    uint32_t nValues, fmt_map_entry* __restrict__ out, uint32_t* __restrict__ tags, uint32_t* __restrict__ nBlobs,
    uint32_t* __restrict__ list) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (uint32_t d = blockIdx.x * kMsWaves + wave; d < nDocs; d += gridDim.x * kMsWaves) {
    const uint32_t n = msUni(counts[d]);
    if (n > 64) {
      if (lane == 0) list[1 + atomicAdd(&list[0], 1u)] = d;
      continue;
    }
    if (n == 0) {
      if (lane == 0) nBlobs[d] = 0;
      continue;
    }
    const uint64_t at = offsets[d];
    const bool live = static_cast<uint32_t>(lane) < n;
    fmt_map_entry e{0, 0, 0};
    if (live) e = in[at + lane];
    const uint32_t rank = live && e.key < nKeys ? keyRank[e.key] : kMsNotIndex;
    // position: the keys (rank, lane) below this lane's; idle lanes keep their own lane
    uint32_t pos = 0;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t rj = msLane(rank, static_cast<int>(j));
      pos += (rj < rank || (rj == rank && j < static_cast<uint32_t>(lane))) ? 1u : 0u;
    }
    if (!live) pos = static_cast<uint32_t>(lane);
    const int to = static_cast<int>(pos << 2);
    const uint32_t key = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(to, static_cast<int>(e.key)));
    const uint32_t value = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(to, static_cast<int>(e.value)));
    const uint32_t birth = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(to, static_cast<int>(e.birth_seq)));
    uint32_t contrib = 0;
    const bool sep = live && msSeparate(value, valUnits, nValues, &contrib);
    MsScan st{0, 0};
    uint64_t flush;
    uint32_t firstBlob;
    const uint32_t tag = msScanTile(live, sep, contrib, st, &flush, &firstBlob);
    if (live) {
      out[at + lane] = fmt_map_entry{key, value, birth};
      tags[at + lane] = tag;
    }
    if (lane == 0) nBlobs[d] = st.blobs;
  }
}

__global__ __launch_bounds__(256) void mapSummaryLargeKernel(
    const fmt_map_entry* __restrict__ in, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ keyRank, uint32_t nKeys,
    const uint32_t* __restrict__ valUnits, uint32_t nValues, fmt_map_entry* __restrict__ out, uint32_t* __restrict__ tags,
    uint32_t* __restrict__ nBlobs) {
  __shared__ uint64_t keys[kMsMax];
  __shared__ uint32_t tg[kMsMax];
  const uint32_t tid = threadIdx.x;
  const uint32_t nList = list[0];
  for (uint32_t i = blockIdx.x; i < nList; i += gridDim.x) {
    const uint32_t d = list[1 + i];
    const uint32_t n = counts[d];
    const uint64_t at = offsets[d];
    if (n > kMsMax) {  // the host orders it: its entries as they are
      for (uint32_t p = tid; p < n; p += 256) {
        out[at + p] = in[at + p];
        tags[at + p] = kMsContent;
      }
      if (tid == 0) nBlobs[d] = 0;
      continue;
    }
    uint32_t m = 128;
    while (m < n) m <<= 1;
    for (uint32_t p = tid; p < m; p += 256) {
      uint64_t k = ~0ull;
      if (p < n) {
        const uint32_t key = in[at + p].key;
        k = (static_cast<uint64_t>(key < nKeys ? keyRank[key] : kMsNotIndex) << 32) | p;
      }
      keys[p] = k;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t p = tid; p < m; p += 256) {
          const uint32_t q = p ^ j;
          if (q > p) {
            const uint64_t a = keys[p], b = keys[q];
            if ((a > b) == ((p & k) == 0)) {
              keys[p] = b;
              keys[q] = a;
            }
          }
        }
        __syncthreads();
      }
    if (tid < 64) {  // the scan: wave 0, tile by tile
      const int lane = static_cast<int>(tid);
      MsScan st{0, 0};
      uint32_t pending = 0;  // first entry of the open member list
      for (uint32_t t0 = 0; t0 < n; t0 += 64) {
        const uint32_t p = t0 + tid;
        const bool valid = p < n;
        uint32_t contrib = 0;
        bool sep = false;
        if (valid) sep = msSeparate(in[at + static_cast<uint32_t>(keys[p])].value, valUnits, nValues, &contrib);
        uint64_t flush;
        uint32_t firstBlob;
        const uint32_t tag = msScanTile(valid, sep, contrib, st, &flush, &firstBlob);
        if (valid) tg[p] = tag;
        if (flush != 0) {  // the members left open by the tiles before
          for (uint32_t q = pending + tid; q < t0; q += 64)
            if (tg[q] == kMsContent) tg[q] = firstBlob;
          pending = t0 + 63u - static_cast<uint32_t>(__builtin_clzll(flush));
        }
        msWaveSync();
      }
      if (lane == 0) nBlobs[d] = st.blobs;
    }
    __syncthreads();
    for (uint32_t p = tid; p < n; p += 256) {
      out[at + p] = in[at + static_cast<uint32_t>(keys[p])];
      tags[at + p] = tg[p];
    }
    __syncthreads();
  }
}

// Ordered entries, tags and blob counts into one buffer of 32-bit words: [0, 3N) the entries of all
// documents back to back (document d's from packedOff[d]), [3N, 4N) their tags, [4N, 4N + nDocs) the
// blob counts.
__global__ void mapSummaryPackKernel(const fmt_map_entry* __restrict__ ordered, const uint32_t* __restrict__ tags,
                                     const uint32_t* __restrict__ nBlobs, const uint64_t* __restrict__ offsets,
                                     const uint32_t* __restrict__ counts, const uint64_t* __restrict__ packedOff,
                                     uint32_t nDocs, uint32_t* __restrict__ packed) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t total = packedOff[nDocs];
  fmt_map_entry* pe = reinterpret_cast<fmt_map_entry*>(packed);
  for (uint32_t d = blockIdx.x * 4 + wave; d < nDocs; d += gridDim.x * 4) {
    const uint64_t src = offsets[d], dst = packedOff[d];
    const uint32_t n = counts[d];
    for (uint32_t i = lane; i < n; i += 64) {
      pe[dst + i] = ordered[src + i];
      packed[3 * total + dst + i] = tags[src + i];
    }
    if (lane == 0) packed[4 * total + d] = nBlobs[d];
  }
}

hipError_t launchMapSummary(const MapSummaryArgs& a, int numCUs, hipStream_t stream) {
  const uint32_t wanted = (a.nDocs + kMsWaves - 1) / kMsWaves;
  const uint32_t cap = static_cast<uint32_t>(numCUs) * 8u;
  const uint32_t grid = wanted < cap ? (wanted > 0 ? wanted : 1) : cap;
  hipLaunchKernelGGL(mapSummarySmallKernel, dim3(grid), dim3(64 * kMsWaves), 0, stream, a.entries, a.offsets, a.counts,
                     a.nDocs, a.keyRank, a.nKeys, a.valUnits, a.nValues, a.ordered, a.tags, a.nBlobs, a.list);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // (its grid strides over the list the first kernel wrote: a batch without such documents costs an empty launch)
  hipLaunchKernelGGL(mapSummaryLargeKernel, dim3(static_cast<uint32_t>(numCUs) * 2u), dim3(256), 0, stream, a.entries,
                     a.offsets, a.counts, a.list, a.keyRank, a.nKeys, a.valUnits, a.nValues, a.ordered, a.tags, a.nBlobs);
  return hipGetLastError();
}

hipError_t launchMapSummaryPack(const fmt_map_entry* ordered, const uint32_t* tags, const uint32_t* nBlobs,
                                const uint64_t* offsets, const uint32_t* counts, const uint64_t* packedOff, uint32_t nDocs,
                                uint32_t* packed, hipStream_t stream) {
  const uint32_t blocks = nDocs / 4 + 1;
  hipLaunchKernelGGL(mapSummaryPackKernel, dim3(blocks < 65536 ? blocks : 65536), dim3(256), 0, stream, ordered, tags,
                     nBlobs, offsets, counts, packedOff, nDocs, packed);
  return hipGetLastError();
}

}  // namespace fmt_kernels
