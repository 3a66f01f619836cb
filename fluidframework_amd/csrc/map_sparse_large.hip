// map_sparse_large.hip — the HBM tier of the sparse SharedMap path (fmt_map_run_sparse_tiered): the
// documents mapSparseKernel refuses (more than 2048 distinct keys after the last clear, or more than
// 16384 ops) replayed with the hash table in HBM and 32-bit ordinals, into the same output buffers
// and layout, so fetch, pack and the pending kernel run on the result unchanged.
//
// Semantics as in map_sparse.hip, over op ordinals i (1-based), every quantity in a word of its own:
//     C = last clear,   D[k] = last delete of k after C,   a set i of k survives iff i > max(D[k], C)
//     first[k] / last[k] = min / max surviving set;   value[k] = value id of op last[k]
// One document's work never sits on one wave: the host (map_plan.h) cuts the overflowing documents'
// op ranges into tiles of 256 ops, and every pass is one kernel whose waves grid-stride over all
// tiles, one wave per tile (the launch boundary is the grid-wide barrier between passes):
//     1 init     key = first = 0xffffffff, D = last = value = 0, C = 0
//     2 clear    C = max ordinal of a clear (atomicMax per wave); a bad key id raises the data bit
//     3 claim    ops after C: a set / delete claims its key's slot (atomicCAS, linear probing; the
//                table has >= 2 slots per op, so a probe always ends), a delete maxes D[slot], a
//                set leaves its slot in its op-slot word (0xffffffff for every other op)
//     4 survive  sets with i > D[slot] (D is final): atomicMin first[slot], atomicMax last[slot]
//     5 value    op last[slot] stores its value id; ops that are first[slot] (births) are counted
//                per tile
//     6 scan     exclusive scan of each document's tile counts (one workgroup per document: 4 B per
//                256 ops); the total is counts[doc]
//     7 emit     birth i writes {key, value[slot], seq} at out[doc_op_offsets[doc] + tile base + its
//                rank among the tile's births]; the capacity bit of the error word is cleared
// No pass reads a word another op of the same pass writes: 3 reads key (CAS) and writes D / op slot,
// 4 reads D and writes first / last, 5 reads first / last and writes value, 7 reads first / value.
// Only vector global loads, stores and atomics; no LDS but the scan's carry.
// Bound: HBM latency of the random table accesses — per op 2 x 16 B of records (passes 2, 3), 3 x 4 B
// of op slots (4, 5, 7), one CAS and up to three atomics in a table of 20 B per slot.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "kernels.h"

namespace fmt_kernels {

namespace {

constexpr uint32_t kLgTile = fmt_plan::kMapLargeTile;
constexpr int kLgWaves = 4;  // tiles in flight per workgroup
constexpr uint32_t kLgNone = 0xffffffffu;
typedef unsigned int lgv4 __attribute__((ext_vector_type(4)));

struct LgTile {
  uint32_t j;       // index of the document in a.docs
  uint32_t first;   // first op of the tile, within the document
  uint32_t len;     // ops in the tile
  fmt_plan::MapLargeDoc d;
};

// fn(tile index, LgTile) for the tiles of this wave (all 64 lanes together).
template <class F>
__device__ __forceinline__ void lgTiles(const MapLargeArgs& a, F&& fn) {
  const uint32_t wave = threadIdx.x >> 6;
  for (uint32_t t = blockIdx.x * kLgWaves + wave; t < a.nTiles; t += gridDim.x * kLgWaves) {
    LgTile T;
    T.j = a.tileDoc[t];
    T.first = a.tileFirst[t];
    T.d = a.docs[T.j];
    T.len = min(kLgTile, T.d.nOps - T.first);
    fn(t, T);
  }
}

__device__ __forceinline__ uint32_t lgLanesBelow(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(ballot >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(ballot), 0u));
}

__device__ __forceinline__ uint32_t lgWaveMax(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off)));
  return v;
}

}  // namespace

// pass 1
__global__ __launch_bounds__(256) void mapLargeInitKernel(MapLargeArgs a) {
  const uint64_t ones = 2 * a.slots, tables = 5 * a.slots, n = tables + a.nDocs;
  uint32_t* clear = a.scratch + a.clearAt;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    if (i < tables) a.scratch[i] = i < ones ? kLgNone : 0u;  // key, first | D, last, value
    else clear[i - tables] = 0u;
  }
}

// pass 2
__global__ __launch_bounds__(64 * kLgWaves) void mapLargeClearKernel(MapLargeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const lgv4* recs = reinterpret_cast<const lgv4*>(a.ops);
  lgTiles(a, [&](uint32_t, const LgTile& T) {
    uint32_t c = 0;
    bool bad = false;
    for (uint32_t at = lane; at < T.len; at += 64) {
      const uint32_t i = T.first + at;
      const lgv4 v = recs[T.d.opBegin + i];
      const uint32_t k = v.w >> FMT_MAP_KIND_SHIFT;
      if (k == FMT_MAP_CLEAR) c = i + 1;
      bad |= (k == FMT_MAP_SET || k == FMT_MAP_DELETE) && v.y >= a.keyBound;  // (before the last clear too)
    }
    c = lgWaveMax(c);
    if (lane == 0 && c != 0) atomicMax(a.scratch + a.clearAt + T.j, c);
    if (__ballot(bad) != 0 && lane == 0) atomicOr(a.error, 1);
  });
}

// pass 3
__global__ __launch_bounds__(64 * kLgWaves) void mapLargeClaimKernel(MapLargeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const lgv4* recs = reinterpret_cast<const lgv4*>(a.ops);
  lgTiles(a, [&](uint32_t, const LgTile& T) {
    const uint32_t C = a.scratch[a.clearAt + T.j];
    uint32_t* key = a.scratch + T.d.tableOff;  // (the key region starts at word 0)
    uint32_t* del = a.scratch + 2 * a.slots + T.d.tableOff;
    uint32_t* opSlot = a.scratch + 5 * a.slots + T.d.opSlotOff;
    for (uint32_t at = lane; at < T.len; at += 64) {
      const uint32_t i = T.first + at;
      uint32_t mine = kLgNone;
      if (i + 1 > C) {
        const lgv4 v = recs[T.d.opBegin + i];
        const uint32_t k = v.w >> FMT_MAP_KIND_SHIFT;
        if ((k == FMT_MAP_SET || k == FMT_MAP_DELETE) && v.y < a.keyBound) {
          uint32_t s = (v.y * 0x9e3779b1u) >> T.d.shift, slot = kLgNone;
          for (uint32_t probe = 0; probe <= T.d.mask; probe++) {
            const uint32_t cur = atomicCAS(&key[s], kLgNone, v.y);
            if (cur == kLgNone || cur == v.y) {
              slot = s;
              break;
            }
            s = (s + 1) & T.d.mask;
          }
          if (slot != kLgNone) {
            if (k == FMT_MAP_DELETE) atomicMax(&del[slot], i + 1);
            else mine = slot;
          }
        }
      }
      opSlot[i] = mine;
    }
  });
}

// pass 4
__global__ __launch_bounds__(64 * kLgWaves) void mapLargeSurviveKernel(MapLargeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  lgTiles(a, [&](uint32_t, const LgTile& T) {
    const uint32_t* del = a.scratch + 2 * a.slots + T.d.tableOff;
    uint32_t* first = a.scratch + a.slots + T.d.tableOff;
    uint32_t* last = a.scratch + 3 * a.slots + T.d.tableOff;
    const uint32_t* opSlot = a.scratch + 5 * a.slots + T.d.opSlotOff;
    for (uint32_t at = lane; at < T.len; at += 64) {
      const uint32_t i = T.first + at, s = opSlot[i];
      if (s != kLgNone && i + 1 > del[s]) {
        atomicMin(&first[s], i + 1);
        atomicMax(&last[s], i + 1);
      }
    }
  });
}

// pass 5
__global__ __launch_bounds__(64 * kLgWaves) void mapLargeValueKernel(MapLargeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  lgTiles(a, [&](uint32_t t, const LgTile& T) {
    const uint32_t* first = a.scratch + a.slots + T.d.tableOff;
    const uint32_t* last = a.scratch + 3 * a.slots + T.d.tableOff;
    uint32_t* value = a.scratch + 4 * a.slots + T.d.tableOff;
    const uint32_t* opSlot = a.scratch + 5 * a.slots + T.d.opSlotOff;
    uint32_t births = 0;
    for (uint32_t c = 0; c < T.len; c += 64) {  // (every lane takes every turn: the ballot below)
      const uint32_t at = c + lane, i = T.first + at;
      bool birth = false;
      if (at < T.len) {
        const uint32_t s = opSlot[i];
        if (s != kLgNone) {
          // only a surviving set ever wrote its own ordinal into first / last
          if (last[s] == i + 1) value[s] = a.ops[T.d.opBegin + i].kind_value & FMT_MAP_VALUE_MASK;
          birth = first[s] == i + 1;
        }
      }
      births += static_cast<uint32_t>(__popcll(__ballot(birth)));
    }
    if (lane == 0) a.scratch[a.tileCountAt + t] = births;
  });
}

// pass 6: one workgroup per overflowing document
__global__ __launch_bounds__(256) void mapLargeScanKernel(MapLargeArgs a) {
  __shared__ uint32_t waveSum[4];
  __shared__ uint32_t carry;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t j = blockIdx.x; j < a.nDocs; j += gridDim.x) {
    const fmt_plan::MapLargeDoc d = a.docs[j];
    uint32_t* cnt = a.scratch + a.tileCountAt + d.firstTile;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < d.nTiles; base += 256) {
      const uint32_t t = base + threadIdx.x;
      const uint32_t v = t < d.nTiles ? cnt[t] : 0u;
      uint32_t incl = v;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), off));
        if (lane >= static_cast<uint32_t>(off)) incl += up;
      }
      if (lane == 63) waveSum[wave] = incl;
      __syncthreads();
      uint32_t before = carry;
      for (uint32_t w = 0; w < wave; w++) before += waveSum[w];
      if (t < d.nTiles) cnt[t] = before + incl - v;
      __syncthreads();
      if (threadIdx.x == 255) carry = before + incl;
      __syncthreads();
    }
    if (threadIdx.x == 0) a.counts[d.doc] = carry;
    __syncthreads();
  }
}

// pass 7
__global__ __launch_bounds__(64 * kLgWaves) void mapLargeEmitKernel(MapLargeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAnd(a.error, ~2);  // every refused document is replayed here
  lgTiles(a, [&](uint32_t t, const LgTile& T) {
    const uint32_t* first = a.scratch + a.slots + T.d.tableOff;
    const uint32_t* value = a.scratch + 4 * a.slots + T.d.tableOff;
    const uint32_t* opSlot = a.scratch + 5 * a.slots + T.d.opSlotOff;
    fmt_map_entry* o = a.out + T.d.opBegin;
    uint32_t rank = a.scratch[a.tileCountAt + t];  // births of the document's earlier tiles
    for (uint32_t c = 0; c < T.len; c += 64) {
      const uint32_t at = c + lane, i = T.first + at;
      bool birth = false;
      uint32_t s = kLgNone;
      if (at < T.len) {
        s = opSlot[i];
        birth = s != kLgNone && first[s] == i + 1;
      }
      const uint64_t bal = __ballot(birth);
      if (birth) {
        const fmt_map_op op = a.ops[T.d.opBegin + i];
        fmt_map_entry e;
        e.key = op.key;
        e.value = value[s];
        e.birth_seq = op.seq;
        o[rank + lgLanesBelow(bal)] = e;  // rank <= i: inside the document's own range
      }
      rank += static_cast<uint32_t>(__popcll(bal));
    }
  });
}

// The seven passes, in order, on `stream`. launches: how many kernels were enqueued.
hipError_t launchMapLarge(const MapLargeArgs& a, int numCUs, hipStream_t stream, uint32_t* launches) {
  *launches = 0;
  if (a.nDocs == 0 || a.nTiles == 0) return hipSuccess;
  const uint32_t cap = static_cast<uint32_t>(numCUs) * 8u;  // 8 workgroups of 4 waves per CU
  const uint32_t wanted = (a.nTiles + kLgWaves - 1) / kLgWaves;
  const dim3 grid(wanted < cap ? wanted : cap), block(64 * kLgWaves);
  const uint64_t initBlocks = (5 * a.slots + a.nDocs + 255) / 256;
  hipLaunchKernelGGL(mapLargeInitKernel, dim3(static_cast<uint32_t>(initBlocks < cap ? initBlocks : cap)), dim3(256), 0,
                     stream, a);
  hipLaunchKernelGGL(mapLargeClearKernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(mapLargeClaimKernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(mapLargeSurviveKernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(mapLargeValueKernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(mapLargeScanKernel, dim3(a.nDocs < cap ? a.nDocs : cap), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(mapLargeEmitKernel, grid, block, 0, stream, a);
  *launches = 7;
  return hipGetLastError();
}

}  // namespace fmt_kernels
