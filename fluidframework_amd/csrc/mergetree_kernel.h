// mergetree_kernel.h — the merge-tree replay kernel template (mt_engine.h) and its launcher, shared
// by the per-tier translation units (mergetree.hip: small tier; mergetree_compact.hip: compact tier;
// mergetree_micro.hip: micro tier; mergetree_large.hip: large tier), which compile in parallel.
//
// One wavefront replays one document end to end; several documents share a workgroup, each with its
// own LDS state (fmt_mt::Scratch). Documents are independent, so the grid simply strides over them;
// there is no inter-workgroup communication. The per-document sequential dependency (every op
// depends on the state its predecessors left) is the reason this kernel is issue/latency-bound rather
// than HBM-bound: its compulsory HBM traffic is the 32-byte op record plus payload per op and the
// converged state written once per document.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"  // (mt_bind.h, and through it mt_engine.h)

namespace fmt_kernels {

// Diagnostic build only: per-phase shader-clock totals summed over all waves (mt_engine.h stamp()),
// one copy per translation unit (no relocatable device code); mergeTreeProfile sums them.
static __device__ unsigned long long g_mtProfile[fmt_mt::kPfCount];

// This translation unit's profile totals added into out[0..n) (and zeroed with reset).
static inline int addTuProfile(uint64_t* out, int n, bool reset) {
  unsigned long long h[fmt_mt::kPfCount];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_mtProfile), sizeof h) != hipSuccess) return -1;
  for (int c = 0; c < n && c < fmt_mt::kPfCount; c++) out[c] += h[c];
  if (reset) {
    unsigned long long z[fmt_mt::kPfCount] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_mtProfile), z, sizeof z) != hipSuccess) return -1;
  }
  return fmt_mt::kPfCount;
}

// LDS bytes per wave: batches without obliterates never touch the live-obliterate table at the end
// of Scratch (1.6 KiB), which is what lets the compact tier hold 4 waves per SIMD (16 × 9312 B).
template <class C, bool Ob>
constexpr size_t scratchBytes() {
  return Ob ? sizeof(fmt_mt::Scratch<C>) : (offsetof(fmt_mt::Scratch<C>, ob) + 15) & ~static_cast<size_t>(15);
}

// A tier over all documents (docList == nullptr) or a list of countDev[0] (when countDev is set:
// the overflow list a previous launch built on the device) or `count` documents. The large tier
// writes leaves/chars/props to slab i of the list (headers stay per document).
template <bool Ob, class C, bool Rm, int Waves, int WavesPerEU, bool Adj = false, bool Loc = false>
__global__ __launch_bounds__(64 * Waves, WavesPerEU) void mergeTreeKernel(MtDeviceBatch batch, MtDeviceOut out,
                                                                      const uint32_t* __restrict__ docList,
                                                                      uint32_t count, const uint32_t* countDev,
                                                                      uint32_t* next) {
  using Doc = fmt_mt::Doc<Ob, C, Rm, Adj, Loc>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));  // wave-uniform
  FMT_LDS fmt_mt::Scratch<C>* scratch = (FMT_LDS fmt_mt::Scratch<C>*)(lds + wave * scratchBytes<C, Ob>());
  if (countDev != nullptr) count = __builtin_amdgcn_readfirstlane(*countDev);
  // Documents are dealt one at a time from a device counter (next != nullptr): a wave that finishes
  // early takes the next document, so the launch ends when the work does, not when the unluckiest
  // static share of documents does. Every wave leaves once the counter passes `count`.
  for (uint32_t i = next ? 0u : blockIdx.x * Waves + wave;; i += next ? 0u : gridDim.x * Waves) {
    if (next != nullptr) {
      uint32_t v = 0;
      if ((threadIdx.x & 63) == 0) v = atomicAdd(next, 1u);
      i = __builtin_amdgcn_readfirstlane(v);
    }
    if (i >= count) break;
    const uint32_t d = docList ? docList[i] : i;
    const size_t slot = C::kHbmChars ? i : d;
    FMT_MT_BIND_DOC(Doc, batch, out, d, slot, Slab<C>::kLeaves, Slab<C>::kChars, Slab<C>::kProps, countDev != nullptr, in, o);
    Doc doc;
    doc.s = scratch;
    doc.run(in, o);
#if FMT_PROFILE && FMT_GPU
    if ((threadIdx.x & 63) == 0)
      for (int c = 0; c < fmt_mt::kPfCount; c++) atomicAdd(&g_mtProfile[c], static_cast<unsigned long long>(doc.prof[c]));
#endif
  }
}

// The documents a tier could not hold (FMT_E_CAPACITY) among docList[0..nDocs) (nDocs = countDev[0]
// when set): esc[0] = count, esc[1..] = ids. A limit the large tier shares (fmt_mt::kCapacityFinal)
// is reported as FMT_E_CAPACITY without escalation. down (or nullptr: the launch let none step down):
// the same for the documents that stopped for the tier below (fmt_mt::kCkptDescend). Both lists are
// appended to, so two launches can fill one. Defined in mergetree.hip.
__global__ __launch_bounds__(256) void collectOverflowKernel(fmt_mt_doc_result* __restrict__ headers,
                                                             const uint32_t* __restrict__ docList, uint32_t nDocs,
                                                             const uint32_t* countDev, uint32_t* esc, uint32_t* down);

#ifdef FMT_MT_COLLECT_DEFINE
__global__ __launch_bounds__(256) void collectOverflowKernel(fmt_mt_doc_result* __restrict__ headers,
                                                             const uint32_t* __restrict__ docList, uint32_t nDocs,
                                                             const uint32_t* countDev, uint32_t* esc, uint32_t* down) {
  if (countDev != nullptr) nDocs = *countDev;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nDocs; i += gridDim.x * blockDim.x) {
    const uint32_t d = docList ? docList[i] : i;
    const HandOff to = collectHeader(headers[d]);
    uint32_t* list = to == HandOff::kUp ? esc : to == HandOff::kDown ? down : nullptr;
    if (list != nullptr) list[1 + atomicAdd(list, 1u)] = d;
  }
}
#endif

// One launch of a tier. docList / count: the documents (nullptr: 0 .. count); countDev: the list length
// lives on the device (an overflow list), `count` then bounds it (grid size). esc / down: the lists
// collectOverflowKernel appends to (esc nullptr: none is collected). next: the dealing counter, or nullptr.
struct TierLaunch {
  const MtDeviceBatch& batch;
  const MtDeviceOut& out;
  const uint32_t* docList;
  uint32_t count;
  uint32_t* esc;
  int numCUs;
  hipStream_t stream;
  const uint32_t* countDev;
  uint32_t* next;
  uint32_t* down;
};

template <class C>
constexpr fmt_plan::MtTier tierOf() {
  return C::kHbmChars                            ? fmt_plan::MtTier::kLarge
         : C::kRows == fmt_mt::MicroTier::kRows   ? fmt_plan::MtTier::kMicro
         : C::kRows == fmt_mt::CompactTier::kRows ? fmt_plan::MtTier::kCompact
                                                  : fmt_plan::MtTier::kSmall;
}

template <bool Ob, class C, bool Rm, int Waves, int WavesPerEU, bool Adj = false, bool Loc = false>
static hipError_t launchTier(const TierLaunch& a) {
  static_assert(fmt_plan::hasMtKernel(tierOf<C>(), fmt_plan::MtVariant{Ob, Rm, Adj, Loc}), "not in mt_route.h kMtKernels");
  const size_t lds = scratchBytes<C, Ob>() * Waves;
  // One resident wave of workgroups: every workgroup strides over the same number of documents,
  // so none waits behind the residency limit (VGPRs cap the small tier at 2 waves/SIMD).
  int blocksPerCU = 0;
  const hipError_t e =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocksPerCU, mergeTreeKernel<Ob, C, Rm, Waves, WavesPerEU, Adj, Loc>, 64 * Waves, lds);
  if (e != hipSuccess) return e;
  const uint32_t wanted = (a.count + Waves - 1) / Waves;
  const uint32_t cap = static_cast<uint32_t>(a.numCUs * (blocksPerCU > 0 ? blocksPerCU : 1));
  const uint32_t grid = wanted < cap ? (wanted > 0 ? wanted : 1) : cap;
  hipLaunchKernelGGL((mergeTreeKernel<Ob, C, Rm, Waves, WavesPerEU, Adj, Loc>), dim3(grid), dim3(64 * Waves), lds, a.stream, a.batch,
                     a.out, a.docList, a.count, a.countDev, a.next);
  if (a.esc != nullptr) {  // over the documents this launch replayed
    const uint32_t g = (a.count + 255) / 256;
    hipLaunchKernelGGL(collectOverflowKernel, dim3(g < 1024 ? (g > 0 ? g : 1) : 1024), dim3(256), 0, a.stream, a.out.headers,
                       a.docList, a.count, a.countDev, a.esc, a.down);
  }
  return hipGetLastError();
}

}  // namespace fmt_kernels
