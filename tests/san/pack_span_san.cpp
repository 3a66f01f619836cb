// pack_span_san.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone program (g++ -fsanitize=address,undefined
// -fno-sanitize-recover) that replays the directed plain documents of tests/pack_span_docs.py through the
// emulated engine (tests/emu/mt_emu_tiers.cpp), one launch per tier, every slab a heap allocation of the
// size the runtime gives it. What it is there for: the 64-bit mask shifts (spanBits, the serial pass's and
// the text move's masks) and the two-row source indices (nthSetBit, deleteSpanLeaves) of scourSpan.
//
//   pack_span_san <dump> : the file tests/test_pack_parent_span_san.py writes:
//     u64 header[8] = { bytes of ops, doc offsets (n_docs + 1), text units, doc_init words, props_off entries,
//                       props_kv entries, marker_id_key, first tier },
//     then ops, doc_op_offsets (u64), text (u16), doc_init (u32), props_off (u32), props_kv (u32) and the
//     expected final leaf count of every document (u32), each padded to 8 bytes.
// Exit status 0: every document replayed with status 0 and the expected leaf count in every tier from the
// first one up to the large tier.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../emu/mt_emu_tiers.cpp"

namespace {

std::vector<uint8_t> readFile(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize(static_cast<size_t>(n));
  if (n > 0 && fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
  fclose(f);
  return v;
}

// One section of `n` elements copied out of the dump into storage of its own (so that a read past its end
// is a heap overflow the sanitizer sees), the cursor moved on past the padding.
template <class T>
std::vector<T> take(const std::vector<uint8_t>& buf, size_t* at, size_t n) {
  std::vector<T> v(n);
  const size_t bytes = n * sizeof(T);
  if (*at + bytes > buf.size()) {
    fprintf(stderr, "dump too short\n");
    exit(2);
  }
  if (bytes) memcpy(v.data(), buf.data() + *at, bytes);
  *at += (bytes + 7) & ~static_cast<size_t>(7);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: pack_span_san <dump>\n");
    return 2;
  }
  const std::vector<uint8_t> buf = readFile(argv[1]);
  size_t at = 0;
  const std::vector<uint64_t> h = take<uint64_t>(buf, &at, 8);
  if (h[0] % sizeof(fmt_mt_op) != 0 || h[1] < 2) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  const std::vector<fmt_mt_op> ops = take<fmt_mt_op>(buf, &at, h[0] / sizeof(fmt_mt_op));
  const std::vector<uint64_t> offs = take<uint64_t>(buf, &at, h[1]);
  const std::vector<uint16_t> text = take<uint16_t>(buf, &at, h[2]);
  const std::vector<uint32_t> init = take<uint32_t>(buf, &at, h[3]);
  const std::vector<uint32_t> propsOff = take<uint32_t>(buf, &at, h[4]);
  const std::vector<uint32_t> propsKv = take<uint32_t>(buf, &at, h[5]);
  const uint32_t nDocs = static_cast<uint32_t>(h[1] - 1);
  const std::vector<uint32_t> expect = take<uint32_t>(buf, &at, nDocs);

  fmt_mt_batch b{};
  b.ops = ops.data();
  b.n_ops = ops.size();
  b.doc_op_offsets = offs.data();
  b.n_docs = nDocs;
  b.text = text.data();
  b.text_len = text.size();
  b.doc_init = init.empty() ? nullptr : init.data();
  b.props_off = propsOff.data();
  b.n_props_ops = static_cast<uint32_t>(propsOff.size() - 1);
  b.props_kv = propsKv.data();
  b.marker_id_key = static_cast<uint32_t>(h[6]);

  uint32_t cl = 0, cc = 0, bl = 0, bc = 0;
  emu_micro_caps(2, &cl, &cc);
  emu_micro_caps(3, &bl, &bc);
  constexpr uint32_t kSmallProps = 32, kLargeProps = 1024;
  int bad = 0;
  for (int tier = static_cast<int>(h[7]); tier <= 3; tier++) {
    const bool large = tier == 3;
    std::vector<fmt_mt_doc_result> hdr(nDocs);
    std::vector<fmt_mt_leaf> smallLeaves(static_cast<size_t>(nDocs) * cl), bigLeaves(large ? static_cast<size_t>(nDocs) * bl : 0);
    std::vector<uint16_t> smallChars(static_cast<size_t>(nDocs) * cc), bigChars(large ? static_cast<size_t>(nDocs) * bc : 0);
    std::vector<fmt_mt_propset> props(static_cast<size_t>(nDocs) * (large ? kLargeProps : kSmallProps));
    std::vector<uint32_t> ckpt(static_cast<size_t>(nDocs) * emu_micro_ckpt_words());
    std::vector<uint32_t> up(nDocs + 1), down(nDocs + 1);
    const int rc = emu_tier_launch(&b, tier, hdr.data(), large ? bigLeaves.data() : smallLeaves.data(),
                                   large ? bigChars.data() : smallChars.data(), props.data(), nullptr, 0, ckpt.data(), nullptr, 0,
                                   up.data(), down.data(), large ? smallLeaves.data() : nullptr, large ? smallChars.data() : nullptr);
    if (rc != static_cast<int>(nDocs)) {
      fprintf(stderr, "tier %d: %d documents replayed of %u\n", tier, rc, nDocs);
      return 1;
    }
    for (uint32_t d = 0; d < nDocs; d++) {
      if (hdr[d].status != 0 || hdr[d].n_leaves != expect[d]) {
        fprintf(stderr, "tier %d document %u: status %d, %u leaves, expected %u\n", tier, d, static_cast<int>(hdr[d].status),
                static_cast<unsigned>(hdr[d].n_leaves), expect[d]);
        bad++;
      }
    }
  }
  printf("%u documents, tiers %d..3: %s\n", nDocs, static_cast<int>(h[7]), bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
