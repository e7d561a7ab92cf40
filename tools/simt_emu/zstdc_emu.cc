// Driver of the emulated Zstd compressor kernel (tools/simt_emu/emu_build.sh).
//   zstdc_emu IN.bin LENS.u32 LEVEL MAX_LEN OUT.bin OUTLENS.u32
// Compresses the blocks (lengths in LENS, packed in IN) one emulated
// workgroup at a time; writes the frames packed, their lengths and statuses.
// MAX_LEN past 20480 drives the call for blocks up to 128 KiB (the second
// kernel, its scratch a malloc of exactly the size the C-ABI asks for). The
// blocks are packed with nothing between them and the last one ends the
// input allocation, so AddressSanitizer sees any read past a block's dword.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lvkv_launch.h"

static std::vector<uint8_t> slurp(const char* p) {
  FILE* f = fopen(p, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  std::vector<uint8_t> v(ftell(f));
  fseek(f, 0, SEEK_SET);
  if (fread(v.data(), 1, v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  std::vector<uint8_t> in = slurp(argv[1]), lb = slurp(argv[2]);
  const uint32_t n = lb.size() / 4;
  const int level = atoi(argv[3]);
  const uint32_t max_len = strtoul(argv[4], 0, 10);
  std::vector<uint32_t> len(n);
  memcpy(len.data(), lb.data(), 4 * n);
  std::vector<uint64_t> off(n), doff(n);
  uint64_t p = 0, q = 0;
  for (uint32_t i = 0; i < n; ++i) {
    off[i] = p;
    doff[i] = q;
    p += len[i];
    q += lvkv::zstd_bound(len[i]) + 16;
  }
  in.resize(p + 64);
  std::vector<uint8_t> dst(q + 64), st(n);
  std::vector<uint32_t> dl(n);
  if (max_len <= 20480) {
    lvkv::launch_zstd_compress(in.data(), off.data(), len.data(), dst.data(), doff.data(),
                               dl.data(), st.data(), n, max_len, level, 0, nullptr);
  } else {
    std::vector<uint8_t> scratch(lvkv::zstd_compress_big_scratch(max_len));
    const size_t exact = (p + 3) & ~uint64_t{3};  // the kernels read whole aligned dwords
    uint8_t* src = static_cast<uint8_t*>(malloc(exact ? exact : 4));
    memcpy(src, in.data(), exact);
    lvkv::launch_zstd_compress_big(src, off.data(), len.data(), dst.data(), doff.data(), dl.data(),
                                   st.data(), n, max_len, level, 0, scratch.data(), nullptr);
    free(src);
  }
  FILE* fo = fopen(argv[5], "wb");
  FILE* fl = fopen(argv[6], "wb");
  for (uint32_t i = 0; i < n; ++i) {
    fwrite(dst.data() + doff[i], 1, dl[i], fo);
    const uint32_t rec[2] = {dl[i], st[i]};
    fwrite(rec, 4, 2, fl);
  }
  fclose(fo);
  fclose(fl);
  return 0;
}
