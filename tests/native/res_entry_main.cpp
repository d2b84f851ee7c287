// A stand-alone check of csrc/mfm_res_entry.hpp (no HIP, no device): the width of the item draw's list entries as a function of
// the plan's largest run index, and pack / unpack at the ends of both fields. Built with -fsanitize=address,undefined by
// tests/test_resident_entry_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "mfm_res_entry.hpp"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

int main() {
  using namespace mfm;
  const int64_t top = ((int64_t)1 << 23) - 1;
  CHECK(RES_ENT_ITEM_BITS == 9 && RES_ENT_RUN_BITS == 23);
  // width: 4 bytes up to run index 2^23 - 1, 8 from 2^23 on; row-sharded plans always 8
  CHECK(res_entry_bytes(0, false) == 4);
  CHECK(res_entry_bytes(top, false) == 4);
  CHECK(res_entry_bytes(top + 1, false) == 8);
  CHECK(res_entry_bytes(((int64_t)1 << 31) - 3, false) == 8);
  CHECK(res_entry_bytes(0, true) == 8 && res_entry_bytes(top, true) == 8 && res_entry_bytes(top + 1, true) == 8);
  // config 3 (2.04 M runs + 256 pad runs + the zero run) and the 14 M-row table (about 2.9 M) take 4 bytes
  CHECK(res_entry_bytes(2040000 + 257, false) == 4 && res_entry_bytes(2900000, false) == 4);
  // pack / unpack: both ends of both fields, and every combination of them
  const int32_t runs[] = {0, 1, 511, 512, (int32_t)top - 1, (int32_t)top}, items[] = {0, 1, 255, 256, 510, 511};
  for (int32_t r : runs)
    for (int32_t i : items) {
      const uint32_t w = res_entry_pack(r, i);
      CHECK(res_entry_run(w) == r && res_entry_item(w) == i);
    }
  CHECK(res_entry_pack(0, 0) == 0u);
  CHECK(res_entry_pack((int32_t)top, 511) == 0xffffffffu);
  CHECK(res_entry_pack(1, 0) == 512u && res_entry_pack(0, 511) == 511u);
  // a run index of 2^23 does not fit: the width function must have said 8 bytes (the top bit would fall off the word)
  CHECK(res_entry_run(res_entry_pack((int32_t)(top + 1), 0)) != (int32_t)(top + 1));
  std::printf("entry: ok\n");
  return 0;
}
