// mfm_res_entry.hpp -- the entries of the persistent sweep's item-draw lists (mfm_res.hpp, ResArgs::entries): their width and
// their packing. Plain C++ (no HIP header): the planners, the kernel and a host-only check share it.
//
// An entry is {run whose partial belongs to the item, item - first item of the slice}. A slice has at most 512 items (a thread of
// the workgroup draws an item), so the item takes 9 bits; a plan whose run indices -- the workgroups' pad runs and the zero run
// behind the last one included -- all fit 23 bits packs an entry into one 32-bit word, run << 9 | item. Every other plan, and the
// row-sharded form, keeps 8 bytes: two words {run, item}.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MFM_RES_ENTRY_FN __host__ __device__ inline
#else
#define MFM_RES_ENTRY_FN inline
#endif

namespace mfm {

constexpr int RES_ENT_ITEM_BITS = 9, RES_ENT_RUN_BITS = 32 - RES_ENT_ITEM_BITS;

// bytes of a list entry of a plan whose largest run index is max_run
MFM_RES_ENTRY_FN int res_entry_bytes(int64_t max_run, bool row_sharded) {
  return !row_sharded && max_run >= 0 && max_run < ((int64_t)1 << RES_ENT_RUN_BITS) ? 4 : 8;
}
MFM_RES_ENTRY_FN uint32_t res_entry_pack(int32_t run, int32_t item) {
  return ((uint32_t)run << RES_ENT_ITEM_BITS) | (uint32_t)item;
}
MFM_RES_ENTRY_FN int32_t res_entry_run(uint32_t w) { return (int32_t)(w >> RES_ENT_ITEM_BITS); }
MFM_RES_ENTRY_FN int32_t res_entry_item(uint32_t w) { return (int32_t)(w & ((1u << RES_ENT_ITEM_BITS) - 1u)); }

}  // namespace mfm
