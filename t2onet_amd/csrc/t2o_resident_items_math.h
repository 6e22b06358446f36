// The per-thread program of the resident-ITEM gather (t2o_resident_items.hip): the batch of t2o_resident_math.h for items of
// up to 16 pictures, plus one row of a device-resident int32 table per sample, in the same launch.
//
//   pictures  gather_thread of t2o_resident_math.h as it is: it does not depend on K, so for K <= 8 the outputs are those
//             of t2o_gather_u8_to_f32 bit for bit.  Slots may repeat, within an item and across items (a picture shared
//             by several items is stored once); -1 = absent: zeros.
//   rows      rows (N, V) int32, out_rows (B, V) int32: out_rows[b][v] = rows[index[b]][v]; an index outside [0, N) gives
//             -1 throughout -- for a table of plane numbers "no entry" (gier.MaskTable).  V = 0: there is no table.
//
// The grid is flat: B K picture_blocks workgroups serve the pictures exactly as k_gather_u8_f32's do, row_blocks more are
// appended behind them, a thread of those owning one element of out_rows.  Every output element has exactly one writer.
//
// `__host__ __device__` like t2o_resident_math.h: tests/host_emul/emul_resident_items.cpp runs items_thread with g++ for
// every thread of every workgroup of the grid (a test harness, never a fallback).
#pragma once
#include "t2o_resident_math.h"

namespace t2o {

constexpr int kItemsMaxK = 16;

struct ItemsArgs {
  GatherArgs g;                  // the pictures: store, slots (N, K), index (B), out_x, out_ys
  const int* rows;               // (N, V), or NULL when V = 0
  int* out_rows;                 // (B, V), or NULL when V = 0
  int V;
  unsigned picture_blocks;       // B K g.blocks_per_image: the workgroups in front of the row workgroups
  unsigned row_blocks;           // ceil(B V / kGatherThreads)
};

// thread t of the row workgroups: element t of out_rows
T2O_IMG_HD void rows_thread(const ItemsArgs& a, long long t) {
  if (t >= (long long)a.g.B * a.V) return;
  const long long b = t / a.V;
  const int v = (int)(t - b * a.V);
  const long long i = a.g.index[b];
  a.out_rows[t] = (i < 0 || i >= (long long)a.g.N) ? -1 : a.rows[(size_t)i * (size_t)a.V + (size_t)v];
}

// thread `thread` of workgroup `block` of the flat grid
T2O_IMG_HD void items_thread(const ItemsArgs& a, unsigned block, unsigned thread) {
  if (block >= a.picture_blocks) {
    rows_thread(a, (long long)(block - a.picture_blocks) * kGatherThreads + thread);
    return;
  }
  const unsigned image = block / a.g.blocks_per_image, within = block - image * a.g.blocks_per_image;
  const unsigned b = image / (unsigned)a.g.K;
  gather_thread(a.g, (int)b, (int)(image - b * (unsigned)a.g.K), (long long)within * kGatherThreads + thread);
}

// ---- host-side checks of a launch (before any launch; no device value is read): the row table's own, then gather_check of
// t2o_resident_math.h for the pictures, with the row workgroups in its grid bound.  0 with *a filled in, or 1 with `why`. ----
inline int items_check(const unsigned char* store, const long long* slots, const long long* index, int N, int K, int B, int h, int w,
                       float* out_x, float* out_ys, const int* rows, int V, int* out_rows, ItemsArgs* a, const char** why) {
  const char *who = "gather_items_u8_to_f32", *aligned = "store 16-byte, slots and index 8-byte, outputs and rows 4-byte aligned";
  if (V < 0) return gather_refuse(why, who, "V must not be negative");
  if ((V > 0) != (rows != nullptr) || (V > 0) != (out_rows != nullptr))
    return gather_refuse(why, who, "rows, out_rows and V do not agree (all three, or none with V = 0)");
  if (((size_t)rows & 3) || ((size_t)out_rows & 3)) return gather_refuse(why, who, aligned);
  const long long row_blocks = ((long long)B * V + kGatherThreads - 1) / kGatherThreads;
  long long per_image = 0;
  if (gather_check(store, slots, index, N, K, B, h, w, out_x, out_ys, &per_image, why, &a->g, who, kItemsMaxK, aligned, row_blocks)) return 1;
  a->rows = rows; a->out_rows = out_rows; a->V = V;
  a->picture_blocks = (unsigned)(per_image * K * B); a->row_blocks = (unsigned)row_blocks;
  return 0;
}

}  // namespace t2o
