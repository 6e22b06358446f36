// The per-thread program of the resident-set gather (t2o_resident.hip): a training batch read out of a device-resident
// store of already resized 8-bit pictures, by an index vector that lies on the device.
//
//   store   N x K slots, each an (h, w, 3) uint8 RGB picture in HWC order at store + slots[i * K + k]; -1 = the item has
//           no picture in column k (an unused step of a planned sequence).  The caller starts every slot on a 16-byte
//           boundary, so that pixel group g of a slot -- 12 bytes at 12 g -- is three aligned dwords.
//   output  image (b, k), i = index[b]: column 0 to out_x[b], columns 1 .. K-1 to out_ys[b, k - 1], each (3, h, w) fp32
//           planar, value = u8_to_unit(byte) -- what k_resize_u8_f32 writes for a source of the output's size.
//
// A thread owns four neighbouring pixels of one picture: three dword loads, one 16-byte store into each of the three
// planes (lanes walk the pixels: loads of a wave are 768 contiguous bytes, stores 1 KiB per plane).  The last
// h w % 4 pixels of a picture are read byte by byte and stored float by float; a slot that is not dword aligned (never
// one of ResidentFiveK's) is read byte by byte throughout.  Every output element has exactly one writer.
//
// `__host__ __device__` like t2o_image_math.h: tests/host_emul/emul_resident.cpp runs the same program with g++, thread
// by thread (a test harness, never a fallback).
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "t2o_image_math.h"

namespace t2o {

constexpr int kGatherThreads = 256;        // 4 waves of 64
constexpr int kGatherMaxK = 8;

struct GatherArgs {
  const unsigned char* store;
  const long long* slots;        // (N, K): byte offset of the slot counted from store, or -1
  const long long* index;        // (B): the items of the batch
  float* out_x;                  // (B, 3, hw)
  float* out_ys;                 // (B, K - 1, 3, hw)
  long long hw;                  // pixels of a picture
  int N, K, B;
  unsigned blocks_per_image;     // workgroups that share one (b, k)
};

// four floats at a 4-byte boundary (planes of an odd h w are not 16-byte aligned); the 12 source bytes of a group
struct GatherFloat4 { float x, y, z, w; };
struct GatherBytes12 { unsigned a, b, c; };

T2O_IMG_HD long long gather_groups(long long hw) { return (hw + 3) >> 2; }

// where image (b, k) goes
T2O_IMG_HD float* gather_dst(const GatherArgs& a, long long b, int k) {
  return k == 0 ? a.out_x + (size_t)b * 3 * (size_t)a.hw
                : a.out_ys + ((size_t)b * (size_t)(a.K - 1) + (size_t)(k - 1)) * 3 * (size_t)a.hw;
}

// the slot of image (b, k), or -1: absent, or an index outside [0, N) (the caller guarantees there is none; nothing is
// read through one)
T2O_IMG_HD long long gather_slot(const GatherArgs& a, long long b, int k) {
  const long long i = a.index[b];
  if (i < 0 || i >= (long long)a.N) return -1;
  return a.slots[(size_t)i * (size_t)a.K + (size_t)k];
}

// thread t of image (b, k): pixels 4 t .. 4 t + 3
T2O_IMG_HD void gather_thread(const GatherArgs& a, int b, int k, long long t) {
  const long long p0 = 4 * t;
  if (p0 >= a.hw) return;
  const long long slot = gather_slot(a, b, k);                       // (uniform over the workgroup)
  float* o = gather_dst(a, b, k) + p0;
  const size_t plane = (size_t)a.hw;
  const int n = a.hw - p0 >= 4 ? 4 : (int)(a.hw - p0);
  float v[3][4];
  if (slot < 0) {
    for (int c = 0; c < 3; ++c)
      for (int j = 0; j < 4; ++j) v[c][j] = 0.0f;
  } else {
    const unsigned char* src = a.store + slot + 3 * p0;
    if (n == 4 && ((size_t)src & 3) == 0) {
      const GatherBytes12 q = *reinterpret_cast<const GatherBytes12*>(src);
      const unsigned word[3] = {q.a, q.b, q.c};
      for (int j = 0; j < 4; ++j)
        for (int c = 0; c < 3; ++c) {
          const int at = 3 * j + c;                                  // byte number in the 12, little-endian dwords
          v[c][j] = u8_to_unit((int)((word[at >> 2] >> (8 * (at & 3))) & 255u));
        }
    } else {
      for (int j = 0; j < 4; ++j)
        for (int c = 0; c < 3; ++c) v[c][j] = j < n ? u8_to_unit((int)src[3 * j + c]) : 0.0f;
    }
  }
  if (n == 4) {
    for (int c = 0; c < 3; ++c) {
      GatherFloat4 f;
      f.x = v[c][0]; f.y = v[c][1]; f.z = v[c][2]; f.w = v[c][3];
      *reinterpret_cast<GatherFloat4*>(o + c * plane) = f;
    }
  } else {
    for (int c = 0; c < 3; ++c)
      for (int j = 0; j < n; ++j) o[c * plane + j] = v[c][j];
  }
}

// ---- host-side checks of a launch (before any launch; no device value is read), for t2o_gather_u8_to_f32 and, through
// items_check of t2o_resident_items_math.h, t2o_gather_items_u8_to_f32.  A refusal leaves "<entry point>: reason" in *why:
// a thread's buffer, good until its next refusal (t2o::set_error copies it).  `reason` may hold one %d, for n. ----
inline int gather_refuse(const char** why, const char* who, const char* reason, int n = 0) {
  static thread_local char text[160];
  const int at = snprintf(text, sizeof(text), "%s: ", who);
  snprintf(text + at, sizeof(text) - at, reason, n);
  *why = text;
  return 1;
}

// The parent form (what t2o_gather_u8_to_f32's host emulation calls): *blocks = the workgroups of one picture.  Behind it:
// a, filled in when given; who, max_k, aligned: the entry point's name, the pictures per item it takes and its alignment rule
// as its message states it; more_blocks: workgroups the caller appends behind the pictures' (they count in the grid bound).
inline int gather_check(const void* store, const void* slots, const void* index, int N, int K, int B, int h, int w, const void* out_x,
                        const void* out_ys, long long* blocks, const char** why, GatherArgs* a = nullptr,
                        const char* who = "gather_u8_to_f32", int max_k = kGatherMaxK,
                        const char* aligned = "store 16-byte, tables 8-byte, outputs 4-byte aligned", long long more_blocks = 0) {
  if (!store || !slots || !index || !out_x || (K > 1 && !out_ys)) return gather_refuse(why, who, "null pointer");
  if (N <= 0 || K <= 0 || B <= 0 || h <= 0 || w <= 0) return gather_refuse(why, who, "N, K, B, h and w must be positive");
  if (K > max_k) return gather_refuse(why, who, "at most %d pictures per item", max_k);
  if (((size_t)store & 15) || ((size_t)slots & 7) || ((size_t)index & 7) || ((size_t)out_x & 3) || ((size_t)out_ys & 3))
    return gather_refuse(why, who, aligned);
  const long long per_image = (gather_groups((long long)h * w) + kGatherThreads - 1) / kGatherThreads;
  if (per_image > (0x7fffffffll - more_blocks) / ((long long)K * B)) return gather_refuse(why, who, "more than 2^31 - 1 workgroups");
  *blocks = per_image;
  if (!a) return 0;
  a->store = (const unsigned char*)store; a->slots = (const long long*)slots; a->index = (const long long*)index;
  a->out_x = (float*)out_x; a->out_ys = (float*)out_ys;
  a->hw = (long long)h * w; a->blocks_per_image = (unsigned)per_image; a->N = N; a->K = K; a->B = B;
  return 0;
}

}  // namespace t2o
