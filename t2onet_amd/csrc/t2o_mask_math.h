// The per-thread programs of the mask kernels (t2o_mask.hip): the local-edit masks of the GIER half of the reference,
// built and chosen on the device.
//
//   union    data/GIER/GIER.py:288-307 (resize_and_union_mask) without a native-size plane: a candidate mask stays what its
//            file holds, COCO run lengths (column-major over size = [h, w], zeros first), uploaded as CUMULATIVE run ends.
//            For output pixel (oy, ox) of an (out_h, out_w) plane the source pixel is OpenCV's INTER_NEAREST one,
//                sy = min(floor(oy * (h / out_h)), h - 1),  sx = min(floor(ox * (w / out_w)), w - 1)       (double)
//            -- edit.nearest_index, operation for operation -- and i = sx * h + sy its place in the run-length order.  The
//            run that holds i is the first one whose cumulative end exceeds i (an upper-bound search; empty runs are
//            passed over by it), the mask's value is that run's index parity, and the output byte is the SUM of the values
//            over the job's selection -- a count, as masks.sum(0).astype(uint8) is; overlapping masks give 2, a repeated id
//            counts twice, an empty selection gives 0.  The sum saturates at 255.
//            A thread owns one ALIGNED dword of the output buffer: a plane is h * w abutting bytes at any byte offset, so
//            the dwords that lie wholly inside it are stored whole and its first and last up to three bytes one by one.
//            No byte outside the plane is written.
//   select   models/actor.py:78-98 (get_gt_mask) for the operator each sample has just chosen, as (B,1,H,W) fp32:
//            out[b] = float(planes[slot[b][op[b]]]), all ones where the slot is -1 (no entry: a global edit) or the
//            operator lies outside [0, V).  A thread owns one aligned group of four floats of the output.
//
// `__host__ __device__` programs -- what ONE thread does -- so that tests/host_emul/emul_mask.cpp runs them thread by
// thread with g++ (a test harness, never a fallback).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "t2o_pixel_math.h"

namespace t2o {

constexpr int kMaskThreads = 256;          // 4 waves of 64

// t2o_rle_mask_t / t2o_union_job_t of include/t2onet_hip.h, field for field
struct RleMask {
  unsigned first_end;        // index of the mask's first cumulative end in the `ends` array
  int n_runs, h, w;
};

struct UnionJob {
  int first_sel, n_sel;      // the job's masks: sel[first_sel .. first_sel + n_sel)
  int out_h, out_w;
  long long out_offset;      // first byte of the (out_h, out_w) plane, counted from `out`
};

struct UnionArgs {
  const UnionJob* jobs;
  const RleMask* masks;
  const int* sel;
  const unsigned* ends;
  unsigned char* out;
};

// edit.nearest_index for one destination sample: the scale src / dst in double (mask_scale), the product, the floor, the clamp
T2O_HD double mask_scale(int src, int dst) { return (double)src / (double)dst; }

T2O_HD int mask_nearest(int o, int src, double scale) {
  const long long s = (long long)floor((double)o * scale);
  return s < (long long)(src - 1) ? (int)s : src - 1;
}

struct alignas(16) MaskFloat4 { float x, y, z, w; };

// the run that holds position i: the first r in [0, n) with ends[r] > i (the caller guarantees ends[n - 1] > i)
T2O_HD int mask_run_of(const unsigned* ends, int n, unsigned i) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ends[mid] > i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the dwords (aligned in the output BUFFER) that a job's plane touches
T2O_HD long long union_job_dwords(const UnionJob& j, size_t out_address) {
  const long long first = (long long)((out_address + (size_t)j.out_offset) & 3);
  return (first + (long long)j.out_h * j.out_w + 3) >> 2;
}

// the union bytes of output pixels p0 .. p0 + 3 (flat, row-major) of job j, those outside [0, n) as 0, little-endian in a dword;
// per mask the four pixels are searched one after the other and a pixel that falls into the run found last is not searched
T2O_HD unsigned union_four(const UnionArgs& a, const UnionJob& j, long long p0, long long n) {
  int sum[4] = {0, 0, 0, 0};
  int oy = p0 >= 0 ? (int)p0 / j.out_w : 0, ox = p0 >= 0 ? (int)p0 % j.out_w : 0;      // (n < 2^31)
  int pyx[4][2];
  T2O_UNROLL
  for (int k = 0; k < 4; ++k) {
    pyx[k][0] = oy; pyx[k][1] = ox;
    if (p0 + k >= 0 && ++ox == j.out_w) { ox = 0; ++oy; }
  }
  for (int s = 0; s < j.n_sel; ++s) {
    const RleMask m = a.masks[a.sel[j.first_sel + s]];
    const unsigned* ends = a.ends + m.first_end;
    const double scale_y = mask_scale(m.h, j.out_h), scale_x = mask_scale(m.w, j.out_w);
    unsigned lo = 1, hi = 0;             // positions [lo, hi) of the run found last: empty at first
    int val = 0;
    T2O_UNROLL
    for (int k = 0; k < 4; ++k) {
      const long long p = p0 + k;
      if (p < 0 || p >= n) continue;
      const unsigned i = (unsigned)mask_nearest(pyx[k][1], m.w, scale_x) * (unsigned)m.h + (unsigned)mask_nearest(pyx[k][0], m.h, scale_y);
      if (!(i >= lo && i < hi)) {
        const int r = mask_run_of(ends, m.n_runs, i);
        lo = r > 0 ? ends[r - 1] : 0u;
        hi = ends[r];
        val = r & 1;
      }
      sum[k] += val;
    }
  }
  unsigned word = 0;
  T2O_UNROLL
  for (int k = 0; k < 4; ++k) word |= (unsigned)(sum[k] > 255 ? 255 : sum[k]) << (8 * k);
  return word;
}

// thread t of job `job`: the aligned dword number t of the plane
T2O_HD void union_thread(const UnionArgs& a, int job, long long t) {
  const UnionJob j = a.jobs[job];
  unsigned char* plane = a.out + j.out_offset;
  const long long n = (long long)j.out_h * j.out_w;
  const long long first = (long long)((size_t)plane & 3);          // bytes of the first dword that lie in front of the plane
  const long long p0 = 4 * t - first;                                  // the flat pixel of the dword's byte 0
  if (p0 >= n) return;
  const unsigned word = union_four(a, j, p0, n);
  if (p0 >= 0 && p0 + 4 <= n) {
    *reinterpret_cast<unsigned*>(plane + p0) = word;
  } else {
    T2O_UNROLL
    for (int k = 0; k < 4; ++k)
      if (p0 + k >= 0 && p0 + k < n) plane[p0 + k] = (unsigned char)(word >> (8 * k));
  }
}

struct SelectArgs {
  const unsigned char* planes;   // (N, H*W) uint8
  const int* slot;               // (B, V): a plane number or -1
  const long long* op;           // (B) int64: the operator each sample chose
  float* out;                    // (B, 1, H*W) fp32
  long long hw;
  int N, B, V;
};

// the plane of sample b, or -1 for all ones
T2O_HD int select_plane(const SelectArgs& a, int b) {
  const long long op = a.op[b];
  if (op < 0 || op >= (long long)a.V) return -1;
  const int p = a.slot[(size_t)b * a.V + (size_t)op];
  return (p < 0 || p >= a.N) ? -1 : p;
}

// thread t of sample b: the 16-byte aligned group number t of the sample's floats
T2O_HD void select_thread(const SelectArgs& a, int b, long long t) {
  float* out = a.out + (size_t)b * (size_t)a.hw;
  const long long first = (long long)(((size_t)out >> 2) & 3);        // floats of the first group in front of the sample
  const long long p0 = 4 * t - first;
  if (p0 >= a.hw) return;
  const int p = select_plane(a, b);
  const unsigned char* plane = a.planes + (size_t)(p < 0 ? 0 : p) * (size_t)a.hw;
  const bool whole = p0 >= 0 && p0 + 4 <= a.hw;
  float v[4];
  if (p >= 0 && whole && ((size_t)(plane + p0) & 3) == 0) {           // four mask bytes as one aligned dword
    const unsigned word = *reinterpret_cast<const unsigned*>(plane + p0);
    T2O_UNROLL
    for (int k = 0; k < 4; ++k) v[k] = (float)((word >> (8 * k)) & 255u);
  } else {
    T2O_UNROLL
    for (int k = 0; k < 4; ++k) {
      const long long q = p0 + k;
      v[k] = (p < 0 || q < 0 || q >= a.hw) ? 1.0f : (float)plane[q];
    }
  }
  if (whole) {
    MaskFloat4 w4;
    w4.x = v[0]; w4.y = v[1]; w4.z = v[2]; w4.w = v[3];
    *reinterpret_cast<MaskFloat4*>(out + p0) = w4;
  } else {
    T2O_UNROLL
    for (int k = 0; k < 4; ++k)
      if (p0 + k >= 0 && p0 + k < a.hw) out[p0 + k] = v[k];
  }
}

// ---- host-side checks of a union launch (before any launch; no device value is read) ----
// 0, or 1 with *why set.  Tables as the HOST holds them.  out_bytes: the size of the output buffer.
inline int union_check(const UnionJob* jobs, int n_jobs, const RleMask* masks, int n_masks, const int* sel, int n_sel,
                       const unsigned* ends, long long n_ends, long long out_bytes, const char** why) {
  for (int m = 0; m < n_masks; ++m) {
    const RleMask& k = masks[m];
    if (k.h <= 0 || k.w <= 0 || k.n_runs <= 0) { *why = "rle_union_u8: mask sizes and run counts must be positive"; return 1; }
    if ((long long)k.h * k.w >= 0x80000000ll) { *why = "rle_union_u8: a mask of 2^31 pixels or more"; return 1; }
    if ((long long)k.first_end + k.n_runs > n_ends) { *why = "rle_union_u8: a mask's runs lie outside the run array"; return 1; }
    const unsigned* e = ends + k.first_end;
    for (int r = 1; r < k.n_runs; ++r)
      if (e[r] < e[r - 1]) { *why = "rle_union_u8: cumulative run ends must not decrease"; return 1; }
    if ((long long)e[k.n_runs - 1] != (long long)k.h * k.w) { *why = "rle_union_u8: a mask's runs do not add up to h * w"; return 1; }
  }
  for (int s = 0; s < n_sel; ++s)
    if (sel[s] < 0 || sel[s] >= n_masks) { *why = "rle_union_u8: a selection index outside the mask table"; return 1; }
  for (int i = 0; i < n_jobs; ++i) {
    const UnionJob& j = jobs[i];
    if (j.out_h <= 0 || j.out_w <= 0) { *why = "rle_union_u8: plane sizes must be positive"; return 1; }
    if ((long long)j.out_h * j.out_w >= 0x80000000ll) { *why = "rle_union_u8: a plane of 2^31 pixels or more"; return 1; }
    if (j.n_sel < 0 || j.first_sel < 0 || (long long)j.first_sel + j.n_sel > n_sel) { *why = "rle_union_u8: a job's selection lies outside the selection list"; return 1; }
    if (j.out_offset < 0 || j.out_offset + (long long)j.out_h * j.out_w > out_bytes) { *why = "rle_union_u8: a plane lies outside the output buffer"; return 1; }
  }
  return 0;
}

}  // namespace t2o
