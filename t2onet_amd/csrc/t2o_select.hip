// t2o_select.hip -- the mask planes of a local edit made from a RULE where the photo already lies: up to 4 uint8 planes,
// each the product of 1..4 terms (a luminance, saturation or hue range of the photo's own bytes, a linear or radial
// gradient over the frame, an existing plane), in ONE launch that covers every job of the call.
//
//   k_select_u8   grid (max tiles over the jobs, J); a workgroup owns 4096 pixels of one plane taken as a stream, a lane
//                 four neighbouring pixels at a time: 12 source bytes at any alignment in, one aligned plane dword out,
//                 single bytes at the two ends of a misaligned plane.  3 + 1 bytes per pixel plus 1 per plane term (the
//                 3 only where a job has a colour term).
// The per-pixel and the lane program are t2o_select_math.h's.  The job table travels in the kernel arguments: no
// workspace, no allocation, no host synchronisation, no float, no atomics; deterministic, capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "t2o_select_math.h"
#include "t2onet_hip.h"

namespace t2o { int set_error(int code, const char* msg); }
using namespace t2o;

static_assert(sizeof(SelectArgs) <= 2048, "the job table must fit the kernel arguments");
static_assert(sizeof(SelectTerm) == sizeof(t2o_select_term_t) && sizeof(SelectJob) == sizeof(t2o_select_job_t), "header and kernel agree");
static_assert(kSelectMaxJobs == T2O_SELECT_MAX_JOBS && kSelectMaxTerms == T2O_SELECT_MAX_TERMS, "header and kernel agree");
static_assert(SELECT_LUM == T2O_SELECT_LUM && SELECT_SAT == T2O_SELECT_SAT && SELECT_HUE == T2O_SELECT_HUE &&
              SELECT_LINEAR == T2O_SELECT_LINEAR && SELECT_RADIAL == T2O_SELECT_RADIAL && SELECT_PLANE == T2O_SELECT_PLANE, "header and kernel agree");

namespace {

__global__ __launch_bounds__(kSelectThreads) void k_select_u8(const SelectArgs a) {
  select_thread(a, (int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x);
}

bool within(int v, int lo, int hi) { return lo <= v && v <= hi; }

const char* term_fault(const t2o_select_term_t& t, int h, int w) {
  if (t.invert != 0 && t.invert != 1) return "select_u8: invert must be 0 or 1";
  const int* p = t.p;
  switch (t.kind) {
    case T2O_SELECT_LUM:
    case T2O_SELECT_SAT:
      if (!(0 <= p[0] && p[0] <= p[1] && p[1] <= 255)) return "select_u8: lum / sat range needs 0 <= lo <= hi <= 255";
      if (!within(p[2], 0, 255)) return "select_u8: lum / sat soft must lie in 0..255";
      return nullptr;
    case T2O_SELECT_HUE:
      if (!within(p[0], 0, kSelectHueSteps - 1) || !within(p[1], 0, kSelectHueSteps - 1)) return "select_u8: hue bounds must lie in 0..1535";
      if (!within(p[2], 0, kSelectHueSteps / 2)) return "select_u8: hue soft must lie in 0..768";
      return nullptr;
    case T2O_SELECT_LINEAR:
    case T2O_SELECT_RADIAL:
      if (h > kSelectMaxSide || w > kSelectMaxSide) return "select_u8: a position term needs h, w <= 65535";
      for (int k = 0; k < 4; ++k)
        if (!within(p[k], -kSelectMaxCoord, kSelectMaxCoord)) return "select_u8: position parameters must lie within +-131070";
      if (t.kind == T2O_SELECT_LINEAR && p[0] == p[2] && p[1] == p[3]) return "select_u8: the end points of a linear term are equal";
      if (t.kind == T2O_SELECT_RADIAL && !(0 <= p[2] && p[2] < p[3])) return "select_u8: radial needs 0 <= RI < RO";
      return nullptr;
    case T2O_SELECT_PLANE:
      return t.plane_offset < 0 ? "select_u8: negative offset" : nullptr;
    default:
      return "select_u8: unknown term kind";
  }
}

bool overlap(uintptr_t a, long long na, uintptr_t b, long long nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

// the checks of the C ABI; returns nullptr or the reason for T2O_EINVAL
const char* select_fault(const unsigned char* src, unsigned char* out, const t2o_select_job_t* jobs, int J) {
  if (!src || !out || !jobs) return "select_u8: null pointer";
  if (J <= 0 || J > kSelectMaxJobs) return "select_u8: 1 <= J <= 4 jobs per call";
  for (int i = 0; i < J; ++i) {
    const t2o_select_job_t& s = jobs[i];
    if (s.h <= 0 || s.w <= 0) return "select_u8: h and w must be positive";
    if ((long long)s.h * s.w >= (1ll << 31)) return "select_u8: h * w must stay below 2^31";
    if (s.src_offset < 0 || s.out_offset < 0) return "select_u8: negative offset";
    if (s.n_terms <= 0 || s.n_terms > kSelectMaxTerms) return "select_u8: 1 <= n_terms <= 4 terms per job";
    for (int t = 0; t < s.n_terms; ++t)
      if (const char* why = term_fault(s.terms[t], s.h, s.w)) return why;
  }
  // one writer per byte, and no job reads what another one writes: by absolute address, so that src == out (or two
  // views of one buffer) is covered
  for (int i = 0; i < J; ++i) {
    const long long n = (long long)jobs[i].h * jobs[i].w;
    const uintptr_t dst = (uintptr_t)out + (uintptr_t)jobs[i].out_offset;
    for (int k = 0; k < i; ++k)
      if (overlap(dst, n, (uintptr_t)out + (uintptr_t)jobs[k].out_offset, (long long)jobs[k].h * jobs[k].w)) return "select_u8: two jobs' destinations overlap";
    for (int k = 0; k < J; ++k) {
      const long long m = (long long)jobs[k].h * jobs[k].w;
      if (overlap(dst, n, (uintptr_t)src + (uintptr_t)jobs[k].src_offset, 3 * m)) return "select_u8: a destination overlaps a photo of the call";
      for (int t = 0; t < jobs[k].n_terms; ++t)
        if (jobs[k].terms[t].kind == T2O_SELECT_PLANE && overlap(dst, n, (uintptr_t)src + (uintptr_t)jobs[k].terms[t].plane_offset, m))
          return "select_u8: a destination overlaps a plane term of the call";
    }
  }
  return nullptr;
}

}  // namespace

extern "C" int t2o_select_u8(const unsigned char* src, unsigned char* out, const t2o_select_job_t* jobs, int J, void* stream) {
  if (const char* why = select_fault(src, out, jobs, J)) return set_error(T2O_EINVAL, why);
  SelectArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.out = out;
  memcpy(a.jobs, jobs, (size_t)J * sizeof(SelectJob));
  int tiles = 0;
  for (int i = 0; i < J; ++i) select_prepare(a.jobs[i]);
  for (int i = 0; i < J; ++i) tiles = select_tiles(a.jobs[i], out) > tiles ? select_tiles(a.jobs[i], out) : tiles;
  k_select_u8<<<dim3((unsigned)tiles, (unsigned)J), kSelectThreads, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? T2O_OK : set_error(T2O_ELAUNCH, "select_u8: launch failed");
}
