// Long-motion handshakes: the windows of one long motion are rows of one sampler batch, and every canvas
// frame that two (or more) windows cover is made equal in all of them on every step.
//   blend mode (weights != NULL): v = fmaf chain of weights[e] * x[row e] over the frame's entries, in entry order, then
//                                 v written to every entry (the step's eps rows, every row group)
//   copy mode  (weights == NULL): the frame's first entry (the owner window) copied bit for bit to the others (x_T, noise)
// One thread per (group, shared frame, feature): consecutive threads walk the features of one frame row, so every load and
// store of a wavefront is one contiguous run.  The entries of a shared frame are that frame's rows in its windows, and the
// window frames of different canvas frames are disjoint (host tables), so each element belongs to one thread: in place is
// safe and needs no barrier.  Memory-bound; no LDS.
#include "kernels.h"

namespace mdm {
namespace {

constexpr int HS_THREADS = 256;

template <bool COPY>
__global__ __launch_bounds__(HS_THREADS) void handshake_kernel(float* x, int64_t group_stride, int F, int nshared,
                                                               int64_t total, const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ rows,
                                                               const float* __restrict__ weights) {
  const int64_t i = (int64_t)blockIdx.x * HS_THREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t gc = i / F;
  const int j = (int)(i - gc * F);
  const int64_t g = gc / nshared;
  const int c = (int)(gc - g * nshared);
  float* xg = x + g * group_stride + j;
  const int e0 = offsets[c], e1 = offsets[c + 1];
  if (e1 <= e0) return;
  float v;
  if (COPY) {
    v = xg[(int64_t)rows[e0] * F];
  } else {
    v = 0.f;
    for (int e = e0; e < e1; ++e) v = fmaf(weights[e], xg[(int64_t)rows[e] * F], v);
  }
  for (int e = COPY ? e0 + 1 : e0; e < e1; ++e) xg[(int64_t)rows[e] * F] = v;
}

}  // namespace
}  // namespace mdm

extern "C" {

int mdm_handshake_blend(float* x, int32_t groups, int64_t group_stride, int32_t F, int32_t nshared,
                        const int32_t* offsets, const int32_t* rows, const float* weights, void* stream) {
  if (nshared < 0 || F < 1 || groups < 1 || group_stride < 0) return MDM_ERR_ARG;
  if (nshared == 0) return MDM_OK;
  if (!x || !offsets || !rows) return MDM_ERR_ARG;
  const int64_t total = (int64_t)groups * nshared * F;
  const int64_t blocks = (total + mdm::HS_THREADS - 1) / mdm::HS_THREADS;
  if (blocks > 0x7FFFFFFF) return MDM_ERR_ARG;
  if (weights)
    hipLaunchKernelGGL((mdm::handshake_kernel<false>), dim3((unsigned)blocks), dim3(mdm::HS_THREADS), 0,
                       (hipStream_t)stream, x, group_stride, F, nshared, total, offsets, rows, weights);
  else
    hipLaunchKernelGGL((mdm::handshake_kernel<true>), dim3((unsigned)blocks), dim3(mdm::HS_THREADS), 0,
                       (hipStream_t)stream, x, group_stride, F, nshared, total, offsets, rows, nullptr);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

}  // extern "C"
