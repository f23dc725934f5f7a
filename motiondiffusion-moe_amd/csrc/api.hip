// extern "C" surface of libmdm_hip.so (declared in include/mdm_hip.h).
#include "gemm.h"
#include "kernels.h"

namespace mdm {
namespace {

__global__ void pack_bf16_kernel(const float* __restrict__ src, int64_t ld_src, int64_t rows, int64_t K,
                                 uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, int64_t ld_dst) {
  const int64_t pairs_per_row = ld_dst >> 1;
  const int64_t total = rows * pairs_per_row;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / pairs_per_row, k = (i - r * pairs_per_row) * 2;
    const float a = k < K ? src[r * ld_src + k] : 0.f;
    const float b = k + 1 < K ? src[r * ld_src + k + 1] : 0.f;
    uint32_t h, l;
    split_bf16(a, b, h, l);
    *(uint32_t*)(hi + r * ld_dst + k) = h;
    if (lo) *(uint32_t*)(lo + r * ld_dst + k) = l;
  }
}

__global__ void pack_f16_kernel(const float* __restrict__ src, int64_t ld_src, int64_t rows, int64_t K,
                                uint16_t* __restrict__ dst, int64_t ld_dst) {
  const int64_t pairs_per_row = ld_dst >> 1;
  const int64_t total = rows * pairs_per_row;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / pairs_per_row, k = (i - r * pairs_per_row) * 2;
    const float a = k < K ? src[r * ld_src + k] : 0.f;
    const float b = k + 1 < K ? src[r * ld_src + k + 1] : 0.f;
    *(uint32_t*)(dst + r * ld_dst + k) = pack_f16(a, b);
  }
}

}  // namespace
}  // namespace mdm

namespace mdm {
int g_variant = MDM_VAR_DEFAULT;
}

extern "C" {

int mdm_set_gemm_variant(int v) {
  switch (v) {
    case MDM_VAR_DEFAULT:
    case MDM_VAR_GEMM_256:
    case MDM_VAR_SD_UNFOLDED:
    case MDM_VAR_GENERIC_DH256:
    case MDM_VAR_SD_FOLD_ANY:
    case MDM_VAR_ROUTER_CONST_E:
    case MDM_VAR_ROUTER_RUNTIME_E:
    case MDM_VAR_MLP_LDS:
    case MDM_VAR_TAIL_SPLIT:
    case MDM_VAR_X3_REG:
    case MDM_VAR_QKV_SPLIT:
    case MDM_VAR_XQ_SPLIT:
    case MDM_VAR_X3_ATTN_CHAIN:
    case MDM_VAR_X3_XATTN_CHAIN:
    case MDM_VAR_X3_STYLE_SPLIT:
    case MDM_VAR_X3_TAILS_SPLIT:
    case MDM_VAR_X3_F32_ROWS:
    case MDM_VAR_STREAM_NEVER:
    case MDM_VAR_STREAM_ALWAYS:
    case MDM_VAR_STREAM3_NEVER:
    case MDM_VAR_STREAM3_ALWAYS:
    case MDM_VAR_ROUTE_LAUNCH:
    case MDM_VAR_SKIP_LAUNCH:
    case MDM_VAR_NO_WARM:
    case MDM_VAR_TEXT_LAUNCH:
      mdm::g_variant = v;
      return MDM_OK;
    default:
      return MDM_ERR_ARG;
  }
}

const char* mdm_version(void) { return "mdm_hip 0.1 (gfx950)"; }

int mdm_gemm(const MdmGemmDesc* d, void* stream) {
  if (!d) return MDM_ERR_ARG;
  return mdm::gemm(*d, (hipStream_t)stream);
}

int mdm_fused_mlp(const MdmMlpDesc* d, void* stream) {
  if (!d) return MDM_ERR_ARG;
  return mdm::fused_mlp(*d, (hipStream_t)stream);
}

int64_t mdm_mlp_stream_elems(int32_t G, int32_t F, int32_t Din, int32_t Dout) { return mdm::mlp_stream_elems(G, F, Din, Dout); }

int mdm_mlp_stream_pack(const float* w1, const float* w2, int32_t G, int32_t F, int32_t Din, int32_t Dout, int32_t h16,
                        uint16_t* out, void* stream) {
  return mdm::mlp_stream_pack(w1, w2, G, F, Din, Dout, h16, out, (hipStream_t)stream);
}

int64_t mdm_gemm_stream_elems(int32_t N, int32_t K) { return mdm::gemm_stream_elems(N, K); }

int mdm_gemm_stream_pack(const float* w, int32_t N, int32_t K, int32_t h16, uint16_t* out, void* stream) {
  return mdm::gemm_stream_pack(w, N, K, h16, out, (hipStream_t)stream);
}

int64_t mdm_gemm_stream1_elems(int32_t N, int32_t K) { return mdm::gemm_stream1_elems(N, K); }

int mdm_gemm_stream1_pack(const float* w, int64_t ldw, int32_t N, int32_t K, int32_t h16, uint16_t* out, void* stream) {
  return mdm::gemm_stream1_pack(w, ldw, N, K, h16, out, (hipStream_t)stream);
}

int64_t mdm_gemm_stream3x_elems(int32_t G, int32_t N, int32_t K) { return mdm::gemm_stream3x_elems(G, N, K); }

int64_t mdm_gemm_stream3x_group_elems(int32_t N, int32_t K) { return mdm::gemm_stream3x_group_elems(N, K); }

int mdm_gemm_stream3x_pack(const float* w, int64_t ldw, int32_t G, int32_t N, int32_t K, uint16_t* out, void* stream) {
  return mdm::gemm_stream3x_pack(w, ldw, G, N, K, out, (hipStream_t)stream);
}

int64_t mdm_gemm_stream3_elems(int32_t N, int32_t K) { return mdm::gemm_stream3_elems(N, K); }

int mdm_gemm_stream3_pack(const float* w, int32_t N, int32_t K, uint16_t* out, void* stream) {
  return mdm::gemm_stream3_pack(w, N, K, out, (hipStream_t)stream);
}

int mdm_pack_bf16(const float* src, int64_t ld_src, int64_t rows, int64_t K, uint16_t* hi, uint16_t* lo,
                  int64_t ld_dst, void* stream) {
  if (!src || !hi || rows < 0 || K <= 0 || ld_dst < K || (ld_dst & 31)) return MDM_ERR_ARG;
  if (rows == 0) return MDM_OK;
  const int64_t total = rows * (ld_dst >> 1);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mdm::pack_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, ld_src, rows, K, hi,
                     lo, ld_dst);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int mdm_pack_f16(const float* src, int64_t ld_src, int64_t rows, int64_t K, uint16_t* dst, int64_t ld_dst, void* stream) {
  if (!src || !dst || rows < 0 || K <= 0 || ld_dst < K || (ld_dst & 31)) return MDM_ERR_ARG;
  if (rows == 0) return MDM_OK;
  const int64_t total = rows * (ld_dst >> 1);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mdm::pack_f16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, ld_src, rows, K, dst, ld_dst);
  MDM_RETURN_IF_LAUNCH_FAILED();
  return MDM_OK;
}

int mdm_fill_i64(int64_t* dst, int64_t n, const int32_t* src_dev, void* stream) {
  if (!dst || !src_dev) return MDM_ERR_ARG;
  return mdm::fill_i64(dst, n, src_dev, (hipStream_t)stream);
}

int mdm_add_i32(int32_t* dst, int32_t delta, void* stream) {
  if (!dst) return MDM_ERR_ARG;
  return mdm::add_i32(dst, delta, (hipStream_t)stream);
}

}  // extern "C"
