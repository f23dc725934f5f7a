// Philox4x32-10 (Salmon et al., SC'11), the counter-based generator behind the sampler's noise (noise.hip) and the training
// step's dropout masks (moe_train.hip).  oracle/philox_ref.py restates it in numpy.  philox_normal4 is the sampler's gaussian
// draw: the element-to-counter mapping and the Box-Muller transform that every kernel drawing sampler noise shares.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace mdm {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
  c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
}

// 4 x 32 random bits for counter (c0, c1, c2, c3) under key (k0, k1): the standard 10-round Philox4x32
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// u in (0, 1]: (bits + 1) * 2^-32 evaluated exactly in fp32 steps that the numpy oracle repeats
__device__ __forceinline__ float philox_u01(uint32_t b) { return ((float)(b >> 8) + 1.0f) * (1.0f / 16777216.0f); }

// The four normals of elements [4 qd, 4 qd + 4) of global sample gs on noise stream `stream` under `seed`: one Philox call on
// counter (qd, gs lo, gs hi, stream), then Box-Muller on (u1, u2) = (c[2h], c[2h+1]).
__device__ __forceinline__ void philox_normal4(int64_t qd, uint64_t gs, uint32_t stream, uint64_t seed, float (&z)[4]) {
  uint32_t c[4] = {(uint32_t)qd, (uint32_t)gs, (uint32_t)(gs >> 32), stream};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = philox_u01(c[2 * h]), u2 = philox_u01(c[2 * h + 1]);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = r * cs, z[2 * h + 1] = r * sn;
  }
}

}  // namespace mdm
