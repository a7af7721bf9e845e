// paged_adamw_8bit (train.py:2271-2288 -> bitsandbytes PagedAdamW8bit): blockwise 8-bit AdamW over many tensors in one launch.
// The arithmetic is the project's restatement of bitsandbytes' blockwise kernel (tests/adamw8bit_ref.py):
// fp32, one rounding per operation, no contraction, correctly rounded division and square root.
//
// One wave64 owns one 256-element block of a tensor's LOGICAL flat order per iteration of a grid-stride loop over the global block
// index: decode the two codes with the block's old absmax, update m / v, wave-reduce the new absmax (cross-lane, no LDS barrier),
// update the parameter, re-encode by an 8-step binary search in the two maps kept in LDS.  fp32-state tensors (numel < 4096) are
// blocks of the same launch with a flag.  Lanes may take a block's elements in any order (max is order-independent); permuted 4-D
// weights (stored (O, kh, kw, I_pad), logical (O, I, kh, kw)) are walked in storage-contiguous runs of the block's elements.
#include "az_common.h"
#include "aozora_hip.h"

namespace {

constexpr int BLK = 256;      // elements per quantisation block
constexpr int SLOTS = 5;      // elements per lane: 4 for a plain block, up to 5 for a permuted one
constexpr int WAVES = 4;      // waves per workgroup

// descriptor words (int64), one record per tensor; the prefix table (ntensors + 1 first-block indices) follows the records
enum { D_P, D_G, D_S1, D_S2, D_A1, D_A2, D_NUMEL, D_FIRST, D_FLAGS, D_S, D_I, D_GROUP, D_WORDS };
enum { F_8BIT = 1, F_PERM = 2, F_VEC = 4 };

struct Hyper { float b1, b2, omb1, omb2, step, eps_c, decay, wd_pos; };

__device__ __forceinline__ int encode(float x, const float* q) {
#pragma clang fp contract(off)
  int lo = 0;
#pragma unroll
  for (int s = 128; s > 0; s >>= 1)
    if (q[lo + s] <= x) lo += s;
  const int hi = lo < 255 ? lo + 1 : 255;
  return ((q[hi] - x) < (x - q[lo])) ? hi : lo;
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}

__device__ __forceinline__ float param_update(float p, float g, float m, float v, const Hyper& h) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(g)) return p;
  float pn = bf2f(f2bf(p + h.step * (m / (sqrtf(v) + h.eps_c))));
  if (h.wd_pos != 0.0f) pn = bf2f(f2bf(pn * h.decay));
  return pn;
}

__global__ void __launch_bounds__(WAVES * 64) adamw8bit_kernel(int ntensors, const long* __restrict__ desc, long nblocks,
                                                                const float* __restrict__ hyper, const float* __restrict__ qmaps,
                                                                const float* __restrict__ coef) {
#pragma clang fp contract(off)
  __shared__ float q1[256], q2[256];
  for (int i = threadIdx.x; i < 512; i += blockDim.x) (i < 256 ? q1[i] : q2[i - 256]) = qmaps[i];
  __syncthreads();
  const long* first = desc + (long)ntensors * D_WORDS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float gc = coef ? coef[0] : 1.0f;
  int t = 0;
  for (long b = (long)blockIdx.x * WAVES + wave; b < nblocks; b += (long)gridDim.x * WAVES) {
    // the tensor of block b: blocks only grow along the loop, so step forward (a few steps linearly, then bisect)
    int steps = 0;
    while (t + 1 < ntensors && first[t + 1] <= b && steps < 4) { ++t; ++steps; }
    if (t + 1 < ntensors && first[t + 1] <= b) {
      int lo = t + 1, hi = ntensors - 1;        // first[lo] <= b; find the last such index
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= b) lo = mid; else hi = mid - 1; }
      t = lo;
    }
    t = __builtin_amdgcn_readfirstlane(t);
    const long* d = desc + (long)t * D_WORDS;
    const long numel = d[D_NUMEL], flags = d[D_FLAGS];
    const long blk = b - d[D_FIRST];
    const long L0 = blk * BLK;
    const int n = (int)(numel - L0 < BLK ? numel - L0 : BLK);
    const float* hp = hyper + d[D_GROUP] * 8;
    const Hyper h{hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7]};
    bf16_t* P = (bf16_t*)d[D_P];
    const bf16_t* G = (const bf16_t*)d[D_G];

    // element slots of this lane: logical index L[k] (in [L0, L0 + n) when ok[k]) and storage index S[k]
    long L[SLOTS], S[SLOTS];
    bool ok[SLOTS];
    if (flags & F_PERM) {
      // logical L = q * KS + s with q = o * I + i; storage (o * KS + s) * I_pad + i.  The block covers q0..q1; slot j of the block
      // takes s = j / Q, q = q0 + j % Q, so consecutive lanes walk consecutive i of one (o, s): storage-contiguous runs.
      // KS <= 32 and numel < 2^31 (host checks): KS*Q <= 255 + 2*KS <= 319 < 64 * SLOTS.
      const uint32_t KS = (uint32_t)d[D_S], I = (uint32_t)(d[D_I] & 0xFFFFFFFF), Ipad = (uint32_t)(d[D_I] >> 32);
      const uint32_t l0 = (uint32_t)L0, q0 = l0 / KS, Q = (l0 + n - 1) / KS - q0 + 1;
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        const uint32_t j = lane + 64 * k;
        const uint32_t s = j / Q, q = q0 + (j - s * Q);
        const uint32_t l = q * KS + s;
        ok[k] = j < KS * Q && l >= l0 && l < l0 + n;
        const uint32_t o = q / I, i = q - o * I;
        L[k] = l;
        S[k] = ((long)o * KS + s) * Ipad + i;
      }
    } else {
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        L[k] = L0 + lane * 4 + k;
        ok[k] = k < 4 && lane * 4 + k < n;
        S[k] = L[k];
      }
    }
    const bool perm = (flags & F_PERM) != 0;     // plain blocks use slots 0..3 only
    const bool vec = (flags & F_VEC) && n == BLK;   // plain, full block, 8-byte aligned p / g: vector loads and stores

    float g[SLOTS], p[SLOTS];
    if (vec) {
      const uint2 pu = *(const uint2*)(P + L0 + lane * 4), gu = *(const uint2*)(G + L0 + lane * 4);
      const uint32_t pw[2] = {pu.x, pu.y}, gw[2] = {gu.x, gu.y};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p[k] = bf2f((bf16_t)(pw[k >> 1] >> (16 * (k & 1))));
        g[k] = bf2f((bf16_t)(gw[k >> 1] >> (16 * (k & 1))));
      }
      p[4] = g[4] = 0.0f;
    } else {
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        p[k] = ok[k] ? bf2f(P[S[k]]) : 0.0f;
        g[k] = ok[k] ? bf2f(G[S[k]]) : 0.0f;
      }
    }
    if (coef) {
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) g[k] = bf2f(f2bf(g[k] * gc));
    }

    float m[SLOTS], v[SLOTS];
    if (flags & F_8BIT) {
      uint8_t* C1 = (uint8_t*)d[D_S1];
      uint8_t* C2 = (uint8_t*)d[D_S2];
      float* A1 = (float*)d[D_A1];
      float* A2 = (float*)d[D_A2];
      const float a1o = A1[blk], a2o = A2[blk];
      int c1[SLOTS], c2[SLOTS];
      if (vec) {
        const uint32_t u1 = *(const uint32_t*)(C1 + L0 + lane * 4), u2 = *(const uint32_t*)(C2 + L0 + lane * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { c1[k] = (u1 >> (8 * k)) & 255; c2[k] = (u2 >> (8 * k)) & 255; }
        c1[4] = c2[4] = 0;
      } else {
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) { c1[k] = ok[k] ? C1[L[k]] : 0; c2[k] = ok[k] ? C2[L[k]] : 0; }
      }
      float mx1 = 0.0f, mx2 = 0.0f;
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        float mm = q1[c1[k]] * a1o, vv = q2[c2[k]] * a2o;
        vv = vv * h.b2 + (h.omb2 * g[k]) * g[k];
        mm = mm * h.b1 + h.omb1 * g[k];
        m[k] = mm; v[k] = vv;
        if (ok[k]) { mx1 = fmaxf(mx1, fabsf(mm)); mx2 = fmaxf(mx2, fabsf(vv)); }
      }
      const float a1 = wave_max(mx1), a2 = wave_max(mx2);
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        if (k == SLOTS - 1 && !perm) break;
        int e1, e2;
        if (a1 == 0.0f) e1 = 127;   // index of 0.0 in the signed map
        else {
          e1 = encode(m[k] / a1, q1);
          const bool neg = __builtin_signbit(q1[e1]);
          if (m[k] > 0.0f && neg) ++e1;
          else if (m[k] < 0.0f && !neg) --e1;
        }
        e2 = a2 == 0.0f ? 0 : encode(v[k] / a2, q2);   // index of 0.0 in the unsigned map
        c1[k] = e1; c2[k] = e2;
      }
      if (vec) {
        uint32_t u1 = 0, u2 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { u1 |= (uint32_t)c1[k] << (8 * k); u2 |= (uint32_t)c2[k] << (8 * k); }
        *(uint32_t*)(C1 + L0 + lane * 4) = u1;
        *(uint32_t*)(C2 + L0 + lane * 4) = u2;
      } else {
#pragma unroll
        for (int k = 0; k < SLOTS; ++k)
          if (ok[k]) { C1[L[k]] = (uint8_t)c1[k]; C2[L[k]] = (uint8_t)c2[k]; }
      }
      if (lane == 0) { A1[blk] = a1; A2[blk] = a2; }
    } else {
      float* M = (float*)d[D_S1];
      float* V = (float*)d[D_S2];
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        if (!ok[k]) { m[k] = v[k] = 0.0f; continue; }
        float mm = M[L[k]] * h.b1 + h.omb1 * g[k];
        float vv = V[L[k]] * h.b2 + h.omb2 * (g[k] * g[k]);
        M[L[k]] = mm; V[L[k]] = vv;
        m[k] = mm; v[k] = vv;
      }
    }

#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
      if (k < SLOTS - 1 || perm) p[k] = param_update(p[k], g[k], m[k], v[k], h);
    if (vec) {
      uint2 pu;
      pu.x = (uint32_t)f2bf(p[0]) | ((uint32_t)f2bf(p[1]) << 16);
      pu.y = (uint32_t)f2bf(p[2]) | ((uint32_t)f2bf(p[3]) << 16);
      *(uint2*)(P + L0 + lane * 4) = pu;
    } else {
#pragma unroll
      for (int k = 0; k < SLOTS; ++k)
        if (ok[k]) P[S[k]] = f2bf(p[k]);
    }
  }
}

}  // namespace

extern "C" {

int az_adamw8bit_step(int ntensors, const void* desc, long nblocks, const void* hyper, const void* qmaps, const void* coef,
                      void* stream) {
  if (ntensors <= 0 || nblocks <= 0 || !desc || !hyper || !qmaps) return AZ_ERR_ARG(90);
  long grid = (nblocks + WAVES - 1) / WAVES;
  if (grid > 1280) grid = 1280;     // one resident round: 256 CUs x 5 workgroups (5 waves per SIMD at 84 VGPRs)
  az_launch(adamw8bit_kernel, dim3((unsigned)grid), dim3(WAVES * 64), 0, (hipStream_t)stream, ntensors, (const long*)desc, nblocks,
            (const float*)hyper, (const float*)qmaps, (const float*)coef);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

}  // extern "C"
