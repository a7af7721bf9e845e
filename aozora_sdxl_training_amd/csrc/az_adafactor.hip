// Adafactor (Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost", arXiv 1804.04235) with the arithmetic of
// transformers.optimization.Adafactor.step on LOGICAL tensor shapes (INTEGRATION.md "The Adafactor optimizer", tests/adafactor_ref.py):
// factored second moments for tensors of two or four dimensions, a full one for vectors, a per-tensor update clip.  One optimizer step
// is FIVE launches whatever the number of tensors; the work is dealt from a descriptor table with one row per trainable tensor:
//   1. row sums -> row EMA, column partial sums per row stripe, sum p^2 (matrices); the whole state update and sum u^2 (vectors, batches)
//   2. column partials added in stripe order -> column EMA and its rsqrt; the row mean per matrix -> the row factors
//   3. sum u^2 per row stripe (matrices)
//   4. per tensor: RMS(u), RMS(p) -> the clip denominator, lr_t, weight_decay * lr_t
//   5. the update itself: one rounding to bf16, to nearest or stochastic
// No floating-point atomics, every sum has a fixed order; the per-tensor sums are fp64 (per thread, per block, then one wave per tensor).
// Nothing is read back by the host.
#include "az_common.h"
#include "aozora_hip.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int SH = 128;            // rows of a matrix stripe (one workgroup of passes 1, 3, 5)
constexpr int VEC_ITEM = 1024;     // elements of a vector per workgroup
constexpr int BATCH_ITEM = 256;    // little matrices of a batch per workgroup: one per thread
constexpr int COL_ITEM = 256;      // columns per workgroup of pass 2

enum { CLS_VEC = 0, CLS_MAT = 1, CLS_BATCH = 2 };
enum { F_WIDE = 1 };               // 16-byte accesses: p, g 16-byte aligned, contiguous columns, row stride and C multiples of 8
// one descriptor row: int64 words
enum { W_CLS, W_FLAGS, W_P, W_G, W_NB0, W_NB1, W_SB0, W_SB1, W_R, W_SR, W_C, W_SC, W_STROW, W_STCOL, W_STM, W_FIRST, W_NWG, W_FIRST2, W_N2,
       W_SCR, W_FAC, W_SR0, W_NUMEL, W_SPARE, W_WORDS };
// hyper (HOST fp64[16])
enum { H_B2T, H_LR, H_EPS1, H_EPS2, H_CLIP, H_B1, H_WD, H_SCALE, H_SR, H_SEED, H_STEP, H_DOMAIN, H_WORDS = 16 };

struct AfK {
  double lr, wd, eps2;
  float b2, omb2, eps1, clip, b1, omb1;
  int scale, has_m, has_wd, sr;
  uint32_t k0, k1, step, dom;
};

// the row t with first[t] <= wg < first[t + 1] (word `w` of the rows is non-decreasing; rows with no work repeat their neighbour's)
__device__ __forceinline__ int find_row(const long* __restrict__ desc, int nt, int w, long wg) {
  int lo = 0, hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[(long)mid * W_WORDS + w] <= wg) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
  return x;
}
// block sum of two doubles in a fixed order (lanes by xor-shuffle, then the waves in index order); valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double* sh) {
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sh[0]; b = sh[1];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) { a = a + sh[2 * q]; b = b + sh[2 * q + 1]; }
  }
}

template <int NC> __device__ __forceinline__ void load_bf(const bf16_t* __restrict__ q, float* x) {
  if constexpr (NC == 8) {
    const uint4 u = *reinterpret_cast<const uint4*>(q);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = __uint_as_float(w[e] << 16); x[2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u); }
  } else {
    x[0] = bf2f(q[0]);
  }
}
template <int NC> __device__ __forceinline__ void load_f(const float* __restrict__ q, float* x) {
  if constexpr (NC == 8) {
    const float4 a = reinterpret_cast<const float4*>(q)[0], b = reinterpret_cast<const float4*>(q)[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else {
    x[0] = q[0];
  }
}
template <int NC> __device__ __forceinline__ void store_f(float* __restrict__ q, const float* x) {
  if constexpr (NC == 8) {
    reinterpret_cast<float4*>(q)[0] = make_float4(x[0], x[1], x[2], x[3]);
    reinterpret_cast<float4*>(q)[1] = make_float4(x[4], x[5], x[6], x[7]);
  } else {
    q[0] = x[0];
  }
}

// fp32 -> bf16 bits, the magnitude rounded up with probability (low half) / 65536 (the convention of az_optim.hip sr_round)
__device__ __forceinline__ bf16_t sr_round(float pp, uint32_t r) {
  const uint32_t u = __float_as_uint(pp);
  if ((u & 0x7F800000u) == 0x7F800000u) return f2bf(pp);
  uint32_t o = (u + r) >> 16;
  if ((o & 0x7F80u) == 0x7F80u) o = u >> 16;
  return (bf16_t)o;
}
__device__ __forceinline__ void sr_group(const AfK& k, long group, uint32_t* w) {
  philox4x32_10((uint32_t)group, (uint32_t)((unsigned long)group >> 32), k.step, k.dom, k.k0, k.k1, w);
}
// the bf16 image of x for the element at flat offset e
__device__ __forceinline__ bf16_t round_one(const AfK& k, float x, long e) {
  if (!k.sr) return f2bf(x);
  uint32_t w[4];
  sr_group(k, e >> 3, w);
  return sr_round(x, sr_lane_bits(w, (int)(e & 7)));
}

struct Tsc { float d, lr, wdlr; };      // per tensor: clip denominator, lr_t, weight_decay * lr_t (tsc[4 t ..])

// one element of pass 5: raw update u, parameter p, first moment m (read and written when has_m) -> the fp32 parameter
__device__ __forceinline__ float apply_math(const AfK& k, const Tsc& s, float u, float p, float& m) {
#pragma clang fp contract(off)
  u = u / s.d;
  u = s.lr * u;
  if (k.has_m) { m = m * k.b1 + k.omb1 * u; u = m; }
  if (k.has_wd) p = p - s.wdlr * p;
  return p - u;
}

// u of a little K x K matrix from its row and column moments
template <int K> __device__ __forceinline__ void batch_u(const float* row, const float* col, const float (*g)[K], float (*u)[K]) {
#pragma clang fp contract(off)
  float s = row[0];
#pragma unroll
  for (int r = 1; r < K; ++r) s = s + row[r];
  const float mean = s / (float)K;
  float rf[K], cf[K];
#pragma unroll
  for (int r = 0; r < K; ++r) { rf[r] = 1.0f / sqrtf(row[r] / mean); cf[r] = 1.0f / sqrtf(col[r]); }
#pragma unroll
  for (int r = 0; r < K; ++r)
#pragma unroll
    for (int c = 0; c < K; ++c) u[r][c] = (rf[r] * cf[c]) * g[r][c];
}

struct Row {
  int cls, wide;
  bf16_t* p; const bf16_t* g;
  long nb0, nb1, sb0, sb1, R, sr, C, sc, strow, stcol, stm, first, nwg, scr, fac, sr0, numel;
};
__device__ __forceinline__ Row read_row(const long* __restrict__ d) {
  Row r;
  r.cls = (int)d[W_CLS]; r.wide = (int)(d[W_FLAGS] & F_WIDE);
  r.p = (bf16_t*)d[W_P]; r.g = (const bf16_t*)d[W_G];
  r.nb0 = d[W_NB0]; r.nb1 = d[W_NB1]; r.sb0 = d[W_SB0]; r.sb1 = d[W_SB1]; r.R = d[W_R]; r.sr = d[W_SR]; r.C = d[W_C]; r.sc = d[W_SC];
  r.strow = d[W_STROW]; r.stcol = d[W_STCOL]; r.stm = d[W_STM]; r.first = d[W_FIRST]; r.nwg = d[W_NWG]; r.scr = d[W_SCR]; r.fac = d[W_FAC];
  r.sr0 = d[W_SR0]; r.numel = d[W_NUMEL];
  return r;
}

// ---- pass 1 ---------------------------------------------------------------------------------------------------------------------
// a stripe of a matrix: thread t owns NC neighbouring columns of each chunk of BLOCK * NC, walks the stripe's rows in order with the
// column sums in registers, and the row sums grow in LDS, one cell per (row, wave), chunk after chunk
template <int NC>
__device__ __forceinline__ void mat_pass1(const Row& t, long stripe, const AfK& k, float* __restrict__ state, float* __restrict__ scratch,
                                          float* rowacc, double& p2) {
#pragma clang fp contract(off)
  const long r0 = stripe * SH, r1 = r0 + SH < t.R ? r0 + SH : t.R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < SH * WAVES; i += BLOCK) rowacc[i] = 0.0f;
  __syncthreads();
  for (long cb = 0; cb < t.C; cb += (long)BLOCK * NC) {
    const long c = cb + (long)threadIdx.x * NC;
    const bool active = c < t.C;
    float cs[NC];
#pragma unroll
    for (int e = 0; e < NC; ++e) cs[e] = 0.0f;
    for (long r = r0; r < r1; ++r) {
      float part = 0.0f;
      if (active) {
        float g[NC];
        load_bf<NC>(t.g + r * t.sr + c, g);
#pragma unroll
        for (int e = 0; e < NC; ++e) { const float upd = g[e] * g[e] + k.eps1; cs[e] = cs[e] + upd; part = part + upd; }
        if (k.scale) {
          float p[NC];
          load_bf<NC>(t.p + r * t.sr + c, p);
#pragma unroll
          for (int e = 0; e < NC; ++e) p2 = p2 + (double)p[e] * (double)p[e];
        }
      }
      part = wave_sum(part);
      if (lane == 0) rowacc[(r - r0) * WAVES + wave] = rowacc[(r - r0) * WAVES + wave] + part;
    }
    if (active) store_f<NC>(scratch + t.scr + stripe * t.C + c, cs);
  }
  __syncthreads();
  for (long i = threadIdx.x; i < r1 - r0; i += BLOCK) {
    float s = rowacc[i * WAVES];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = s + rowacc[i * WAVES + w];
    const float mean = s / (float)t.C;
    float* q = state + t.strow + r0 + i;
    *q = *q * k.b2 + k.omb2 * mean;
  }
}

template <int K>
__device__ __forceinline__ void batch_pass1(const Row& t, long local, const AfK& k, float* __restrict__ state, double& u2, double& p2) {
#pragma clang fp contract(off)
  const long q = local * BATCH_ITEM + threadIdx.x;
  if (q >= t.nb0 * t.nb1) return;
  const long o = q / t.nb1, i = q - o * t.nb1, base = o * t.sb0 + i * t.sb1;
  float g[K][K], upd[K][K], row[K], col[K], u[K][K];
#pragma unroll
  for (int r = 0; r < K; ++r)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      g[r][c] = bf2f(t.g[base + r * t.sr + c * t.sc]);
      upd[r][c] = g[r][c] * g[r][c] + k.eps1;
      if (k.scale) { const float p = bf2f(t.p[base + r * t.sr + c * t.sc]); p2 = p2 + (double)p * (double)p; }
    }
#pragma unroll
  for (int r = 0; r < K; ++r) {
    float s = upd[r][0], v = upd[0][r];
#pragma unroll
    for (int c = 1; c < K; ++c) { s = s + upd[r][c]; v = v + upd[c][r]; }
    float* qr = state + t.strow + q * K + r;
    float* qc = state + t.stcol + q * K + r;
    row[r] = *qr * k.b2 + k.omb2 * (s / (float)K);
    col[r] = *qc * k.b2 + k.omb2 * (v / (float)K);
    *qr = row[r]; *qc = col[r];
  }
  batch_u<K>(row, col, g, u);
#pragma unroll
  for (int r = 0; r < K; ++r)
#pragma unroll
    for (int c = 0; c < K; ++c) u2 = u2 + (double)u[r][c] * (double)u[r][c];
}

__global__ void __launch_bounds__(BLOCK) af_pass1_kernel(const long* __restrict__ desc, int nt, float* __restrict__ state,
                                                          float* __restrict__ scratch, double* __restrict__ partials, AfK k) {
#pragma clang fp contract(off)
  __shared__ float rowacc[SH * WAVES];
  __shared__ double sh[2 * WAVES];
  const long wg = blockIdx.x;
  const Row t = read_row(desc + (long)find_row(desc, nt, W_FIRST, wg) * W_WORDS);
  const long local = wg - t.first;
  double u2 = 0.0, p2 = 0.0;
  if (t.cls == CLS_MAT) {
    if (t.wide) mat_pass1<8>(t, local, k, state, scratch, rowacc, p2); else mat_pass1<1>(t, local, k, state, scratch, rowacc, p2);
  } else if (t.cls == CLS_VEC) {
    for (int j = 0; j < VEC_ITEM / BLOCK; ++j) {
      const long i = local * VEC_ITEM + j * BLOCK + threadIdx.x;
      if (i < t.C) {
        const float g = bf2f(t.g[i]);
        float* q = state + t.strow + i;
        const float v = *q * k.b2 + k.omb2 * (g * g + k.eps1);
        *q = v;
        const float u = (1.0f / sqrtf(v)) * g;
        u2 = u2 + (double)u * (double)u;
        if (k.scale) { const float p = bf2f(t.p[i]); p2 = p2 + (double)p * (double)p; }
      }
    }
  } else {
    if (t.R == 1) batch_pass1<1>(t, local, k, state, u2, p2); else batch_pass1<3>(t, local, k, state, u2, p2);
  }
  block_sum2(u2, p2, sh);
  if (threadIdx.x == 0) { partials[2 * wg] = u2; partials[2 * wg + 1] = p2; }
}

// ---- pass 2 (matrices only) -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) af_pass2_kernel(const long* __restrict__ desc, int nmat, float* __restrict__ state,
                                                          const float* __restrict__ scratch, float* __restrict__ fac, AfK k) {
#pragma clang fp contract(off)
  __shared__ double sd[BLOCK];
  const long wg = blockIdx.x;
  const long* d = desc + (long)find_row(desc, nmat, W_FIRST2, wg) * W_WORDS;
  const Row t = read_row(d);
  const long local = wg - d[W_FIRST2];
  if (local < d[W_N2] - 1) {                  // a chunk of columns: the stripes in stripe order
    const long c = local * COL_ITEM + threadIdx.x;
    if (c >= t.C) return;
    float s = scratch[t.scr + c];
    for (long st = 1; st < t.nwg; ++st) s = s + scratch[t.scr + st * t.C + c];
    float* q = state + t.stcol + c;
    const float v = *q * k.b2 + k.omb2 * (s / (float)t.R);
    *q = v;
    fac[t.fac + c] = 1.0f / sqrtf(v);
    return;
  }
  double a = 0.0;                            // the row mean, then the row factors
  for (long r = threadIdx.x; r < t.R; r += BLOCK) a = a + (double)state[t.strow + r];
  sd[threadIdx.x] = a;
  __syncthreads();
  for (int o = BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sd[threadIdx.x] = sd[threadIdx.x] + sd[threadIdx.x + o];
    __syncthreads();
  }
  const float mean = (float)(sd[0] / (double)t.R);
  for (long r = threadIdx.x; r < t.R; r += BLOCK) fac[t.fac + t.C + r] = 1.0f / sqrtf(state[t.strow + r] / mean);
}

// ---- pass 3 (matrices only): sum u^2 per stripe -----------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void mat_pass3(const Row& t, long stripe, const float* __restrict__ fac, double& u2) {
#pragma clang fp contract(off)
  const long r0 = stripe * SH, r1 = r0 + SH < t.R ? r0 + SH : t.R;
  for (long cb = 0; cb < t.C; cb += (long)BLOCK * NC) {
    const long c = cb + (long)threadIdx.x * NC;
    if (c >= t.C) break;
    float cf[NC];
    load_f<NC>(fac + t.fac + c, cf);
    for (long r = r0; r < r1; ++r) {
      const float rf = fac[t.fac + t.C + r];
      float g[NC];
      load_bf<NC>(t.g + r * t.sr + c, g);
#pragma unroll
      for (int e = 0; e < NC; ++e) { const float u = (rf * cf[e]) * g[e]; u2 = u2 + (double)u * (double)u; }
    }
  }
}

__global__ void __launch_bounds__(BLOCK) af_pass3_kernel(const long* __restrict__ desc, int nmat, const float* __restrict__ fac,
                                                          double* __restrict__ partials) {
  __shared__ double sh[2 * WAVES];
  const long wg = blockIdx.x;
  const Row t = read_row(desc + (long)find_row(desc, nmat, W_FIRST, wg) * W_WORDS);
  double u2 = 0.0, none = 0.0;
  if (t.wide) mat_pass3<8>(t, wg - t.first, fac, u2); else mat_pass3<1>(t, wg - t.first, fac, u2);
  block_sum2(u2, none, sh);
  if (threadIdx.x == 0) partials[2 * wg] = u2;
}

// ---- pass 4: one wave per tensor ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) af_pass4_kernel(const long* __restrict__ desc, const double* __restrict__ partials,
                                                       float* __restrict__ tsc, AfK k) {
#pragma clang fp contract(off)
  const long* d = desc + (long)blockIdx.x * W_WORDS;
  const long first = d[W_FIRST], nwg = d[W_NWG], n = d[W_NUMEL];
  double a = 0.0, b = 0.0;
  for (long i = threadIdx.x; i < nwg; i += 64) { a = a + partials[2 * (first + i)]; b = b + partials[2 * (first + i) + 1]; }
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  if (threadIdx.x != 0) return;
  const float rms_u = (float)sqrt(a / (double)n);
  const float den = fmaxf(1.0f, rms_u / k.clip);
  double lr = k.lr;
  if (k.scale) {
    const float rms_p = (float)sqrt(b / (double)n);
    lr = fmax(k.eps2, (double)rms_p) * lr;
  }
  float* o = tsc + 4 * (long)blockIdx.x;
  o[0] = den; o[1] = (float)lr; o[2] = (float)(k.wd * lr); o[3] = rms_u;
}

// ---- pass 5 ------------------------------------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void mat_pass5(const Row& t, long stripe, const AfK& k, const Tsc& s, float* __restrict__ state,
                                          const float* __restrict__ fac) {
#pragma clang fp contract(off)
  const long r0 = stripe * SH, r1 = r0 + SH < t.R ? r0 + SH : t.R;
  for (long cb = 0; cb < t.C; cb += (long)BLOCK * NC) {
    const long c = cb + (long)threadIdx.x * NC;
    if (c >= t.C) break;
    float cf[NC];
    load_f<NC>(fac + t.fac + c, cf);
    for (long r = r0; r < r1; ++r) {
      const float rf = fac[t.fac + t.C + r];
      const long off = r * t.sr + c;
      float g[NC], p[NC], m[NC];
      load_bf<NC>(t.g + off, g);
      load_bf<NC>(t.p + off, p);
      float* qm = state + t.stm + r * t.C + c;
      if (k.has_m) load_f<NC>(qm, m);
#pragma unroll
      for (int e = 0; e < NC; ++e) { if (!k.has_m) m[e] = 0.0f; p[e] = apply_math(k, s, (rf * cf[e]) * g[e], p[e], m[e]); }
      if (k.has_m) store_f<NC>(qm, m);
      if constexpr (NC == 8) {
        uint32_t o[4];
        if (k.sr) {
          uint32_t w[4];
          sr_group(k, (t.sr0 + off) >> 3, w);        // (sr0 + off) % 8 == 0 on the wide path
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (uint32_t)sr_round(p[2 * e], w[e] & 0xFFFFu) | ((uint32_t)sr_round(p[2 * e + 1], w[e] >> 16) << 16);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = pack2bf(p[2 * e], p[2 * e + 1]);
        }
        *reinterpret_cast<uint4*>(t.p + off) = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
        t.p[off] = round_one(k, p[0], t.sr0 + off);
      }
    }
  }
}

template <int K>
__device__ __forceinline__ void batch_pass5(const Row& t, long local, const AfK& k, const Tsc& s, float* __restrict__ state) {
#pragma clang fp contract(off)
  const long q = local * BATCH_ITEM + threadIdx.x;
  if (q >= t.nb0 * t.nb1) return;
  const long o = q / t.nb1, i = q - o * t.nb1, base = o * t.sb0 + i * t.sb1;
  float g[K][K], row[K], col[K], u[K][K];
#pragma unroll
  for (int r = 0; r < K; ++r) {
    row[r] = state[t.strow + q * K + r]; col[r] = state[t.stcol + q * K + r];
#pragma unroll
    for (int c = 0; c < K; ++c) g[r][c] = bf2f(t.g[base + r * t.sr + c * t.sc]);
  }
  batch_u<K>(row, col, g, u);
#pragma unroll
  for (int r = 0; r < K; ++r)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const long off = base + r * t.sr + c * t.sc;
      float* qm = state + t.stm + q * (K * K) + r * K + c;
      float m = k.has_m ? *qm : 0.0f;
      const float x = apply_math(k, s, u[r][c], bf2f(t.p[off]), m);
      if (k.has_m) *qm = m;
      t.p[off] = round_one(k, x, t.sr0 + off);
    }
}

__global__ void __launch_bounds__(BLOCK) af_pass5_kernel(const long* __restrict__ desc, int nt, float* __restrict__ state,
                                                          const float* __restrict__ fac, const float* __restrict__ tsc, AfK k) {
#pragma clang fp contract(off)
  const long wg = blockIdx.x;
  const int ti = find_row(desc, nt, W_FIRST, wg);
  const Row t = read_row(desc + (long)ti * W_WORDS);
  const long local = wg - t.first;
  const Tsc s = {tsc[4 * (long)ti], tsc[4 * (long)ti + 1], tsc[4 * (long)ti + 2]};
  if (t.cls == CLS_MAT) {
    if (t.wide) mat_pass5<8>(t, local, k, s, state, fac); else mat_pass5<1>(t, local, k, s, state, fac);
  } else if (t.cls == CLS_VEC) {
    for (int j = 0; j < VEC_ITEM / BLOCK; ++j) {
      const long i = local * VEC_ITEM + j * BLOCK + threadIdx.x;
      if (i < t.C) {
        const float g = bf2f(t.g[i]);
        const float u = (1.0f / sqrtf(state[t.strow + i])) * g;
        float* qm = state + t.stm + i;
        float m = k.has_m ? *qm : 0.0f;
        const float x = apply_math(k, s, u, bf2f(t.p[i]), m);
        if (k.has_m) *qm = m;
        t.p[i] = round_one(k, x, t.sr0 + i);
      }
    }
  } else {
    if (t.R == 1) batch_pass5<1>(t, local, k, s, state); else batch_pass5<3>(t, local, k, s, state);
  }
}

inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// The whole table, on the host, before anything is launched: classes, alignment, the work-item numbering and every offset against
// the sizes of the buffers it points into.  -> 0, or the argument error.
int check_table(int nt, const long* desc, long state_numel, long scratch_numel, long fac_numel, bool has_m, long* nwg_all, long* nwg_mat,
                long* n2_all, int* nmat) {
  long first = 0, first2 = 0;
  bool mats_over = false;
  *nmat = 0;
  for (int ti = 0; ti < nt; ++ti) {
    const long* d = desc + (long)ti * W_WORDS;
    const long cls = d[W_CLS], R = d[W_R], C = d[W_C], nb0 = d[W_NB0], nb1 = d[W_NB1];
    if (cls != CLS_VEC && cls != CLS_MAT && cls != CLS_BATCH) return AZ_ERR_ARG(112);
    if (!d[W_P] || !d[W_G] || (d[W_P] & 1) || (d[W_G] & 1)) return AZ_ERR_ARG(113);
    if (R < 1 || C < 1 || nb0 < 1 || nb1 < 1 || d[W_SB0] < 0 || d[W_SB1] < 0 || d[W_SR] < 0 || d[W_SC] < 0 || d[W_SR0] < 0) return AZ_ERR_ARG(114);
    if (d[W_STROW] < 0 || d[W_STCOL] < 0 || (has_m && d[W_STM] < 0) || d[W_SCR] < 0 || d[W_FAC] < 0) return AZ_ERR_ARG(114);
    if (d[W_FLAGS] & ~(long)F_WIDE) return AZ_ERR_ARG(112);
    long nwg, n2 = 0, numel;
    if (cls == CLS_MAT) {
      if (mats_over || nb0 != 1 || nb1 != 1 || d[W_SC] != 1 || d[W_SR] < C) return AZ_ERR_ARG(115);
      nwg = cdiv(R, SH); n2 = cdiv(C, COL_ITEM) + 1; numel = R * C;
      if (d[W_STROW] + R > state_numel || d[W_STCOL] + C > state_numel || d[W_SCR] + nwg * C > scratch_numel || d[W_FAC] + R + C > fac_numel)
        return AZ_ERR_ARG(116);
      if (d[W_FLAGS] & F_WIDE)
        if ((d[W_P] & 15) || (d[W_G] & 15) || (C & 7) || (d[W_SR] & 7) || (d[W_SR0] & 7) || (d[W_SCR] & 3) || (d[W_FAC] & 3) || (has_m && (d[W_STM] & 3)))
          return AZ_ERR_ARG(117);
      ++*nmat;
    } else if (cls == CLS_VEC) {
      mats_over = true;
      if (R != 1 || nb0 != 1 || nb1 != 1) return AZ_ERR_ARG(115);
      nwg = cdiv(C, VEC_ITEM); numel = C;
      if (d[W_STROW] + C > state_numel || d[W_FLAGS]) return AZ_ERR_ARG(116);
    } else {
      mats_over = true;
      if (R != C || (R != 1 && R != 3) || d[W_FLAGS]) return AZ_ERR_ARG(115);
      nwg = cdiv(nb0 * nb1, BATCH_ITEM); numel = nb0 * nb1 * R * C;
      if (d[W_STROW] + nb0 * nb1 * R > state_numel || d[W_STCOL] + nb0 * nb1 * C > state_numel) return AZ_ERR_ARG(116);
    }
    if (has_m && d[W_STM] + numel > state_numel) return AZ_ERR_ARG(116);
    if (d[W_FIRST] != first || d[W_NWG] != nwg || d[W_FIRST2] != first2 || d[W_N2] != n2 || d[W_NUMEL] != numel) return AZ_ERR_ARG(118);
    first += nwg; first2 += n2;
    if (cls == CLS_MAT) *nwg_mat = first;
  }
  *nwg_all = first; *n2_all = first2;
  if (first > 0x7FFFFFFFl || first2 > 0x7FFFFFFFl) return AZ_ERR_ARG(119);
  return AZ_OK;
}

}  // namespace

extern "C" {

long az_adafactor_geometry(int what) {
  switch (what) {
    case 0: return W_WORDS;
    case 1: return SH;
    case 2: return VEC_ITEM;
    case 3: return BATCH_ITEM;
    case 4: return COL_ITEM;
    case 5: return BLOCK * 8;      // columns of a chunk on the 16-byte path
    default: return AZ_ERR_ARG(110);
  }
}

int az_adafactor_step(int ntensors, const void* desc_host, const void* desc, void* state, long state_numel, void* scratch, long scratch_numel,
                      void* fac, long fac_numel, void* partials, void* tsc, const void* hyper_host, void* stream) {
  if (ntensors < 0 || state_numel < 0 || scratch_numel < 0 || fac_numel < 0) return AZ_ERR_ARG(111);
  if (!hyper_host || ((uintptr_t)hyper_host & 7)) return AZ_ERR_ARG(111);
  if (ntensors == 0) return AZ_OK;
  if (!desc_host || !desc || !state || !scratch || !fac || !partials || !tsc) return AZ_ERR_ARG(111);
  if (((uintptr_t)desc_host & 7) || ((uintptr_t)desc & 7) || ((uintptr_t)state & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)fac & 15) ||
      ((uintptr_t)partials & 7) || ((uintptr_t)tsc & 3))
    return AZ_ERR_ARG(111);
  const double* h = (const double*)hyper_host;
  AfK k;
  k.lr = h[H_LR]; k.wd = h[H_WD];
  k.b2 = (float)h[H_B2T]; k.omb2 = (float)(1.0 - h[H_B2T]); k.eps1 = (float)h[H_EPS1]; k.eps2 = h[H_EPS2]; k.clip = (float)h[H_CLIP];
  k.has_m = h[H_B1] >= 0.0; k.b1 = k.has_m ? (float)h[H_B1] : 0.0f; k.omb1 = k.has_m ? (float)(1.0 - h[H_B1]) : 0.0f;
  k.scale = h[H_SCALE] != 0.0; k.has_wd = h[H_WD] != 0.0; k.sr = h[H_SR] != 0.0;
  if (!(h[H_CLIP] > 0.0) || !(h[H_B1] < 1.0) || h[H_SEED] < 0.0 || h[H_STEP] < 1.0) return AZ_ERR_ARG(111);
  const unsigned long seed = (unsigned long)h[H_SEED];
  k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32); k.step = (uint32_t)(unsigned long)h[H_STEP]; k.dom = (uint32_t)(unsigned long)h[H_DOMAIN];
  long nwg = 0, nwg_mat = 0, n2 = 0;
  int nmat = 0;
  const int rc = check_table(ntensors, (const long*)desc_host, state_numel, scratch_numel, fac_numel, k.has_m, &nwg, &nwg_mat, &n2, &nmat);
  if (rc != AZ_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long* d = (const long*)desc;
  az_launch(af_pass1_kernel, dim3((unsigned)nwg), dim3(BLOCK), 0, st, d, ntensors, (float*)state, (float*)scratch, (double*)partials, k);
  AZ_CHECK_LAUNCH();
  if (nmat > 0) {
    az_launch(af_pass2_kernel, dim3((unsigned)n2), dim3(BLOCK), 0, st, d, nmat, (float*)state, (const float*)scratch, (float*)fac, k);
    AZ_CHECK_LAUNCH();
    az_launch(af_pass3_kernel, dim3((unsigned)nwg_mat), dim3(BLOCK), 0, st, d, nmat, (const float*)fac, (double*)partials);
    AZ_CHECK_LAUNCH();
  }
  az_launch(af_pass4_kernel, dim3((unsigned)ntensors), dim3(64), 0, st, d, (const double*)partials, (float*)tsc, k);
  AZ_CHECK_LAUNCH();
  az_launch(af_pass5_kernel, dim3((unsigned)nwg), dim3(BLOCK), 0, st, d, ntensors, (float*)state, (const float*)fac, (const float*)tsc, k);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

}  // extern "C"
