// Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner", arXiv 2306.06101) over flat ranges
// with an fp32 master copy: the step size d is estimated on the device from two global sums per step, so a step is two passes over the
// state with a scalar state machine between them -- begin (1 thread), moments (one launch per range), finish (one workgroup), apply
// (one launch per range).  The host reads nothing back.  The arithmetic is the project's contract (INTEGRATION.md "The Prodigy
// optimizer", tests/prodigy_ref.py): fp32 per element, one rounding per operation, no contraction beyond the fused multiply-adds that
// are written; scalars and both sums in fp64; no floating-point atomics, every sum in a fixed order.
#include "az_common.h"
#include "aozora_hip.h"
#include <initializer_list>

namespace {

// dstate (device fp64[8]): the scalar state that persists between steps
enum { S_D, S_DMAX, S_DNUM, S_DDEN, S_DHAT, S_K, S_D0, S_WORDS = 8 };
// hyper (HOST fp64[16], read during az_prodigy_begin: the values travel in the kernel's arguments)
enum { H_LR, H_B1, H_B2, H_B3, H_EPS, H_WD, H_DCOEF, H_GROWTH, H_BIASCORR, H_SAFEGUARD, H_WORDS = 16 };
// consts (device, 128 bytes, 8-byte aligned): fp32[16] read by the two element passes, then fp64[8] carried from begin to finish
enum { C_CM, C_CV, C_CS, C_B1, C_B2, C_B3, C_DLR, C_WDDLR, C_EPSD, C_HASWD, C_SKIP, C_F32 = 16 };
enum { CD_DLR, CD_FACTOR, CD_B3, CD_DCOEF, CD_GROWTH, CD_WD, CD_EPS, CD_F64 = 8 };

struct HyperArgs { double v[H_WORDS]; };

#ifndef AZ_PRODIGY_BLOCKS_PER_CU
#define AZ_PRODIGY_BLOCKS_PER_CU 8       // one resident round at 8 waves per SIMD (both passes: 44 / 56 VGPRs)
#endif
constexpr int BLOCK = 256;
constexpr int GROUP = 8;                 // elements per 16-byte group of the bf16 operand (two 16-byte accesses of an fp32 one)

// How a pass walks a range of n elements: [0, head) scalar, then `groups` aligned groups of 8, then the scalar tail (az_optim.hip)
struct Split { long head, groups; };
struct Operand { const void* ptr; size_t esz; };
inline Split split_for(long n, std::initializer_list<Operand> ptrs) {
  long head = n;
  for (long h = 0; h < 8; ++h) {
    bool aligned = true;
    for (const Operand& o : ptrs) aligned = aligned && (((uintptr_t)o.ptr + o.esz * h) & 15) == 0;
    if (aligned) { head = h < n ? h : n; break; }
  }
  return Split{head, (n - head) >> 3};
}

// Blocks of a pass over n elements: one group of 8 per thread and iteration, at most 8 blocks per CU, a grid-stride loop for the
// rest.  A function of n (and the device) alone -- not of the alignment -- because the host sizes the partial sums with it.
int g_cus[64];
inline int cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (!g_cus[dev]) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
    g_cus[dev] = cus;
  }
  return g_cus[dev];
}
inline long grid_for(long n, int cus) {
  long g = (n + (long)BLOCK * GROUP - 1) / ((long)BLOCK * GROUP);
  const long cap = (long)cus * AZ_PRODIGY_BLOCKS_PER_CU;
  if (g > cap) g = cap;
  return g < 1 ? 1 : g;
}

__device__ __forceinline__ void load8f(const float* __restrict__ q, float* x) {
  const float4 a = reinterpret_cast<const float4*>(q)[0], b = reinterpret_cast<const float4*>(q)[1];
  x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
__device__ __forceinline__ void load8b(const bf16_t* __restrict__ q, float* x) {
  const uint4 u = reinterpret_cast<const uint4*>(q)[0];
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) { x[2 * e] = __uint_as_float(w[e] << 16); x[2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u); }
}
template <typename TG> __device__ __forceinline__ void load8g(const TG* __restrict__ q, float* x) {
  if constexpr (sizeof(TG) == 4) load8f(q, x); else load8b(q, x);
}
template <typename TG> __device__ __forceinline__ float ldg(const TG* __restrict__ q, long i) {
  if constexpr (sizeof(TG) == 4) return q[i]; else return bf2f(q[i]);
}
__device__ __forceinline__ void store8f(float* __restrict__ q, const float* x) {
  reinterpret_cast<float4*>(q)[0] = make_float4(x[0], x[1], x[2], x[3]);
  reinterpret_cast<float4*>(q)[1] = make_float4(x[4], x[5], x[6], x[7]);
}
__device__ __forceinline__ void store8b(bf16_t* __restrict__ q, const float* x) {
  reinterpret_cast<uint4*>(q)[0] = make_uint4(pack2bf(x[0], x[1]), pack2bf(x[2], x[3]), pack2bf(x[4], x[5]), pack2bf(x[6], x[7]));
}

struct MomK { float cm, cv, cs, b1, b2, b3, gc; };

// One element of the moments pass.  g: the gradient as read; w, p0: master and initial point; m, v, s in and out; the element's two
// terms are added to num / den in fp64.
template <typename TG>
__device__ __forceinline__ void moments_math(const MomK& k, float g, float w, float p0, float& m, float& v, float& s, double& num, double& den) {
#pragma clang fp contract(off)
  float gr = g * k.gc;
  if constexpr (sizeof(TG) == 2) gr = bf2f(f2bf(gr));      // = reading a gradient that was clipped in place (bf16 rounding)
  float t = m * k.b1; m = __builtin_fmaf(gr, k.cm, t);
  v = v * k.b2 + ((k.cv * gr) * gr);
  t = s * k.b3; s = __builtin_fmaf(gr, k.cs, t);
  const float diff = p0 - w;
  num = num + (double)gr * (double)diff;                    // the product of two fp32 values is exact in fp64
  den = den + (double)fabsf(s);
}

// Block sum of two doubles in a fixed order: xor-shuffles inside a wave, then the waves of the block in index order.
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
  return x;
}

template <typename TG>
__global__ void __launch_bounds__(BLOCK) prodigy_moments_kernel(long n, const float* __restrict__ w, const float* __restrict__ p0,
                                                                 const TG* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                                 float* __restrict__ s, const float* __restrict__ consts,
                                                                 const float* __restrict__ coef, double* __restrict__ partials, Split sp) {
#pragma clang fp contract(off)
  __shared__ double sh[2 * (BLOCK / 64)];
  const MomK k = {consts[C_CM], consts[C_CV], consts[C_CS], consts[C_B1], consts[C_B2], consts[C_B3], coef ? coef[0] : 1.0f};
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  const long body = sp.head + (sp.groups << 3);             // <= n (split_for)
  double num = 0.0, den = 0.0;
  for (long gi = tid; gi < sp.groups; gi += nthr) {
    const long i = sp.head + (gi << 3);
    float gg[8], ww[8], pp[8], mm[8], vv[8], ss[8];
    load8g<TG>(g + i, gg); load8f(w + i, ww); load8f(p0 + i, pp); load8f(m + i, mm); load8f(v + i, vv); load8f(s + i, ss);
#pragma unroll
    for (int e = 0; e < 8; ++e) moments_math<TG>(k, gg[e], ww[e], pp[e], mm[e], vv[e], ss[e], num, den);
    store8f(m + i, mm); store8f(v + i, vv); store8f(s + i, ss);
  }
  const long nscalar = n - (sp.groups << 3);                // head + tail
  for (long j = tid; j < nscalar; j += nthr) {
    const long i = j < sp.head ? j : j - sp.head + body;
    float mm = m[i], vv = v[i], ss = s[i];
    moments_math<TG>(k, ldg<TG>(g, i), w[i], p0[i], mm, vv, ss, num, den);
    m[i] = mm; v[i] = vv; s[i] = ss;
  }
  num = wave_sum_f64(num); den = wave_sum_f64(den);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[2 * wave] = num; sh[2 * wave + 1] = den; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sh[0], b = sh[1];
#pragma unroll
    for (int q = 1; q < BLOCK / 64; ++q) { a = a + sh[2 * q]; b = b + sh[2 * q + 1]; }
    partials[2 * (long)blockIdx.x] = a;
    partials[2 * (long)blockIdx.x + 1] = b;
  }
}

struct AppK { float dlr, wddlr, epsd; bool wd; };

__device__ __forceinline__ float apply_math(const AppK& k, float w, float m, float v) {
#pragma clang fp contract(off)
  if (k.wd) w = __builtin_fmaf(w, -k.wddlr, w);
  const float denom = sqrtf(v) + k.epsd;
  return w + ((-k.dlr * m) / denom);
}

__global__ void __launch_bounds__(BLOCK) prodigy_apply_kernel(long n, bf16_t* __restrict__ p, float* __restrict__ w, const float* __restrict__ m,
                                                               const float* __restrict__ v, const float* __restrict__ consts, Split sp) {
#pragma clang fp contract(off)
  if (consts[C_SKIP] != 0.0f) return;                       // d_denom == 0: the step ended in az_prodigy_finish
  const AppK k = {consts[C_DLR], consts[C_WDDLR], consts[C_EPSD], consts[C_HASWD] != 0.0f};
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  const long body = sp.head + (sp.groups << 3);
  for (long gi = tid; gi < sp.groups; gi += nthr) {
    const long i = sp.head + (gi << 3);
    float ww[8], mm[8], vv[8];
    load8f(w + i, ww); load8f(m + i, mm); load8f(v + i, vv);
#pragma unroll
    for (int e = 0; e < 8; ++e) ww[e] = apply_math(k, ww[e], mm[e], vv[e]);
    store8f(w + i, ww); store8b(p + i, ww);
  }
  const long nscalar = n - (sp.groups << 3);
  for (long j = tid; j < nscalar; j += nthr) {
    const long i = j < sp.head ? j : j - sp.head + body;
    const float x = apply_math(k, w[i], m[i], v[i]);
    w[i] = x; p[i] = f2bf(x);
  }
}

// The constants of the moments pass from the state before the step.  One lane, plain stores.
__global__ void prodigy_begin_kernel(const double* __restrict__ ds, HyperArgs h, float* __restrict__ cf, double* __restrict__ cd) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double d = ds[S_D], k = ds[S_K], d0 = ds[S_D0];
  const double lr = h.v[H_LR], b1 = h.v[H_B1], b2 = h.v[H_B2];
  double bc = 1.0;
  if (h.v[H_BIASCORR] != 0.0) bc = sqrt(1.0 - pow(b2, k + 1.0)) / (1.0 - pow(b1, k + 1.0));
  const double dlr = d * lr * bc;
  const double r = d / d0;
  cf[C_CM] = (float)(d * (1.0 - b1));
  cf[C_CV] = (float)(d * d * (1.0 - b2));
  cf[C_CS] = (float)(r * (h.v[H_SAFEGUARD] != 0.0 ? d : dlr));
  cf[C_B1] = (float)b1; cf[C_B2] = (float)b2; cf[C_B3] = (float)h.v[H_B3];
  cf[C_HASWD] = h.v[H_WD] != 0.0 ? 1.0f : 0.0f;
  cf[C_SKIP] = 1.0f;                                        // until az_prodigy_finish says otherwise
  cd[CD_DLR] = dlr; cd[CD_FACTOR] = r * dlr; cd[CD_B3] = h.v[H_B3]; cd[CD_DCOEF] = h.v[H_DCOEF]; cd[CD_GROWTH] = h.v[H_GROWTH];
  cd[CD_WD] = h.v[H_WD]; cd[CD_EPS] = h.v[H_EPS];
}

// Both sums over all partial pairs in a fixed order (thread t takes pairs t, t + 256, ...; then a tree over the threads), the step
// size update, the constants of the apply pass.  One workgroup; the results are written by thread 0 with plain stores.
__global__ void __launch_bounds__(BLOCK) prodigy_finish_kernel(long npairs, const double* __restrict__ partials, double* __restrict__ ds,
                                                                float* __restrict__ cf, const double* __restrict__ cd) {
#pragma clang fp contract(off)
  __shared__ double sa[BLOCK], sb[BLOCK];
  double a = 0.0, b = 0.0;
  for (long i = threadIdx.x; i < npairs; i += BLOCK) { a = a + partials[2 * i]; b = b + partials[2 * i + 1]; }
  sa[threadIdx.x] = a; sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { sa[threadIdx.x] = sa[threadIdx.x] + sa[threadIdx.x + o]; sb[threadIdx.x] = sb[threadIdx.x] + sb[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double d = ds[S_D], dmax = ds[S_DMAX];
  const double d0 = ds[S_D0], dlr = cd[CD_DLR];
  const double dnum = cd[CD_B3] * ds[S_DNUM] + cd[CD_FACTOR] * sa[0];
  const double dden = sb[0];
  ds[S_DNUM] = dnum;
  ds[S_DDEN] = dden;
  if (dden == 0.0) return;                                  // cf[C_SKIP] stays 1: no parameter update, k unchanged
  const double dhat = cd[CD_DCOEF] * dnum / dden;
  if (d == d0) d = dhat > d ? dhat : d;
  dmax = dhat > dmax ? dhat : dmax;
  const double grown = d * cd[CD_GROWTH];
  d = grown < dmax ? grown : dmax;
  ds[S_D] = d; ds[S_DMAX] = dmax; ds[S_DHAT] = dhat; ds[S_K] = ds[S_K] + 1.0;
  cf[C_DLR] = (float)dlr;                                   // the OLD d
  cf[C_WDDLR] = (float)(cd[CD_WD] * dlr);
  cf[C_EPSD] = (float)(d * cd[CD_EPS]);                     // the NEW d
  cf[C_SKIP] = 0.0f;
}

}  // namespace

extern "C" {

long az_prodigy_partials(long n) {
  if (n < 0) return AZ_ERR_ARG(95);
  if (n == 0) return 0;
  const int cus = cu_count();
  if (cus <= 0) return AZ_ERR_ARG(96);
  return grid_for(n, cus);
}

int az_prodigy_begin(const void* dstate, const void* hyper_host, void* consts, void* stream) {
  if (!dstate || !hyper_host || !consts || ((uintptr_t)dstate & 7) || ((uintptr_t)consts & 7) || ((uintptr_t)hyper_host & 7)) return AZ_ERR_ARG(91);
  HyperArgs h;
  for (int i = 0; i < H_WORDS; ++i) h.v[i] = ((const double*)hyper_host)[i];
  az_launch(prodigy_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)dstate, h, (float*)consts,
            (double*)((char*)consts + C_F32 * sizeof(float)));
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_prodigy_moments(long n, const void* w, const void* p0, const void* g, int gdtype, void* m, void* v, void* s, const void* consts,
                       const void* coef, void* partials, void* stream) {
  if (n < 0 || !w || !p0 || !g || !m || !v || !s || !consts || !partials || gdtype < 0 || gdtype > 1) return AZ_ERR_ARG(92);
  const uintptr_t gmask = gdtype == 0 ? 1 : 3;
  if (((uintptr_t)w & 3) || ((uintptr_t)p0 & 3) || ((uintptr_t)g & gmask) || ((uintptr_t)m & 3) || ((uintptr_t)v & 3) || ((uintptr_t)s & 3) ||
      ((uintptr_t)consts & 7) || ((uintptr_t)coef & 3) || ((uintptr_t)partials & 7))
    return AZ_ERR_ARG(93);
  if (n == 0) return AZ_OK;
  const int cus = cu_count();
  if (cus <= 0) return AZ_ERR_ARG(96);
  const Split sp = split_for(n, {{w, 4}, {p0, 4}, {g, gmask + 1}, {m, 4}, {v, 4}, {s, 4}});
  const dim3 grid((unsigned)grid_for(n, cus)), blk(BLOCK);
  hipStream_t st = (hipStream_t)stream;
  if (gdtype == 0)
    az_launch(prodigy_moments_kernel<bf16_t>, grid, blk, 0, st, n, (const float*)w, (const float*)p0, (const bf16_t*)g, (float*)m, (float*)v,
              (float*)s, (const float*)consts, (const float*)coef, (double*)partials, sp);
  else
    az_launch(prodigy_moments_kernel<float>, grid, blk, 0, st, n, (const float*)w, (const float*)p0, (const float*)g, (float*)m, (float*)v,
              (float*)s, (const float*)consts, (const float*)coef, (double*)partials, sp);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_prodigy_finish(long npartials, const void* partials, void* dstate, void* consts, void* stream) {
  if (npartials < 0 || !dstate || !consts || (npartials > 0 && !partials) || ((uintptr_t)partials & 7) || ((uintptr_t)dstate & 7) ||
      ((uintptr_t)consts & 7))
    return AZ_ERR_ARG(94);
  az_launch(prodigy_finish_kernel, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, npartials, (const double*)partials, (double*)dstate,
            (float*)consts, (const double*)((const char*)consts + C_F32 * sizeof(float)));
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_prodigy_apply(long n, void* p, void* w, const void* m, const void* v, const void* consts, void* stream) {
  if (n < 0 || !p || !w || !m || !v || !consts) return AZ_ERR_ARG(97);
  if (((uintptr_t)p & 1) || ((uintptr_t)w & 3) || ((uintptr_t)m & 3) || ((uintptr_t)v & 3) || ((uintptr_t)consts & 7)) return AZ_ERR_ARG(98);
  if (n == 0) return AZ_OK;
  const int cus = cu_count();
  if (cus <= 0) return AZ_ERR_ARG(96);
  const Split sp = split_for(n, {{p, 2}, {w, 4}, {m, 4}, {v, 4}});
  az_launch(prodigy_apply_kernel, dim3((unsigned)grid_for(n, cus)), dim3(BLOCK), 0, (hipStream_t)stream, n, (bf16_t*)p, (float*)w, (const float*)m,
            (const float*)v, (const float*)consts, sp);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

}  // extern "C"
