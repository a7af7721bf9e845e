// Optimizer-side kernels: global grad norm / clip (train.py:2771-2781, titan.py:162-184) and the
// Raven / Titan fused AdamW update (raven.py:96-147, titan.py:230-296) over a flat parameter range
// with first/second moments resident in PINNED HOST memory, streamed through the GPU by async copies.
#include "az_common.h"
#include "aozora_hip.h"
#include <initializer_list>
#include <map>
#include <mutex>
#include <type_traits>

namespace {

typedef _Float16 f16_t;   // momentum_dtype torch.float16 (raven.py:37-42): IEEE half, round-to-nearest-even, overflow -> inf

constexpr int SUMSQ_BLOCKS = 1024;

template <typename T> __device__ __forceinline__ float ldf(const T* p, long i);
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p, long i) { return bf2f(p[i]); }
template <> __device__ __forceinline__ float ldf<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float ldf<f16_t>(const f16_t* p, long i) { return (float)p[i]; }
// value of a moment as it is stored: the fp32 value rounded to the moment type
template <typename T> __device__ __forceinline__ T cvt_moment(float v);
// fp16 moments store the fp32 value rounded once more, as the reference's `.to(float16)` of an fp32 tensor does.  The empty asm hides
// where v came from: left alone the compiler folds the fused multiply-add behind exp_avg into v_fma_mixlo_f16, ONE rounding of the
// exact a * b + c to fp16 -- a different fp16 neighbour on 0.4 % of the elements (tests/test_elem_gpu.py, mdtype 2).
template <> __device__ __forceinline__ f16_t cvt_moment<f16_t>(float v) { asm volatile("" : "+v"(v)); return (f16_t)v; }
template <> __device__ __forceinline__ bf16_t cvt_moment<bf16_t>(float v) { return f2bf(v); }
template <> __device__ __forceinline__ float cvt_moment<float>(float v) { return v; }
template <typename T> __device__ __forceinline__ void stf(T* p, long i, float v) { p[i] = cvt_moment<T>(v); }

template <typename T>
__global__ void sumsq_partial_kernel(long n, const T* __restrict__ g, float* __restrict__ partial) {
  __shared__ float sh[16];
  float s = 0.f;
  if (sizeof(T) == 2) {
    const long n8 = n >> 3;
    const uint4* g8 = reinterpret_cast<const uint4*>(g);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
      uint4 u = g8[i];
      const uint32_t* w = reinterpret_cast<const uint32_t*>(&u);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = __uint_as_float(w[e] << 16), b = __uint_as_float(w[e] & 0xFFFF0000u);
        s += a * a + b * b;
      }
    }
    for (long i = (n8 << 3) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      float a = ldf<T>(g, i); s += a * a;
    }
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      float a = ldf<T>(g, i); s += a * a;
    }
  }
  float tot = block_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void sumsq_final_kernel(int nblk, const float* __restrict__ partial, float* out, int accumulate) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += blockDim.x) s += (double)partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.f) + (float)sh[0];
}

__global__ void clip_coef_kernel(const float* sumsq, float max_norm, float unscale, float* coef, float* norm) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float nrm = sqrtf(sumsq[0]) * unscale;
    norm[0] = nrm;
    float c = max_norm / (nrm + 1e-6f);
    coef[0] = (c < 1.0f ? c : 1.0f) * unscale;
  }
}

// ---- stochastic rounding of the bf16 parameter write (an option the reference does not have: INTEGRATION.md) -------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain integer arithmetic: counter-based, so
// the bits of an element are a function of (seed, optimizer step, domain, GLOBAL element index) and of nothing else -- not of how the
// flat range is cut into launches, chunks, regions or rank shards.
struct SrArgs {
  uint32_t k0, k1;     // key: seed low / high word
  uint32_t step, dom;  // counter words 2, 3
  long elem0;          // global index of the call's first element; counter words 0, 1 = (elem0 + i) >> 3
};
// How the wide kernels walk a range of n elements: [0, head) scalar, then `groups` aligned groups of 8 (16-byte accesses), then the
// scalar tail up to n (split_for)
struct Split { long head, groups; };

__device__ __forceinline__ void sr_group_bits(const SrArgs& sr, long group, uint32_t* w) {
  philox4x32_10((uint32_t)group, (uint32_t)((unsigned long)group >> 32), sr.step, sr.dom, sr.k0, sr.k1, w);
}

// fp32 -> bf16 bits, rounding the MAGNITUDE up with probability (low half) / 65536: r is uniform in [0, 65536).  Non-finite values and a
// carry into the all-ones exponent (a finite value never becomes inf) keep today's behaviour / truncate.
__device__ __forceinline__ bf16_t sr_round(float pp, uint32_t r) {
  const uint32_t u = __float_as_uint(pp);
  if ((u & 0x7F800000u) == 0x7F800000u) return f2bf(pp);
  uint32_t o = (u + r) >> 16;
  if ((o & 0x7F80u) == 0x7F80u) o = u >> 16;
  return (bf16_t)o;
}

struct AdamwK { float b1, b2, eps, wdf, step, sbc2, gc, omb1, omb2; };

__device__ __forceinline__ AdamwK adamw_consts(const float* __restrict__ hyper, const float* __restrict__ coef) {
  AdamwK k;
  k.b1 = hyper[1]; k.b2 = hyper[2]; k.eps = hyper[3]; k.wdf = hyper[4]; k.step = hyper[5]; k.sbc2 = hyper[6];
  k.gc = coef ? coef[0] : 1.0f;
  k.omb1 = 1.0f - k.b1; k.omb2 = 1.0f - k.b2;
  return k;
}

// One element of the update: reads its four inputs through the callables ldg / ldm / ldv / ldp (memory in the scalar form, registers
// in the 8-wide form -- read where the original kernel read them, so the scalar form compiles to the instruction stream it always had)
// and leaves the new fp32 values: mm, vv still to be rounded to the moment type, pp to bf16 (the ONE place where the forms differ).
template <typename TG, typename LG, typename LM, typename LV, typename LP>
__device__ __forceinline__ void adamw_math(const AdamwK& k, LG ldg, LM ldm, LV ldv, LP ldp, float& mm, float& vv, float& pp) {
  // The reference's operation order (raven.py:125-143, fp32 scratch tensors), rounding for rounding -- this TU's default
  // contraction would fuse differently and the update is host-link-bound, so the extra roundings cost nothing:
  //   exp_avg.mul_(b1).add_(g, alpha=1-b1)            ATen's add-with-alpha is a fused multiply-add (vec::fmadd)
  //   exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2)  self + ((value * g) * g), each product and the sum rounded
  //   p.mul_(wd_factor); denom = sqrt(v) / sqrt_bc2 + eps; p.addcdiv_(m, denom, value=-step_size)   self + ((value * m) / denom)
#pragma clang fp contract(off)
  float gr = ldg() * k.gc;
  if constexpr (sizeof(TG) == 2) gr = bf2f(f2bf(gr));   // = reading a gradient that was clipped in place (bf16 rounding)
  mm = ldm() * k.b1; mm = __builtin_fmaf(gr, k.omb1, mm);
  vv = ldv() * k.b2; vv = vv + ((k.omb2 * gr) * gr);
  pp = ldp() * k.wdf;
  const float denom = sqrtf(vv) / k.sbc2 + k.eps;
  pp = pp + ((-k.step * mm) / denom);
}

// Element i of the range through memory; the parameter operand is read by ldp() and written by stp(pp) (raven.py:144: bf16, round to
// nearest even, in the default kernel).
template <typename TM, typename TG, typename LP, typename SP>
__device__ __forceinline__ void adamw_elem(const AdamwK& k, long i, const TG* __restrict__ g, TM* __restrict__ m, TM* __restrict__ v, LP ldp,
                                           SP stp) {
  float mm, vv, pp;
  adamw_math<TG>(k, [&] { return ldf<TG>(g, i); }, [&] { return ldf<TM>(m, i); }, [&] { return ldf<TM>(v, i); }, ldp, mm, vv, pp);
  stp(pp);
  stf<TM>(m, i, mm);
  stf<TM>(v, i, vv);
}

// 8 consecutive elements <-> registers with 16-byte accesses (the pointer is 16-byte aligned: split_for)
template <typename T> __device__ __forceinline__ void load8(const T* __restrict__ q, float* x) {
  if constexpr (sizeof(T) == 4) {
    const float4 a = reinterpret_cast<const float4*>(q)[0], b = reinterpret_cast<const float4*>(q)[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else {
    const uint4 u = reinterpret_cast<const uint4*>(q)[0];
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (std::is_same<T, f16_t>::value) {
        x[2 * e] = (float)__builtin_bit_cast(f16_t, (uint16_t)(w[e] & 0xFFFFu));
        x[2 * e + 1] = (float)__builtin_bit_cast(f16_t, (uint16_t)(w[e] >> 16));
      } else {
        x[2 * e] = __uint_as_float(w[e] << 16);
        x[2 * e + 1] = __uint_as_float(w[e] & 0xFFFF0000u);
      }
    }
  }
}
template <typename T> __device__ __forceinline__ void store8_moment(T* __restrict__ q, const float* x) {
  if constexpr (sizeof(T) == 4) {
    reinterpret_cast<float4*>(q)[0] = make_float4(x[0], x[1], x[2], x[3]);
    reinterpret_cast<float4*>(q)[1] = make_float4(x[4], x[5], x[6], x[7]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      w[e] = (uint32_t)__builtin_bit_cast(uint16_t, cvt_moment<T>(x[2 * e])) | ((uint32_t)__builtin_bit_cast(uint16_t, cvt_moment<T>(x[2 * e + 1])) << 16);
    reinterpret_cast<uint4*>(q)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// hyper: [0] lr (unused here) [1] beta1 [2] beta2 [3] eps [4] wd_factor [5] step_size [6] sqrt_bc2
// (the grid-stride loops stay in the kernels themselves: blockDim / gridDim read from an inlined device function take the slow path)
template <typename TM, typename TG>
__global__ void adamw_kernel(long n, bf16_t* __restrict__ p, const TG* __restrict__ g, TM* __restrict__ m, TM* __restrict__ v,
                             const float* __restrict__ hyper, const float* __restrict__ coef) {
  const AdamwK k = adamw_consts(hyper, coef);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    adamw_elem<TM, TG>(k, i, g, m, v, [&] { return bf2f(p[i]); }, [&](float pp) { p[i] = f2bf(pp); });
}

// The parameter operand of the wide kernel is a policy P, passed by value: read 8 / read 1 / write 8 / write 1 at element i.
// SrParam (az_adamw_flat_sr): bf16 p written with stochastic rounding -- one Philox evaluation per aligned group of 8 ((elem0 + i) & 7
// == 0 there); a scalar element evaluates its group's word for itself.
struct SrParam {
  bf16_t* p;
  SrArgs sr;
  __device__ __forceinline__ void load8(long i, float* x) const { ::load8<bf16_t>(p + i, x); }
  __device__ __forceinline__ float load(long i) const { return bf2f(p[i]); }
  __device__ __forceinline__ void store8(long i, const float* x) const {
    uint32_t w[4], o[4];
    sr_group_bits(sr, (sr.elem0 + i) >> 3, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (uint32_t)sr_round(x[2 * e], w[e] & 0xFFFFu) | ((uint32_t)sr_round(x[2 * e + 1], w[e] >> 16) << 16);
    reinterpret_cast<uint4*>(p + i)[0] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  __device__ __forceinline__ void store(long i, float x) const {
    const long e = sr.elem0 + i;
    uint32_t w[4];
    sr_group_bits(sr, e >> 3, w);
    p[i] = sr_round(x, sr_lane_bits(w, (int)(e & 7)));
  }
};
// MasterParam (az_adamw_flat_master; INTEGRATION.md "fp32 master weights"): the fp32 master w is the operand; writes w = pp and p =
// bf16(pp), round to nearest even -- p is never read.
struct MasterParam {
  bf16_t* p;
  float* w;
  __device__ __forceinline__ void load8(long i, float* x) const { ::load8<float>(w + i, x); }
  __device__ __forceinline__ float load(long i) const { return w[i]; }
  __device__ __forceinline__ void store8(long i, const float* x) const { store8_moment<float>(w + i, x); store8_moment<bf16_t>(p + i, x); }
  __device__ __forceinline__ void store(long i, float x) const { w[i] = x; p[i] = f2bf(x); }
};

// The element update over the split s: one thread per aligned group of 8 (16-byte accesses), head and tail one element per thread.
template <typename TM, typename TG, typename P>
__global__ void adamw_wide_kernel(long n, P par, const TG* __restrict__ g, TM* __restrict__ m, TM* __restrict__ v,
                                  const float* __restrict__ hyper, const float* __restrict__ coef, Split s) {
  const AdamwK k = adamw_consts(hyper, coef);
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  const long body = s.head + (s.groups << 3);               // <= n (split_for)
  for (long gi = tid; gi < s.groups; gi += nthr) {
    const long i = s.head + (gi << 3);
    float gg[8], mm[8], vv[8], pp[8];
    load8<TG>(g + i, gg); load8<TM>(m + i, mm); load8<TM>(v + i, vv); par.load8(i, pp);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      adamw_math<TG>(k, [&] { return gg[e]; }, [&] { return mm[e]; }, [&] { return vv[e]; }, [&] { return pp[e]; }, mm[e], vv[e], pp[e]);
    par.store8(i, pp);
    store8_moment<TM>(m + i, mm);
    store8_moment<TM>(v + i, vv);
  }
  const long nscalar = n - (s.groups << 3);                  // head + tail
  for (long j = tid; j < nscalar; j += nthr) {
    const long i = j < s.head ? j : j - s.head + body;
    adamw_elem<TM, TG>(k, i, g, m, v, [&] { return par.load(i); }, [&](float pp) { par.store(i, pp); });
  }
}

// ---- parameter groups (an option the reference's trainer does not use: INTEGRATION.md "Parameter groups") -----------------------------
// az_adamw_flat_seg: wd_factor and step_size of an element come from ITS group; everything else (adamw_math included) is shared with
// the kernels above.  PlainParam: the bf16 parameter of adamw_kernel as a policy of the wide form, round to nearest even.
struct PlainParam {
  bf16_t* p;
  __device__ __forceinline__ void load8(long i, float* x) const { ::load8<bf16_t>(p + i, x); }
  __device__ __forceinline__ float load(long i) const { return bf2f(p[i]); }
  __device__ __forceinline__ void store8(long i, const float* x) const { store8_moment<bf16_t>(p + i, x); }
  __device__ __forceinline__ void store(long i, float x) const { p[i] = f2bf(x); }
};
// Global element e belongs to the first segment s with end[s] > e (ends ascending, exclusive); its group is gid[s], whose values are
// gh[2 * gid] = wd_factor, gh[2 * gid + 1] = step_size.  Every index is clamped: s to [0, nseg), gid to [0, ngroups) -- whatever the
// tables hold, nothing outside them is read (an element past the last end takes the last segment).
struct SegTab {
  const long* __restrict__ end;
  const int* __restrict__ gid;
  const float* __restrict__ gh;
  int nseg, ngroups;
  long elem0;        // global index of the call's first element
};
// first s in [lo, hi] with end[s] > e; hi when there is none.  0 <= lo <= hi < nseg: reads end[lo .. hi - 1] only
__device__ __forceinline__ int seg_find(const SegTab& t, long e, int lo, int hi) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (t.end[mid] > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// The same lookups with WAVE-UNIFORM operands, read through the constant address space: the tables are never written while a kernel
// runs, and saying so lets the compiler use scalar loads -- they run on the scalar unit and its own counter, beside the vector loads
// of the operands instead of in a queue behind them.
#define AZ_CONST_AS __attribute__((address_space(4)))
__device__ __forceinline__ long seg_end_u(const SegTab& t, int s) { return ((const AZ_CONST_AS long*)(uintptr_t)t.end)[s]; }
__device__ __forceinline__ int seg_find_u(const SegTab& t, long e, int lo, int hi) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (seg_end_u(t, mid) > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ void seg_enter_u(const SegTab& t, int s, AdamwK& k) {
  int g = ((const AZ_CONST_AS int*)(uintptr_t)t.gid)[s];
  g = g < 0 ? 0 : (g >= t.ngroups ? t.ngroups - 1 : g);
  const AZ_CONST_AS float* gh = (const AZ_CONST_AS float*)(uintptr_t)t.gh;
  k.wdf = gh[2 * g]; k.step = gh[2 * g + 1];
}
__device__ __forceinline__ long uniform64(long x) {            // x holds the same value in every lane: tell the compiler
  return (long)(((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long)x >> 32)) << 32) |
                (unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)x));
}
// the group values of segment s into k, and the first element that is no longer in s (the last segment never ends)
__device__ __forceinline__ long seg_enter(const SegTab& t, int s, AdamwK& k) {
  int g = t.gid[s];
  g = g < 0 ? 0 : (g >= t.ngroups ? t.ngroups - 1 : g);
  k.wdf = t.gh[2 * g]; k.step = t.gh[2 * g + 1];
  return s == t.nseg - 1 ? 0x7FFFFFFFFFFFFFFFL : t.end[s];
}

// The split of adamw_wide_kernel.  The 64 groups of a wave are consecutive, so the wave brackets the segments it touches with uniform
// operands (seg_find_u: scalar loads, under the operand loads already in flight): [lo, hi] is ONE segment almost always -- the table
// of an AozoraUNet has segments of >= 64 elements and a wave covers 512 -- and the wave then runs the wide kernel's loop body with
// that segment's two values.  Otherwise a lane searches the bracket only, and walks forward inside its 8 elements where a segment
// ends among them.
template <typename TM, typename TG, typename P>
__global__ void adamw_seg_kernel(long n, P par, const TG* __restrict__ g, TM* __restrict__ m, TM* __restrict__ v,
                                 const float* __restrict__ hyper, const float* __restrict__ coef, Split s, SegTab t) {
  const AdamwK k = adamw_consts(hyper, coef);
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  const long body = s.head + (s.groups << 3);               // <= n (split_for)
  const int last = t.nseg - 1;
  for (long gi = tid; gi < s.groups; gi += nthr) {
    const long i = s.head + (gi << 3), e0 = t.elem0 + i;
    float gg[8], mm[8], vv[8], pp[8];                         // issued first: the searches run under these loads
    load8<TG>(g + i, gg); load8<TM>(m + i, mm); load8<TM>(v + i, vv); par.load8(i, pp);
    const long gf = uniform64(gi - (long)(threadIdx.x & 63));  // the wave's first group (lane 0 is active whenever any lane is)
    const long gl = gf + 63 < s.groups ? gf + 63 : s.groups - 1;
    const long el = t.elem0 + s.head + (gl << 3) + 7;         // the wave's last element
    const int lo = seg_find_u(t, t.elem0 + s.head + (gf << 3), 0, last);
    const int hi = lo < last && seg_end_u(t, lo) <= el ? seg_find_u(t, el, lo + 1, last) : lo;
    AdamwK ke = k;
    if (lo == hi) {
      seg_enter_u(t, lo, ke);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        adamw_math<TG>(ke, [&] { return gg[e]; }, [&] { return mm[e]; }, [&] { return vv[e]; }, [&] { return pp[e]; }, mm[e], vv[e], pp[e]);
    } else {
      int sg = seg_find(t, e0, lo, hi);
      long end = seg_enter(t, sg, ke);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (e0 + e >= end) {                                  // (never for e == 0: end > e0 or sg is the last segment)
          while (sg < last && t.end[sg] <= e0 + e) ++sg;
          end = seg_enter(t, sg, ke);
        }
        adamw_math<TG>(ke, [&] { return gg[e]; }, [&] { return mm[e]; }, [&] { return vv[e]; }, [&] { return pp[e]; }, mm[e], vv[e], pp[e]);
      }
    }
    par.store8(i, pp);
    store8_moment<TM>(m + i, mm);
    store8_moment<TM>(v + i, vv);
  }
  const long nscalar = n - (s.groups << 3);                  // head + tail
  for (long j = tid; j < nscalar; j += nthr) {
    const long i = j < s.head ? j : j - s.head + body;
    AdamwK ke = k;
    seg_enter(t, seg_find(t, t.elem0 + i, 0, last), ke);
    adamw_elem<TM, TG>(ke, i, g, m, v, [&] { return par.load(i); }, [&](float pp) { par.store(i, pp); });
  }
}

template <typename TG>
__global__ void offload_kernel(long n, const TG* __restrict__ g, float* __restrict__ gh, int accumulate) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = ldf<TG>(g, i);
    gh[i] = accumulate ? gh[i] + v : v;
  }
}

// in-place clip of bf16 grads (torch.nn.utils.clip_grad_norm_ semantics: g = bf16(g * coef)); a
// coefficient of exactly 1 leaves the buffer untouched (no traffic).
__global__ void scale_bf16_kernel(long n, bf16_t* g, const float* coef) {
  const float c = coef[0];
  if (c == 1.0f) return;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) g[i] = f2bf(bf2f(g[i]) * c);
}

__global__ void scale_f32_kernel(long n, float* x, const float* coef) {
  const float c = coef[0];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] *= c;
}

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

// The split of a range over the operands `ptrs`: head = the first h in [0, 8) at which every pointer is 16-byte aligned -- with
// forced >= 0 that h or nothing; none, or beyond the range: every element takes the scalar form.
struct Operand { const void* ptr; size_t esz; };
inline Split split_for(long n, std::initializer_list<Operand> ptrs, long forced = -1) {
  long head = n;
  for (long h = forced < 0 ? 0 : forced, end = forced < 0 ? 8 : forced + 1; h < end; ++h) {
    bool aligned = true;
    for (const Operand& o : ptrs) aligned = aligned && (((uintptr_t)o.ptr + o.esz * h) & 15) == 0;
    if (aligned) { head = h < n ? h : n; break; }
  }
  return Split{head, (n - head) >> 3};
}
inline int grid_for(long n, Split s) {
  const long nscalar = n - (s.groups << 3);
  return grid_for(s.groups > nscalar ? s.groups : nscalar);
}

// (mdtype, gdtype) -> f(moment type tag, gradient type tag); false: no such pair, f was not called
template <typename T> struct Tag { typedef T type; };
template <typename F> bool adamw_dispatch(int mdtype, int gdtype, F f) {
  if (gdtype < 0 || gdtype > 1) return false;
  auto with_g = [&](auto tm) { if (gdtype == 0) f(tm, Tag<bf16_t>()); else f(tm, Tag<float>()); };
  if (mdtype == 0) with_g(Tag<bf16_t>());
  else if (mdtype == 1) with_g(Tag<float>());
  else if (mdtype == 2) with_g(Tag<f16_t>());
  else return false;
  return true;
}

// par = the bf16 parameter pointer (the default kernel, s unused) or a policy of the wide kernel
template <typename P>
int launch_adamw(long n, P par, Split s, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                 hipStream_t st) {
  constexpr bool wide = !std::is_pointer<P>::value;
  dim3 grid(wide ? grid_for(n, s) : grid_for(n)), blk(256);
  const float* hy = (const float*)hyper; const float* cf = (const float*)coef;
  const bool ok = adamw_dispatch(mdtype, gdtype, [&](auto tm, auto tg) {
    typedef typename decltype(tm)::type TM; typedef typename decltype(tg)::type TG;
    if constexpr (wide) az_launch((adamw_wide_kernel<TM, TG, P>), grid, blk, 0, st, n, par, (const TG*)g, (TM*)m, (TM*)v, hy, cf, s);
    else az_launch((adamw_kernel<TM, TG>), grid, blk, 0, st, n, par, (const TG*)g, (TM*)m, (TM*)v, hy, cf);
  });
  if (!ok) return AZ_ERR_ARG(60);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}
int launch_adamw(long n, void* p, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                 hipStream_t st) {
  return launch_adamw(n, (bf16_t*)p, Split{n, 0}, g, gdtype, m, v, mdtype, hyper, coef, st);
}

// Stochastic rounding: a group needs (elem0 + i) % 8 == 0 AND 16-byte aligned p, g, m, v at the same i -- true whenever the range
// starts on an owner's flat buffer (elem0 is then the offset in it); otherwise every element takes the scalar path.
int launch_adamw_sr(long n, void* p, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                    long seed, long step, long domain, long elem0, hipStream_t st) {
  if (mdtype < 0 || mdtype > 2 || gdtype < 0 || gdtype > 1 || elem0 < 0) return AZ_ERR_ARG(68);
  const size_t esz = mdtype == 1 ? 4 : 2, gsz = gdtype == 0 ? 2 : 4;
  const SrArgs sr = {(uint32_t)(unsigned long)seed, (uint32_t)((unsigned long)seed >> 32), (uint32_t)step, (uint32_t)domain, elem0};
  const Split s = split_for(n, {{p, 2}, {g, gsz}, {m, esz}, {v, esz}}, (8 - (elem0 & 7)) & 7);
  return launch_adamw(n, SrParam{(bf16_t*)p, sr}, s, g, gdtype, m, v, mdtype, hyper, coef, st);
}

template <typename P>
int launch_adamw_seg(long n, P par, Split s, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                     const SegTab& t, hipStream_t st) {
  dim3 grid(grid_for(n, s)), blk(256);
  const float* hy = (const float*)hyper; const float* cf = (const float*)coef;
  const bool ok = adamw_dispatch(mdtype, gdtype, [&](auto tm, auto tg) {
    typedef typename decltype(tm)::type TM; typedef typename decltype(tg)::type TG;
    az_launch((adamw_seg_kernel<TM, TG, P>), grid, blk, 0, st, n, par, (const TG*)g, (TM*)m, (TM*)v, hy, cf, s, t);
  });
  if (!ok) return AZ_ERR_ARG(79);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

// ---- fp32 exponential moving average of the bf16 parameters (an option the reference does not have: INTEGRATION.md) -------------------
// diffusers' EMAModel.step form, s.sub_(one_minus_decay * (s - p)): three fp32 operations, three roundings, no contraction.
__device__ __forceinline__ float ema_math(float e, float p, float omd) {
#pragma clang fp contract(off)
  float t = e - p;
  t = omd * t;
  return e - t;
}

// az_ema_flat: the scalar head [0, head), then `groups` groups of 8 elements with 16-byte accesses (one load of p, two loads and two
// stores of e per thread), then the scalar tail up to n -- the split of adamw_wide_kernel (split_for).
__global__ void ema_kernel(long n, const bf16_t* __restrict__ p, float* __restrict__ e, float omd, Split s) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  const long head = s.head, groups = s.groups;
  const long body = head + (groups << 3);                    // <= n (split_for)
  for (long gi = tid; gi < groups; gi += nthr) {
    const long i = head + (gi << 3);
    float pp[8], ee[8];
    load8<bf16_t>(p + i, pp); load8<float>(e + i, ee);
#pragma unroll
    for (int k = 0; k < 8; ++k) ee[k] = ema_math(ee[k], pp[k], omd);
    store8_moment<float>(e + i, ee);
  }
  const long nscalar = n - (groups << 3);                    // head + tail
  for (long j = tid; j < nscalar; j += nthr) {
    const long i = j < head ? j : j - head + body;
    e[i] = ema_math(e[i], bf2f(p[i]), omd);
  }
}

// Hand-off events of the chunk pipeline, one set per COMPUTE STREAM (a stream belongs to one device, so two optimizers,
// threads or devices in one process never share a set); creation is serialised by a mutex.  Calls that name the same
// compute stream must come from one host thread at a time -- the stream's own order is what sequences them.
struct EvPool {
  hipEvent_t h2d[2], comp[2], d2h[2];
};
std::mutex g_ev_mutex;
std::map<hipStream_t, EvPool> g_ev_pools;

int ev_pool_for(hipStream_t sc, EvPool** out) {
  std::lock_guard<std::mutex> lock(g_ev_mutex);
  auto it = g_ev_pools.find(sc);
  if (it == g_ev_pools.end()) {
    EvPool ep;
    for (int i = 0; i < 2; ++i) {
      AZ_HIP(hipEventCreateWithFlags(&ep.h2d[i], hipEventDisableTiming));
      AZ_HIP(hipEventCreateWithFlags(&ep.comp[i], hipEventDisableTiming));
      AZ_HIP(hipEventCreateWithFlags(&ep.d2h[i], hipEventDisableTiming));
    }
    it = g_ev_pools.emplace(sc, ep).first;
  }
  *out = &it->second;
  return AZ_OK;
}

struct SrCall { long seed, step, domain, elem0; };

// Chunk pipeline: H2D(m,v)[c+1]  ||  adamw[c]  ||  D2H(m,v)[c-1]; staging = 2 buffers x (m,v) x chunk.  sr: stochastic rounding, each
// chunk's launch names the global index of ITS first element (elem0 + chunk offset).
int raven_pipeline(long n, void* p, const void* g, int gdtype, void* m_host, void* v_host, int mdtype, const void* hyper,
                   const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                   void* stream_d2h, const SrCall* sr) {
  if (n <= 0 || chunk_elems <= 0 || mdtype < 0 || mdtype > 2) return AZ_ERR_ARG(64);
  hipStream_t sc = (hipStream_t)stream_compute, sh = (hipStream_t)stream_h2d, sd = (hipStream_t)stream_d2h;
  EvPool* evp = nullptr;
  { int rc0 = ev_pool_for(sc, &evp); if (rc0) return rc0; }
  EvPool& g_ev = *evp;
  const size_t esz = mdtype == 1 ? 4 : 2;
  const size_t gsz = gdtype == 0 ? 2 : 4;
  char* stg = (char*)staging;
  const long nchunk = (n + chunk_elems - 1) / chunk_elems;
  // the copy streams must not start before work already queued on the compute stream (grads, coef)
  hipEvent_t& start = g_ev.comp[0];
  AZ_HIP(hipEventRecord(start, sc));
  AZ_HIP(hipStreamWaitEvent(sh, start, 0));
  for (long c = 0; c < nchunk; ++c) {
    const int buf = (int)(c & 1);
    const long off = c * chunk_elems;
    const long len = (off + chunk_elems <= n) ? chunk_elems : (n - off);
    char* mb = stg + (size_t)buf * 2 * chunk_elems * esz;
    char* vb = mb + (size_t)chunk_elems * esz;
    if (c >= 2) AZ_HIP(hipStreamWaitEvent(sh, g_ev.d2h[buf], 0));       // staging buffer free again
    AZ_HIP(hipMemcpyAsync(mb, (char*)m_host + off * esz, len * esz, hipMemcpyHostToDevice, sh));
    AZ_HIP(hipMemcpyAsync(vb, (char*)v_host + off * esz, len * esz, hipMemcpyHostToDevice, sh));
    AZ_HIP(hipEventRecord(g_ev.h2d[buf], sh));
    AZ_HIP(hipStreamWaitEvent(sc, g_ev.h2d[buf], 0));
    int rc = sr ? launch_adamw_sr(len, (bf16_t*)p + off, (const char*)g + off * gsz, gdtype, mb, vb, mdtype, hyper, coef, sr->seed, sr->step,
                                  sr->domain, sr->elem0 + off, sc)
                : launch_adamw(len, (bf16_t*)p + off, (const char*)g + off * gsz, gdtype, mb, vb, mdtype, hyper, coef, sc);
    if (rc) return rc;
    AZ_HIP(hipEventRecord(g_ev.comp[buf], sc));
    AZ_HIP(hipStreamWaitEvent(sd, g_ev.comp[buf], 0));
    AZ_HIP(hipMemcpyAsync((char*)m_host + off * esz, mb, len * esz, hipMemcpyDeviceToHost, sd));
    AZ_HIP(hipMemcpyAsync((char*)v_host + off * esz, vb, len * esz, hipMemcpyDeviceToHost, sd));
    AZ_HIP(hipEventRecord(g_ev.d2h[buf], sd));
  }
  // join: the compute stream observes the end of the last write-backs
  AZ_HIP(hipStreamWaitEvent(sc, g_ev.d2h[0], 0));
  if (nchunk > 1) AZ_HIP(hipStreamWaitEvent(sc, g_ev.d2h[1], 0));
  return AZ_OK;
}

}  // namespace

extern "C" {

int az_sumsq(long n, const void* g, int dtype, void* out_f32, int accumulate, void* scratch_f32, void* stream) {
  if (n <= 0) return AZ_ERR_ARG(61);
  hipStream_t st = (hipStream_t)stream;
  int nblk = grid_for(n); if (nblk > SUMSQ_BLOCKS) nblk = SUMSQ_BLOCKS;
  if (dtype == 0) {
    if ((uintptr_t)g & 15) return AZ_ERR_ARG(62);
    az_launch(sumsq_partial_kernel<bf16_t>, dim3(nblk), dim3(256), 0, st, n, (const bf16_t*)g, (float*)scratch_f32);
  } else {
    az_launch(sumsq_partial_kernel<float>, dim3(nblk), dim3(256), 0, st, n, (const float*)g, (float*)scratch_f32);
  }
  AZ_CHECK_LAUNCH();
  az_launch(sumsq_final_kernel, dim3(1), dim3(256), 0, st, nblk, (const float*)scratch_f32, (float*)out_f32, accumulate);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_sumsq_bf16(long n, const void* g, void* out_f32, int accumulate, void* scratch_f32, void* stream) {
  return az_sumsq(n, g, 0, out_f32, accumulate, scratch_f32, stream);
}

int az_clip_coef(const void* sumsq_f32, float max_norm, float grad_unscale, void* coef_f32, void* norm_f32, void* stream) {
  az_launch(clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)sumsq_f32, max_norm, grad_unscale,
                     (float*)coef_f32, (float*)norm_f32);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_adamw_flat(long n, void* p, const void* g, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                  void* stream) {
  if (n <= 0) return AZ_ERR_ARG(63);
  return launch_adamw(n, p, g, 0, m, v, mdtype, hyper, coef, (hipStream_t)stream);
}

int az_adamw_flat_ex(long n, void* p, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                     const void* coef, void* stream) {
  if (n <= 0) return AZ_ERR_ARG(63);
  return launch_adamw(n, p, g, gdtype, m, v, mdtype, hyper, coef, (hipStream_t)stream);
}

int az_adamw_flat_sr(long n, void* p, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                     long seed, long step, long domain, long elem0, void* stream) {
  if (n <= 0) return AZ_ERR_ARG(63);
  return launch_adamw_sr(n, p, g, gdtype, m, v, mdtype, hyper, coef, seed, step, domain, elem0, (hipStream_t)stream);
}

int az_ema_flat(long n, const void* p, void* ema_f32, float one_minus_decay, void* stream) {
  if (n < 0 || !p || !ema_f32 || ((uintptr_t)p & 1) || ((uintptr_t)ema_f32 & 3)) return AZ_ERR_ARG(69);
  if (n == 0) return AZ_OK;
  const Split s = split_for(n, {{p, 2}, {ema_f32, 4}});
  az_launch(ema_kernel, dim3(grid_for(n, s)), dim3(256), 0, (hipStream_t)stream, n, (const bf16_t*)p, (float*)ema_f32, one_minus_decay, s);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_adamw_flat_master(long n, void* p, void* w_f32, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                         const void* coef, void* stream) {
  if (n < 0 || !p || !w_f32 || !g || !m || !v || !hyper || mdtype < 0 || mdtype > 2 || gdtype < 0 || gdtype > 1) return AZ_ERR_ARG(76);
  const uintptr_t emask = mdtype == 1 ? 3 : 1, gmask = gdtype == 0 ? 1 : 3;
  if (((uintptr_t)p & 1) || ((uintptr_t)w_f32 & 3) || ((uintptr_t)g & gmask) || ((uintptr_t)m & emask) || ((uintptr_t)v & emask))
    return AZ_ERR_ARG(77);
  if (n == 0) return AZ_OK;
  const Split s = split_for(n, {{p, 2}, {w_f32, 4}, {g, gmask + 1}, {m, emask + 1}, {v, emask + 1}});
  return launch_adamw(n, MasterParam{(bf16_t*)p, (float*)w_f32}, s, g, gdtype, m, v, mdtype, hyper, coef, (hipStream_t)stream);
}

int az_adamw_flat_seg(long n, void* p, void* w_f32, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                      const void* coef, const void* seg_end, const void* seg_gid, long nseg, const void* ghyper, int ngroups, long elem0,
                      int rounding, long seed, long step, long domain, void* stream) {
  if (n < 0 || !p || !g || !m || !v || !hyper || !seg_end || !seg_gid || !ghyper || nseg <= 0 || nseg > 0x7FFFFFFFL || ngroups <= 0 ||
      ngroups > 255 || elem0 < 0 || mdtype < 0 || mdtype > 2 || gdtype < 0 || gdtype > 1 || rounding < 0 || rounding > 1 || (w_f32 && rounding))
    return AZ_ERR_ARG(79);
  const uintptr_t emask = mdtype == 1 ? 3 : 1, gmask = gdtype == 0 ? 1 : 3;
  if (((uintptr_t)p & 1) || ((uintptr_t)w_f32 & 3) || ((uintptr_t)g & gmask) || ((uintptr_t)m & emask) || ((uintptr_t)v & emask) ||
      ((uintptr_t)seg_end & 7) || ((uintptr_t)seg_gid & 3) || ((uintptr_t)ghyper & 3))
    return AZ_ERR_ARG(80);
  if (n == 0) return AZ_OK;
  const SegTab t = {(const long*)seg_end, (const int*)seg_gid, (const float*)ghyper, (int)nseg, ngroups, elem0};
  hipStream_t st = (hipStream_t)stream;
  if (w_f32) {
    const Split s = split_for(n, {{p, 2}, {w_f32, 4}, {g, gmask + 1}, {m, emask + 1}, {v, emask + 1}});
    return launch_adamw_seg(n, MasterParam{(bf16_t*)p, (float*)w_f32}, s, g, gdtype, m, v, mdtype, hyper, coef, t, st);
  }
  if (rounding) {           // a group of 8 is a Philox group: (elem0 + i) % 8 == 0 there (launch_adamw_sr)
    const SrArgs sr = {(uint32_t)(unsigned long)seed, (uint32_t)((unsigned long)seed >> 32), (uint32_t)step, (uint32_t)domain, elem0};
    const Split s = split_for(n, {{p, 2}, {g, gmask + 1}, {m, emask + 1}, {v, emask + 1}}, (8 - (elem0 & 7)) & 7);
    return launch_adamw_seg(n, SrParam{(bf16_t*)p, sr}, s, g, gdtype, m, v, mdtype, hyper, coef, t, st);
  }
  const Split s = split_for(n, {{p, 2}, {g, gmask + 1}, {m, emask + 1}, {v, emask + 1}});
  return launch_adamw_seg(n, PlainParam{(bf16_t*)p}, s, g, gdtype, m, v, mdtype, hyper, coef, t, st);
}

int az_raven_step_ex(long n, void* p, const void* g, int gdtype, void* m_host, void* v_host, int mdtype, const void* hyper,
                     const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                     void* stream_d2h) {
  return raven_pipeline(n, p, g, gdtype, m_host, v_host, mdtype, hyper, coef, staging, chunk_elems, stream_compute, stream_h2d, stream_d2h,
                        nullptr);
}

int az_raven_step_sr(long n, void* p, const void* g, int gdtype, void* m_host, void* v_host, int mdtype, const void* hyper,
                     const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                     void* stream_d2h, long seed, long step, long domain, long elem0) {
  if (gdtype < 0 || gdtype > 1 || elem0 < 0) return AZ_ERR_ARG(64);
  const SrCall sr = {seed, step, domain, elem0};
  return raven_pipeline(n, p, g, gdtype, m_host, v_host, mdtype, hyper, coef, staging, chunk_elems, stream_compute, stream_h2d, stream_d2h,
                        &sr);
}
int az_raven_step(long n, void* p, const void* g, void* m_host, void* v_host, int mdtype, const void* hyper,
                  const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                  void* stream_d2h) {
  return az_raven_step_ex(n, p, g, 0, m_host, v_host, mdtype, hyper, coef, staging, chunk_elems, stream_compute, stream_h2d, stream_d2h);
}

int az_titan_offload(long n, const void* g, void* g_host_f32, void* staging_f32, int accumulate, void* stream) {
  (void)staging_f32;
  if (n <= 0) return AZ_ERR_ARG(65);
  az_launch(offload_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (const bf16_t*)g, (float*)g_host_f32, accumulate);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_scale_bf16(long n, void* g, const void* coef_f32, void* stream) {
  if (n <= 0) return AZ_ERR_ARG(67);
  az_launch(scale_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (bf16_t*)g, (const float*)coef_f32);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_scale_f32(long n, void* x, const void* coef_f32, void* stream) {
  if (n <= 0) return AZ_ERR_ARG(66);
  az_launch(scale_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (float*)x, (const float*)coef_f32);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

}  // extern "C"
