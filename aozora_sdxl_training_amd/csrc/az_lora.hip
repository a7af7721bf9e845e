// LoRA adapter products (include/aozora_hip.h az_lora_*): three shapes of product with one tiny dimension, each on
// v_mfma_f32_16x16x32_bf16 with the small dimension padded to 16 (or 32 as the k-depth) by zero FRAGMENTS -- never in memory.
//   down  : OUT[M][r]   = s X[M][K] . W[r][K]^T          one pass over X; a block's 4 waves split the k-range, fixed-order sum
//   up    : Y[M][N]    += s U[M][r] . W[N][r]^T          read-modify-write of Y, k-depth r (+ the GEGLU of ff.net.0.proj in the epilogue)
//   wgrad : OUT[ns][nb] (+)= s S[M][ns]^T . G[M][nb]     sum over M: fp32 partials per row range, then a fixed-order second stage
// All three use the operand order of az_gemm.hip (D^T = small-frag x big-frag), so a lane owns 4 consecutive output columns.
// Operand maps of the MFMA: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7; the result
// D[row = 4 (l >> 4) + i][col = l & 15], i = 0..3.  No floating-point atomics anywhere: every sum has a fixed order.
// Behind them, the same three shapes for an adapter on a 3x3 convolution (az_lora_conv_*): the big operand gathered over the nine taps.
// Last, the two passes that are no product of activations: the dropout masks (az_lora_dropout_bf16) and max-norm regularisation
// (az_lora_max_norm_bf16: the Gram matrices A A^T and B^T B of every module in one launch).  Behind those, DoRA (az_dora_*): the row
// norms of W + s B A of every module in one launch, the per-column gain of the forward and its backward.
#include "az_common.h"
#include "aozora_hip.h"

namespace {

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// elements k .. k + 7 of a row of kdim (a multiple of 4) elements that is only 8-byte aligned; zeros from kdim on and when !ok
__device__ __forceinline__ bf16x8 load_small8(const bf16_t* row, int k, int kdim, bool ok) {
  bf16x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
  if (ok && k < kdim) lo = *(const bf16x4*)(row + k);
  if (ok && k + 4 < kdim) hi = *(const bf16x4*)(row + k + 4);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ bf16x4 pack4(f32x4 v) {
  bf16x4 o;
  o[0] = (short)f2bf(v[0]); o[1] = (short)f2bf(v[1]); o[2] = (short)f2bf(v[2]); o[3] = (short)f2bf(v[3]);
  return o;
}

// ---- down: OUT[m][p r + n] = bf16(s sum_k X[m][p xps + k] W_p[n][k]) ---------------------------------------------------------------
// A block owns 16 rows of X and all r outputs of part blockIdx.y (NT tiles of 16).  Its 4 waves deal the k-range among themselves in
// groups of KU 32-deep steps (the loads of a group are issued together: the product is bound by the latency of its one pass over X,
// and a grid of M / 16 blocks keeps 4 waves per row tile in flight); wave 0 adds the other three partial sums in wave order.
template <int NT, int KU>
__global__ __launch_bounds__(256) void lora_down_kernel(int M, int K, int r, float s, const bf16_t* __restrict__ X, long ldx, long xps,
                                                        const bf16_t* __restrict__ W, long ldw, long wps, bf16_t* __restrict__ U, long ldu) {
  __shared__ f32x4 red[3][NT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.y;
  const long m0 = (long)blockIdx.x * 16;
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const long m = m0 + li;
  const bool mok = m < M;
  const bf16_t* xrow = X + (mok ? m : 0) * ldx + (long)p * xps;
  const bf16_t* wp = W + (long)p * wps;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 32 * KU; k0 < K; k0 += 4 * 32 * KU) {
    bf16x8 xf[KU], wf[KU][NT];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = k0 + 32 * u + kq;
      const bool kok = k < K;                     // K % 8 == 0: an 8-chunk is inside or outside as a whole
      xf[u] = zero8;
      if (mok && kok) xf[u] = *(const bf16x8*)(xrow + k);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n = t * 16 + li;
        wf[u][t] = zero8;
        if (kok && n < r) wf[u][t] = *(const bf16x8*)(wp + (long)n * ldw + k);
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma16(wf[u][t], xf[u], acc[t]);
    }
  }
  if (wave) {
#pragma unroll
    for (int t = 0; t < NT; ++t) red[wave - 1][t][lane] = acc[t];
  }
  __syncthreads();
  if (wave || !mok) return;
  bf16_t* urow = U + m * ldu + (long)p * r;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n4 = t * 16 + (lane >> 4) * 4;
    const f32x4 v = ((acc[t] + red[0][t][lane]) + red[1][t][lane]) + red[2][t][lane];
    if (n4 < r) *(bf16x4*)(urow + n4) = pack4(v * s);
  }
}

// One 16 x 16 tile of an up product, shared by lora_up_kernel and lora_up_geglu_kernel so that both give the same bits: the sum over
// the KS 32-deep k-steps in ascending order (W fragment x U fragment: a lane owns 4 consecutive columns of its row), then the
// epilogue bf16(float(previous) + s sum).
template <int KS>
__device__ __forceinline__ f32x4 up_tile_sum(const bf16_t* wrow, const bf16x8 (&uf)[KS], int kq, int r, bool wok) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) acc = mfma16(load_small8(wrow, ks * 32 + kq, r, wok), uf[ks], acc);
  return acc;
}
__device__ __forceinline__ bf16x4 up_tile_out(bf16x4 y, f32x4 acc, float s) {
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = bf2f((bf16_t)y[i]) + s * acc[i];
  return pack4(o);
}

// ---- up: Y[m][p yps + n] = bf16(float(Y) + s sum_{k < r} U[m][p ups + k] W_p[n][k]) -------------------------------------------------
// A wave owns 16 rows and 128 columns of part blockIdx.z; its U fragments (KS k-steps of 32) are loaded once.
template <int KS>
__global__ __launch_bounds__(256) void lora_up_kernel(int M, int N, int r, float s, const bf16_t* __restrict__ U, long ldu, long ups,
                                                      const bf16_t* __restrict__ W, long ldw, long wps, bf16_t* Y, long ldy, long yps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.z;
  const long m0 = ((long)blockIdx.y * 4 + wave) * 16;
  if (m0 >= M) return;
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const long m = m0 + li;
  const bool mok = m < M;
  const bf16_t* urow = U + (mok ? m : 0) * ldu + (long)p * ups;
  bf16x8 uf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) uf[ks] = load_small8(urow, ks * 32 + kq, r, mok);
  const bf16_t* wp = W + (long)p * wps;
  bf16_t* yrow = Y + (mok ? m : 0) * ldy + (long)p * yps;
  const int nbeg = blockIdx.x * 128, nend = min(N, nbeg + 128);
  for (int n0 = nbeg; n0 < nend; n0 += 16) {
    const int nw = n0 + li;
    const bool wok = nw < N;
    const bf16_t* wrow = wp + (long)(wok ? nw : 0) * ldw;
    const int n4 = n0 + (lane >> 4) * 4;
    const bool yok = mok && n4 < N;               // N % 4 == 0: a 4-group is inside or outside as a whole
    bf16x4 y = {0, 0, 0, 0};
    if (yok) y = *(const bf16x4*)(yrow + n4);     // issued with the W loads: one latency per tile, not two
    const f32x4 acc = up_tile_sum<KS>(wrow, uf, kq, r, wok);
    if (yok) *(bf16x4*)(yrow + n4) = up_tile_out(y, acc, s);
  }
}

// ---- up + GEGLU: proj[m][n] = bf16(float(proj) + s sum_{k < r} U[m][k] W[n][k]), n < 2 H; out[m][h] = bf16(value * gelu(gate)) ------------
// lora_up_kernel on the [M][2 H] projection of ff.net.0.proj with az_geglu_fwd in its epilogue.  A wave owns 16 rows and 64 VALUE
// columns together with the 64 GATE columns H + n of the same n: two MFMA chains per 16-column tile (same operand order, same k-step
// order, same epilogue expression as lora_up_kernel: proj gets that kernel's bits), both halves are packed and stored, and out is
// formed from the PACKED values in registers -- the bits az_geglu_fwd computes from the stored proj, without reading it back.
template <int KS>
__global__ __launch_bounds__(256) void lora_up_geglu_kernel(int M, int H, int r, float s, const bf16_t* __restrict__ U, long ldu,
                                                            const bf16_t* __restrict__ W, long ldw, bf16_t* P, long ldp,
                                                            bf16_t* __restrict__ out, long ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long m0 = ((long)blockIdx.y * 4 + wave) * 16;
  if (m0 >= M) return;
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const long m = m0 + li;
  const bool mok = m < M;
  const bf16_t* urow = U + (mok ? m : 0) * ldu;
  bf16x8 uf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) uf[ks] = load_small8(urow, ks * 32 + kq, r, mok);
  bf16_t* prow = P + (mok ? m : 0) * ldp;
  bf16_t* orow = out + (mok ? m : 0) * ldo;
  const int nbeg = blockIdx.x * 64, nend = min(H, nbeg + 64);
  for (int n0 = nbeg; n0 < nend; n0 += 16) {
    const int nw = n0 + li;
    const bool wok = nw < H;
    const bf16_t* wval = W + (long)(wok ? nw : 0) * ldw;
    const bf16_t* wgate = wval + (long)H * ldw;
    const int n4 = n0 + (lane >> 4) * 4;
    const bool yok = mok && n4 < H;               // H % 8 == 0: a 4-group is inside or outside as a whole, in both halves
    bf16x4 yv = {0, 0, 0, 0}, yg = {0, 0, 0, 0};
    if (yok) {                                    // issued with the W loads: one latency per tile, not two
      yv = *(const bf16x4*)(prow + n4);
      yg = *(const bf16x4*)(prow + H + n4);
    }
    const f32x4 av = up_tile_sum<KS>(wval, uf, kq, r, wok);
    const f32x4 ag = up_tile_sum<KS>(wgate, uf, kq, r, wok);
    if (yok) {
      const bf16x4 pv = up_tile_out(yv, av, s), pg = up_tile_out(yg, ag, s);
      *(bf16x4*)(prow + n4) = pv;
      *(bf16x4*)(prow + H + n4) = pg;
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = bf2f((bf16_t)pv[i]) * gelu_erf(bf2f((bf16_t)pg[i]));
      *(bf16x4*)(orow + n4) = pack4(o);
    }
  }
}

// ---- wgrad, stage 1: P[p][split][i_s][i_b] = sum over the split's rows of S[m][p sps + i_s] G[m][p gps + i_b] (fp32) -----------------
// A block owns 64 columns of G (16 per wave), all ns columns of S (NT tiles of 16) and rows [split rps, min(M, (split + 1) rps)).
// Both operands are k-strided in memory (k = the row), so each 32-row slice goes through LDS transposed: T[column][40] with the 32
// rows contiguous (80-byte row stride: 16-byte aligned fragment reads).  One buffer, two barriers per slice.
constexpr int LKP = 40;
template <int NT>
__global__ __launch_bounds__(256) void lora_wgrad_partial_kernel(int M, int ns, int nb, int rps, const bf16_t* __restrict__ S, long ld_s, long sps,
                                                                 const bf16_t* __restrict__ G, long ld_g, long gps, float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) bf16_t St[NT * 16 * LKP];
  __shared__ __attribute__((aligned(16))) bf16_t Gt[64 * LKP];
  constexpr int SQ = NT * 4;                       // 4-element groups per row of the S slice (padded to NT * 16 columns)
  constexpr int SI = (32 * SQ + 255) / 256;        // ... per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.y, nsplit = gridDim.y, p = blockIdx.z;
  const int b0 = blockIdx.x * 64;
  const long mbeg = (long)split * rps, mend = min((long)M, mbeg + rps);
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const bf16_t* Sp = S + (long)p * sps;
  const bf16_t* Gp = G + (long)p * gps;
  const int grow = tid >> 3, gcol = (tid & 7) * 8;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 gv;
  bf16x4 sv[SI];
  // the global loads of a slice are issued one slice ahead (registers), so they fly under the previous slice's LDS round and MFMAs
  auto load_slice = [&](long mk) {
    gv = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (mk + grow < mend && b0 + gcol < nb) gv = *(const bf16x8*)(Gp + (mk + grow) * ld_g + b0 + gcol);      // nb % 8 == 0
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int it = tid + i * 256, row = it / SQ, c4 = (it % SQ) * 4;
      sv[i] = bf16x4{0, 0, 0, 0};
      if (it < 32 * SQ && mk + row < mend && c4 < ns) sv[i] = *(const bf16x4*)(Sp + (mk + row) * ld_s + c4);  // ns % 4 == 0
    }
  };
  load_slice(mbeg);
  for (long mk = mbeg; mk < mend; mk += 32) {
    __syncthreads();                               // the previous slice's fragments have been read
#pragma unroll
    for (int j = 0; j < 8; ++j) Gt[(gcol + j) * LKP + grow] = (bf16_t)gv[j];
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int it = tid + i * 256, row = it / SQ, c4 = (it % SQ) * 4;
      if (it < 32 * SQ) {
#pragma unroll
        for (int j = 0; j < 4; ++j) St[(c4 + j) * LKP + row] = (bf16_t)sv[i][j];
      }
    }
    __syncthreads();
    if (mk + 32 < mend) load_slice(mk + 32);
    const bf16x8 gf = *(const bf16x8*)(Gt + (wave * 16 + li) * LKP + kq);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma16(*(const bf16x8*)(St + (t * 16 + li) * LKP + kq), gf, acc[t]);
  }
  const int ib = b0 + wave * 16 + li;
  if (ib >= nb) return;
  float* Pp = P + ((long)p * nsplit + split) * ns * nb;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int is = t * 16 + (lane >> 4) * 4 + i;
      if (is < ns) Pp[(long)is * nb + ib] = acc[t][i];
    }
  }
}

// ---- wgrad, stage 2: out(p, i_s, i_b) = bf16((accumulate ? float(out) : 0) + s sum_split P[p][split][i_s][i_b]), splits ascending -----
__global__ __launch_bounds__(256) void lora_wgrad_finish_kernel(int ns, int nb, int parts, int nsplit, float s, const float* __restrict__ P,
                                                                bf16_t* out, long os_s, long os_b, long ops, int accumulate) {
  const long per = (long)ns * nb, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per * parts) return;
  const int p = (int)(i / per);
  const long e = i - (long)p * per;
  const int is = (int)(e / nb), ib = (int)(e - (long)is * nb);
  const float* src = P + (long)p * nsplit * per + e;
  float sum = 0.f;
  for (int k = 0; k < nsplit; ++k) sum += src[(long)k * per];
  bf16_t* o = out + (long)p * ops + (long)is * os_s + (long)ib * os_b;
  float v = s * sum;
  if (accumulate) v = bf2f(*o) + v;
  *o = f2bf(v);
}

// ==== adapters on 3x3 convolutions (stride 1, pad 1; az_lora_conv_*) ================================================================
// The same three shapes of product with the big operand GATHERED: row m = (b, h, w) of an NHWC activation [B H W][C] (any row stride)
// meets, at tap t = 3 kh + kw, the row of pixel (h + kh - 1, w + kw - 1) of the SAME image.  A tap outside the image is a zero
// fragment and never a load.  k = t Cin + c is the summed index of the down product and the column index of the weight gradient
// (A is stored [r][3][3][Cin]: a row of A is one k-contiguous vector of 9 Cin elements; Cin % 8 == 0, so an 8-chunk never straddles
// two taps); the data gradient sums over (t, j) through the copy At [Cin][3][3][r] with the taps mirrored.

// row of the neighbour (dh, dw) of pixel row m = (b, h, w), or -1 outside image b
__device__ __forceinline__ long nbr_row(long m, int h, int w, int H, int W, int dh, int dw) {
  return ((unsigned)(h + dh) < (unsigned)H && (unsigned)(w + dw) < (unsigned)W) ? m + (long)dh * W + dw : -1;
}

// ---- conv down: U[m][n] = bf16(s sum_t sum_c X[nbr(m, t)][c] A[n][t][c]) ------------------------------------------------------------
// lora_down_kernel over the k-range 9 Cin with the row pointer re-derived per 8-chunk (its tap): a block owns 16 pixels, its 4 waves
// deal the k-range among themselves in groups of KU 32-deep steps, wave 0 adds the other three partial sums in wave order.
template <int NT, int KU>
__global__ __launch_bounds__(256) void lora_conv_down_kernel(int M, int H, int W, int Cin, int r, float s, const bf16_t* __restrict__ X, long ldx,
                                                             const bf16_t* __restrict__ A, bf16_t* __restrict__ U, long ldu) {
  __shared__ f32x4 red[3][NT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long m0 = (long)blockIdx.x * 16;
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const long m = m0 + li;
  const bool mok = m < M;
  const long pix = mok ? m : 0;
  const int pw = (int)(pix % W), ph = (int)((pix / W) % H);
  const int K = 9 * Cin;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 32 * KU; k0 < K; k0 += 4 * 32 * KU) {
    bf16x8 xf[KU], wf[KU][NT];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = k0 + 32 * u + kq;
      const bool kok = k < K;                     // K % 8 == 0: an 8-chunk is inside or outside as a whole
      const int tap = kok ? k / Cin : 0, c = k - tap * Cin;
      const long row = nbr_row(pix, ph, pw, H, W, tap / 3 - 1, tap % 3 - 1);
      xf[u] = zero8;
      if (mok && kok && row >= 0) xf[u] = *(const bf16x8*)(X + row * ldx + c);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n = t * 16 + li;
        wf[u][t] = zero8;
        if (kok && n < r) wf[u][t] = *(const bf16x8*)(A + (long)n * K + k);
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma16(wf[u][t], xf[u], acc[t]);
    }
  }
  if (wave) {
#pragma unroll
    for (int t = 0; t < NT; ++t) red[wave - 1][t][lane] = acc[t];
  }
  __syncthreads();
  if (wave || !mok) return;
  bf16_t* urow = U + m * ldu;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n4 = t * 16 + (lane >> 4) * 4;
    const f32x4 v = ((acc[t] + red[0][t][lane]) + red[1][t][lane]) + red[2][t][lane];
    if (n4 < r) *(bf16x4*)(urow + n4) = pack4(v * s);
  }
}

// ---- conv dgrad: dX[m][c] = bf16(float(dX[m][c]) + s sum_t sum_{j < r} dU[nbr(m, mirrored t)][j] At[c][t][j]) ------------------------
// lora_up_kernel with k = (tap, j): a wave owns 16 pixels and 128 channels; its dU fragments -- nine gathered rows, KS k-steps of 32
// each, the rank padded by zero fragments -- are loaded once.  The sum runs over the taps in ascending order.
template <int KS>
__global__ __launch_bounds__(256) void lora_conv_dgrad_kernel(int M, int H, int W, int Cin, int r, float s, const bf16_t* __restrict__ dU, long ldu,
                                                              const bf16_t* __restrict__ At, bf16_t* dX, long ldx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long m0 = ((long)blockIdx.y * 4 + wave) * 16;
  if (m0 >= M) return;
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const long m = m0 + li;
  const bool mok = m < M;
  const long pix = mok ? m : 0;
  const int pw = (int)(pix % W), ph = (int)((pix / W) % H);
  bf16x8 uf[9][KS];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const long row = nbr_row(pix, ph, pw, H, W, 1 - tap / 3, 1 - tap % 3);      // y[q] reads x[q + d]: x[p] is read by y[p - d]
    const bool ok = mok && row >= 0;
    const bf16_t* urow = dU + (ok ? row : 0) * ldu;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) uf[tap][ks] = load_small8(urow, ks * 32 + kq, r, ok);
  }
  bf16_t* xrow = dX + pix * ldx;
  const int nbeg = blockIdx.x * 128, nend = min(Cin, nbeg + 128);
  for (int n0 = nbeg; n0 < nend; n0 += 16) {
    const int nw = n0 + li;
    const bool wok = nw < Cin;
    const bf16_t* wrow = At + (long)(wok ? nw : 0) * 9 * r;
    const int n4 = n0 + (lane >> 4) * 4;
    const bool yok = mok && n4 < Cin;             // Cin % 8 == 0: a 4-group is inside or outside as a whole
    bf16x4 y = {0, 0, 0, 0};
    if (yok) y = *(const bf16x4*)(xrow + n4);     // issued with the At loads: one latency per tile, not two
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = mfma16(load_small8(wrow + tap * r, ks * 32 + kq, r, wok), uf[tap][ks], acc);
    }
    if (yok) *(bf16x4*)(xrow + n4) = up_tile_out(y, acc, s);
  }
}

// ---- conv wgrad, stage 1: P[split][j][t Cin + c] = sum over the split's pixels of dU[m][j] X[nbr(m, t)][c] (fp32) ---------------------
// lora_wgrad_partial_kernel whose big operand has 9 Cin gathered columns: a block owns 64 of them (8-chunks of one tap each), all
// r columns of dU and one row range.  Stage 2 is lora_wgrad_finish_kernel (out strides 9 Cin, 1).
template <int NT>
__global__ __launch_bounds__(256) void lora_conv_wgrad_partial_kernel(int M, int H, int W, int Cin, int ns, int rps, const bf16_t* __restrict__ S, long ld_s,
                                                                      const bf16_t* __restrict__ X, long ldx, float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) bf16_t St[NT * 16 * LKP];
  __shared__ __attribute__((aligned(16))) bf16_t Gt[64 * LKP];
  constexpr int SQ = NT * 4;
  constexpr int SI = (32 * SQ + 255) / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.y, nb = 9 * Cin;
  const int b0 = blockIdx.x * 64;
  const long mbeg = (long)split * rps, mend = min((long)M, mbeg + rps);
  const int li = lane & 15, kq = (lane >> 4) * 8;
  const int grow = tid >> 3, gcol = b0 + (tid & 7) * 8;
  const bool gok = gcol < nb;                      // nb % 8 == 0
  const int gtap = gok ? gcol / Cin : 0, gc = gcol - gtap * Cin, gdh = gtap / 3 - 1, gdw = gtap % 3 - 1;
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 gv;
  bf16x4 sv[SI];
  auto load_slice = [&](long mk) {
    gv = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    const long pix = mk + grow;
    if (pix < mend && gok) {
      const long row = nbr_row(pix, (int)((pix / W) % H), (int)(pix % W), H, W, gdh, gdw);
      if (row >= 0) gv = *(const bf16x8*)(X + row * ldx + gc);
    }
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int it = tid + i * 256, row = it / SQ, c4 = (it % SQ) * 4;
      sv[i] = bf16x4{0, 0, 0, 0};
      if (it < 32 * SQ && mk + row < mend && c4 < ns) sv[i] = *(const bf16x4*)(S + (mk + row) * ld_s + c4);  // ns % 4 == 0
    }
  };
  load_slice(mbeg);
  for (long mk = mbeg; mk < mend; mk += 32) {
    __syncthreads();                               // the previous slice's fragments have been read
#pragma unroll
    for (int j = 0; j < 8; ++j) Gt[((tid & 7) * 8 + j) * LKP + grow] = (bf16_t)gv[j];
#pragma unroll
    for (int i = 0; i < SI; ++i) {
      const int it = tid + i * 256, row = it / SQ, c4 = (it % SQ) * 4;
      if (it < 32 * SQ) {
#pragma unroll
        for (int j = 0; j < 4; ++j) St[(c4 + j) * LKP + row] = (bf16_t)sv[i][j];
      }
    }
    __syncthreads();
    if (mk + 32 < mend) load_slice(mk + 32);
    const bf16x8 gf = *(const bf16x8*)(Gt + (wave * 16 + li) * LKP + kq);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma16(*(const bf16x8*)(St + (t * 16 + li) * LKP + kq), gf, acc[t]);
  }
  const int ib = b0 + wave * 16 + li;
  if (ib >= nb) return;
  float* Pp = P + (long)split * ns * nb;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int is = t * 16 + (lane >> 4) * 4 + i;
      if (is < ns) Pp[(long)is * nb + ib] = acc[t][i];
    }
  }
}

// ---- dropout on the adapter's inner activation (include/aozora_hip.h az_lora_dropout_bf16) --------------------------------------
// In place on U[rows][parts r]: element (row, part p, j) is kept iff its three draws are all >= their thresholds, then scaled by inv;
// a dropped one is SELECTED to +0.  The draws are Philox4x32-10 words of (seed; group, step, domain) in the stochastic-rounding
// layout: element index e takes the 16 bits of lane e & 7 of group e >> 3.  The step is read from memory: a replayed launch carries
// its scalar arguments unchanged.
struct DropArgs {
  uint32_t k0, k1;            // key: seed low / high word
  int mid[3];                 // module id per part: e = (mid << 35) + ...
  uint32_t t_net, t_rank;     // thresholds, 0 = the kind is off (nothing drawn)
  uint32_t t_mod;
  float inv;                  // applied iff t_net or t_rank is on
};
constexpr uint32_t DROP_DOM_NET = 0x10A1u, DROP_DOM_RANK = 0x10A2u, DROP_DOM_MOD = 0x10A3u;

__device__ __forceinline__ void drop_group_bits(const DropArgs& a, uint32_t step, uint32_t dom, long e, uint32_t* w) {
  const long group = e >> 3;
  philox4x32_10((uint32_t)group, (uint32_t)((unsigned long)group >> 32), step, dom, a.k0, a.k1, w);
}

// r % 8 == 0, ldu % 8 == 0, U 16-byte aligned: one thread per 8 contiguous columns, which lie in one part, one row and one Philox
// group of each kind (row r + j and b r + j are multiples of 8 with j).
__global__ __launch_bounds__(256) void lora_dropout_vec_kernel(long groups, int r, int gpr, int rows_per_sample, bf16_t* __restrict__ U,
                                                               long ldu, DropArgs a, const uint32_t* __restrict__ step_word) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  long row; int c8;
  divmod(g, gpr, row, c8);
  const int col = c8 * 8, p = col / r, j = col - p * r;
  const uint32_t step = step_word[0];
  const long base = (long)a.mid[p] << 35;
  uint32_t w[4];
  bool on = true;
  if (a.t_mod) {
    drop_group_bits(a, step, DROP_DOM_MOD, base, w);
    on = sr_lane_bits(w, 0) >= a.t_mod;
  }
  uint32_t keep = on ? 0xFFu : 0u;               // bit l: element l of the 8 is kept
  if (a.t_net && keep) {
    drop_group_bits(a, step, DROP_DOM_NET, base + row * r + j, w);
#pragma unroll
    for (int l = 0; l < 8; ++l) if (sr_lane_bits(w, l) < a.t_net) keep &= ~(1u << l);
  }
  if (a.t_rank && keep) {
    const long b = (long)((unsigned)row / (unsigned)rows_per_sample);       // row < rows < 2^31
    drop_group_bits(a, step, DROP_DOM_RANK, base + b * r + j, w);
#pragma unroll
    for (int l = 0; l < 8; ++l) if (sr_lane_bits(w, l) < a.t_rank) keep &= ~(1u << l);
  }
  bf16x8* ptr = (bf16x8*)(U + row * ldu + col);
  bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (keep) {
    v = *ptr;
    const bool scale = (a.t_net | a.t_rank) != 0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      const bf16_t x = (bf16_t)v[l];
      const bf16_t y = scale ? f2bf(bf2f(x) * a.inv) : x;
      v[l] = (keep >> l) & 1u ? (short)y : (short)0;
    }
  }
  *ptr = v;
}

// every other shape (rank 4: 8 columns would span two parts or two rows): one thread per element, the same draws
__global__ __launch_bounds__(256) void lora_dropout_elem_kernel(long n, int r, int width, int rows_per_sample, bf16_t* __restrict__ U, long ldu,
                                                                DropArgs a, const uint32_t* __restrict__ step_word) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long row; int col;
  divmod(i, width, row, col);
  const int p = col / r, j = col - p * r;
  const uint32_t step = step_word[0];
  const long base = (long)a.mid[p] << 35;
  uint32_t w[4];
  bool keep = true;
  if (a.t_mod) {
    drop_group_bits(a, step, DROP_DOM_MOD, base, w);
    keep = sr_lane_bits(w, 0) >= a.t_mod;
  }
  if (a.t_net && keep) {
    const long e = base + row * r + j;
    drop_group_bits(a, step, DROP_DOM_NET, e, w);
    keep = sr_lane_bits(w, (int)(e & 7)) >= a.t_net;
  }
  if (a.t_rank && keep) {
    const long e = base + (long)((unsigned)row / (unsigned)rows_per_sample) * r + j;
    drop_group_bits(a, step, DROP_DOM_RANK, e, w);
    keep = sr_lane_bits(w, (int)(e & 7)) >= a.t_rank;
  }
  bf16_t* ptr = U + row * ldu + col;
  bf16_t y = 0;
  if (keep) {
    y = *ptr;
    if (a.t_net | a.t_rank) y = f2bf(bf2f(y) * a.inv);
  }
  *ptr = y;
}

// ---- max-norm regularisation (kohya-ss scale_weight_norms): || s B A ||_F of every adapted module, both matrices scaled down where it
// exceeds the limit.  || B A ||_F^2 = sum_ij (A A^T)_ij (B^T B)_ij: two r x r Gram matrices, neither they nor the product reach memory.
// One workgroup per module (a row of the job table), so every sum has one fixed order and the result is a pure function of the inputs:
//   G_A = A A^T   the rows of A are k-contiguous: fragments straight from memory, the 4 waves deal the k-steps among themselves
//   G_B = B^T B   the sum runs over the ROWS of B [out][r]: 128 rows at a time are staged in LDS (row stride r + 2: the column reads of
//                 a fragment fall on different banks), wave w takes rows 32 w .. 32 w + 31 of the stage.  An MFMA may see the k index in
//                 any order as long as both operands agree -- here they are the same registers.
// Both run on v_mfma_f32_16x16x32_bf16 with the rank padded to 16 by zero fragments (ranks 4 and 8 included).  The waves' partial Gram
// matrices are added in wave order into LDS, the r^2 products are summed by block_sum, and every thread holds the same norm and takes
// the same decision.  The scaling pass re-reads the module (out of L2) in 16-byte groups.
struct NormJob { const bf16_t* A; const bf16_t* B; long r, K, out, s_bits; float* mA; float* mB; };      // one row of the job table: 8 words
constexpr int MN_STAGE_ROWS = 128;

template <int NT, int KU>
__device__ __forceinline__ void mn_gram_rows(const bf16_t* A, int r, int K, f32x4 (&acc)[NT][NT]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = (lane >> 4) * 8;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k0 = wave * 32 * KU; k0 < K; k0 += 4 * 32 * KU) {
    bf16x8 f[KU][NT];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = k0 + 32 * u + kq;             // K % 8 == 0: an 8-chunk is inside or outside as a whole
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int row = t * 16 + li;
        f[u][t] = zero8;
        if (k < K && row < r) f[u][t] = *(const bf16x8*)(A + (long)row * K + k);
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = mfma16(f[u][ti], f[u][tj], acc[ti][tj]);
      }
    }
  }
}

template <int NT>
__device__ __forceinline__ void mn_gram_cols(const bf16_t* B, int r, int lg, int out, uint32_t* stage, f32x4 (&acc)[NT][NT]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
  const int ld = r + 2;
  const long total = (long)out * r;
  const bf16_t* st16 = (const bf16_t*)stage;
  for (int o0 = 0; o0 < out; o0 += MN_STAGE_ROWS) {
    __syncthreads();                              // the readers of the previous stage are done
    for (int c = threadIdx.x; c < MN_STAGE_ROWS * r / 8; c += 256) {
      const long e = (long)o0 * r + 8L * c;       // out r % 8 == 0: a 16-byte group is inside or outside as a whole
      if (e < total) {
        const u32x4 v = *(const u32x4*)(B + e);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int idx = 8 * c + 2 * p;          // r is even: a pair of columns never straddles a row
          stage[((idx >> lg) * ld + (idx & (r - 1))) >> 1] = v[p];
        }
      }
    }
    __syncthreads();
    bf16x8 f[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int i = t * 16 + li, o = wave * 32 + g * 8;
      const bool ok = i < r && o0 + o < out;      // out % 8 == 0: 8 rows are inside or outside as a whole
#pragma unroll
      for (int j = 0; j < 8; ++j) f[t][j] = ok ? (short)st16[(o + j) * ld + i] : (short)0;
    }
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = mfma16(f[ti], f[tj], acc[ti][tj]);
    }
  }
}

// G[row][col] = ((wave 0 + wave 1) + wave 2) + wave 3 of the waves' partial Gram matrices
template <int NT>
__device__ __forceinline__ void mn_gram_store(float* G, int r, const f32x4 (&acc)[NT][NT]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = ti * 16 + g * 4 + i, col = tj * 16 + li;
            if (row < r && col < r) G[row * r + col] = w ? G[row * r + col] + acc[ti][tj][i] : acc[ti][tj][i];
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int NT, int KU>
__device__ __forceinline__ void mn_grams(const NormJob& jb, int r, int lg, float* gA, float* gB, uint32_t* stage) {
  f32x4 acc[NT][NT];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  mn_gram_rows<NT, KU>(jb.A, r, (int)jb.K, acc);
  mn_gram_store<NT>(gA, r, acc);
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  mn_gram_cols<NT>(jb.B, r, lg, (int)jb.out, stage, acc);
  mn_gram_store<NT>(gB, r, acc);
}

// x <- bf16(float(x) q), or with a master copy w <- w q in fp32 and x <- bf16(w): n % 8 == 0 elements in 16-byte groups
__device__ __forceinline__ void mn_scale(bf16_t* X, float* Wm, long n, float q) {
  for (long c = threadIdx.x; c < n / 8; c += 256) {
    bf16x8* px = (bf16x8*)(X + 8 * c);
    bf16x8 v;
    if (Wm) {
      f32x4* pw = (f32x4*)(Wm + 8 * c);
      const f32x4 a = pw[0] * q, b = pw[1] * q;
      pw[0] = a; pw[1] = b;
#pragma unroll
      for (int l = 0; l < 4; ++l) { v[l] = (short)f2bf(a[l]); v[4 + l] = (short)f2bf(b[l]); }
    } else {
      v = *px;
#pragma unroll
      for (int l = 0; l < 8; ++l) v[l] = (short)f2bf(bf2f((bf16_t)v[l]) * q);
    }
    *px = v;
  }
}

__global__ __launch_bounds__(256) void lora_max_norm_kernel(const NormJob* __restrict__ jobs, float max_norm, float* __restrict__ stats) {
  __shared__ float gA[64 * 64], gB[64 * 64], red[16];
  __shared__ uint32_t stage[MN_STAGE_ROWS * (64 + 2) / 2];
  const NormJob jb = jobs[blockIdx.x];
  const int r = (int)jb.r;
  const int lg = r == 4 ? 2 : r == 8 ? 3 : r == 16 ? 4 : r == 32 ? 5 : r == 64 ? 6 : -1;
  // a row the table builder should never have written touches no memory and reports NaN (uniform over the block)
  const uintptr_t ptrs = (uintptr_t)jb.A | (uintptr_t)jb.B | (uintptr_t)jb.mA | (uintptr_t)jb.mB;
  if (lg < 0 || jb.r != r || !jb.A || !jb.B || (ptrs & 15) || jb.K <= 0 || jb.out <= 0 || ((jb.K | jb.out) & 7) || jb.K > (1L << 24) || jb.out > (1L << 24)) {
    if (!threadIdx.x) { stats[2 * blockIdx.x] = __uint_as_float(0x7FC00000u); stats[2 * blockIdx.x + 1] = 1.f; }
    return;
  }
  if (r <= 16) mn_grams<1, 4>(jb, r, lg, gA, gB, stage);
  else if (r == 32) mn_grams<2, 4>(jb, r, lg, gA, gB, stage);
  else mn_grams<4, 2>(jb, r, lg, gA, gB, stage);
  float part = 0.f;
  for (int e = threadIdx.x; e < r * r; e += 256) part += gA[e] * gB[e];
  const float sum = block_sum(part, red);         // the same bits in every thread: one decision per module
  const float s = __uint_as_float((uint32_t)jb.s_bits);
  const float norm = sqrtf(s * s * sum);
  const bool over = norm > max_norm;              // false for a NaN norm: the module stays as it is
  const float q = over ? sqrtf(max_norm / norm) : 1.f;
  if (!threadIdx.x) { stats[2 * blockIdx.x] = norm; stats[2 * blockIdx.x + 1] = q; }
  if (!over) return;
  mn_scale((bf16_t*)jb.A, jb.mA, (long)r * jb.K, q);
  mn_scale((bf16_t*)jb.B, jb.mB, jb.out * (long)r, q);
}

// ==== DoRA (weight-decomposed LoRA; include/aozora_hip.h az_dora_*) ===================================================================
// ---- norm: n2[o] = sum_k (float(W[o][k]) + s sum_j B[o][j] A[j][k])^2, inv = 1 / sqrt(n2), g = float(m) inv, for every adapted module in
// one launch.  A workgroup owns 64 output rows of one module (16 per wave) and walks K in chunks of 64 columns.  The B A tile of a
// chunk is formed on the MFMA with the contraction over the rank (padded to 32 per k-step by zero fragments): the wave's B rows are
// loaded once (j contiguous), the chunk of A [r][64] is j-strided in memory and goes through LDS transposed, At[column][j] (row stride
// 72 elements: 16-byte aligned fragment reads), shared by the four waves; one buffer, two barriers per chunk.  A lane owns row o0 + li
// and the 4 consecutive columns 16 t + 4 (lane >> 4) + i of each 16-column tile: it adds W (one 8-byte load per tile, the four of a
// chunk issued together: a row's 128 bytes), squares and accumulates in ascending column order; the four lanes of a row are added in
// lane order.  One fixed order, no atomics.
struct DoraJob { const bf16_t* W; const bf16_t* A; const bf16_t* B; bf16_t* m; float* g; float* inv; long r, K, N, s_bits, tile_start, pad; };   // 12 words
constexpr int DN_ROWS = 64, DN_KC = 64, DN_LD = 72;

template <int KS>
__device__ __forceinline__ float dora_row_sumsq(const DoraJob& jb, int r, int lg, long o0, float s, bf16_t* At) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g4 = lane >> 4, kq = g4 * 8;
  const int K = (int)jb.K;
  const long o = o0 + wave * 16 + li;
  const bool ook = o < jb.N;
  bf16x8 bfr[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) bfr[ks] = load_small8(jb.B + (ook ? o : 0) * r, ks * 32 + kq, r, ook);
  const bf16_t* wrow = jb.W + (ook ? o : 0) * K;
  for (int e = tid; e < DN_KC * DN_LD / 8; e += 256) ((bf16x8*)At)[e] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};      // the rank's padding stays zero
  float sq = 0.f;
  for (int k0 = 0; k0 < K; k0 += DN_KC) {
    __syncthreads();                              // the previous chunk's fragments have been read (first pass: the zeros are written)
    for (int c = tid; c < r * 8; c += 256) {      // j fastest: the transposed 2-byte writes of a wave fall on consecutive addresses
      const int j = c & (r - 1), kk = (c >> lg) * 8;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (k0 + kk < K) v = *(const bf16x8*)(jb.A + (long)j * K + k0 + kk);       // K % 8 == 0: an 8-chunk is inside or outside as a whole
#pragma unroll
      for (int e = 0; e < 8; ++e) At[(kk + e) * DN_LD + j] = (bf16_t)v[e];
    }
    __syncthreads();
    bf16x4 w[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k4 = k0 + 16 * t + 4 * g4;
      w[t] = bf16x4{0, 0, 0, 0};
      if (ook && k4 < K) w[t] = *(const bf16x4*)(wrow + k4);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = mfma16(*(const bf16x8*)(At + (16 * t + li) * DN_LD + ks * 32 + kq), bfr[ks], acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float val = __fmaf_rn(s, acc[i], bf2f((bf16_t)w[t][i]));
        sq = __fmaf_rn(val, val, sq);
      }
    }
  }
  const float p0 = __shfl(sq, li, 64), p1 = __shfl(sq, li + 16, 64), p2 = __shfl(sq, li + 32, 64), p3 = __shfl(sq, li + 48, 64);
  return ((p0 + p1) + p2) + p3;
}

__global__ __launch_bounds__(256) void dora_norm_kernel(const DoraJob* __restrict__ jobs, int njobs, int init) {
  __shared__ __attribute__((aligned(16))) bf16_t At[DN_KC * DN_LD];
  const long tg = blockIdx.x;
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile_start <= tg) lo = mid; else hi = mid - 1;
  }
  const DoraJob jb = jobs[lo];
  const long tile = tg - jb.tile_start, o0 = tile * DN_ROWS;
  const int r = (int)jb.r;
  const int lg = r == 4 ? 2 : r == 8 ? 3 : r == 16 ? 4 : r == 32 ? 5 : r == 64 ? 6 : -1;
  const bool out_ok = jb.g && jb.inv && !(((uintptr_t)jb.g | (uintptr_t)jb.inv) & 3) && jb.N > 0 && jb.N <= (1L << 24) && tile >= 0;
  // a row the table builder should never have written (uniform over the block): nothing of W, A, B, m is touched, and where the
  // addresses of its gains and its N can be trusted they report NaN
  const uintptr_t ptrs = (uintptr_t)jb.W | (uintptr_t)jb.A | (uintptr_t)jb.B;
  if (lg < 0 || jb.r != r || !jb.W || !jb.A || !jb.B || !jb.m || (ptrs & 15) || ((uintptr_t)jb.m & 1) || !out_ok || jb.K <= 0 || ((jb.K | jb.N) & 7) ||
      jb.K > (1L << 24)) {
    if (out_ok) {
      const long o = o0 + threadIdx.x;
      if (threadIdx.x < DN_ROWS && o < jb.N) { jb.g[o] = __uint_as_float(0x7FC00000u); jb.inv[o] = __uint_as_float(0x7FC00000u); }
    }
    return;
  }
  if (o0 >= jb.N) return;
  const float s = __uint_as_float((uint32_t)jb.s_bits);
  const float n2 = r <= 32 ? dora_row_sumsq<1>(jb, r, lg, o0, s, At) : dora_row_sumsq<2>(jb, r, lg, o0, s, At);
  const int lane = threadIdx.x & 63;
  const long o = o0 + (threadIdx.x >> 6) * 16 + lane;
  if (lane < 16 && o < jb.N) {
    const float root = sqrtf(n2), inv = 1.f / root;
    bf16_t mm;
    if (init) { mm = f2bf(root); jb.m[o] = mm; } else mm = jb.m[o];
    jb.g[o] = bf2f(mm) * inv;
    jb.inv[o] = inv;
  }
}

// ---- scale: Y[m][o] = bf16(fmaf(g[o], float(V[m][o]), bias[o] or 0) + (float(R[m][o]) or 0)): one thread per 8 columns ----------------
__global__ __launch_bounds__(256) void dora_scale_kernel(long groups, int gpr, const bf16_t* __restrict__ V, long ldv, const float* __restrict__ g,
                                                         const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R, long ldr, bf16_t* __restrict__ Y, long ldy) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= groups) return;
  long row; int c8;
  divmod(i, gpr, row, c8);
  const int col = c8 * 8;
  const bf16x8 v = *(const bf16x8*)(V + row * ldv + col);
  const f32x4 g0 = *(const f32x4*)(g + col), g1 = *(const f32x4*)(g + col + 4);
  bf16x8 b = {0, 0, 0, 0, 0, 0, 0, 0}, rr = {0, 0, 0, 0, 0, 0, 0, 0}, y;
  if (bias) b = *(const bf16x8*)(bias + col);
  if (R) rr = *(const bf16x8*)(R + row * ldr + col);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    float t = __fmaf_rn(l < 4 ? g0[l & 3] : g1[l & 3], bf2f((bf16_t)v[l]), bias ? bf2f((bf16_t)b[l]) : 0.f);
    if (R) t = t + bf2f((bf16_t)rr[l]);
    y[l] = (short)f2bf(t);
  }
  *(bf16x8*)(Y + row * ldy + col) = y;
}

// ---- backward: dV[m][o] = bf16(g[o] float(dY[m][o])) and, with P, the partial column sums P[split][o] = sum over the split's rows of
// float(dY) float(V) (a product of two bf16 is exact in fp32).  A block owns 256 columns (a thread 8 of them) and the rows
// [split rps, min(M, (split + 1) rps)); its 8 row lanes take every 8th row in ascending order and are added in lane order.
__global__ __launch_bounds__(256) void dora_bwd_kernel(int M, int N, int rps, const bf16_t* __restrict__ dY, long lddy, const bf16_t* __restrict__ V, long ldv,
                                                       const float* __restrict__ g, bf16_t* dV, long lddv, float* __restrict__ P) {
  __shared__ float red[8][256];
  const int tid = threadIdx.x, cg = tid & 31, rs = tid >> 5;
  const int col = blockIdx.x * 256 + cg * 8, split = blockIdx.y;
  const long mbeg = (long)split * rps, mend = min((long)M, mbeg + rps);
  const bool cok = col < N;                       // N % 8 == 0: an 8-group is inside or outside as a whole
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (cok) {
    const f32x4 g0 = *(const f32x4*)(g + col), g1 = *(const f32x4*)(g + col + 4);
#pragma unroll
    for (int l = 0; l < 4; ++l) { gg[l] = g0[l]; gg[4 + l] = g1[l]; }
    for (long m = mbeg + rs; m < mend; m += 8) {
      const bf16x8 dy = *(const bf16x8*)(dY + m * lddy + col);
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0}, dv;
      if (P) v = *(const bf16x8*)(V + m * ldv + col);
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        const float d = bf2f((bf16_t)dy[l]);
        dv[l] = (short)f2bf(gg[l] * d);
        acc[l] = __fmaf_rn(d, bf2f((bf16_t)v[l]), acc[l]);
      }
      *(bf16x8*)(dV + m * lddv + col) = dv;
    }
  }
  if (!P) return;                                 // uniform over the grid
#pragma unroll
  for (int l = 0; l < 8; ++l) red[rs][cg * 8 + l] = acc[l];
  __syncthreads();
  const int c = blockIdx.x * 256 + tid;
  if (c >= N) return;
  float sum = red[0][tid];
#pragma unroll
  for (int k = 1; k < 8; ++k) sum += red[k][tid];
  P[(long)split * N + c] = sum;
}

// dm[o] = bf16(fmaf(inv[o], sum_split P[split][o], float(dm[o]))), splits ascending
__global__ __launch_bounds__(256) void dora_bwd_finish_kernel(int N, int nsplit, const float* __restrict__ P, const float* __restrict__ inv, bf16_t* dm) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= N) return;
  float sum = 0.f;
  for (int k = 0; k < nsplit; ++k) sum += P[(long)k * N + o];
  dm[o] = f2bf(__fmaf_rn(inv[o], sum, bf2f(dm[o])));
}

inline bool al(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

// the checks the three az_lora_conv_* entry points share: geometry, channel count, rank; -> B H W or 0
inline long conv_rows(int B, int H, int W, int Cin, int r) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 7) || r < 4 || r > 64 || (r & 3)) return 0;
  const long M = (long)B * H * W;
  return (M > 0x7FFFFFF0L || 9L * Cin > 0x7FFFFFF0L) ? 0 : M;
}

}  // namespace

extern "C" {

int az_lora_down_bf16(int M, int K, int r, int parts, float s, const void* X, long ldx, long x_part_stride, const void* W, long ldw,
                      long w_part_stride, void* out, long ldo, void* stream) {
  if (M <= 0 || K <= 0 || (K & 7) || r < 4 || (r & 3) || parts < 1 || parts > 3 || (long)parts * r > 192) return AZ_ERR_ARG(110);
  if (!X || !W || !out || !al(X, 16) || !al(W, 16) || !al(out, 8)) return AZ_ERR_ARG(111);
  if ((ldx & 7) || (ldw & 7) || (ldo & 3) || (x_part_stride & 7) || (w_part_stride & 7) || x_part_stride < 0 || w_part_stride < 0 ||
      ldx < (parts - 1) * x_part_stride + K || ldw < K || ldo < (long)parts * r)
    return AZ_ERR_ARG(112);
  const dim3 grid((unsigned)((M + 15) / 16), (unsigned)parts), block(256);
  const bf16_t *x = (const bf16_t*)X, *w = (const bf16_t*)W;
  bf16_t* u = (bf16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  if (r <= 16) az_launch(lora_down_kernel<1, 4>, grid, block, 0, st, M, K, r, s, x, ldx, x_part_stride, w, ldw, w_part_stride, u, ldo);
  else if (r <= 32) az_launch(lora_down_kernel<2, 4>, grid, block, 0, st, M, K, r, s, x, ldx, x_part_stride, w, ldw, w_part_stride, u, ldo);
  else if (r <= 64) az_launch(lora_down_kernel<4, 2>, grid, block, 0, st, M, K, r, s, x, ldx, x_part_stride, w, ldw, w_part_stride, u, ldo);
  else az_launch(lora_down_kernel<12, 1>, grid, block, 0, st, M, K, r, s, x, ldx, x_part_stride, w, ldw, w_part_stride, u, ldo);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_up_bf16(int M, int N, int r, int parts, float s, const void* U, long ldu, long u_part_stride, const void* W, long ldw,
                    long w_part_stride, void* Y, long ldy, long y_part_stride, void* stream) {
  if (M <= 0 || N <= 0 || (N & 3) || r < 4 || (r & 3) || r > 192 || parts < 1 || parts > 3) return AZ_ERR_ARG(113);
  if (!U || !W || !Y || !al(U, 8) || !al(W, 8) || !al(Y, 8)) return AZ_ERR_ARG(114);
  if ((ldu & 3) || (ldw & 3) || (ldy & 3) || (u_part_stride & 3) || (w_part_stride & 3) || (y_part_stride & 3) || u_part_stride < 0 ||
      w_part_stride < 0 || y_part_stride < 0 || ldu < (parts - 1) * u_part_stride + r || ldw < r || ldy < (parts - 1) * y_part_stride + N ||
      (parts > 1 && y_part_stride < N))
    return AZ_ERR_ARG(115);
  const long gy = ((long)M + 63) / 64;
  if (gy > 65535) return AZ_ERR_ARG(115);
  const dim3 grid((unsigned)((N + 127) / 128), (unsigned)gy, (unsigned)parts), block(256);
  const bf16_t *u = (const bf16_t*)U, *w = (const bf16_t*)W;
  bf16_t* y = (bf16_t*)Y;
  hipStream_t st = (hipStream_t)stream;
  if (r <= 32) az_launch(lora_up_kernel<1>, grid, block, 0, st, M, N, r, s, u, ldu, u_part_stride, w, ldw, w_part_stride, y, ldy, y_part_stride);
  else if (r <= 64) az_launch(lora_up_kernel<2>, grid, block, 0, st, M, N, r, s, u, ldu, u_part_stride, w, ldw, w_part_stride, y, ldy, y_part_stride);
  else az_launch(lora_up_kernel<6>, grid, block, 0, st, M, N, r, s, u, ldu, u_part_stride, w, ldw, w_part_stride, y, ldy, y_part_stride);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_up_geglu_bf16(int M, int H, int r, float s, const void* U, long ldu, const void* W, long ldw, void* proj, long ldp, void* out,
                          long ldo, void* stream) {
  if (M <= 0) return AZ_ERR_ARG(120);
  if (H <= 0 || (H & 7)) return AZ_ERR_ARG(121);
  if (r < 4 || r > 64 || (r & 3)) return AZ_ERR_ARG(122);
  if (!U || !W || !proj || !out || !al(U, 8) || !al(W, 8) || !al(proj, 8) || !al(out, 8)) return AZ_ERR_ARG(123);
  if ((ldu & 3) || (ldw & 3) || (ldp & 3) || (ldo & 3) || ldu < r || ldw < r || ldp < 2L * H || ldo < H) return AZ_ERR_ARG(124);
  // proj is read and written in place: neither the down product nor the GEGLU output may share a byte with it
  const uintptr_t p0 = (uintptr_t)proj, p1 = p0 + (uintptr_t)(((long)(M - 1) * ldp + 2L * H) * 2);
  const uintptr_t u0 = (uintptr_t)U, u1 = u0 + (uintptr_t)(((long)(M - 1) * ldu + r) * 2);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(((long)(M - 1) * ldo + H) * 2);
  if ((u0 < p1 && p0 < u1) || (o0 < p1 && p0 < o1)) return AZ_ERR_ARG(125);
  const long gy = ((long)M + 63) / 64;
  if (gy > 65535) return AZ_ERR_ARG(126);
  const dim3 grid((unsigned)((H + 63) / 64), (unsigned)gy), block(256);
  const bf16_t *u = (const bf16_t*)U, *w = (const bf16_t*)W;
  bf16_t *p = (bf16_t*)proj, *o = (bf16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  if (r <= 32) az_launch(lora_up_geglu_kernel<1>, grid, block, 0, st, M, H, r, s, u, ldu, w, ldw, p, ldp, o, ldo);
  else az_launch(lora_up_geglu_kernel<2>, grid, block, 0, st, M, H, r, s, u, ldu, w, ldw, p, ldp, o, ldo);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_wgrad_bf16(int M, int ns, int nb, int parts, float s, const void* S, long ld_s, long s_part_stride, const void* G, long ld_g,
                       long g_part_stride, void* out, long out_stride_s, long out_stride_b, long out_part_stride, int accumulate,
                       void* workspace, long workspace_bytes, void* stream) {
  if (M <= 0 || ns < 4 || (ns & 3) || ns > 192 || nb <= 0 || (nb & 7) || parts < 1 || parts > 3) return AZ_ERR_ARG(116);
  if (!S || !G || !out || !workspace || !al(S, 8) || !al(G, 16) || !al(out, 2) || !al(workspace, 4)) return AZ_ERR_ARG(117);
  if ((ld_s & 3) || (ld_g & 7) || (s_part_stride & 3) || (g_part_stride & 7) || s_part_stride < 0 || g_part_stride < 0 ||
      ld_s < (parts - 1) * s_part_stride + ns || ld_g < (parts - 1) * g_part_stride + nb || out_stride_s <= 0 || out_stride_b <= 0 ||
      out_part_stride < 0)
    return AZ_ERR_ARG(118);
  // rows per split: about 512 workgroups in all, at most 64 splits, whole 32-row slices, and partials that fit the workspace
  const long per = (long)parts * ns * nb * 4;
  long cap = workspace_bytes / per;
  if (cap < 1) return AZ_ERR_ARG(119);
  const long base = (((long)nb + 63) / 64) * parts;
  long want = (512 + base - 1) / base;
  if (want > 64) want = 64;
  if (want > cap) want = cap;
  const long slices = ((long)M + 31) / 32;
  if (want > slices) want = slices;
  const long rps = ((slices + want - 1) / want) * 32;
  const int nsplit = (int)(((long)M + rps - 1) / rps);
  const dim3 grid((unsigned)((nb + 63) / 64), (unsigned)nsplit, (unsigned)parts), block(256);
  const bf16_t *sp = (const bf16_t*)S, *gp = (const bf16_t*)G;
  float* P = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (ns <= 16) az_launch(lora_wgrad_partial_kernel<1>, grid, block, 0, st, M, ns, nb, (int)rps, sp, ld_s, s_part_stride, gp, ld_g, g_part_stride, P);
  else if (ns <= 32) az_launch(lora_wgrad_partial_kernel<2>, grid, block, 0, st, M, ns, nb, (int)rps, sp, ld_s, s_part_stride, gp, ld_g, g_part_stride, P);
  else if (ns <= 64) az_launch(lora_wgrad_partial_kernel<4>, grid, block, 0, st, M, ns, nb, (int)rps, sp, ld_s, s_part_stride, gp, ld_g, g_part_stride, P);
  else az_launch(lora_wgrad_partial_kernel<12>, grid, block, 0, st, M, ns, nb, (int)rps, sp, ld_s, s_part_stride, gp, ld_g, g_part_stride, P);
  AZ_CHECK_LAUNCH();
  const long total = (long)parts * ns * nb;
  az_launch(lora_wgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ns, nb, parts, nsplit, s, (const float*)P, (bf16_t*)out,
            out_stride_s, out_stride_b, out_part_stride, accumulate);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_conv_down_bf16(int B, int H, int W, int Cin, int r, float s, const void* X, long ldx, const void* A, void* out, long ldo,
                           void* stream) {
  const long M = conv_rows(B, H, W, Cin, r);
  if (!M) return AZ_ERR_ARG(130);
  if (!X || !A || !out || !al(X, 16) || !al(A, 16) || !al(out, 8)) return AZ_ERR_ARG(131);
  if ((ldx & 7) || (ldo & 3) || ldx < Cin || ldo < r) return AZ_ERR_ARG(132);
  const dim3 grid((unsigned)((M + 15) / 16)), block(256);
  const bf16_t *x = (const bf16_t*)X, *a = (const bf16_t*)A;
  bf16_t* u = (bf16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  if (r <= 16) az_launch(lora_conv_down_kernel<1, 4>, grid, block, 0, st, (int)M, H, W, Cin, r, s, x, ldx, a, u, ldo);
  else if (r <= 32) az_launch(lora_conv_down_kernel<2, 4>, grid, block, 0, st, (int)M, H, W, Cin, r, s, x, ldx, a, u, ldo);
  else az_launch(lora_conv_down_kernel<4, 2>, grid, block, 0, st, (int)M, H, W, Cin, r, s, x, ldx, a, u, ldo);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_conv_dgrad_bf16(int B, int H, int W, int Cin, int r, float s, const void* dU, long ldu, const void* At, void* dX, long ldx,
                            void* stream) {
  const long M = conv_rows(B, H, W, Cin, r);
  if (!M) return AZ_ERR_ARG(133);
  if (!dU || !At || !dX || !al(dU, 8) || !al(At, 8) || !al(dX, 8)) return AZ_ERR_ARG(134);
  if ((ldu & 3) || (ldx & 3) || ldu < r || ldx < Cin) return AZ_ERR_ARG(135);
  // dX is read and written in place while neighbouring rows of dU are gathered: the two may not share a byte
  const uintptr_t x0 = (uintptr_t)dX, x1 = x0 + (uintptr_t)(((M - 1) * ldx + Cin) * 2);
  const uintptr_t u0 = (uintptr_t)dU, u1 = u0 + (uintptr_t)(((M - 1) * ldu + r) * 2);
  if (u0 < x1 && x0 < u1) return AZ_ERR_ARG(135);
  const long gy = (M + 63) / 64;
  if (gy > 65535) return AZ_ERR_ARG(133);
  const dim3 grid((unsigned)((Cin + 127) / 128), (unsigned)gy), block(256);
  const bf16_t *du = (const bf16_t*)dU, *at = (const bf16_t*)At;
  bf16_t* dx = (bf16_t*)dX;
  hipStream_t st = (hipStream_t)stream;
  if (r <= 32) az_launch(lora_conv_dgrad_kernel<1>, grid, block, 0, st, (int)M, H, W, Cin, r, s, du, ldu, at, dx, ldx);
  else az_launch(lora_conv_dgrad_kernel<2>, grid, block, 0, st, (int)M, H, W, Cin, r, s, du, ldu, at, dx, ldx);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_conv_wgrad_bf16(int B, int H, int W, int Cin, int r, float s, const void* dU, long ldu, const void* X, long ldx, void* dA,
                            int accumulate, void* workspace, long workspace_bytes, void* stream) {
  const long M = conv_rows(B, H, W, Cin, r);
  if (!M) return AZ_ERR_ARG(136);
  if (!dU || !X || !dA || !workspace || !al(dU, 8) || !al(X, 16) || !al(dA, 2) || !al(workspace, 4)) return AZ_ERR_ARG(137);
  if ((ldu & 3) || (ldx & 7) || ldu < r || ldx < Cin) return AZ_ERR_ARG(138);
  // rows per split: the rule of az_lora_wgrad_bf16 with nb = 9 Cin gathered columns
  const long nb = 9L * Cin, per = (long)r * nb * 4;
  long cap = workspace_bytes / per;
  if (cap < 1) return AZ_ERR_ARG(139);
  const long base = (nb + 63) / 64;
  long want = (512 + base - 1) / base;
  if (want > 64) want = 64;
  if (want > cap) want = cap;
  const long slices = (M + 31) / 32;
  if (want > slices) want = slices;
  const long rps = ((slices + want - 1) / want) * 32;
  const int nsplit = (int)((M + rps - 1) / rps);
  const dim3 grid((unsigned)base, (unsigned)nsplit), block(256);
  const bf16_t *sp = (const bf16_t*)dU, *xp = (const bf16_t*)X;
  float* P = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (r <= 16) az_launch(lora_conv_wgrad_partial_kernel<1>, grid, block, 0, st, (int)M, H, W, Cin, r, (int)rps, sp, ldu, xp, ldx, P);
  else if (r <= 32) az_launch(lora_conv_wgrad_partial_kernel<2>, grid, block, 0, st, (int)M, H, W, Cin, r, (int)rps, sp, ldu, xp, ldx, P);
  else az_launch(lora_conv_wgrad_partial_kernel<4>, grid, block, 0, st, (int)M, H, W, Cin, r, (int)rps, sp, ldu, xp, ldx, P);
  AZ_CHECK_LAUNCH();
  const long total = (long)r * nb;
  az_launch(lora_wgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, r, (int)nb, 1, nsplit, s, (const float*)P, (bf16_t*)dA,
            nb, 1L, 0L, accumulate);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_dropout_bf16(int rows, int r, int parts, int rows_per_sample, void* U, long ldu, int mid0, int mid1, int mid2, int t_net,
                         int t_rank, int t_mod, float inv, long seed, const void* step_word, void* stream) {
  if (parts < 1 || parts > 3) return AZ_ERR_ARG(140);
  if (r != 4 && r != 8 && r != 16 && r != 32 && r != 64) return AZ_ERR_ARG(141);
  // row r + j stays below the module id's bit 35 (rows < 2^29 at rank 64)
  if (rows <= 0 || rows_per_sample <= 0 || rows % rows_per_sample || (long)rows * r > (1L << 35)) return AZ_ERR_ARG(142);
  if (ldu < (long)parts * r) return AZ_ERR_ARG(143);
  if (t_net < 0 || t_net > 65535 || t_rank < 0 || t_rank > 65535 || t_mod < 0 || t_mod > 65535) return AZ_ERR_ARG(144);
  if (!step_word || !al(step_word, 4) || !U || !al(U, 2)) return AZ_ERR_ARG(145);
  const int mids[3] = {mid0, mid1, mid2};
  for (int p = 0; p < parts; ++p)
    if (mids[p] < 0 || mids[p] >= (1 << 27)) return AZ_ERR_ARG(146);
  if (!(t_net | t_rank | t_mod)) return AZ_OK;      // every kind off: nothing to draw, nothing to write, no launch
  DropArgs a;
  a.k0 = (uint32_t)((unsigned long)seed & 0xFFFFFFFFul); a.k1 = (uint32_t)((unsigned long)seed >> 32);
  a.mid[0] = mid0; a.mid[1] = parts > 1 ? mid1 : 0; a.mid[2] = parts > 2 ? mid2 : 0;
  a.t_net = (uint32_t)t_net; a.t_rank = (uint32_t)t_rank; a.t_mod = (uint32_t)t_mod; a.inv = inv;
  const int width = parts * r;
  bf16_t* u = (bf16_t*)U;
  const uint32_t* sw = (const uint32_t*)step_word;
  hipStream_t st = (hipStream_t)stream;
  if ((r & 7) == 0 && (ldu & 7) == 0 && al(U, 16)) {
    const long groups = (long)rows * (width / 8);
    az_launch(lora_dropout_vec_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, groups, r, width / 8, rows_per_sample, u, ldu, a, sw);
  } else {
    const long n = (long)rows * width;
    az_launch(lora_dropout_elem_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, r, width, rows_per_sample, u, ldu, a, sw);
  }
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_lora_max_norm_bf16(const void* jobs_dev, int n_modules, float max_norm, void* stats, void* stream) {
  if (!jobs_dev || ((uintptr_t)jobs_dev & 7)) return AZ_ERR_ARG(150);
  if (n_modules <= 0 || n_modules > 65535) return AZ_ERR_ARG(151);
  if (!(max_norm > 0.f) || !(max_norm <= 3.402823466e38f)) return AZ_ERR_ARG(152);      // NaN fails the first, inf the second
  if (!stats || ((uintptr_t)stats & 7)) return AZ_ERR_ARG(153);
  az_launch(lora_max_norm_kernel, dim3((unsigned)n_modules), dim3(256), 0, (hipStream_t)stream, (const NormJob*)jobs_dev, max_norm, (float*)stats);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_dora_norm_bf16(const void* jobs_dev, int n_modules, long tiles, int init, void* stream) {
  if (!jobs_dev || ((uintptr_t)jobs_dev & 7)) return AZ_ERR_ARG(160);
  if (n_modules <= 0 || n_modules > 65535) return AZ_ERR_ARG(161);
  if (tiles <= 0 || tiles > 0x7FFFFFF0L) return AZ_ERR_ARG(162);
  if (init != 0 && init != 1) return AZ_ERR_ARG(163);
  az_launch(dora_norm_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const DoraJob*)jobs_dev, n_modules, init);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_dora_scale_bf16(int M, int N, const void* V, long ldv, const void* g, const void* bias, const void* residual, long ldr, void* Y, long ldy,
                       void* stream) {
  if (M <= 0 || N <= 0 || (N & 7)) return AZ_ERR_ARG(164);
  if (!V || !g || !Y || !al(V, 16) || !al(g, 16) || !al(Y, 16) || !al(bias, 16) || !al(residual, 16)) return AZ_ERR_ARG(165);
  if ((ldv & 7) || (ldy & 7) || ldv < N || ldy < N || (residual && ((ldr & 7) || ldr < N))) return AZ_ERR_ARG(166);
  const long groups = (long)M * (N / 8);
  if ((groups + 255) / 256 > 0x7FFFFFF0L) return AZ_ERR_ARG(167);
  az_launch(dora_scale_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, groups, N / 8, (const bf16_t*)V, ldv, (const float*)g,
            (const bf16_t*)bias, (const bf16_t*)residual, ldr, (bf16_t*)Y, ldy);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int az_dora_bwd_bf16(int M, int N, const void* dY, long lddy, const void* V, long ldv, const void* g, const void* inv, void* dV, long lddv,
                     void* dm, void* workspace, long workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0 || (N & 7)) return AZ_ERR_ARG(168);
  if (!dY || !g || !dV || !al(dY, 16) || !al(g, 16) || !al(dV, 16)) return AZ_ERR_ARG(169);
  if (dm && (!V || !inv || !workspace || !al(V, 16) || !al(inv, 4) || !al(dm, 2) || !al(workspace, 4))) return AZ_ERR_ARG(169);
  if ((lddy & 7) || (lddv & 7) || lddy < N || lddv < N || (dm && ((ldv & 7) || ldv < N))) return AZ_ERR_ARG(170);
  // rows per split: about 1024 workgroups in all, at most 64 splits, whole groups of 8 rows, and partials that fit the workspace
  const long cb = ((long)N + 255) / 256;
  long want = (1024 + cb - 1) / cb;
  if (want > 64) want = 64;
  if (dm) {
    const long cap = workspace_bytes / ((long)N * 4);
    if (cap < 1) return AZ_ERR_ARG(171);
    if (want > cap) want = cap;
  }
  const long slices = ((long)M + 7) / 8;
  if (want > slices) want = slices;
  const long rps = ((slices + want - 1) / want) * 8;
  const int nsplit = (int)(((long)M + rps - 1) / rps);
  hipStream_t st = (hipStream_t)stream;
  float* P = dm ? (float*)workspace : nullptr;
  az_launch(dora_bwd_kernel, dim3((unsigned)cb, (unsigned)nsplit), dim3(256), 0, st, M, N, (int)rps, (const bf16_t*)dY, lddy, (const bf16_t*)V, ldv,
            (const float*)g, (bf16_t*)dV, lddv, P);
  AZ_CHECK_LAUNCH();
  if (dm) {
    az_launch(dora_bwd_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, nsplit, (const float*)P, (const float*)inv, (bf16_t*)dm);
    AZ_CHECK_LAUNCH();
  }
  return AZ_OK;
}

}  // extern "C"
