// Strip-staged 3x3 convolution weight gradient (option CONVWG_STRIP; included by az_gemm.hip, which documents Params and the
// DMA helpers):  dW[co][(tap, ci)] = sum over pixels  dY[pixel][co] * X[pixel + tap displacement][ci].
//
// gemm_kernel<A_COL, B_CONVWG> stages the B operand as [64 pixels][128 columns of (tap, ci)]: the nine column tiles of one channel
// range pull the SAME pixels of X from L2 into LDS nine times, once per tap.  For a stride-1, pad-1 filter on same-size grids the nine
// B images of a k-tile are ONE image of X read at nine pixel offsets, so this kernel stages that image once:
//
//   tile      128 output channels x (9 taps x 32 input channels) x 64 pixels (the host k-tile: 64 consecutive output pixels)
//   waves     8 = 4 (16 output channels of each of the MI = 2 blocks of 64) x 2 (16 input channels x 9 taps each): 2 x 9 accumulators of 16 x 16
//   A image   dY  two blocks of [64 pixels][64 co], 128-byte rows, 8 KiB each (one DMA piece per wave and block)
//   B image   X   [strip pixel][32 ci], 64 bytes per pixel: the k-tile's rows plus one row above and below, each with one pad
//             pixel left and right (3 x 66 pixels for W >= 64, 4 x 34 for W = 32); positions outside the image are zeros (out-of-range DMA)
//   bytes     16 KiB + <= 12.4 KiB per 64-deep step for 2.25 x the products of the 128 x 128 tile's 32 KiB; 11 fragment reads per 18 MFMAs
//             (gemm_kernel: 6 per 8).  Measured in isolation (profiles/LEDGER.md): the 64-row form of the same kernel (MI = 1: 20.4 KiB,
//             10 reads per 9 MFMAs) was the slower one on 11 of 13 shapes and lost 4 % to gemm_kernel where the grid is not split
//
// The k-tile must be whole rows or an aligned part of one row and must not straddle samples: W % 64 == 0 or 64 % W == 0, and
// H * W % 64 == 0 (the host checks; everything else stays on gemm_kernel).  Strip<LW> is the geometry for min(W, 64) = 2^LW pixels
// of a row per k-tile.  A tap is a displacement of the strip pixel index, so every tap, both 32-deep halves and both stages are
// IMMEDIATE offsets from six per-lane addresses (two reads x three column displacements).
//
// Banks (ds_read_b64_tr_b16 counts conflicts per 32-lane half: lane groups g = 0, 1 read strip pixels s .. s + 3 and s + 8 .. s + 11 of
// one strip row, 32 bytes of each): the 32-byte halves of a pixel are exchanged when bit 3 of its strip COLUMN is set -- the row
// displacement of a tap leaves the column alone -- so the two groups cover the 256-byte bank row once (for W >= 16; narrower grids,
// which the model does not have, read two-way conflicted).  The A image exchanges the 32-byte units of row k by
// ((k >> 1) & 1) + 2 ((k >> 3) & 1) for the same reason (two 128-byte rows per bank row).
//
// Arithmetic is gemm_kernel's: v_mfma_f32_16x16x32_bf16 with swapped operands, the same two 32-deep halves of the same 64-pixel
// k-tiles in the same order, so at equal split_k every output element sums the same products in the same order.  Split-K slabs,
// XCD dealing of the splits, accumulate, streamed C stores and the fused column sums of dY are as there; the in-kernel finish
// (INKERNEL_FINISH) is not implemented here -- the host leaves the finish to the separate launches, which give the same bits.

constexpr int SCI = 32, SMI = 2, SBM = 64 * SMI;        // input channels of a tile; 64-row blocks and output channels of a tile

template <int LW> struct Strip {
  static constexpr int WT = 1 << LW;                 // pixels of one row inside a k-tile
  static constexpr int ROWS = 64 >> LW;              // rows of a k-tile
  static constexpr int SWP = WT + 2;                 // strip row pitch in pixels: 66, 34, 18, 10
  static constexpr int NPIX = (ROWS + 2) * SWP;      // 198, 136, 108, 100
  static constexpr int NPB = (NPIX + 15) / 16;       // 1-KiB DMA pieces of the B image: 13, 9, 7, 7
  static constexpr int KK_OFF = (LW == 6 ? 32 : (32 >> LW) * SWP) * 64;      // byte displacement of the second 32-pixel half
  static constexpr int B_BYTES = NPB * 1024;
};

// dma16 with the scalar offset as the literal 0 (no SGPR to hold it)
__device__ __forceinline__ void dma16z(u32x4 r, unsigned voff, unsigned dst_wave_uniform) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" :: "s"(dst_wave_uniform), "v"(voff), "s"(r) : "memory");
}

__device__ __forceinline__ bf16x8 tr_frag(const char* lo_p, const char* hi_p) {
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(lo_p));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(hi_p));
  bf16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return v;
}

template <int LW>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void convwg_strip_kernel(const Params p) {      // <= 128 registers: two workgroups per CU
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using S = Strip<LW>;
  constexpr int MI = SMI, BM = SBM, A_BYTES = BM * BK * 2, STAGE = A_BYTES + S::B_BYTES, SWP = S::SWP;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // tile and split of this workgroup: gemm_kernel's dealing (splits to the XCDs, or tiles to the XCDs) and grouped raster
  const int nwg = p.tiles_m * p.tiles_n;
  int id = blockIdx.x, z = blockIdx.y;
  if (p.xsplit) {
    const int W = nwg * p.ksplit, L = blockIdx.x, xcd = L & 7;
    const int q = W >> 3, r = W & 7;
    const int idx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    z = idx / nwg; id = idx - z * nwg;
  } else {
    const int q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  constexpr int GROUP = 8;
  const int per_group = GROUP * p.tiles_n;
  const int grp = id / per_group;
  const int first_m = grp * GROUP;
  const int gsize = (p.tiles_m - first_m) < GROUP ? (p.tiles_m - first_m) : GROUP;
  const int in_grp = id - grp * per_group;
  const int tn = in_grp / gsize;
  const int tm = first_m + (in_grp - tn * gsize);
  const int m0 = tm * BM, c0 = tn * SCI;
  const int kt_begin = z * p.ktiles_per_split;
  int kt_end = kt_begin + p.ktiles_per_split;
  if (kt_end > p.K / BK) kt_end = p.K / BK;
  const int nk = kt_end > kt_begin ? kt_end - kt_begin : 0;

  const u32x4 rsA = make_rsrc_words(p.A), rsB = make_rsrc_words(p.B);
  const unsigned smem_lds = lds_addr(smem);
  const int Wi = p.g.Win, Hi = p.g.Hin;

  // A: wave w fetches k-rows 8w .. 8w + 7 of every 64-row block; lane -> row 8w + (l >> 3), 16-byte position l & 7 of the swizzled 128-byte row
  unsigned a_base[MI];
  {
    const int krow = 8 * wave + (lane >> 3), pos = lane & 7;
    const int f = ((krow >> 1) & 1) | (((krow >> 3) & 1) << 1);
#pragma unroll
    for (int b = 0; b < MI; ++b) {
      const int m = m0 + 64 * b + (((pos >> 1) ^ f) << 4) + ((pos & 1) << 3);
      a_base[b] = m < p.M ? (unsigned)m * 2u + (unsigned)krow * (unsigned)p.lda2 : OOB;
    }
  }
  // B: wave w fetches pieces w and w + 8; lane -> strip pixel 16 q + (l >> 2), 16-byte position l & 3.  b_rel: byte offset of the lane's
  // chunk from the k-tile's first pixel (negative in the row above / the left pad); b_cls: what the slot is -- bit 0 the row above the
  // k-tile, bit 1 the row below, bit 2 the left pad column, bit 3 the right one, bit 4 a slot behind the strip -- tested per k-tile
  // against the wave-uniform set of classes that lie outside the image
  constexpr int NPW = (S::NPB + 7) / 8;
  int b_rel[NPW], b_cls[NPW];
#pragma unroll
  for (int j = 0; j < NPW; ++j) {
    const int s = 16 * (wave + 8 * j) + (lane >> 2);
    const int sr = s / SWP, sx = s - sr * SWP;
    const int c = (lane & 3) ^ (((sx >> 3) & 1) << 1);
    b_rel[j] = ((sr - 1) * Wi + (sx - 1)) * p.ldb2 + (c0 + 8 * c) * 2;
    b_cls[j] = (sr == 0 ? 1 : 0) | (sr == S::ROWS + 1 ? 2 : 0) | (sx == 0 ? 4 : 0) | (sx == S::WT + 1 ? 8 : 0) | (s >= S::NPIX ? 16 : 0);
  }
  auto issue = [&](int kt, int buf) {
    const int k0 = kt * BK;
    const unsigned ka = (unsigned)__builtin_amdgcn_readfirstlane(k0 * p.lda2);
#pragma unroll
    for (int b = 0; b < MI; ++b) dma16s(rsA, a_base[b], ka, smem_lds + (unsigned)(buf * STAGE + b * 8192 + wave * 1024));
    const unsigned q1 = __umulhi((unsigned)k0, p.magic_w);      // row over all samples (exact: the host checks K * W < 2^32)
    const int x0 = k0 - (int)q1 * Wi;
    const unsigned q2 = __umulhi(q1, p.magic_h);
    const int y0 = (int)q1 - (int)q2 * Hi;
    const unsigned kb = (unsigned)k0 * (unsigned)p.ldb2;
    const int outside = (y0 == 0 ? 1 : 0) | (y0 + S::ROWS == Hi ? 2 : 0) | (x0 == 0 ? 4 : 0) | (x0 + S::WT == Wi ? 8 : 0) | 16;
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      const int q = wave + 8 * j;
      if (q >= S::NPB) continue;                                  // (wave-uniform)
      dma16z(rsB, (b_cls[j] & outside) == 0 ? kb + (unsigned)b_rel[j] : OOB, smem_lds + (unsigned)(buf * STAGE + A_BYTES + q * 1024));
    }
  };

  // fragment addresses (stage 0, first half, block 0, top row of taps): everything else is an immediate
  const int g = lane >> 4, i = lane & 15;
  const char* pa = smem + (8 * g + (i >> 2)) * 128 + ((wm ^ (((i >> 3) & 1) | ((g & 1) << 1))) << 5) + (i & 3) * 8;
  const char* pb[3][2];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int px = 8 * g + (i >> 2) + 4 * rd;
      const int sx = (px & (S::WT - 1)) + kx;
      pb[kx][rd] = smem + A_BYTES + ((px >> LW) * SWP + sx) * 64 + ((wn ^ ((sx >> 3) & 1)) << 5) + (i & 3) * 8;
    }

  f32x4 acc[MI][9];
  f32x4 accs[MI];
#pragma unroll
  for (int b = 0; b < MI; ++b) {
    accs[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[b][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bool cs_on = p.cs_ws != nullptr && tn == 0 && wn == 0;      // column sums of dY: one more MFMA per A fragment (see gemm_kernel)
  const bf16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  // LDS-DMA double buffer as in gemm_kernel (NS == 2); the two buffers are the two unrolled halves of the loop
  if (nk > 0) issue(kt_begin, 0);
  wait_dma();
  __syncthreads();
  auto step = [&](int it, auto cur_c) {
    constexpr int CUR = decltype(cur_c)::value;
    if (it + 1 < nk) issue(kt_begin + it + 1, CUR ^ 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fa[MI];
#pragma unroll
      for (int b = 0; b < MI; ++b) fa[b] = tr_frag(pa + CUR * STAGE + b * 8192 + kk * 4096, pa + CUR * STAGE + b * 8192 + kk * 4096 + 512);
      // one row of taps at a time: with 72 accumulator registers there is no room for all nine B fragments
      constexpr int TB = 3;
#pragma unroll
      for (int j0 = 0; j0 < 9; j0 += TB) {
        bf16x8 fb[TB];
#pragma unroll
        for (int jj = 0; jj < TB; ++jj) {
          const int j = j0 + jj;
          const int off = CUR * STAGE + kk * S::KK_OFF + (j / 3) * SWP * 64;
          fb[jj] = tr_frag(pb[j % 3][0] + off, pb[j % 3][1] + off);
        }
#pragma unroll
        for (int b = 0; b < MI; ++b)
#pragma unroll
          for (int jj = 0; jj < TB; ++jj) acc[b][j0 + jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[jj], fa[b], acc[b][j0 + jj], 0, 0, 0);
      }
      if (cs_on) {
#pragma unroll
        for (int b = 0; b < MI; ++b) accs[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, fa[b], accs[b], 0, 0, 0);
      }
    }
    if (cs_on) {      // flush at the end of a k-segment (= one sample's pixels) and at the end of this split's range
      const int kb = (kt_begin + it) * BK;
      const int seg = kb / p.cs_rps;
      if (it + 1 == nk || (kb + BK) / p.cs_rps != seg) {
        if ((lane >> 4) == 0) {
#pragma unroll
          for (int b = 0; b < MI; ++b) {
            const int m = m0 + 64 * b + wm * 16 + (lane & 15);
            if (m < p.M) p.cs_ws[((long)z * p.cs_nseg + seg) * p.M + m] = accs[b][0];
          }
        }
#pragma unroll
        for (int b = 0; b < MI; ++b) accs[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    wait_dma();
    __syncthreads();
  };
  for (int it = 0; it < nk; it += 2) {
    step(it, std::integral_constant<int, 0>{});
    if (it + 1 < nk) step(it + 1, std::integral_constant<int, 1>{});
  }

  // ---- epilogue: three taps per pass through the wave's LDS window, 16-byte pieces of full rows out ----------------------
  constexpr int EP = 3 * 16 * 4 + 16;       // window pitch: 48 fp32 + one 16-byte unit
  static_assert(16 * EP * 8 <= 2 * STAGE, "epilogue window exceeds the LDS allocation");
  char* win = smem + wave * (16 * EP);
  const int lm = lane & 15;
#pragma unroll
  for (int b = 0; b < MI; ++b)
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      const f32x4 a = acc[b][3 * pass + jj];
      *reinterpret_cast<float4*>(win + lm * EP + ((4 * jj + (lane >> 4)) << 4)) = make_float4(a[0], a[1], a[2], a[3]);
    }
#pragma unroll
    for (int q0 = 0; q0 < 96; q0 += 64) {
      const int q = q0 + lane;
      if (q >= 96) break;
      const int r = q / 6, cc = q - r * 6;
      const int m = m0 + 64 * b + wm * 16 + r;
      const int n = (3 * pass + (cc >> 1)) * p.g.Cin + c0 + wn * 16 + (cc & 1) * 8;
      const float4 lo = *reinterpret_cast<const float4*>(win + r * EP + ((2 * cc) << 4));
      const float4 hi = *reinterpret_cast<const float4*>(win + r * EP + ((2 * cc + 1) << 4));
      if (m >= p.M) continue;
      if (p.ksplit > 1) {
        float* dst = p.ws + ((long)z * p.M + m) * p.N + n;
        *reinterpret_cast<float4*>(dst) = lo;
        *reinterpret_cast<float4*>(dst + 4) = hi;
        continue;
      }
      float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      bf16_t* cp = p.C + (long)m * p.ldc + n;
      if (p.accumulate) {
        const uint4 u = ld_stream16(cp);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&u);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[2 * e] += __uint_as_float(w[e] << 16); v[2 * e + 1] += __uint_as_float(w[e] & 0xFFFF0000u); }
      }
      uint4 o;
      o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]); o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
      st_stream16(cp, o);
    }
  }
}

// The strip form covers a 3x3 weight gradient when: the fast gather's conditions hold (stride 1, same-size grids, no upsample), pad 1,
// Cin % 32 == 0, Cout >= 64 (conv_out's 4 channels stay where they were), 8 <= W with W % 64 == 0 or 64 % W == 0, H * W % 64 == 0,
// and dW and the slabs are 16-byte aligned.
bool strip_applies(const Params& p, const void* workspace) {
  const Geom& g = p.g;
  return p.conv_fast_b && g.ks == 3 && g.pad == 1 && (g.Cin % SCI) == 0 && g.Cout >= 64 && g.Win >= 8 && ((g.Win % 64) == 0 || (64 % g.Win) == 0) &&
         ((g.Hin * g.Win) % 64) == 0 && (p.ldc & 7) == 0 && ((uintptr_t)p.C & 15) == 0 && ((uintptr_t)workspace & 15) == 0;
}

template <int LW>
int launch_strip_lw(const Params& p, hipStream_t st) {
  constexpr int LDS = 2 * (SBM * BK * 2 + Strip<LW>::B_BYTES);
  static_assert(LDS <= 65536, "two workgroups and the other stream's kernels share a CU's LDS");
  dim3 grid(p.tiles_m * p.tiles_n, p.ksplit, 1);
  if (p.xsplit) grid = dim3(p.tiles_m * p.tiles_n * p.ksplit, 1, 1);
  az_launch(convwg_strip_kernel<LW>, grid, dim3(512), LDS, st, p);
  AZ_CHECK_LAUNCH();
  return AZ_OK;
}

int launch_strip(Params& p, hipStream_t st) {
  const long GB2 = 0x7FFFFFF0L;      // 32-bit buffer offsets, as launch()
  const long ext_a = ((long)p.K * p.lda + p.M + 8) * 2, ext_b = (long)p.K * p.ldb * 2;
  if (ext_a >= GB2 || ext_b >= GB2) return AZ_ERR_ARG(8);
  p.lda2 = (int)(p.lda * 2); p.ldb2 = (int)(p.ldb * 2);
  p.k_full = 1; p.vec_epi = 1;
  const int wt = p.g.Win >= 64 ? 64 : p.g.Win;
  if (wt == 64) return launch_strip_lw<6>(p, st);
  if (wt == 32) return launch_strip_lw<5>(p, st);
  if (wt == 16) return launch_strip_lw<4>(p, st);
  return launch_strip_lw<3>(p, st);
}
