/* aozora_hip.h -- C ABI of libaozora_hip.so (MI355X / gfx950).
 *
 * The reference (Hysocs/Aozora_SDXL_Training) is pure Python and has no FFI; every native
 * instruction on its hot path comes from PyTorch/ATen through diffusers.  This library is the
 * native layer a maintainer would bind (ctypes stub: INTEGRATION.md) to replace those calls for
 * the SDXL-UNet training step.  Each entry point cites the reference call it stands in for.
 *
 * Conventions: every pointer is a DEVICE pointer unless its name ends in `_host`
 * (pinned host memory).  Memory is caller-owned.  `stream` is a hipStream_t passed as void*.
 * bf16 tensors are raw uint16 bits.  Activations are NHWC: row-major [pixels][channels] with a
 * leading dimension (elements) per row.  Conv weights are [Cout][ky][kx][Cin] (the memory of a
 * torch (Cout,Cin,kh,kw) tensor in channels_last format).  Every function returns 0 on success,
 * -(hipError_t) for a HIP failure, or -1000-k for argument error k; nothing throws or prints.
 * All launches are asynchronous on `stream` and graph-capturable (no allocation, no sync).
 */
#ifndef AOZORA_HIP_H
#define AOZORA_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ----------------------------------------------------------------------------- */
int az_version(void);
/* device properties of the current device: out[0]=CU count, out[1]=is_gfx950, out[2]=LDS/CU bytes */
int az_device_info(int* out3);
/* hipGraph capture of everything launched on `stream` between begin/end (thread-local capture) */
int az_graph_begin(void* stream);
int az_graph_end(void* stream, void** graph_exec_out);
int az_graph_launch(void* graph_exec, void* stream);
int az_graph_destroy(void* graph_exec);
/* pinned host memory for Raven/Titan state (raven.py:83-84 allocates pageable; we pin) */
int az_host_alloc(void** ptr_host, long bytes);
int az_host_free(void* ptr_host);
/* HIP events on an explicit stream (bench.py times kernels on the stream they run on) */
int az_event_create(void** ev);
int az_event_record(void* ev, void* stream);
int az_event_sync(void* ev);
int az_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
int az_event_destroy(void* ev);
/* fork / join events of the two-stream executor (the reference has one stream and no such events): created with
 * hipEventDisableTiming | hipEventDisableSystemFence -- they order kernels of one device only, and without the system-scope fence a
 * record costs the recording stream about half (tools/event_cost.cpp).  az_event_record / az_event_destroy serve both kinds. */
int az_event_create_fork(void** ev);
int az_stream_wait_event(void* stream, void* ev);
/* While set (per thread; NULL clears), every kernel this thread launches through the library carries `ev` as its own completion
 * signal (hipExtLaunchKernel's stop event): az_set_launch_stop_event(ev); az_xxx(..., stream); az_set_launch_stop_event(NULL) leaves
 * `ev` in the state az_event_record(ev, stream) behind az_xxx would, without the record packet on `stream`.  Used by the launch
 * tape's peephole (tape.fuse_records) for the executor's forks. */
int az_set_launch_stop_event(void* ev);
int az_stream_sync(void* stream);
/* one idle wave for `microseconds` (<= 100 000) on `stream`: concurrency probe for the executor's stream choice (HIP streams
 * share a few hardware queues; the data-gradient chain, the weight-gradient branch and the exchange stream must not) */
int az_spin(long microseconds, void* stream);
int az_memset_async(void* ptr, int value, long bytes, void* stream);
/* kind: 0 default, 1 H2D, 2 D2H, 3 D2D */
int az_memcpy_async(void* dst, const void* src, long bytes, int kind, void* stream);

/* ---- dense contractions (torch.nn.functional.linear / conv2d and their autograd backward as
 *      executed inside diffusers' UNet, train.py:2760-2761 fwd, 2765 bwd) ------------------------ */
/* C[M,N] (+)= op(A) . op(B) (+bias[n]) (+rowbias[m / rows_per_seg][n]) (+residual[m][n])
 *   transA=0: A[m*lda+k]   transA=1: A[k*lda+m]
 *   transB=1: B[n*ldb+k]   transB=0: B[k*ldb+n]        (transA=1,transB=1 unsupported)
 *   linear fwd  : transA=0, transB=1  (B = weight[out][in])
 *   linear dgrad: transA=0, transB=0  (A = dY, B = weight)
 *   linear wgrad: transA=1, transB=0  (A = dY, B = X ; M=out, N=in, K=rows)
 * split_k: 1 = none, 0 = auto, >1 = forced (needs fp32 workspace of split*M*N*4 bytes).
 * K, lda, ldb multiples of 8; A, B 16-byte aligned. */
/* tuning hook: force the cooperative tile (128|256 x 128|256) of the GEMM/conv core; (0,0) = heuristic */
int az_gemm_set_tile(int bm, int bn);
/* the same with the 128x160 tile (k-contiguous B only; waves = 4: 64x80 per wave, 8: 32x80 per wave, 0: default) */
int az_gemm_set_tile_ex(int bm, int bn, int waves);
/* scheduling hint from the executor: 1 while no other stream has work that wants to share the CUs' LDS (the forward
 * pass) -- products on <= 256-tile grids then use the 3-stage / 108-KiB variant; 0 during the backward pass, where the
 * weight-gradient stream's workgroups must stay co-resident */
int az_gemm_set_exclusive(int on);
/* Runtime options: one process-wide table of integer knobs read by the launchers at launch time (tile policy, split-K
 * heuristics, LDS exclusivity ...; names and defaults: csrc/az_common.h AzOption / csrc/az_runtime.hip).  Each knob is an atomic --
 * setting one from any thread between launches is safe -- and starts from the environment variable AZ_<NAME> when that is set.
 * Options steer speed only: every setting computes the same mathematical result (split-K changes the fp32 summation order).
 * Unknown name: -1092.  The library keeps no other mutable state besides the contexts below and the forced tile of az_gemm_set_tile_ex (a test hook). */
/* ref: none (execution policy of this library; the reference has no counterpart) */
int az_set_option(const char* name, int value);
int az_get_option(const char* name, int* value);
/* Per-device / per-owner state (SURVEY.md section 8b `az_init(device, *handle)`): a context carries its OWN copy of the option
 * table (initialised from the process-wide one).  az_make_current(handle) binds it to the CALLING THREAD: every launcher called
 * from that thread, and az_set_option / az_get_option, then use the context's table; az_make_current(NULL) returns the thread to
 * the process-wide table.  The context holds no device memory and makes no HIP call (the caller selects the device: one process
 * -- or one thread -- per GPU); az_context_device returns the device it was created for.  az_destroy drops the owner's reference
 * (and unbinds the context from the calling thread if current); a thread that still has it current keeps its table alive until
 * that thread makes something else current or exits, so a handle destroyed on one thread never dangles on another.  SCOPE of
 * az_set_option: the calling thread's current context when it has one, else the process-wide table -- a context created later
 * copies the process-wide table, not another context's.  Errors: -1093 for a NULL handle / negative device. */
/* ref: train.py:2551 (`device = cuda if available else cpu`: the reference's one device per process) */
int az_init(int device, void** handle);
int az_make_current(void* handle);
int az_context_device(void* handle, int* device);
int az_destroy(void* handle);
/* WORKSPACE CONTRACT (az_gemm_bf16, az_gemm_wgrad_bias_bf16, az_conv2d_bf16, az_conv2d_wgrad_bias_bf16): `workspace` holds the
 * fp32 split-K slabs and the column-sum slots; give each stream that issues products concurrently its own.  Nothing is assumed
 * about its contents and nothing in it survives a call.  While option INKERNEL_FINISH is set (default 0 -- measured slower than
 * the separate reduce launch in the two-stream step) its LAST 16 KiB hold one arrival counter per output tile, zeroed by the
 * library in front of every launch: the workgroup that arrives last at a tile's counter sums the tile's slabs in ascending split
 * order and finishes its column sums (no reduce / finish kernel follows the product).  Grids of more than 4096 tiles, or a
 * workspace of < 80 KiB, use the separate finish launches. */
/* ref: train.py:2760-2761 (every torch.nn.Linear inside unet(...): time/add embedding MLPs, proj_in/out, to_q/k/v/out, ff.net.*), train.py:2765 (their autograd dgrad / wgrad) */
int az_gemm_bf16(int transA, int transB, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                 void* C, long ldc, const void* bias, const void* rowbias, int rows_per_seg, long ld_rowbias,
                 const void* residual, long ldr, int accumulate, int split_k, void* workspace, long workspace_bytes,
                 void* stream);

/* MANY linear products that share the A operand in ONE launch: C_g[M, N_g] = A[M, K] . W_g[N_g, K]^T (+ bias_g) for every group g.
 * groups_dev: device array of ngroups records of seven int64 each -- W pointer, C pointer, bias pointer (or 0), N, ldb, ldc, index of
 * the group's first 160-wide tile column (a group takes (N + 159) / 160 columns; first-column indices ascend from 0);
 * total_tiles_n = their total.  Every group: N % 8 == 0, ldb % 8 == 0, ldc % 8 == 0, W and C 16-byte aligned, extents below
 * 2 GiB (the caller checks: the records live in device memory).  Used for the products whose A operand does not depend on the layer:
 * the cross-attention to_k|to_v projections of the text context (70 per step) and the ResnetBlock2D time_emb_proj linears (17). */
/* ref: train.py:2760-2761 (attn2.to_k / attn2.to_v and time_emb_proj inside unet(...): same input for every layer) */
int az_gemm_nt_grouped_bf16(int M, int K, const void* A, long lda, const void* groups_dev, int ngroups, long total_tiles_n, void* stream);

/* MANY independent weight-gradient products in ONE launch: dW_g[M_g, N_g] += dY_g[K_g, M_g]^T . X_g[K_g, N_g] (and, where a bias
 * gradient pointer is given, bias_g[:n_real] += column sums of dY_g) for every product g, each over its WHOLE k-range on 128x128
 * tiles -- no split-K slabs, no reduce / finish launches: the tiles of all products fill the chip together.
 * groups_dev: device array of ngroups records of sixteen int64 each -- dY, X, dW, bias-gradient pointer (or 0), M, N, K, lddy, ldx,
 * lddw, first tile id, tiles_m = ceil(M / 128), tiles_n = ceil(N / 128), n_real (<= M), vec (1: N % 8 == 0, lddw % 8 == 0 and dW
 * 16-byte aligned -> 16-byte epilogue), 0.  First tile ids ascend from 0; total_tiles = their total.  Every product: lddy % 8 == 0,
 * ldx % 8 == 0, dY / X 16-byte aligned, rows readable in 8-element chunks, operand extents below 2 GiB (the caller checks: the
 * records live in device memory).  Results are deterministic (one workgroup owns a tile and its bias-gradient rows). */
/* ref: train.py:2765 (loss.backward(): grad_weight = dY^T X, grad_bias = dY.sum(0) of every nn.Linear of a transformer block) */
int az_gemm_tn_grouped_bf16(const void* groups_dev, int ngroups, long total_tiles, void* stream);

/* The GEGLU projection with the GEGLU itself in the epilogue: proj[M, 2H] = X[M, K] . W[2H, K]^T + bias (value | gate halves, kept
 * for the backward pass) AND out[M, H] = value * gelu(gate) (erf GELU), computed from the bf16-rounded projection -- bit for bit what
 * az_gemm_bf16 followed by az_geglu_fwd produces, without reading proj back (one launch and an [M, 2H] read less per
 * transformer block).  H % 8 == 0, K % 8 == 0, leading dimensions % 8 == 0, all pointers 16-byte aligned; bias may be NULL. */
/* ref: train.py:2760-2761 (diffusers FeedForward: GEGLU.proj Linear, then hidden * gelu(gate)) */
int az_gemm_geglu_fwd_bf16(int M, int H, int K, const void* X, long lda, const void* W, long ldb, const void* bias, void* proj, long ldp,
                           void* out, long ldo, void* stream);

/* linear weight gradient dW[M=out][N=in] (+)= dY^T . X with the BIAS gradient fused into the same pass over dY
 * (torch autograd computes grad_bias = dY.sum(0) as a separate reduction): bias_grad[m] += sum_k dY[k][m] for m < n_real.
 * The column sums ride on the matrix pipe (one extra MFMA per A fragment against an all-ones fragment); split-K
 * partials are summed in a fixed order.  Needs the fp32 workspace (>= 64*M*4 bytes beyond the split-K slabs). */
/* ref: train.py:2765 (autograd of nn.Linear: grad_weight = dY^T X and grad_bias = dY.sum(0)) */
int az_gemm_wgrad_bias_bf16(int M, int N, int K, const void* dY, long lddy, const void* X, long ldx, void* dW, long lddw,
                            int accumulate, int split_k, void* workspace, long workspace_bytes, void* bias_grad, int n_real,
                            void* stream);

/* 3x3 (pad 1, stride 1|2) or 1x1 convolution on NHWC as implicit GEMM.
 *   mode 0 forward : out = Y[B,Hout,Wout,Cout] from X, W (+bias[co]) (+rowbias[b][co]) (+residual)
 *   mode 1 dgrad   : out = dX[B,Hin,Win,Cin]   from dY, W   (3x3 only; 1x1 dgrad is az_gemm_bf16)
 *   mode 2 wgrad   : out = dW[Cout][k][k][Cin] from dY, X   (accumulate / split_k as az_gemm_bf16)
 *   mode 3 dgrad   : as mode 1 but W is the pre-transposed copy W'[Cin][ky][kx][Cout] (Cout % 8 == 0): NT-form product
 * `cpad` (mode 1): channel count dY rows are padded to (>= Cout, multiple of 8; 0 => Cout).
 * mode | 16 (with mode 0 or 2, 3x3, stride 1): X is stored at HALF resolution [B][ceil(Hin/2)][ceil(Win/2)][Cin] and is read
 *   through a nearest-neighbour gather (source pixel (y >> 1, x >> 1)) -- diffusers Upsample2D (F.interpolate(mode="nearest")
 *   followed by the conv) without materialising the upsampled tensor; Hin / Win stay the UPSAMPLED extents.  They may be odd:
 *   that is F.interpolate(size=(2n - 1, ...)), the nearest-2x image with its last row / column cropped, and the conv pads with
 *   zeros at the cropped edge.  Even extents are F.interpolate(scale_factor=2).  az_conv2d_wgrad_bias_bf16 takes the same flag
 *   as ksize | 16.
 * ldx / lddy / ldo / ldr: elements between consecutive pixels.  Cin multiple of 8. */
/* ref: train.py:2760-2761 / 2765 (every nn.Conv2d of ResnetBlock2D, Downsample2D, Upsample2D, conv_in, conv_out and its backward) */
int az_conv2d_bf16(int mode, int batch, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int ksize, int stride,
                   int pad, int cpad, const void* X, long ldx, const void* W, const void* dY, long lddy, void* out,
                   long ldo, const void* bias, const void* rowbias, long ld_rowbias, const void* residual, long ldr,
                   int accumulate, int split_k, void* workspace, long workspace_bytes, void* stream);
/* conv weight gradient (mode 2 of az_conv2d_bf16) with fused bias gradient and, optionally, the per-sample column sums
 * seg_grad[b][co] = sum over the sample's pixels of dY (ResnetBlock2D: the gradient of the time-embedding projection
 * that was broadcast-added after conv1).  bias_grad (+=) and seg_grad (overwritten) are bf16; either may be NULL. */
/* ref: train.py:2765 (autograd of nn.Conv2d weight / bias; the per-sample sums are the gradient of ResnetBlock2D's time_emb_proj broadcast add) */
int az_conv2d_wgrad_bias_bf16(int batch, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int ksize, int stride, int pad,
                              const void* X, long ldx, const void* dY, long lddy, void* dW, int accumulate, int split_k,
                              void* workspace, long workspace_bytes, void* bias_grad, void* seg_grad, void* stream);

/* ---- attention (F.scaled_dot_product_attention via diffusers AttnProcessor2_0,
 *      train.py:204-228; head_dim 64, no mask, dropout 0) -------------------------------------- */
/* Q[b][tq][h*64+d] with row stride ldq (elements) and batch stride sq; same for K,V (tk), O.
 * lse[b][h][tq] fp32 = log-sum-exp of scaled scores (saved for backward). */
/* ref: train.py:204-228 (attention processor choice) -> F.scaled_dot_product_attention executed at train.py:2760-2761 */
int az_attn_fwd(int batch, int heads, int Tq, int Tk, float scale, const void* Q, long ldq, long sq, const void* K,
                long ldk, long sk, const void* V, long ldv, long sv, void* O, long ldo, long so, void* lse,
                void* stream);
/* dQ,dK,dV from dO (+ saved Q,K,V,O,lse); delta[b][h][tq] fp32 scratch. dQ/dK/dV are overwritten.
 * workspace (optional fp32 scratch): lets short-context (cross-attention) dK/dV split the query range across
 * workgroups; partials are summed in a fixed order (no atomics).
 * parts: bit0 delta = rowsum(dO*O), bit1 dQ kernel, bit2 dK/dV kernel (0 = all); dQ and dK/dV only need delta,
 * so a caller may issue them on different streams. */
/* ref: train.py:2765 (autograd of scaled_dot_product_attention) */
int az_attn_bwd(int batch, int heads, int Tq, int Tk, float scale, const void* Q, long ldq, long sq, const void* K,
                long ldk, long sk, const void* V, long ldv, long sv, const void* O, long ldo, long so, const void* dO,
                long lddo, long sdo, const void* lse, void* delta, void* dQ, long lddq, long sdq, void* dK, long lddk,
                long sdk, void* dV, long lddv, long sdv, void* workspace, long workspace_bytes, int parts, void* stream);

/* ---- normalisation (torch GroupNorm / LayerNorm inside diffusers blocks; fp32 statistics) ---- */
/* GroupNorm over NHWC x[B][HW][C] (ld = ldx), G groups, optional fused SiLU.  stats[B][G][2] fp32
 * (mean, rstd) is written by fwd and consumed by bwd.  partial: fp32 scratch >= az_gn_scratch_floats.
 * gamma / beta: 16-byte aligned (read 8 channels at a time), stats 8-byte aligned. */
/* ref: no reference counterpart (workspace size query) */
long az_gn_scratch_floats(int batch, int HW, int C, int G);
/* ref: train.py:2760-2761 (nn.GroupNorm(32) + SiLU of ResnetBlock2D, Transformer2DModel.norm, conv_norm_out) */
int az_groupnorm_fwd(int batch, int HW, int C, int G, float eps, int fuse_silu, const void* x, long ldx,
                     const void* gamma, const void* beta, void* y, long ldy, void* stats, void* partial, void* stream);
/* dx (overwritten or accumulated), dgamma/dbeta (bf16, ACCUMULATED in place) */
/* ref: train.py:2765 (its autograd) */
int az_groupnorm_bwd(int batch, int HW, int C, int G, int fuse_silu, const void* x, long ldx, const void* gamma,
                     const void* beta, const void* stats, const void* dy, long lddy, void* dx, long lddx,
                     int accumulate_dx, void* dgamma, void* dbeta, void* partial, void* stream);
/* the same with the accumulation source named separately: dx = (dx_add ? dx_add : 0) + gradient.  dx_add == dx is the in-place
 * form above; a different buffer leaves dx_add untouched, so a weight-gradient product that still reads it (the residual stream's
 * gradient is some layer's dY) need not have finished */
/* ref: train.py:2765 (autograd accumulates the residual stream's gradient out of place as well) */
int az_groupnorm_bwd_ex(int batch, int HW, int C, int G, int fuse_silu, const void* x, long ldx, const void* gamma,
                        const void* beta, const void* stats, const void* dy, long lddy, void* dx, long lddx,
                        const void* dx_add, long ld_add, void* dgamma, void* dbeta, void* partial, void* stream);
/* LayerNorm over rows of x[M][C]; stats[M][2] fp32.  partial: fp32 scratch >= az_ln_scratch_floats. */
/* ref: no reference counterpart (workspace size query) */
long az_ln_scratch_floats(int M, int C);
/* ref: train.py:2760-2761 (nn.LayerNorm norm1-3 of BasicTransformerBlock) */
int az_layernorm_fwd(int M, int C, float eps, const void* x, long ldx, const void* gamma, const void* beta, void* y,
                     long ldy, void* stats, void* stream);
/* dx may be NULL (gamma / beta gradients only); dgamma / dbeta may be NULL (data gradient only) */
/* ref: train.py:2765 (its autograd) */
int az_layernorm_bwd(int M, int C, const void* x, long ldx, const void* gamma, const void* stats, const void* dy,
                     long lddy, void* dx, long lddx, int accumulate_dx, void* dgamma, void* dbeta, void* partial,
                     void* stream);
/* the same with the accumulation source named separately (see az_groupnorm_bwd_ex) */
/* ref: train.py:2765 (same) */
int az_layernorm_bwd_ex(int M, int C, const void* x, long ldx, const void* gamma, const void* stats, const void* dy,
                        long lddy, void* dx, long lddx, const void* dx_add, long ld_add, void* dgamma, void* dbeta, void* partial,
                        void* stream);
/* The one-pass LayerNorm backward with the gamma / beta gradients left as partial sums: dx (= dx_add + gradient) is final,
 * partial[nblk][C][2] fp32 holds per-block (dgamma, dbeta) sums, to be finished later by az_ln_param_finish_multi -- the
 * parameter gradients are not needed before the end of the backward pass.  nblk: the block count the caller sized `partial`
 * (and its finish job) for, as returned by az_ln_partial_blocks(M) when it did; the launch derives its rows per block from
 * nblk and returns an argument error for a count that function cannot have returned, so a recorded launch replayed after the
 * LN_RPB option changed fails instead of writing past the buffer. */
/* ref: train.py:2765 (autograd of nn.LayerNorm; grad of weight / bias) */
int az_layernorm_bwd_partial(int M, int C, const void* x, long ldx, const void* gamma, const void* stats, const void* dy,
                             long lddy, void* dx, long lddx, const void* dx_add, long ld_add, void* partial, int nblk, void* stream);
/* ref: no reference counterpart (size query of the above: rows of the partial-sum buffer) */
int az_ln_partial_blocks(int M);
/* dgamma[c] += sum_k partial[k][c][0], dbeta[c] += sum_k partial[k][c][1] for MANY LayerNorms in one launch.  jobs_dev: device array
 * of njobs records of six int64 each -- partial, dgamma (or 0), dbeta (or 0), number of partial rows, C, index of the job's first
 * block (a job takes (C + 31) / 32 blocks; first-block indices ascend from 0); nblocks = their total. */
/* ref: train.py:2765 (same) */
int az_ln_param_finish_multi(const void* jobs_dev, int njobs, long nblocks, void* stream);

/* ---- elementwise / reductions ------------------------------------------------------------------ */
/* GEGLU (diffusers GEGLU, exact-erf GELU): proj[M][2H] -> out[M][H] = proj[:, :H] * gelu(proj[:, H:]) */
/* ref: train.py:2760-2761 (diffusers GEGLU of ff.net.0: hidden * gelu(gate), exact erf) */
int az_geglu_fwd(int M, int H, const void* proj, long ldp, void* out, long ldo, void* stream);
/* ref: train.py:2765 (its autograd) */
int az_geglu_bwd(int M, int H, const void* proj, long ldp, const void* dout, long lddo, void* dproj, long lddp,
                 void* stream);
/* ref: train.py:2760-2761 (SiLU on the summed time / text embedding before time_emb_proj) */
int az_silu_fwd(long n, const void* x, void* y, void* stream);
/* ref: train.py:2765 (its autograd) */
int az_silu_bwd(long n, const void* x, const void* dy, void* dx, int accumulate, void* stream);
/* y[rows][C] (ldy) = a (lda) + b (ldb) ; b may be null (strided copy) */
/* ref: train.py:2765 (autograd accumulation of a residual / skip gradient: grad += grad) */
int az_add_rows(long rows, int C, const void* a, long lda, const void* b, long ldb, void* y, long ldy, void* stream);
/* nearest-neighbour 2x upsample NHWC and its adjoint (2x2 sum) */
/* ref: train.py:2760-2761 (Upsample2D: F.interpolate(scale_factor=2, mode="nearest")) */
int az_upsample2x_fwd(int batch, int H, int W, int C, const void* x, void* y, void* stream);
/* ref: train.py:2765 (its autograd) */
int az_upsample2x_bwd(int batch, int H, int W, int C, const void* dy, void* dx, void* stream);
/* nearest-neighbour upsample NHWC x[B][H][W][C] -> y[B][Hout][Wout][C] to a target size, Hout in {2H - 1, 2H}, Wout in {2W - 1, 2W}
 * (anything else is an argument error): y[oy][ox] = x[oy >> 1][ox >> 1], which is what F.interpolate(size=, mode="nearest")
 * computes for these targets -- the 2x image with its last row / column cropped.  The adjoint is the 2x2 fold in which a source
 * pixel on a cropped edge receives 2 or 1 contributions instead of 4 (fp32 sums, rounded once).  C multiple of 8. */
/* ref: train.py:2760-2761 (Upsample2D with output_size: F.interpolate(size=upsample_size, mode="nearest"), taken by diffusers
 *      UNet2DConditionModel.forward when a sample side is not a multiple of 2**num_upsamplers) */
int az_upsample_nearest_fwd(int batch, int H, int W, int Hout, int Wout, int C, const void* x, void* y, void* stream);
/* ref: train.py:2765 (its autograd) */
int az_upsample_nearest_bwd(int batch, int H, int W, int Hout, int Wout, int C, const void* dy, void* dx, void* stream);
/* out[seg][C] fp32 = column sums of x[seg*rows_per_seg ...][C] (bias / time-embedding grads); two ordered
 * passes through scratch_f32 (>= az_colsum_scratch_floats), no atomics: bitwise reproducible */
/* ref: no reference counterpart (workspace size query) */
long az_colsum_scratch_floats(long rows, int C, int rows_per_seg);
/* ref: train.py:2765 (sum over rows as used by bias / broadcast gradients) */
int az_colsum(long rows, int C, int rows_per_seg, const void* x, long ldx, void* out_f32, void* scratch_f32, void* stream);
/* fused gradient form: seg_out_bf16[seg][C] = per-segment column sums (nullable: the time-embedding gradient of
 * ResnetBlock2D), bias_grad_bf16[c] += total column sums for c < n_real (nullable). Same scratch as az_colsum. */
/* ref: train.py:2765 (grad_bias of Linear / Conv2d and the gradient of the time-embedding broadcast add) */
int az_colsum_grad(long rows, int C, int rows_per_seg, const void* x, long ldx, void* seg_out_bf16, void* bias_grad_bf16,
                   int n_real, void* scratch_f32, void* stream);
/* dst_bf16[n] (+)= src_f32[seg][n] summed over nseg segments (finishes az_colsum into a bf16 grad) */
/* ref: train.py:2765 (finishes az_colsum into a bf16 .grad) */
int az_reduce_segs_to_bf16(int nseg, int n, const void* src_f32, void* dst, int accumulate, void* stream);
/* dst[c*ld_dst + r] = src[r*ld_src + c]: transposed weight copies W^T that turn every linear dgrad into the faster
 * k-contiguous (NT) product; refreshed once per optimizer step */
/* ref: no reference counterpart: W^T copies so that F.linear's dgrad (train.py:2765) reads k-contiguous operands */
int az_transpose_bf16(int R, int C, const void* src, long ld_src, void* dst, long ld_dst, void* stream);
/* the same for `batch` matrices at element strides bstride_src / bstride_dst (the 9 taps of a conv weight
 * [Cout][3][3][Cin] -> [Cin][3][3][Cout] in one launch) */
/* ref: no reference counterpart (same, all 9 taps of a conv weight) */
int az_transpose_bf16_batched(int batch, int R, int C, const void* src, long ld_src, long bstride_src, void* dst, long ld_dst,
                              long bstride_dst, void* stream);
/* many such transposes in ONE launch.  jobs_dev: device array of njobs records of eight int64 each -- src pointer, dst pointer, R, C,
 * ld_src, ld_dst, index of the job's first 64x64 tile, tiles per row ((C + 63) / 64) -- with first-tile indices ascending from 0;
 * ntiles = their total.  Every job must satisfy the 16-byte form: R, C, ld_src, ld_dst multiples of 8, pointers 16-byte aligned
 * (the caller checks; the whole W^T refresh of a UNet region is one call) */
/* ref: no reference counterpart (same, all weights of a parameter region) */
int az_transpose_multi_bf16(const void* jobs_dev, int njobs, long ntiles, void* stream);
/* fp32 [rows][C] -> bf16 */
/* ref: train.py:2760 (`.to(config.compute_dtype)` casts around the UNet call) */
int az_f32_to_bf16(long n, const void* src, void* dst, void* stream);
/* sinusoidal embedding (diffusers get_timestep_embedding, flip_sin_to_cos, shift 0):
 * out[i][0:half]=cos, [half:dim]=sin of t[i]*exp(-ln(1e4)*j/half); t fp32; out bf16 (ld = ldo) */
/* ref: train.py:2760-2761 (diffusers Timesteps / get_timestep_embedding inside unet(...)) */
int az_timestep_embed(int n, int dim, const void* t_f32, void* out, long ldo, void* stream);
/* NCHW (fp32 or bf16) <-> NHWC bf16 with channel padding (latents 4ch -> 8ch) */
/* ref: train.py:2760 (the NCHW latent handed to unet(...); layout change only) */
int az_nchw_to_nhwc_pad(int batch, int C, int HW, int Cpad, const void* src, int src_is_f32, void* dst, void* stream);
/* ref: train.py:2761 (`.sample` returned in NCHW) */
int az_nhwc_to_nchw(int batch, int C, int HW, int ldsrc, const void* src, void* dst, int dst_is_f32, void* stream);

/* ---- step glue (train.py:2743-2765) ------------------------------------------------------------- */
/* mode 0 epsilon, 1 v_prediction, 2 rectified_flow.  latents/noise NCHW [B][CHW]: latents bf16,
 * noise fp32.  coef_a/coef_b fp32 [B]: (sqrt_ab, sqrt_1m_ab) or (1-t, t).  Outputs: noisy NHWC bf16
 * padded to cpad channels (the UNet input), target fp32 NCHW. */
/* ref: train.py:2743-2758 (rectified-flow mix / scheduler.add_noise / get_velocity) */
int az_noise_target(int mode, int batch, int C, int HW, int cpad, const void* latents, const void* noise,
                    const void* coef_a, const void* coef_b, void* noisy_nhwc, void* target_f32, void* stream);
/* Noise modes (NOISE_MODE; an option outside the reference, not in the reference's loop): noise offset, multi-resolution
 * ("pyramid") noise and input perturbation, between the staged inputs and az_noise_target's arithmetic.
 * az_noise_shape writes, in place over the fp32 noise NCHW [B][C][H][W],
 *     u = eps + offset * o[b][c] + sum_{l=1..nlev} weight_l * up_l(z_l)[b][c][y][x]
 * o fp32 [B][C] (null: no offset term); fields: the level fields z_l packed in one fp32 buffer of nfields floats, level l at
 * table[4l] as [B][C][h_l][w_l]; table: DEVICE int32 [nlev][4] = (offset, h_l, w_l, bits of the fp32 weight_l).  up_l: bilinear
 * resampling to (H, W), half-pixel centres (F.interpolate(mode="bilinear", align_corners=False)), taps and fractions from the
 * integer numerator (2y+1) h_l - H.  Plain fp32 operations, no contraction.  partials (null: none): fp32 [B][nblk][2], nblk =
 * min(ceil(H W / 256), 64), the sums (u, u^2) of each block of a sample in a fixed order (no atomics; independent of B).
 * Refused: nlev outside 0..8, a null fields / table with nlev > 0, offset < 0 or NaN, C H W >= 2^24. */
/* ref: train.py:2743 (the noise handed to the mix; the reference has the plain draw only) */
int az_noise_shape(int batch, int C, int H, int W, void* noise_f32, const void* o, float offset, const void* fields, long nfields,
                   const void* table, int nlev, void* partials, void* stream);
/* az_noise_target with two optional inputs.  partials + nblk (az_noise_shape's): the noise is first normalised per sample,
 * eps' = u * r_b, r_b = 1 / sqrt((S2 - S1 (S1 / n)) / (n - 1)), n = C HW, S1 / S2 the sample's partials summed in block order
 * (unbiased std about the sample's mean; correctly rounded / and sqrt).  xi fp32 NCHW + perturb: the noisy latents are mixed from
 * eps' + perturb * xi while the target is built from eps'.  Both null: az_noise_target bit for bit. */
/* ref: train.py:2743-2758 (as az_noise_target) */
int az_noise_target_ex(int mode, int batch, int C, int HW, int cpad, const void* latents, const void* noise, const void* coef_a,
                       const void* coef_b, const void* partials, int nblk, const void* xi, float perturb, void* noisy_nhwc,
                       void* target_f32, void* stream);
/* weighted_sdxl_mse_loss (train.py:2408-2416) forward + d(loss*scale)/dpred.
 * pred NHWC bf16 [B][HW][ldp], target fp32 NCHW, w fp32 [B] (curve[timestep]).  loss_out fp32[1]
 * is overwritten; scratch_f32 >= 64*B floats (ordered partial sums, no atomics).  dpred NHWC bf16 padded to cpad channels (zeros). */
/* ref: train.py:2408-2416 (weighted_sdxl_mse_loss), train.py:2763-2765 ((loss / GA).backward() seed) */
int az_mse_loss_fwd_bwd(int batch, int C, int HW, const void* pred, long ldp, const void* target_f32, const void* w,
                        float grad_scale, void* loss_out, void* per_sample_out, void* dpred, int cpad, void* scratch_f32,
                        void* stream);
/* Robust losses in the place of the squared error (LOSS_TYPE; an option outside the reference): kind 1 l1 |x|, 2 huber
 * 2c x^2 / (sqrt(x^2+c^2) + c), 3 smooth_l1 2 x^2 / (sqrt(x^2+c^2) + c), x = float(pred) - target, c fp32 [B] the per-sample width
 * (null only for kind 1).  per_sample = mean over (C, HW) of l, loss = (1/B) sum_b w_b per_sample_b,
 * dpred = bf16(grad_scale w_b / (C HW B) * l'(x)).  Operands, padding, scratch and summation order as az_mse_loss_fwd_bwd; the squared
 * error is not a kind of this entry.  Refused: kind outside 1..3, cpad < C, ldp < C, a null c for kinds 2 and 3. */
/* ref: train.py:2408-2416, train.py:2763-2765 (the loss seam; the reference has the squared error only) */
int az_robust_loss_fwd_bwd(int kind, int batch, int C, int HW, const void* pred, long ldp, const void* target_f32, const void* w,
                           const void* c, float grad_scale, void* loss_out, void* per_sample_out, void* dpred, int cpad,
                           void* scratch_f32, void* stream);

/* ---- optimizer (raven.py:89-149, titan.py:119-131,162-184,230-296; clip train.py:2771-2781) ------- */
/* sum of squares of n bf16 grads -> out_f32[0] (accumulate=1 adds to existing value) */
/* ref: train.py:2771-2781 (torch.nn.utils.clip_grad_norm_: global L2 norm) */
int az_sumsq_bf16(long n, const void* g, void* out_f32, int accumulate, void* scratch_f32, void* stream);
/* same with dtype 0 = bf16, 1 = fp32 (fp32 may be pinned host memory: Titan's CPU-resident grads).
 * scratch_f32: >= 1024 floats */
/* ref: train.py:2771-2781, titan.py:162-184 (norm of host fp32 gradients) */
int az_sumsq(long n, const void* g, int dtype, void* out_f32, int accumulate, void* scratch_f32, void* stream);
/* clip coefficient on device: coef[0] = min(1, max_norm / (sqrt(sumsq*inv_scale2) + 1e-6)); norm[0] = sqrt(...) */
/* ref: train.py:2775-2778 (clip coefficient max_norm / (norm + 1e-6), clamped to 1) */
int az_clip_coef(const void* sumsq_f32, float max_norm, float grad_unscale, void* coef_f32, void* norm_f32, void* stream);
/* fused AdamW on a flat range: p bf16 (device), g bf16 (device), m/v (device staging copies of the
 * host state, dtype mdtype: 0 bf16, 1 fp32, 2 fp16 -- raven.py:37-42 momentum_dtype).  hyper (device fp32[8]): lr, beta1, beta2, eps,
 * wd_factor, step_size(lr/bc1), sqrt_bc2, unused.  coef (device fp32[1]) multiplies g (clip); a bf16 gradient is
 * rounded to bf16 after the multiplication, i.e. exactly the value an in-place clip_grad_norm_ would have left. */
/* ref: raven.py:89-149 (RavenAdamW.step element math) */
int az_adamw_flat(long n, void* p, const void* g, void* m, void* v, int mdtype, const void* hyper, const void* coef,
                  void* stream);
/* Raven step over a flat parameter range with m,v resident in PINNED HOST memory: chunked
 * H2D(m,v) -> az_adamw_flat -> D2H(m,v) pipelined over 3 streams with double-buffered device staging
 * (staging: device scratch >= 4 * chunk_elems * sizeof(mdtype)).  The hand-off events are kept per compute stream (created
 * on first use under a mutex), so optimizers on different streams / devices of one process are independent; calls naming the
 * SAME compute stream must not be issued from two host threads at once. */
/* ref: raven.py:103-149 (per-parameter H2D of exp_avg / exp_avg_sq, update, D2H) */
int az_raven_step(long n, void* p, const void* g, void* m_host, void* v_host, int mdtype, const void* hyper,
                  const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                  void* stream_d2h);
/* _ex variants: gdtype 0 = bf16 grads (device), 1 = fp32 grads (device or pinned host: Titan) */
/* ref: raven.py:89-149, titan.py:230-296 (fp32 host gradients) */
int az_adamw_flat_ex(long n, void* p, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                     const void* coef, void* stream);
/* ref: raven.py:103-149, titan.py:230-296 */
int az_raven_step_ex(long n, void* p, const void* g, int gdtype, void* m_host, void* v_host, int mdtype, const void* hyper,
                     const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                     void* stream_d2h);
/* _sr variants (an option the reference does not have; off by default -- INTEGRATION.md "Stochastic rounding"): the same arithmetic and
 * the same m / v as the _ex entry points, but the fp32 result is written to the bf16 parameter with STOCHASTIC rounding instead of
 * round-to-nearest-even: o = (bits(pp) + r) >> 16 with r uniform in [0, 65536) (non-finite pp, and a carry into the all-ones exponent,
 * excepted), so the magnitude rounds up with probability (low half) / 65536 and a representable value never changes.  r comes from
 * Philox4x32-10: key = (seed low word, seed high word), counter = (group low word, group high word, step, domain) with
 * group = e >> 3 for the element's GLOBAL index e = elem0 + offset in the call; element e takes the low (e even) or high (e odd)
 * half of output word (e & 7) >> 1.  The bits of an element therefore do not depend on how a flat range is cut into calls, chunks,
 * regions or rank shards; the caller keeps (seed, step, domain, e) distinct for all elements updated in one step.  16-byte accesses
 * when (elem0 + i) % 8 == 0 coincides with 16-byte alignment of p, g, m, v, element-wise otherwise.  elem0 >= 0.
 * `step` is an argument, not device memory: the optimizer step is issued eagerly.  Should it ever be issued from a recorded tape,
 * step (and the hyper vector's contents) must not be frozen into the recording. */
/* ref: raven.py:144 (p.copy_(p32): the bf16 write-back being varied), raven.py:89-149, titan.py:230-296 */
int az_adamw_flat_sr(long n, void* p, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                     const void* coef, long seed, long step, long domain, long elem0, void* stream);
/* the chunked pinned-host pipeline of az_raven_step_ex; chunk c is launched with elem0 + c * chunk_elems */
/* ref: raven.py:103-149, raven.py:144, titan.py:230-296 */
int az_raven_step_sr(long n, void* p, const void* g, int gdtype, void* m_host, void* v_host, int mdtype, const void* hyper,
                     const void* coef, void* staging, long chunk_elems, void* stream_compute, void* stream_h2d,
                     void* stream_d2h, long seed, long step, long domain, long elem0);
/* fp32 exponential moving average of bf16 parameters over a flat range (an option the reference does not have; off by default --
 * INTEGRATION.md "EMA of the weights"): e[i] <- e[i] - omd * (e[i] - float(p[i])), i in [0, n), omd = 1 - decay.  p bf16 (read only),
 * e fp32 (in place).  Three fp32 operations, each rounded (no contraction): t = e - float(p); t = omd * t; e = e - t -- the form of
 * diffusers' EMAModel.step.  NaN and inf follow IEEE rules; omd == 1 is not special.  16-byte accesses from the first element at which p
 * and e are both 16-byte aligned, element-wise before it, in the tail, and everywhere when the two cannot be co-aligned.  n == 0
 * returns 0 without a launch; n < 0, a null pointer, p not 2-byte aligned or e not 4-byte aligned are argument errors. */
/* ref: not in the reference; runs behind `optimizer.step()`, train.py:2783 */
int az_ema_flat(long n, const void* p, void* ema_f32, float one_minus_decay, void* stream);
/* AdamW over a flat range with an fp32 MASTER copy of the parameters (an option the reference does not have; off by default --
 * INTEGRATION.md "fp32 master weights"): the arithmetic of az_adamw_flat_ex operation for operation (the reference's order, no
 * contraction, the clip coefficient applied in-kernel, a bf16 gradient rounded to bf16 after the multiplication) with ONE difference:
 * the parameter operand is w[i] (fp32, read) instead of float(p[i]).  Writes w[i] = pp and p[i] = bf16(pp), round to nearest even; p
 * is never read.  m, v, mdtype, gdtype, hyper and coef (may be null) as az_adamw_flat_ex.  NaN and inf follow IEEE rules through both
 * outputs.  16-byte accesses from the first element at which p, g, m, v and w are all 16-byte aligned, element-wise before it, in the
 * tail, and everywhere when the five cannot be co-aligned.  n == 0 returns 0 without a launch; n < 0, a null p / w / g / m / v / hyper,
 * mdtype or gdtype out of range, or a pointer not aligned to its element (p 2 bytes, w 4 bytes) are argument errors. */
/* ref: raven.py:109-147 (the update with p32 kept between steps instead of p.copy_(p32) alone), titan.py:230-296 */
int az_adamw_flat_master(long n, void* p, void* w_f32, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                         const void* coef, void* stream);
/* AdamW over a flat range whose elements belong to PARAMETER GROUPS with their own learning rate and weight decay (an option the
 * reference's trainer does not use; off by default -- INTEGRATION.md "Parameter groups"): ONE launch for the range, however many
 * groups alternate in it.  The call's element i has the global index e = elem0 + i and belongs to the first segment s with
 * seg_end[s] > e (seg_end: device int64[nseg], ascending, exclusive ends; an element past the last end takes the last segment); its
 * group is seg_gid[s] (device int32[nseg], clamped to [0, ngroups)), and it is updated with wd_factor = ghyper[2 * group] and
 * step_size = ghyper[2 * group + 1] (device fp32[ngroups][2]) in place of hyper[4] and hyper[5]; beta1, beta2, eps and sqrt_bc2
 * are hyper's.  The arithmetic is az_adamw_flat_ex's operation for operation; a segment may end anywhere, inside an aligned group
 * of 8 elements too.  The parameter operand: w_f32 null and rounding 0 -- bf16 p, round to nearest even (az_adamw_flat_ex);
 * rounding 1 -- stochastic rounding with (seed, step, domain, elem0) as az_adamw_flat_sr; w_f32 given -- the fp32 master of
 * az_adamw_flat_master (rounding must be 0).  No lookup ever leaves the three tables, whatever they hold.  n == 0 returns 0 without
 * a launch; n < 0, a null p / g / m / v / hyper / table, nseg <= 0, ngroups <= 0 or > 255, elem0 < 0, mdtype, gdtype or rounding out
 * of range, or a pointer not aligned to its element are argument errors. */
/* ref: raven.py:96-105 (the loop over param_groups with their own lr / weight_decay), train.py:347-352 (lr_scale per group) */
int az_adamw_flat_seg(long n, void* p, void* w_f32, const void* g, int gdtype, void* m, void* v, int mdtype, const void* hyper,
                      const void* coef, const void* seg_end, const void* seg_gid, long nseg, const void* ghyper, int ngroups,
                      long elem0, int rounding, long seed, long step, long domain, void* stream);
/* g_bf16[i] = bf16(g[i] * coef[0]) in place -- the in-place clip of torch.nn.utils.clip_grad_norm_
 * (train.py:2775-2778); skipped entirely when coef[0] == 1 */
/* ref: train.py:2775-2778 (in-place gradient scaling of clip_grad_norm_) */
int az_scale_bf16(long n, void* g, const void* coef_f32, void* stream);
/* x_f32[i] *= coef[0]  (Titan's CPU-side clip of host grads, titan.py:177-182) */
/* ref: titan.py:177-182 */
int az_scale_f32(long n, void* x, const void* coef_f32, void* stream);
/* Per-micro-step input staging in ONE launch.  src_ptrs / dst_ptrs: HOST arrays of nseg <= 8 device pointers (4-byte aligned),
 * seg_bytes: HOST array of nseg longs (each % 4 == 0): dst[i][0 .. bytes[i]) = src[i][..]; coef_host: HOST array of ncoef <= 256
 * floats -> coef_dev[0 .. ncoef).  All four host arrays are read DURING the call (the floats travel in the kernel arguments: the
 * caller may reuse them at once -- no pinned buffer, no event).  Replaces the per-micro-step tensor placements of the reference's
 * loop body (train.py:2731 time_ids, 2733-2758 noise / timestep-derived coefficients, 2760 the UNet's inputs) when the batch is
 * already on the device: as hipMemcpyAsync copies they ran as blit kernels with 0.1-0.4 ms of idle stream time around each. */
int az_stage_inputs(int nseg, const void* src_ptrs, const void* dst_ptrs, const void* seg_bytes, int ncoef, const void* coef_host,
                    void* coef_dev, void* stream);
/* Titan: offload grad range to host fp32 (copy, or add when accumulate) via device staging */
/* ref: titan.py:93-100, 119-131 (post-accumulate hook: copy_ on the first micro-step, add_ afterwards) */
int az_titan_offload(long n, const void* g, void* g_host_f32, void* staging_f32, int accumulate, void* stream);
/* paged_adamw_8bit: one blockwise 8-bit AdamW step over ntensors bf16 tensors in one launch.
 * desc (device): ntensors records of 12 int64 words -- p, g (storage pointers), state1, state2 (uint8 codes, or fp32 moments),
 * absmax1, absmax2 (fp32 per 256-element block, 8-bit path), numel, first global block, flags (1 = 8-bit state, 2 = 4-D weight
 * stored (O, kh, kw, I_pad) and read as (O, I, kh, kw), 4 = plain with 8-byte aligned p / g and 4-byte aligned codes), kh*kw
 * (<= 32), I | I_pad << 32, hyper row -- then ntensors + 1 int64 first-block indices (the last = nblocks).  State is in LOGICAL
 * element order; numel < 2^31.  hyper (device fp32 [rows][8]): b1, b2, 1-b1, 1-b2, step_size, eps*sqrt(1-b2^t), 1-lr*wd, wd>0.
 * qmaps (device fp32 [2][256]): signed map of state1, unsigned map of state2.  coef (device fp32[1], may be null): g = bf16(g*coef). */
/* ref: train.py:2271-2288 (create_optimizer: bnb.optim.PagedAdamW8bit) */
int az_adamw8bit_step(int ntensors, const void* desc, long nblocks, const void* hyper, const void* qmaps, const void* coef,
                      void* stream);
/* Prodigy (arXiv 2306.06101; an optimizer the reference does not have -- INTEGRATION.md "The Prodigy optimizer" states the arithmetic in
 * full, tests/prodigy_ref.py restates it on the CPU): AdamW-shaped moments scaled by a step size d that the device estimates itself
 * from two sums over all trainable elements, with an fp32 master copy w of the bf16 parameters.  One step is az_prodigy_begin, one
 * az_prodigy_moments per contiguous range, az_prodigy_finish, one az_prodigy_apply per range, all on ONE stream: 2 R + 2 launches for
 * R ranges, no copy to the host, no synchronisation; every sum has a fixed order (no floating-point atomics), so a step is
 * bit-reproducible.  Shared buffers:
 *   dstate (device fp64[8], 8-byte aligned): d, d_max, d_numerator, d_denom, d_hat, k, d0, one spare word.  The caller initialises
 *     d = d_max = d0 > 0 and the rest to 0.
 *   hyper (HOST fp64[16], 8-byte aligned, read DURING az_prodigy_begin -- the values travel in the kernel's arguments, the caller may
 *     reuse the array at once): lr, beta1, beta2, beta3, eps, weight_decay, d_coef, growth_rate (+inf = none), use_bias_correction
 *     (0 / 1), safeguard_warmup (0 / 1); the rest unused.  The caller issues no step when lr == 0.
 *   consts (device, 128 bytes, 8-byte aligned): fp32[16] = c_m, c_v, c_s, beta1, beta2, beta3 (written by begin), dlr, wd_dlr, eps_d
 *     (written by finish), weight_decay != 0, skip (1 from begin until finish has found d_denom != 0); then fp64[8] carried from begin
 *     to finish.  Every fp32 constant is computed in fp64 on the device and rounded once.
 *   partials (device fp64 pairs, 8-byte aligned): az_prodigy_moments over n elements writes az_prodigy_partials(n) pairs (numerator
 *     sum, denominator sum), one per block, at the pointer it is given; the caller lays the slices of a step's launches back to back
 *     and passes the total to az_prodigy_finish.
 * az_prodigy_partials(n): that pair count for the current device (blocks of 256 threads, 8 elements per thread and iteration, at most
 *   8 blocks per CU, a grid-stride loop beyond); 0 for n == 0; n < 0 or no device are errors (negative).
 * az_prodigy_begin: bc = sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) or 1; dlr = d lr bc; c_m = d (1 - beta1); c_v = d d (1 - beta2);
 *   c_s = (d / d0) dlr, or (d / d0) d with safeguard_warmup.  A null or misaligned pointer is an argument error.
 * az_prodigy_moments, element i in [0, n): gr = g[i] * coef[0] (coef: device fp32[1] or null = 1; a bf16 gradient is rounded to bf16
 *   after the multiplication); m = fma(gr, c_m, m beta1); v = v beta2 + ((c_v gr) gr); s = fma(gr, c_s, s beta3); the sums take
 *   (double)gr * (double)(p0 - w) -- the difference rounded to fp32, the product exact -- and (double)|s|, accumulated in fp64 per
 *   thread, then per block.  w, p0 fp32 (read), g bf16 (gdtype 0) or fp32 (1), m / v / s fp32 in place.  16-byte accesses from the
 *   first element at which w, p0, g, m, v and s are all 16-byte aligned, element-wise before it, in the tail, and everywhere when the
 *   six cannot be co-aligned.  n == 0 returns 0 without a launch (and writes no pair); n < 0, a null w / p0 / g / m / v / s / consts /
 *   partials, gdtype out of range or a pointer not aligned to its element are argument errors.
 * az_prodigy_finish: sums npartials pairs in a fixed order; d_numerator = beta3 d_numerator + (d / d0) dlr * sum; d_denom = sum.  If
 *   d_denom == 0 the step ends there: skip stays 1, d / d_max / d_hat / k are unchanged.  Otherwise d_hat = d_coef d_numerator /
 *   d_denom; d = max(d, d_hat) while d == d0; d_max = max(d_max, d_hat); d = min(d_max, d growth_rate); k += 1; dlr (the OLD d),
 *   wd_dlr = weight_decay dlr and eps_d = d_new eps for the apply pass.  npartials == 0 is a step with d_denom == 0; npartials < 0, a
 *   null dstate / consts, null partials with npartials > 0 or a misaligned pointer are argument errors.
 * az_prodigy_apply, element i in [0, n), nothing when skip is set: w = fma(w, -wd_dlr, w) when weight_decay != 0; w = w + ((-dlr m) /
 *   (sqrtf(v) + eps_d)); p = bf16(w), round to nearest even.  p bf16 (written, never read), w fp32 in place, m / v fp32 (read).
 *   16-byte accesses where p, w, m and v are co-aligned, as above.  n == 0 returns 0 without a launch; n < 0, a null pointer or one not
 *   aligned to its element are argument errors.  NaN and inf follow IEEE rules throughout. */
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
long az_prodigy_partials(long n);
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
int az_prodigy_begin(const void* dstate, const void* hyper_host, void* consts, void* stream);
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
int az_prodigy_moments(long n, const void* w, const void* p0, const void* g, int gdtype, void* m, void* v, void* s, const void* consts,
                       const void* coef, void* partials, void* stream);
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
int az_prodigy_finish(long npartials, const void* partials, void* dstate, void* consts, void* stream);
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
int az_prodigy_apply(long n, void* p, void* w, const void* m, const void* v, const void* consts, void* stream);
/* Adafactor (arXiv 1804.04235; an optimizer the reference does not have -- INTEGRATION.md "The Adafactor optimizer" states the
 * arithmetic, that of transformers.optimization.Adafactor.step on logical tensor shapes, in full; tests/adafactor_ref.py restates it in
 * float64): factored second moments (row and column vectors) for tensors of two or four dimensions, a full second moment for vectors,
 * the update clipped per tensor by its own RMS.  az_adafactor_step is one whole optimizer step in FIVE launches on one stream whatever
 * ntensors is (three when the table holds no matrix), no copy to the host, no synchronisation, no floating-point atomics: every sum
 * has a fixed order, the per-tensor sums of u^2 and p^2 are fp64, a step is bit-reproducible.
 *   desc (int64 words, az_adafactor_geometry(0) = 24 per row, one row per tensor, the SAME table on the host (desc_host, checked in full
 *     before anything is launched) and on the device (desc, read by the kernels)): class (0 vector, 1 matrix, 2 batch of little
 *     matrices), flags (1 = 16-byte accesses: p and g 16-byte aligned, C, the row stride and sr0 multiples of 8), p, g (addresses of
 *     bf16 storage, read-write and read), batch extents nb0, nb1 with strides sb0, sb1, R with row stride sr, C with column stride sc
 *     (strides in elements), state offsets of row (or v), col and exp_avg (fp32 elements of `state`; exp_avg in logical order, unused
 *     without beta1), first workgroup and workgroup count of passes 1 / 3 / 5, first workgroup and count of pass 2, offset of the column
 *     partials in `scratch` (stripes x C), offset of the C column factors and, behind them, the R row factors in `fac`, sr0 (flat offset of the tensor's first
 *     element: stochastic rounding draws the bits of element sr0 + storage offset), logical element count, one spare word.
 *     A matrix is nb0 = nb1 = 1, sc = 1 and takes ceil(R / geometry(1)) workgroups (row stripes) and ceil(C / geometry(4)) + 1 of pass 2;
 *     a vector is R = 1, C = n and takes ceil(n / geometry(2)); a batch has R = C in {1, 3}, one thread per (b0, b1), and takes
 *     ceil(nb0 nb1 / geometry(3)).  Matrices come first in the table; the numbering is cumulative in table order.
 *   state, scratch, fac (device fp32, 16-byte aligned, with their element counts: every offset of the table is checked against them),
 *   partials (device fp64, two per workgroup of pass 1), tsc (device fp32, four per tensor: clip denominator, lr_t, weight_decay lr_t,
 *   RMS(u)).
 *   hyper (HOST fp64[16], read during the call): beta2t, lr (the relative step where that is on), eps1, eps2, clip_threshold, beta1
 *     (negative = none), weight_decay, scale_parameter (0 / 1), stochastic rounding (0 / 1), seed, step (>= 1), Philox domain.  beta2t,
 *     1 - beta2t, beta1, 1 - beta1 are rounded once to fp32; lr_t = max(eps2, RMS(p)) lr (or lr) is formed in fp64 on the device and
 *     rounded once.
 * Per element: upd = g g + eps1; row / col / v = old beta2t + (1 - beta2t) mean; u = ((1 / sqrt(row / mean(row))) (1 / sqrt(col))) g or
 * (1 / sqrt(v)) g; u = u / max(1, RMS(u) / clip); u = lr_t u; with beta1 m = m beta1 + (1 - beta1) u, u = m; with weight decay
 * p = p - (weight_decay lr_t) p; p = p - u, rounded ONCE to bf16: to nearest even, or stochastically with the Philox layout of
 * az_adamw_flat_sr.  Elements outside the logical tensor (channel padding, slot padding) are neither read nor written.
 * ntensors == 0 returns 0 without a launch; a negative count, a null or misaligned pointer, an unknown class, a table whose numbering
 * or offsets do not fit are argument errors before any launch. */
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
long az_adafactor_geometry(int what);
/* ref: not in the reference; stands where optimizer.step() does, train.py:2783 */
int az_adafactor_step(int ntensors, const void* desc_host, const void* desc, void* state, long state_numel, void* scratch, long scratch_numel,
                      void* fac, long fac_numel, void* partials, void* tsc, const void* hyper_host, void* stream);

/* ---- LoRA adapter products (an option the reference does not have -- train.py is full fine-tuning only; INTEGRATION.md "LoRA
 *      (`az_lora_*`)" states the arithmetic, tests/lora_ref.py restates it in float64) -------------------------------------------
 * For a linear with base weight W[N][K], adapters A[r][K] ("down") and B[N][r] ("up") and s = alpha / r, all bf16, sums in fp32:
 *     forward   u  = bf16(x A^T)                      y  = bf16(float(y_base) + s (u B^T))
 *     backward  du = bf16(s (dy B))                   dx = bf16(float(dx_base) + du A)
 *               dA = bf16(float(dA_prev) + du^T x)    dB = bf16(float(dB_prev) + s (dy^T u))
 * Three shape classes, one entry point each; all are NT products (both operands contiguous along the summed index) except the
 * gradient, which sums over rows.  The backward data products therefore take TRANSPOSED copies of the adapters (B^T [r][N] for du,
 * A^T [K][r] for dx), which the caller refreshes after an optimizer step (az_transpose_bf16).  `parts` (1..3) projections that the
 * executor fuses (to_q|to_k|to_v, to_k|to_v) go in one launch: part p takes its operands at p * the part strides (elements).  The
 * small dimension is a multiple of 4 and is padded to the MFMA's 16 inside the kernels, never in memory.  Rows at or beyond M and
 * columns outside the addressed slices are neither read into a result nor written.  Deterministic: no floating-point atomics, so a
 * replayed launch reproduces the eager one bit for bit.  Argument errors -1110 .. -1119.
 *
 * az_lora_down_bf16 (skinny output): out[m][p r + n] = bf16(s sum_k X[m][p x_part_stride + k] W_p[n][k]), n < r, W_p = W + p
 *   w_part_stride, rows of W at ldw.  u = x A_cat^T is parts = 1 with r = the stacked rank R of the group (the down matrices are
 *   adjacent, x is read once); du is parts = the group's with X = dY, x_part_stride = N and W = the stacked B^T copies.  K % 8 == 0;
 *   r % 4 == 0, parts r <= 192; X, W 16-byte aligned with ldx, ldw and the part strides multiples of 8; out 8-byte aligned, ldo % 4 == 0.
 * az_lora_up_bf16 (skinny k, read-modify-write): Y[m][p y_part_stride + n] = bf16(float(Y[..]) + s sum_{k < r} U[m][p u_part_stride
 *   + k] W_p[n][k]), n < N.  y += s u B^T is parts = the group's with W = the stacked B (w_part_stride = N r) and Y_p the column
 *   slices of the fused output; dx += du A_cat is parts = 1, r = R, W = the A_cat^T copy [K][R].  N % 4 == 0, r % 4 == 0, r <= 192;
 *   U, W, Y 8-byte aligned, every leading dimension and part stride a multiple of 4.
 * az_lora_wgrad_bf16 (tall reduction): out[p out_part_stride + i_s out_stride_s + i_b out_stride_b] (+)= s sum_{m < M} S[m][p
 *   s_part_stride + i_s] G[m][p g_part_stride + i_b], i_s < ns (the small operand: du or u), i_b < nb (x or dy).  dA_cat[R][K] is
 *   out_stride_s = K, out_stride_b = 1; dB_p[N][r] is out_stride_s = 1, out_stride_b = r.  The rows are split into at most 64 ranges
 *   (a function of the shapes and workspace_bytes only) whose fp32 partial sums go to `workspace` (parts * splits * ns * nb floats,
 *   nothing in it survives the call); a second kernel adds them in ascending order, scales, adds the previous bf16 gradient when
 *   `accumulate` and rounds once.  ns % 4 == 0, ns <= 192, nb % 8 == 0; S 8-byte aligned, ld_s and s_part_stride % 4 == 0; G 16-byte
 *   aligned, ld_g and g_part_stride % 8 == 0.
 * az_lora_up_geglu_bf16 (the up product of ff.net.0.proj with the GEGLU in its epilogue; argument errors -1120 .. -1126):
 *     proj[m][n] = bf16(float(proj[m][n]) + s sum_{k < r} U[m][k] W[n][k])                 n < 2 H   (az_lora_up_bf16, parts = 1)
 *     out[m][h]  = bf16(float(proj[m][h]) * gelu_erf(float(proj[m][H + h])))               h < H     (az_geglu_fwd)
 *   with the second line taken on the ROUNDED, stored proj -- the rule of az_gemm_geglu_fwd_bf16's epilogue, so az_geglu_bwd, which
 *   re-reads proj, sees what the forward used.  U[M][r] is the down product, W[2 H][r] the up matrix (value rows, then gate rows),
 *   proj[M][2 H] the base product plus bias, updated in place; out[M][H] is written.  proj comes out with az_lora_up_bf16's bits and
 *   out with az_geglu_fwd's, in one launch and without the second read of proj.  One error number per rule, in this order: M > 0
 *   (-1120); H > 0, H % 8 == 0 (-1121); 4 <= r <= 64, r % 4 == 0 (-1122); no null pointer, all four 8-byte aligned (-1123); every row
 *   stride a multiple of 4 and at least its width r, r, 2 H, H (-1124); neither U nor out overlaps proj (-1125); M <= 64 * 65535
 *   (-1126). */
/* ref: not in the reference (train.py:2760-2761 runs the un-adapted nn.Linear); follows the base product of an adapted projection */
int az_lora_down_bf16(int M, int K, int r, int parts, float s, const void* X, long ldx, long x_part_stride, const void* W, long ldw,
                      long w_part_stride, void* out, long ldo, void* stream);
/* ref: not in the reference (same) */
int az_lora_up_bf16(int M, int N, int r, int parts, float s, const void* U, long ldu, long u_part_stride, const void* W, long ldw,
                    long w_part_stride, void* Y, long ldy, long y_part_stride, void* stream);
/* ref: not in the reference (train.py:2760-2761 runs the un-adapted GEGLU.proj Linear, then hidden * gelu(gate)) */
int az_lora_up_geglu_bf16(int M, int H, int r, float s, const void* U, long ldu, const void* W, long ldw, void* proj, long ldp, void* out,
                          long ldo, void* stream);
/* ref: not in the reference; stands beside the weight gradients of train.py:2765 */
int az_lora_wgrad_bf16(int M, int ns, int nb, int parts, float s, const void* S, long ld_s, long s_part_stride, const void* G, long ld_g,
                       long g_part_stride, void* out, long out_stride_s, long out_stride_b, long out_part_stride, int accumulate,
                       void* workspace, long workspace_bytes, void* stream);

/* ---- LoRA adapters on 3x3 convolutions (conv1 / conv2 of a ResnetBlock2D; kohya-ss conv_dim, LoCon; INTEGRATION.md "LoRA";
 *      tests/lora_conv_ref.py restates the arithmetic in float64) ---------------------------------------------------------------
 * For a 3x3, stride-1, pad-1 convolution with base weight W[Cout][3][3][Cin], adapters A[r][3][3][Cin] ("down", the base weight's
 * own layout) and B[Cout][r] ("up") and s = alpha / r:
 *     forward   u  = bf16(A (*) x)                    y  = bf16(float(y_base) + s (u B^T))            (az_lora_up_bf16)
 *     backward  du = bf16(s (dy B))  (az_lora_down_bf16)     dx = bf16(float(dx_base) + A^T (*) du)
 *               dA = bf16(float(dA) + du^T (*) x)            dB = bf16(float(dB) + s (dy^T u))        (az_lora_wgrad_bf16)
 * The three gathered products are the entry points below.  Activations are NHWC rows [B H W][C] with any row stride; pixel m =
 * (b, h, w) meets, at tap t = 3 kh + kw, pixel nbr(m, t) = (b, h + kh - 1, w + kw - 1) of the SAME image, and a tap outside the
 * image contributes zero (a predicated zero fragment, never a load, never memory padding).  All on v_mfma_f32_16x16x32_bf16 in
 * az_lora_*'s operand order; the rank is padded by zero fragments.  No floating-point atomics: every sum has one fixed order.
 * Cin % 8 == 0; 4 <= r <= 64, r % 4 == 0; B H W < 2^31.  Argument errors -1130 .. -1139 (first of each entry point: geometry,
 * Cin or r; second: a null or misaligned pointer; third: a row stride).
 *
 * az_lora_conv_down_bf16: out[m][n] = bf16(s sum_t sum_c X[nbr(m, t)][c] A[n][t][c]), n < r.  One pass over X per tap; the 4 waves
 *   of a 16-pixel block split the k-range 9 Cin and are added in wave order.  X, A 16-byte aligned, ldx % 8 == 0; out 8-byte
 *   aligned, ldo % 4 == 0; A contiguous.
 * az_lora_conv_dgrad_bf16: dX[m][c] = bf16(float(dX[m][c]) + s sum_t sum_{j < r} dU[nbr'(m, t)][j] At[c][t][j]) with the taps
 *   mirrored, nbr'(m, t) = (b, h - kh + 1, w - kw + 1): read-modify-write of the base data gradient with one rounding.  At is the
 *   copy [Cin][3][3][r] of A (j contiguous per (c, t)), contiguous.  dU, At, dX 8-byte aligned, ldu % 4 == 0, ldx % 4 == 0; dU
 *   and dX may not overlap (-1135).
 * az_lora_conv_wgrad_bf16: dA[j][t][c] (+)= s sum_m dU[m][j] X[nbr(m, t)][c].  Two stages like az_lora_wgrad_bf16: fp32 partial
 *   sums per row range in `workspace` (at most 64 ranges, a function of the shapes and workspace_bytes only; r * 9 Cin floats per
 *   range, -1139 when not even one fits), then a finish in ascending order that scales, adds the previous bf16 gradient when
 *   `accumulate` and rounds once.  dU 8-byte aligned, ldu % 4 == 0; X 16-byte aligned, ldx % 8 == 0; dA contiguous. */
/* ref: not in the reference (train.py:2760-2761 runs the un-adapted ResnetBlock2D convolutions); follows the base convolution */
int az_lora_conv_down_bf16(int B, int H, int W, int Cin, int r, float s, const void* X, long ldx, const void* A, void* out, long ldo,
                           void* stream);
/* ref: not in the reference; follows the base convolution's data gradient in the backward of train.py:2765 */
int az_lora_conv_dgrad_bf16(int B, int H, int W, int Cin, int r, float s, const void* dU, long ldu, const void* At, void* dX, long ldx,
                            void* stream);
/* ref: not in the reference; stands beside the weight gradients of train.py:2765 */
int az_lora_conv_wgrad_bf16(int B, int H, int W, int Cin, int r, float s, const void* dU, long ldu, const void* X, long ldx, void* dA,
                            int accumulate, void* workspace, long workspace_bytes, void* stream);

/* ---- LoRA dropout (kohya-ss network_dropout / rank_dropout / module_dropout; INTEGRATION.md "LoRA dropout"; tests/lora_dropout_ref.py
 *      restates it in numpy) ----------------------------------------------------------------------------------------------------
 * In place on the adapter's inner activation U[rows][parts r] (bf16, row stride ldu; u in the forward pass, du in the backward
 * pass), part p of module id mid_p, sample(row) = row / rows_per_sample:
 *     m[row][p][j] = keep_net[row][p][j] * keep_rank[sample(row)][p][j] * keep_mod[p]                  (each 0 or 1)
 *     U[row][p r + j] = m ? bf16(float(U[row][p r + j]) * inv) : +0.0 (bits 0x0000)
 * A dropped element is SELECTED to +0, never multiplied: a dropped inf or NaN leaves nothing behind.  inv is applied iff t_net or
 * t_rank is nonzero (the caller passes float(1 / ((1 - p_net)(1 - p_rank))) evaluated in double; module dropout is not rescaled).
 * Columns at and beyond parts r are never touched.
 * The random bits: Philox4x32-10 in the layout of the stochastic-rounding write (tests/sr_ref.sr_bits16(seed, step, domain, e)):
 * key = (seed low word, seed high word); counter = (group low word, group high word, step, domain) with group = e >> 3; element e
 * takes the low (e even) or high (e odd) half of output word (e & 7) >> 1.  `step` is the uint32 at step_word, a DEVICE pointer (a
 * native tape and a captured graph replay their scalar arguments unchanged, so the micro-step is read from memory; the module ids
 * go by value for the same reason).  mid = the index of `<module>.weight` in unet_spec.param_table(cfg): a module's masks do not
 * depend on scope, targets or which neighbours are adapted.
 *     keep_net[row][j]   e = (mid << 35) + row r + j                  domain 0x10A1
 *     keep_rank[b][j]    e = (mid << 35) + b r + j                    domain 0x10A2
 *     keep_mod           e = mid << 35                                domain 0x10A3
 * An element is kept iff its 16 bits are >= t, where t = clamp(int(p 65536 + 0.5), 1, 65535) for p > 0; a kind with p = 0 has t = 0,
 * draws nothing and multiplies nothing.  With r % 8 == 0, ldu % 8 == 0 and U 16-byte aligned one thread covers 8 contiguous columns
 * (one 16-byte load, one 16-byte store, one Philox evaluation per kind that is on: such a group never straddles a part or a row);
 * every other shape (rank 4) takes a per-element kernel with the same bits.  All three t = 0 returns 0 without a launch.
 * Argument errors, nothing launched: parts outside 1..3 (-1140); r not one of 4, 8, 16, 32, 64 (-1141); rows <= 0, rows_per_sample
 * <= 0, rows % rows_per_sample != 0 or rows r > 2^35 (-1142); ldu < parts r (-1143); a t outside [0, 65535] (-1144); a null or
 * misaligned step_word or U (-1145); a module id of a used part outside [0, 2^27) (-1146). */
/* ref: not in the reference (train.py is full fine-tuning only); kohya-ss networks/lora.py LoRAModule.forward */
int az_lora_dropout_bf16(int rows, int r, int parts, int rows_per_sample, void* U, long ldu, int mid0, int mid1, int mid2, int t_net,
                         int t_rank, int t_mod, float inv, long seed, const void* step_word, void* stream);

/* ---- LoRA max-norm regularisation (kohya-ss scale_weight_norms; INTEGRATION.md "LoRA max-norm"; tests/lora_maxnorm_ref.py restates
 *      it in numpy) -----------------------------------------------------------------------------------------------------------------
 * After an optimizer step, for every adapted module with A[r][K] ("down", dense; a 3x3 convolution's [r][3][3][Cin] is K = 9 Cin:
 * the norm does not depend on the order of K), B[out][r] ("up", dense) and s = alpha / rank:
 *     G_A = A A^T,  G_B = B^T B            bf16 operands, fp32 accumulation, the summation order is the kernel's own (but fixed)
 *     n2 = s * s * sum_ij G_A[i][j] G_B[i][j]   ( = || s B A ||_F^2 without the product)        norm = sqrtf(n2)
 *     norm > max_norm:  q = sqrtf(max_norm / norm), and every element of A and of B
 *                           x <- bf16(float(x) q)                                    without a master copy
 *                           w <- w q in fp32, x <- bf16(w)                           with one (the norm is still taken from the bf16 values)
 *     otherwise q = 1 and NOTHING of the module is written -- a NaN norm compares false; B = 0 gives norm 0, q = 1 and no NaN.
 * stats[m] = (norm before scaling, q), fp32.  ONE launch serves every module: jobs_dev is a DEVICE table of n_modules rows of eight
 * 64-bit words (address of A, address of B, r, K, out, the fp32 bits of s in the low half, address of the fp32 master copy of A or 0,
 * the same for B), built once by the caller.  r is one of 4, 8, 16, 32, 64; K and out positive multiples of 8 up to 2^24; every
 * address 16-byte aligned.  A row that breaks one of these is skipped by its workgroup -- no byte of it is read or written -- and
 * reports (NaN, 1).  One workgroup per module, no floating-point atomics: the result is a pure function of the inputs.  Elements
 * outside the r K and out r of a module (the padding between slots) are never touched.
 * Argument errors, nothing launched: jobs_dev null or not 8-byte aligned (-1150); n_modules outside [1, 65535] (-1151); max_norm not
 * a positive finite number (-1152); stats null or not 8-byte aligned (-1153). */
/* ref: not in the reference (train.py is full fine-tuning only); kohya-ss networks/lora.py apply_max_norm_regularization */
int az_lora_max_norm_bf16(const void* jobs_dev, int n_modules, float max_norm, void* stats, void* stream);

/* ---- DoRA: weight-decomposed LoRA (Liu et al., arXiv 2402.09353; INTEGRATION.md "DoRA"; tests/dora_ref.py restates it in float64
 *      and in the rounded steps below) ----------------------------------------------------------------------------------------
 * An adapted linear W[N][K], A[r][K], B[N][r], s = alpha / r carries a trainable magnitude m[N] (bf16).  bf16 in memory, sums in fp32:
 *     once per parameter change   n2[o] = sum_k fmaf(s, sum_j B[o][j] A[j][k], float(W[o][k]))^2      (direct form: no cancellation)
 *                                 inv[o] = 1 / sqrtf(n2[o])        g[o] = float(m[o]) * inv[o]         (fp32 vectors, derived state)
 *     forward    v = bf16(x W^T), v = bf16(float(v) + s (u B^T)) (az_lora_up_bf16), y = bf16(fmaf(g[o], float(v), bias[o] or 0) + (float(residual) or 0))
 *     backward   dv = bf16(g[o] * float(dy))       dm[o] = bf16(fmaf(inv[o], sum_rows float(dy[row][o]) float(v[row][o]), float(dm[o])))
 * The norm is a constant of the backward (the paper's section 4.3).  No floating-point atomics: every sum has one fixed order.
 *
 * az_dora_norm_bf16: ONE launch serves every module.  jobs_dev is a DEVICE table of n_modules rows of twelve 64-bit words: the addresses
 *   of W, A, B, m, g, inv; r, K, N; the fp32 bits of s in the low half; the index of the module's first tile (a tile = 64 output rows;
 *   ascending over the table); one unused word.  `tiles` = the tiles of all rows together = the grid.  A workgroup owns a tile and walks
 *   K: the B A tile on v_mfma_f32_16x16x32_bf16 (rank padded by zero fragments), plus W, squared and accumulated per row.  init = 1
 *   also writes m[o] = bf16(sqrtf(n2[o])) (then g = float(m) inv is within 2^-8 of 1 -- bf16 keeps 8 significant bits -- and not exactly 1); init = 0 only reads m.  r is one
 *   of 4, 8, 16, 32, 64; K and N positive multiples of 8 up to 2^24; W, A, B 16-byte aligned and dense ([N][K], [r][K], [N][r]: a 3x3
 *   convolution is not accepted), m 2-byte, g and inv 4-byte aligned.  A row that breaks one of these is skipped by its workgroups:
 *   nothing of W, A, B, m is read or written, and g, inv of the tile's rows are set to NaN where their addresses and N are themselves
 *   well-formed (else nothing at all is touched).  Argument errors, nothing launched: jobs_dev null or not 8-byte aligned (-1160);
 *   n_modules outside [1, 65535] (-1161); tiles outside [1, 2^31 - 16] (-1162); init not 0 or 1 (-1163).
 * az_dora_scale_bf16: Y[M][N] (row stride ldy) from V (ldv), the fp32 gains g[N], bias[N] or NULL, residual (ldr) or NULL, by the
 *   forward rule above -- one fmaf, then the residual's add, then one rounding.  Columns at and beyond N are never touched: Y, V may be
 *   column slices of fused outputs.  N % 8 == 0; every pointer 16-byte aligned, every row stride a multiple of 8 and >= N.  Errors:
 *   M, N (-1164); a null or misaligned pointer (-1165); a row stride (-1166); more than 2^31 - 16 workgroups (-1167).
 * az_dora_bwd_bf16: one pass over dY (and V): dV by the rule above and, with dm != NULL, fp32 partial column sums of dY * V per row
 *   range in `workspace` (at most 64 ranges, a function of the shapes and workspace_bytes only; N floats per range, -1171 when not even
 *   one fits), then a finish on the same stream that adds them in ascending order and accumulates into dm.  dm == NULL: dV only (V, inv
 *   and workspace are not read).  Same alignment rules as the forward.  Errors: M, N (-1168); pointers (-1169); strides (-1170). */
/* ref: not in the reference (train.py is full fine-tuning only); arXiv 2402.09353 section 4, peft's DoraLinearLayer.get_weight_norm */
int az_dora_norm_bf16(const void* jobs_dev, int n_modules, long tiles, int init, void* stream);
/* ref: not in the reference (same); follows the up product of an adapted projection */
int az_dora_scale_bf16(int M, int N, const void* V, long ldv, const void* g, const void* bias, const void* residual, long ldr, void* Y, long ldy,
                       void* stream);
/* ref: not in the reference (same); in front of the adapter's and the base layer's gradients in the backward of train.py:2765 */
int az_dora_bwd_bf16(int M, int N, const void* dY, long lddy, const void* V, long ldv, const void* g, const void* inv, void* dV, long lddv,
                     void* dm, void* workspace, long workspace_bytes, void* stream);

/* ---- native launch tape: the executor seam (SURVEY.md 8b "az_unet_step") ----------------------------------------------------
 * The step's launch sequence is static (same entry points, pointers, streams and events every step of a resolution bucket).  The
 * host executor records it once; az_tape_play re-issues it from C: entry-point calls (arguments as 64-bit words: int / long by
 * value, float by bit pattern, pointers as integers), hipEventRecord, hipStreamWaitEvent, until a BREAK (kind 3: host logic of the
 * caller runs between two plays) or the end.  kind: 0 = call of entry point `fn` (az_tape_fn_id), 1 = event record (words: event,
 * stream), 2 = stream wait (words: stream, event), 3 = break.  az_tape_play returns the index to resume from (= the number of
 * operations when the tape is done), -2 after a failing operation (az_tape_last_error names it). */
/* ref: train.py:2743-2767 (the loop body whose launch sequence is recorded and replayed) */
int az_tape_fn_id(const char* name);
/* ref: train.py:2743-2767 (same) */
int az_tape_create(void** tape);
/* ref: train.py:2743-2767 (same) */
int az_tape_destroy(void* tape);
/* ref: train.py:2743-2767 (same) */
int az_tape_add(void* tape, int kind, int fn, const void* words, int nwords);
/* ref: train.py:2743-2767 (same) */
long az_tape_play(void* tape, long start);
/* ref: train.py:2743-2767 (same) */
int az_tape_last_error(void* tape, long* index, int* rc);

#ifdef __cplusplus
}
#endif
#endif
