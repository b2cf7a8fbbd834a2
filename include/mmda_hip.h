/*
 * mmda_hip.h - C ABI of libmmda_hip.so: the MI355X (gfx950) hot path of MISA training.
 *
 * The reference (SoyeonHH/MMDA) is 100 % Python and has no FFI: every FLOP is a stock PyTorch module call
 * (SURVEY.md section 8b).  Each entry point below therefore names the reference *call site* whose arithmetic it
 * replaces.  The Python host in mmda_amd/ binds these with ctypes (mmda_amd/_lib.py); INTEGRATION.md shows the
 * binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory unless the name ends in _host
 *   - all matrices row-major fp32; sequences time-major (T,B,d) like the reference (data_loader.py:70-72)
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *   - return 0 on success, negative MMDA_E* on error (no exceptions cross the ABI); the caller owns all buffers
 *   - `mode`: MMDA_F32 = exact fp32 (f32 MFMA, parity 1e-4), MMDA_BF16 = bf16 MFMA operands, fp32 accumulate/state
 */
#ifndef MMDA_HIP_H
#define MMDA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMDA_F32 0
#define MMDA_BF16 1

/* recurrent cell (reference config.py:147 --rnncell, models.py:39: nn.LSTM if 'lstm' else nn.GRU) */
#define MMDA_CELL_LSTM 0
#define MMDA_CELL_GRU 1

#define MMDA_OK 0
#define MMDA_EINVAL (-1)   /* bad argument / unsupported shape */
#define MMDA_ELAUNCH (-2)  /* hipLaunch / runtime error (hipGetLastError text via mmda_last_error) */

/* activation ids (reference config.py:25-27 activation_dict).  Ids 0..7 need no parameters and are accepted wherever an `act` is
 * taken; PReLU and RReLU need mmda_act_params, so only the entry points that carry one accept them (LayerNorm, mmda_act_dropout_*_p,
 * the whole-model API).  Any other id is MMDA_EINVAL everywhere: no entry point reads an unknown id as the identity. */
#define MMDA_ACT_NONE 0
#define MMDA_ACT_RELU 1
#define MMDA_ACT_SIGMOID 2
#define MMDA_ACT_LEAKYRELU 3
#define MMDA_ACT_TANH 4
#define MMDA_ACT_ELU 5
#define MMDA_ACT_HARDTANH 6
#define MMDA_ACT_HARDSHRINK 7
#define MMDA_ACT_PRELU 8          /* nn.PReLU(): x > 0 ? x : a x with ONE learned slope a (mmda_act_params.slope) */
#define MMDA_ACT_RRELU 9          /* nn.RReLU(): x >= 0 ? x : s x; training: s ~ U(lo, hi) per element, else s = (lo + hi) / 2 */
/* Parameters of the two parametrised activations of the reference's activation_dict (config.py:25-27); ignored by the others.
 * slope / dslope: device pointers to the PReLU slope and (backward) its gradient, accumulated with one atomic per row.
 * rand != 0 (training): the RReLU slope of element idx is lo + (hi - lo) * u(seed, site, idx), regenerated in the backward pass.
 * Checked on the host before any launch: MMDA_ACT_PRELU with slope == NULL is MMDA_EINVAL, and so is MMDA_ACT_RRELU unless
 * 0 <= lo <= hi and hi > 0 (a zeroed struct is not a request for ReLU). */
typedef struct mmda_act_params {
  const float* slope; float* dslope;
  float lo, hi; int rand; uint64_t seed; int site;
} mmda_act_params;

const char* mmda_last_error(void);
int mmda_abi_version(void);
/* The GEMM entry points split long reductions over K and combine the slices DETERMINISTICALLY: every slice writes its partial tile
 * into a slab, a reduce launch on the same stream sums the slabs in slice order (no float atomics: two identical calls give
 * identical bits; reference train.py:46-51 asks for reproducible runs).  The slabs live in a scratch buffer the library keeps per
 * stream -- the one exception to "the caller owns every buffer": it is grown on demand (hipMalloc, i.e. during warm-up) and
 * released by this call (or at process exit).  Call it only when no GEMM of this library is in flight. */
int mmda_scratch_release(void);

/* ---------------------------------------------------------------------------------------------- GEMM
 * C[b] = epilogue( opA(A[b] (+A2[b])) * opB(B[b]) + bias[b] + bias2[b] (+ C[b] if accumulate) )
 *   opA: transA=0 -> A is (M,K) row-major with leading dim lda; transA=1 -> A is (K,M) row-major
 *   opB: transB=1 -> B is (N,K) row-major (an nn.Linear weight: y = x W^T); transB=0 -> B is (K,N)
 *   gather: optional int64 row ids: row m of A is A + gather[m]*lda (embedding lookup fused into the GEMM).  Read at m < M only:
 *             the array needs no more than M entries, whatever the tile grid covers.
 *   epilogue: act (MMDA_ACT_*), then optional inverted dropout (p, seed, site) on the result,
 *             then optional gate: C *= (gate[m,n] > 0 ? gate_scale : 0)   (relu/dropout backward)
 *   batch: entry b reads A + b*strideA, B + b*strideB, bias / bias2 / bias_grad + b*strideBias and writes C + b*strideC.  The gate
 *             has no stride of its own: entry b reads gate + b*strideC + m*ldgate + n, so a batched gate lies as its C does (one
 *             batch stride for both, ldgate free).
 * Replaces: every nn.Linear / aten::mm / addmm on the path (models.py:48-55 W_ih, :63-153, :160-161) and their
 * autograd transposes. */
typedef struct mmda_gemm_args {
  int mode, transA, transB, M, N, K, batch;
  const float* A;  int lda;  int64_t strideA;
  const float* A2;                              /* optional, same layout as A */
  const int64_t* gather;                        /* optional, M entries (transA must be 0) */
  const float* B;  int ldb;  int64_t strideB;
  float* C;        int ldc;  int64_t strideC;
  const float* bias; const float* bias2; int64_t strideBias;
  int accumulate, act;
  float drop_p; uint64_t drop_seed; int drop_site;
  const float* gate; int ldgate; float gate_scale;
  float alpha;                                  /* scales the product before bias/accumulate; 0 is read as 1 */
  float* bias_grad; float* bias_grad2;          /* optional (transA=1 weight-gradient GEMMs): bias_grad[m] += sum_k A[k,m], i.e. the
                                                   column sums of dY come out of the same MFMA pass as a virtual all-ones column
                                                   of B; bias_grad2 receives the same sums (b_ih and b_hh share a gradient) */
} mmda_gemm_args;
/* act: MMDA_ACT_NONE .. MMDA_ACT_HARDSHRINK (no mmda_act_params here: PReLU / RReLU and unknown ids are MMDA_EINVAL).  K must be
 * positive unless the problem is empty (M, N or batch zero); an empty problem launches nothing. */
int mmda_gemm(const mmda_gemm_args* args, void* stream);
/* n independent GEMMs (any mix of shapes / layouts / modes) in one launch; results as n mmda_gemm calls in any order */
int mmda_gemm_grouped(const mmda_gemm_args* args, int n, void* stream);
/* A read-only view of what mmda_gemm (grouped = 0: each of the n problems as a call of its own) or mmda_gemm_grouped (grouped = 1: the
 * list in launches of 16) would launch: rows[i] describes problem i.  Host code only -- no launch, no device call; pointers are
 * validated and inspected for alignment as by the real call but never followed.  The split-K scratch is taken to start 16-byte
 * aligned.  Returns the number of GEMM launches (the reduce launches behind them not counted), or a negative error; capacity < n is
 * MMDA_EINVAL. */
enum { MMDA_GEMM_NONE = -1, MMDA_GEMM_TILE64 = 0, MMDA_GEMM_TILE64TINY = 1, MMDA_GEMM_TILE128 = 2, MMDA_GEMM_GROUPSLOT = 3 };
typedef struct mmda_gemm_plan_row {
  int cls;                           /* MMDA_GEMM_*: the 64 x 64 tile with one k-tile of prefetch / with up to four k-tiles loaded up
                                        front / the 128 x 128 bf16 tile / a slot of the grouped kernel; NONE: an empty problem */
  int mode, ta, tb;                  /* with cls, the kernel instance: MMDA_F32 / MMDA_BF16, transA, transB */
  int tx, ty, sk;                    /* output tiles along n (the bias gradient's column included) and m; K slices */
  int per, last;                     /* k-tiles (of 32) per slice, and of the last slice */
  int ldn;                           /* row length of a split-K slab: N, + 1 with a bias gradient */
  int blocks;                        /* workgroups of the problem: tx * ty * batch * sk */
  int launch;                        /* index of its launch within the call, in issue order (-1: none) */
  int64_t slab_off;                  /* grouped, sk > 1: where its slab starts in the launch's scratch request, in floats */
  int reduce;                        /* the reduce launch behind a split problem: 0 none, 1 scalar form, 2 16-byte form */
} mmda_gemm_plan_row;
int mmda_gemm_plan_describe(const mmda_gemm_args* args, int n, int grouped, mmda_gemm_plan_row* rows, int capacity);

/* ---------------------------------------------------------------------------------------------- bf16-operand GEMM
 * The LSTM-sized GEMMs of the bf16 mode read bf16 operands that are K-MAJOR (rows of A and of B are contiguous along k):
 *   C[M,N] (+)= alpha * A[M,K] * B[N,K]^T + bias + bias2,  fp32 accumulate and output.
 * Leading dimensions are in bf16 elements and must be multiples of 8 (16-byte rows); K may be ragged (k >= K reads as 0 as
 * long as the copies are zero-padded up to a multiple of 8, which mmda_convert_bf16 guarantees).  bias_grad[m] += sum_k A[m,k]
 * (a virtual all-ones row of B).  Operand copies come from mmda_convert_bf16 (plain and/or transposed).  Up to 16 problems go
 * out as one grouped launch; few-tile/long-K problems are split along K with float atomics (C zeroed first if !accumulate). */
typedef struct mmda_gemm_bf16_args {
  int M, N, K;
  const void* A; int lda;            /* bf16 (M, lda) */
  const void* B; int ldb;            /* bf16 (N, ldb) */
  float* C; int ldc;
  const float* bias; const float* bias2;
  float* bias_grad; float* bias_grad2;
  int accumulate; float alpha;       /* alpha 0 is read as 1 */
  /* gate interleave (the LSTM's gate-minor layout, see mmda_lstm_desc.gate_minor): index j of the interleaved axis stands for
   * torch's index orig(j) = (j / 4H) * 4H + (j % 4) * H + (j % 4H) / 4.   perm_n_H = H: bias/bias2 are read at orig(n)
   * (forward: B rows were interleaved by mmda_convert_bf16).  perm_m_H = H: C rows and bias_grad entries are written at
   * orig(m) (weight gradients: A rows are interleaved).  0 = no interleave. */
  int perm_n_H, perm_m_H;
  /* tn = 1: BOTH operands are M/N-major -- A is bf16 (K, lda) with row k holding A[., k] along m, B is bf16 (K, ldb) likewise:
   * C[M,N] (+)= alpha * A^T B, the weight-gradient form dW = dG^T X on the tensors as the backward pass leaves them (no transposed
   * copies: the kernel stages k-rows into LDS and takes its MFMA fragments with the transposing LDS read of gfx950,
   * ds_read_b64_tr_b16).  lda / ldb multiples of 4 (8-byte rows), bases 4-byte aligned; columns m >= M / n >= N of a row may hold
   * anything finite (they only reach outputs that are not stored).  bias_grad then is a virtual all-ones COLUMN n == N of B. */
  int tn;
} mmda_gemm_bf16_args;
int mmda_gemm_bf16_grouped(const mmda_gemm_bf16_args* args, int n, void* stream);
/* A read-only view of what mmda_gemm_bf16_grouped(args, n) would launch: rows[i] describes problem i.  Host code only -- no launch,
 * no device call, no environment: `switches` = {dma_on, dma_stages, dma_min_rows, dma_tall} stands for MMDA_GEMM_DMA,
 * MMDA_GEMM_DMA_STAGES, MMDA_GEMM_DMA_MIN_ROWS and MMDA_GEMM_DMA_TALL (NULL: their defaults 1, 2, 8192, 0).  Pointers are validated
 * and inspected for alignment as by the real call but never followed.  Returns the number of GEMM launches of the call (the one
 * reduce launch behind them, which exists when some sk > 1, not counted), or a negative error; capacity < n is MMDA_EINVAL. */
enum { MMDA_BF16_REG64 = 0, MMDA_BF16_REG128 = 1, MMDA_BF16_DMA128 = 2, MMDA_BF16_DMA256 = 3 };
typedef struct mmda_gemm_bf16_plan_row {
  int cls;                           /* MMDA_BF16_*; -1: an empty problem (M or N zero), nothing is launched for it */
  int mixed;                         /* 1: its launch runs the tn-capable instance of a register-staged class */
  int tx, ty, sk;                    /* output tiles along n (the bias gradient's column included) and m; K slices */
  int per, last;                     /* k-tiles (of 64) per slice, and of the last slice */
  int launch;                        /* index of its launch within the call, in issue order */
} mmda_gemm_bf16_plan_row;
int mmda_gemm_bf16_plan_describe(const mmda_gemm_bf16_args* args, int n, const int switches[4], mmda_gemm_bf16_plan_row* rows,
                                 int capacity);
/* fp32 (rows, cols) matrix with leading dim ld -> bf16 copies: `plain` (rows, ldp) and/or `transposed` (cols, ldt); either may be
 * NULL.  ldp >= round_up(cols,8), ldt >= round_up(rows,8); the padding columns are written as zero.  `gather` (optional int64
 * row ids) reads row ids[r] of `src` instead of row r (embedding lookup).  Up to 16 jobs per launch. */
typedef struct mmda_convert_job {
  const float* src; int ld; int rows, cols;
  const int64_t* gather;
  void* plain; int ldp;
  void* transposed; int ldt;
  int row_perm_H;                    /* H > 0: output row r reads source row orig(r) (gate interleave, see mmda_gemm_bf16_args) */
  int src_bf16;                      /* 1: `src` points at bf16 elements (ld in elements): re-layout (transpose / pad) without conversion */
} mmda_convert_job;
int mmda_convert_bf16(const mmda_convert_job* jobs, int n, void* stream);
int mmda_debug_gemm_dma_mode(int mode);      /* tools/ only: bit 0 = the LDS-DMA kernel skips its MFMA work, bit 1 = its DMA (wrong results) */

/* ---------------------------------------------------------------------------------------------- block-scaled fp8 GEMM (MX)
 * The two feed-forward products of the fusion transformer layer (linear1 128 -> 2048, linear2 2048 -> 128; reference
 * models.py:160-161) on v_mfma_scale_f32_16x16x128_f8f6f4: OCP MX operands -- e4m3 elements, one E8M0 scale per 32 consecutive k
 * (shared exponent floor(log2 amax) - 8, elements clamped to +-448, round to nearest even) -- fp32 accumulate.  BASELINE.json
 * configs[4] ("mixed fp8 fusion GEMMs"); off by default (mmda_misa_set_fusion_fp8).
 * mmda_mx8_quant: fp32 (rows, K) row-major, K a multiple of 128 (16-byte loads when the rows are 16-byte aligned) -> q: rows * K element bytes in the MFMA's
 * operand order ([row][k-step of 128][lane group 0..3][32 bytes]) and s: rows * K / 32 scale bytes ([row][block]).  <= 8 jobs / launch.
 * mmda_gemm_mx8: C (M, N) = act(A (M, K) . B (N, K)^T + bias) * dropout, both operands quantised as above; N a multiple of 16. */
typedef struct mmda_mx8_quant_job {
  const float* src; int ld; int rows, K;
  unsigned char* q; unsigned char* s;
} mmda_mx8_quant_job;
typedef struct mmda_mx8_args {
  int M, N, K;
  const unsigned char* Aq; const unsigned char* As;
  const unsigned char* Bq; const unsigned char* Bs;
  float* C; int ldc;
  const float* bias; int act;
  float drop_p; uint64_t drop_seed; int drop_site;     /* element index m * N + n, as in the f32 path */
} mmda_mx8_args;      /* act: MMDA_ACT_NONE .. MMDA_ACT_HARDSHRINK, anything else is MMDA_EINVAL; M, N, K positive */
int64_t mmda_mx8_quant_bytes(int rows, int K);
int mmda_mx8_quant(const mmda_mx8_quant_job* jobs, int n, void* stream);
int mmda_gemm_mx8(const mmda_mx8_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------- row-skinny f32 GEMM
 * The fusion block's GEMMs have M = B or 6B rows (models.py:63-153,243-249 and their input gradients): one workgroup per
 * 32 x 16 output tile whose eight waves split K, exact f32 MFMA, operands straight from global memory, fixed-order reduction
 * (bitwise reproducible), fused epilogue.  Up to 8 independent problems per launch.
 *   raw   = alpha * ( (A (+A2)) * op(B)  +  A_2nd * op(B_2nd) )          op(B) = B^T (transB=1: B is (N, ldb), y = x W^T)
 *                                                                               or B   (transB=0: B is (K, ldb), dx = dy W)
 *   C[m,n]  = dsig( gate( dropout( act( raw + bias[n] (+ C[m,n] if accumulate) ) ) ) )
 *   C2[m,n] = dsig2( raw (+ C2[m,n] if accumulate) )                        (optional second destination of the same product)
 * gate: v *= gate[m,n] > 0 ? gate_scale : 0 (relu/dropout mask of a stored activation); dsig: v *= s (1 - s), s = dsig[m,n].
 * float4 operand loads are used when the bases are 16-B aligned, ld % 4 == 0 and K % 4 == 0; otherwise scalar loads. */
typedef struct mmda_skinny_args {
  int M, N, K, transB;
  const float* A; const float* A2; int lda;
  const float* B; int ldb;
  int K2; const float* A_2nd; int lda_2nd; const float* B_2nd; int ldb_2nd;   /* optional second product (K2 = 0: none) */
  float* C; int ldc;
  float* C2; int ldc2;
  const float* bias;
  int accumulate; float alpha; int act;                                        /* alpha 0 is read as 1 */
  float drop_p; uint64_t drop_seed; int drop_site;                             /* element index m * N + n */
  const float* gate; int ldgate; float gate_scale;
  const float* dsig; const float* dsig2; int lddsig;
} mmda_skinny_args;
/* act: MMDA_ACT_NONE .. MMDA_ACT_HARDSHRINK, anything else is MMDA_EINVAL; K must be positive. */
int mmda_gemm_skinny(const mmda_skinny_args* args, int n, void* stream);

/* fp32 transposes, up to 20 per launch: dst[c * ldd + r] = src[r * ld + c] for r < rows, c < cols. */
typedef struct mmda_transpose_job { const float* src; int rows, cols, ld; float* dst; int ldd; } mmda_transpose_job;
int mmda_transpose_f32(const mmda_transpose_job* jobs, int n, void* stream);

/* column sums: out[n] += sum_m X[m*ld + n] (and out2[n] += the same, if out2 != NULL)   (bias gradients; atomics) */
int mmda_colsum(const float* X, int ld, int M, int N, float* out, float* out2, void* stream);

/* ---------------------------------------------------------------------------------------------- embedding
 * models.py:47,201 nn.Embedding forward; backward = dense scatter-add (sparse=False). */
int mmda_embed_gather(const float* W, const int64_t* ids, int rows, int dim, float* out, void* stream);
int mmda_embed_scatter_add(float* dW, const int64_t* ids, int rows, int dim, const float* dX, void* stream);
/* Deterministic form of the scatter-add for data-parallel ranks (and any caller that needs run-to-run identical sums):
 *   dW[id] = sum over the list positions p with ids[p] == id of rows[p], added in LIST ORDER (fixed two-level order: runs of <= 64
 * sorted positions, then the runs of a segment); rows of dW whose id occurs are OVERWRITTEN, all others are left alone; ids < 0 are
 * skipped.  ids (n) int64 and rows (n, D) fp32 on the device.  `work`: mmda_embed_segment_sum_work_bytes(n, D) bytes, 256-B aligned.
 * Ranks all-gather (ids, rows) and each runs this on the identical gathered list: replicas stay bit-identical, which the atomic
 * scatter-add cannot give (<= T*B rows per rank on the wire instead of V rows). */
int64_t mmda_embed_segment_sum_work_bytes(int n, int D);
int mmda_embed_segment_sum(float* dW, const int64_t* ids, int n, int D, const float* rows, void* work, int64_t work_bytes, void* stream);
/* In-place sum all-reduce of n_floats fp32 values on an RCCL communicator (ncclComm_t passed as void*) -- the data-parallel exchange
 * the reference never had (its only trace: the commented nn.DataParallel, solver.py:88-91) for hosts that own a communicator.
 * ncclAllReduce is resolved at run time (process symbols first, then librccl.so): no link-time dependency. */
int mmda_allreduce(void* buf, size_t n_floats, void* nccl_comm, void* stream);

/* ---------------------------------------------------------------------------------------------- LayerNorm
 * y = LN(act(x) + res * dropmask) * gamma + beta over the last dim n (eps 1e-5).   models.py:155-157,172 and the
 * LayerNorms inside project_* (models.py:65-80) and the fusion layer (torch TransformerEncoderLayer norm1/norm2).
 *   permute_sb > 0: rows are (s,b) with s-major, b < permute_sb... output row (s*Bp + b) is written at
 *   out + b*(S*n) + s*n  (i.e. (S,B,n) -> (B,S,n)), used to emit h = cat(h[0..5],dim=1) (models.py:245).
 *   stash: mean,rstd (rows each). */
typedef struct mmda_ln_args {
  int rows, n;
  const float* x; const float* res;             /* res optional */
  const float* gamma; const float* beta;
  float* y; float* mean; float* rstd;
  int act;                                      /* applied to x before the residual add */
  float drop_p; uint64_t drop_seed; int drop_site;   /* dropout on res */
  int permute_S, permute_B;                     /* 0,0 = no permutation */
  float eps;
  mmda_act_params actp;                         /* act = MMDA_ACT_PRELU / MMDA_ACT_RRELU only */
  void* y_bf16; int ld_bf16;                    /* optional second output (then y may be NULL): y as bf16 (rows, ld_bf16), columns n..ld_bf16-1 zero -- the
                                                 * K-major operand copy the next layer's input GEMM reads (no conversion launch between) */
} mmda_ln_args;
/* act: MMDA_ACT_NONE .. MMDA_ACT_RRELU, with actp as mmda_act_params asks; anything else is MMDA_EINVAL from all five LayerNorm
 * entry points, before any launch. */
int mmda_layernorm_fwd(const mmda_ln_args* a, void* stream);
/* backward: dx_pre = LN'(dy); outputs: d_x = dx_pre * act'(x) (written or accumulated), d_res = dx_pre*dropmask,
 * dgamma += , dbeta += .  dy may be given in permuted (B,S,n) layout (same permute args as forward). */
typedef struct mmda_ln_bwd_args {
  int rows, n;
  const float* dy; const float* x; const float* res; const float* gamma;
  const float* mean; const float* rstd;
  float* d_x; int accumulate_dx; float* d_res;  /* either may be NULL */
  float* dgamma; float* dbeta;                  /* accumulated with atomics */
  int act; float drop_p; uint64_t drop_seed; int drop_site;
  int permute_S, permute_B;
  mmda_act_params actp;                         /* act = MMDA_ACT_PRELU / MMDA_ACT_RRELU only (dslope accumulated when d_x is written) */
} mmda_ln_bwd_args;      /* act / actp: as mmda_ln_args */
int mmda_layernorm_bwd(const mmda_ln_bwd_args* a, void* stream);
/* Several independent LayerNorms in one launch (the three modalities'): results as n single calls. */
int mmda_layernorm_fwd_multi(const mmda_ln_args* args, int n, void* stream);
int mmda_layernorm_bwd_multi(const mmda_ln_bwd_args* args, int n, void* stream);
/* dgamma / dbeta alone (same argument struct; d_x / d_res are ignored).  With dgamma = dbeta = NULL mmda_layernorm_bwd computes
 * only the input gradients, so the parameter gradients of the large inter-layer LayerNorms (rows = T*B) can run on another
 * stream, off the path into the next recurrent kernel. */
int mmda_layernorm_param_grads(const mmda_ln_bwd_args* args, int n, void* stream);

/* ---------------------------------------------------------------------------------------------- biLSTM
 * Recurrent part of nn.LSTM(bidirectional=True) on a packed sequence (models.py:48-55 via extract_features
 * :163-180), PyTorch gate order i,f,g,o, variable lengths (a sample stops updating at t >= len_b; the reverse
 * direction starts at len_b-1), final h written straight into the utterance layout of models.py:203.
 *
 * Weight packing: W_hh (4H,H) of each direction must first be packed into MFMA fragment order with
 * mmda_lstm_pack_whh (once per optimizer step).  Packed sizes from mmda_lstm_packed_bytes. */
int64_t mmda_lstm_packed_bytes(int mode, int H, int which);   /* which: 0 forward, 1 backward, 2 cluster-backward (bf16 only) */
int mmda_lstm_pack_whh(int mode, int H, const float* whh, void* packed_fwd, void* packed_bwd, void* stream);
/* the cluster-backward packing of one matrix (bf16): [(ht*nHT + nt)*2 + ks2][lane][8] */
int mmda_lstm_pack_whh_cluster(int H, const float* whh, void* packed_c, void* stream);
/* n (<= 16) matrices in one launch */
int mmda_lstm_pack_whh_multi(int mode, int n, const int* H, const float* const* whh, void* const* packed_fwd,
                             void* const* packed_bwd /* entries may be NULL: that packing is skipped (as may packed_fwd's, not both) */,
                             void* const* packed_c /* NULL or per-matrix (bf16) */, void* stream);
/* The same packings (bf16 mode) and up to 16 conversion jobs (mmda_convert_bf16) in ONE launch: both depend only on the step's inputs
 * and weights; as two launches on two streams they cost a fork and a cross-stream wait in front of the first recurrent kernel. */
int mmda_lstm_pack_whh_and_convert(int n, const int* H, const float* const* whh, void* const* packed_fwd, void* const* packed_bwd,
                                   void* const* packed_c, const mmda_convert_job* jobs, int njobs, void* stream);
/* ... and up to 20 fp32 transposes (mmda_transpose_f32) in the same launch: the K-major copies of the fusion block's weights that
 * the backward pass reads depend on the weights only, and a launch of their own costs a stream 7 - 15 us for 6 MB of traffic. */
int mmda_lstm_pack_convert_transpose(int n, const int* H, const float* const* whh, void* const* packed_fwd, void* const* packed_bwd,
                                     void* const* packed_c, const mmda_convert_job* jobs, int njobs, const mmda_transpose_job* tjobs,
                                     int ntjobs, void* stream);

typedef struct mmda_lstm_desc {
  int H;
  float* gates;        /* (T,B,2,4H)  in: x W_ih^T + b_ih + b_hh per direction; out: activated i,f,g,o (stash) */
  float* cstash;       /* (T,B,2,H)   cell state after each step (stash).  With gate_minor = 1 the resident kernels keep it
                          batch-minor-by-4, (T, ceil(B/4), 2, H, 4): allocate T * round_up(B,4) * 2 * H floats */
  float* hseq;         /* (T,B,2H)    layer output [fwd H | rev H], zero at padded positions */
  const void* wpack[2];/* packed W_hh per direction (forward packing for fwd, backward packing for bwd) */
  const void* wpack_c[2]; /* backward only, optional: "cluster-backward" packing (mmda_lstm_packed_bytes(mode,H,2)) used by the
                          resident-weights kernel; NULL -> the streaming backward kernel runs */
  float* utt;          /* (B,4H)      final-h destination / its gradient source in backward */
  int layer;           /* 0 or 1: column block (dir*2+layer)*H of utt */
  const float* d_hseq; /* backward only: (T,B,2H) gradient w.r.t. hseq, or NULL */
  void* xchg;          /* optional cluster-exchange buffer of mmda_lstm_xchg_bytes(H,B) bytes, ZEROED once by the caller when
                          allocated.  Non-NULL (all descriptors) + MMDA_BF16 selects the LDS-resident-weights kernels; NULL
                          selects the streaming kernels. */
  uint32_t epoch_base; /* cluster kernels: monotonic epoch counter of descs[0] is used for the launch; the caller advances it by
                          at least T+1 between launches that share an xchg buffer (flags are never reset) */
  int gate_minor;      /* 0: `gates` columns are [dir][gate][unit] (torch's weight_ih row order).  1: [dir][unit][gate], i.e. the four
                          gates of one hidden unit are 16 contiguous bytes: the resident-weights kernels then move them with one
                          16-byte access instead of four 4-byte ones (the address unit, shared by the CU's four waves, is what
                          their per-step stash traffic is bound by).  Only the resident-weights kernels accept 1. */
  int forward_only;    /* forward: 1 = no backward pass will follow (evaluation): the activated gates and the cell states need not be
                          stashed; `gates` / `cstash` contents are then unspecified after the call.  hseq and utt are written as usual.
                          Honoured by the wave-autonomous kernel, ignored (stash written) by the others. */
  int cell;            /* MMDA_CELL_LSTM (0) or MMDA_CELL_GRU.  GRU: the caller pads torch's three gate blocks into the four slots,
                          W_ih / b_ih rows [r; z; n; 0] and W_hh / b_hh rows [r; z; 0; n] (so `gates` slot 2 = x W_in^T + b_in and slot 3 =
                          b_hn), see mmda_gru_pad_params.  Stash after forward: gates = [r, z, n, h W_hn^T + b_hn], cstash = h_t;
                          after backward gates = d[pre_r, pre_z, pre_n, h W_hn^T + b_hn].  Runs on the streaming kernels and on the
                          wave-autonomous resident-weights kernels (H <= 320; gate_minor allowed there), not on the barrier-form
                          resident kernels; all descriptors of one launch share the cell. */
  void* dg_bf16;       /* backward, optional: (T*B, 8H) bf16, the gate gradients rounded to bf16 in the column order of `gates` (the A
                          operand of dX = dG W_ih on the bf16 GEMM; mmda_convert_bf16 with src_bf16 makes its transpose for the
                          weight-gradient GEMMs).  Written only by the wave-autonomous resident kernel with gate_minor = 1; NULL
                          otherwise / ignored by the other kernels, so a caller passes it only when
                          mmda_lstm_resident_applicable() said those kernels will run. */
  int dg_bf16_only;    /* with dg_bf16: 1 = the fp32 gate gradients are NOT written (`gates` is unspecified after the call): the
                          per-step stores are what the backward kernel's memory pipeline is busy with */
} mmda_lstm_desc;
int64_t mmda_lstm_xchg_bytes(int H, int B);
/* 1 if mmda_lstm_fwd/bwd would run these descriptors on the resident-weights kernels (so gate_minor = 1 may be used), else 0 */
int mmda_lstm_resident_applicable(int mode, int n, const mmda_lstm_desc* descs, int B, int T, int backward);
/* 1 if mmda_lstm_bwd on these descriptors will write mmda_lstm_desc.dg_bf16 (wave-autonomous resident kernel, gate_minor = 1) */
int mmda_lstm_bwd_emits_dg_bf16(int mode, int n, const mmda_lstm_desc* descs, int B, int T);
/* A read-only view of what mmda_lstm_fwd (backward = 0) / mmda_lstm_bwd (backward = 1) would run for these descriptors in bf16 mode
 * on the resident-weights kernels.  Host code only: no launch and no environment; descriptor pointers are checked for NULL as the
 * real call checks them (xchg, wpack_c, dg_bf16, d_hseq) and never followed.  `switches` = {no_quad, quad_cap}: no_quad stands for
 * MMDA_LSTM_NO_QUAD; quad_cap > 0 is the most workgroups a four-waves-per-tile launch may hold, quad_cap = 0 asks the runtime for it
 * as a launch does (an occupancy query: the only device call, and only for a gate-minor wave-sized plan); NULL = {0, 0}.
 * Returns MMDA_OK with plan->ok = 0 where the streaming kernels would run instead (every other field then 0, kernel -1). */
enum { MMDA_LSTM_FORM_BARRIER = 0, MMDA_LSTM_FORM_WAVE = 1, MMDA_LSTM_FORM_QUAD = 2 };
enum { MMDA_LSTM_DHSEQ_RUNTIME = 0, MMDA_LSTM_DHSEQ_ABSENT = 1, MMDA_LSTM_DHSEQ_PRESENT = 2 };
/* the kernel instances of lstm_barrier.hip, lstm_wave.hip and lstm_quad.hip, ordered by form, then pass, then specialisation
 * (mmda_lstm_kernel_name gives the C++ name) */
enum {
  MMDA_LSTM_K_FWD_BARRIER_GM = 0, MMDA_LSTM_K_FWD_BARRIER, MMDA_LSTM_K_BWD_BARRIER_GM, MMDA_LSTM_K_BWD_BARRIER,
  MMDA_LSTM_K_FWD_WAVE_GM_NOSTASH, MMDA_LSTM_K_FWD_WAVE_GM, MMDA_LSTM_K_FWD_WAVE, MMDA_LSTM_K_FWD_WAVE_GRU_GM, MMDA_LSTM_K_FWD_WAVE_GRU,
  MMDA_LSTM_K_BWD_WAVE_ABSENT_PAIR, MMDA_LSTM_K_BWD_WAVE_ABSENT, MMDA_LSTM_K_BWD_WAVE_PRESENT_PAIR, MMDA_LSTM_K_BWD_WAVE_PRESENT,
  MMDA_LSTM_K_BWD_WAVE_GM, MMDA_LSTM_K_BWD_WAVE, MMDA_LSTM_K_BWD_WAVE_GRU_GM, MMDA_LSTM_K_BWD_WAVE_GRU,
  MMDA_LSTM_K_STAMPED,               /* mmda_debug_set_lstm_stamps: one entry for the forward and the backward debug kernel (wave form) */
  MMDA_LSTM_K_FWD_QUAD_NOSTASH, MMDA_LSTM_K_FWD_QUAD, MMDA_LSTM_K_FWD_QUAD_GRU_NOSTASH, MMDA_LSTM_K_FWD_QUAD_GRU,
  MMDA_LSTM_K_BWD_QUAD_PRESENT, MMDA_LSTM_K_BWD_QUAD_ABSENT, MMDA_LSTM_K_BWD_QUAD, MMDA_LSTM_K_BWD_QUAD_GRU,
  MMDA_LSTM_K_COUNT
};
typedef struct mmda_lstm_plan {
  int ok;                            /* 1: the resident-weights kernels run */
  int form, wpb;                     /* MMDA_LSTM_FORM_*; waves per block (wave form: 1, 2 or 4; quad: 1 tile per block; barrier: 4) */
  int groups, groups_per_launch, launches;   /* 32-sample batch groups, how many a launch takes (<= groups), launches of the call */
  int wg_per_group;                  /* workgroups of one batch group, both directions, all descriptors */
  int wg_per_desc[4];                /* ... and of each descriptor */
  int gru, gate_minor, no_stash;
  int dhseq;                         /* MMDA_LSTM_DHSEQ_*: what the backward instance knows about d_hseq at compile time */
  int pair;                          /* 1: the instance that runs pre-reduces the partial dh tiles of a producer pair (PAIR = 1) */
  int kernel;                        /* MMDA_LSTM_K_* */
} mmda_lstm_plan;
int mmda_lstm_plan_describe(int n, const mmda_lstm_desc* descs, int B, int T, int backward, const int switches[2], mmda_lstm_plan* plan);
/* C++ name of instance `kernel` (MMDA_LSTM_K_*), NULL beyond the last */
const char* mmda_lstm_kernel_name(int kernel);
/* diagnostics only: 8 x uint64 per workgroup, phase cycle sums of the resident-weights forward kernel (NULL disables) */
int mmda_debug_set_lstm_stamps(void* device_buffer);
/* up to 4 independent biLSTMs (modalities) in ONE launch; all share B, T and lengths (device int32, B entries) */
int mmda_lstm_fwd(int mode, int n, const mmda_lstm_desc* descs, int B, int T, const int32_t* lengths, void* stream);
/* backward: reads gates/cstash (forward stash), utt = d(utterance), d_hseq; overwrites `gates` with d(pre-activation)
 * (zero at padded positions) for the time-batched weight/input gradient GEMMs. */
int mmda_lstm_bwd(int mode, int n, const mmda_lstm_desc* descs, int B, int T, const int32_t* lengths, void* stream);

/* GRU parameters <-> the four-slot layout the recurrent kernels and the time-batched GEMMs work on (mmda_lstm_desc.cell).
 * torch side (per direction d): w_ih[d] (3H, D), w_hh[d] (3H, H), b_ih[d] (3H), b_hh[d] (3H), gate blocks r, z, n (nn.GRU).
 * padded side: pw_ih (8H, D) rows [dir][r; z; n; 0], pw_hh[d] (4H, H) rows [r; z; 0; n], pb_ih / pb_hh (8H) alike.
 * mmda_gru_pad_params : padded <- torch.
 * mmda_gru_unpad_grads: the same pointers name GRADIENTS: torch-side += padded, padded <- 0.  The padded bias gradient is ONE
 *   vector, pb_ih (8H) = column sums of the four-slot gate gradients (what the weight-gradient GEMMs emit); it feeds both b_ih
 *   (slots r, z, n) and b_hh (slots r, z and the fourth); pb_hh is not read.  Rows of the padded weight gradients that have no
 *   torch gate (W_ih slot 4, W_hh slot 3) hold by-products of the padded GEMMs and are dropped. */
#define MMDA_GRU_PAD_MAX 6
typedef struct mmda_gru_pad_job {
  int H, D;
  float* w_ih[2]; float* w_hh[2]; float* b_ih[2]; float* b_hh[2];
  float* pw_ih; float* pw_hh[2]; float* pb_ih; float* pb_hh;
} mmda_gru_pad_job;
int mmda_gru_pad_params(const mmda_gru_pad_job* jobs, int n, void* stream);
int mmda_gru_unpad_grads(const mmda_gru_pad_job* jobs, int n, void* stream);

/* ---------------------------------------------------------------------------------------------- fusion attention
 * Self-attention core of nn.TransformerEncoderLayer(d_model=E, nhead) on (S,B,E) with S small (6): softmax(QK^T/sqrt(hd))V
 * per (sample, head), attention-prob dropout.  qkv: (S*B, 3E) rows (s,b); ctx: (S*B, E); probs: (B,nhead,S,S). */
int mmda_attn_fwd(const float* qkv, int S, int B, int E, int nhead, float* ctx, float* probs,
                  float drop_p, uint64_t seed, int site, void* stream);
int mmda_attn_bwd(const float* qkv, const float* probs, const float* dctx, int S, int B, int E, int nhead,
                  float* dqkv, float drop_p, uint64_t seed, int site, void* stream);

/* ---------------------------------------------------------------------------------------------- elementwise
 * y = a + b */
int mmda_add(const float* a, const float* b, float* y, int64_t n, void* stream);
/* d *= y*(1-y)  (sigmoid backward, in place) */
int mmda_sigmoid_bwd_inplace(float* d, const float* y, int64_t n, void* stream);
/* h = dropout(act(z));  dz = dh * dropmask * act'(z)   (discriminator hidden layer, models.py:124-126) */
int mmda_act_dropout_fwd(const float* z, float* h, int64_t n, int act, float drop_p, uint64_t seed, int site, void* stream);
int mmda_act_dropout_bwd(const float* dh, const float* z, float* dz, int64_t n, int act, float drop_p, uint64_t seed, int site,
                         void* stream);
/* the same for the parametrised activations (MMDA_ACT_PRELU / MMDA_ACT_RRELU): parameters in *ap (host struct, copied; may be NULL for
 * ids 0..7).  act outside MMDA_ACT_NONE .. MMDA_ACT_RRELU, or parameters that mmda_act_params rules out: MMDA_EINVAL.  The two entry
 * points above pass ap = NULL, so they accept ids 0..7. */
int mmda_act_dropout_fwd_p(const float* z, float* h, int64_t n, int act, const mmda_act_params* ap, float drop_p, uint64_t seed, int site,
                           void* stream);
int mmda_act_dropout_bwd_p(const float* dh, const float* z, float* dz, int64_t n, int act, const mmda_act_params* ap, float drop_p,
                           uint64_t seed, int site, void* stream);

/* ---------------------------------------------------------------------------------------------- heads + losses
 * logits12 (B,12) = h [W_conf;W_cls]^T + b.  tcp = sigmoid(logits[:, :6]); scores = sigmoid(dropout(logits[:,6:]));
 * labels = scores > threshold.   models.py:138-153,247-249, functions.py:112-115 */
int mmda_heads_fwd(const float* logits, int B, int ncls, float threshold, float* tcp, float* scores, float* labels,
                   float drop_p, uint64_t seed, int site, void* stream);
/* dlogits from dscores/dtcp (either may be NULL = zero) */
int mmda_heads_bwd(const float* tcp, const float* scores, const float* dtcp, const float* dscores, int B, int ncls,
                   float* dlogits, float drop_p, uint64_t seed, int site, void* stream);
/* The same pair under a task.  MMDA_TASK_EMOTION: the two calls above.  MMDA_TASK_SENTIMENT: the score columns are regression outputs,
 * scores = dropout(logits[:, 6:]) with no sigmoid (the reference's classifier is Linear, Dropout, Sigmoid: the task drops the last stage)
 * and dlogits = dscores * dropout with no s (1 - s); tcp, labels = scores > threshold and the six confidence columns are as above. */
#define MMDA_TASK_EMOTION 0
#define MMDA_TASK_SENTIMENT 1
int mmda_heads_fwd_task(const float* logits, int B, int ncls, float threshold, float* tcp, float* scores, float* labels,
                        float drop_p, uint64_t seed, int site, int task, void* stream);
int mmda_heads_bwd_task(const float* tcp, const float* scores, const float* dtcp, const float* dscores, int B, int ncls,
                        float* dlogits, float drop_p, uint64_t seed, int site, int task, void* stream);

/* Every loss entry point computes the loss value AND d(loss)/d(inputs) in one pass ("gradient in forward").
 * `scale` multiplies the gradients (loss weight); *loss gets the UNscaled value added (zero it first).
 * Gradients are ACCUMULATED into the d_* buffers.
 * cls: solver.py:373-385   sum_c mean_b BCE (log clamp -100) */
int mmda_loss_cls(const float* scores, const float* emo, int B, int ncls, float scale, float* loss, float* dscores, void* stream);
/* The classification criterion beyond the reference's plain BCE: a positive-class weight w_c >= 0 and a focusing exponent g,
 *   l(s, y) = -( w_c y (1-s)^g lp + (1-y) s^g lq ),  lp = max(log s, -100), lq = max(log1p(-s), -100);  cls = sum_c mean_b l
 *   dl/ds   = - w_c y ( (1-s)^g / max(s, 1e-12) - g (1-s)^(g-1) lp ) + (1-y) ( s^g / max(1-s, 1e-12) - g s^(g-1) lq )
 * g = 0: F.binary_cross_entropy(s, y, weight = y w + (1 - y)); w = 1: the focal loss on probabilities; both: the plain criterion.
 * focal_gamma: 0, or 1 .. 8 (between 0 and 1 the gradient diverges where the loss vanishes: refused).  n_weights: 0 (every weight 1)
 * or ncls, which is then at most 16; pos_weight[c] finite and >= 0.  A NULL mmda_cls_opts* stands for the plain criterion everywhere;
 * so does {0, 0}, and both run the expressions the entry points without _opts have always run.  Anything else: MMDA_EINVAL, no launch. */
typedef struct mmda_cls_opts { float focal_gamma; int n_weights; float pos_weight[16]; } mmda_cls_opts;
int mmda_loss_cls_opts(const float* scores, const float* emo, int B, int ncls, float scale, float* loss, float* dscores,
                       const mmda_cls_opts* opts, void* stream);
/* The sentiment task's criterion, a mean over the batch as nn.L1Loss / nn.MSELoss(reduction="mean") over a (B,) column (config.py's
 * criterion_dict['mosi'] = 'L1Loss'; the commented nn.L1Loss of solver.py):
 *   MMDA_SENTI_L1   l = |s - y|,    dl/ds = sign(s - y), 0 where s == y (torch's l1_loss backward)
 *   MMDA_SENTI_MSE  l = (s - y)^2,  dl/ds = 2 (s - y)
 * *loss += sum_c mean_b l; dscores += scale * dl/ds / B (each optional). */
#define MMDA_SENTI_L1 0
#define MMDA_SENTI_MSE 1
int mmda_loss_reg(const float* scores, const float* y, int B, int ncls, int kind, float scale, float* loss, float* dscores, void* stream);
/* conf: solver.py:451-462 */
int mmda_loss_conf(const float* scores, const float* tcp, const float* emo, int B, int ncls, float scale,
                   float* loss, float* dscores, float* dtcp, void* stream);
/* diff: solver.py:422-441 + functions.py:54-78.  x: 6 tensors (B,D) at x + k*stride, order
 * [private_t, private_v, private_a, shared_t, shared_v, shared_a]; the six reference pairs are built in. */
int mmda_loss_diff(const float* x, int64_t stride, int B, int D, float scale, float* loss, float* dx, float* work, void* stream);
int64_t mmda_loss_diff_work_floats(int B, int D);
/* general form: nt (2..6) tensors at x + k*stride, np (1..6) index pairs (host array of 2*np ints).  The utils.DiffLoss
 * module call DiffLoss()(a, b) (functions.py:54-78) is nt=2, pairs={0,1}. */
int mmda_loss_diff_pairs(const float* x, int64_t stride, int nt, int np, const int* pairs_host, int B, int D, float scale,
                         float* loss, float* dx, float* work, void* stream);
/* cmd: solver.py:409-420 + functions.py:88-109 over shared_t, shared_v, shared_a = x + k*stride (k=0..2), 5 moments */
int mmda_loss_cmd(const float* x, int64_t stride, int B, int D, float scale, float* loss, float* dx, void* stream);
/* general form: nt (2..3) tensors, np (1..6) pairs, n_moments (1..5), D <= 512; *loss += value_scale * sum over pairs; gradients are
 * scaled by scale*value_scale.  utils.CMD()(x1, x2, n) (functions.py:88-109) is nt=2, pairs={0,1}, value_scale=1. */
int mmda_loss_cmd_pairs(const float* x, int64_t stride, int nt, int np, const int* pairs_host, int n_moments, int B, int D,
                        float scale, float value_scale, float* loss, float* dx, void* stream);
/* recon: solver.py:443-449.  recon/orig: 3 tensors (B,D) each at +k*stride */
int mmda_loss_recon(const float* recon, const float* orig, int64_t stride, int B, int D, float scale, float* loss,
                    float* drecon, float* dorig, void* stream);
/* domain: solver.py:388-407.  dom: (3,B,3) logits stacked t,v,a; labels 0/1/2 */
/* cls + conf (ConfidNet, ncls == 6 only, with_conf) + recon over n_recon contiguous elements in ONE launch, plus the weighted
 * total L[5] = L[0] + diff_w L[1] + sim_w L[2] + recon_w L[3] (+ conf_w L[4] if use_conf) written by the last block to finish.
 * L: 8 floats {cls, diff, sim, recon, conf, total, -, ticket}; L[0], L[3], L[4], L[7] must be zero on entry, L[1], L[2] final.
 * Gradients (optional) are ADDED to d_scores / d_tcp (atomics: cls and conf share d_scores) and d_recon / d_orig.
 * Replaces: solver.py:165-181 (the criterion, get_conf_loss, get_recon_loss calls and the weighted sum). */
int mmda_loss_misc(const float* scores, const float* tcp, const float* emo, int B, int ncls, float* d_scores, float* d_tcp,
                   int with_conf, int conf_grads, float conf_scale, const float* recon, const float* orig, int64_t n_recon,
                   float recon_scale, float* d_recon, float* d_orig, float* L, float diff_w, float sim_w, float recon_w,
                   float conf_w, int use_conf, void* stream);
/* the same launch with the classification term under `opts` (NULL: mmda_loss_misc) */
int mmda_loss_misc_opts(const float* scores, const float* tcp, const float* emo, int B, int ncls, float* d_scores, float* d_tcp,
                        int with_conf, int conf_grads, float conf_scale, const float* recon, const float* orig, int64_t n_recon,
                        float recon_scale, float* d_recon, float* d_orig, float* L, float diff_w, float sim_w, float recon_w,
                        float conf_w, int use_conf, const mmda_cls_opts* opts, void* stream);
/* Positives per class of an (N, C) fp32 label table, an entry counting as set when > 0 (the convention of mmda_eval_accumulate),
 * ADDED into counts[C] (device, 64-bit, zeroed by the caller): one launch, integer sums throughout, so the result is exact and the
 * same on every run.  1 <= C <= 16, N >= 0 (N == 0: MMDA_OK, no launch).  What mmda_amd.class_pos_weight turns into (N - n_c) / n_c. */
int mmda_label_counts(const float* emo, int64_t N, int C, int64_t* counts, void* stream);
/* Evaluation counts on the device (reference utils/eval.py:14-31 get_accuracy and the tp/fp/fn that sklearn's
 * f1/precision/recall in get_metrics :33-65 are functions of), ACCUMULATED into `state` = 3*C + 2 doubles (zeroed by the caller
 * before the first batch): tp[C], fp[C], fn[C], sum_i |y_i & p_i| / max(|y_i | p_i|, 1), number of samples.  pred / truth are
 * (N, C) fp32, an entry counts as set when > 0.  C <= 16.  One read-back per evaluation pass instead of one per batch. */
int mmda_eval_accumulate(const float* pred, const float* truth, int N, int C, double* state, void* stream);
int mmda_loss_domain(const float* dom, int B, float scale, float* loss, float* ddom, void* stream);
/* A read-only view of which kernel form the loss entry points above pick for a shape.  Host code only: no launch, no device call.
 * The launchers take their decisions from the same functions, so what this reports is what runs.
 *   B, D               rows and columns of one tensor
 *   have_loss, have_dx whether the call passes `loss` / `dx` (NULL or not)
 *   cmd_nt             tensors of the CMD call (2..3; the stream form launches one workgroup per tensor when dx is given)
 *   n_recon            elements of the recon call; <= 0 stands for 3 * B * D (the model's three contiguous tensors) */
enum { MMDA_LOSS_DIFF_GENERIC = 0, MMDA_LOSS_DIFF_FAST4, MMDA_LOSS_DIFF_FAST8, MMDA_LOSS_DIFF_FAST16, MMDA_LOSS_DIFF_FAST32 };
enum { MMDA_LOSS_DIFF_SKINNY = 0, MMDA_LOSS_DIFF_BATCHED = 1 };
enum { MMDA_LOSS_DIFF_SUM_NONE = 0, MMDA_LOSS_DIFF_SUM_FINISH, MMDA_LOSS_DIFF_SUM_OWN_LAUNCH };
enum { MMDA_LOSS_CMD_FAST4 = 0, MMDA_LOSS_CMD_FAST8, MMDA_LOSS_CMD_STREAM, MMDA_LOSS_CMD_SERIAL, MMDA_LOSS_CMD_REJECT };
typedef struct mmda_loss_forms {
  int diff_form;                     /* MMDA_LOSS_DIFF_GENERIC / FAST*: the prep and the finish kernel */
  int diff_products;                 /* MMDA_LOSS_DIFF_SKINNY (row-skinny launches) or MMDA_LOSS_DIFF_BATCHED (one mmda_gemm) */
  int diff_loss_sum;                 /* MMDA_LOSS_DIFF_SUM_*: who adds the combine launch's loss partials (NONE: loss == NULL) */
  int diff_combine_blocks;           /* workgroups of the combine launch = loss partials */
  int cmd_form;                      /* MMDA_LOSS_CMD_*; REJECT: the call returns MMDA_EINVAL */
  int cmd_grid;                      /* workgroups of the CMD launch (0 when rejected) */
  int recon_blocks;                  /* workgroups of mmda_loss_recon's launch over n_recon contiguous elements */
  int misc_recon_blocks;             /* recon workgroups of mmda_loss_misc for n_recon elements */
} mmda_loss_forms;
int mmda_loss_forms_describe(int B, int D, int have_loss, int have_dx, int cmd_nt, int64_t n_recon, mmda_loss_forms* out);

/* ---------------------------------------------------------------------------------------------- threshold calibration
 * The decision is labels = scores > threshold (reference models.py:249).  A sweep counts, for EVERY cut-off of a grid at once, what
 * get_metrics / get_accuracy (utils/eval.py:14-65) are functions of -- in integers, so the result is the same bits on every run.
 *   pos(i,c) = truth[i,c] > 0;  bin(s) = #{k : s > thr[k]} in 0..K for a strictly increasing fp32 grid thr[0..K) (NaN: bin 0);
 *   "predicted at cut-off k" = bin > k = s > thr[k].
 * mmda_calib_accumulate ADDS into hist[C][K+1][2] (hist[c][j][p]: rows with bin(scores[i,c]) == j and pos(i,c) == p) and, where pairs
 * is given, into pairs[K][C+1][C+1] (pairs[k][a][b]: rows with |y & p| == a and |y | p| == b at cut-off k); both are zeroed by the
 * caller before the first batch.  scores / truth (N, C) fp32 and thr are device pointers.  1 <= C <= 16, 1 <= K <= 256, N >= 0
 * (N == 0: MMDA_OK, no launch); a NULL among scores / truth / thr / hist or a bound violation is MMDA_EINVAL before any launch. */
int mmda_calib_accumulate(const float* scores, const float* truth, int64_t N, int C, const float* thr, int K,
                          unsigned long long* hist, unsigned long long* pairs, void* stream);
/* One workgroup, no read-back: tp / fp per cut-off as suffix sums of hist, fn from the class's positives, fp64 in a fixed order.
 * table (optional, K x 10 doubles): the reference's ten figures {acc, f1, precision, recall, micro_*, weighted_*} with ONE cut-off k
 * for all classes, zero where a denominator is zero; acc = sum pairs[k][a][b] a (720720 / max(b, 1)) / (720720 N), unrounded, NaN
 * where pairs is NULL.  out_thr[C], out_k[C] (device): the cut-off that maximises `objective`, ties to the lowest k; per_class = 1
 * (objectives F1 and WEIGHTED_F1 only): every class takes the k of its own best F1, which maximises both over all per-class
 * assignments on the grid.  MMDA_EINVAL: per_class with MICRO_F1 or ACC; ACC without pairs. */
enum { MMDA_CALIB_F1 = 0, MMDA_CALIB_MICRO_F1 = 1, MMDA_CALIB_WEIGHTED_F1 = 2, MMDA_CALIB_ACC = 3 };
int mmda_calib_select(const unsigned long long* hist, const unsigned long long* pairs, int C, int K, const float* thr, int objective,
                      int per_class, float* out_thr, int32_t* out_k, double* table, void* stream);
/* mmda_eval_accumulate with the labels made inside: scores[i,c] > thr_c[c], thr_c = C device floats.  The same `state`;
 * labels_out (optional) receives the (N, C) 0/1 labels. */
int mmda_eval_accumulate_thr(const float* scores, const float* truth, int N, int C, const float* thr_c, float* labels_out,
                             double* state, void* stream);

/* ---------------------------------------------------------------------------------------------- ranking metrics
 * How well a score table RANKS, before any cut-off is chosen (mmda_amd/ranking.py): per class AUROC, average precision
 * (of the positives, and of the negatives under the negated score) and FPR at a TPR level; per row the label-ranking figures.  All
 * counting is in integers, so the same bits come out on every run.
 *   order: scores compare as fp32 with -0 == +0; a NaN counts as -inf (it ties with other NaNs and with a real -inf).
 *   pos(i,c) = truth[i,c] > 0.
 * mmda_rank_counts OVERWRITES counts[N][C][4] = {gp, gn, ep, en}: among the rows j of class c, the positives / negatives with
 * s_j > s_i (gp, gn) and with s_j == s_i, row i itself included (ep, en).  N^2 C comparisons: 1 <= C <= 16, 0 <= N <= 2^20 and
 * N^2 C <= 2^42, else MMDA_EINVAL (the launch is quadratic; a mistaken call must not hold the device for minutes).
 * mmda_rank_finish: out[(C + 1)][6] doubles {n_pos, n_neg, auroc, ap, ap_neg, fpr_at_tpr} per class, from counts and truth:
 *   ln = n_neg - gn - en, lp = n_pos - gp - ep
 *   auroc      = (2 sum_{i pos} ln_i + sum_{i pos} en_i) / (2 n_pos n_neg)            NaN when n_pos == 0 or n_neg == 0
 *   ap         = (1 / n_pos) sum_{i pos} (gp + ep) / (gp + ep + gn + en)              NaN when n_pos == 0
 *   ap_neg     = (1 / n_neg) sum_{i neg} (ln + en) / (ln + en + lp + ep)              NaN when n_neg == 0
 *   fpr_at_tpr = min{gn_i + en_i : i pos, gp_i + ep_i >= need} / n_neg, need = max(1, ceil(tpr_level * (double)n_pos))
 *                                                                                     NaN when n_pos == 0 or n_neg == 0
 * The AUROC numerator and the FPR minimum are integer reductions followed by one fp64 division; the two AP sums are fp64 in a fixed
 * order.  Row C: the means over the classes where a figure is defined, added in class order (NaN where none is); its first two
 * columns hold the number of classes that entered auroc and ap.  0 < tpr_level <= 1, else MMDA_EINVAL.  Two launches, no read-back.
 * mmda_rank_rows_accumulate ADDS one batch of rows into state[2 + 3 (C + 1)] (uint64, zeroed by the caller before the first batch):
 *   state[0] rows, state[1] coverage_sum, then rows_by_P[C + 1], lrap_num[C + 1], bad_sum[C + 1], indexed by P = the row's positives:
 *   with rank_j = #{k : s_k >= s_j} and L_j = #{k positive : s_k >= s_j} over the row's C scores,
 *   lrap_num += sum_{j positive} L_j (720720 / rank_j), bad_sum += sum_{j positive} (rank_j - L_j), coverage_sum += max_{j positive} rank_j.
 * Common to the three: scores / truth (N, C) fp32 device pointers; N == 0: MMDA_OK, no launch and nothing written (the
 * figures of an empty split are the caller's to state); counts 16-byte, out and state 8-byte aligned; a NULL pointer, C outside 1..16, N < 0 or N over the cap above: MMDA_EINVAL before any launch.
 * mmda_rank_plan_describe (host only, the launcher of mmda_rank_counts reads the same function): the launch a shape gets. */
typedef struct mmda_rank_plan {
  int rows_per_wg;                   /* elements i of one class a workgroup owns: one thread each */
  int tile;                          /* rows j staged in LDS at a time, split into a positives and a negatives list */
  int tiles;                         /* ceil(N / tile) */
  int splits;                        /* ranges the j rows are cut into (grid z); > 1: counts is cleared, then 32-bit integer adds */
  int tiles_per_split;
  int grid_x, grid_y, grid_z;        /* row blocks, classes, splits */
  int64_t counts_bytes;              /* N * C * 4 * sizeof(uint32_t) */
} mmda_rank_plan;
int mmda_rank_plan_describe(int64_t N, int C, mmda_rank_plan* out);
int mmda_rank_counts(const float* scores, const float* truth, int64_t N, int C, uint32_t* counts, void* stream);
int mmda_rank_finish(const uint32_t* counts, const float* truth, int64_t N, int C, double tpr_level, double* out, void* stream);
int mmda_rank_rows_accumulate(const float* scores, const float* truth, int64_t N, int C, unsigned long long* state, void* stream);

/* ---------------------------------------------------------------------------------------------- sentiment table
 * The figures of the reference's eval_mosei_senti (src/utils/eval_metrics.py) from one device state, one launch per batch.
 * state: MMDA_SENTI_STATE_WORDS 8-byte words, 8-byte aligned, cleared by the caller before the first batch:
 *   uint64  [0] n  [1] n_nonzero (truth != 0)  [2] Acc-7 hits  [3] Acc-5 hits (rint of the values clipped to +-3 / +-2: half to even, as
 *           np.round)  [4..7] the 2x2 table of (truth >= 0, pred >= 0) over all rows, index 2 * truth bit + pred bit  [8..11] the table of
 *           (truth > 0, pred > 0) over the rows with truth != 0  [12] n_extreme (|truth| > 2)  [13] the launch's ticket, 0 between launches
 *   double  [16] sum |p - t|  [17] the same over the extreme rows  [18] sum p  [19] sum t  [20] sum p^2  [21] sum t^2  [22] sum p t
 * The counts are integer adds and do not depend on how the rows are split into batches; the float64 sums are added in a fixed order
 * (per-workgroup partials, then workgroup order, no float atomic), so the same batches give the same bits on every run.  One state
 * takes launches of one stream at a time.
 * mmda_senti_finish writes MMDA_SENTI_FIGURES doubles: mae, corr (Pearson, clipped to [-1, 1]), acc7 (the reference's 'mult'), acc5,
 * acc2 and f1 (>= 0 over all rows), acc2_non0 and f1_non0 (> 0 over the rows with truth != 0), mae_intensity (over |truth| > 2).  The F1s
 * are sklearn's average='weighted' over the labels present.  NaN where numpy gives NaN: corr of a constant column or a single row,
 * mae_intensity without an extreme row; the two non0 figures are NaN without a non-zero truth, where the reference itself fails. */
#define MMDA_SENTI_STATE_WORDS 24
#define MMDA_SENTI_FIGURES 9
int mmda_senti_accumulate(const float* pred, const float* truth, int64_t N, void* state, void* stream);
int mmda_senti_finish(const void* state, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------- reliability and logit scaling
 * Are the numbers of a score table probabilities (mmda_amd/reliability.py).  prob / target: (N, C) fp32 device tables,
 * y = target > 0.  A NaN prob counts in n_nan[c] and nowhere else; any other value is clamped to [0, 1] (-0 becomes 0).  Its bin is
 * j = min(M - 1, (int)(p * (float)M)): one fp32 multiply, truncated.  1 <= C <= 16, 1 <= M <= 64, at most 2^20 rows per call and per state.
 * state: MMDA_RELIAB_STATE_WORDS(C, M) 8-byte words, 8-byte aligned, cleared by the caller before the first batch:
 *   uint64  [0] the launch's ticket, 0 between launches  [1] unused  [2 + c] n_nan
 *   double  [2 + C + c] sum (p - y)^2   [2 + 2 C + c] sum -[y max(log p, -100) + (1 - y) max(log(1 - p), -100)], logs in float64
 *   uint64  [2 + 3 C + 3 (c M + j) + {0, 1, 2}] cnt, pos, sum_p = sum rint(p 2^40) of bin j of class c
 * The integers do not depend on the order of arrival or on how the rows are split into batches.  The float64 sums use no float atomic:
 * thread (r, c) of a workgroup adds rows 16 (b + k gridDim) + r of class c in row order, the 16 row lanes of a class are added as
 * ((r0 + r1) + (r2 + r3)) per wave and the four waves in order, the workgroups leave partials and the last one to arrive adds them in
 * workgroup order on top of the state: the same batches give the same bits.  At most MMDA_RELIAB_GRID_CAP workgroups; beyond
 * 16 MMDA_RELIAB_GRID_CAP rows a workgroup strides.  One state takes launches of one stream at a time.
 * mmda_reliab_finish: figures (C + 2, MMDA_RELIAB_FIGURES) doubles {n, n_nan, base_rate, mean_p, ece, mce, brier, nll} -- the class rows,
 * row C their means (each column over the classes where it is not NaN, added in class order; NaN where none is), row C + 1 all classes'
 * bins and sums pooled -- and diagram (C, M, 3) doubles {cnt, pos / cnt, sum_p / (2^40 cnt)} (an empty bin: 0, NaN, NaN).
 *   ece = sum_j |pos_j 2^40 - sum_p_j| / (2^40 n), mce = max_j |pos_j 2^40 - sum_p_j| / (2^40 cnt_j): exact integers, one division each.
 *   n = 0: every figure of the row but n and n_nan is NaN.  One workgroup, nothing read back.
 * mmda_scaling_fit: q = sigmoid(a z + b), z = log p' - log1p(-p') in float64 of the fp32 score clamped to [2^-23, 1 - 2^-23], NaN scores
 * left out.  how: MMDA_SCALING_TEMPERATURE fits a (b = 0), MMDA_SCALING_PLATT a and b; per_class: one group per class, else one group
 * of all classes; a group's parameters minimise its mean NLL.  A clear of the work header and a prepare launch (z, the groups' n and
 * positives), then exactly max_iter (1 .. MMDA_SCALING_MAX_ITER) iteration launches: the workgroups leave float64 partials of
 * (NLL, gradient, Hessian) per group in the order above, the last one to arrive adds them in workgroup order and takes one damped
 * Newton step per group -- accept the trial point unless its NLL rose (beyond 2^-43 relative, the rounding of the sum), else go back and
 * raise the damping -- and a group that has converged (max |d mean NLL / d theta| <= 1e-12) or is degenerate is frozen: later launches
 * leave its bits alone, and return at once when every group is frozen.  No workgroup waits for another; nothing is read back.
 * Outputs, per class (a group's values repeated for its classes): a, b doubles -- the last accepted point -- status int32
 * (MMDA_SCALING_OK; MMDA_SCALING_DEGENERATE: no positive or no negative, a = 1, b = 0; MMDA_SCALING_MAXITER), iterations int32 (the
 * evaluations the group took part in).  work: mmda_scaling_work_bytes(N, C) bytes, 8-byte aligned (-1 for a shape out of range).
 * mmda_scaling_apply: out = (float) sigmoid(a_c z + b_c), out of place; NaN stays NaN.
 * Common: N == 0 is MMDA_OK with no launch and nothing written.  MMDA_EINVAL before any launch: a NULL pointer, a misaligned one
 * (8 bytes for state, figures, diagram, work, a, b; 4 for the rest), C, M or N outside the limits, max_iter outside
 * 1 .. MMDA_SCALING_MAX_ITER, an unknown how, work_bytes below mmda_scaling_work_bytes(N, C). */
#define MMDA_RELIAB_MAX_CLASSES 16
#define MMDA_RELIAB_MAX_BINS 64
#define MMDA_RELIAB_MAX_ROWS (1 << 20)
#define MMDA_RELIAB_GRID_CAP 32
#define MMDA_RELIAB_FIGURES 8
#define MMDA_RELIAB_STATE_WORDS(C, M) (2 + 3 * (C) + 3 * (C) * (M))
#define MMDA_SCALING_TEMPERATURE 0
#define MMDA_SCALING_PLATT 1
#define MMDA_SCALING_MAX_ITER 256
#define MMDA_SCALING_OK 0
#define MMDA_SCALING_DEGENERATE 1
#define MMDA_SCALING_MAXITER 2
int mmda_reliab_accumulate(const float* prob, const float* target, int64_t N, int C, int M, void* state, void* stream);
int mmda_reliab_finish(const void* state, int C, int M, double* figures, double* diagram, void* stream);
int64_t mmda_scaling_work_bytes(int64_t N, int C);
int mmda_scaling_fit(const float* prob, const float* target, int64_t N, int C, int how, int per_class, int max_iter, void* work,
                     int64_t work_bytes, double* a, double* b, int32_t* status, int32_t* iterations, void* stream);
int mmda_scaling_apply(const float* prob, const double* a, const double* b, int64_t N, int C, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------- optimizer
 * clip_grad_value_(clip) then Adam (solver.py:185-186, :97-99; betas 0.9/0.999, eps 1e-8, no weight decay), fused over
 * a flat bucket.  step = 1-based step count.  grad_scale multiplies g first (1/world for DP averaging). */
int mmda_clamp_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float clip, float grad_scale, int step, void* stream);
int mmda_clamp(float* g, int64_t n, float clip, void* stream);
/* The same update over the rows of a (rows, dim) table whose mask byte equals `want`; mmda_mark_rows clears a mask of `rows` bytes and
 * sets the bytes of the ids that occur (ids outside [0, rows) are ignored).  The fused training step uses the pair to update the
 * embedding rows a batch does not touch (zero gradient, known from the ids alone) beside the last recurrence -- torch.optim.Adam's dense
 * update (reference solver.py:97-99, nn.Embedding without sparse=True) moves every row with momentum, touched or not -- and only the
 * touched rows after the scatter. */
int mmda_clamp_adam_rows(float* p, const float* g, float* m, float* v, int rows, int dim, const unsigned char* mask, int want, float lr,
                         float beta1, float beta2, float eps, float clip, float grad_scale, int step, void* stream);
int mmda_mark_rows(unsigned char* mask, int rows, const int64_t* ids, int n, void* stream);
/* torch.optim.SparseAdam on the rows of a (table_rows, D) table that an id list touches (embed_update = sparse), fused with the
 * coalescing of the gradient rows: for every distinct id at a non-padding position of `ids` (n = T*B positions; position p = t*B + b
 * is padding when lengths != NULL and t >= lengths[b]; ids outside [0, table_rows) are skipped)
 *   g = clamp(grad_scale * sum of rows[p] over the id's positions in position order, +-clip)
 *   m = b1 m + (1-b1) g,  v = b2 v + (1-b2) g^2,  p -= lr sqrt(1-b2^step)/(1-b1^step) * m / (sqrt(v) + eps)
 * on row id of P, M, V in place.  Untouched rows keep parameter and both moments bit for bit; no dense gradient is written or read.
 * No float atomics: identical bits on every run.  Lists of fewer than 3072 positions run in one launch (the owner workgroup of the
 * short-list scatter), longer ones through the stable sort and the two-level list-order sum of mmda_embed_segment_sum. */
int mmda_embed_rows_sparse_adam(float* P, float* M, float* V, const int64_t* ids, int n, int D, const float* rows, const int32_t* lengths,
                                int B, int table_rows, float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int step,
                                void* stream);
/* Dense Adam on a (table_rows, D) table without a pass over it (embed_update = deferred).  A row whose gradient is zero takes an update
 * that needs nothing but the row and the update's two scalars, so it is applied when the row is next needed.  The caller counts the
 * updates it applies, seq = 1, 2, 3 ... since the reset; the Adam step NUMBER `step` that makes an update's bias corrections is free
 * (it may skip or repeat, as it may for mmda_clamp_adam).  State, owned by the caller on the device:
 *   row_step[table_rows]   seq of the last update each row has taken
 *   step_scalars           mmda_embed_deferred_scalar_floats(window) = 2 * window floats: for each of the last `window` updates s, at
 *                          2 (s % window), the floats mmda_clamp_adam passes its kernel for that update -- lr / (1 - b1^step) and
 *                          1 / sqrt(1 - b2^step), made in double
 * mmda_embed_deferred_reset: every row current, no update counted yet (a new or a loaded table); the next update is seq 1.
 * mmda_embed_rows_dense_adam, seq = the last update's + 1: the rows of the distinct ids at non-padding positions of `ids` (as in
 *   mmda_embed_rows_sparse_adam) first take the updates they missed, then update `seq` with g = the position-order sum of their rows[p] --
 *   through the same arithmetic as mmda_clamp_adam, so that after mmda_embed_rows_flush P, M and V hold the bits mmda_clamp_adam over
 *   the whole table would have left, given the scattered gradient, the same lr, step, clip and grad_scale (> 0) at every update.  beta1,
 *   beta2 and eps must not change while rows are stale.  An update whose seq is a multiple of `window` flushes the table first, so the
 *   ring never loses scalars a row still needs; no other call reads or writes more than the listed rows.  A seq that is not the last
 *   one + 1 gives wrong rows without an error: mmda_misa_* and the Python wrapper count for their callers.
 * mmda_embed_rows_catch_up: the listed rows take the updates they missed up to `upto` (the last seq); one launch, one writer per row
 *   (an integer claim on row_step), no float atomics.  Run it before reading rows of the table.
 * mmda_embed_rows_flush: every stale row takes the updates it missed up to `upto`; with nothing stale nothing is written. */
int64_t mmda_embed_deferred_scalar_floats(int window);
int mmda_embed_deferred_reset(int32_t* row_step, int table_rows, void* stream);
int mmda_embed_rows_dense_adam(float* P, float* M, float* V, int32_t* row_step, float* step_scalars, int window, const int64_t* ids, int n,
                               int D, const float* rows, const int32_t* lengths, int B, int table_rows, float lr, float beta1, float beta2,
                               float eps, float clip, float grad_scale, int seq, int step, void* stream);
int mmda_embed_rows_catch_up(float* P, float* M, float* V, int32_t* row_step, const float* step_scalars, int window, const int64_t* ids,
                             int n, int D, const int32_t* lengths, int B, int table_rows, float beta1, float beta2, float eps, int upto,
                             void* stream);
int mmda_embed_rows_flush(float* P, float* M, float* V, int32_t* row_step, const float* step_scalars, int window, int D, int table_rows,
                          float beta1, float beta2, float eps, int upto, void* stream);
/* clip_grad_value_(clip) + torch.optim.RMSprop with torch's defaults besides lr (alpha 0.99, eps 1e-8, no momentum, not centered):
 * the other entry of the reference's optimizer_dict (config.py:24).  grad_scale as in mmda_clamp_adam. */
int mmda_clamp_rmsprop(float* p, const float* g, float* square_avg, int64_t n, float lr, float alpha, float eps, float clip,
                       float grad_scale, void* stream);
/* Gradient accumulation (config.accum_steps): one optimizer step from the gradients of N micro-batches, with the arithmetic of N
 * data-parallel ranks -- A = ((G_0 + G_1) + G_2) + ..., one fp32 add per element and micro-batch, then mmda_clamp_adam's update with
 * grad_scale = 1/N.  The accumulator is the caller's, outside any workspace.
 * mmda_grad_accumulate: acc[i] = g[i] (first != 0: a plain copy, so the accumulator never needs clearing) or acc[i] = acc[i] + g[i],
 *   i < n.  Any n >= 0; both pointers 16-byte aligned, else MMDA_EINVAL.
 * mmda_clamp_adam_sum: mmda_clamp_adam with the gradient acc[i] + g[i] -- the closing step reads the last micro-batch's gradients where
 *   the backward pass left them instead of adding them into the accumulator first; P, M and V get the bits mmda_grad_accumulate followed
 *   by mmda_clamp_adam over acc would leave, and neither acc nor g is written.  acc == NULL (one micro-batch): mmda_clamp_adam itself.
 * mmda_embed_rows_append (embed_update = sparse): the n = T*B gradient rows (n, D) and ids of a micro-batch copied to position `offset`
 *   of a list of `capacity` positions (ids_out int64[capacity], rows_out (capacity, D)); the id of a padding position (lengths != NULL
 *   and t >= lengths[b], position p = t*B + b) is written as -1, which mmda_embed_rows_sparse_adam skips.  One launch.  MMDA_EINVAL when
 *   offset + n > capacity.  mmda_embed_rows_sparse_adam with lengths = NULL on the concatenated list then updates the rows any micro-batch
 *   touched, with sums in list order. */
int mmda_grad_accumulate(float* acc, const float* g, int64_t n, int first, void* stream);
int mmda_clamp_adam_sum(float* p, const float* acc, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, float clip, float grad_scale, int step, void* stream);
int mmda_embed_rows_append(int64_t* ids_out, float* rows_out, int64_t offset, int64_t capacity, const int64_t* ids, const float* rows,
                           int n, int D, const int32_t* lengths, int B, void* stream);
/* Frozen parameters (requires_grad = False): the updates above over the TRAINABLE RUNS of a bucket only.  A run is a range of bucket
 * floats [begin, begin + len) that trains; what lies between runs is neither loaded nor stored -- P, M, V (square_avg) keep their bits
 * there, and the gradient there may hold anything, NaN included.  Inside the runs P, M and V get the bits of the dense entry
 * (mmda_clamp_adam, mmda_clamp_adam_sum, mmda_clamp_rmsprop) with the same scalars.  Runs begin and end anywhere; a launch works in
 * items, one per 16-byte aligned quad of the bucket that a run touches (16-byte accesses where the quad lies inside the run, single
 * floats at a run's ends), and `first` is the count of the items of the runs in front.
 * mmda_runs_build (host only, no device needed): n ranges, ascending and disjoint inside [0, bucket_floats), as a table of at most n
 *   runs -- empty ranges dropped, touching ranges merged, `first` filled in; returns the table's items (>= 0), *n_out its runs, or
 *   MMDA_EINVAL.  The caller copies the table to the device once per change of the set, not per step.
 * The launches take a DEVICE table -- or a slice of one that starts at a run: `items` is then the slice's own count -- of runs that lie
 * inside the buffers (pointers to bucket offset 0, 16-byte aligned for the Adam forms).  n_runs == 0 or items == 0: nothing is launched. */
typedef struct mmda_run { int64_t begin, len, first; } mmda_run;
int64_t mmda_runs_build(const int64_t* begin, const int64_t* len, int n, int64_t bucket_floats, mmda_run* out, int* n_out);
int mmda_clamp_adam_runs(float* p, const float* g, float* m, float* v, const mmda_run* runs, int n_runs, int64_t items, float lr,
                         float beta1, float beta2, float eps, float clip, float grad_scale, int step, void* stream);
int mmda_clamp_adam_sum_runs(float* p, const float* acc, const float* g, float* m, float* v, const mmda_run* runs, int n_runs,
                             int64_t items, float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int step,
                             void* stream);
int mmda_clamp_rmsprop_runs(float* p, const float* g, float* square_avg, const mmda_run* runs, int n_runs, int64_t items, float lr,
                            float alpha, float eps, float clip, float grad_scale, void* stream);
/* Optimizer settings beyond lr: Adam's betas and eps, weight decay, and a gradient scale that lives on the device.
 *   weight_decay > 0, decoupled == 0 (torch.optim.Adam(weight_decay)): g' = clamp(g grad_scale, +-clip), g'' = fma(wd, p, g'); moments
 *     and update from g''.
 *   weight_decay > 0, decoupled != 0 (torch.optim.AdamW): p <- fma(-(lr wd), p, p) first (lr wd made in double, rounded once), then the
 *     plain update from g' on the decayed p.
 *   scale_dev != NULL: one float on the device; grad_scale * *scale_dev, rounded once, takes grad_scale's place.  The host never reads
 *     it: it is the coefficient mmda_grad_norm wrote in front of this launch on the same stream (clip_grad_norm_).
 * Every rounding is spelled out and the rule is the same element function under every layout below, so an element gets the same bits
 * through the dense launch, a run table and the rows form.  weight_decay == 0 and scale_dev == NULL: the launch, and the bits, of the
 * entries above.  0 <= beta < 1, eps >= 0, weight_decay >= 0, else MMDA_EINVAL.
 * mmda_clamp_adam_opts: what mmda_clamp_adam, _sum, _runs and _sum_runs cover.  acc == NULL: the gradient is g, else acc + g;
 *   runs == NULL with n_runs == items == 0: the dense range of n floats, else the run table (n unused).
 * mmda_clamp_adam_rows_opts: mmda_clamp_adam_rows with the settings. */
typedef struct mmda_adam_opts {
  float beta1, beta2, eps, weight_decay;
  int decoupled;
  const float* scale_dev;
} mmda_adam_opts;
int mmda_clamp_adam_opts(float* p, const float* acc, const float* g, float* m, float* v, int64_t n, const mmda_run* runs, int n_runs,
                         int64_t items, float lr, float clip, float grad_scale, int step, const mmda_adam_opts* opts, void* stream);
int mmda_clamp_adam_rows_opts(float* p, const float* g, float* m, float* v, int rows, int dim, const unsigned char* mask, int want, float lr,
                              float clip, float grad_scale, int step, const mmda_adam_opts* opts, void* stream);
/* torch.nn.utils.clip_grad_norm_ in two halves, nothing of it read by the host.
 * mmda_grad_norm: the global L2 norm of the gradient g (acc != NULL: acc + g, the one fp32 add of mmda_clamp_adam_sum) over n floats,
 *   or -- runs != NULL -- over the runs of a table, where no float outside a run is loaded.  Squares are summed in double (exact
 *   products), per lane, then in a fixed order per wave, per block and over the blocks' partials: no atomics, equal bits on every run.
 *   out2[0] = norm = (float)(grad_scale sqrt(sum)), out2[1] = coef = min(1, max_norm / (norm + 1e-6)) in fp32.  Nothing to sum: 0 and 1.
 *   partials: device doubles, 8-byte aligned, at least mmda_grad_norm_partials(n) (dense) or mmda_grad_norm_partials(items) (runs) of
 *   them (at most 2048); a smaller partials_capacity, max_norm < 0 or g / acc not 16-byte aligned: MMDA_EINVAL.  Two launches.
 * mmda_grad_scale: g[i] *= *scale_dev over n floats or over the runs of a table, in place (one launch): with out2 + 1 of the call
 *   above, clip_grad_norm_'s g.mul_(clip_coef).  mmda_clamp_adam_opts with scale_dev = out2 + 1 and grad_scale = 1 gives the same
 *   update without writing the gradient. */
int64_t mmda_grad_norm_partials(int64_t n_or_items);
int mmda_grad_norm(const float* g, const float* acc, int64_t n, const mmda_run* runs, int n_runs, int64_t items, float max_norm,
                   float grad_scale, double* partials, int64_t partials_capacity, float* out2, void* stream);
int mmda_grad_scale(float* g, int64_t n, const mmda_run* runs, int n_runs, int64_t items, const float* scale_dev, void* stream);

/* ============================================================================================== whole-model API
 * The reference's per-batch loop body (solver.py:139-186) as five calls.  `mmda_misa` is the native runtime object
 * behind mmda_amd.models.MISA: it owns NO device memory - the host binds one flat fp32 parameter bucket (+ grad, Adam
 * m/v buckets of the same size) and one workspace; the library only lays tensors out inside them.
 *
 * Flat bucket layout: all non-embedding parameters first ("dense" part, the RCCL all-reduce bucket), embed.weight last.
 * mmda_misa_param_info enumerates (state_dict key, offset, rows, cols) - keys are exactly the reference's
 * state_dict keys, so reference checkpoints load by name. */
typedef struct mmda_misa mmda_misa;
typedef struct mmda_misa_config {
  int vocab, d_t, d_v, d_a, hidden, ncls;       /* config.embedding_size / visual_size / acoustic_size / hidden_size / num_classes */
  int act;                                      /* MMDA_ACT_* for project_* and the discriminator (config.activation) */
  int use_cmd_sim, use_confidNet;               /* config.use_cmd_sim / use_confidNet */
  float dropout;                                /* config.dropout: classifier + discriminator dropout */
  float fusion_dropout;                         /* nn.TransformerEncoderLayer default 0.1 (not a reference flag) */
  float threshold, reverse_grad_weight;         /* config.threshold, config.reverse_grad_weight */
  float diff_weight, sim_weight, recon_weight, conf_weight;   /* config.py:134-138 */
  int mode;                                     /* MMDA_F32 / MMDA_BF16 for the encoder + fusion GEMMs and the recurrences */
  int rnncell;                                  /* MMDA_CELL_LSTM / MMDA_CELL_GRU (config.rnncell, models.py:39) */
} mmda_misa_config;

int mmda_misa_create(const mmda_misa_config* cfg, mmda_misa** out);
void mmda_misa_destroy(mmda_misa* m);
int mmda_misa_num_params(const mmda_misa* m);
int mmda_misa_param_info(const mmda_misa* m, int i, const char** name, int64_t* offset, int* rows, int* cols);
int64_t mmda_misa_flat_floats(const mmda_misa* m);    /* whole bucket incl. embedding (multiple of 4) */
int64_t mmda_misa_dense_floats(const mmda_misa* m);   /* non-embedding prefix */
int mmda_misa_bind(mmda_misa* m, float* params, float* grads, float* adam_m, float* adam_v);
int64_t mmda_misa_workspace_floats(const mmda_misa* m, int B, int T);
/* A read-only view, in the style of mmda_lstm_plan_describe and mmda_gemm_bf16_plan_describe, of the plan a forward pass over (B, T)
 * batches gets on this handle as it is set now: every choice of a form of the training step, one int per choice (the fields are
 * StepPlan's, csrc/step_plan.h, which documents each).  Host code only: no launch, no device call, no environment; works without a
 * workspace or buffers bound.  req: what the pass is asked to be -- fused: it belongs to mmda_misa_train_step; has_labels: labels are
 * given; has_opt_step: an optimizer step of the kind that may run the background pass over the table follows (from a batch, do_adam,
 * no clip_norm); enc_cached: it starts behind the encoders (mmda_misa_forward_encoded).  mmda_misa_forward is {0, 0, 0, 0}.
 * switches: NULL = the defaults (NOT the process's environment), else MMDA_MISA_STEP_SWITCHES values standing for, in this order,
 *   MMDA_GEMM_TN MMDA_WT_MERGE MMDA_ROW_FUSE MMDA_FFN_FUSE MMDA_LOSS_SEEDS MMDA_FLAG_JOIN MMDA_ZERO_GRAD_SIDE MMDA_FUSED_SPLIT
 *   MMDA_SORT_EARLY MMDA_EMBED_BG MMDA_EMBED_BG_WGS MMDA_EMBED_BG_LATE MMDA_EMBED_BG_LDS
 * (defaults 1 1 1 1 1 1 -1 1 1 1 0 0 1024).  MMDA_EINVAL, with *out untouched: m, req or out NULL, B <= 0, T <= 0, or switches given
 * with another n_switches. */
#define MMDA_MISA_STEP_SWITCHES 13
typedef struct mmda_misa_step_request { int fused, has_labels, has_opt_step, enc_cached; } mmda_misa_step_request;
typedef struct mmda_misa_step_plan {
  int fused, inf, enc_cut, enc_nostash, enc_cached, bfg, gm, kdg, tn_wgrad, want_b, want_c, want_wT, wT_merge, skinny, row_fuse,
      ffn_fuse_fwd, ffn_fuse_bwd, seed_recon, seed_cls, fj_on, fj_fwd, fj_device, zg_here, rec_hoisted, sort_early, embed_update,
      embed_deferred, embed_bg, embed_bg_late, embed_bg_wgs, embed_bg_lds;
} mmda_misa_step_plan;
int mmda_misa_plan_describe(const mmda_misa* m, int B, int T, const mmda_misa_step_request* req, const int* switches, int n_switches,
                            mmda_misa_step_plan* out);
int mmda_misa_set_workspace(mmda_misa* m, float* ws, int64_t floats, int B, int T);
/* The same with the (rare) clears enqueued on `stream`.  The exchange buffers of the recurrences sit at the front of the workspace at
 * offsets that depend on B alone and are cleared only when the buffer or B changes, so a new T per batch (the reference's collate pads
 * to the batch maximum, data_loader.py:70-72) costs no device work; abort words found before a clear stay visible through
 * mmda_misa_cluster_status.  Before handing over a NEW buffer read mmda_misa_cluster_status yourself: the old one is not touched. */
int mmda_misa_set_workspace_async(mmda_misa* m, float* ws, int64_t floats, int B, int T, void* stream);
/* offset (in floats, inside the workspace) of a named activation / activation-gradient; -1 if unknown, and for every name while no
 * workspace is bound. Names (all of them: the table in tensor_offset(), step_plan.hip):
 *   scores labels tcp logits hfused x6 orig recon dom losses grad_norm utt_t utt_v utt_a
 *   d_scores d_tcp d_x6 d_orig d_recon d_dom
 *   pub_begin pub_end (the solver-visible outputs orig .. labels, contiguous)   zero_begin zero_end (the region cleared per step)
 *   hseq1_t hseq1_v hseq1_a (layer-1 hseq, (T,B,2H))   d_x_t (gradient w.r.t. the gathered embedding rows, (T*B, d_t))
 *   xchg_t xchg_v xchg_a (exchange buffers; word 0 of each = its sticky abort word; -1 where a modality has none)
 * x6 = [private_t, private_v, private_a, shared_t, shared_v, shared_a] each (B,hidden); orig/recon = (3,B,hidden);
 * losses = float[8]: cls, diff, sim, recon, conf, total; grad_norm = float[2]: norm, clip coefficient (mmda_misa_set_adam) */
int64_t mmda_misa_tensor_offset(const mmda_misa* m, const char* name);
/* set the mode / loss switches after creation (bench toggles) */
int mmda_misa_set_mode(mmda_misa* m, int mode);
/* bf16 recurrences: 1 (default) = W_hh resident in LDS across a cluster of workgroups, 0 = streamed from L2 every step */
int mmda_misa_set_recurrence(mmda_misa* m, int resident_weights);
/* bf16 mode only: 1 (default) = the LSTM-sized GEMMs read bf16 operand copies made by mmda_convert_bf16 (gemm_bf16.hip);
 * 0 = they stage the fp32 tensors through the generic kernel (same rounding of the operands, different summation order). */
int mmda_misa_set_gemm_operands(mmda_misa* m, int bf16_copies);
/* 1 = forward passes are evaluation passes (no backward follows): the recurrences skip their stash stores and the transposed
 * bf16 copies that only the weight-gradient GEMMs read are not made.  Default 0.  mmda_misa_backward after a forward in this mode
 * returns MMDA_EINVAL. */
int mmda_misa_set_inference(mmda_misa* m, int forward_only);
/* 1 = the forward feed-forward products of the fusion transformer layer (linear1 / linear2) run on block-scaled fp8 operands
 * (mmda_gemm_mx8); their backward stays on the exact f32 path with the stored activations (straight-through).  Default 0. */
int mmda_misa_set_fusion_fp8(mmda_misa* m, int on);
/* How a training step treats embed.weight (config.embed_update): 0 = dense (default: the gradient is scattered into the bucket and
 * dense Adam walks all rows), 1 = sparse (only the rows a batch touches are updated, with torch.optim.SparseAdam's rule: see
 * mmda_embed_rows_sparse_adam; untouched rows keep parameter and moments), 2 = frozen (the table never changes and no gradient for it
 * is computed).  In modes 1 and 2 the gradient bucket that mmda_misa_zero_grad clears and mmda_misa_adam_step / mmda_misa_train_step walk
 * ends at mmda_misa_dense_floats(); no launch of a step reads or writes the whole table.  Mode 1 after mmda_misa_backward or a
 * train step with do_adam = 0: mmda_misa_adam_step applies the rows update from the (ids, lengths) of that backward, which must
 * still be alive.  Other values: MMDA_EINVAL. */
int mmda_misa_set_embed_update(mmda_misa* m, int mode);
/* Frozen parameters (requires_grad = False on the host side).  flags: one byte per parameter in mmda_misa_param_info order, non-zero =
 * trains; n_params must be mmda_misa_num_params().  Host only (no device call): the caller sends the set when it differs from the
 * last one it sent, between steps.  From then on
 *   - every optimizer launch of mmda_misa_train_step, mmda_misa_adam_step and mmda_misa_adam_step_accumulated walks the trainable runs
 *     of its range only (mmda_clamp_adam_runs and kin: the bits of the dense launch inside the runs, not one byte of P, M or V
 *     touched outside them); a range in which nothing trains gets no launch.  The table of runs is copied to the device by the first
 *     such launch after a change, behind a wait for the stream -- the only synchronisation, once per change of the set.
 *   - the frozen ranges of the gradient bucket are unspecified (gradients the pass computes anyway may land there; nothing reads them).
 *   - encoder cut: when every recurrent parameter and the three inter-layer LayerNorms ({t,v,a}layer_norm) are frozen and the table
 *     is -- by its own flag in dense mode, or by mmda_misa_set_embed_update(2) -- mmda_misa_backward stops behind the fusion block: no
 *     backward recurrence, no encoder weight-gradient product, no scatter, no early optimizer pass (mmda_misa_early_grad_floats() is
 *     0), and the forward pass of such a step keeps no encoder stash (mmda_misa_set_cut_forward(m, 1): it stashes all the same).
 *     mmda_misa_backward returns MMDA_EINVAL when the forward pass in front of it was planned under a cut that the set no longer allows.
 * With every flag set (the state after mmda_misa_create) a step is launch for launch what it is without this call.
 * mmda_misa_trainable_info (host only): the trainable runs -- sorted, disjoint, touching ones merged; a tensor's range includes the
 * alignment padding behind it -- up to `capacity` of them in runs[], their number, the floats they cover and whether the cut is on. */
int mmda_misa_set_trainable(mmda_misa* m, const unsigned char* flags, int n_params);
int mmda_misa_trainable_info(const mmda_misa* m, mmda_run* runs, int capacity, int* n_runs, int64_t* trainable_floats, int* encoder_cut_on);
int mmda_misa_set_cut_forward(mmda_misa* m, int keep_stash);
/* Dense mode (mmda_misa_set_embed_update 0) with the table's update deferred (config.embed_update = deferred): the weights dense Adam
 * gives, while no launch of a step reads or writes the whole table -- see mmda_embed_rows_dense_adam.  Binds the caller's device memory
 * (row_step: vocab int32; step_scalars: mmda_embed_deferred_scalar_floats(window) floats; the runtime owns none), marks every row
 * current (one memset on `stream`) and starts counting updates at zero.  From then on every mmda_misa_forward first catches up the rows
 * of its batch, a step's bucket ends at mmda_misa_dense_floats() as in modes 1 and 2, and the optimizer step updates the batch's rows
 * where their sums become final.  The model counts the updates itself, so the `step` numbers of mmda_misa_train_step /
 * mmda_misa_adam_step are as free as in plain dense mode.  Both pointers NULL: deferral off (flush first).
 * MMDA_EINVAL: one pointer NULL, window < 1, or embed_update != 0.  mmda_misa_set_embed_update(1 or 2) unbinds.
 * mmda_misa_embed_deferred_step: after mmda_misa_backward or a train step with do_adam = 0, the rows update of that backward (whose ids
 *   and lengths must still be alive) with the optimizer's own scalars; mmda_misa_adam_step calls it with Adam's defaults.  MMDA_EINVAL
 *   when nothing is bound or no backward is pending.
 * mmda_misa_embed_flush: every stale row of the table takes the updates it missed (required before embed.weight or its moments are read
 * from outside, saved, or handed to another mode); nothing deferred, or no update since the last flush: no launch. */
int mmda_misa_set_embed_deferred(mmda_misa* m, int32_t* row_step, float* step_scalars, int window, void* stream);
int mmda_misa_embed_deferred_step(mmda_misa* m, float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int step,
                                  void* stream);
int mmda_misa_embed_flush(mmda_misa* m, void* stream);
/* Plain dense mode, fused step (mmda_misa_train_step with do_adam = 1): the rows of embed.weight that the batch does not index have a
 * zero gradient, so their Adam step runs as a background pass of `workgroups` workgroups on an internal low-priority stream beside the
 * forward pass, and the step's last optimizer launch walks only the rows the batch does index.  The bits of the dense launch; the step
 * still completes on `stream` only when the pass has.  on = 0: the one dense launch over the whole table; on = 1: the pass in every
 * eligible step (a handle left alone runs it where it pays: batches of up to 32 samples); workgroups = 0: the default throttle; on not
 * 0 / 1, workgroups outside [0, 4096]: MMDA_EINVAL.  Overrides MMDA_EMBED_BG / MMDA_EMBED_BG_WGS for this handle.
 * The pass runs only where the step is eligible: from a batch (not the encoder cache), no norm clip, nothing frozen, embed_update 0
 * without deferral, T > 0, a table of whole 16-byte quads; every other step is launch for launch what it was.
 * One caveat: after a step that returns an error, rows the batch does not index may already have taken the step.
 * mmda_misa_embed_background_active: 1 if the last mmda_misa_train_step ran the pass, else 0 (host only). */
int mmda_misa_set_embed_background(mmda_misa* m, int on, int workgroups);
int mmda_misa_embed_background_active(const mmda_misa* m);
/* Data parallel: the gradient bucket is laid out in the order the backward pass completes it (fusion block, LayerNorms,
 * layer-2 recurrent layers, layer-1 recurrent layers, embedding).  After mmda_misa_backward / mmda_misa_train_step has been
 * ISSUED, the first mmda_misa_early_grad_floats() floats of the bucket are final as soon as an event recorded inside that call
 * fires -- beside the layer-1 backward recurrence, long before the call's last kernel; mmda_misa_wait_early_grads makes `stream`
 * wait for that event, so a collective enqueued on it overlaps the rest of the backward pass.  0 floats = nothing is early. */
int64_t mmda_misa_early_grad_floats(const mmda_misa* m);
int mmda_misa_wait_early_grads(mmda_misa* m, void* stream);
/* 1 (default) = weight-gradient GEMMs run on an internal side stream underneath the recurrent kernels (joined before
 * mmda_misa_backward returns control of `stream`); 0 = everything on `stream` */
int mmda_misa_set_overlap(mmda_misa* m, int side_stream);
/* *aborted_host: bit 0 = a cluster exchange of a recurrence ever timed out, bit 1 = a kernel of the fused training step ever timed
 * out waiting on the device for the other stream's chain (flag joins: e.g. under a tool that serialises dispatches -- run those with
 * MMDA_FLAG_JOIN=0 MMDA_SORT_EARLY=0); results after either are invalid.  Synchronous D2H, off the step path */
int mmda_misa_cluster_status(const mmda_misa* m, int* aborted_host);

/* models.py:282-285 forward.  t_ids (T,B) int64, v (T,B,d_v), a (T,B,d_a) device; lengths (B) int32 device.
 * training != 0 enables dropout with the given seed.  Packs W_hh first (weights may have changed). */
int mmda_misa_forward(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                      int training, uint64_t seed, void* stream);
/* solver.py:163-181: the six losses into `losses`; with_grads != 0 also zeroes and seeds the d_* activation gradients
 * with the weighted loss gradients (loss.backward() seeds). emo (B,ncls) fp32. */
int mmda_misa_losses(mmda_misa* m, const float* emo, int with_grads, void* stream);
/* Data-parallel "global statistics" mode (no reference counterpart: the reference is single-device, where DiffLoss
 * functions.py:64-76, CMD :89-108 and the confidence loss solver.py:451-462 see the whole batch).  on != 0: the next mmda_misa_losses
 * (with_grads) does NOT clear the activation gradients and does not compute DiffLoss / CMD / conf -- the caller has, behind
 * mmda_misa_zero_act_grads, on the all-gathered tensors of every rank with mmda_loss_diff / mmda_loss_cmd / mmda_loss_conf, added
 * the sums into losses[1], [2], [4] and this rank's gradient rows (times the world size: the exchange averages) into d_x6 / d_scores /
 * d_tcp (mmda_misa_tensor_offset).  cls, recon and the weighted total are added as usual. */
int mmda_misa_set_external_batch_losses(mmda_misa* m, int on);
/* solver.py:183 loss.backward(): from d_scores/d_tcp/d_x6/d_orig/d_recon/d_dom to every parameter gradient
 * (ACCUMULATED into the bound grad bucket: zero it first with mmda_misa_zero_grad).  External seeds (the autograd
 * compat path) are whatever the caller left in the d_* buffers. */
int mmda_misa_backward(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                       void* stream);
int mmda_misa_zero_grad(mmda_misa* m, void* stream);
int mmda_misa_zero_act_grads(mmda_misa* m, void* stream);
/* solver.py:185-186: clip_grad_value_(clip) + Adam over the whole bucket; grad_scale = 1/world after an all-reduce
 * (mmda_misa_set_embed_update 1 / 2: over the non-embedding prefix, plus the pending rows update in mode 1) */
int mmda_misa_adam_step(mmda_misa* m, float lr, float clip, float grad_scale, int step, void* stream);
/* The optimizer's settings, kept by the handle: every Adam launch of mmda_misa_train_step(_encoded), mmda_misa_adam_step,
 * mmda_misa_adam_step_accumulated, the sparse rows update and the deferred table's replay reads opts' betas, eps, weight decay and
 * decay kind (opts->scale_dev is not kept).  opts == NULL: the defaults -- betas 0.9 / 0.999, eps 1e-8, no decay -- under which
 * every launch and every bit is what it was without this call.  Decay covers what the dense launch covers: with the sparse table the
 * table's rows follow SparseAdam, which has none.
 * clip_norm > 0 (0 = off): torch.nn.utils.clip_grad_norm_(clip_norm) in front of clip_grad_value_ and the update.  No update may
 *   precede the norm, so a training step then runs its backward pass as it does for do_adam = 0 (no early optimizer pass, event join),
 *   followed by mmda_grad_norm over the gradient bucket (the trainable runs of it when parameters are frozen; acc + G with
 *   grad_scale = 1/N in the accumulated step) and ONE Adam launch over the bucket with scale_dev = the coefficient.  Norm and coefficient
 *   stay in the workspace, two floats at mmda_misa_tensor_offset("grad_norm").
 * MMDA_EINVAL with nothing changed: a beta outside [0, 1), eps < 0, weight_decay < 0, clip_norm < 0, or betas / eps that change while
 *   rows of a deferred table are stale (flush first).
 * The stepping entries return MMDA_EINVAL in front of their first launch for: weight_decay > 0 with the deferred table bound (its
 *   replay ring holds two scalars per update, a decayed zero-gradient step needs a third); clip_norm > 0 with embed_update sparse or
 *   the deferred table (their rows are updated where the row sums become final, before a norm exists). */
int mmda_misa_set_adam(mmda_misa* m, const mmda_adam_opts* opts, float clip_norm);
/* The classification criterion of the handle (mmda_cls_opts above; NULL: the plain one, which is the default).  The handle keeps a
 * copy, and every classification loss it computes follows it: mmda_misa_losses, mmda_misa_train_step, mmda_misa_train_step_encoded,
 * accumulated steps, the loss-value launch a step defers to its backward pass, and the seed the forward stretch stores.  The step's
 * plan does not depend on it: no launch is added or moved.  MMDA_EINVAL with nothing changed and nothing launched: a focal_gamma other
 * than 0 or 1 .. 8, n_weights other than 0 or the model's ncls, weights for more than 16 classes, a negative or non-finite weight. */
int mmda_misa_set_cls_loss(mmda_misa* m, const mmda_cls_opts* opts);
/* The task of the handle.  MMDA_TASK_EMOTION (the default): the classifier above; loss_kind is not read.  MMDA_TASK_SENTIMENT: the
 * model's one score column is a regression output (mmda_heads_fwd_task) and the loss the handle calls cls is mmda_loss_reg's loss_kind
 * (MMDA_SENTI_L1 / MMDA_SENTI_MSE) against the (B, 1) target given where the labels were.  Read when a step begins, at the sites that
 * read the criterion; the step's plan does not depend on it.  MMDA_EINVAL with nothing changed: an unknown task or kind; under the
 * sentiment task a model with ncls != 1 or use_confidNet (the confidence target truth * pred is defined for labels in {0, 1}), or a
 * weighted / focal criterion set -- and mmda_misa_set_cls_loss refuses such a criterion while the task is set. */
int mmda_misa_set_task(mmda_misa* m, int task, int loss_kind);
/* One optimizer step from N micro-batches (config.accum_steps; the arithmetic of mmda_grad_accumulate above).  Every micro-batch is
 * mmda_misa_train_step with do_adam = 0; behind each but the last call mmda_misa_grad_accumulate, behind the last
 * mmda_misa_adam_step_accumulated with grad_scale = 1/N.  The runtime owns none of the memory:
 *   acc        the bucket's length in floats (mmda_misa_flat_floats() in dense mode, mmda_misa_dense_floats() in modes 1 and 2), 16-byte
 *              aligned, never cleared by anyone (first != 0 copies)
 *   list_ids / list_rows   mode 1 (sparse) only, else ignored: int64[list_capacity] and (list_capacity, d_t) floats.  The micro-batch's
 *              T*B rows of d_x_t (workspace: the next micro-batch overwrites them) and its ids, padding as -1, are appended at position
 *              list_used, and the pending rows update of that backward is dropped: a later mmda_misa_adam_step applies nothing stale.
 *              The caller adds T*B to list_used per micro-batch and starts every optimizer step at 0; micro-batches may differ in T and B.
 * mmda_misa_adam_step_accumulated: clip + Adam over the bucket with the gradient acc + current bucket (acc == NULL: one micro-batch, the
 *   current bucket alone); in mode 1 it appends the last micro-batch's rows as above and runs mmda_embed_rows_sparse_adam once on the
 *   list_used + T*B positions of the list.
 * MMDA_EINVAL, with nothing launched: deferral bound (mmda_misa_set_embed_deferred: its contract is dense Adam's bits, which a rows
 * update on a concatenated list does not give), mode 1 without a pending backward or with a list too short, step < 1. */
int mmda_misa_grad_accumulate(mmda_misa* m, float* acc, int first, int64_t* list_ids, float* list_rows, int64_t list_used,
                              int64_t list_capacity, void* stream);
int mmda_misa_adam_step_accumulated(mmda_misa* m, const float* acc, int64_t* list_ids, float* list_rows, int64_t list_used,
                                    int64_t list_capacity, float lr, float clip, float grad_scale, int step, void* stream);
/* zero_grad + forward + losses + backward (+ adam if do_adam) = one reference loop iteration */
int mmda_misa_train_step(mmda_misa* m, const int64_t* t_ids, const float* v, const float* a, const int32_t* lengths,
                         const float* emo, int training, uint64_t seed, int do_adam, float lr, float clip, int step,
                         void* stream);

/* Per-kernel timing of the recurrent launches with HIP events recorded on the SAME stream the kernels run on
 * (bench.py's roofline leg).  begin(max_steps) arms it; every train_step/forward/backward then brackets its four
 * recurrent launches (0: fwd layer1, 1: fwd layer2, 2: bwd layer2, 3: bwd layer1); collect() synchronises the events and
 * returns the mean milliseconds per launch of each and the number of timed steps; end() disarms and frees the events. */
/* record the recurrent kernels' event pairs only on every stride-th step (default 1; set before mmda_misa_timing_begin, whose
 * max_steps then counts RECORDED steps): eight event records per step cost ~35 us of a 1.4 ms step */
int mmda_misa_timing_stride(mmda_misa* m, int stride);
/* on != 0: a sampled step brackets ONE of the four recurrent launches (they take turns): two event records (~9 us) instead of eight;
 * mmda_misa_timing_collect then returns per-launch means over the steps that sampled that launch and, in *steps, the fewest samples behind a mean */
int mmda_misa_timing_rotate(mmda_misa* m, int on);
int mmda_misa_timing_begin(mmda_misa* m, int max_steps);
int mmda_misa_timing_collect(mmda_misa* m, float mean_ms[4], int* steps);
int mmda_misa_timing_end(mmda_misa* m);

/* ---------------------------------------------------------------------------------------------- device-resident dataset
 * One batch of the reference's collate_fn (data_loader.py:59-122, use_bert = False) gathered from a dataset that lives on the device, in
 * ONE launch (mmda_amd/data.py: DeviceLoader).  The dataset: the n samples' time positions back to back, P in all -- words int32 [P],
 * visual fp32 [P, dv], acoustic fp32 [P, da] -- with offsets int64 [n + 1] (sample i owns positions offsets[i] .. offsets[i + 1] - 1),
 * emo fp32 [n, 6] (NULL: the dataset has no emotion table) and sentiment fp32 [n].  The batch: order int32 [B], sample indices in batch
 * order (the host sorts by length, descending), T time steps.  Outputs, time-major: out_ids int64 [T, B], out_v fp32 [T, B, dv],
 * out_a fp32 [T, B, da], out_emo fp32 [B, 6] (may be NULL), out_y fp32 [B].  With len_b = offsets[order[b] + 1] - offsets[order[b]],
 * position (t, b) is a copy of row offsets[order[b]] + t when t < len_b, and pad_id / zeros otherwise: every output element is written,
 * so the outputs need no clearing.  A T below a sample's length cuts the sample off at T.  Copies only: the outputs hold the dataset's
 * bits.  MMDA_EINVAL, with nothing launched: a NULL pointer other than emo / out_emo, out_emo without emo, B, T, dv or da <= 0.
 * Nothing checks the indices: an `order` entry outside [0, n) reads out of bounds (the caller validates them on the host). */
int mmda_collate_gather(const int32_t* words, const float* visual, const float* acoustic, const int64_t* offsets, const float* emo,
                        const float* sentiment, const int32_t* order, int B, int T, int dv, int da, int pad_id, int64_t* out_ids,
                        float* out_v, float* out_a, float* out_emo, float* out_y, void* stream);

/* ---------------------------------------------------------------------------------------------- inference pass
 * What one evaluation forward left in the workspace, copied into per-SAMPLE result tables in ONE launch per batch (mmda_amd/inference.py:
 * InferencePass).  The reference only names the pass: src/inference.py is a TODO, utils/tools.py save_hidden / load_hidden want the
 * per-sample h, models.py:159 asks how to extract the attention scores.
 * src: the batch, B columns.  scores, labels (B, ncls); tcp (B, 6); hfused (B, 6 hs), row b = h = cat(h[0..5], dim=1) of column b
 *   (LayerNorm 2 writes it permuted, the head GEMM reads it so); x6 (6, B, hs) = [private t, v, a, shared t, v, a]; probs
 *   (B, nhead, 6, 6), the softmax rows before attention dropout (mmda_attn_fwd writes them in every mode).
 * out: tables of n rows, each may be NULL (skipped).  scores, labels (n, ncls); tcp (n, 6); hidden (n, 6 hs) = the hfused row;
 *   utterance (n, 6, hs): [r][k] = x6[k][b]; attention (n, 6, 6): the heads of probs summed in head order in fp32 and divided by
 *   nhead -- what nn.MultiheadAttention(need_weights=True) returns.
 * Column b goes to row dst[b] (int32, device), or to row base + b when dst is NULL.  NOTHING checks the rows: the caller guarantees
 * that they lie inside the tables and are distinct within a launch (as for mmda_collate_gather's order).  Offsets are 64-bit.  Rows
 * whose width is a multiple of four floats move as 16-byte accesses when both bases are 16-byte aligned, everything else as 4-byte ones.
 * MMDA_EINVAL, with nothing launched: src or out NULL, every table NULL, B <= 0, ncls / hs / nhead <= 0, or a table whose source
 * pointer is NULL.
 * mmda_misa_infer_collect: the same with src taken from the model's current workspace carve, B columns of its last forward; MMDA_EINVAL
 * also when the model has no workspace. */
typedef struct mmda_infer_src {
  const float* scores; const float* labels; const float* tcp; const float* hfused; const float* x6; const float* probs;
  int ncls, hs, nhead;
} mmda_infer_src;
typedef struct mmda_infer_out {
  float* scores; float* labels; float* tcp; float* hidden; float* utterance; float* attention;
} mmda_infer_out;
int mmda_infer_collect(const mmda_infer_src* src, const mmda_infer_out* out, const int32_t* dst, int64_t base, int B, void* stream);
int mmda_misa_infer_collect(mmda_misa* m, const mmda_infer_out* out, const int32_t* dst, int64_t base, void* stream);

/* ---------------------------------------------------------------------------------------------- encoder cache
 * With every encoder parameter frozen (the encoder cut of mmda_misa_set_trainable) and no dropout in the encoders (nn.LSTM / nn.GRU, one
 * layer each, models.py:48-55) a sample's utterance vectors utt_t (4 H_t), utt_v (4 H_v), utt_a (4 H_a) are constants, and nothing behind
 * the encoders reads anything else of them.  They are kept in tables of one row per SAMPLE (mmda_amd/encoded.py: EncoderCache) and a
 * step starts at the projections (models.py:63-80) from a gather of B rows.  Row movers, one launch each; offsets are 64-bit; a row moves
 * as 16-byte accesses when its width is a multiple of four floats and both bases are 16-byte aligned, as 4-byte ones otherwise.  A
 * segment (t, v, a, emo) is requested by giving BOTH its pointers and skipped by giving neither.
 * mmda_encoded_collect: utt_* are (B, w*) row-major; row b goes to table row dst[b] (int32, device), or base + b when dst is NULL.
 *   NOTHING checks the rows: the caller guarantees that they lie inside the tables and are distinct within a launch.
 * mmda_encoded_gather: output row b is table row rows[b] (int32, device; repeats allowed); tab_emo (n, ncls) -> emo (B, ncls) rides along
 *   when both are given.  Nothing checks the rows either.
 * MMDA_EINVAL, with nothing launched: a segment with one pointer NULL, every segment NULL, B <= 0, a requested width <= 0, rows NULL.
 * mmda_misa_encoded_collect: collect with the sources and widths 4 H_i of the model's current workspace carve (B columns of its last
 *   forward); MMDA_EINVAL also without a workspace. */
int mmda_encoded_collect(const float* utt_t, const float* utt_v, const float* utt_a, int wt, int wv, int wa, float* tab_t, float* tab_v,
                         float* tab_a, const int32_t* dst, int64_t base, int B, void* stream);
int mmda_encoded_gather(const float* tab_t, const float* tab_v, const float* tab_a, int wt, int wv, int wa, const float* tab_emo, int ncls,
                        const int32_t* rows, int B, float* utt_t, float* utt_v, float* utt_a, float* emo, void* stream);
int mmda_misa_encoded_collect(mmda_misa* m, float* tab_t, float* tab_v, float* tab_a, const int32_t* dst, int64_t base, void* stream);
/* A batch of cached rows: the three tables (n, 4 H_i), the label table (n, ncls; NULL where no labels are gathered) and the B row
 * indices (int32, device).  B must equal the B of the workspace carve; the carve's T is free (nothing such a step runs depends on it:
 * the host carves (B, 1)).
 * mmda_misa_forward_encoded: mmda_misa_forward from the projections on -- one mmda_encoded_gather into the workspace's utt_t / utt_v /
 *   utt_a, then the fusion block and the heads exactly as mmda_misa_forward runs them.  No W_hh packing, no operand conversion, no
 *   input GEMM, no recurrence.  Follows mmda_misa_set_inference like mmda_misa_forward.
 * mmda_misa_train_step_encoded: mmda_misa_train_step with that forward; emo_out (B, ncls) receives the gathered labels the losses read
 *   and must stay alive until the step has run.  From the projections on it issues the launches of a step under the encoder cut at the
 *   same B, with the same arguments: parameters, moments and losses get the same bits.
 * MMDA_EINVAL, with nothing launched: the encoder cut is not in force (a training forward: utt would need a gradient nobody computes),
 *   eb->B differs from the carve's, a NULL table / rows / emo_out, eb->tab_emo NULL in a train step. */
typedef struct mmda_encoded_batch {
  const float* tab_t; const float* tab_v; const float* tab_a; const float* tab_emo;
  const int32_t* rows; int B;
} mmda_encoded_batch;
int mmda_misa_forward_encoded(mmda_misa* m, const mmda_encoded_batch* eb, int training, uint64_t seed, void* stream);
int mmda_misa_train_step_encoded(mmda_misa* m, const mmda_encoded_batch* eb, float* emo_out, int training, uint64_t seed, int do_adam,
                                 float lr, float clip, int step, void* stream);

/* ---------------------------------------------------------------------------------------------- modality masking
 * A batch with some of its three inputs blanked, and what each input contributes to a value (mmda_amd/modality.py).
 * Modalities: 0 = text, 1 = visual, 2 = acoustic.  A keep set is three bits, bit m set = modality m is kept; 7 keeps everything, 0
 * nothing.  Blanking column b: every word id at t < len becomes unk_id (padding keeps pad_id), the column's visual / acoustic rows
 * become 0.0f.  Lengths and labels do not change, nothing is rescaled.
 * The random keep set of SAMPLE s (its dataset index, whatever batch it sits in): with u_m = (float)(rng_u32(seed, 11, 3 s + m) >> 8)
 *   * 2^-24 (the counter-based generator of the dropout sites, site 11), modality m is dropped iff p_m > 0 && u_m < p_m (fp32); a draw
 *   that would drop all three drops none.  A column's keep set is random_keep(s) & keep_const.
 * mmda_collate_gather_masked: mmda_collate_gather's arguments, grid and outputs under that keep set, in the same ONE launch; a dropped
 *   modality is written without its source being read.  out_keep (optional): uint8 [B], the columns' keep sets.  keep_const = 7 with
 *   p = {0, 0, 0} writes the bytes of mmda_collate_gather.  MMDA_EINVAL also for keep_const outside 0 .. 7 or a p outside [0, 1).
 * mmda_modality_mask: the out-of-place form for a batch that exists already.  ids int64 [T, B], v fp32 [T, B, dv], a fp32 [T, B, da]
 *   are read and never written; out_ids / out_v / out_a of the same shapes receive the masked copies (every element is written).
 *   Column b's keep set is keep[b] & 7 (uint8 [B], device) or, keep == NULL, keep_const.  An id equal to pad_id stays: pad_id is
 *   reserved, never a word, so no lengths are read.  One launch.  MMDA_EINVAL, nothing launched: a NULL pointer other than keep,
 *   T, B, dv or da <= 0, keep_const outside 0 .. 7, an output that is its input.
 * mmda_modality_attrib: V fp32 [8, n, C], V[k] = a value (a score column, tcp) under keep set k.  One thread per (row, class) writes
 *   phi [n, 3, C]: the exact Shapley value of three players, phi_m = sum over the S without m of w(|S|) (V[S | m] - V[S]),
 *     w(0) = w(2) = 1/3, w(1) = 1/6, the four terms added in ascending S in fp32;
 *   loo [n, 3, C] = V[7] - V[7 without m];
 *   dominant int32 [n, C]: the m of the largest phi_m, compared by a strict > in ascending m among the phi_m that are not NaN (ties go
 *     to the lowest m, a NaN never wins); -1 where all three are NaN;
 *   counts int64 [3, C], OVERWRITTEN (cleared on the stream, then integer adds): the rows each modality dominates, per class.  The
 *     same bits on every run.
 *   MMDA_EINVAL, nothing launched: a NULL pointer, n or C <= 0, n C >= 2^39. */
typedef struct mmda_modality_p { float p[3]; } mmda_modality_p;      /* the drop rates of text, visual, acoustic; passed by value */
int mmda_collate_gather_masked(const int32_t* words, const float* visual, const float* acoustic, const int64_t* offsets, const float* emo,
                               const float* sentiment, const int32_t* order, int B, int T, int dv, int da, int pad_id, int keep_const,
                               mmda_modality_p p, uint64_t seed, int unk_id, int64_t* out_ids, float* out_v, float* out_a,
                               float* out_emo, float* out_y, uint8_t* out_keep, void* stream);
int mmda_modality_mask(const int64_t* ids, const float* v, const float* a, int T, int B, int dv, int da, const uint8_t* keep,
                       int keep_const, int pad_id, int unk_id, int64_t* out_ids, float* out_v, float* out_a, void* stream);
int mmda_modality_attrib(const float* V, int64_t n, int C, float* phi, float* loo, int32_t* dominant, int64_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------- MC-dropout statistics
 * K stochastic draws per sample reduced to per-SAMPLE float64 tables in ONE launch (mmda_amd/uncertainty.py).
 * p fp32 (B K, W) row-major: row b K + k is draw k of sample b.  Sample b writes row dst[b] (int32, device) of every table that is not
 * NULL, or row base + b when dst is NULL; offsets are 64-bit and NOTHING checks the rows (mmda_infer_collect's contract).  The tables
 * are (n, W) float64; draws is (n, K, W) fp32, the draws themselves, copied.  Per (sample, column), every fp32 draw widened once:
 *   mean = (1/K) sum p_k;  var = (1/K) sum (p_k - mean)^2, the population form, a second pass over the same values, exactly 0 at K = 1;
 *   vote = the share of draws with p_k > thr[w] (fp32 compare; a NaN draw is not above); skipped when thr is NULL;
 *   bernoulli != 0, with h(q) = -q ln q - (1 - q) ln(1 - q) in nats and h(0) = h(1) = 0: entropy = h(mean), expected_entropy =
 *     (1/K) sum h(p_k), mutual_info = max(0, entropy - expected_entropy).  bernoulli == 0: those three pointers must be NULL.
 * A NaN draw makes mean, var and the three entropy figures of its (sample, column) NaN -- the vote stays the count it is -- and touches
 * no other element.  One wave per (sample, column); lane l adds its draws k = l, l + 64, ... in that order and a fixed xor butterfly
 * adds the lanes: the order of every addition is a function of K alone, so the bits of a sample depend neither on B, dst nor the run.
 * No atomics.  MMDA_EINVAL, with nothing launched: p or out NULL; every table NULL (a vote table without thr counts as NULL); B < 1, K
 * outside 1 .. 256, W outside 1 .. 64; an entropy table without bernoulli.
 * mmda_misa_mc_reduce: the same with p and W taken from the model's current workspace carve -- which = 0: scores (B K, ncls), Bernoulli
 *   (but not under the sentiment task, whose one column is no probability); which = 1: tcp (B K, 6), not Bernoulli.  The carve's B must
 *   be a multiple of K; MMDA_EINVAL otherwise, for another `which`, or when the model has no workspace. */
typedef struct mmda_mc_out {
  double* mean; double* var; double* entropy; double* expected_entropy; double* mutual_info; double* vote;
  float* draws;
} mmda_mc_out;
int mmda_mc_reduce(const float* p, int B, int K, int W, const float* thr, int bernoulli, const mmda_mc_out* out, const int32_t* dst,
                   int64_t base, void* stream);
int mmda_misa_mc_reduce(mmda_misa* m, int K, int which, const float* thr, const mmda_mc_out* out, const int32_t* dst, int64_t base,
                        void* stream);

/* ---------------------------------------------------------------------------------------------- bootstrap intervals
 * How far a figure of a report would move on another draw of the split (mmda_amd/bootstrap.py): the non-parametric
 * bootstrap over the n rows.  Replicate r = 0 .. R - 1 draws, for k = 0 .. n - 1,
 *   u = rng_u32(seed, 12, ((uint64)r << 32) + k)   (csrc/common.h; 12 = SITE_BOOTSTRAP),   j(r, k) = ((uint64)u * n) >> 32,
 * so a replicate depends on (seed, r, n) alone; replicate R is the identity j(R, k) = k, the point estimate.  Every table below has
 * R + 1 rows, row R the identity's.  1 <= n <= 2^20, 1 <= C <= 16, 1 <= R <= 8192; anything else is MMDA_EINVAL with nothing launched.
 * mmda_boot_pack: labels, truth fp32 (n, C) -> codes[n], bit c = labels[i][c] > 0, bit 16 + c = truth[i][c] > 0.
 * mmda_boot_counts OVERWRITES state[(R + 1)][3 C + 2] (int64): tp[C], fp[C], fn[C] of the drawn rows, acc_num = sum over the draws of
 *   720720 |y & p| / max(|y | p|, 1) (an integer: 720720 = lcm(1 .. 16)), and n.  form: 0 = what mmda_boot_plan_describe names,
 *   1 = the code table in LDS (n <= 16384, else MMDA_EINVAL), 2 = codes gathered from memory.  Integer adds only: the state depends
 *   neither on the form nor on the run.
 * mmda_boot_figures: out[(R + 1)][10 + 3 C] doubles from the states: acc (= acc_num / (720720 n), not rounded), f1, precision, recall
 *   (macro), micro_f1, micro_precision, micro_recall, weighted_f1, weighted_precision, weighted_recall -- utils/eval.py's
 *   metrics_from_counts -- then f1[C], precision[C], recall[C].
 * mmda_boot_rank: n <= 16384.  The tables describe each class's rows in sorted order (descending score under ranking.py's order, ties
 *   adjacent), all int32 (C, n): inv[c][row] = the row's sorted position; first[c][p] / last[c][p] = the first / last position of
 *   the tie group position p is in; pos[c][p] != 0 = the row at position p is a positive.  out[(R + 1)][(C + 1)][6] doubles, the
 *   columns and NaN rules of mmda_rank_finish with every row counted as often as the replicate draws it, row C the means.
 * mmda_boot_summary: a (and b, or NULL) doubles [(R + 1)][F]; x_r = a[r][f] (- b[r][f]); out[F][ncols], ncols 6: point (row R), mean,
 *   std (two-pass, ddof 1), lo, hi (the q_lo / q_hi percentiles, linear interpolation at h = (m - 1) q), defined (m, the replicates
 *   where x is not NaN); ncols 9: and p_le = (1 + #{x <= 0}) / (m + 1), p_ge = (1 + #{x >= 0}) / (m + 1), p_two = min(1, 2 min(p_le,
 *   p_ge)).  Sums in sorted order; m < 2: std NaN; m == 0: mean, std, lo, hi NaN.  R <= 8192, F >= 1.
 * mmda_boot_plan_describe (host only; mmda_boot_counts reads the same function): the form of the count launch of a shape. */
typedef struct mmda_boot_plan {
  int form;                 /* 1 = LDS, 2 = global */
  int threads;              /* of a workgroup of the count kernel */
  int wgs_per_replicate;
  int lds_bytes;            /* dynamic LDS of the count kernel */
  int state_words;          /* 3 C + 2 */
  int lds_rows;             /* the largest n of the LDS form and of mmda_boot_rank */
  int rank_lds_bytes;       /* dynamic LDS of mmda_boot_rank's kernel, 0 where n is over its limit */
  int max_replicates;
} mmda_boot_plan;
int mmda_boot_plan_describe(int64_t n, int C, int R, mmda_boot_plan* out);
int mmda_boot_pack(const float* labels, const float* truth, int64_t n, int C, uint32_t* codes, void* stream);
int mmda_boot_counts(const uint32_t* codes, int64_t n, int C, int R, uint64_t seed, int form, int64_t* state, void* stream);
int mmda_boot_figures(const int64_t* state, int C, int R, double* out, void* stream);
int mmda_boot_rank(const int32_t* inv, const int32_t* first, const int32_t* last, const int32_t* pos, int64_t n, int C, int R,
                   uint64_t seed, double tpr_level, double* out, void* stream);
int mmda_boot_summary(const double* a, const double* b, int R, int F, double q_lo, double q_hi, int ncols, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------- nearest neighbours, Trust Score
 * Exact set-wise k-nearest-neighbour search between two device tables (mmda_amd/neighbours.py; csrc/knn.hip).
 * mmda_knn_sets: query (Q, D), base (N, D) fp32, row-major, dense; member[N]: bit s set = base row in set s (any number of sets, or
 *   none).  dist / index (Q, S, k): per (query row, set) the k nearest member rows -- squared Euclidean distances ascending, equal
 *   distances by lower row number; where a set has fewer than k eligible rows the tail is +inf / -1.  exclude_self != 0: query row i
 *   ignores base row i (by row number, whatever its distance).  A pair whose distance is NaN or +inf (a non-finite entry in either
 *   row) is never selected.  Three launches, no float atomics, no read-back:
 *     1. row norms |q|^2, |b|^2 (one wave per row, lane l adds elements l, l + 64, .. by fmaf, a fixed xor butterfly adds the lanes);
 *     2. grid (query tiles, slabs): the products q.b of a tile_q x 128 tile on v_mfma_f32_32x32x2_f32, operands staged through LDS in
 *        32-wide pieces of D, k ascending from 0 -- one fmaf chain per pair whatever the tile --, d = fmaf(-2, q.b, |q|^2 + |b|^2),
 *        and the running lists of the workgroup's (query row, set)s updated in LDS from the tile; the Q x N matrix is never written;
 *     3. one wave per (query row, set): the slabs' lists merged by (distance, row number), the k survivors recomputed as
 *        sum_i (q_i - b_i)^2 (fmaf, lane l the elements l, l + 64, .., the same butterfly) and sorted by (that distance, row number).
 *   dist holds the recomputed value: a query equal to a base row reports exactly 0.  Both forms are functions of the two rows and D
 *   alone, so Q calls over one row each give the bits of one call over Q rows.  1 <= D <= 1024, 1 <= S <= 16, 1 <= k <= 16, N >= 1,
 *   Q >= 0 (0: MMDA_OK, no launch); work: what mmda_knn_plan_describe sizes, 16-byte aligned; work_bytes below that, a NULL pointer
 *   or a shape outside the limits: MMDA_EINVAL before any launch.
 * mmda_knn_plan_describe (host only; the launcher reads the same function): the launches of a shape.
 * mmda_trust_score: dist (n, 2 C, k) fp32 as mmda_knn_sets wrote it over the sets s = 2 c + v (the base rows with truth[:, c] == v),
 *   labels (n, C) fp32 the decisions (> 0: positive).  With y = labels[i][c] > 0, p = dist[i][2 c + y][0], o = dist[i][2 c + 1 - y][0]:
 *   trust[i][c] = sqrt(o) / (sqrt(p) + 1e-12) in float64 (1e-12: the published implementation's min_dist); p = +inf (no row of the
 *   decided label) gives 0, else o = +inf gives +inf.  Optional (NULL: not written) d_pred / d_other (n, C) fp32 = p / o and, with index
 *   (n, 2 C, k), nearest_pred / nearest_other (n, C) int32 their row numbers.  One launch.  1 <= C <= 8, 1 <= k <= 16, n >= 0;
 *   dist, labels or trust NULL, a nearest table without index: MMDA_EINVAL. */
typedef struct mmda_knn_plan {
  int tile_q;               /* query rows of a workgroup: 64, or 32 where the lists of 64 rows would not fit (S k > 200) */
  int tile_b;               /* base rows of one distance tile */
  int slab_rows;            /* base rows of a slab: a multiple of tile_b */
  int slabs;
  int merge;                /* 1: the last launch merges the lists of more than one slab */
  int launches;
  int grid_x, grid_y;       /* of the search launch: query tiles, slabs */
  int threads;              /* of a workgroup of the search launch */
  int lds_bytes;            /* dynamic LDS of a workgroup of the search launch */
  int vector_loads;         /* 1: D % 4 == 0, rows are staged by 16-byte loads (where the tables are 16-byte aligned) */
  int max_slabs;
  int64_t work_bytes;       /* row norms, then the slabs' lists */
} mmda_knn_plan;
int mmda_knn_plan_describe(int64_t Q, int64_t N, int D, int S, int k, mmda_knn_plan* out);
int mmda_knn_sets(const float* query, const float* base, const uint32_t* member, int64_t Q, int64_t N, int D, int S, int k,
                  int exclude_self, float* dist, int32_t* index, void* work, int64_t work_bytes, void* stream);
int mmda_trust_score(const float* dist, const int32_t* index, const float* labels, int64_t n, int C, int k, double* trust,
                     float* d_pred, float* d_other, int32_t* nearest_pred, int32_t* nearest_other, void* stream);

#ifdef __cplusplus
}
#endif
#endif
