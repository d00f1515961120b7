/* neunet_hip.h -- C ABI of libneunet_hip.so: the MI355X (gfx950) drop-in for the CUDA .so files
 * that neunet's experimental layer binds through ctypes (reference:
 * neunet/nn/experimental/utils.py:64-92 -- ctypes.CDLL + getattr + argtypes).
 *
 * Conventions (differences from the reference's exports are deliberate and listed here):
 *   - every entry point returns int: 0 = ok, >0 = hipError_t, <0 = NNHIP_E* argument error
 *     (the reference returns void and printf+exit()s on failure, e.g.
 *     linear_cublaslt_no_manual_mem.cu:91-94,117-120; cross_entropy.cu:287-291);
 *   - every launch takes an explicit stream (hipStream_t passed as void*) as its LAST argument
 *     (the reference's Linear and CrossEntropy exports implicitly use stream 0);
 *   - sizes are int64_t (the reference mixes int / size_t: linear.py:46-48 vs .cu:114);
 *   - all tensor pointers are DEVICE pointers to C-contiguous fp32 (labels: int32); the caller owns
 *     and pre-allocates every buffer (reference: utils.py:72-82, `xp.empty` before each call);
 *     optional pointers may be NULL where noted;
 *   - argument ORDER and MEANING follow the reference export each function replaces (cited).
 * The library never synchronises the device inside a compute entry point.
 */
#ifndef NEUNET_HIP_H
#define NEUNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nnhipStream_t; /* hipStream_t */

#define NNHIP_OK 0
#define NNHIP_EINVAL (-1)   /* bad argument (null pointer, negative size, bad enum) */
#define NNHIP_EALIGN (-2)   /* pointer not aligned as the entry requires (4 bytes unless the entry says otherwise) */
#define NNHIP_ENOMEM (-3)   /* workspace allocation failed */
#define NNHIP_EDEVICE (-5)  /* a kernel of an EARLIER launch found the device state broken and raised the library's device error
                             * word; sticky until nnhipClearDeviceError() (-4 is NNHIP_ECOMM, below) */

/* ---- library ------------------------------------------------------------------------------ */
int nnhipVersion(void);
/* Human-readable text for the last non-zero status returned on the calling thread. */
const char* nnhipGetLastErrorString(void);
/* Free the grow-only device workspace (split-K slabs, column-sum partials).
 * Replaces cleanupCudaMemory() (linear_cublaslt_no_manual_mem.cu:186, linear_cutlass.cu:107,
 * linear_swish_cutlass_evt_full.cu:820).  Synchronises the device. */
int nnhipCleanup(void);
/* Device-side errors (ABI 210).  A kernel cannot return a status, and the reference's convention for a failure inside its CUDA
 * path is printf + exit(1) (linear_cublaslt_no_manual_mem.cu:91-94).  Here a kernel that finds the device state broken -- today
 * only the optimizer-in-backward launch whose arrival barrier saw no progress for 20 s -- skips its side effect, stores a code in
 * a library-owned word of pinned host memory and ends normally.  nnhipDeviceError() reads that word without synchronising:
 * 0, or NNHIP_EDEVICE with the story in nnhipGetLastErrorString().  nnhipLinearReLULinearBackwardAdam and the optimizer step
 * entries check it on entry, so a training loop stops at its next step instead of losing the context to a trap.
 * nnhipClearDeviceError() resets the word.  nnhipRaiseDeviceErrorForTest() stores `code` from a one-block kernel on `stream`
 * (the tests' way to exercise the path without a broken device). */
int nnhipDeviceError(void);
int nnhipClearDeviceError(void);
int nnhipRaiseDeviceErrorForTest(int32_t code, nnhipStream_t stream);
/* Grow the workspace to at least `bytes` now (e.g. before capturing a hipGraph). */
int nnhipWorkspaceReserve(int64_t bytes);
/* locked != 0: the workspace may no longer move -- a launch that needs more than it holds returns NNHIP_ENOMEM instead
 * of freeing the block a captured hipGraph still points into.  nnhipCleanup() unlocks. */
int nnhipWorkspaceLock(int locked);

/* GEMM arithmetic of every Linear / attention GEMM that runs on the 128x128-tile kernel:
 *   0 (default)  exact fp32: v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain;
 *   1            split-bf16 ("bf16x3"): every fp32 operand is split EXACTLY into three bf16 pieces and six of the nine
 *                piece products are accumulated in fp32 on the bf16 matrix cores -- relative error <= ~2^-23 per
 *                product (the order of fp32 rounding itself), up to 2.67x the fp32 MFMA rate.  Opt-in; also
 *                NNHIP_GEMM_MODE=1 in the environment.  Small problems (gemm_small) stay exact either way. */
int nnhipSetGemmMode(int mode);
int nnhipGetGemmMode(void);
/* Lock-step mode of the exact-fp32 128x128-tile kernel for reductions of >= 2048 (off by default; also NNHIP_GEMM_LOCKSTEP=1):
 * the two blocks resident on a CU hold each other to within a few k-tiles through issue priorities, so the tiles that share an
 * operand panel in an XCD's L2 fetch it from the fabric once instead of twice (4096^3 forward: 808 -> 575 MB of L2->fabric
 * reads, dW 655 -> 574; dX, already at 541, is left alone) at +2.7 % kernel time (dW +0.6 %).  Results are bit-identical either way (the arithmetic and its order do not change).  For
 * deployments where the fabric is shared with collectives.  ABI 205 */
int nnhipSetGemmLockstep(int enable);
int nnhipGetGemmLockstep(void);
/* Launches since the library was loaded, per GEMM kernel family: 0 = classic fp32 128x128 tiles (gemm_f32_kernel),
 * 1 = persistent fp32 (gemm_pst_kernel), 2 = small-problem kernel (gemm_small*), 3 = split-bf16 (gemm_bf3_kernel),
 * 4 = the weight-streaming Linear forward for 1..8 rows (linear_gemv_kernel, ABI 214); -1 for any other argument.  Host-side
 * bookkeeping for tests that must know which kernel produced a result.  ABI 203 */
int64_t nnhipGemmLaunchCount(int family);

/* ---- a1/a2 Linear  (replaces cudaLinearModuleForward/Backward,
 *      linear_cublaslt_no_manual_mem.cu:114,142 and linear_cutlass.cu:40,67) ------------------ */
/* O[rows,out] = X[rows,in] * W[out,in]^T + b[out]      (b may be NULL) */
int nnhipLinearModuleForward(const float* X, const float* W, const float* b, float* O,
                             int64_t rows, int64_t in_features, int64_t out_features,
                             nnhipStream_t stream);
/* dX[rows,in] = dO*W ; dW[out,in] = dO^T*X ; db[out] = sum_rows dO.  Any of dX/dW/db may be NULL
 * (skipped). */
int nnhipLinearModuleBackward(const float* X, const float* W, const float* dO, float* dX,
                              float* dW, float* db, int64_t rows, int64_t in_features,
                              int64_t out_features, nnhipStream_t stream);
/* Extensions with an addend folded into the GEMM epilogue (both NULL-able; NULL == the plain entry points):
 *   forward : O  = X*W^T + b + addend        (addend [rows,out]: the residual of `x + linear(h)`, neunet/autograd.py add)
 *   backward: dX = dO*W + dX_addend          (dX_addend [rows,in]: a gradient X has already received -- replaces the
 *                                             separate accumulation of Tensor.apply_grad, neunet/autograd.py:85-93)
 * The addend is read once per output float4 (may alias nothing that is written). db is produced by the dW GEMM itself. */
int nnhipLinearModuleForwardEx(const float* X, const float* W, const float* b, const float* addend, float* O,
                               int64_t rows, int64_t in_features, int64_t out_features, nnhipStream_t stream);
int nnhipLinearModuleBackwardEx(const float* X, const float* W, const float* dO, const float* dX_addend, float* dX,
                                float* dW, float* db, int64_t rows, int64_t in_features, int64_t out_features,
                                nnhipStream_t stream);

/* Weight-streaming forward for a handful of rows (extension, ABI 214; no reference counterpart): the single-token steps of
 * KV-cached decoding, where a 128x128-tile GEMM is 127/128 empty and needs a split-K reduce behind it.
 *   O[r,n] = sum_k X[r,k]*W[n,k] (+ b[n]) (+ addend[r,n]),   0 <= rows <= NNHIP_LINEAR_GEMV_MAX_ROWS; b and addend may be NULL;
 *   addend under the aliasing contract of nnhipLinearModuleForwardEx.
 * One kernel launch, no workspace, exact fp32 on the vector ALU; every weight is read once and used for all rows.  Results are
 * bit-identical from run to run, and the bits of O[r,:] depend on X[r,:], W, b and addend[r,:] only: row r of an 8-row call equals
 * a 1-row call on that row.  The epilogue is (acc + b[n]) + addend[r,n], each step rounded.  Any in_features / out_features;
 * 4-byte alignment is enough (16-byte loads are used when in_features % 4 == 0 and X, W are 16-byte aligned).
 * This entry always runs the kernel.  NNHIP_EINVAL: rows > NNHIP_LINEAR_GEMV_MAX_ROWS, a negative size, a null X, W or O with work
 * to do; NNHIP_EALIGN: any pointer not 4-byte aligned.  rows == 0 or out_features == 0: returns 0, launches nothing;
 * in_features == 0: what nnhipLinearModuleForwardEx does for the same arguments. */
#define NNHIP_LINEAR_GEMV_MAX_ROWS 8
int nnhipLinearGemvForward(const float* X, const float* W, const float* b, const float* addend, float* O, int64_t rows,
                           int64_t in_features, int64_t out_features, nnhipStream_t stream);
/* Process-wide switch, 0 (default) or 1; anything else is NNHIP_EINVAL and changes nothing.  While it is 1,
 * nnhipLinearModuleForward and nnhipLinearModuleForwardEx with 1 <= rows <= NNHIP_LINEAR_GEMV_MAX_ROWS run the kernel above, in
 * either GEMM mode (small problems stay exact fp32).  Off by default because another summation order moves results in their last
 * bits.  Every other entry -- the activation-fused forwards, LinearSwish, every backward -- ignores it.  ABI 214 */
int nnhipSetLinearGemv(int enable);
/* The current value of the switch. */
int nnhipGetLinearGemv(void);

/* Deferred parameter gradients (extension; the reference computes each layer's dW where its backward runs, linear.py:17-24).
 * enable != 0: from now on the Linear backward entry points (nnhipLinearModuleBackward[Ex|Act], nnhipLinearSwishBackward) QUEUE
 * a dW/db GEMM that is too small to fill the chip alone (<= 256 output tiles of 128x128, >= 4096 rows, 16-B aligned operands;
 * either GEMM mode); dX is still computed by the call itself.  nnhipWeightGradFlush launches everything queued as ONE grid and
 * ONE reduce -- a transformer layer's four dW GEMMs stop paying four launch ramps, four simultaneous slab epilogues and four
 * tails.  A job's reduction is always cut into four chunks, so a gradient's bits do not depend on what else was in the queue.
 * Contract while a job is queued: its X and dO stay alive and unmodified, its dW/db are not read.  enable == 0: flush on
 * `stream`, then every later dW is launched where it is asked for (the default).  nnhipWeightGradPending: queued jobs.
 * The switch and the queue are ONE per process, for ONE host thread and ONE stream at a time (like the workspace): while it is
 * on, a backward entry called from another thread or on another stream is queued all the same -- a caller that defers must be
 * the only caller until it has flushed (Tensor.backward() switches it on for the duration of its own tape walk only).  ABI 204 */
int nnhipWeightGradDefer(int32_t enable, nnhipStream_t stream);
int nnhipWeightGradFlush(nnhipStream_t stream);
/* Only the queued dW/db GEMMs (one grouped launch + its reduce) on `stream`, which may be a SIDE stream: the caller orders it behind
 * the producers of the queued calls' X / dO, keeps those alive until it has joined `stream` again, and reads dW / db only after the
 * join.  The launch keeps its split-K slabs in a block of its own, so kernels of the main stream may run next to it; a later user
 * of that block on another stream (the next grouped launch, from any flush) is ordered behind it by the library.  Everything
 * else a flush does (conv reduces, RMSNorm column sums) stays with nnhipWeightGradFlush.  ABI 210 */
int nnhipWeightGradFlushGemms(nnhipStream_t stream);
int nnhipWeightGradPending(void);

/* ---- a6 fused Linear -> Swish  (replaces cudaLinearSwishForward/Backward,
 *      linear_swish_cutlass_evt_full.cu:558-570, 680-695) ------------------------------------- */
/* z = X*W^T + b ; O = z*sigmoid(beta*z).  If save_preactivation != 0, z is also written to
 * `preact` (must be non-NULL then).  save_preactivation == 2 (ABI 210, no reference counterpart): `preact` receives
 * swish'(z) = s + beta*O*(1 - s), s = sigmoid(beta*z), instead of z -- the same sigmoid serves both outputs, and the backward
 * pass (nnhipLinearSwishBackward with recompute_preactivation = 2, nnhipLinearInputGradScaled, nnhipLinearModuleBackwardAct with
 * act_grad = 3) only multiplies: in an fp32 MFMA kernel every vector instruction of an epilogue is paid in matrix-pipe time. */
int nnhipLinearSwishForward(const float* X, const float* W, const float* b, float* O, float* preact,
                            int64_t M, int64_t K, int64_t N, float swish_beta,
                            int save_preactivation, nnhipStream_t stream);
/* tmp[M,N]: if recompute_preactivation == 0 it holds z on entry (saved by the forward); 2: it holds swish'(z) (forward with
 * save_preactivation = 2); otherwise (1) it is scratch and z is recomputed into it.  On exit tmp holds dZ (reference in-place contract,
 * ...evt_full.cu:707-711).  dX/dW/db may be NULL. */
int nnhipLinearSwishBackward(const float* X, const float* W, const float* b, const float* dO,
                             float* tmp, float* dX, float* dW, float* db, int64_t M, int64_t K,
                             int64_t N, float swish_beta, int recompute_preactivation,
                             nnhipStream_t stream);

/* ---- general fp32 MFMA GEMM (net-new; used by the entries above and by the batched matmul of
 *      SURVEY 8f-1, neunet/autograd.py:192-230) -------------------------------------------------
 * C[b] (M x N, row-major, ldc) = op(A[b]) * op(B[b]) (+ bias[N]) ;  b = 0..batch-1.
 *   a_kmajor != 0: A element (m,k) at A[m*lda + k]   (reduction dim contiguous)
 *   a_kmajor == 0: A element (m,k) at A[k*lda + m]
 *   b_kmajor != 0: B element (k,n) at B[n*ldb + k]
 *   b_kmajor == 0: B element (k,n) at B[k*ldb + n]
 * strideA/B/C: element offsets between consecutive batches (0 = shared operand). */
int nnhipGemmF32(const float* A, const float* B, float* C, const float* bias, int64_t M, int64_t N,
                 int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor,
                 int64_t batch, int64_t strideA, int64_t strideB, int64_t strideC,
                 nnhipStream_t stream);

/* Same, with an output scale and a two-level batch: batch index z = z1*batch2 + z2 addresses
 * A + z1*sA1 + z2*sA2 (likewise B, C):  C = alpha * op(A) op(B) (+ bias).  Lets attention read Q/K/V
 * straight out of their [B,T,H*dh] projection buffers and write the context back in that layout -- no
 * transpose copies (examples/gpt.ipynb cell 2 transposes/reshapes on the host side instead). */
int nnhipGemmF32Ex(const float* A, const float* B, float* C, const float* bias, int64_t M, int64_t N,
                   int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor,
                   int64_t batch1, int64_t sA1, int64_t sB1, int64_t sC1, int64_t batch2, int64_t sA2,
                   int64_t sB2, int64_t sC2, float alpha, nnhipStream_t stream);

/* ---- a12 ReLU (net-new export; reference CPU: neunet/nn/activations.py:40-59) --------------- */
/* out = max(0, in) as np.maximum computes it: a NaN stays a NaN (it is not clamped to 0); -0.0 gives +0.0 */
int nnhipReLUForward(float* out, const float* in, int64_t size, nnhipStream_t stream);
/* dIn = dOut * (out > 0), `out` = forward output */
int nnhipReLUBackward(float* dIn, const float* dOut, const float* out, int64_t size,
                      nnhipStream_t stream);

/* Input gradient of a Linear whose input was h = swish(z) (the FFN's fc_2 after the fused Linear->Swish fc_1,
 * examples/gpt.ipynb cell 2): dZ[rows,in] = (dO[rows,out] * W[out,in]) (.) swish'(Z; beta), i.e. the dX GEMM of
 * nnhipLinearModuleBackward with the element-wise Swish backward (neunet/nn/activations.py:223-232) applied in its
 * epilogue.  dZ may alias Z (each element is read once, then written).  Feed dZ to nnhipLinearModuleBackward of fc_1. */
int nnhipLinearInputGradSwish(const float* dO, const float* W, const float* Z, float* dZ, int64_t rows,
                              int64_t in_features, int64_t out_features, float swish_beta, nnhipStream_t stream);

/* The same with the derivative in hand: dZ = (dO * W) (.) D, D = what nnhipLinearSwishForward(save_preactivation = 2) left in
 * `preact`.  dZ may alias D.  ABI 210 */
int nnhipLinearInputGradScaled(const float* dO, const float* W, const float* D, float* dZ, int64_t rows,
                               int64_t in_features, int64_t out_features, nnhipStream_t stream);

/* The same for h = relu(z): dZ = (dO * W) (.) [F > 0] with F = the ReLU's forward output (activations.py:44-45); dZ must
 * not alias F (F is still the Linear's input for its dW). */
int nnhipLinearInputGradReLU(const float* dO, const float* W, const float* F, float* dZ, int64_t rows,
                             int64_t in_features, int64_t out_features, nnhipStream_t stream);
/* Both of the above plus the parameter gradients in one call: dZ = (dO * W) (.) act'(act_arg) -- act_grad 1: swish'(act_arg = Z;
 * beta), dZ may alias Z; 2: [act_arg = F > 0], dZ must not alias F; 3 (ABI 210): act_arg is the saved derivative swish'(z) itself, a plain
 * multiplier, dZ may alias it -- and dW = dO^T X, db = column sums of dO (either may be NULL),
 * i.e. _LinearTensor.grad_fn (linear.py:17-24) followed by the activation's backward.  A small layer (the README MLP's
 * 128 -> 10 head) gets dZ, dW and db from ONE launch. */
int nnhipLinearModuleBackwardAct(const float* X, const float* W, const float* dO, const float* act_arg, int32_t act_grad,
                                 float beta, float* dZ, float* dW, float* db, int64_t rows, int64_t in_features,
                                 int64_t out_features, nnhipStream_t stream);
/* Backward of out = Linear2(relu(Linear1(X1))) when X1 needs no gradient (README quick-start MLP, README.md:57-71): dW2 =
 * dO^T H, db2, dW1 = dZ^T X1, db1 with dZ = (dO W2) (.) [H > 0] formed inside the dW1 tiles (never written) -- ONE launch where
 * nnhipLinearModuleBackwardAct + nnhipLinearModuleBackward take two dependent ones.  H = the ReLU output [rows, hidden].
 * rows <= 256, out2 <= 16, small layers only: NNHIP_EINVAL otherwise (use the two calls).  ABI 203 */
int nnhipLinearReLULinearBackward(const float* X1, const float* H, const float* W2, const float* dO, float* dW2, float* db2,
                                  float* dW1, float* db1, int64_t rows, int64_t in1, int64_t hidden, int64_t out2,
                                  nnhipStream_t stream);
/* The same with the optimizer inside: every gradient element is handed to Adam / AdamW (neunet/optim.py:17-33, 52-69) by the
 * thread that produced it -- the README-MLP step then has no optimizer launch.  Gradients are still written.  pmv: 12 device
 * pointers {param, m, v} x {W2, b2, W1, b1}.  step >= 1: host stepping; step == 0: device stepping through `opt`
 * (nnhipCreateFusedOptimizer + SetStep / SetHyper).  Hyper-parameters as nnhipFusedAdamWMultiTensorStep.  ABI 203 */
int nnhipLinearReLULinearBackwardAdam(const float* X1, const float* H, const float* W2, const float* dO, float* dW2, float* db2,
                                      float* dW1, float* db1, int64_t rows, int64_t in1, int64_t hidden, int64_t out2,
                                      void* opt, float* const* pmv, double lr, double beta1, double beta2, double eps,
                                      double weight_decay, int32_t step, int32_t decay_mode, float grad_scale,
                                      nnhipStream_t stream);
/* 1 when the two entries above (with_adam 0 / 1) take these sizes on the current device, 0 when they would answer NNHIP_EINVAL
 * -- for a caller that decides BEFORE it defers the launch (neunet_hip defers it to optimizer.step() so that the README MLP's
 * default training step gets the backward + Adam launch without opting in).  No device work.  ABI 209 */
int nnhipLinearReLULinearBackwardFits(int64_t rows, int64_t in1, int64_t hidden, int64_t out2, int32_t with_adam);
/* O = act(X*W^T + b), activation in the GEMM epilogue: 1 = swish(beta) without saving z, 2 = relu, 3 = sigmoid.
 * Activation 2 is np.maximum(0, z) (activations.py:55), as nnhipReLUForward: a NaN in z stays NaN, -0 becomes +0, on
 * every kernel family the call can reach (small, 128x128 float4 / scalar epilogue, split-K reduce).
 * One launch for what `act(Linear(x))` is on the reference's tape (linear.py:48-58 + activations.py); the host side
 * uses it when an activation module is applied to a Linear output nobody else has looked at yet. */
int nnhipLinearActivationForward(const float* X, const float* W, const float* b, float* O, int64_t rows,
                                 int64_t in_features, int64_t out_features, int32_t activation, float beta,
                                 nnhipStream_t stream);

/* ---- a5 Swish  (replaces cudaSwishForward/Backward, swish.cu:50,65) ------------------------- */
int nnhipSwishForward(float* out, const float* in, float beta, int64_t size, nnhipStream_t stream);
int nnhipSwishBackward(float* dIn, const float* dOut, const float* in, float beta, int64_t size,
                       nnhipStream_t stream);

/* ---- a7 fused Swish-and-mul / SwiGLU gate  (replaces cudaFusedSwishAndMul[Backward],
 *      fused_swish_and_mul.cu:60,76).  in rows = [gate(hidden), up(hidden)], size = #OUTPUT elems */
int nnhipFusedSwishAndMul(float* out, const float* in, float beta, int64_t hidden, int64_t size,
                          nnhipStream_t stream);
int nnhipFusedSwishAndMulBackward(float* dIn, const float* dOut, const float* in, float beta,
                                  int64_t hidden, int64_t size, nnhipStream_t stream);

/* ---- a8 Softmax  (replaces cudaSoftmaxForward/Backward, softmax.cu:144,229).
 *      Slice s = outer*stride + inner starts at element outer*slice_size*stride + inner; its
 *      slice_size elements are `stride` apart (stride == 1: softmax over contiguous rows). */
int nnhipSoftmaxForward(float* out, const float* in, int64_t num_slices, int64_t slice_size,
                        int64_t stride, nnhipStream_t stream);
int nnhipSoftmaxBackward(float* dX, const float* dY, const float* Y, int64_t num_slices,
                         int64_t slice_size, int64_t stride, nnhipStream_t stream);

/* Attention-score softmax with scale and mask fused (examples/gpt.ipynb cell 2):
 *   y = softmax_j( masked(b,i,j) ? -1e9 : scale * x[b,h,i,j] ),  x,y: [B,H,Tq,Tk]
 *   masked = (key_valid && key_valid[b*Tk + j] == 0) || (causal && j > i + Tk - Tq).   key_valid may be NULL.
 * Backward: dX = masked ? 0 : scale * (dY - sum_j dY*Y) * Y. */
int nnhipMaskedSoftmaxForward(float* out, const float* in, const int32_t* key_valid, int64_t B, int64_t H,
                              int64_t Tq, int64_t Tk, float scale, int causal, nnhipStream_t stream);
int nnhipMaskedSoftmaxBackward(float* dX, const float* dY, const float* Y, const int32_t* key_valid,
                               int64_t B, int64_t H, int64_t Tq, int64_t Tk, float scale, int causal,
                               nnhipStream_t stream);

/* The same with an additional dense mask [B,Tq,Tk] int32 (0 = masked; broadcast over heads; NULL = none): what the notebook's
 * MultiHeadAttention.forward receives (get_pad_mask & get_sub_mask, cell 7), for callers that want the attention map. */
int nnhipMaskedSoftmaxForwardEx(float* out, const float* in, const int32_t* key_valid, const int32_t* dense_mask, int64_t B,
                                int64_t H, int64_t Tq, int64_t Tk, float scale, int causal, nnhipStream_t stream);
int nnhipMaskedSoftmaxBackwardEx(float* dX, const float* dY, const float* Y, const int32_t* key_valid,
                                 const int32_t* dense_mask, int64_t B, int64_t H, int64_t Tq, int64_t Tk, float scale,
                                 int causal, nnhipStream_t stream);

/* Fused (flash-style) attention, head_dim 32 / 64 / 128: same math as  QK^T*scale -> mask(-1e9) -> softmax -> dropout -> *V
 * above, but the [B,H,Tq,Tk] score matrix is never written.  O/dO are [B,T,H*head_dim] (the projection layout); Q/K/V/dQ/dK/dV
 * are [B,T,*] with row stride ld_qkv floats (0 = H*head_dim; 3*H*head_dim when they are the three column blocks of one fused
 * q|k|v projection buffer).  LSE [B,H,Tq,2] = (row max, log2 row sum) of each masked score row in log2 units, saved by the
 * forward and consumed by the backward; the pair is kept apart because a fully-masked row has max = -1e9*log2(e),
 * where fp32 cannot hold max + log(sum).
 * Status (all checked on the host before any launch; nothing is written when a call is refused): a NULL operand or output, Tk == 0 with
 * Tq > 0 (forward), a head_dim other than 32 / 64 / 128, ld_qkv that is neither 0 nor a multiple of 4 that is >= H*head_dim, mask_bits
 * without mask_bitsT, dropout_p outside [0, 1): NNHIP_EINVAL.  Q, K, V, O, dO, dQ, dK, dV not 16-byte aligned, or LSE not 8-byte aligned
 * (the kernels store and load a row's pair as one float2): NNHIP_EALIGN -- since ABI 215 from the forward too, which used to answer
 * NNHIP_EINVAL for a misaligned O and did not check LSE.  B == 0 or Tq == 0 (backward: or Tk == 0): returns 0, launches nothing. */
int nnhipAttentionForward(const float* Q, const float* K, const float* V, const int32_t* key_valid, float* O,
                          float* LSE, int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t head_dim, int64_t ld_qkv,
                          float scale, int causal, nnhipStream_t stream);
/* dQ, dK, dV from (Q, K, V, O, dO, LSE): P is recomputed tile by tile; deterministic (no atomics): one kernel owns
 * 128-key blocks (dK, dV), one owns 128-query blocks (dQ). */
int nnhipAttentionBackward(const float* Q, const float* K, const float* V, const int32_t* key_valid, const float* O,
                           const float* dO, const float* LSE, float* dQ, float* dK, float* dV, int64_t B, int64_t H,
                           int64_t Tq, int64_t Tk, int64_t head_dim, int64_t ld_qkv, float scale, int causal,
                           nnhipStream_t stream);
/* The same with the rest of examples/gpt.ipynb cell 2 inside the kernels (all fields optional; a NULL struct == the calls
 * above):
 *   mask_bits / mask_bitsT / row_any: an arbitrary dense [B,Tq,Tk] mask (what the notebook builds with get_pad_mask &
 *     get_sub_mask and passes down), packed by nnhipAttentionPackMask; when given it REPLACES key_valid and causal;
 *   attention dropout (the notebook's self.dropout(softmax(scores)), dropout.py:17-37): the multiplier of element
 *     (b,h,q,k) is dropout_mask[b,h,q,k] (0 or 1/(1-p): an injected mask, for parity tests against the oracle) or, with
 *     dropout_mask == NULL and dropout_p > 0, (hash(dropout_seed, b, h, q, k) >= p*2^32) / (1-p) -- a counter-based hash
 *     that the forward and both backward kernels re-evaluate (nothing is stored); nnhipAttentionDropoutMask writes the
 *     same multipliers out.  Pass the SAME options to the forward and the backward of one step. */
typedef struct nnhipAttentionOptions {
    const uint64_t* mask_bits;    /* [B, Tq, ceil(Tk/64)] */
    const uint64_t* mask_bitsT;   /* [B, Tk, ceil(Tq/64)] */
    const uint8_t* row_any;       /* [B, Tq] (NULL: no tile skipping under a dense mask) */
    const float* dropout_mask;    /* [B, H, Tq, Tk] */
    float dropout_p;
    uint32_t dropout_seed;
    const uint32_t* dropout_seed_dev; /* NULL, or a device word added to dropout_seed when the kernel runs: point it at a
                                       * per-step counter so that a captured hipGraph draws a fresh mask on every replay */
} nnhipAttentionOptions;
int nnhipAttentionForwardEx(const float* Q, const float* K, const float* V, const int32_t* key_valid, float* O,
                            float* LSE, int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t head_dim, int64_t ld_qkv,
                            float scale, int causal, const nnhipAttentionOptions* opts, nnhipStream_t stream);
int nnhipAttentionBackwardEx(const float* Q, const float* K, const float* V, const int32_t* key_valid, const float* O,
                             const float* dO, const float* LSE, float* dQ, float* dK, float* dV, int64_t B, int64_t H,
                             int64_t Tq, int64_t Tk, int64_t head_dim, int64_t ld_qkv, float scale, int causal,
                             const nnhipAttentionOptions* opts, nnhipStream_t stream);
/* mask [B,Tq,Tk] int32 (non-zero = visible) -> mask_bits, mask_bitsT, row_any (one launch). */
int nnhipAttentionPackMask(const int32_t* mask, uint64_t* mask_bits, uint64_t* mask_bitsT, uint8_t* row_any, int64_t B,
                           int64_t Tq, int64_t Tk, nnhipStream_t stream);
/* out [B,H,Tq,Tk] = the hash dropout multipliers the fused kernels use for (dropout_p, seed). */
int nnhipAttentionDropoutMask(float* out, int64_t B, int64_t H, int64_t Tq, int64_t Tk, float dropout_p, uint32_t seed,
                              nnhipStream_t stream);
/* The same with an optional device word added to the seed (the fused kernels' dropout_seed_dev: a per-step counter that lets a
 * captured hipGraph draw a fresh mask on every replay) -- what the UNFUSED attention path (need_weights = True) multiplies its
 * attention map by, so that both paths draw from the library's one counter hash.  ABI 208 */
int nnhipAttentionDropoutMaskEx(float* out, int64_t B, int64_t H, int64_t Tq, int64_t Tk, float dropout_p, uint32_t seed,
                                const uint32_t* seed_dev, nnhipStream_t stream);

/* ---- a9 fused CrossEntropy forward+backward  (replaces cudaCrossEntropyForwardBackward,
 *      cross_entropy.cu:249-260).
 *   logits [n_rows, logits_stride]; loss[n_rows], lse[n_rows] outputs; labels int32.
 *   reduction 'n' | 'm' | 's'.  Gradient scale for 'm' = 1/n_non_ignore, taken from the int
 *   argument, or -- if n_non_ignore_dev != NULL -- read from that device int (no host sync).
 *   dlogits: where to write (softmax - onehot)*scale.  NULL = in place over `logits`
 *   (the reference's behaviour, cross_entropy.cu:211); rows with label == ignore_index get zero
 *   gradient and zero loss.  dlogits has the same row stride as logits. */
int nnhipCrossEntropyForwardBackward(float* logits, float* loss, float* lse, const int32_t* labels,
                                     int64_t logits_stride, int32_t ignore_index, int64_t n_rows,
                                     int64_t n_cols, char reduction, int64_t n_non_ignore,
                                     const int32_t* n_non_ignore_dev, float* dlogits,
                                     nnhipStream_t stream);
/* out_count[0] = #{i : labels[i] != ignore_index}   (device scalar; replaces the host-side
 * cp.sum(labels != ignore_index).item() of cross_entropy.py:72) */
int nnhipCountNotEqual(const int32_t* labels, int64_t n, int32_t ignore_index, int32_t* out_count,
                       nnhipStream_t stream);
/* The 'mean' denominator on its own (labels int16/32/64): count_out[0] = #{labels != ignore_index} (int) and/or
 * denom_out[0] = that count -- or, with class weights, sum of class_weight[label] over those rows -- as a FLOAT.
 * Data-parallel use: every rank back-propagates reduction 's', writes its local denominator into the extra slot of the
 * gradient bucket with this call, and the all-reduced slot becomes the optimizer's gradient divisor
 * (nnhipFusedOptimizerSetGradDivisor): the global mean without a host read. */
int nnhipCrossEntropyDenominator(const void* labels, int32_t label_bytes, int64_t n, int64_t ignore_index,
                                 const float* class_weight_or_null, int64_t n_cols, int32_t* count_out_or_null,
                                 float* denom_out_or_null, nnhipStream_t stream);
/* out[0] = sum(loss_rows) ('s'), or sum/count ('m', count from count_dev) -- the device-side
 * reduction cross_entropy.py:98-101 does with cupy. */
int nnhipReduceLoss(const float* loss_rows, int64_t n_rows, char reduction,
                    const int32_t* count_dev, float* out, nnhipStream_t stream);
/* The three calls above as one launch (reduction 'm' or 's'): d(logits) (NULL = in place), per-row loss, lse, the reduced
 * loss (device scalar) and, for 'm', the non-ignored count (device int, also the 'mean' denominator).
 * = nnhipCrossEntropyLossEx with int32 labels and no class weights. */
int nnhipCrossEntropyLoss(float* logits, float* dlogits_or_null, float* loss_rows, float* lse, const int32_t* labels,
                          int64_t logits_stride, int32_t ignore_index, int64_t n_rows, int64_t n_cols, char reduction,
                          float* loss_out, int32_t* count_out, nnhipStream_t stream);

/* The whole CrossEntropyLoss (neunet/nn/losses.py:59-126) in ONE launch, any reduction:
 *   labels: int16 / int32 / int64 (label_bytes = 2 / 4 / 8; losses.py:100 accepts the three);
 *   class_weight [n_cols] or NULL: loss_i = -logp[y_i] * w[y_i]; 'm' divides by sum_i w[y_i] over non-ignored rows
 *     (losses.py:115-118); gradient rows are scaled by w[y_i];
 *   reduction 'n': loss_rows only (loss_out may be NULL); 'm' / 's': loss_out[0] as well;
 *   count_out (NULL-able): #{labels != ignore_index} for 'm'.
 * The 'mean' denominator is derived from the labels inside the launch (no count launch, no host sync); the per-block
 * loss sums meet in the last block to finish (arrival ticket).  A label outside [0, n_cols) that is not ignore_index
 * gives zero loss and zero gradient.  'mean' with no live row at all (every label ignored or out of range): loss 0 and a zero
 * gradient, as nnhipNLLLossForwardBackward, not NumPy's 0 / 0.  Rows of any width (looped above 16384 columns). */
int nnhipCrossEntropyLossEx(float* logits, float* dlogits_or_null, float* loss_rows, float* lse, const void* labels,
                            int32_t label_bytes, const float* class_weight_or_null, int64_t logits_stride,
                            int64_t ignore_index, int64_t n_rows, int64_t n_cols, char reduction,
                            float* loss_out_or_null, int32_t* count_out_or_null, nnhipStream_t stream);

/* A small classifier head and its loss in one launch: logits[rows, classes] = X * W^T + b (Linear.forward, linear.py:48-58), then
 * exactly nnhipCrossEntropyLossEx on them (out of place: dlogits != logits).  1 <= rows <= 256, 1 <= classes <= 32,
 * 1 <= in_features <= 2048, else NNHIP_EINVAL -- the two entries called separately give the same results.  At README-MLP scale
 * (32 x 128 -> 10) a launch is ~1/8 of the training step whatever it computes. */
int nnhipLinearCrossEntropyLoss(const float* X, const float* W, const float* b, float* logits, float* dlogits,
                                float* loss_rows, float* lse, const void* labels, int32_t label_bytes,
                                const float* class_weight_or_null, int64_t ignore_index, int64_t rows, int64_t in_features,
                                int64_t classes, char reduction, float* loss_out_or_null, int32_t* count_out_or_null,
                                nnhipStream_t stream);

/* ---- a10 RMSNorm  (replaces RMSNormForward/Backward, rmsnorm.cu:116-140, 282-308) ---------- */
/* X_std[rows] = sqrt(mean(x^2)+eps) always written.  X_norm[rows,cols] may be NULL (not stored;
 * the backward recomputes it) -- the reference always stores it. */
int nnhipRMSNormForward(const float* X, const float* weight, const float* bias_or_null, float* Y,
                        float* X_std, float* X_norm_or_null, int64_t rows, int64_t cols, float eps,
                        nnhipStream_t stream);
/* X_norm is accepted for signature parity and ignored (recomputed from X and X_std).  dW / db are finished inside the
 * same launch (per-block column partials + arrival ticket; the last blocks to arrive column-sum them).  Rows of any
 * width (looped above 16384 columns, like rmsnorm.cu:17-113). */
int nnhipRMSNormBackward(const float* dY, const float* X, const float* weight, const float* X_std,
                         const float* X_norm_unused, float* dX, float* dW, float* db_or_null,
                         int64_t rows, int64_t cols, nnhipStream_t stream);
/* dX = RMSNorm gradient + dX_addend (NULL-able): folds the accumulation onto a gradient X already holds. */
int nnhipRMSNormBackwardEx(const float* dY, const float* X, const float* weight, const float* X_std,
                           const float* X_norm_unused, const float* dX_addend, float* dX, float* dW,
                           float* db_or_null, int64_t rows, int64_t cols, nnhipStream_t stream);

/* ---- a11 fused AdamW  (replaces FusedAdamWStep, fused_adamw.cu:58-71 -- one tensor) --------- */
/* decay_mode 0: decoupled weight decay (AdamW, neunet/optim.py:52-69);
 * decay_mode 1: L2 decay folded into the gradient (Adam, neunet/optim.py:17-33).
 * grad_scale multiplies g on load (1.0 = reference behaviour; 1/world after a DP sum-all-reduce).
 * Hyper-parameters are DOUBLE (the reference passes float): the CPU path forms (1-beta) and
 * 1-beta^step from Python doubles (optim.py:27-31); (float)0.999 would put a 1.3e-5 relative error
 * into (1-beta2) and hence into v.  They are rounded to fp32 exactly where NumPy rounds them. */
int nnhipFusedAdamWStep(float* p, const float* g, float* m, float* v, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int32_t step, int64_t n,
                        int32_t decay_mode, float grad_scale, nnhipStream_t stream);

/* ---- a11 multi-tensor AdamW  (replaces CreateFusedOptimizer / DestroyFusedOptimizer /
 *      FusedAdamWStep(void*,...), fused_adamw_multitensor.cu:308-333) -------------------------- */
void* nnhipCreateFusedOptimizer(void);
int nnhipDestroyFusedOptimizer(void* opt);
/* p/g/m/v: HOST arrays of n_tensors DEVICE pointers; sizes: HOST array of element counts.
 * One kernel launch for all tensors.  Tables are re-uploaded only when they changed. */
int nnhipFusedAdamWMultiTensorStep(void* opt, int32_t n_tensors, float* const* p,
                                   const float* const* g, float* const* m, float* const* v,
                                   const int64_t* sizes, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, int32_t step, int32_t decay_mode,
                                   float grad_scale, nnhipStream_t stream);

/* Device-driven stepping for hipGraph replay (a captured launch freezes its by-value arguments): after
 * nnhipFusedOptimizerSetStep(opt, t) AND nnhipFusedOptimizerSetHyper(...), calls of nnhipFusedAdamWMultiTensorStep with
 * step == 0 take the step count (advanced by the kernel itself), lr, weight_decay and grad_scale from device memory;
 * the lr / weight_decay / grad_scale ARGUMENTS of such a call are ignored.  Both setters are stream-ordered launches
 * (no synchronisation): call SetHyper between replays to run an LR schedule or change the DP gradient scale. */
int nnhipFusedOptimizerSetStep(void* opt, int32_t step, nnhipStream_t stream);
int nnhipFusedOptimizerSetHyper(void* opt, double lr, double weight_decay, float grad_scale, nnhipStream_t stream);
/* Gradients are additionally divided by divisor_dev[0] (a device float; NULL switches it off): with
 * CrossEntropy(ignore_index) under data parallelism every rank back-propagates the SUM loss and the all-reduced count
 * of non-ignored targets (one extra float in the gradient bucket) is the divisor -- no host read, no scale pass. */
int nnhipFusedOptimizerSetGradDivisor(void* opt, const float* divisor_dev_or_null);

/* ---- SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax, NAdam (net-new exports, ABI 221; csrc/optim_rules.hip: the reference has
 *      no CUDA kernels for them).  CPU semantics: neunet/optim.py:76-244.  A rule moves only the streams it has:
 *        rule      state streams            coef1     coef2   bytes / element
 *        SGD       -                        -         -       12
 *        MOMENTUM  s1 = m                   momentum  -       20
 *        RMSPROP   s1 = m                   alpha     -       20
 *        ADAGRAD   s1 = m                   -         -       20
 *        ADADELTA  s1 = m, s2 = v           rho       -       28   (lr is not part of the reference's rule: ignored)
 *        ADAMAX    s1 = m, s2 = v           beta1     beta2   28
 *        NADAM     s1 = m, s2 = v           beta1     beta2   28
 *   State pointers / tables a rule does not have may be NULL; coefficients it does not have are ignored.  Hyper-parameters are
 *   DOUBLE and rounded to fp32 where NumPy rounds them, (1 - coef) and 1 - beta^step formed in double first, as for
 *   nnhipFusedAdamWStep.  grad_scale multiplies g on load.  Status codes, never an exit: NNHIP_EINVAL for an unknown rule, a NULL
 *   state pointer the rule needs, a negative size, step < 1 (per-tensor entry) or step == 0 without nnhipFusedOptimizerSetStep and
 *   SetHyper (multi-tensor entry); n == 0 / n_tensors == 0 return 0 without a launch. */
enum {
    NNHIP_OPT_SGD = 0,
    NNHIP_OPT_MOMENTUM = 1,
    NNHIP_OPT_RMSPROP = 2,
    NNHIP_OPT_ADAGRAD = 3,
    NNHIP_OPT_ADADELTA = 4,
    NNHIP_OPT_ADAMAX = 5,
    NNHIP_OPT_NADAM = 6
};
/* One tensor, one launch. */
int nnhipOptimizerRuleStep(int32_t rule, float* p, const float* g, float* s1, float* s2, int64_t n, double lr, double coef1,
                           double coef2, double eps, int32_t step, float grad_scale, nnhipStream_t stream);
/* All tensors in one launch, on a handle of nnhipCreateFusedOptimizer: tables and sizes as nnhipFusedAdamWMultiTensorStep, the
 * plan re-uploaded only when it changed.  step == 0: device-driven stepping (hipGraph replay) -- the step count, lr and grad_scale
 * come from the handle's device state (nnhipFusedOptimizerSetStep / SetHyper; the weight_decay written there is unused), and the
 * kernel advances the step itself.  nnhipFusedOptimizerSetGradDivisor is honoured as by the Adam entry. */
int nnhipOptimizerRuleMultiTensorStep(void* opt, int32_t rule, int32_t n_tensors, float* const* p, const float* const* g,
                                      float* const* s1, float* const* s2, const int64_t* sizes, double lr, double coef1,
                                      double coef2, double eps, int32_t step, float grad_scale, nnhipStream_t stream);

/* ---- Gradient clipping by global norm (net-new exports, ABI 226; csrc/grad_norm.hip: the reference has no gradient clipping).
 *   The norm of ALL gradient tensors in one launch, finished inside that launch (no float atomics: the same gradients give the same
 *   bits; no memset, no host synchronisation: legal in a captured step), on a handle of nnhipCreateFusedOptimizer.  The result is the
 *   one-float device word the update kernels already divide the gradient by (nnhipFusedOptimizerSetGradDivisor): clipping needs no
 *   pass over the gradients.
 *   words: 4 device floats.
 *     out [0] = the norm of the EFFECTIVE gradient g * gs, gs = grad_scale / divisor_in[0] -- the factor the update kernels apply:
 *               |gs| * sqrt(sum g^2) (NNHIP_NORM_L2; float32 sums per block, the blocks' sums added in double) or |gs| * max |g|
 *               (NNHIP_NORM_INF; exact, and a NaN element gives NaN)
 *     out [1] = the divisor an update must use = divisor_in[0] * max(1, (norm + 1e-6f) / max_norm): torch's clip_coef, clamped,
 *               inverted (divisor_in == NULL counts as 1; equal to divisor_in[0] bit for bit when nothing is clipped; NaN when the
 *               norm is NaN)
 *     out [2] = 1.0f when the norm is NaN or inf, else 0.0f
 *     in  [3] = max_norm for step == 0
 *   g / sizes: HOST arrays of n_tensors DEVICE pointers / element counts, as nnhipFusedAdamWMultiTensorStep's; the plan (the handle's
 *   second plan slot, so the update's plan stays cached) is re-uploaded only when it changed.  step >= 1: grad_scale and max_norm are
 *   the arguments.  step == 0: device-driven stepping -- grad_scale comes from the handle's device state (nnhipFusedOptimizerSetStep /
 *   SetHyper) and max_norm from words[3]; the two arguments are ignored.  The handle's bound divisor is not read: pass it as
 *   divisor_in.  n_tensors == 0 or all sizes 0: one one-block launch writes norm 0, divisor = divisor_in[0] (or 1), flag 0.
 *   NNHIP_EINVAL: NULL handle, NULL words, NULL table with n_tensors > 0, negative n_tensors / size / step, NULL tensor pointer with a
 *   non-zero size, unknown norm_type, max_norm NaN or <= 0 at step >= 1, step == 0 without SetStep and SetHyper.  NNHIP_EALIGN: a
 *   tensor, words or divisor pointer that is not 4-byte aligned.  NNHIP_ENOMEM: the handle's partials buffer (one float per block,
 *   grow-only) would have to grow inside a stream capture -- run the step eagerly once first.  A refused call launches nothing. */
enum { NNHIP_NORM_L2 = 0, NNHIP_NORM_INF = 1 };
int nnhipGradNormMultiTensor(void* opt, int32_t n_tensors, const float* const* g, const int64_t* sizes, int32_t norm_type,
                             double max_norm, const float* divisor_in_or_null, int32_t step, float grad_scale, float* words,
                             nnhipStream_t stream);
/* g[i] /= divisor_dev[0] for every tensor, in place, one launch, on the same plan slot: for callers that clip without one of the
 * optimizers here or want to look at the clipped gradients.  A divisor of 1.0f leaves every bit as it is.  Status codes as above
 * (NULL divisor_dev: NNHIP_EINVAL); n_tensors == 0 or all sizes 0: returns 0 without a launch. */
int nnhipScaleMultiTensor(void* opt, int32_t n_tensors, float* const* g, const int64_t* sizes, const float* divisor_dev,
                          nnhipStream_t stream);

/* ---- a3/a4 Conv2d  (net-new exports; reference CPU: neunet/nn/layers/conv2d.py:297-355, 16-115)
 *   X [B,Cin,H,W], W [Cout,Cin,kh,kw], bias [Cout] or NULL, O [B,Cout,Ho,Wo]; NCHW fp32.
 *   pad = (up, down, left, right) as Conv2d.build resolves it (conv2d.py:237-243);
 *   Ho = (H+pu+pd-dh*(kh-1)-1)/sh+1 (conv2d.py:245-258), likewise Wo. */
typedef struct nnhipConv2dDesc {
    int64_t B, Cin, H, W, Cout, kh, kw;
    int64_t sh, sw, dh, dw;
    int64_t pu, pd, pl, pr;
} nnhipConv2dDesc;
int nnhipConv2dForward(const float* X, const float* W, const float* bias, float* O,
                       const nnhipConv2dDesc* d, nnhipStream_t stream);
/* dX/dW/db may be NULL (skipped). */
int nnhipConv2dBackward(const float* X, const float* W, const float* dO, float* dX, float* dW,
                        float* db, const nnhipConv2dDesc* d, nnhipStream_t stream);

/* ---- ConvTranspose2d  (net-new exports, ABI 216; reference CPU: neunet/nn/layers/convtranspose2d.py:249-262, 293-384, 16-120)
 *   X [B,Cin,H,W], W [Cout,Cin,kh,kw] (the reference's layout, NOT torch's [in,out,kh,kw]), bias [Cout] or NULL, O [B,Cout,Ho,Wo].
 *   O[b,o,y,x] = bias[o] + sum_{i,k,l} W[o,i,k,l] X[b,i,h,w]  with  h sh = y + pu - (kh-1-k) dh,  w sw = x + pl - (kw-1-l) dw
 *   (terms with exact divisions and 0 <= h < H, 0 <= w < W);  Ho = (H-1) sh - (pu+pd) + dh (kh-1) + oph + 1, likewise Wo.
 *   = torch conv_transpose2d(X, W.flip(2,3).transpose(0,1), bias, stride, padding, output_padding, dilation) for symmetric padding;
 *   pd / pr and the output padding only change Ho / Wo.  Padding beyond d (k-1) and strides beyond the kernel are accepted;
 *   output padding must stay below max(stride, dilation) per axis (NNHIP_EINVAL otherwise).  Status rules as nnhipConv2d*:
 *   bad descriptor / empty output / a tensor of 2 GiB or more / null required pointer: NNHIP_EINVAL; B == 0: NNHIP_OK, nothing
 *   launched; 4-byte alignment suffices.  Deterministic; dW / db are written, not accumulated. */
typedef struct nnhipConvTranspose2dDesc {
    int64_t B, Cin, H, W, Cout, kh, kw;
    int64_t sh, sw, dh, dw;
    int64_t pu, pd, pl, pr;
    int64_t oph, opw;
} nnhipConvTranspose2dDesc;
int nnhipConvTranspose2dForward(const float* X, const float* W, const float* bias, float* O,
                                const nnhipConvTranspose2dDesc* d, nnhipStream_t stream);
/* dX/dW/db may be NULL (skipped). */
int nnhipConvTranspose2dBackward(const float* X, const float* W, const float* dO, float* dX, float* dW, float* db,
                                 const nnhipConvTranspose2dDesc* d, nnhipStream_t stream);
/* How a forward runs.  Stride 1 with pu <= dh (kh-1), pl <= dw (kw-1) always goes to nnhipConv2d* (CONV2D: it is a Conv2d of the
 * same weight; so do its three gradients).  Otherwise PHASE = one dense implicit GEMM per stride phase over exactly the taps that
 * reach it, GATHER = the Conv2d input-gradient kernel, which walks every tap for every output pixel (handles everything).
 * AUTO: PHASE where every phase has at least one tap, GATHER otherwise.  A request for PHASE falls to GATHER at stride 1 and
 * above 65535 phases.  The setter returns the previous value (an unknown route changes nothing); process-wide. */
#define NNHIP_CONVT_ROUTE_AUTO 0
#define NNHIP_CONVT_ROUTE_PHASE 1
#define NNHIP_CONVT_ROUTE_GATHER 2
#define NNHIP_CONVT_ROUTE_CONV2D 3   /* reported by nnhipConvTranspose2dPlan only */
int nnhipSetConvTransposeRoute(int route);
int nnhipGetConvTransposeRoute(void);
/* Host only, no device work: the plan the forward would use.  Returns the number of stride phases (sh*sw) and fills, per phase
 * (row-major in (py, px) = ((y+pu) mod sh, (x+pl) mod sw)), the number of taps that reach it and the number of output pixels per
 * image in it; *route = the route AUTO resolves to.  capacity < phases (or a bad descriptor / null pointer): NNHIP_EINVAL. */
int nnhipConvTranspose2dPlan(const nnhipConvTranspose2dDesc* d, int32_t* route, int32_t* phase_taps, int32_t* phase_pixels,
                             int32_t capacity);

/* ---- Embedding (reference CPU: neunet/nn/layers/embedding.py:61-75 via
 *      Tensor.__getitem__, neunet/autograd.py:895-916) ------------------------------------------------
 * out[p,:] = weight[ids[p],:] * scale + (pe ? pe[p % seq_len,:] : 0);  ids int32 (negative = from the end).
 * Backward reproduces the reference's ASSIGNMENT semantics (autograd.py:909-910): for repeated ids only
 * the last occurrence contributes:  dW[v,:] = scale * grad_out[last_pos(v),:], 0 for unused rows. */
int nnhipEmbeddingForward(float* out, const float* weight, const int32_t* ids, const float* pe,
                          int64_t n_ids, int64_t dim, int64_t seq_len, int64_t vocab, float scale,
                          nnhipStream_t stream);
int nnhipEmbeddingBackward(float* dW, const float* grad_out, const int32_t* ids, int64_t n_ids,
                           int64_t dim, int64_t vocab, float scale, nnhipStream_t stream);
/* out[i] = (ids[i] != value) as int32: the key-padding mask of examples/gpt.ipynb cell 7 (get_pad_mask:
 * (x != pad_idx).astype(int)) without leaving the library (torch would run a compare and a cast kernel).  ABI 203 */
int nnhipNotEqualInt32(int32_t* out, const int32_t* ids, int64_t n, int32_t value, nnhipStream_t stream);
/* neunet.argmax (neunet/__init__.py:132-139 = np.argmax cast to int32): out[o, j] = index of the FIRST maximum of
 * x[o, :, j] over the middle axis of the C-contiguous view [outer, n, inner] (axis = -1: inner = 1; axis = None: outer = inner
 * = 1, n = numel); a NaN counts as the maximum, the first NaN wins (NumPy's rule).  out int32 [outer, inner].  Bit-exact: a
 * comparison network on (value, index) pairs, no arithmetic.  n == 0 with outer * inner > 0 is NNHIP_EINVAL (NumPy raises
 * ValueError).  ABI 208 */
int nnhipArgmaxF32(int32_t* out, const float* x, int64_t outer, int64_t n, int64_t inner, nnhipStream_t stream);
/* Dropout (neunet/nn/layers/dropout.py:17-37): out[i] = in[i] * m(i), m(i) = 1/(1-p) with probability 1-p, else 0, from a
 * counter-based hash of (seed + *seed_dev, i) -- never stored: the backward pass calls the same entry with the upstream
 * gradient as `in` (same seed) and gets dX = dY * m.  seed_dev (optional device uint32, e.g. a step counter) makes a
 * captured hipGraph draw a fresh mask on every replay.  out may alias in.  ABI 203 */
int nnhipDropout(float* out, const float* in, int64_t n, float p, uint32_t seed, const uint32_t* seed_dev,
                 nnhipStream_t stream);
/* *word += by (one thread): the per-step device counter that nnhipDropout / the attention kernels add to their dropout
 * seed, advanced on the stream in front of a graph replay.  ABI 203 */
int nnhipIncrementU32(uint32_t* word, uint32_t by, nnhipStream_t stream);

/* ---- the rest of the conv-classifier step (examples/convolutional_digits_classifier.ipynb) ----
 * LeakyReLU (neunet/nn/activations.py:60-84): f = x <= 0 ? alpha*x : x ; dx = dy * (f <= 0 ? alpha : 1). */
int nnhipLeakyReLUForward(float* out, const float* in, float alpha, int64_t size, nnhipStream_t stream);
int nnhipLeakyReLUBackward(float* dIn, const float* dOut, const float* out, float alpha, int64_t size,
                           nnhipStream_t stream);
/* Sigmoid (activations.py:9-28): f = 1/(1+exp(-x)) ; dx = dy * f * (1 - f), `out` = forward output. */
int nnhipSigmoidForward(float* out, const float* in, int64_t size, nnhipStream_t stream);
int nnhipSigmoidBackward(float* dIn, const float* dOut, const float* out, int64_t size, nnhipStream_t stream);
/* MaxPool2d (neunet/nn/layers/maxpool2d.py:85-249), NCHW, dilation 1.  pad = (up, down, left, right), padded
 * with -inf; argmax[b,c,ho,wo] = r*kw + s of the FIRST maximum (np.nanargmax).  Backward gathers, so
 * overlapping windows accumulate deterministically. */
typedef struct nnhipPool2dDesc {
    int64_t B, C, H, W, kh, kw, sh, sw, pu, pd, pl, pr;
    int64_t dh, dw;   /* dilation (maxpool2d.py:170-186: taps at r*dh, s*dw; 0 is read as 1).  ABI 203 */
} nnhipPool2dDesc;
int nnhipMaxPool2dForward(float* out, int32_t* argmax, const float* X, const nnhipPool2dDesc* d,
                          nnhipStream_t stream);
int nnhipMaxPool2dBackward(float* dX, const float* dY, const int32_t* argmax, const nnhipPool2dDesc* d,
                           nnhipStream_t stream);
/* MaxPool2d(LeakyReLU(X; alpha)) forward / backward as ONE launch each (alpha > 0): the composition
 * neunet/nn/activations.py:72-84 -> neunet/nn/layers/maxpool2d.py:85-249 of the conv classifier.  `out`/`argmax` as above;
 * the backward takes the pooled forward output and returns the gradient of the LeakyReLU's INPUT. */
int nnhipMaxPool2dLeakyForward(float* out, int32_t* argmax, const float* X, float alpha, const nnhipPool2dDesc* d,
                               nnhipStream_t stream);
int nnhipMaxPool2dLeakyBackward(float* dX, const float* dY, const int32_t* argmax, const float* pooled, float alpha,
                                const nnhipPool2dDesc* d, nnhipStream_t stream);
/* AvgPool2d (neunet/nn/layers/avgpool2d.py:14-46, :126-172), NCHW float32, on the same descriptor; dh / dw must be 0 or 1 (the
 * layer has no dilation).  pad = (up, down, left, right), padded with zeros that COUNT in the mean:
 *   out[b,c,ho,wo] = (sum of the window's taps inside the image) / (kh kw),   Ho = (H + pu + pd - kh) / sh + 1 (floor), Wo likewise.
 * A window wholly inside the padding gives 0.  Backward is a gather: dX[b,c,y,x] = (sum of dY over the windows that cover (y, x), in
 * (ho, wo) order) / (kh kw); an input pixel no window covers (stride > kernel, rows / columns left over by the floor) gets +0.  Both
 * entries write every element of their output exactly once, in ONE launch, with no memset, atomics or workspace: reruns are
 * bit-identical and the launches may be captured into a hipGraph.  NaN and +-inf propagate as the arithmetic gives.
 * Three kernel tiers, by descriptor alone (nnhipAvgPool2dTier): TILES when kernel == stride, no padding and
 * H = Ho kh, W = Wo kw (one thread per window; 16-byte accesses only where W and the base pointers allow); GLOBAL_WAVE / _BLOCK
 * when kh = H, kw = W, no padding (one wave per plane up to 1024 elements, one block per plane above); GENERAL otherwise.
 * Refused before any launch, outputs untouched -- NNHIP_EINVAL: a NULL pointer or descriptor; B, C, H, W, kh, kw, sh or sw < 1 (so
 * B * C == 0 is not accepted); a negative pad; dilation > 1; an output extent < 1; an input or output of 2^31 elements or more (the
 * kernels index with 32 bits).  NNHIP_EALIGN: a pointer that is not 4-byte aligned.  ABI 225 */
int nnhipAvgPool2dForward(float* out, const float* X, const nnhipPool2dDesc* d, nnhipStream_t stream);
int nnhipAvgPool2dBackward(float* dX, const float* dY, const nnhipPool2dDesc* d, nnhipStream_t stream);
#define NNHIP_AVGPOOL_TIER_GENERAL 0
#define NNHIP_AVGPOOL_TIER_TILES 1
#define NNHIP_AVGPOOL_TIER_GLOBAL_WAVE 2
#define NNHIP_AVGPOOL_TIER_GLOBAL_BLOCK 3
/* The tier both entries take for this descriptor under the current route (host only, no device call), or NNHIP_EINVAL. */
int nnhipAvgPool2dTier(const nnhipPool2dDesc* d);
#define NNHIP_AVGPOOL_ROUTE_AUTO 0
#define NNHIP_AVGPOOL_ROUTE_GENERAL 1    /* every descriptor on the general tier: for tests and A/B timing (tools/kbench.py) */
/* Process-wide; returns the previous route.  An unknown value changes nothing. */
int nnhipSetAvgPool2dRoute(int route);
/* Conv2d weight / bias gradient straight from the gradient of a MaxPool2d that consumed the conv's output, through an optional
 * LeakyReLU (the backward of conv2d.py:16-115 composed with maxpool2d.py:11-82 and activations.py:72-84, restricted to dW, db):
 *   dW, db of   P = MaxPool2d([LeakyReLU(] Conv2d(X) [; alpha)])   given dP, the pool's window-local arg-max and -- with the
 *   activation -- the pooled output P (its sign is the activation's slope at the arg-max); pooled = NULL: no activation.
 * For a conv whose INPUT needs no gradient and whose output nobody else reads (the conv classifier's first layer): the conv-output
 * gradient [B,Cout,Ho,Wo] is never materialised and the pool's backward launch is not needed.  Pool windows must tile the conv
 * output exactly (kernel == stride, no padding, no dilation, Ho % kh == Wo % kw == 0, kh*kw <= 16) and the conv must be in the
 * small-channel 3x3 domain of the LDS-resident weight-gradient kernel: nnhipConv2dWeightGradPooledOk(conv, pool) = 1 says so
 * (0 otherwise; the pool descriptor's B, C, H, W are the conv output's).  Same values as nnhipMaxPool2d[Leaky]Backward followed by
 * nnhipConv2dBackward(dX = NULL).  ABI 206 */
int nnhipConv2dWeightGradPooledOk(const nnhipConv2dDesc* conv, const nnhipPool2dDesc* pool);
int nnhipConv2dWeightGradPooled(const float* X, const float* dP, const int32_t* argmax, const float* pooled, float alpha,
                                float* dW, float* db, const nnhipConv2dDesc* conv, const nnhipPool2dDesc* pool,
                                nnhipStream_t stream);
/* P = MaxPool2d(2, 2)(LeakyReLU(Conv2d(X); alpha)) and the pool's window-local arg-max in ONE launch (alpha = 1: no activation)
 * -- conv2d.py:297-355 -> activations.py:79-81 -> maxpool2d.py:85-249 for a 3x3, unit-stride, unit-dilation conv with few input
 * channels (Cin <= 4 < Cout <= 16) whose output the windows tile exactly and a batch large enough that one thread per window
 * fills the chip (...Ok = 1; else 0: call the three entries).  The conv output is not written: the chain's backward needs only
 * the arg-max and P (nnhipMaxPool2dLeakyBackward, nnhipConv2dWeightGradPooled).  The same products in the same order as the separate
 * entries (values agree to an ulp or two: the compiler's choice of fused multiply-adds differs between the kernels).  ABI 207 */
int nnhipConv2dLeakyMaxPoolForwardOk(const nnhipConv2dDesc* conv, const nnhipPool2dDesc* pool);
int nnhipConv2dLeakyMaxPoolForward(const float* X, const float* W, const float* bias, float alpha, float* P, int32_t* argmax,
                                   const nnhipConv2dDesc* conv, const nnhipPool2dDesc* pool, nnhipStream_t stream);
/* BatchNorm2d (neunet/nn/layers/batchnorm2d.py:57-115, 11-54), X [B,C,HW].  training != 0: batch mean / biased
 * variance per channel, running = momentum*running + (1-momentum)*stat (the reference's convention; running_*
 * may be NULL); else the running statistics are used.  save_mean / save_inv [C] feed the backward.
 * weight / bias [C] may both be NULL (affine = False). */
int nnhipBatchNorm2dForward(const float* X, const float* weight, const float* bias, float* Y, float* save_mean,
                            float* save_inv, float* running_mean, float* running_var, int64_t B, int64_t C,
                            int64_t HW, float eps, float momentum, int training, nnhipStream_t stream);
int nnhipBatchNorm2dBackward(const float* dY, const float* X, const float* weight, const float* save_mean,
                             const float* save_inv, float* dX, float* dW, float* db, int64_t B, int64_t C,
                             int64_t HW, nnhipStream_t stream);
/* The tail of the reference's conv classifier (examples/convolutional_digits_classifier.ipynb cell 2) as ONE launch, without any block
 * waiting for another.  Producer side: nnhipConv2dLeakyMaxPoolForwardStats = nnhipConv2dLeakyMaxPoolForward that also leaves, per block
 * of 64 pooling windows and per output channel, (mean, M2 = sum of squared deviations) of the pooled values in stats
 * [blocks][Cout][2]; nnhipConv2dLeakyMaxPoolStatsBlocks = that block count (0: no statistics variant for the geometry).
 * Consumer side: nnhipBatchNorm2dLinearSigmoidMSE = BatchNorm2d(training) on X [B,C,HW] (statistics combined from the pairs, Chan
 * et al., in a fixed order) -> reshape [B, C*HW] -> Linear(W [N, C*HW], b [N] or NULL) -> Sigmoid -> MSELoss against target [B,N].
 * Y / save_mean / save_inv / running statistics as nnhipBatchNorm2dForward (equal to rounding: combined instead of two-pass
 * statistics), pred [B,N] = the Sigmoid output, dz [B,N] = d(loss)/d(Linear output), loss[0] = mean squared error.
 * C <= 16, N <= 16, C*HW % 4 == 0 and <= 2048, B <= 4096 (...Fits answers 1 / 0); nstat * count == B * HW.  ABI 209 */
int nnhipConv2dLeakyMaxPoolStatsBlocks(const nnhipConv2dDesc* conv, const nnhipPool2dDesc* pool);
int nnhipConv2dLeakyMaxPoolForwardStats(const float* X, const float* W, const float* bias, float alpha, float* P, int32_t* argmax,
                                        const nnhipConv2dDesc* conv, const nnhipPool2dDesc* pool, float* stats, nnhipStream_t stream);
int nnhipBatchNorm2dLinearSigmoidMSEFits(int64_t B, int64_t C, int64_t HW, int64_t N);
int nnhipBatchNorm2dLinearSigmoidMSE(const float* X, const float* stats, int64_t nstat, int64_t count, const float* bn_weight,
                                     const float* bn_bias, float* Y, float* save_mean, float* save_inv, float* running_mean,
                                     float* running_var, int64_t B, int64_t C, int64_t HW, float eps, float momentum, const float* W,
                                     const float* b, int64_t N, const float* target, float* pred, float* dz, float* loss,
                                     nnhipStream_t stream);
/* MSELoss (neunet/nn/losses.py:9-22): loss[0] = sum((pred-target)^2)/n ; dpred = 2 (pred-target)/n (may be NULL). */
int nnhipMSELossForwardBackward(const float* pred, const float* target, float* loss, float* dpred, int64_t n,
                                nnhipStream_t stream);
/* MSELoss(Sigmoid(z), target) with the Sigmoid backward folded in: `pred` = the sigmoid output, dz_out = d(loss)/dz
 * (neunet/nn/losses.py:9-22 composed with neunet/nn/activations.py:12-13; the conv classifier's last two modules). */
int nnhipMSELossSigmoidForwardBackward(const float* pred, const float* target, float* loss, float* dz_out, int64_t n,
                                       nnhipStream_t stream);

/* ---- the MLP generative examples (examples/gan.ipynb, examples/vae.ipynb).  ABI 218 ---------------------------------------
 * BatchNorm1d (neunet/nn/layers/batchnorm1d.py:46-99 forward, 15-41 backward), X [N,F] row-major (csrc/batchnorm1d.hip).
 * training != 0: batch mean and BIASED variance over axis 0, two passes (np.var); running = momentum*running + (1-momentum)*stat
 * (the reference's convention, :76-81; running_* may both be NULL); else mean / variance are the running statistics.  save_mean /
 * save_inv [F] are written in BOTH modes: the backward is the reference's one formula whatever the mode (in eval it reads
 * X - running_mean and treats that mean and 1/std as batch statistics).  weight / bias [F] may both be NULL (affine = False), and
 * so may dW / db.  One launch per call; no workspace, no atomics, no host synchronisation (legal inside a stream capture); sums
 * in a fixed order (reruns are bit-identical).  Features run along the lanes and a block owns a strip of features: a column is
 * NEVER split across blocks, so a very tall, narrow input (N >> 10^4 with a few features) is a few blocks walking long columns --
 * slow by construction.  1 <= N < 2^31, 1 <= F < 2^31, else NNHIP_EINVAL.  N = 1 in training: var = 0, Y = bias, dX = 0. */
int nnhipBatchNorm1dForward(const float* X, const float* weight, const float* bias, float* Y, float* save_mean,
                            float* save_inv, float* running_mean, float* running_var, int64_t N, int64_t F, float eps,
                            float momentum, int training, nnhipStream_t stream);
int nnhipBatchNorm1dBackward(const float* dY, const float* X, const float* weight, const float* save_mean,
                             const float* save_inv, float* dX, float* dW, float* db, int64_t N, int64_t F,
                             nnhipStream_t stream);
/* Tanh (neunet/nn/activations.py:107-126): out = tanh(in) ; dIn = dOut * (1 - out^2), `out` = forward output. */
int nnhipTanhForward(float* out, const float* in, int64_t size, nnhipStream_t stream);
int nnhipTanhBackward(float* dIn, const float* dOut, const float* out, int64_t size, nnhipStream_t stream);
/* BCELoss (neunet/nn/losses.py:36-53): term = -(y log p + (1-y) log(1-p)) * w, the reference's expression literally (no clamp:
 * p = 0 or 1 gives inf / NaN as np.log does).  w = weight[i] (an array of n) or, weight == NULL, weight_scalar.  reduction 'm':
 * loss[0] = sum / n, 's': loss[0] = sum, 'n': loss[0..n) = the terms.  dpred (may be NULL) = d(loss)/dpred, scale = 1/n for 'm',
 * else 1: -(y/p - (1-y)/(1-p)) w scale; sigmoid_fold != 0: pred is a Sigmoid's output and dpred receives the gradient of the
 * Sigmoid's INPUT, (p - y) w scale (losses.py composed with activations.py:12-13) -- finite at a saturated p. */
int nnhipBCELossForwardBackward(const float* pred, const float* target, const float* weight, float weight_scalar, float* loss,
                                float* dpred, int64_t n, char reduction, int sigmoid_fold, nnhipStream_t stream);
/* The VAE's latent expressions (examples/vae.ipynb: VAE.reparameterize, VAE.loss_function).
 * Reparameterisation: std_out = exp(logvar / 2), z = mu + eps * std_out ; backward dmu = dz, dlogvar = dz * eps * 0.5 * std.
 * KL term: loss[0] = -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) ; dmu = mu, dlogvar = 0.5 (exp(logvar) - 1) (both may be NULL). */
int nnhipGaussianReparamForward(const float* mu, const float* logvar, const float* eps, float* z, float* std_out, int64_t n,
                                nnhipStream_t stream);
int nnhipGaussianReparamBackward(const float* dz, const float* eps, const float* std_saved, float* dmu, float* dlogvar, int64_t n,
                                 nnhipStream_t stream);
int nnhipGaussianKLDForwardBackward(const float* mu, const float* logvar, float* loss, float* dmu, float* dlogvar, int64_t n,
                                    nnhipStream_t stream);

/* ---- the remaining activations and losses of neunet.nn (ABI 222) ----------------------------------------------------------------
 * Softplus, Softsign, Mish, TanhExp, ELU, SELU (neunet/nn/activations.py:140-194, 250-383) and Tensor.log (neunet/autograd.py:357)
 * as functors on the elementwise map kernels.  out = f(in) ; dIn = dOut * f'(in): the backward reads the forward INPUT (12 B per
 * element), never the output.  `alpha` is ELU's, ignored by every other kind.  size 0: nothing to do.
 * The reference's float32 expressions overflow or cancel -- log(1 + exp(x)) is inf above 88 and exactly 0 below -17, the Mish
 * backward forms exp(3x), the TanhExp backward inf * 0 above 88, the ELU backward's alpha + f cancels -- so the kernels evaluate the
 * SAME mathematical functions in forms that stay finite and keep relative accuracy (as nnhipGELUForward does):
 *   NNHIP_ACT_SOFTPLUS  max(x, 0) + log1p(exp(-|x|))                    f' = sigmoid(x)
 *   NNHIP_ACT_SOFTSIGN  x / (1 + |x|)                                   f' = 1 / (1 + |x|)^2
 *   NNHIP_ACT_MISH      x t, t = tanh(softplus(x)) = n (n + 2) / (n (n + 2) + 2), n = exp(x)
 *                                                                       f' = t + x sigmoid(x) (1 - t^2)
 *   NNHIP_ACT_TANHEXP   x t, t = tanh(exp(x))                           f' = t + x exp(x) (1 - t^2); the second term is exactly 0
 *                                                                            once 1 - t^2 is 0: no inf * 0
 *   NNHIP_ACT_ELU       x <= 0 ? alpha expm1(x) : x                     f' = x <= 0 ? alpha exp(x) : 1   (alpha at x = 0)
 *   NNHIP_ACT_SELU      lambda (x > 0 ? x : a expm1(x))                 f' = lambda (x > 0 ? 1 : a exp(x)) (lambda a at x = 0);
 *                       lambda, a: the reference's two constants (activations.py:372-373)
 *   NNHIP_ACT_LOG       log(x), literally: log(0) = -inf, negative -> NaN  f' = 1 / x
 * A NaN input gives a NaN output and a NaN gradient in every kind. */
#define NNHIP_ACT_SOFTPLUS 0
#define NNHIP_ACT_SOFTSIGN 1
#define NNHIP_ACT_MISH 2
#define NNHIP_ACT_TANHEXP 3
#define NNHIP_ACT_ELU 4
#define NNHIP_ACT_SELU 5
#define NNHIP_ACT_LOG 6
/* ABI 223, the unary maps of the Tensor tape (neunet/autograd.py:339-440, 588-602), the library functions literally:
 *   NNHIP_ACT_EXP   exp(x)   f' = exp(x)          NNHIP_ACT_SQRT  sqrt(x)  f' = 0.5 / sqrt(x) (inf at 0, NaN below)
 *   NNHIP_ACT_SIN   sin(x)   f' = cos(x)          NNHIP_ACT_COS   cos(x)   f' = -sin(x)
 *   NNHIP_ACT_ABS   |x|      f' = sign(x) (0 at 0)
 * Kind 7 is not assigned: it stays an unknown kind. */
#define NNHIP_ACT_EXP 8
#define NNHIP_ACT_SQRT 9
#define NNHIP_ACT_SIN 10
#define NNHIP_ACT_COS 11
#define NNHIP_ACT_ABS 12
int nnhipActivationForward(int kind, float* out, const float* in, float alpha, int64_t size, nnhipStream_t stream);
int nnhipActivationBackward(int kind, float* dIn, const float* dOut, const float* in, float alpha, int64_t size,
                            nnhipStream_t stream);
/* LogSoftmax (neunet/nn/activations.py:462-492) over slices addressed like nnhipSoftmaxForward's (num_slices, slice_size, stride),
 * with the same three layouts and the same dispatch.  y = x - m - log(sum exp(x - m)), m the slice's maximum, the slice held in
 * registers between the passes; dX = dY - exp(Y) * sum_c dY, Y the forward OUTPUT.  Sums in a fixed order, no atomics (reruns are
 * bit-identical), no workspace.  A zero size is a no-op. */
int nnhipLogSoftmaxForward(float* out, const float* in, int64_t num_slices, int64_t slice_size, int64_t stride,
                           nnhipStream_t stream);
int nnhipLogSoftmaxBackward(float* dX, const float* dY, const float* Y, int64_t num_slices, int64_t slice_size, int64_t stride,
                            nnhipStream_t stream);
/* NLLLoss (neunet/nn/losses.py:83-126).  logp [outer, n_cols, inner] (the reference's [N, C] is inner = 1, its [N, C, d1, ...] is
 * inner = prod d), labels [outer, inner] of label_bytes = 2 / 4 / 8 (int16 / int32 / int64), class_weight [n_cols] or NULL (ones).
 * Per position p = (n, i) with label y: term = -logp[n, y, i] * w[y] when y != ignore_index and 0 <= y < n_cols, else 0 -- an ignored
 * or out-of-range position is never dereferenced, in logp or in the weights (the reference indexes weight[y] BEFORE it masks:
 * its default ignore_index = -100 raises IndexError below 100 classes and reads class C - 100 above).  reduction 'n': loss[p] =
 * term; 's': loss[0] = sum; 'm': loss[0] = sum / sum_p w[y] [p counts], the denominator derived inside the launch (no host read); a
 * zero denominator gives loss 0 and a zero gradient (nnhipCrossEntropyLossEx's rule; the reference gives NaN).
 * dlogp (may be NULL): the dense gradient [outer, n_cols, inner], zero-filled, plus one value per counted position, already scaled
 * for 'm' / 's'.  pos_grad (may be NULL): that one value per position, [outer * inner] (0 where the position does not count) -- the
 * sparse form nnhipLogSoftmaxNLLBackward consumes.  One block up to 16384 positions; beyond, per-block partial sums in the library
 * workspace, a one-block finish and a gradient pass.  No float atomics: reruns are bit-identical. */
int nnhipNLLLossForwardBackward(const float* logp, const void* labels, int32_t label_bytes, const float* class_weight_or_null,
                                int64_t ignore_index, int64_t outer, int64_t n_cols, int64_t inner, char reduction, float* loss,
                                float* dlogp_or_null, float* pos_grad_or_null, nnhipStream_t stream);
/* NLLLoss(LogSoftmax(X)) for 2-D [n_rows, n_cols] over axis 1 (the reference's own CrossEntropyLoss, losses.py:66-77), backward in
 * one pass: dX[n, c] = g_n ([c == y_n] - exp(Y[n, c])) u, Y the LogSoftmax output, g_n = pos_grad[n] (as written by
 * nnhipNLLLossForwardBackward), u the scalar upstream gradient read from the device (NULL: 1).  Reads Y once and writes dX once:
 * the dense [N, C] gradient of the NLL never exists.  Rows with g_n == 0 (ignored) are written as zeros. */
int nnhipLogSoftmaxNLLBackward(float* dX, const float* Y, const void* labels, int32_t label_bytes, const float* pos_grad,
                               const float* upstream_scalar_or_null, int64_t n_rows, int64_t n_cols, nnhipStream_t stream);
/* L1Loss (neunet/nn/losses.py:129-146): term = |p - t|; dpred (may be NULL) = sign(p - t) * scale, sign(0) = 0 as np.sign
 * (neunet/autograd.py:599).  reduction 'm' (scale 1/n), 's' (1) or 'n' (loss[0..n) = the terms, scale 1).  n > 0. */
int nnhipL1LossForwardBackward(const float* pred, const float* target, float* loss, float* dpred, int64_t n, char reduction,
                               nnhipStream_t stream);
/* KLDivLoss (neunet/nn/losses.py:152-175): term = t (log t - p), or with log_target != 0 exp(t) (t - p) -- the reference's expression
 * literally, so t = 0 gives NaN as np.log does.  dpred (may be NULL) = -t * scale or -exp(t) * scale.  reduction 'm' (scale 1/n),
 * 'b' (batchmean: 1/batch, batch > 0), 's' (1) or 'n' (the terms).  The target receives no gradient.  n > 0. */
int nnhipKLDivLossForwardBackward(const float* pred, const float* target, float* loss, float* dpred, int64_t n, int64_t batch,
                                  int log_target, char reduction, nnhipStream_t stream);

/* ---- vector quantisation (examples/vqvae.ipynb).  ABI 219 --------------------------------------------------------------------
 * nnhipVQNearest replaces VQVAE.quantize: `similarity = matmul(z, codebook.weight.T)`, `distances = sum(z**2, axis=1, keepdims=True)
 * + sum(codebook.weight**2, axis=1) - 2 * similarity`, `min_indices = argmin(distances, axis=1)`, `z_q = codebook(min_indices)`.
 * z [N, D] and codebook [K, D] row-major.  idx[n] = the index of the code nearest to row n in squared Euclidean distance;
 * zq[n, :] = a bit copy of codebook[idx[n], :] (zq may be NULL: indices only).  Ties and NaNs follow np.argmin: equal scores
 * resolve to the lower index; a NaN score beats any number and the first NaN wins, so a NaN anywhere in row n gives idx[n] = 0 and
 * a NaN in code k makes k the answer of every NaN-free row unless an earlier code holds one too.
 * Two tiers, chosen from D alone.  D <= NNHIP_VQ_NARROW_MAX_D: one lane per row, the codebook through LDS, the score in the direct
 * form sum_j (z_j - e_j)^2.  D > NNHIP_VQ_NARROW_MAX_D: exact-fp32 MFMA, the score in the expansion |e|^2 - 2 z.e (|z|^2 is constant
 * in a row).  Neither form is the reference's float32 arithmetic; the guarantee is near-optimality in exact arithmetic,
 * d(n, idx[n]) - min_k d(n, k) <= bound_n with bound_n = 2 g(D + 2) min_k d(n, k) / (1 - g(D + 2)) (narrow) and
 * 2 g(D + 3) (|z_n| + max_k |e_k|)^2 (wide), g(m) = m 2^-24 / (1 - m 2^-24), plus a few float32 underflow quanta
 * (csrc/vector_quantize.hip, tests/vq_ref.py).
 * ONE launch; no workspace, no atomics, no N x K buffer, no host synchronisation (legal inside a stream capture); reruns are
 * bit-identical.  4-byte alignment of every pointer is enough.  Rows are split over blocks and the codebook is NEVER split across
 * blocks: a few rows against a huge codebook is one block walking all of it -- slow by construction.
 * 1 <= N, D, K < 2^31 and z, codebook, idx non-NULL, else NNHIP_EINVAL. */
#define NNHIP_VQ_NARROW_MAX_D 8      /* the last D of the narrow (one lane per row, direct form) tier */
int nnhipVQNearest(const float* z, const float* codebook, int32_t* idx, float* zq, int64_t N, int64_t D, int64_t K,
                   nnhipStream_t stream);
/* VQVAE.loss_function's `vq_loss + beta * commit_loss` = `loss_fn(z_q, z_e.detach()) + beta * loss_fn(z_q.detach(), z_e)` (MSELoss,
 * mean over the n elements): loss[0] = (1 + beta) sum (z_q - z_e)^2 / n ; dz_q = 2 (z_q - z_e) / n ; dz_e = 2 beta (z_e - z_q) / n
 * (either may be NULL).  One launch of ONE block, a fixed-order sum: meant for latent tensors (a block walks the n elements). */
int nnhipVQLossForwardBackward(const float* z_e, const float* z_q, float beta, float* loss, float* dz_e, float* dz_q, int64_t n,
                               nnhipStream_t stream);

/* ---- gradient-bucket helpers for data-parallel training (net-new) ---------------- */
/* x[i] *= alpha */
int nnhipScale(float* x, float alpha, int64_t n, nnhipStream_t stream);
/* out[r,c] = in[r,c] * scale[r * scale_stride], scale_stride 0 (one device scalar) or 1 (a factor per row): a loss node's product
 * with its upstream gradient (cross_entropy.py:111-114 `y_pred.apply_grad(grad_y_pred * grad)`).  ABI 208 */
int nnhipScaleRows(float* out, const float* in, const float* scale, int64_t rows, int64_t cols, int64_t scale_stride,
                   nnhipStream_t stream);
/* out[i] = a[i] + b[i]   (Tensor.apply_grad accumulation, neunet/autograd.py:85-93) */
int nnhipAdd(float* out, const float* a, const float* b, int64_t n, nnhipStream_t stream);
/* out[i] = a[i] * b[i]   (Dropout mask application, neunet/nn/layers/dropout.py:17-37) */
int nnhipMul(float* out, const float* a, const float* b, int64_t n, nnhipStream_t stream);

/* ---- (e) the data-parallel exchange: RCCL behind this ABI (net-new; SURVEY 8b "add AllReduce*", 8e, 7 step 7) ------------
 * The reference has no collective (neunet/autograd.py:8-14: device is "cpu" | "cuda"); these are what a binder that holds
 * plain device pointers (CuPy arrays through neunet/nn/experimental/utils.py:64-92) needs for the ONE exchange of the path:
 * a SUM all-reduce of the flat fp32 gradient bucket (Module.parameters() order, neunet/nn/modules.py:23-39) after
 * backward() and before optimizer.step() -- the optimizer's grad_scale = 1/world (or nnhipFusedOptimizerSetGradDivisor)
 * turns the sum into the mean.  One process per GPU; hipSetDevice(LOCAL_RANK) before nnhipCommInitRank.
 * librccl is bound with dlopen at the first call here (a copy already mapped into the process -- e.g. torch's -- is
 * shared; NNHIP_RCCL_LIB overrides the path): libneunet_hip.so itself loads on a box without RCCL.  Failures return
 * NNHIP_ECOMM with RCCL's text in nnhipGetLastErrorString().  Collectives are enqueued on the caller's stream, in
 * order with the kernels that produced the buffer; they may be captured into a hipGraph like any other launch.  ABI 208 */
#define NNHIP_ECOMM (-4)             /* RCCL missing, or an RCCL call failed */
#define NNHIP_UNIQUE_ID_BYTES 128    /* sizeof(ncclUniqueId) */
typedef struct nnhipComm* nnhipComm_t;
/* Rank 0: fill `id` (NNHIP_UNIQUE_ID_BYTES HOST bytes) -- ncclGetUniqueId; ship it to every rank out of band
 * (a file, a socket, MPI_Bcast, torch's TCPStore). */
int nnhipCommUniqueId(void* id);
/* Every rank, collectively: join the communicator `id` names as `rank` of `world` on the current device. */
int nnhipCommInitRank(nnhipComm_t* comm, const void* id, int rank, int world);
int nnhipCommDestroy(nnhipComm_t comm);                    /* NULL is a no-op */
int nnhipCommRank(nnhipComm_t comm, int* rank, int* world); /* either out pointer may be NULL */
/* Which librccl was bound (path as passed to dlopen; `version` = ncclGetVersion or 0); both out arguments may be NULL. */
int nnhipCommLibrary(char* path, int64_t path_bytes, int* version);
/* buf[i] = sum over ranks of buf[i], in place, n floats (n == 0: no call).  Deterministic for a fixed communicator
 * (same algorithm, same rank order every step), so replicas that start identical stay bit-identical. */
int nnhipAllReduceSumF32(nnhipComm_t comm, float* buf, int64_t n, nnhipStream_t stream);
/* Same with RCCL's pre-scaled average (sum / world). */
int nnhipAllReduceAvgF32(nnhipComm_t comm, float* buf, int64_t n, nnhipStream_t stream);
/* buf on every rank = buf of `root` (identical initial parameters: SURVEY 8e "broadcast from rank 0 or same seed"). */
int nnhipBroadcastF32(nnhipComm_t comm, float* buf, int64_t n, int root, nnhipStream_t stream);

/* ---- nn.LSTM (net-new exports, ABI 211: the reference has no CUDA LSTM; CPU semantics neunet/nn/layers/lstm.py:312-362 forward,
 *      :16-143 backward) ----------------------------------------------------------------------------------------------------
 * One layer, batch-major X [B, T, in].  Gate order f, i, o, c (the reference's parameter order, lstm.py:188-247); the layout is
 * X W (weights [in, H] / [H, H]), not X W^T:
 *   f, i, o = rnl(X_t W_{f,i,o} + h_{t-1} W_h{f,i,o} + b),  g = nl(X_t W_c + h_{t-1} W_hc + b_c),
 *   c_t = f c_{t-1} + i g,  h_t = o nl(c_t).
 * Every recurrence is ONE launch whatever T is (csrc/recurrent.hip); the input projection and the parameter gradients are
 * whole-sequence GEMMs around it.  1 <= H <= 512.  Hp below is H rounded up to a multiple of 16.
 * Saved state (caller-allocated, written by the forward, read by the backward):
 *   gates [B, T, 4Hp]  activated f | i | o | g per row (columns >= H of each gate block are padding),
 *   cell  [B, T+1, H]  c_{t-1} at index t (index 0 = c0),   hprev [B, T, H]  h_{t-1}.
 * h0 / c0 [B, H] may be NULL (zeros).  hT / cT [B, H] (NULL-able) receive the last state and may alias h0 / c0 (cycled states).
 * The backward takes the gradient of the whole sequence dY [B, T, H] and/or of the last state alone dYlast [B, H] (either may be
 * NULL, not both) and writes dX [B, T, in] (NULL-able) and the twelve parameter gradients (each NULL-able; written, not
 * accumulated).  No gradient flows into h0 / c0 (the reference gives none either).  Scratch (packed weights, the pre-activation
 * gate gradients dG [B, T, 4Hp]) comes from the library's grow-only workspace: nothing allocates or synchronises once it has
 * grown, so both entries can be captured into a hipGraph.
 * Refusals, all before anything is launched (no output is touched): a size < 1, hidden > 512, a nonlinearity code outside 0..2, a
 * NULL X / weights / gate weight / Y / saved-state buffer, dY and dYlast both NULL: NNHIP_EINVAL; any pointer (members of the two
 * structs included) that is not 4-byte aligned: NNHIP_EALIGN. */
#define NNHIP_LSTM_TANH 0
#define NNHIP_LSTM_SIGMOID 1
#define NNHIP_LSTM_RELU 2
typedef struct nnhipLSTMWeights {
    const float* wx[4];   /* weight_f, weight_i, weight_o, weight_c      [in, H] */
    const float* wh[4];   /* weight_hf, weight_hi, weight_ho, weight_hc  [H, H]  */
    const float* b[4];    /* bias_f, bias_i, bias_o, bias_c              [H]; NULL = zero */
} nnhipLSTMWeights;
typedef struct nnhipLSTMGrads {
    float* dwx[4];
    float* dwh[4];
    float* db[4];
} nnhipLSTMGrads;
int nnhipLSTMForward(const float* X, const nnhipLSTMWeights* w, const float* h0, const float* c0, float* Y, float* gates,
                     float* cell, float* hprev, float* hT, float* cT, int64_t B, int64_t T, int64_t in_features,
                     int64_t hidden, int nonlinearity, int recurrent_nonlinearity, nnhipStream_t stream);
int nnhipLSTMBackward(const float* X, const nnhipLSTMWeights* w, const float* gates, const float* cell, const float* hprev,
                      const float* dY, const float* dYlast, float* dX, const nnhipLSTMGrads* grads, int64_t B, int64_t T,
                      int64_t in_features, int64_t hidden, int nonlinearity, int recurrent_nonlinearity,
                      nnhipStream_t stream);

/* ---- GPT-2 inference (net-new exports, ABI 212): LayerNorm, GELU, KV-cached decode attention ---------------------------------
 * LayerNorm over the last axis of X [rows, cols] (neunet/nn/layers/layernorm.py:115-147): biased variance, rstd = 1/sqrt(var+eps),
 * Y = (X - mean) rstd [* weight + bias].  weight / bias NULL: elementwise_affine=False.  Saved for the backward: mean and rstd,
 * rows floats each (the reference keeps X_centered, a whole tensor).  The backward writes dX (closed form of layernorm.py:48-93,
 * two row sums) and, where asked (each NULL-able), dW = sum_rows dY xhat and dB = sum_rows dY -- written, not accumulated; the Ex
 * form adds dX_addend (an already accumulated gradient of X, e.g. the residual branch's) to dX in the same pass.  Inside
 * nnhipWeightGradDefer(1) the finishing column sums of dW / dB ride in the RMSNorm queue and are launched by nnhipWeightGradFlush. */
int nnhipLayerNormForward(const float* X, const float* weight, const float* bias, float* Y, float* mean, float* rstd,
                          int64_t rows, int64_t cols, float eps, nnhipStream_t stream);
int nnhipLayerNormBackward(const float* dY, const float* X, const float* weight, const float* mean, const float* rstd,
                           float* dX, float* dW, float* dB, int64_t rows, int64_t cols, nnhipStream_t stream);
int nnhipLayerNormBackwardEx(const float* dY, const float* X, const float* weight, const float* mean, const float* rstd,
                             const float* dX_addend, float* dX, float* dW, float* dB, int64_t rows, int64_t cols,
                             nnhipStream_t stream);
/* GELU, tanh form (neunet/nn/activations.py:386-422): out = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))); the backward is the
 * exact derivative of that form (the reference's uses the same constants rounded to six digits). */
int nnhipGELUForward(float* out, const float* in, int64_t size, nnhipStream_t stream);
int nnhipGELUBackward(float* dIn, const float* dOut, const float* in, int64_t size, nnhipStream_t stream);
/* KV-cached attention for one new token per batch row (csrc/attention_decode.hip).
 *   qkv       [B, 3D] (row stride ld_qkv floats, D = H * head_dim): the new token's fused projection q | k | v
 *   Kcache, Vcache  [B, H, Tmax, head_dim] each, HEAD-MAJOR: a head's keys are one contiguous stream
 *   cache_len DEVICE int32 [B]: tokens already cached in row b (rows may differ).  Read only: the caller advances it.
 * Row b: k and v of the new token are written at index cache_len[b]; the query attends keys 0 .. cache_len[b] inclusive with
 * softmax(scale q.k); O [B, D] receives the result.  Nothing depends on a host-side position, so the call can be captured into a
 * hipGraph and replayed while cache_len advances on the device.  The key range of each (b, h) is split over blocks whose partial
 * (max, sum, o) land in `workspace` (nnhipAttentionDecodeWorkspace bytes; it may be NULL when that returns 0) and are combined in
 * split order: the output is bit-identical from run to run.  A row with cache_len[b] outside 0 .. Tmax-1 writes NOTHING (cache
 * and O untouched) and raises the device error word: nnhipDeviceError() / the next call return NNHIP_EDEVICE.
 * head_dim 32, 64 or 128, anything else: NNHIP_EINVAL.  qkv and the caches 16-byte aligned, ld_qkv % 4 == 0: else NNHIP_EALIGN. */
int64_t nnhipAttentionDecodeWorkspace(int64_t B, int64_t H, int64_t Tmax, int64_t head_dim);   /* bytes, or a negative status */
int nnhipAttentionDecode(const float* qkv, float* Kcache, float* Vcache, const int32_t* cache_len, float* O, float* workspace,
                         int64_t B, int64_t H, int64_t Tmax, int64_t head_dim, int64_t ld_qkv, float scale, nnhipStream_t stream);
/* Prefill: k and v of T tokens out of a fused projection qkv [B, T, 3D] (row stride ld_qkv) into the caches at token index
 * cache_len[b] + i (cache_len NULL: 0 + i).  T > Tmax: NNHIP_EINVAL; a row whose cache_len leaves no room for T tokens is skipped
 * and raises the device error word. */
int nnhipKVCacheFill(const float* qkv, float* Kcache, float* Vcache, const int32_t* cache_len, int64_t B, int64_t H, int64_t T,
                     int64_t Tmax, int64_t head_dim, int64_t ld_qkv, nnhipStream_t stream);

/* ---- device-side top-k sampling (net-new export, ABI 213; csrc/sample.hip) ---------------------------------------------------------
 * Replaces the host-side choice of the next token in the reference's GPT-2 script (examples/gpt2/gpt2_infer.py:331-338: last /
 * max(temperature, 1e-6), np.argpartition, softmax_np, np.random.choice), which needs the whole row of logits on the host.
 *   logits  [rows, n], row stride ld >= n floats (rows need not be 16-byte aligned);  out_ids int32 [rows];
 *   u_out   NULL, or float [rows]: receives the uniform each row used.
 * Row r.  Candidates: the k = min(top_k, n) best elements under nnhipArgmaxF32's total order (a NaN beats any number, a larger
 * value beats a smaller one, ties go to the lower index -- which also decides which of several equal values at the k-th place
 * belong), sorted by that order: x_0 is the argmax.  t = max(temperature, 1e-6); e_j = exp((x_j - x_0) / t) in float32;
 * c_j = e_0 + ... + e_j summed sequentially in sorted order.  s = seed + (seed_dev ? *seed_dev : 0) mod 2^32;
 * u = (hash(s, r) >> 8) * 2^-24 in [0, 1), the counter-based hash of nnhipDropout / the attention dropout with key 0.
 * out_ids[r] = index of the first sorted candidate with c_j > u * c_{k-1}; if rounding leaves none, the last one with e_j > 0.
 * If x_0 is NaN or not finite, out_ids[r] is its index (argmax's answer); -inf logits are legal otherwise and are never drawn.
 * Bit-identical from run to run.  seed_dev (optional DEVICE uint32, e.g. a position counter) is read inside the kernel, so a
 * captured hipGraph draws a fresh token on every replay.  At most two kernel launches and nothing else; partial results go through
 * the library workspace (reserve or warm up before capturing).  top_k outside 1 .. NNHIP_SAMPLE_MAX_K, temperature NaN or
 * negative, ld < n, n >= 2^31, n < 1 or a null out_ids / logits with rows > 0: NNHIP_EINVAL.  rows == 0: returns 0. */
#define NNHIP_SAMPLE_MAX_K 1024
int nnhipSampleTopK(int32_t* out_ids, float* u_out, const float* logits, int64_t rows, int64_t n, int64_t ld, int32_t top_k,
                    float temperature, uint32_t seed, const uint32_t* seed_dev, nnhipStream_t stream);

/* ---- seq2seq inference (net-new exports, ABI 217; csrc/attention_cross_decode.hip) -------------------------------------------------
 * The cross-attention of ONE new decoder row against a read-only encoder memory: what a cached step of the reference's predict()
 * loop (examples/seq2seq.ipynb cell 17, which re-runs the whole decoder per token) needs from DecoderLayer.cross_attn (cell 5) and
 * MultiHeadAttention.forward (cell 2), with the attention map of cell 21's plot.
 *   Q          [B, D], D = H * head_dim, row stride ld_q floats (it may be a column block of a wider buffer)
 *   Kmem, Vmem [B, H, S, head_dim] each, HEAD-MAJOR (the KVCache layout with Tmax = S); only read
 *   key_valid  NULL, or int32 [B, S]: 0 = padding (holes allowed)
 *   O          [B, D] dense;   P  NULL, or [B, H, S]: receives the softmax probabilities (cell 2's `attn` for this query row)
 * s_j = (key_valid && !key_valid[b*S+j]) ? -1e9 : scale * q.k_j and O = softmax(s) V -- the rule of nnhipMaskedSoftmaxForward: a masked
 * key is -1e9, not -inf, so a fully masked row is the plain average of all S values.  One launch, no workspace, no atomics; fixed
 * reduction orders: bit-identical from run to run, and O has the same bits with and without P.  One block per (b, h) walks all S
 * keys -- there is no key split, so a long memory with a small B*H is slow by construction.
 * Checked on the host before any launch.  NNHIP_EINVAL: a NULL Q / Kmem / Vmem / O, head_dim outside {32, 64, 128}, S < 1 with
 * B > 0, ld_q < D or ld_q % 4 != 0.  NNHIP_EALIGN: Q, Kmem, Vmem or O not 16-byte aligned.  B == 0: returns 0, launches nothing. */
int nnhipAttentionDecodeCross(const float* Q, const float* Kmem, const float* Vmem, const int32_t* key_valid, float* O, float* P,
                              int64_t B, int64_t H, int64_t S, int64_t head_dim, int64_t ld_q, float scale, nnhipStream_t stream);
/* Fills such a memory once per source sentence (cell 17 encodes once): token-major projections K, V [B, S, D] with one common row
 * stride ld floats (2D for the two column blocks of a fused K|V projection) -> Kmem, Vmem [B, H, S, head_dim], one launch.  The
 * same status rules (ld in place of ld_q; K, V, Kmem, Vmem in place of the four operands). */
int nnhipKVMemoryFill(const float* K, const float* V, float* Kmem, float* Vmem, int64_t B, int64_t H, int64_t S, int64_t head_dim,
                      int64_t ld, nnhipStream_t stream);

/* ---- nn.GRU, nn.RNN, nn.Bidirectional (net-new exports, ABI 220; csrc/recurrent_gru.hip: the reference has no CUDA recurrences) -------
 * GRU (CPU semantics neunet/nn/layers/gru.py:273-311 forward, :66-110 backward), gate order z, r, h (the reference's parameter order,
 * gru.py:170-215), layout X W as for the LSTM:
 *   z, r = rnl(X_t W_{z,r} + h_{t-1} W_h{z,r} + b),  c = nl(X_t W_h + (r * h_{t-1}) W_hh + b_h),  h_t = z h_{t-1} + (1 - z) c.
 * RNN (rnn.py:151-159 forward, :46-56 backward):  h_t = nl(X_t W + h_{t-1} W_h + b).
 * Derivatives are taken from the activated values (the reference's derivative(unactivated) restated); relu' is 0 at 0.
 * ndir is 1 or 2 and every struct argument is an array of ndir structs.  Direction 1 consumes the input backwards: its step s reads
 * X[:, T-1-s] and writes its output at index s -- what the reference's reverse_layer(X.flip(1)) yields (bidirectional.py:55-56; the
 * reverse output is not flipped back).  Both directions of a call are ONE recurrence launch whatever T is; no flipped copy of X or
 * dX is made, and dX [B, T, in] is the sum of the two directions' contributions, in input order.
 * Every other buffer has a leading direction axis.  Hp = H rounded up to a multiple of 16.  1 <= H <= 512.
 *   Y      [ndir, B, T, H]    h of step s at index s
 *   gates  [ndir, B, T, 3Hp]  GRU only: activated z | r | c of the step that read X[:, t], at index t (columns >= H of a block: padding)
 *   hprev  [ndir, B, T, H]    the h that met X[:, t], at index t
 *   h0     [ndir, B, H] or NULL (zeros);  hT [ndir, B, H] or NULL: the last step's h; hT may alias h0 (cycled states)
 *   dY     [ndir, B, T, H] (step index, as Y) and / or dYlast [ndir, B, H] (the last step's h alone); either may be NULL, not both
 * The backward writes dX (NULL-able) and the parameter gradients (grads NULL-able, each member NULL-able; written, not accumulated).
 * No gradient flows into h0.  A NULL bias is a zero bias.  Scratch (packed weights, dG, r * h_{t-1}, the RNN's pre-activations)
 * comes from the library's grow-only workspace: once it has grown nothing allocates or synchronises, so every entry can be
 * captured into a hipGraph.  No atomics: bit-identical from run to run.
 * Refusals, all before anything is launched: a size < 1, hidden > 512, ndir outside {1, 2}, a nonlinearity code outside 0..2
 * (NNHIP_LSTM_TANH / _SIGMOID / _RELU), a NULL X / weights / weight / Y / saved-state buffer, dY and dYlast both NULL: NNHIP_EINVAL;
 * any pointer (struct members included) that is not 4-byte aligned: NNHIP_EALIGN. */
typedef struct nnhipGRUWeights {
    const float* wx[3];   /* weight_z, weight_r, weight_h     [in, H] */
    const float* wh[3];   /* weight_hz, weight_hr, weight_hh  [H, H]  */
    const float* b[3];    /* bias_z, bias_r, bias_h           [H]; NULL = zero */
} nnhipGRUWeights;
typedef struct nnhipGRUGrads {
    float* dwx[3];
    float* dwh[3];
    float* db[3];
} nnhipGRUGrads;
typedef struct nnhipRNNWeights {
    const float* wx;      /* weight    [in, H] */
    const float* wh;      /* weight_h  [H, H]  */
    const float* b;       /* bias      [H]; NULL = zero */
} nnhipRNNWeights;
typedef struct nnhipRNNGrads {
    float* dwx;
    float* dwh;
    float* db;
} nnhipRNNGrads;
int nnhipGRUForward(const float* X, const nnhipGRUWeights* w, const float* h0, float* Y, float* gates, float* hprev, float* hT,
                    int64_t B, int64_t T, int64_t in_features, int64_t hidden, int nonlinearity, int recurrent_nonlinearity,
                    int ndir, nnhipStream_t stream);
int nnhipGRUBackward(const float* X, const nnhipGRUWeights* w, const float* gates, const float* hprev, const float* dY,
                     const float* dYlast, float* dX, const nnhipGRUGrads* grads, int64_t B, int64_t T, int64_t in_features,
                     int64_t hidden, int nonlinearity, int recurrent_nonlinearity, int ndir, nnhipStream_t stream);
int nnhipRNNForward(const float* X, const nnhipRNNWeights* w, const float* h0, float* Y, float* hprev, float* hT, int64_t B,
                    int64_t T, int64_t in_features, int64_t hidden, int nonlinearity, int ndir, nnhipStream_t stream);
/* Y: the forward's output (the activated states are the only saved values the RNN's backward needs besides hprev). */
int nnhipRNNBackward(const float* X, const nnhipRNNWeights* w, const float* Y, const float* hprev, const float* dY,
                     const float* dYlast, float* dX, const nnhipRNNGrads* grads, int64_t B, int64_t T, int64_t in_features,
                     int64_t hidden, int nonlinearity, int ndir, nnhipStream_t stream);
/* The merge of nn.Bidirectional (bidirectional.py:89-103; backward :16-23), one elementwise launch each way.  D, R [rows, H] are the
 * two directions' outputs (rows = B*T, or B for the last state); out and grad are [rows, 2H] for CONCAT (last axis), else [rows, H].
 * SUM: D + R, gradients (g, g).  MUL: D R, gradients (g R, g D).  AVG: (D + R) / 2, gradients (g / 2, g / 2).  D and R may be NULL
 * in the backward unless the mode is MUL.  NNHIP_EINVAL: a size < 1, an unknown mode, a NULL buffer; NNHIP_EALIGN as above. */
#define NNHIP_MERGE_CONCAT 0
#define NNHIP_MERGE_SUM 1
#define NNHIP_MERGE_MUL 2
#define NNHIP_MERGE_AVG 3
int nnhipBidirectionalMergeForward(const float* D, const float* R, float* out, int64_t rows, int64_t hidden, int mode,
                                   nnhipStream_t stream);
int nnhipBidirectionalMergeBackward(const float* grad, const float* D, const float* R, float* dD, float* dR, int64_t rows,
                                    int64_t hidden, int mode, nnhipStream_t stream);

/* ---- the arithmetic core of the Tensor tape (ABI 223; neunet/autograd.py:96-531, 605-640) ---------------------------------------
 * Shapes travel as `rank` (0..NNHIP_TENSOR_MAX_RANK) host int64 extents and per-operand host int64 strides in ELEMENTS, 0 along an
 * axis the operand is broadcast over.  The entries drop axes of extent 1, merge adjacent axes every operand walks contiguously, and
 * then allow at most 6 axis groups; the description reaches the kernels by value (no device upload: every entry may be captured).
 * Status rules: a rank outside the limit, a negative extent, more than 6 groups, an unknown kind or a NULL required pointer is
 * NNHIP_EINVAL, a pointer that is not 4-byte aligned NNHIP_EALIGN, a failed workspace request NNHIP_ENOMEM.  A zero-size tensor is a
 * no-op.  No float atomics anywhere: reruns are bit-identical.  csrc/tensor_ops.hip describes the tiers.
 *
 * nnhipBroadcastBinaryForward: out[shape] (contiguous) = a (kind) b.  a or b (not both) may be NULL: that operand is `scalar`, by
 *   value.  A one-element device tensor (all strides 0) is read on the device.  maximum / minimum propagate a NaN.
 * nnhipBroadcastBinaryBackward: dA and / or dB (either may be NULL) from dOut[shape] (contiguous), the reference's expressions:
 *   add (g, g)  sub (g, -g)  mul (g b, a g)  div (g / b, -g a / b^2)  power (g b a^(b-1), g a^b log a)
 *   maximum (g (a >= b), g (a <= b))  minimum (g (a <= b), g (a >= b)).
 *   dA is contiguous in a's OWN shape (extent 1 where stride_a is 0): the gradient of a broadcast operand is summed over its
 *   broadcast axes inside the same launch, the full-shape gradient is never written.  One launch per gradient (two when the
 *   reduced extent is split over blocks).  A by-value scalar has no gradient. */
#define NNHIP_TENSOR_MAX_RANK 8
#define NNHIP_BIN_ADD 0
#define NNHIP_BIN_SUB 1
#define NNHIP_BIN_MUL 2
#define NNHIP_BIN_DIV 3
#define NNHIP_BIN_POW 4
#define NNHIP_BIN_MAX 5
#define NNHIP_BIN_MIN 6
int nnhipBroadcastBinaryForward(int kind, float* out, const float* a, const float* b, float scalar, int rank, const int64_t* shape,
                                const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t stream);
int nnhipBroadcastBinaryBackward(int kind, float* dA, float* dB, const float* dOut, const float* a, const float* b, float scalar,
                                 int rank, const int64_t* shape, const int64_t* stride_a, const int64_t* stride_b,
                                 nnhipStream_t stream);
/* nnhipReduceAxesForward: out (contiguous over the axes with reduce[i] == 0, in order) = the reduction of in[shape] (strides
 *   `stride`) over the axes with reduce[i] != 0.  var is the population variance (ddof 0) from sums of (x - mean)^2, never
 *   E[x^2] - E[x]^2; mean_out (var only, may be NULL) receives the means.  max / min propagate a NaN.  At most two launches; the
 *   partials of a split reduction live in the library workspace (nnhipWorkspaceReserve before a capture).
 * nnhipReduceAxesBackward: dX[shape] (contiguous) from grad (contiguous over the kept axes): sum g, mean g / n,
 *   var g 2 (x - saved) / n with saved = the forward's means, max / min g (x == saved) with saved = the forward's output (every tie
 *   receives g).  x and saved are not read for sum / mean.  One launch. */
#define NNHIP_RED_SUM 0
#define NNHIP_RED_MEAN 1
#define NNHIP_RED_VAR 2
#define NNHIP_RED_MAX 3
#define NNHIP_RED_MIN 4
int nnhipReduceAxesForward(int kind, float* out, float* mean_out, const float* in, int rank, const int64_t* shape,
                           const int64_t* stride, const int32_t* reduce, nnhipStream_t stream);
int nnhipReduceAxesBackward(int kind, float* dX, const float* grad, const float* x, const float* saved, int rank,
                            const int64_t* shape, const int32_t* reduce, nnhipStream_t stream);
/* out[shape] (contiguous) = scale * in (strides stride_in, 0 allowed): transpose / swapaxes and their backward.  A tile goes through
 * LDS when `in` is contiguous along the second-to-last group of `out` (the 2-D-transpose pattern). */
int nnhipStridedCopy(float* out, const float* in, float scale, int rank, const int64_t* shape, const int64_t* stride_in,
                     nnhipStream_t stream);
/* Test hook: the tier the most recent launch of the five entries above took (of the LAST launch of a call: for
 * nnhipBroadcastBinaryBackward that is dB's when both gradients are asked for), and through `segments` (may be NULL) the number of
 * segments a reduction split its reduced extent into (1: one launch, no finishing pass).  Not a status code. */
#define NNHIP_TIER_NONE 0
#define NNHIP_TIER_EW_SAME 1
#define NNHIP_TIER_EW_SCALAR 2
#define NNHIP_TIER_EW_VEC2D 3
#define NNHIP_TIER_EW_GENERAL 4
#define NNHIP_TIER_COPY_TILE 5
#define NNHIP_TIER_RED_ROW_WAVE 10
#define NNHIP_TIER_RED_ROW_BLOCK 11
#define NNHIP_TIER_RED_COL 12
#define NNHIP_TIER_RED_GENERAL 13
#define NNHIP_TIER_IDX_VEC4 20          /* compare / logical / where forward: four results per lane */
#define NNHIP_TIER_IDX_GENERAL 21       /* the strided tier of csrc/tensor_index.hip (also: typed copy, strided / masked assign) */
#define NNHIP_TIER_SLICE_BWD_VEC 22     /* nnhipSliceBackward: float4 stores */
#define NNHIP_TIER_SLICE_BWD_SCALAR 23
#define NNHIP_TIER_IDX_ROW_VEC 24       /* gather / index assign: a wave per row, 16 bytes per lane */
#define NNHIP_TIER_IDX_ROW 25           /* a wave per row, one element per lane */
#define NNHIP_TIER_IDX_ELEMENT 26       /* inner == 1: a lane per output */
int nnhipTensorOpsLastTier(int64_t* segments);

/* ---- the rest of the Tensor tape (ABI 224; neunet/autograd.py:642-808, 895-923): comparisons, logical ops, where, indexing ----------
 * csrc/tensor_index.hip.  The rules of the section above hold: shapes and strides by value (rank <= 8, <= 6 groups after collapsing),
 * status codes for bad arguments, a zero-size problem returns 0 without a launch, no float atomics, reruns bit-identical, every entry
 * may be captured.  Strides are SIGNED element strides; an element offset is an argument (`offset`), added to the base inside the
 * entry.  Element types travel as NNHIP_DT_*; bool storage is one byte holding 0 or 1.  Pointers are aligned to their element size
 * (NNHIP_EALIGN).  nnhipTensorOpsLastTier reports the tier of the last launch of these entries too.
 *
 * nnhipCompare: out (bytes, contiguous over shape) = a (kind) b.  a and b share `dtype`; a or b (not both) may be NULL: that operand is
 *   the by-value scalar -- `scalar_i64` when scalar_is_int, else `scalar`.  NumPy 2's rules: against float32 the scalar is rounded to
 *   float32 first; an integer (or bool) tensor against an integer scalar compares in int64, against a floating scalar in double.  A NaN
 *   makes every kind false except NE; -0.0 == 0.0.
 * nnhipLogical: truth is value != 0 (a NaN is true); the operands may differ in dtype; b is ignored for NOT. */
#define NNHIP_DT_F32 0
#define NNHIP_DT_I32 1
#define NNHIP_DT_I64 2
#define NNHIP_DT_U8 3                   /* bool and uint8 */
#define NNHIP_CMP_EQ 0
#define NNHIP_CMP_NE 1
#define NNHIP_CMP_GT 2
#define NNHIP_CMP_GE 3
#define NNHIP_CMP_LT 4
#define NNHIP_CMP_LE 5
#define NNHIP_LOGICAL_AND 0
#define NNHIP_LOGICAL_OR 1
#define NNHIP_LOGICAL_NOT 2
int nnhipCompare(int kind, uint8_t* out, const void* a, const void* b, double scalar, int64_t scalar_i64, int scalar_is_int, int dtype,
                 int rank, const int64_t* shape, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t stream);
int nnhipLogical(int kind, uint8_t* out, const void* a, const void* b, int dtype_a, int dtype_b, int rank, const int64_t* shape,
                 const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t stream);
/* nnhipWhereForward: out (float32, contiguous over shape) = cond ? a : b.  cond (NNHIP_DT_U8, _I32 or _F32; truth is != 0) broadcasts
 *   against both operands through stride_c; a and / or b may be NULL: scalar_a / scalar_b.
 * nnhipWhereBackward: dA = cond ? g : 0, dB = cond ? 0 : g -- a select, so an inf or a NaN of g at a position the operand did not supply
 *   gives exactly 0.  Each gradient is contiguous in the operand's OWN shape (extent 1 where its stride is 0; a one-element operand gets
 *   a one-element gradient): the sum over its broadcast axes happens inside the launch that forms it (the reduction kernels with the
 *   select as their load functor, as nnhipBroadcastBinaryBackward).  Either output may be NULL (its strides are then not read). */
int nnhipWhereForward(float* out, const void* cond, int cond_dtype, const float* a, const float* b, float scalar_a, float scalar_b, int rank,
                      const int64_t* shape, const int64_t* stride_c, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t stream);
int nnhipWhereBackward(float* dA, float* dB, const float* grad, const void* cond, int cond_dtype, int rank, const int64_t* shape,
                       const int64_t* stride_c, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t stream);
/* nnhipSliceForward: out[shape] (contiguous) = in[offset + sum_i c_i stride_in[i]]: the forward of __getitem__ with a basic key and of
 *   flip, and flip's backward.  Strides may be negative or 0; the caller guarantees that every address lies inside `in`.  4-byte elements
 *   take the elementwise copy of the section above (never its LDS tile tier), 1- and 8-byte elements a typed general kernel.
 *   (nnhipStridedCopy keeps its contract -- non-negative use by transpose / swapaxes, no offset -- and its tiers unchanged.)
 * nnhipSliceBackward: dX[x_shape] (contiguous float32) from grad (contiguous over count): ONE launch that writes every element of dX
 *   exactly once -- grad[j] where the element's coordinate is start + j * step with 0 <= j < count on every axis, 0 elsewhere.
 *   step may be negative (never 0); an axis taken by an integer has count 1.  A lattice that leaves the tensor is NNHIP_EINVAL.
 * nnhipStridedAssign: out[offset + sum_i c_i stride_out[i]] = in[sum_i c_i stride_in[i]] over shape (in == NULL: the scalar, converted
 *   to dtype; stride_in may be 0 on broadcast axes; stride_out is never 0 on an axis of extent > 1).  One launch. */
int nnhipSliceForward(void* out, const void* in, int64_t offset, int dtype, int rank, const int64_t* shape, const int64_t* stride_in,
                      nnhipStream_t stream);
int nnhipSliceBackward(float* dX, const float* grad, int rank, const int64_t* x_shape, const int64_t* start, const int64_t* step,
                       const int64_t* count, nnhipStream_t stream);
int nnhipStridedAssign(void* out, int64_t offset, const int64_t* stride_out, const void* in, const int64_t* stride_in, double scalar,
                       int64_t scalar_i64, int scalar_is_int, int dtype, int rank, const int64_t* shape, nnhipStream_t stream);
/* Integer-array indexing on adjacent axes: x as [outer, D1..Dk, inner], k <= NNHIP_INDEX_MAX_ARRAYS index arrays of M elements each
 * (idx: a HOST array of k device pointers, all NNHIP_DT_I32 or all NNHIP_DT_I64; dims: D1..Dk), M < 2^31.  Negative indices wrap inside
 * the kernels.  An index outside its axis is NOT an error here (a device index tensor cannot be checked without a host read): the gather
 * reads 0 for it and the assign skips it -- nnhipEmbeddingForward's rule.  The host checks the indices it can see.
 * nnhipIndexGather: out [outer, M, inner] (contiguous) = x[o, idx_1[m], .., idx_k[m], :].  One launch.
 * nnhipIndexAssign: dst [outer, D1..Dk, inner] <- src [outer, M, inner] (src == NULL: the scalar), last occurrence in C order wins (the
 *   reference ASSIGNS, also in its backward: `_grad[index] = grad`).  zero_fill != 0 (the gather's backward): every element of dst is
 *   written once, 0 where no index points; zero_fill == 0 (__setitem__): untouched elements are left alone.  Three launches: the `last`
 *   table over D1*..*Dk in the library workspace (nnhipWorkspaceReserve before a capture) is filled with -1 on every call, an integer
 *   atomicMax of the positions, one pass over dst.  The table takes 4 * D1 * .. * Dk bytes of the grow-only workspace -- the WHOLE indexed
 *   extent, not the M positions: for x[arange(N), y] on [N, C] that is 4 N C bytes (983 MB at [16384, 15000]), as much as x itself.  A
 *   call that needs more than the workspace holds grows it (a device synchronisation and an allocation: not legal inside a capture);
 *   under nnhipWorkspaceLock it returns NNHIP_ENOMEM instead.  Reserve at least that many bytes with nnhipWorkspaceReserve before
 *   capturing a call.
 * nnhipMaskedAssign: dst [rows, inner]; dst[r, :] = value [inner] (NULL: the scalar) where mask[r] != 0.  One launch, no compaction. */
#define NNHIP_INDEX_MAX_ARRAYS 4
int nnhipIndexGather(void* out, const void* x, int dtype, const void* const* idx, int idx_dtype, int k, const int64_t* dims, int64_t outer,
                     int64_t M, int64_t inner, nnhipStream_t stream);
int nnhipIndexAssign(void* dst, const void* src, double scalar, int64_t scalar_i64, int scalar_is_int, int dtype, int zero_fill,
                     const void* const* idx, int idx_dtype, int k, const int64_t* dims, int64_t outer, int64_t M, int64_t inner,
                     nnhipStream_t stream);
int nnhipMaskedAssign(void* dst, const uint8_t* mask, const void* value, double scalar, int64_t scalar_i64, int scalar_is_int, int dtype,
                      int64_t rows, int64_t inner, nnhipStream_t stream);
/* np.argmin on nnhipArgmaxF32's kernels with the mirrored order: the FIRST minimum wins, a NaN wins.  Arguments and status as
 * nnhipArgmaxF32. */
int nnhipArgminF32(int32_t* out, const float* x, int64_t outer, int64_t n, int64_t inner, nnhipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUNET_HIP_H */
